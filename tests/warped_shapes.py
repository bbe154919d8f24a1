"""Scenes and patch sets for the odd-image-size, border and view-count tests of
the warped family (test_warped_shapes_host.py, test_warped_shapes_gpu.py).  No
GPU: everything here comes from the restatements under tests/.

The sphere scene of the other warped tests (rad 0.02) sits in the image centre
and wr.sphere_patches keeps 8 px away from the border, so no patch of any
earlier set lies in a border cell or has a window on a border.  Here the
sphere (rad 0.05) fills every view of every size, the patches' pixels are drawn
over the whole image, and aimed sets put windows on each border and centres
into each border cell, each corner cell and the pixel strips past the last
whole cell.  The view counts run on random-texture rings of 23 x 29 pixels.

Every builder is cached per process: a set and the restatement's results on it
are computed once, shared by the tests and not to be modified.
"""
import functools
import importlib

import numpy as np

import expand_reference as er
import filter_reference as fr
import warped_reference as wr
from conftest import PKG_NAME
from test_expand_gpu import random_masks

RAD = 0.05
V_SPHERE = 24
SIZES = ((45, 61), (39, 45), (26, 31), (89, 125))          # (H, W)
CHAIN_SIZE = (89, 125)
RING_H, RING_W = 23, 29
VIEW_COUNTS = (1, 2, 63, 64, 65, 128, 129, 192, 193, 256)
WIDS = (1, 2, 3, 4, 5)
CELLS = (1, 2, 3, 4)
MIN_NCC, RING_MIN_NCC = 0.7, -0.05      # random textures scatter around 0: a threshold near 0 sets bits in every word
N_UNIFORM = 200                          # patches with the pixel uniform over the image, per scoring set
SHIFTS = (0.0, 0.0, 0.008, -0.008)       # half of them 8 mm off the surface: scored pairs that do not pass
WINDOW_SPOTS = ("right", "right2", "bottom", "left", "top", "corner00", "cornerN0", "corner0N", "cornerNN",
                "out_right", "out_left", "out_bottom", "out_top")


class Scene:
    """A scene as the restatements take it: the projection rotations are
    rodrigues_roundtrip(R), which MvsContext.rproj() returns bit for bit."""

    def __init__(self, rgb, K, R, t):
        pkg = importlib.import_module(PKG_NAME)
        self.rgb, self.K, self.R, self.t_raw = rgb, K, R, t
        self.t = np.asarray(t, np.float64).reshape(-1, 3)
        self.Rp = np.stack([pkg.rodrigues_roundtrip(r) for r in R])
        self.gray = wr.gray_stack(rgb)
        self.V, self.H, self.W = rgb.shape[:3]
        self.words = (self.V + 63) // 64
        self.O = np.array([er.centre_of([float(x) for x in self.Rp[v].reshape(9)], [float(x) for x in self.t[v]])
                           for v in range(self.V)])

    def cam(self):
        return self.K, self.Rp, self.t, self.W, self.H

    def ray(self, v, x, y):
        return self.Rp[v].T @ np.array([(x - self.K[v][0, 2]) / self.K[v][0, 0],
                                        (y - self.K[v][1, 2]) / self.K[v][1, 1], 1.0])

    def at_pixel(self, v, x, y, depth_scale=1.0):
        """A point on the ray of pixel (x, y) of view v, at depth_scale times the depth of the origin."""
        return self.O[v] + self.ray(v, x, y) * (float(self.t[v][2]) * depth_scale)

    def on_sphere(self, v, x, y, rad=RAD):
        """The first hit of the ray of pixel (x, y) of view v with |X| = rad -> (c, outward normal)."""
        d = self.ray(v, x, y)
        d /= np.linalg.norm(d)
        b = d @ self.O[v]
        disc = b * b - (self.O[v] @ self.O[v] - rad * rad)
        assert disc > 0, "the sphere fills every view"
        X = self.O[v] + (-b - np.sqrt(disc)) * d
        return X, X / np.linalg.norm(X)


@functools.lru_cache(maxsize=None)
def sphere(H, W):
    syn = importlib.import_module(PKG_NAME + ".synthetic")
    return Scene(*syn.sphere_scene(V=V_SPHERE, H=H, W=W, rad=RAD, n_seeds=0)[:4])


@functools.lru_cache(maxsize=None)
def ring(V):
    syn = importlib.import_module(PKG_NAME + ".synthetic")
    return Scene(*syn.ring_scene(V=V, H=RING_H, W=RING_W))


def toward_camera(sc, c, ref):
    n = sc.O[ref] - c
    return n / np.linalg.norm(n, axis=1, keepdims=True)


# ---------------------------------------------------------------------------
# patches that reach the border
# ---------------------------------------------------------------------------
def border_patches(sc, n, seed, shifts=(0.0,)):
    """wr.sphere_patches with the pixel drawn over the whole image."""
    c, nrm, ref, _ = wr.sphere_patches(sc.K, sc.R, sc.t, n, RAD, np.random.default_rng([seed, sc.H, sc.W]), shifts,
                                       H=sc.H, W=sc.W, margin=0)
    return c, nrm, ref


def patches_at(sc, ref, x, y):
    """Sphere patches with true normals at pixels (x, y) of the views ref."""
    hits = [sc.on_sphere(int(v), float(a), float(b)) for v, a, b in zip(ref, x, y)]
    return (np.array([h[0] for h in hits]).reshape(-1, 3), np.array([h[1] for h in hits]).reshape(-1, 3),
            np.asarray(ref, np.int32))


def aimed_windows(sc, wid, seed, per=4):
    """per patches for each of WINDOW_SPOTS: the reference window's last column
    at W - 1 and at W - 2, its last row at H - 1, its first column / row at 0,
    the four corners, and one pixel further out each way (an invalid window).
    -> c, nrm, ref, spot (index into WINDOW_SPOTS)."""
    rng = np.random.default_rng([seed, wid, sc.H, sc.W])
    lo, xh, yh = wid, sc.W - 1 - wid, sc.H - 1 - wid
    x0, y0, spot = [], [], []
    for _ in range(per):
        ax, ay = (int(v) for v in rng.integers(lo, xh + 1, 13)), (int(v) for v in rng.integers(lo, yh + 1, 13))
        ax, ay = list(ax), list(ay)
        spots = [(xh, ay[0]), (xh - 1, ay[1]), (ax[2], yh), (lo, ay[3]), (ax[4], lo), (lo, lo), (xh, lo), (lo, yh),
                 (xh, yh), (xh + 1, ay[9]), (lo - 1, ay[10]), (ax[11], yh + 1), (ax[12], lo - 1)]
        x0 += [s[0] for s in spots]
        y0 += [s[1] for s in spots]
        spot += list(range(13))
    m = len(spot)
    ref = rng.integers(0, sc.V, m).astype(np.int32)
    c, nrm, ref = patches_at(sc, ref, np.array(x0) + rng.uniform(0.1, 0.9, m), np.array(y0) + rng.uniform(0.1, 0.9, m))
    return c, nrm, ref, np.array(spot)


@functools.lru_cache(maxsize=None)
def score_set(H, W, wid):
    """The scoring set of one size and window: N_UNIFORM border-reaching patches, then the aimed windows.
    -> dict c, nrm, ref, spot (-1 for the uniform part)."""
    sc = sphere(H, W)
    c, nrm, ref = border_patches(sc, N_UNIFORM, 11, SHIFTS)
    ac, an, ar, spot = aimed_windows(sc, wid, 12)
    return {"c": np.concatenate([c, ac]), "nrm": np.concatenate([nrm, an]), "ref": np.concatenate([ref, ar]),
            "spot": np.concatenate([np.full(len(ref), -1), spot])}


@functools.lru_cache(maxsize=None)
def score_case(H, W, wid, min_cos):
    """score_set and the restatement's results on it."""
    sc, s = sphere(H, W), score_set(H, W, wid)
    return dict(s, o=wr.warped_batch(sc.gray, sc.K, sc.Rp, sc.t, s["c"], s["nrm"], s["ref"], wid, min_cos))


@functools.lru_cache(maxsize=None)
def refine_set(H, W, wid, n_uniform=24):
    """The refinement set: the first n_uniform patches of score_set and its
    aimed windows on a border (not the ones aimed one pixel out).  Their depth
    hypotheses move the samples of the other views across the near border."""
    s = score_set(H, W, wid)
    rows = np.concatenate([np.arange(n_uniform), np.flatnonzero((s["spot"] >= 0) & (s["spot"] < 9))])
    return {k: s[k][rows] for k in ("c", "nrm", "ref", "spot")}


@functools.lru_cache(maxsize=None)
def ring_score_case(V, wid=2, min_cos=0.3):
    """Patches near the origin of the V-view ring, the normal towards the
    reference camera: 128 of them, 64 at V >= 128."""
    sc = ring(V)
    rng = np.random.default_rng([4, V])
    n = 64 if V >= 128 else 128
    c = rng.uniform(-0.005, 0.005, (n, 3)) / np.sqrt(3)
    ref = rng.integers(0, V, n).astype(np.int32)
    nrm = toward_camera(sc, c, ref)
    return {"c": c, "nrm": nrm, "ref": ref, "wid": wid, "min_cos": min_cos,
            "o": wr.warped_batch(sc.gray, sc.K, sc.Rp, sc.t, c, nrm, ref, wid, min_cos)}


def score_coverage(sc, o, ref, wid, min_ncc, border_band, cos_band):
    """What a scored set reaches, and what test_warped_gpu.check_against_reference
    would leave out of its comparison, from the restatement alone."""
    n, V = len(ref), sc.V
    valid = np.asarray(o["valid"], bool)
    x0, y0 = np.floor(o["xy"][:, 0]), np.floor(o["xy"][:, 1])
    is_ref = np.arange(V)[None, :] == np.asarray(ref)[:, None]
    band = np.abs(o["cosm"]) < cos_band
    cand_band = band[np.arange(n), ref]
    tested = valid[:, None] & ~is_ref & (o["cosm"] > 0)
    left_out = tested & (band | cand_band[:, None] | (np.abs(o["border"]) < border_band))
    both = tested & ~left_out & ~np.isnan(o["ncc"])
    tol = 1e-8 / np.minimum(1.0, np.where(o["sigma_b"] > 0, o["sigma_b"], 1.0))
    thr_band = both & (np.abs(o["ncc"] - min_ncc) <= tol)
    with np.errstate(invalid="ignore"):
        passing = tested & (o["ncc"] > min_ncc)
    return {"valid": int(valid.sum()), "left": int((valid & (x0 - wid == 0)).sum()),
            "right": int((valid & (x0 + wid == sc.W - 1)).sum()), "right2": int((valid & (x0 + wid == sc.W - 2)).sum()),
            "top": int((valid & (y0 - wid == 0)).sum()), "bottom": int((valid & (y0 + wid == sc.H - 1)).sum()),
            "tested": int(tested.sum()), "clamp": int((tested & (o["border"] > border_band) & (o["border"] <= 1.0)).sum()),
            "border_fail": int((tested & (o["border"] < 0)).sum()), "passing": int(passing.sum()),
            "non_passing": int((tested & ~passing).sum()), "scored_non_passing": int((both & ~passing).sum()),
            "left_out": int(left_out.sum()) + int(thr_band.sum()),
            "words_set": [bool(passing[:, 64 * g:64 * g + 64].any()) for g in range(sc.words)]}


# ---------------------------------------------------------------------------
# cells
# ---------------------------------------------------------------------------
def cell_boxes(H, W, cell):
    """Pixel boxes (x_lo, x_hi, y_lo, y_hi) of the border cell columns and rows,
    the corner cells and the strips past the last whole cell (where there are any)."""
    nci, ncj = er.grid_shape(W, H, cell)
    X = {"0": (0, cell), "N": ((nci - 1) * cell, nci * cell), "any": (0, nci * cell), "strip": (nci * cell, W)}
    Y = {"0": (0, cell), "N": ((ncj - 1) * cell, ncj * cell), "any": (0, ncj * cell), "strip": (ncj * cell, H)}
    boxes = {"col0": X["0"] + Y["any"], "colN": X["N"] + Y["any"], "row0": X["any"] + Y["0"], "rowN": X["any"] + Y["N"],
             "corner00": X["0"] + Y["0"], "cornerN0": X["N"] + Y["0"], "corner0N": X["0"] + Y["N"],
             "cornerNN": X["N"] + Y["N"]}
    if nci * cell < W:
        boxes["strip_x"] = X["strip"] + Y["any"]
    if ncj * cell < H:
        boxes["strip_y"] = X["any"] + Y["strip"]
    if nci * cell < W and ncj * cell < H:
        boxes["strip_xy"] = X["strip"] + Y["strip"]
    return boxes


@functools.lru_cache(maxsize=None)
def cell_set(H, W, cell, n_uniform=40, per=4):
    """n_uniform border-reaching patches, then per patches aimed at each box of
    cell_boxes in their reference view, with random masks; the strip patches'
    masks are empty, so that their reference view alone places them.
    -> dict c, nrm, ref, mask, avg, box (names; 'uniform' for the first part), strip (bool)."""
    sc = sphere(H, W)
    rng = np.random.default_rng([21, H, W, cell])
    c, nrm, ref = border_patches(sc, n_uniform, 22 + cell)
    box = ["uniform"] * len(ref)
    xs, ys = [], []
    for name, (xl, xh, yl, yh) in cell_boxes(H, W, cell).items():
        xs += list(rng.uniform(xl + 0.05, xh - 0.05, per))
        ys += list(rng.uniform(yl + 0.05, yh - 0.05, per))
        box += [name] * per
    ac, an, ar = patches_at(sc, rng.integers(0, sc.V, len(xs)), xs, ys)
    c, nrm, ref = np.concatenate([c, ac]), np.concatenate([nrm, an]), np.concatenate([ref, ar]).astype(np.int32)
    box = np.array(box)
    strip = np.char.startswith(box, "strip")
    mask = random_masks(rng, len(ref), sc.V, 0.4)
    mask[strip] = 0
    return {"c": c, "nrm": nrm, "ref": ref, "mask": mask, "avg": rng.uniform(0.5, 1.0, len(ref)), "box": box,
            "strip": strip}


def own_cells(sc, s, cell):
    """The cell of every patch in its reference view (None in a strip)."""
    return [er.cell_of(sc.K, sc.Rp, sc.t, int(r), c, sc.W, sc.H, cell) for c, r in zip(s["c"], s["ref"])]


def border_cell_counts(sc, s, cell):
    """Placements (patch, view of its mask or ref) per border cell column / row and corner cell."""
    nci, ncj = er.grid_shape(sc.W, sc.H, cell)
    out = {k: 0 for k in ("col0", "colN", "row0", "rowN", "corner00", "cornerN0", "corner0N", "cornerNN",
                          "skipped_neighbours", "short_neighbourhoods")}
    for row in fr.placements(*sc.cam(), s["c"], s["ref"], s["mask"], cell):
        for _, (i, j), _ in row or ():
            out["col0"] += i == 0
            out["colN"] += i == nci - 1
            out["row0"] += j == 0
            out["rowN"] += j == ncj - 1
            out["corner00"] += (i, j) == (0, 0)
            out["cornerN0"] += (i, j) == (nci - 1, 0)
            out["corner0N"] += (i, j) == (0, ncj - 1)
            out["cornerNN"] += (i, j) == (nci - 1, ncj - 1)
            out["skipped_neighbours"] += sum(not (0 <= i + di < nci and 0 <= j + dj < ncj) for di, dj in er.NEIGHBOURS)
            out["short_neighbourhoods"] += i in (0, nci - 1) or j in (0, ncj - 1)
    return {k: int(v) for k, v in out.items()}


def dense_front(rng, shape, n):
    """A front grid that was not built from the set: -1 in 30 % of the cells, any row elsewhere, so that
    every neighbour walk meets patches and a walk past a grid row or column would meet one too."""
    return np.where(rng.random(shape) < 0.3, -1, rng.integers(0, n, shape)).astype(np.int32)


def cell_dense_front(sc, s, cell):
    """The dense grid the support and conflict tests of one cell set share."""
    nci, ncj = er.grid_shape(sc.W, sc.H, cell)
    return dense_front(np.random.default_rng([7, cell, sc.W]), (sc.V, ncj, nci), len(s["ref"]))


def seed_style_jobs(sc, s, cell):
    """Every patch as a winner of its own cell: jobs (-1, ref, cell), (-1, -1) in a strip."""
    return er.seed_jobs(sc.K, sc.Rp, sc.t, sc.W, sc.H, s["c"], s["ref"], cell)[0]


# ---------------------------------------------------------------------------
# view counts
# ---------------------------------------------------------------------------
def plant_pad_bits(mask, V):
    """Bits >= V of the last word set in every third row (they name no view)."""
    if V & 63:
        pad = np.uint64((1 << 64) - (1 << (V & 63)))
        mask[::3, -1] |= pad
    return mask


@functools.lru_cache(maxsize=None)
def ring_set(V, n=96, spread=0.02, p=0.5):
    """n patches in a box of +-spread / sqrt(3) around the origin of the V-view
    ring (a few pixels around the image centre: many patches per cell), random
    masks with pad bits planted, avg in [0.5, 1)."""
    sc = ring(V)
    rng = np.random.default_rng([6, V, n])
    c = rng.uniform(-spread, spread, (n, 3)) / np.sqrt(3)
    ref = rng.integers(0, V, n).astype(np.int32)
    nrm = toward_camera(sc, c, ref)
    mask = plant_pad_bits(random_masks(rng, n, V, p), V)
    return {"c": c, "nrm": nrm, "ref": ref, "mask": mask, "avg": rng.uniform(0.5, 1.0, n)}


def planted_front(sc, s, cell, every=5):
    """The set's own front grid with, for every `every`-th patch p, the cells of
    all its placements handed to one patch q far from p: q is in front of p in
    views of every group, so the distinct-set walk of the conflict kernel has
    duplicates to remove across groups.  -> front (V, ncj, nci) int32."""
    front = fr.front_grid(*sc.cam(), s["c"], s["ref"], s["mask"], cell)[0].copy()
    n = len(s["ref"])
    rows = fr.placements(*sc.cam(), s["c"], s["ref"], s["mask"], cell)
    for p in range(0, n, every):
        q = int(np.argmax(((s["c"] - s["c"][p]) ** 2).sum(1)))
        for v, (i, j), _ in rows[p] or ():
            front[v, j, i] = q
    return front


def conflict_groups(sc, s, cell, adj_px, front):
    """Per patch {f: set of the groups (view >> 6) in which f hides p}: the
    namings k_wfilt_conflict has to reduce to a set."""
    n = len(s["ref"])
    cl = [[float(x) for x in row] for row in s["c"]]
    nl = [[float(x) for x in row] for row in s["nrm"]]
    out = []
    for p, row in enumerate(fr.placements(*sc.cam(), s["c"], s["ref"], s["mask"], cell)):
        d = {}
        for v, (i, j), z in row or ():
            f = int(front[v, j, i])
            if f < 0 or f >= n or f == p:
                continue
            if not fr.adjacent(cl[p], nl[p], cl[f], nl[f], float(adj_px), z, float(sc.K[v][0, 0]), float(sc.K[v][1, 1])):
                d.setdefault(f, set()).add(v >> 6)
        out.append(d)
    return out


# ---------------------------------------------------------------------------
# colour at the edge
# ---------------------------------------------------------------------------
def _exact(sc, v, want_x=None, want_y=None, tries=400):
    """A centre built by Scene.at_pixel whose projection into view v (the
    restatement's) has x == want_x or y == want_y exactly: pixels and depths are
    tried until the round trip returns the value."""
    rng = np.random.default_rng([31, v, int(want_x or 0), int(want_y or 0)])
    for _ in range(tries):
        x = want_x if want_x is not None else rng.uniform(1, sc.W - 2)
        y = want_y if want_y is not None else rng.uniform(1, sc.H - 2)
        c = sc.at_pixel(v, x, y, rng.uniform(0.9, 1.1))
        px, py, depth = wr.project_ref(sc.K[v], sc.Rp[v], sc.t[v], c)
        if depth > 0 and (want_x is None or px == want_x) and (want_y is None or py == want_y):
            return c
    raise AssertionError("no centre projects onto the edge exactly")


@functools.lru_cache(maxsize=None)
def color_edge_rows(kind, key):
    """Patch-colour rows at the right and bottom edge, each seen by its
    reference view alone (empty mask): per view of 0, 5, V - 1
      0  x == W - 1 exactly (counted; the next column is clamped)
      1  y == H - 1 exactly (counted)
      2  x in (W - 2, W - 1) (counted)      3  x in (W - 1, W) (not counted)
      4  y in (H - 1, H) (not counted)
    -> dict c, ref, mask, kind (0..4)."""
    sc = sphere(*key) if kind == "sphere" else ring(key)
    rng = np.random.default_rng(41)
    c, ref, kinds = [], [], []
    for v in sorted({0, min(5, sc.V - 1), sc.V - 1}):
        rows = [_exact(sc, v, want_x=float(sc.W - 1)), _exact(sc, v, want_y=float(sc.H - 1)),
                sc.at_pixel(v, sc.W - 1 - rng.uniform(0.1, 0.9), rng.uniform(1, sc.H - 2)),
                sc.at_pixel(v, sc.W - 1 + rng.uniform(0.1, 0.9), rng.uniform(1, sc.H - 2)),
                sc.at_pixel(v, rng.uniform(1, sc.W - 2), sc.H - 1 + rng.uniform(0.1, 0.9))]
        c += rows
        ref += [v] * 5
        kinds += [0, 1, 2, 3, 4]
    return {"c": np.array(c), "ref": np.array(ref, np.int32), "mask": np.zeros((len(ref), sc.words), np.uint64),
            "kind": np.array(kinds)}


# ---------------------------------------------------------------------------
# chains
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def chain_seeds(n=24, lo=3.0, hi=7.0):
    """Seeds of the chains on the CHAIN_SIZE sphere: border-reaching patches whose
    reference pixel lies lo to hi px from a border -- a wid 3 window just fits
    (the first n of a larger draw)."""
    sc = sphere(*CHAIN_SIZE)
    c, nrm, ref = border_patches(sc, 1500, 51)
    near = []
    for k in range(len(ref)):
        x, y, _ = wr.project_ref(sc.K[ref[k]], sc.Rp[ref[k]], sc.t[ref[k]], c[k])
        if lo <= min(int(x), sc.W - 1 - int(x), int(y), sc.H - 1 - int(y)) < hi:
            near.append(k)
    near = near[:n]
    assert len(near) == n
    return c[near], nrm[near], ref[near]


CHAIN_KW = dict(min_ncc=0.7, min_cos=0.3, vlb=2)
# (cell, wid) of the chains.  A patch with a valid window lies wid px inside its
# reference view and a view of its mask holds the whole warped window, so at
# wid 3 a cell-2 grid's border cells (2 px, then a 1 px strip) cannot be
# reached; the cell-3 grid's last column and row (3 px, then a 2 px strip) can.
# The wid 1 chain is there to reach the border cells of the cell-2 grid.
CHAINS = ((2, 3), (3, 3), (2, 1))


@functools.lru_cache(maxsize=None)
def cpu_chain(cell, wid=3, rounds=3):
    """The restatement's chain from chain_seeds (no refinement, score_batch_fast)."""
    sc = sphere(*CHAIN_SIZE)
    return er.expand_chain(sc.gray, sc.K, sc.Rp, sc.t, *chain_seeds(), rounds, cell=cell, wid=wid,
                           scorer=er.score_batch_fast, **CHAIN_KW)


@functools.lru_cache(maxsize=None)
def chain_mixed_set(cell, wid=3, shift=0.006):
    """filter_reference.mixed_set's recipe on cpu_chain(cell): the chain's rows,
    then every other one of them moved alternately +shift and -shift along the
    radius and re-scored, those with count >= 2 (cell (-1, -1), kind 1 / 2);
    src: the chain rows the outliers were made from."""
    sc = sphere(*CHAIN_SIZE)
    ch = cpu_chain(cell, wid)
    P = len(ch["ref"])
    pick = np.arange(0, P, 2)
    sign = np.where(np.arange(len(pick)) % 2 == 0, 1.0, -1.0)
    radial = ch["c"][pick] / np.linalg.norm(ch["c"][pick], axis=1, keepdims=True)
    oc = ch["c"][pick] + (sign * shift)[:, None] * radial
    on, orf = ch["nrm"][pick], ch["ref"][pick]
    m, k, a, _ = er.score_batch_fast(sc.gray, sc.K, sc.Rp, sc.t, oc, on, orf, wid, 0.7, 0.3)
    ok = k >= 2
    return {"c": np.concatenate([ch["c"], oc[ok]]), "nrm": np.concatenate([ch["nrm"], on[ok]]),
            "ref": np.concatenate([ch["ref"], orf[ok]]).astype(np.int32),
            "mask": np.concatenate([ch["mask"], m[ok]]).astype(np.uint64),
            "avg": np.concatenate([ch["avg"], a[ok]]),
            "cell": np.concatenate([ch["cell"], np.full((int(ok.sum()), 2), -1)]).astype(np.int32),
            "kind": np.concatenate([np.zeros(P, np.int32), np.where(sign[ok] > 0, 1, 2).astype(np.int32)]),
            "src": pick[ok]}


def in_border_cells(sc, ref, cell_ij, cell):
    """Flags of the rows whose own cell lies in the first or last cell column or row."""
    nci, ncj = er.grid_shape(sc.W, sc.H, cell)
    ij = np.asarray(cell_ij).reshape(-1, 2)
    return (ij[:, 0] == 0) | (ij[:, 0] == nci - 1) | (ij[:, 1] == 0) | (ij[:, 1] == ncj - 1)


@functools.lru_cache(maxsize=None)
def planted_chain_set(cell, wid=3):
    """A start set for the loop with wrong patches in it (loop_reference.
    planted_set's recipe): cpu_chain's rows, each outlier of chain_mixed_set put
    in the place of the chain patch it was made from.  Every row counts as a
    seed (round 0, parent -1).  -> (set dict with max_dist and kind, rows of the outliers)."""
    sc = sphere(*CHAIN_SIZE)
    m = chain_mixed_set(cell, wid)
    P = int((m["kind"] == 0).sum())
    src = m["src"]
    out = {k: m[k][:P].copy() for k in ("c", "nrm", "ref", "mask", "avg", "cell", "kind")}
    for k in ("c", "nrm", "mask", "avg", "kind"):
        out[k][src] = m[k][P:]
    assert np.array_equal(out["ref"][src], m["ref"][P:])
    out["count"] = np.array([sum(bin(int(w)).count("1") for w in row) for row in out["mask"]], np.int32)
    out["round"] = np.zeros(P, np.int32)
    out["parent"] = np.full(P, -1, np.int64)
    out["max_dist"] = er.default_max_dist(sc.K, sc.Rp, sc.t, out["c"][0], out["ref"][0], cell)
    return out, src
