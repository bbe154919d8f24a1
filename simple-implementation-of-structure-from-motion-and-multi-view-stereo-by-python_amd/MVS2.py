"""Drop-in for the reference's MVS stage (MVS2.py), running on MI355X.

DensePointsWithMVS2(imgs, global_set, args)   MVS2.py:176-295
    Same arguments, prints and side effects (initial_patches.ply,
    all_patches.ply in the working directory).  Seeding, the 100k-pop FIFO
    expansion and the cell-table output order run in libmvs_amd.so: photo
    tests on the GPU (HIP, gfx950), the order-dependent commit on the host.
MyPatch.photo_consistenecy_test(...)          MVS2.py:62-77
    Same method on the same fields; one-candidate call of the batched GPU
    scorer.  Use photo_consistency_batch for many candidates.
"""
import os
import sys
import time
import zlib

import numpy as np

from . import _lib
from .utils import export2ply, export2ply_mesh, export2ply_oriented, pars_to_arrays, read_pars, tracks_to_arrays

last_stats = {}
_ctx_cache = {}


def _device_index():
    import os
    return int(os.environ.get("LOCAL_RANK", os.environ.get("MVS_DEVICE", "0")))


def _images_key(imgs):
    """Identity and a content fingerprint of the image list: the element
    arrays' ids, buffers and shapes, and a CRC of every 5th pixel of every
    61st row of each image (~0.15 MB for dinoRing's 48 views, so the
    per-candidate drop-in stays cheap).  The reference re-reads imgs on every
    photo test; a caller that replaces an array, or rewrites sampled pixels in
    place, gets a fresh context.  (A change confined to unsampled pixels is
    not seen: call clear_context_cache().)"""
    parts = [id(imgs), len(imgs)]
    crc = 0
    for a in imgs:
        a = np.asarray(a)
        parts += [id(a), a.shape, a.__array_interface__["data"][0]]
        crc = zlib.crc32(np.ascontiguousarray(a[::61, ::5]).tobytes(), crc)
    parts.append(crc)
    return tuple(parts)


def clear_context_cache():
    """Forget the cached GPU context (e.g. after editing images in place).  The
    context itself is not closed here: whoever still holds it (a running
    Stage, an SfM matcher) keeps a valid handle, and it is destroyed when the
    last reference goes."""
    _ctx_cache.clear()


def scene_context(imgs, par_K, par_r, par_t, device=None):
    """MvsContext for (imgs, cameras), cached on the images (identity + a
    sampled content fingerprint, _images_key) and the camera values (SfM and
    MVS each call read_pars, MVS2.py:178 / SFM.py:54)."""
    K, R, t = pars_to_arrays(par_K, par_r, par_t, len(imgs))
    key = (_images_key(imgs), K.tobytes(), R.tobytes(), t.tobytes())
    ctx = _ctx_cache.get(key)
    if ctx is None:
        ctx = _lib.MvsContext(imgs, K, R, t, device=_device_index() if device is None else device)
        clear_context_cache()
        _ctx_cache[key] = (ctx, imgs)
        return ctx
    return ctx[0]


class MyPatch(object):
    """Patch record with the reference's fields (MVS2.py:45-57)."""

    def __init__(self, centroid, normal, reference_img_index, visible_set, color, dist, patch_size=5):
        self.dist = dist
        self.c = centroid
        self.n = normal
        self.R = reference_img_index
        self.V = visible_set if visible_set is not None else []
        self.color = color
        self.patch_size = patch_size
        self.avg_ncc_score = 0

    def visible_ct(self):
        return len(self.V)

    def photo_consistenecy_test(self, imgs, par_K, par_r, par_t, MIN_NCC=0.7):
        ctx = scene_context(imgs, par_K, par_r, par_t)
        xy, mask, count, avg = ctx.score(np.asarray(self.c, np.float64)[None], [self.R], MIN_NCC, 5)
        for idx in _mask_views(mask[0]):
            self.V.append([idx, xy[0, 0], xy[0, 1]])
        # the reference's own sum of the passing nccs / |V| (MVS2.py:73-76), bit-exact
        self.avg_ncc_score = float(ctx.exact_avg([self.R], xy, mask, 5)[0]) if count[0] else 0
        return self.V


def _mask_views(words):
    out = []
    for w, m in enumerate(np.asarray(words, np.uint64)):
        m = int(m)
        while m:
            b = (m & -m).bit_length() - 1
            out.append(64 * w + b)
            m &= m - 1
    return out


def photo_consistency_batch(ctx, centroids, ref_views, MIN_NCC=0.7, wid=5):
    """Batched photo test: (xy, mask, count, avg) per candidate."""
    return ctx.score(centroids, ref_views, MIN_NCC, wid)


def photo_consistency_warped(ctx, centroids, normals, ref_views, MIN_NCC=0.7, wid=5, min_cos=0.0):
    """Batched plane-warped photo test (no reference counterpart; see
    MvsContext.score_warped): (xy, mask, count, avg) per candidate."""
    return ctx.score_warped(centroids, normals, ref_views, MIN_NCC, wid, min_cos)


def refine_patches_warped(ctx, centroids, normals, ref_views, MIN_NCC=0.7, wid=5, min_cos=0.0, **kw):
    """Depth and normal refinement of patches against the plane-warped photo
    test (no reference counterpart; see MvsContext.refine_warped, which takes
    the remaining keywords): refined centroids, refined normals, the final
    test's (xy, mask, count, avg) and the info dict."""
    return ctx.refine_warped(centroids, normals, ref_views, wid=wid, min_ncc=MIN_NCC, min_cos=min_cos, **kw)


def expand_patches_warped(ctx, centroids, normals, ref_views, rounds=4, cell_size=2, MIN_NCC=0.7, wid=5,
                          min_cos=0.3, **kw):
    """Level-synchronous patch expansion driven by the plane-warped photo test
    and, with refine_levels > 0, the refinement (no reference counterpart; see
    MvsContext.expand_warped, which takes the remaining keywords): the dict of
    patch arrays grown from the seed patches."""
    return ctx.expand_warped(centroids, normals, ref_views, rounds, cell_size=cell_size, wid=wid, min_ncc=MIN_NCC,
                             min_cos=min_cos, **kw)


def filter_patches_warped(ctx, patches, **kw):
    """Visibility-consistency filter of a warped patch set (no reference
    counterpart; see MvsContext.filter_warped, which takes the keywords):
    `patches` is the dict expand_patches_warped returns; the surviving patches
    with their rows in the input, the front grid and the occupancy."""
    return ctx.filter_warped(patches, **kw)


def resume_patches_warped(ctx, patches, rounds=2, cell_size=2, MIN_NCC=0.7, wid=5, min_cos=0.3, **kw):
    """More rounds of the expansion from an existing warped patch set, e.g. the
    survivors of filter_patches_warped (no reference counterpart; see
    MvsContext.resume_warped, which takes the remaining keywords)."""
    return ctx.resume_warped(patches, rounds, cell_size=cell_size, wid=wid, min_ncc=MIN_NCC, min_cos=min_cos, **kw)


def reconstruct_patches_warped(ctx, centroids, normals, ref_views, **kw):
    """The expand -> filter loop of the warped pipeline (no reference
    counterpart; see MvsContext.reconstruct_warped, which takes the keywords):
    the filtered patch set grown from the seed patches, and the loop's history."""
    return ctx.reconstruct_warped(centroids, normals, ref_views, **kw)


def depth_maps_warped(ctx, patches, **kw):
    """Per-view depth and normal maps of a warped patch set and the dense cloud
    fused from them (no reference counterpart; see MvsContext.depth_maps, which
    takes the keywords): `patches` is the dict expand_patches_warped,
    filter_patches_warped or reconstruct_patches_warped returns."""
    return ctx.depth_maps(patches, **kw)


def densify_depth_warped(ctx, maps, **kw):
    """The maps of depth_maps_warped densified by per-pixel plane propagation
    and fused again (no reference counterpart; see MvsContext.densify_depth,
    which takes the keywords): `maps` needs z and normal."""
    return ctx.densify_depth(maps, **kw)


def mesh_depth_warped(ctx, maps, **kw):
    """A triangle mesh of the maps of depth_maps_warped or densify_depth_warped:
    signed-distance fusion and marching tetrahedra (no reference counterpart;
    see MvsContext.mesh_depth, which takes the keywords): `maps` needs z."""
    return ctx.mesh_depth(maps, **kw)


def write_depth_maps(maps, directory, first_view=0, dense_path="warped_dense"):
    """The files of a depth_maps_warped or densify_depth_warped result:
    directory/depth_%04d.npy (H,W) float32, nan for empty pixels, and
    directory/normal_%04d.npy (H,W,3) float32 per view, score_%04d.npy (H,W)
    float32 where the result has a score (the densified maps), and the fused
    cloud as dense_path + '.ply' (export2ply_oriented)."""
    os.makedirs(directory, exist_ok=True)
    for k in range(len(maps["z"])):
        z = np.where(np.isfinite(maps["z"][k]), maps["z"][k], np.nan).astype(np.float32)
        np.save(os.path.join(directory, "depth_%04d.npy" % (first_view + k)), z)
        np.save(os.path.join(directory, "normal_%04d.npy" % (first_view + k)), maps["normal"][k].astype(np.float32))
        if "score" in maps:
            np.save(os.path.join(directory, "score_%04d.npy" % (first_view + k)), maps["score"][k].astype(np.float32))
    export2ply_oriented(maps["points"], maps["normals"], maps["colors"], path=dense_path)


def DensePointsWarped(imgs, args, rounds=4, iterations=3, epi_px=1.5, min_sin2=1e-4, neighbours=4, min_axis_cos=0.5,
                      feats=None, pairs=None, path="warped_patches", device=None, depth_maps=None, depth_radius=1,
                      dense_path="warped_dense", densify=0, mesh=0, mesh_path="warped_mesh", **kw):
    """An oriented, coloured point cloud from calibrated images alone (no
    reference counterpart; PMVS's match -> expand -> filter on the warped
    pipeline, without SfM tracks):

      1. read_pars(args) and the scene context;
      2. MvsContext.seed_warped: Harris features of every view matched along the
         epipolar lines of their neighbour views (wseed_pairs(neighbours,
         min_axis_cos), epi_px, min_sin2) into oriented seed candidates
         (feats, pairs: the caller's own features and view pairs instead);
      3. MvsContext.reconstruct_warped from them: `rounds` rounds of
         expand_warped (its round 0 keeps the best-scoring candidate per
         (reference view, cell)), then `iterations` of filter and resumption;
         the remaining keywords (resume_rounds, expand, filter) are its own;
      4. MvsContext.wpatch_color of the final set;
      5. export2ply_oriented -> path + '.ply' (points, normals, colours);
      6. one line of counts.

    depth_maps (a directory, default None: nothing more happens): after step 5,
    MvsContext.depth_maps of the final set at radius depth_radius, written by
    write_depth_maps -- depth_%04d.npy and normal_%04d.npy per view into the
    directory and the fused cloud as dense_path + '.ply'; the count line and
    the counts gain "dense", the number of fused points, and the returned dict
    gains "maps".  densify = N > 0 (default 0: nothing changes): the first N sweeps
    of MvsContext.densify_depth's default schedule run on those maps; the
    densified maps are written instead, with score_%04d.npy per view, the dense
    cloud is fused from them, and the count line and the counts gain
    "densified", the pixels that hold a depth afterwards.  N above the schedule's
    12 sweeps, or N > 0 without depth_maps, raises RuntimeError.  mesh = N > 0
    (default 0: nothing changes): MvsContext.mesh_depth of those maps (densified
    when densify is given) at resolution N, written by export2ply_mesh as
    mesh_path + '.ply'; the count line and the counts gain "mesh_vertices" and
    "mesh_faces" and the returned dict gains "mesh".  N > 0 without depth_maps
    raises RuntimeError.

    Returns a dict: points, normals, colors (n,3), nviews, patches (the final
    set as reconstruct_warped returns it) and counts (features, pairs, tests,
    candidates, winners0, patches per iteration); the counts are also left in
    MVS2.last_stats."""
    t0 = time.time()
    densify = int(densify)
    if densify < 0 or densify > len(_lib.MvsContext.DENSIFY_SCHEDULE):
        raise RuntimeError(f"densify must be in 0..{len(_lib.MvsContext.DENSIFY_SCHEDULE)} (the sweeps of the default schedule)")
    if densify > 0 and depth_maps is None:
        raise RuntimeError("densify needs depth_maps (a directory for the maps it densifies)")
    mesh = int(mesh)
    if mesh < 0:
        raise RuntimeError("mesh must be >= 0 (the lattice's resolution along the longest side)")
    if mesh > 0 and depth_maps is None:
        raise RuntimeError("mesh needs depth_maps (a directory for the maps it fuses)")
    par_K, par_r, par_t = read_pars(args)
    ctx = scene_context(imgs, par_K, par_r, par_t, device)
    expand = dict(kw.pop("expand", None) or {})
    if pairs is None:
        pairs = ctx.wseed_pairs(neighbours, min_axis_cos)
    c, nrm, ref, cand, err = ctx.seed_warped(feats=feats, pairs=pairs, epi_px=epi_px, min_sin2=min_sin2,
                                             wid=expand.get("wid", 5))
    counts = {k: ctx.last_seed[k] for k in ("features", "pairs", "tests", "candidates")}
    # the seeds' expansion here, so that round 0's winners can be counted; the loop takes it from there
    first = ctx.expand_warped(c, nrm, ref, rounds, **expand)
    counts["winners0"] = int((first["round"] == 0).sum())
    ps = ctx.reconstruct_warped(None, None, None, iterations=iterations, rounds=rounds, expand=expand, start=first,
                                **kw)
    counts["patches"] = [h["patches"] for h in ps["history"]] + [len(ps["ref"])]
    colors, nviews = ctx.wpatch_color(ps["c"], ps["ref"], ps["mask"])
    export2ply_oriented(ps["c"], ps["nrm"], colors, path=path)
    maps = surface = None
    if depth_maps is not None:
        maps = ctx.depth_maps(ps, radius=depth_radius)
        if densify > 0:
            maps = ctx.densify_depth(maps, schedule=ctx.DENSIFY_SCHEDULE[:densify])
            counts["densified"] = int(np.isfinite(maps["z"]).sum())
        write_depth_maps(maps, depth_maps, dense_path=dense_path)
        counts["dense"] = len(maps["points"])
        if mesh > 0:
            surface = ctx.mesh_depth(maps, resolution=mesh)
            export2ply_mesh(surface["vertices"], surface["colors"], surface["faces"], path=mesh_path)
            counts["mesh_vertices"], counts["mesh_faces"] = len(surface["vertices"]), len(surface["faces"])
    counts["seconds"] = time.time() - t0
    print("warped: features {features} pairs {pairs} candidates {candidates} round-0 winners {winners0} "
          "patches per iteration {patches}".format(**counts) + (" dense {dense}".format(**counts) if maps else "")
          + (" densified {densified}".format(**counts) if "densified" in counts else "")
          + (" mesh vertices {mesh_vertices} faces {mesh_faces}".format(**counts) if surface is not None else ""))
    last_stats.clear()
    last_stats.update(counts)
    out = {"points": ps["c"], "normals": ps["nrm"], "colors": colors, "nviews": nviews, "patches": ps,
           "counts": counts}
    if maps is not None:
        out["maps"] = maps
    if surface is not None:
        out["mesh"] = surface
    return out


def DensePointsWithMVS2(imgs, global_set, args, max_pops=100000, device=None):
    """MVS2.py:176-295 on the GPU.  Returns None like the reference; the run's
    counters are left in MVS2.last_stats.

    Under torch.distributed with world size > 1 (one process per GPU), the
    expansion sweeps are sharded across ranks (parallel.stage_sharded); every
    rank ends with the same patches and rank 0 writes the PLY files.

    `args.filter_outliers` (opt-in, default off) runs CellTable.filter_out_outlier
    (MVS2.py:132-158) before the reconstruction, as if the reference's
    commented-out call at MVS2.py:281 were enabled, with its prints."""
    t0 = time.time()
    filter_outliers = bool(getattr(args, "filter_outliers", False))
    par_K, par_r, par_t = read_pars(args)
    n_observations, n_world_points, legal_sets = global_set.getInfo()
    track_off, obs_view, obs_xy = tracks_to_arrays(legal_sets)
    ctx = scene_context(imgs, par_K, par_r, par_t, device)
    import torch.distributed as dist
    world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
    if world > 1:
        from . import parallel
        initial, allp, stats = parallel.stage_sharded(
            ctx, track_off, obs_view, obs_xy, cell_size=args.cell_size, scale=args.scale, wid=5,
            max_pops=max_pops, device=device, filter_outliers=filter_outliers)
        if dist.get_rank() != 0:
            last_stats.clear()
            last_stats.update(stats)
            return None
    else:
        initial, allp, stats = ctx.stage(track_off, obs_view, obs_xy, cell_size=args.cell_size,
                                         scale=args.scale, wid=5, max_pops=max_pops,
                                         filter_outliers=filter_outliers)
    print("len of initial patches", len(initial))
    export2ply(initial[:, :3], initial[:, 3:], path="initial_patches")
    print("filter outliers")
    if filter_outliers:
        # filter_out_outlier's own prints (MVS2.py:155), one per removed Q-table entry
        left = stats["outlier_lines"]
        while left > 0:
            k = min(left, 1 << 16)
            sys.stdout.write("remove a outlier\n" * k)
            left -= k
    print("reconstruct point cloud")
    t1 = time.time()
    print("Optimization took {0:.0f} seconds".format(t1 - t0))
    print("points len:", len(allp))
    export2ply(allp[:, :3], allp[:, 3:], path="all_patches")
    stats["seconds"] = t1 - t0
    last_stats.clear()
    last_stats.update(stats)
    return None
