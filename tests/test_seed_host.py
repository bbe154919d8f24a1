"""The seed matcher's restatement (tests/seed_reference.py) and the host pieces
of the seeding path, no GPU: the planted set, seed_view_pairs, the oriented PLY
round trip, the colour rule and refused arguments."""
import numpy as np
import pytest

import seed_reference as sd


def test_planted_pairs_are_found(pkg):
    """At epi_px 1.5 every pair of features of one planted point, over the
    pairs (r, r+1), (r, r-1), (r, r+2), is among the candidates (a condition:
    7,481 of 7,481; at 1.0, 32 are missed), and the points triangulated from
    them lie within 9 % of the radius of the surface."""
    p = sd.planted(pkg)
    m = sd.planted_match(pkg, 1.5)
    true = sd.true_rows(p, m)
    planted = sum(len(np.intersect1d(p["ids"][r], p["ids"][v])) for r, v in p["pairs"])
    rows = sum(len(p["feats"][r]) for r, _ in p["pairs"])
    print(f"{len(p['feat'])} features, {planted} planted pairs, {len(m['err'])} candidates, "
          f"{len(m['err']) / len(p['feat']):.1f} per feature, {len(m['err']) / rows:.2f} per (pair, feature)")
    assert planted == 7481 and int(true.sum()) == planted and len(m["err"]) == 52822
    found = set(map(tuple, m["cand"][true][:, :3].tolist()))
    for k, (r, v) in enumerate(p["pairs"]):
        common, ia, ib = np.intersect1d(p["ids"][r], p["ids"][v], return_indices=True)
        assert all((k, int(a), int(b)) in found for a, b in zip(ia, ib)), k
    assert int(sd.true_rows(p, sd.planted_match(pkg, 1.0)).sum()) == planted - 32
    dev = np.abs(np.linalg.norm(m["c"][true], axis=1) - p["rad"]) / p["rad"]
    assert dev.max() < 0.09
    # order, normals, the seed on its own feature's ray
    key = m["cand"][:, 0].astype(np.int64) * 10**8 + m["cand"][:, 1].astype(np.int64) * 10**4 + m["cand"][:, 2]
    assert np.all(np.diff(key) > 0)
    assert np.allclose(np.linalg.norm(m["nrm"], axis=1), 1.0, rtol=0, atol=1e-15)
    assert np.array_equal(m["ref"], p["pairs"][m["cand"][:, 0], 0]) and np.array_equal(m["cand"][:, 3],
                                                                                        p["pairs"][m["cand"][:, 0], 1])
    for i in range(0, len(m["err"]), 997):
        r, a = int(m["ref"][i]), int(m["cand"][i, 1])
        x, y, depth = sd.wr.project_ref(p["K"][r], p["Rp"][r], p["t"][r], m["c"][i])
        assert depth > 0 and abs(x - p["feats"][r][a, 0]) < 1e-9 and abs(y - p["feats"][r][a, 1]) < 1e-9


def test_match_rules_and_refusals(pkg):
    p = sd.planted(pkg)
    K, Rp, t = p["K"], p["Rp"], p["t"]
    off = np.zeros(25, np.int64)
    off[1:] = 1
    off[2:] = 2
    feat = np.array([p["feats"][0][0], p["feats"][1][0]], np.int32)
    assert len(sd.match(K, Rp, t, feat, off, [(0, 1)], 1e6, 0.0)["err"]) == 1
    assert len(sd.match(K, Rp, t, feat, off, [(0, 1)], 1e6, 0.999)["err"]) == 0         # 15 degrees apart
    assert len(sd.match(K, Rp, t, feat, off, [], 1.5, 0.0)["err"]) == 0
    for bad in (dict(pairs=[(0, 0)]), dict(pairs=[(0, 24)]), dict(pairs=[(-1, 0)]), dict(epi_px=0.0),
                dict(epi_px=float("inf")), dict(min_sin2=1.0), dict(min_sin2=-1e-9), dict(off=off[::-1].copy()),
                dict(off=off[:-1])):
        kw = dict(pairs=[(0, 1)], epi_px=1.5, min_sin2=1e-4, off=off)
        kw.update(bad)
        with pytest.raises(ValueError):
            sd.match(K, Rp, t, feat, kw["off"], kw["pairs"], kw["epi_px"], kw["min_sin2"])


def test_view_pairs(pkg):
    p = sd.planted(pkg)
    pairs = pkg._lib.seed_view_pairs(p["Rp"], 4, 0.5)
    assert pairs.dtype == np.int32 and pairs.shape == (96, 2)
    for r in range(24):
        assert np.all(pairs[4 * r:4 * r + 4, 0] == r)
        assert set(pairs[4 * r:4 * r + 4, 1].tolist()) == {(r + d) % 24 for d in (-2, -1, 1, 2)}
        assert set(pairs[4 * r:4 * r + 2, 1].tolist()) == {(r + 1) % 24, (r - 1) % 24}       # nearest first
    assert len(pkg._lib.seed_view_pairs(p["Rp"], 4, 1.1)) == 0                 # removes every view
    assert pkg._lib.seed_view_pairs(p["Rp"], 4, 1.1).shape == (0, 2)
    assert len(pkg._lib.seed_view_pairs(p["Rp"], 0, 0.5)) == 0
    # cos 30 degrees = 0.866: only the two nearest views of the 15-degree ring
    assert len(pkg._lib.seed_view_pairs(p["Rp"], 4, 0.9)) == 48
    # exact ties go to the lower view: axes at right angles and one repeated
    Rp = np.tile(np.eye(3), (5, 1, 1))
    Rp[0, 2], Rp[1, 2], Rp[2, 2], Rp[3, 2], Rp[4, 2] = (0, 0, 1), (0, 0.6, 0.8), (0.6, 0, 0.8), (0, 0, 1), (0, -0.6, 0.8)
    got = pkg._lib.seed_view_pairs(Rp, 3, 0.5)
    assert got[:3].tolist() == [[0, 3], [0, 1], [0, 2]]
    assert got[9:12].tolist() == [[3, 0], [3, 1], [3, 2]]
    assert pkg._lib.seed_view_pairs(Rp, 4, 0.5)[:4].tolist() == [[0, 3], [0, 1], [0, 2], [0, 4]]
    assert pkg._lib.seed_view_pairs(Rp, 4, 0.9)[:1].tolist() == [[0, 3]]


def test_oriented_ply_roundtrip(pkg, tmp_path):
    rng = np.random.default_rng(0)
    pts, nrm, col = rng.normal(size=(50, 3)), rng.normal(size=(50, 3)), rng.uniform(0, 255, (50, 3))
    path = str(tmp_path / "o")
    pkg.export2ply_oriented(pts, nrm, col, path=path)
    raw = open(path + ".ply", "rb").read()
    head = raw[:raw.index(b"end_header\n")].decode().splitlines()
    assert head[:3] == ["ply", "format binary_little_endian 1.0", "element vertex 50"]
    assert head[3:] == [f"property double {k}" for k in ("x", "y", "z", "nx", "ny", "nz", "red", "green", "blue")]
    back = pkg.read_ply_oriented(path + ".ply")
    for got, want in zip(back, (pts, nrm, col)):
        assert got.tobytes() == want.tobytes()
    pkg.export2ply_oriented(np.empty((0, 3)), np.empty((0, 3)), np.empty((0, 3)), path=path)
    assert all(x.shape == (0, 3) for x in pkg.read_ply_oriented(path + ".ply"))
    with pytest.raises(RuntimeError):
        pkg.export2ply_oriented(pts, nrm[:4], col, path=path)
    pkg.export2ply(pts, col, path=path)                      # the six-property file is not an oriented cloud
    with pytest.raises(RuntimeError):
        pkg.read_ply_oriented(path + ".ply")
    assert pkg.read_ply(path + ".ply").shape == (50, 6)


def test_colour_rule(pkg):
    p = sd.planted(pkg)
    K, Rp, t = p["K"], p["Rp"], p["t"]
    const = np.empty_like(p["rgb"])
    const[..., 0], const[..., 1], const[..., 2] = 201, 17, 255
    m = sd.planted_match(pkg, 1.5)
    c, ref = m["c"][::4000], m["ref"][::4000]
    mask = np.full((len(ref), 1), 0xFFFFFF, np.uint64)
    col, nv = sd.color(const, K, Rp, t, c, ref, mask)
    assert nv.min() >= 2 and nv.max() == 24 and np.all(col == [201.0, 17.0, 255.0])          # exactly the constant
    # no view sees it: behind every camera's image, nan, a dead ref with an empty mask
    far = np.array([[5.0, 5.0, 5.0], [np.nan, 0, 0], c[0]])
    col, nv = sd.color(p["rgb"], K, Rp, t, far, np.array([0, 1, -1], np.int32), np.array([[0xFFFFFF], [1], [0]], np.uint64))
    assert not nv.any() and not col.any()
    # bits >= V name no view; the reference view counts once
    col1, nv1 = sd.color(p["rgb"], K, Rp, t, c[:1], ref[:1], np.array([[1 << 40 | 1 << int(ref[0])]], np.uint64))
    assert nv1[0] == 1
    # a hand-made sample: a 2 x 2 ramp seen by one camera at a half-pixel offset
    col2, _ = sd.color(p["rgb"], K, Rp, t, c[:1], ref[:1], np.zeros((1, 1), np.uint64))
    assert col1.tobytes() == col2.tobytes()
    assert np.all(col2 * 256 == np.round(col2 * 256))                      # steps of 1/256 with one view
