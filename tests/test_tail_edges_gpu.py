"""The Frame-tail kernels (csrc/planes_tail.hip, line3d.hip, lpvo.hip) away from 640 x 480 and away from what PEAC happens to output:
odd and tiny geometries, a depth image that is a view into a wider parent (stride != 2 * w), hand-written labels and plane records that
reach the branches of the per-plane tail one by one, capacity edges, and the resident paths (pitch != w) at 501 x 397.

The reference side is the CPU oracle.  Every input is first run through the oracle in a module-scope fixture, which asserts what makes the
case non-vacuous (the `*_cases` fixtures; test_preconditions_hold_without_a_gpu runs them in the CPU suite).  The device results are then
compared with the exactness the project uses everywhere else: normals, 3-D lines and LPVO byte for byte, voxel clouds and the integer plane
fields exactly, refit coefficients at 1e-5, n_inliers by the recount rule of tests/test_planes_tail.py."""
import numpy as np
import pytest

import tail_abi as abi

FX, FY, CX, CY = 535.4, 539.2, 320.1, 247.6
K0 = (FX, FY, CX, CY)
DIST_TH = 0.05


def plane_depth(n, d, w, h, K=K0, units=5000.0):
    """u16 depth image of the plane n . X = d seen through K = (fx, fy, cx, cy); `units` raw steps per metre"""
    j = np.arange(w)[None, :]; i = np.arange(h)[:, None]
    z = d / (n[0] * (j - K[2]) / K[0] + n[1] * (i - K[3]) / K[1] + n[2])
    return np.clip(np.rint(z * units), 0, 65535).astype(np.uint16)


# ====================================================================================================== 1. surface normals over geometry
#  h, w         grid W x H
SN_GEOMS = [(130, 187),   # W = 63: one row of k_sn_serial's 64-lane loops, last lane idle
            (130, 190),   # W = 64: exactly one trip
            (130, 193),   # W = 65: a second trip for one element
            (61, 64),     # W = 22, H = 21: a 2 x 1 interior past the 10-cell border -- at the even row 10, which is not sampled: all NaN
            (67, 64),     # W = 22, H = 23: the smallest grid with a sampled interior position (row 11, column 11)
            (60, 60),     # W = H = 20: everything is border
            (247, 322), (397, 501),                                    # odd sizes, W odd and even
            (480, 335),   # portrait
            (3, 3)]       # one 1 x 1 grid, zero outputs
SN_ALL_NAN = {(61, 64), (60, 60), (3, 3)}
SN_SEED = 0x5EED3001


def sn_grid(h, w):
    return (w + 2) // 3, (h + 2) // 3


def sn_inputs(synth, h, w):
    plane = plane_depth((0.1, 0.2, 1.0), 2.0, w, h)
    step = plane.copy()                                               # a depth step and a zero hole, both touching the first and the last grid column
    step[h // 3: h // 2, :] = plane_depth((0.1, 0.2, 1.0), 3.0, w, h)[h // 3: h // 2, :]
    r0 = (2 * h) // 3; r1 = r0 + max(3, h // 10); k = max(w // 5, 1)
    step[r0:r1, :k] = 0; step[r0:r1, w - k:] = 0
    return [("plane", plane), ("step", step), ("synth", synth.make_depth(SN_SEED, w, h))]


@pytest.fixture(scope="module")
def sn_cases(orc, synth):
    cases = {}
    for h, w in SN_GEOMS:
        W, H = sn_grid(h, w)
        rows = []
        for name, d in sn_inputs(synth, h, w):
            so = orc.surface_normals(d)
            assert len(so) == (H // 2) * (W // 2), (h, w, name)
            fin = np.isfinite(so["normal"][:, 0])
            gx = so["frame_x"] // 3; gy = so["frame_y"] // 3
            inside = (gx >= 10) & (gx < W - 10) & (gy >= 10) & (gy < H - 10)
            assert not fin[~inside].any()
            if (h, w) in SN_ALL_NAN:
                assert not fin.any() and not inside.any()
            elif name == "plane":
                assert fin.sum() >= 1 and np.array_equal(fin, inside)
            elif name == "step" and inside.sum() >= 4:
                assert fin[inside].any() and (~fin[inside]).any(), (h, w)
            rows.append((name, d, so))
        cases[(h, w)] = rows
    assert len(cases[(3, 3)][0][2]) == 0 and cases[(67, 64)][0][2]["frame_x"][np.isfinite(cases[(67, 64)][0][2]["normal"][:, 0])].tolist() == [33]
    return cases


@pytest.mark.gpu
@pytest.mark.parametrize("h,w", SN_GEOMS)
def test_surface_normals_over_geometry(hvo, gpu_ctx, sn_cases, h, w):
    for name, d, so in sn_cases[(h, w)]:
        rc, sg, n = abi.surface_normals(hvo, gpu_ctx, d)
        assert rc == abi.OK and n == len(so), (name, rc, n)
        assert sg[:n].tobytes() == so.tobytes(), (name, [f for f in so.dtype.names if not np.array_equal(sg[:n][f], so[f], equal_nan=True)])


SN_TOO_WIDE = 2272            # W = 758: k_sn_serial would need 9 * 3 * 760 * 8 = 164160 bytes of LDS, more than the 160 KiB there are


@pytest.mark.gpu
def test_surface_normals_refuses_a_width_past_the_lds_limit(hvo, gpu_ctx):
    """HVO_ERR_UNSUPPORTED before anything is uploaded or launched (hvo_surface_normals and sn_enqueue both check first), nothing is
    written to the caller's array, and the context goes on working"""
    assert 9 * 3 * (sn_grid(9, SN_TOO_WIDE)[0] + 2) * 8 > 160 * 1024 and sn_grid(9, SN_TOO_WIDE)[0] + 2 > 758
    d = plane_depth((0.1, 0.2, 1.0), 2.0, SN_TOO_WIDE, 9)
    rc, sg, n = abi.surface_normals(hvo, gpu_ctx, d, fill=0xA5)
    assert rc == abi.UNSUPPORTED and n == 0
    assert sg.tobytes() == b"\xa5" * sg.nbytes
    rc, sg, n = abi.surface_normals(hvo, gpu_ctx, plane_depth((0.1, 0.2, 1.0), 2.0, 64, 67))
    assert rc == abi.OK and n == 11 * 11


# ====================================================================================================== 2. stride
PADS = (2, 64, 258)
STRIDE_IMAGES = [(397, 501, 0x5EED3101), (480, 640, 0x5EED3102)]


def random_keylines(orc, w, h, n, seed):
    """random key lines as in tests/test_line3d.py, scaled to the image: some outside it, ten with integer end points, ten of (int)length 0"""
    rng = np.random.default_rng(seed)
    kl = np.zeros(n, orc.KEYLINE_DT)
    ext = 200.0 * min(w, h) / 480.0
    kl["sx"] = rng.uniform(-20, w + 20, n); kl["sy"] = rng.uniform(-20, h + 20, n)
    kl["ex"] = kl["sx"] + rng.uniform(-ext, ext, n); kl["ey"] = kl["sy"] + rng.uniform(-ext, ext, n)
    kl["sx"][:10] = np.floor(kl["sx"][:10]); kl["sy"][:10] = np.floor(kl["sy"][:10])
    kl["ex"][5:15] = kl["sx"][5:15]; kl["ey"][5:15] = kl["sy"][5:15] + 0.5
    return kl


@pytest.fixture(scope="module")
def stride_cases(orc, synth):
    cases = {}
    for h, w, seed in STRIDE_IMAGES:
        d = synth.make_depth(seed, w, h)
        assert d.max() < 0xFFFF                                       # the padding value occurs nowhere in the image
        c = dict(depth=d)
        c["sn"] = orc.surface_normals(d)
        assert np.isfinite(c["sn"]["normal"][:, 0]).sum() > 500
        lab, pl = orc.peac(d)
        c["labels"], c["planes"] = lab, pl
        c["pc"] = orc.plane_clouds(d, lab, pl, dist_th=DIST_TH)
        assert c["pc"][0]["valid"].sum() >= 1 and len(c["pc"][1]) > 100
        c["kl"] = random_keylines(orc, w, h, 200, seed & 0xFFFF)
        c["l3"] = orc.lines_3d(c["kl"], d, seed=7)
        assert 5 < c["l3"]["good"].sum() < len(c["kl"])
        c["lpvo"] = orc.normals_lpvo(d)
        assert len(c["lpvo"][0]) > 200
        cases[(h, w)] = c
    return cases


def _stride_calls(hvo, ctx, c, entry, view, stride=None):
    """-> (rc, bytes of everything the entry point wrote)"""
    if entry == "surface_normals":
        rc, out, n = abi.surface_normals(hvo, ctx, view, stride=stride)
        return rc, out.tobytes() + bytes([n & 0xFF])
    if entry == "plane_clouds":
        rc, out, cloud, n = abi.plane_clouds(hvo, ctx, view, c["labels"], c["planes"], dist_th=DIST_TH, stride=stride)
        return rc, out.tobytes() + cloud.tobytes() + int(n).to_bytes(4, "little", signed=True)
    if entry == "lines_3d":
        rc, out = abi.lines_3d(hvo, ctx, c["kl"], view, seed=7, stride=stride)
        return rc, out.tobytes()
    rc, nrm, dz, px = abi.normals_lpvo(hvo, ctx, view, stride=stride)
    return rc, nrm.tobytes() + dz.tobytes() + px.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ["surface_normals", "plane_clouds", "lines_3d", "normals_lpvo"])
@pytest.mark.parametrize("h,w", [g[:2] for g in STRIDE_IMAGES])
def test_depth_as_a_view_into_a_wider_parent(hvo, gpu_ctx, orc, stride_cases, h, w, entry):
    """rows 2, 64 and 258 bytes longer than the image, the padding filled with 0xFFFF: byte-equal to the contiguous call (which equals
    the oracle); a stride below 2 * w is HVO_ERR_INVALID_ARG"""
    c = stride_cases[(h, w)]; d = c["depth"]
    rc, ref = _stride_calls(hvo, gpu_ctx, c, entry, d)
    assert rc == abi.OK
    if entry == "surface_normals":
        assert ref[:-1] == c["sn"].tobytes()
    elif entry == "lines_3d":
        assert ref == c["l3"].tobytes()
    elif entry == "normals_lpvo":
        assert ref == c["lpvo"][0].tobytes() + c["lpvo"][1].tobytes() + c["lpvo"][2].tobytes()
    else:
        rc, pg, cg, n = abi.plane_clouds(hvo, gpu_ctx, d, c["labels"], c["planes"], dist_th=DIST_TH)
        check_plane_clouds(pg, cg, n, *c["pc"])
    for pad in PADS:
        rc, got = _stride_calls(hvo, gpu_ctx, c, entry, abi.padded(d, pad))
        assert rc == abi.OK and got == ref, pad
    rc, _ = _stride_calls(hvo, gpu_ctx, c, entry, d, stride=2 * w - 2)
    assert rc == abi.INVALID_ARG


# ====================================================================================================== 3. plane clouds on hand-made labels
def check_plane_clouds(pg, cg, n_total, po, co, upto=None, th=DIST_TH):
    """device records / cloud / total against the oracle's, the comparisons of tests/test_planes_tail.py; upto: only the first planes"""
    k = len(po) if upto is None else upto
    assert len(pg) == len(po)
    for f in ("valid", "gate_ok", "first", "n_points", "n_pixels"):
        assert np.array_equal(pg[f][:k], po[f][:k]), (f, pg[f][:k], po[f][:k])
    rows = len(co) if upto is None else int(po["first"][k - 1] + po["n_points"][k - 1]) if k else 0
    if upto is None:
        assert n_total == int(po["n_points"].sum()) and len(cg) == len(co)
    assert np.array_equal(cg[:rows], co[:rows])                       # voxel centroids: bit-exact
    assert np.allclose(pg["coef"][:k], po["coef"][:k], rtol=0, atol=1e-5), np.abs(pg["coef"][:k] - po["coef"][:k]).max()
    # n_inliers: recounted from each side's own coefficients in the reference's float order, each side's count is reproduced to the point
    for i in np.nonzero(pg["valid"][:k] == 1)[0]:
        pts = cg[pg["first"][i]: pg["first"][i] + pg["n_points"][i]].astype(np.float32)
        for coef, cnt in ((pg["coef"][i], pg["n_inliers"][i]), (po["coef"][i], po["n_inliers"][i])):
            c = coef.astype(np.float32)
            dist = ((c[0] * pts[:, 0] + c[1] * pts[:, 1]) + c[2] * pts[:, 2]) + c[3]
            assert int((np.abs(dist.astype(np.float64)) < th).sum()) == int(cnt), (i, cnt)
    assert np.all(np.abs(pg["n_inliers"][:k] - po["n_inliers"][:k]) <= 2)
    assert np.array_equal(pg["n_inliers"][:k][pg["valid"][:k] == 0], po["n_inliers"][:k][po["valid"][:k] == 0])


N_A, D_A = (0.1, 0.2, 1.0), 2.0
N_B, D_B = (-0.3, 0.1, 1.0), 2.5


def plane_record(orc, n, d, count=1, flip=False, shift=0.0):
    """the record of the plane n . X = d: unit normal (or its negative), the point of the plane nearest the origin (moved `shift` metres
    along the normal) as centre"""
    r = np.zeros(1, orc.PLANE_DT)
    nn = np.asarray(n, np.float64); s = np.linalg.norm(nn); nn = nn / s
    r["center"][0] = nn * (d / s + shift)
    r["normal"][0] = -nn if flip else nn
    return np.repeat(r, count)


def two_plane_scene(orc, w=160, h=120, K=K0, units=5000.0, na=N_A, da=D_A, nb=N_B, db=D_B):
    """left half plane A (label 0), right half plane B (label 1)"""
    d = plane_depth(na, da, w, h, K, units); d[:, w // 2:] = plane_depth(nb, db, w, h, K, units)[:, w // 2:]
    lab = np.zeros((h, w), np.int32); lab[:, w // 2:] = 1
    return d, lab, np.concatenate([plane_record(orc, na, da), plane_record(orc, nb, db)])


def pc_build(orc, synth):
    """name -> dict(depth, labels, planes[, n_planes, cap, K, depth_factor])"""
    S = {}
    w, h = 160, 120
    flat = plane_depth(N_A, D_A, w, h)
    # (a) planes of 0, 1, 2 and 3 pixels next to full ones, an empty plane between two full ones, 64 records of which six are used
    lab = np.zeros((h, w), np.int32); lab[60:, :] = 5
    lab[5, 5] = 2; lab[10, 10] = lab[10, 60] = 3; lab[20, 10] = lab[25, 80] = lab[100, 150] = 4
    pl = np.zeros(64, orc.PLANE_DT); pl[:6] = plane_record(orc, N_A, D_A, 6)
    S["a_tiny"] = dict(depth=flat, labels=lab, planes=pl)
    # (b) a one-row strip on the slanted plane (voxel centroids on a line up to depth quantisation) ...
    lab = np.zeros((h, w), np.int32); lab[60, :] = 1
    S["b_row_strip"] = dict(depth=flat, labels=lab, planes=plane_record(orc, N_A, D_A, 2))
    # ... and one on a fronto-parallel plane: y and z of every centroid are the same two floats, the centroids are exactly collinear
    lab = np.zeros((h, w), np.int32); lab[40, 8:152] = 1
    S["b_exact_strip"] = dict(depth=plane_depth((0, 0, 1.0), 1.5, w, h), labels=lab, planes=plane_record(orc, (0, 0, 1.0), 1.5, 2))
    # (c) exactly 3 voxel points (a thin triangle: the RANSAC model is kept, ninl = 3) and exactly 4 (refit, ninl = 4)
    lab = np.full((h, w), -1, np.int32); lab[:, 100:] = 0
    lab[30, 5] = lab[30, 45] = lab[31, 85] = 1
    lab[60, 5] = lab[60, 60] = lab[110, 5] = lab[110, 60] = 2
    S["c_three_four"] = dict(depth=flat, labels=lab, planes=plane_record(orc, N_A, D_A, 3))
    # (d) (e) (f) two half-image planes
    d2, lab2, pl2 = two_plane_scene(orc)
    S["d_plain"] = dict(depth=d2, labels=lab2, planes=pl2)
    bad = pl2.copy(); bad[0] = plane_record(orc, N_A, D_A, shift=0.3)[0]
    S["d_gate"] = dict(depth=d2, labels=lab2, planes=bad)
    S["e_negated"] = dict(depth=d2, labels=lab2, planes=np.concatenate([plane_record(orc, N_A, D_A, flip=True), plane_record(orc, N_B, D_B, flip=True)]))
    rng = np.random.default_rng(31)
    at = rng.choice(w * h, 400, replace=False)
    lf = lab2.copy().reshape(-1); lf[at] = np.tile(np.array([-1, -7, 2, 5], np.int32), 100); lm = lab2.copy().reshape(-1); lm[at] = -1
    S["f_sprinkled"] = dict(depth=d2, labels=lf.reshape(h, w), planes=pl2)
    S["f_minus_one"] = dict(depth=d2, labels=lm.reshape(h, w), planes=pl2)
    # (g) 64 planes: an 8 x 8 checkerboard of 40 x 30 patches on one slanted plane
    w, h = 320, 240
    lab = (np.arange(h)[:, None] // 30) * 8 + (np.arange(w)[None, :] // 40)
    S["g_64"] = dict(depth=plane_depth(N_A, 4.0, w, h), labels=lab.astype(np.int32), planes=plane_record(orc, N_A, 4.0, 64))
    # (h) depth in millimetres, intrinsics of a 320 x 240 camera
    Kd = synth.intrinsics(w, h); K = tuple(float(np.float32(Kd[k])) for k in ("fx", "fy", "cx", "cy")); mm = float(np.float32(0.001))
    d3, lab3, pl3 = two_plane_scene(orc, w, h, K, 1000.0)
    S["h_mm"] = dict(depth=d3, labels=lab3, planes=pl3, K=K, depth_factor=mm)
    # a wall in the upper rows (label 0), then a floor 1.5 m below the camera that runs out to 60 m (label 1), then a strip of the wall again (label 2)
    horizon = int(np.ceil(K[3])); far = 1.5 * K[1] / 60.0                                   # rows below cy + far are nearer than 60 m
    r0 = horizon + int(np.ceil(far))
    d4 = plane_depth((0, 0, 1.0), 3.0, w, h, K, 1000.0); d4[r0:, :] = plane_depth((0, 1.0, 0), 1.5, w, h, K, 1000.0)[r0:, :]
    lab4 = np.zeros((h, w), np.int32); lab4[r0:, :] = 1; lab4[:20, :] = 2
    S["h_overflow"] = dict(depth=d4, labels=lab4, K=K, depth_factor=mm,
                           planes=np.concatenate([plane_record(orc, (0, 0, 1.0), 3.0), plane_record(orc, (0, 1.0, 0), 1.5), plane_record(orc, (0, 0, 1.0), 3.0)]))
    return S


def floor_cells(c):
    """k_pc_setup's arithmetic for plane 1 of the overflow scene: floor(min * 10) .. floor(max * 10) per axis in float, the product of the extents"""
    K = c["K"]; f = np.float32
    i, j = np.nonzero(c["labels"] == 1)
    z = c["depth"][i, j].astype(np.float64) * np.float64(f(c["depth_factor"]))
    P = np.stack([((j - np.float64(f(K[2]))) * z / np.float64(f(K[0]))), ((i - np.float64(f(K[3]))) * z / np.float64(f(K[1]))), z], axis=1).astype(f)
    inv = f(1.0) / f(0.1)
    lo = np.floor(P.min(axis=0) * inv).astype(np.int64); hi = np.floor(P.max(axis=0) * inv).astype(np.int64)
    return int(np.prod(hi - lo + 1)), (hi - lo + 1).tolist()


@pytest.fixture(scope="module")
def pc_cases(orc, synth):
    S = pc_build(orc, synth)
    seen = dict(valid=0, gate_fail=0, gated_invalid=0, flipped=0, kept=0)
    for name, c in S.items():
        K = c.get("K", K0)
        kw = dict(fx=K[0], fy=K[1], cx=K[2], cy=K[3], depth_factor=c.get("depth_factor"), dist_th=DIST_TH)
        po, co = orc.plane_clouds(c["depth"], c["labels"], c["planes"], **kw)
        c["oracle"] = (po, co); c["kw"] = kw
        seen["valid"] += int((po["valid"] == 1).sum()); seen["gate_fail"] += int(((po["gate_ok"] == 0) & (po["n_points"] > 0)).sum())
        seen["gated_invalid"] += int(((po["gate_ok"] == 1) & (po["valid"] == 0)).sum())
        for k in np.nonzero(po["valid"] == 1)[0]:                     # the sign rule: the oracle's coefficients against the unflipped refit of the same points
            _, nc = orc.sac_plane(co[po["first"][k]: po["first"][k] + po["n_points"][k]], DIST_TH)
            assert nc[3] != 0 and (np.array_equal(po["coef"][k], nc) or np.array_equal(po["coef"][k], -nc))
            c.setdefault("flipped", {})[int(k)] = bool(np.array_equal(po["coef"][k], -nc))
            seen["flipped" if c["flipped"][int(k)] else "kept"] += 1
    # (a)
    po, co = S["a_tiny"]["oracle"]
    assert po["n_pixels"][:6].tolist() == [160 * 60 - 5, 0, 1, 2, 3, 160 * 60 - 1] and (po["n_pixels"][6:] == 0).all()
    assert po["n_points"][1:5].tolist() == [0, 1, 2, 3] and po["gate_ok"][:6].tolist() == [1, 0, 1, 1, 1, 1] and po["valid"][:6].tolist() == [1, 0, 0, 0, 1, 1]
    assert po["first"][2] == po["first"][1] == po["n_points"][0] and po["n_inliers"][4] == 3
    # (b)
    po, _ = S["b_row_strip"]["oracle"]; assert po["n_points"][1] >= 5 and po["gate_ok"][1] == 1
    po, co = S["b_exact_strip"]["oracle"]
    strip = co[po["first"][1]: po["first"][1] + po["n_points"][1]]
    assert len(strip) >= 5 and len(np.unique(strip[:, 1])) == 1 and len(np.unique(strip[:, 2])) == 1
    assert po["gate_ok"][1] == 1 and po["valid"][1] == 0 and po["valid"][0] == 1
    # (c)
    po, _ = S["c_three_four"]["oracle"]
    assert po["n_points"].tolist()[1:] == [3, 4] and po["n_inliers"].tolist()[1:] == [3, 4] and po["valid"].tolist() == [1, 1, 1]
    # (d)
    po, _ = S["d_gate"]["oracle"]; p0, _ = S["d_plain"]["oracle"]
    assert po["gate_ok"].tolist() == [0, 1] and po["valid"].tolist() == [0, 1] and p0["valid"].tolist() == [1, 1] and po[1].tobytes() == p0[1].tobytes()
    # (e) the negated records flip where the plain ones do not, and the other way round
    assert S["d_plain"]["flipped"] == {k: not v for k, v in S["e_negated"]["flipped"].items()} and len(S["d_plain"]["flipped"]) == 2
    assert np.array_equal(S["e_negated"]["oracle"][0]["coef"], -p0["coef"])
    # (f)
    assert S["f_sprinkled"]["oracle"][0].tobytes() == S["f_minus_one"]["oracle"][0].tobytes() and (S["f_sprinkled"]["oracle"][0]["n_pixels"] < p0["n_pixels"]).all()
    # (g)
    po, _ = S["g_64"]["oracle"]; assert (po["n_pixels"] == 1200).all() and (po["valid"] == 1).all() and (np.diff(po["first"]) == po["n_points"][:-1]).all()
    # (h)
    po, _ = S["h_mm"]["oracle"]; assert po["valid"].tolist() == [1, 1]
    c = S["h_overflow"]; po, co = c["oracle"]
    c["cells"], ext = floor_cells(c)
    print("h_overflow: the floor's voxel box is %s = %d cells, %.2f x the table's 2^18" % (ext, c["cells"], c["cells"] / 2.0 ** 18))
    assert c["cells"] > 2 ** 18 and po["valid"][0] == 1 and po["n_points"][1] > 1000 and c["depth"].max() <= 60000
    # (i) a capacity inside plane 1's slice
    po, co = S["d_plain"]["oracle"]
    cap = int(po["first"][1] + po["n_points"][1] // 2)
    c = dict(S["d_plain"]); c["cap"] = cap; c["oracle"] = orc.plane_clouds(c["depth"], c["labels"], c["planes"], cap=cap, **c["kw"])
    pi, ci = c["oracle"]
    assert pi["valid"].tolist() == [1, 0] and pi["gate_ok"].tolist() == [1, 1] and len(ci) == cap and pi[0].tobytes() == po[0].tobytes() and np.array_equal(ci, co[:cap])
    S["i_small_cap"] = c
    assert seen["valid"] >= 1 and seen["gate_fail"] >= 1 and seen["gated_invalid"] >= 1 and seen["flipped"] >= 1 and seen["kept"] >= 1, seen
    return S


@pytest.fixture(scope="module")
def mm_ctx(hvo, pc_cases):
    K = pc_cases["h_mm"]["K"]
    ctx = hvo.Context(fx=K[0], fy=K[1], cx=K[2], cy=K[3], depth_map_factor=pc_cases["h_mm"]["depth_factor"])
    yield ctx
    ctx.close()


def run_pc(hvo, ctx, c, **kw):
    return abi.plane_clouds(hvo, ctx, c["depth"], c["labels"], c["planes"], dist_th=DIST_TH, **kw)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["a_tiny", "b_row_strip", "b_exact_strip", "c_three_four", "d_plain", "d_gate", "e_negated", "f_sprinkled", "g_64"])
def test_plane_clouds_on_hand_made_labels(hvo, gpu_ctx, pc_cases, name):
    """(a) tiny and empty planes among 64 records, (b) thin strips -- the exactly collinear one draws 50 degenerate models (a zero cross
    product, NaN coefficients, no inlier) and ends without a plane: pcl's `collinear` branch of computeModelCoefficients (st == 2 in
    k_pc_refit) cannot be reached, because isSampleGood rejects the same triples by the same comparison first --, (c) 3 and 4 voxel
    points, (d) a gate failure, (e) negated normals, (f) labels outside [0, n_planes), (g) 64 planes"""
    c = pc_cases[name]
    rc, pg, cg, n = run_pc(hvo, gpu_ctx, c)
    assert rc == abi.OK
    check_plane_clouds(pg, cg, n, *c["oracle"])
    for k, flipped in c.get("flipped", {}).items():                   # the coefficient signs follow the oracle's sign rule
        assert np.array_equal(np.sign(pg["coef"][k][3]), np.sign(c["oracle"][0]["coef"][k][3]))


@pytest.mark.gpu
def test_plane_clouds_ignored_labels_and_plane_count(hvo, gpu_ctx, orc, pc_cases):
    """labels below 0 or at and above n_planes count as no plane: the same bytes as with -1 in their place; 65 planes are refused"""
    a = run_pc(hvo, gpu_ctx, pc_cases["f_sprinkled"]); b = run_pc(hvo, gpu_ctx, pc_cases["f_minus_one"])
    assert a[0] == b[0] == abi.OK and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes() and a[3] == b[3]
    c = pc_cases["g_64"]
    rc, pg, cg, n = abi.plane_clouds(hvo, gpu_ctx, c["depth"], c["labels"], np.concatenate([c["planes"], c["planes"][:1]]), n_planes=65)
    assert rc == abi.INVALID_ARG and n <= 0 and not pg.view(np.uint8).any()


@pytest.mark.gpu
def test_plane_clouds_millimetre_depth_and_table_overflow(hvo, mm_ctx, pc_cases):
    """depth_map_factor 1/1000 and the intrinsics of a 320 x 240 camera: parity; a floor out to 60 m needs more voxel cells than the
    table has (the count is printed by the fixture): HVO_ERR_CAPACITY, the plane before it equals the oracle's (which has no such limit),
    the floor itself comes back empty and the plane after it is still processed"""
    c = pc_cases["h_mm"]
    rc, pg, cg, n = run_pc(hvo, mm_ctx, c)
    assert rc == abi.OK
    check_plane_clouds(pg, cg, n, *c["oracle"])
    c = pc_cases["h_overflow"]; po, co = c["oracle"]
    rc, pg, cg, n = run_pc(hvo, mm_ctx, c)
    assert rc == abi.CAPACITY
    check_plane_clouds(pg, cg, n, po, co, upto=1)
    assert pg["n_points"][1] == 0 and pg["valid"][1] == 0 and pg["gate_ok"][1] == 0
    assert pg["n_pixels"][2] == po["n_pixels"][2] and pg["n_points"][2] == po["n_points"][2] and pg["valid"][2] == po["valid"][2] == 1
    assert pg["first"][2] == pg["n_points"][0] and n == pg["n_points"][0] + pg["n_points"][2]
    assert np.array_equal(cg[pg["first"][2]:], co[po["first"][2]:]) and np.allclose(pg["coef"][2], po["coef"][2], rtol=0, atol=1e-5)


@pytest.mark.gpu
def test_plane_clouds_small_cap(hvo, gpu_ctx, pc_cases):
    """a caller capacity inside the second plane's slice: HVO_ERR_CAPACITY, the true total, the first `cap` rows, the first plane refit as
    with a large capacity, the cut plane not refit"""
    c = pc_cases["i_small_cap"]; po, co = c["oracle"]; full, _ = pc_cases["d_plain"]["oracle"]
    rc, pg, cg, n = run_pc(hvo, gpu_ctx, c, cap=c["cap"])
    assert rc == abi.CAPACITY and n == int(full["n_points"].sum()) and len(cg) == c["cap"]
    check_plane_clouds(pg, cg, int(po["n_points"].sum()), po, co[: c["cap"]], upto=None)
    rc, pf, cf, _ = run_pc(hvo, gpu_ctx, pc_cases["d_plain"])
    assert rc == abi.OK and pg[0].tobytes() == pf[0].tobytes() and np.array_equal(cg, cf[: c["cap"]])
    rc, pg, cg, n = run_pc(hvo, gpu_ctx, c, cap=0)
    assert rc == abi.INVALID_ARG


# ====================================================================================================== 4. 3-D lines and LPVO over geometry
L3_GEOMS = [(480, 335), (397, 501), (240, 322), (960, 1280)]


@pytest.fixture(scope="module")
def l3_cases(orc, synth):
    cases = {}
    for h, w in L3_GEOMS:
        Kd = synth.intrinsics(w, h); K = tuple(float(np.float32(Kd[k])) for k in ("fx", "fy", "cx", "cy"))
        d = plane_depth((0.2, -0.1, 1.0), 2.0, w, h, K)
        d[h // 5: h // 5 + h // 12, :] = 0
        d[:, (5 * w) // 8:] = plane_depth((0.0, 0.1, 1.0), 3.1, w, h, K)[:, (5 * w) // 8:]
        n = 300
        kl = random_keylines(orc, w, h, n + 2, 9 + w)
        # two hand-made lines: Frame::isLineGood drops a sample whose ROW >= the image WIDTH or whose COLUMN >= the image HEIGHT (sic,
        # src/Frame.cc:1249): line n lies where that test drops everything (or, for the square-free control, nowhere), line n + 1 where it cannot
        m = min(w, h)
        if w < h:
            kl[n]["sx"], kl[n]["sy"], kl[n]["ex"], kl[n]["ey"] = 20.3, w + 10.4, w - 20.6, h - 10.2          # rows >= w
        else:
            kl[n]["sx"], kl[n]["sy"], kl[n]["ex"], kl[n]["ey"] = h + 10.3, h * 0.5 + 0.4, w - 10.6, h * 0.8 + 0.2    # columns >= h
        kl[n + 1]["sx"], kl[n + 1]["sy"], kl[n + 1]["ex"], kl[n + 1]["ey"] = 10.3, m * 0.5 + 0.4, m * 0.55 + 0.6, m * 0.8 + 0.2
        o = orc.lines_3d(kl, d, seed=5, fx=K[0], fy=K[1], cx=K[2], cy=K[3])
        assert 5 < o["good"][:n].sum() < n, (h, w, o["good"].sum())
        assert o["n_samples"][n] == 0 and o["good"][n] == 0 and o["n_samples"][n + 1] == 21 and o["good"][n + 1] == 1, (h, w, o[n:])
        cases[(h, w)] = dict(K=K, depth=d, kl=kl, oracle=o)
    return cases


@pytest.mark.gpu
@pytest.mark.parametrize("h,w", L3_GEOMS)
def test_lines_3d_over_geometry(hvo, l3_cases, h, w):
    c = l3_cases[(h, w)]; K = c["K"]
    ctx = hvo.Context(fx=K[0], fy=K[1], cx=K[2], cy=K[3])
    try:
        rc, r = abi.lines_3d(hvo, ctx, c["kl"], c["depth"], seed=5)
    finally:
        ctx.close()
    o = c["oracle"]
    assert rc == abi.OK and r.tobytes() == o.tobytes(), [f for f in o.dtype.names if not np.array_equal(r[f], o[f])]


#  h, w: 12 + 15 k puts the last sample of range(10, size - 1, 15) at size - 2; one less leaves size - 1 just past a sample
LPVO_GEOMS = [(237, 312), (236, 311), (237, 311), (236, 312)]


@pytest.fixture(scope="module")
def lpvo_cases(orc, synth):
    cases = {}
    for h, w in LPVO_GEOMS:
        us = list(range(10, w - 1, 15)); vs = list(range(10, h - 1, 15))
        assert us[-1] == (w - 2 if w == 312 else w - 16) and vs[-1] == (h - 2 if h == 237 else h - 16)
        d = plane_depth((0.1, 0.2, 1.0), 3.0, w, h)
        o = orc.normals_lpvo(d)
        assert len(o[0]) == len(us) * len(vs) and o[2][-1].tolist() == [us[-1], vs[-1]]
        d2 = synth.make_depth(0x5EED3201, w, h)
        o2 = orc.normals_lpvo(d2)
        assert 50 < len(o2[0]) < len(us) * len(vs)
        cases[(h, w)] = [(d, o), (d2, o2)]
    d = synth.make_depth(0x5EED3202, 501, 397)
    o = orc.normals_lpvo(d)
    assert len(o[0]) > 300
    cases[(397, 501)] = [(d, o)]
    return cases


@pytest.mark.gpu
@pytest.mark.parametrize("h,w", LPVO_GEOMS + [(397, 501)])
def test_lpvo_over_geometry(hvo, gpu_ctx, lpvo_cases, h, w):
    for d, (no, zo, po) in lpvo_cases[(h, w)]:
        rc, ng, zg, pg = abi.normals_lpvo(hvo, gpu_ctx, d)
        assert rc == abi.OK and np.array_equal(pg, po)
        assert ng.tobytes() == no.tobytes() and zg.tobytes() == zo.tobytes()


def test_preconditions_hold_without_a_gpu(sn_cases, stride_cases, pc_cases, l3_cases, lpvo_cases):
    """the fixtures above run every input through the oracle and assert what makes it non-vacuous; nothing here touches a device"""
    assert len(sn_cases) == len(SN_GEOMS) and len(l3_cases) == len(L3_GEOMS) and len(lpvo_cases) == len(LPVO_GEOMS) + 1
    assert {"a_tiny", "b_row_strip", "b_exact_strip", "c_three_four", "d_gate", "e_negated", "f_sprinkled", "g_64", "h_mm", "h_overflow", "i_small_cap"} <= set(pc_cases)


# ====================================================================================================== 5. the resident paths at 501 x 397
RW, RH = 501, 397
FULL_TAIL = 1 | 2 | 4 | 16 | 32 | 64 | 128          # ORB, LSD, planes, 3-D lines, vanishing points, plane tail, grids


@pytest.mark.gpu
def test_stream_tail_at_501_by_397(hvo, orc, synth):
    """two frames through hvo_stream_* at a geometry whose resident depth pitch (512) differs from the width, and whose int8 label image is
    no multiple of anything: every tail field against the oracle"""
    from test_tail_gpu import check_tail
    seed = 21
    st = hvo.Stream(width=RW, height=RH, depth=2, stages=FULL_TAIL, bf=40.0, seed=seed)
    try:
        assert st.bounds.tolist() == [0.0, float(RW), 0.0, float(RH)]
        for i in range(2):
            g, d = synth.make_frame("std", 0x5EED3300 + i, RW, RH)
            t = st.submit(g, d)
            r = st.collect(t)
            assert r["status"] == 0 and len(r["kl"]) > 5 and len(r["planes"]) >= 2 and r["plane_clouds"]["valid"].sum() >= 1
            check_tail(r, d, orc, seed + t, (0.0, float(RW), 0.0, float(RH)))
    finally:
        st.close()


@pytest.mark.gpu
def test_batch_tail_at_501_by_397(hvo, orc, synth):
    from test_tail_gpu import check_tail
    g, d = synth.make_batch("std", 0x5EED3310, 3, w=RW, h=RH)
    ctx = hvo.Context(max_batch=3)
    try:
        ctx.batch_upload(g, d)
        ctx.set_tail_params(seed=9)
        ctx.batch_run(FULL_TAIL)
        res = ctx.batch_download(hvo.STAGE_ALL)
        ctx.batch_download_tail(FULL_TAIL, res)
        for f, r in enumerate(res):
            assert len(r["kl"]) > 5 and len(r["planes"]) >= 2 and r["plane_clouds"]["valid"].sum() >= 1
            check_tail(r, d[f], orc, 9 + f, (0.0, float(RW), 0.0, float(RH)))
    finally:
        ctx.close()
