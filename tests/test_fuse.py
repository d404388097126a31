"""CPU checks of the restatement the GPU tests of Fuse compare against (tests/fuse_ref.py): the names the feature adds, hand-computed known
answers of ORBmatcher::Fuse(pKF, vpMapPoints, th) (reference src/ORBmatcher.cc:838-994) under a pose whose arithmetic is exact, and that
the random scenes the GPU tests run are not vacuous.  No GPU call."""
import os
import re
import subprocess
import sys

import numpy as np

import fuse_ref as ref
import point_map_ref as pm
from conftest import ROOT, PKG_DIR

F32 = np.float32
NEW = ["hvo_fuse_points", "hvo_fuse_points_slots", "hvo_stream_fuse_points"]
B4 = pm.BOUNDS


def run(kf, mp, cam=ref.CAM2, **kw):
    return ref.fuse(kf, mp, cam, B4, **kw)


def test_the_header_and_the_binding_name_the_new_calls(hvo):
    hdr = open(os.path.join(ROOT, "include", "hvo.h")).read()
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert n in hvo.EXPORTS, n
    for t in ("hvo_fuse_keyframe", "hvo_fuse_map", "hvo_fuse_params", "hvo_fuse_result"):
        assert re.search(r"}\s*%s;" % t, hdr), t
    assert "#define HVO_ABI_VERSION 3 " in hdr
    for i, name in enumerate(("SEARCHED", "SKIP", "BEHIND", "OUT_OF_IMAGE", "DIST_MIN", "DIST_MAX", "VIEW_ANGLE")):
        assert re.search(r"#define HVO_FUSE_GATE_%s\s+%d\b" % (name, i), hdr), name
    assert hasattr(hvo.Context, "fuse_points") and hasattr(hvo.Context, "fuse_points_slots") and hasattr(hvo.Stream, "fuse_points")
    assert (hvo.FUSE_MAX_FEATURES, hvo.FUSE_MAX_ENTRIES) == (ref.MAX_FEATURES, ref.MAX_ENTRIES) and tuple(hvo.FUSE_GATES) == ref.GATES
    hpp = open(os.path.join(ROOT, "include", "hvo.hpp")).read()
    assert "hvo_fuse_points(" in hpp and "hvo_stream_fuse_points(" in hpp


def test_the_example_compiles_and_links():
    """examples/fuse_neighbors.cpp against libhvo.so (it runs in tests/test_fuse_gpu.py)"""
    csrc = os.path.join(PKG_DIR, "csrc")
    assert os.path.exists(os.path.join(csrc, "libhvo.so"))
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-O1", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "fuse_neighbors.cpp"),
                               "-L" + csrc, "-lhvo", "-Wl,-rpath," + csrc, "-o", os.path.join(d, "fuse_neighbors")])


def test_every_gate_alone():
    """each crafted row gives its gate, its projection as far as the reference computed it, and a level exactly where it was searched"""
    rows = ref.crafted_gates()
    mp, skip = ref.rows_map(rows)
    kf = dict(kp_un=np.zeros(0, _kp_dt()), uright=None, desc=np.zeros((0, 32), np.uint8), Tcw=ref.T_CRAFTED, skip=skip)
    w = run(kf, mp)
    seen = set()
    for i, (name, _, _, _, _, _, g, p3, lvl) in enumerate(rows):
        assert w["gate"][i] == g, (name, ref.GATES[w["gate"][i]])
        assert (w["level"][i] >= 0) == (g == 0), name
        assert w["best_idx"][i] == -1 and w["best_dist"][i] == 256           # no feature: searched entries find nothing
        if lvl is not None: assert w["level"][i] == lvl, (name, w["level"][i])
        if p3 is not None:
            for k in range(3):
                if p3[k] is not None: assert w["proj"][i, k] == F32(p3[k]), (name, k, w["proj"][i])
        seen.add(g)
    assert seen == set(range(7))
    names = [r[0] for r in rows]
    i = names.index("z = 0: NaN projection fails IsInImage")
    assert np.isnan(w["proj"][i, 0]) and np.isnan(w["proj"][i, 1]) and w["proj"][i, 2] == 0
    i = names.index("NaN position")
    assert np.isnan(w["proj"][i, :2]).all() and w["gate"][i] == ref.OUT_OF_IMAGE
    assert w["n_searched"] == sum(1 for r in rows if r[6] == 0) and w["n_fused"] == 0 and len(w["fused_entry"]) == 0


def _kp_dt(hvo=None):
    return np.dtype([("x", F32), ("y", F32), ("size", F32), ("angle", F32), ("response", F32), ("octave", np.int32), ("class_id", np.int32)])


def test_level_band_at_both_ends_and_at_the_clamp():
    """an entry of level 3 takes octaves 2 and 3 only; an entry of level 0 takes octave 0 only (the band [-1, 0] has no feature at -1); an entry
    whose level is clamped to 7 takes 6 and 7"""
    dt = _kp_dt()
    for level, octaves, want in ((3, (1, 2, 3, 4), (False, True, True, False)), (0, (0, 1), (True, False)), (7, (5, 6, 7), (False, True, True))):
        for o, ok in zip(octaves, want):
            kf, mp = ref.hand_scene(dt, [(300.0, 200.0, ref.BASE)], [(300.5, 200.0, o, ref.flip(4))], uright=False, level=level)
            if level == 7: mp["max_dist"][0] = F32(mp["max_dist"][0] * 1.2 ** 20)       # far past the top: PredictScale clamps
            w = run(kf, mp)
            assert w["level"][0] == level and (w["best_idx"][0] == 0) == ok, (level, o, w["best_idx"][0])
            assert w["best_dist"][0] == (4 if ok else 256)
    kf, mp = ref.hand_scene(dt, [(300.0, 200.0, ref.BASE)], [(300.5, 200.0, -1, ref.flip(4))], uright=False, level=0)
    assert run(kf, mp)["best_idx"][0] == -1                                              # a negative octave is in no band


def test_chi_square_gates_one_float_step_either_side():
    kf, mp, want = ref.chi2_cases(_kp_dt())
    w = run(kf, mp)
    assert (w["gate"] == 0).all() and (w["level"] == 0).all()
    assert [int(b) for b in w["best_idx"]] == [k if ok else -1 for k, ok in enumerate(want)], w["best_idx"]
    assert want == [True, False, True, False, True]
    # each is one float step from the other side: e2 of the accepted ones with the coordinate one step further is above the literal, and
    # e2 of the refused ones one step nearer is not
    sq = lambda c, a: float(F32(F32(F32(c) - a) * F32(F32(c) - a)))
    x = kf["kp_un"]["x"]; r = kf["uright"]; u = [64.0 + 96.0 * k for k in range(5)]
    assert sq(u[0], x[0]) <= 5.99 < sq(u[0], np.nextafter(x[0], F32(-np.inf))) and sq(u[1], np.nextafter(x[1], F32(np.inf))) <= 5.99 < sq(u[1], x[1])
    assert sq(u[2] - 32, r[2]) <= 7.8 < sq(u[2] - 32, np.nextafter(r[2], F32(-np.inf))) and sq(u[3] - 32, np.nextafter(r[3], F32(np.inf))) <= 7.8 < sq(u[3] - 32, r[3])
    assert 5.99 < sq(u[4], x[4]) <= 7.8 and r[4] == F32(u[4] - 32)
    # uright = NULL: every feature takes the mono gate: the stereo pair (e2 = 0 without er) passes, the mono pair is unchanged, and the
    # fifth (e2 just above 5.99, accepted by the stereo gate before) is refused
    w = run(dict(kf, uright=None), mp)
    assert [int(b) for b in w["best_idx"]] == [0, -1, 2, 3, -1]


def test_ties_follow_the_visiting_order():
    kf, mp = ref.tie_cases(_kp_dt())
    w = run(kf, mp)
    assert w["best_idx"].tolist() == [1, 2, -1] and w["best_dist"].tolist() == [9, 9, 256], (w["best_idx"], w["best_dist"])
    assert w["n_ties"].tolist() == [2, 2, 0] and (w["gate"] == 0).all()
    grid, _, _ = pm.build_grid(kf["kp_un"], B4)
    assert grid[(21, 20)] == [0] and grid[(20, 20)] == [1] and grid[(40, 20)] == [2, 3] and all(4 not in v for v in grid.values())
    assert w["fused_entry"].tolist() == [0, 1] and w["fused_idx"].tolist() == [1, 2] and w["n_fused"] == 2


def test_th_low_is_inclusive():
    dt = _kp_dt()
    ent = [(100.0, 100.0, ref.BASE), (300.0, 100.0, ref.BASE), (500.0, 100.0, ref.BASE)]
    kf, mp = ref.hand_scene(dt, ent, [(101.0, 100.0, 1, ref.flip(50)), (301.0, 100.0, 1, ref.flip(51)), (501.0, 100.0, 1, ref.flip(256))], uright=False)
    w = run(kf, mp)
    assert w["best_idx"].tolist() == [0, 1, -1] and w["best_dist"].tolist() == [50, 51, 256]     # the complement (256) never enters bestDist
    assert w["fused_entry"].tolist() == [0] and w["fused_idx"].tolist() == [0] and w["n_fused"] == 1
    assert run(kf, mp, th_low=51)["fused_entry"].tolist() == [0, 1]


def test_the_random_scene_is_not_vacuous():
    """seed fuse_ref.SCENE_SEED: at least a quarter of the entries fused, every gate code present, an entry with several candidates at the
    best distance -- on the restatement alone; tests/test_fuse_gpu.py compares the device with the same output"""
    kf, mp = ref.random_scene(_kp_dt(), 1000, 1500)
    w = ref.fuse(kf, mp, pm.CAM)
    ref.vacuity(w, 1500)
    assert (w["n_cand"] > 1).sum() > 50
    kf, mp = ref.random_scene(_kp_dt(), 200, 257, seed=ref.SCENE_SEED + 3, crowd=200)
    w = ref.fuse(kf, mp, pm.CAM)
    assert w["n_cand"].max() >= 8 and w["n_fused"] * 4 >= 257


def test_the_ragged_key_frames_say_something(hvo):
    """fuse_ref.ragged_keyframes, on the restatement: an empty key frame and an empty map side inside the list give empty answers, the others
    fuse, the monocular key frame among them; against the shared map side the key frame whose features made it fuses most of it"""
    kfs, maps, shared_kfs, shared = ref.ragged_keyframes(hvo.KEYPOINT_DT)
    assert [(len(k["kp_un"]), len(m["pos"])) for k, m in zip(kfs, maps)] == list(ref.RAGGED) == [(65, 257), (0, 40), (300, 0), (64, 17)]
    assert kfs[2]["uright"] is None and kfs[1]["skip"] is None and all(k["uright"] is not None for j, k in enumerate(kfs) if j != 2)
    w = [ref.fuse(kf, mp, pm.CAM) for kf, mp in zip(kfs, maps)]
    assert w[0]["n_fused"] > 40 and w[3]["n_fused"] > 3 and w[0]["n_searched"] > w[0]["n_fused"]
    assert w[1]["n_fused"] == 0 and w[1]["n_searched"] == 40 and (w[1]["best_idx"] == -1).all()        # searched, and no feature to find
    assert w[2]["n_fused"] == w[2]["n_searched"] == 0 and len(w[2]["best_idx"]) == 0
    ws = [ref.fuse(kf, shared, pm.CAM) for kf in shared_kfs]
    assert len(shared["pos"]) == 257 and ws[2]["n_fused"] > 40 and ws[1]["n_fused"] == 0 and ws[1]["n_searched"] > 100
    assert all(kf["skip"] is None or len(kf["skip"]) == 257 for kf in shared_kfs)


def test_the_host_restatement_agrees(tmp_path):
    """tools/fuse_host.cpp, the single-thread host restatement the timing tool measures beside the device, gives fuse_ref's answer"""
    exe = str(tmp_path / "fuse_host")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-ffp-contract=off", "-Wall", "-Werror", os.path.join(ROOT, "tools", "fuse_host.cpp"), "-o", exe])
    kf, mp = ref.random_scene(_kp_dt(), 300, 400, seed=ref.SCENE_SEED + 5)
    w = ref.fuse(kf, mp, pm.CAM)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import fuse_host_io as io
    finally:
        sys.path.pop(0)
    got = io.run(exe, str(tmp_path), [kf], mp, pm.CAM, B4, pm.SF, ref.INV_SIGMA2, ref.TH, ref.TH_LOW, pm.LOG_SF, pm.N_LEVELS)[0]
    assert np.array_equal(got["best_idx"], w["best_idx"]) and np.array_equal(got["best_dist"], w["best_dist"]) and np.array_equal(got["gate"], w["gate"])
