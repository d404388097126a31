"""The restatement tests/map_refresh_ref.py on crafted cases, the accuracy of its float sum, the Python binding's refusals and the host tool,
on the CPU.  tests/test_map_refresh_gpu.py compares the device with the restatement bit for bit."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import map_refresh_ref as ref
from conftest import ROOT

F32 = np.float32
NEW = ["hvo_refresh_map_points", "hvo_refresh_map_lines", "hvo_point_map_refresh", "hvo_line_map_refresh"]
_cache = {}


def scene(which):
    if which not in _cache:
        pos, obs = ref.random_scene(**which_args(which))
        _cache[which] = (pos, obs, (ref.refresh_lines if which == "lines" else ref.refresh_points)(pos, obs))
    return _cache[which]


def which_args(which):
    return ref.SCENE_LINES if which == "lines" else ref.SCENE_POINTS


def one(values, bad=None, **kw):
    """one point observed by len(values) key frames whose descriptors lie on a line"""
    n = len(values)
    obs = dict(obs_start=[0, n], obs_desc=ref.on_a_line(values), obs_Ow=np.zeros((n, 3), F32), kf_bad=bad, ref_Ow=np.zeros((1, 3), F32), ref_level=[0], skip=None)
    return ref.refresh_points(np.array([[0, 0, 2]], F32), obs, **kw)


def test_exports(hvo):
    assert all(n in hvo.EXPORTS for n in NEW)
    for n in ("refresh_map_points", "refresh_map_lines"): assert callable(getattr(hvo.Context, n))
    assert callable(hvo.PointMap.refresh) and callable(hvo.LineMap.refresh)
    assert (hvo.MR_DESCRIPTOR, hvo.MR_GEOMETRY, hvo.MR_MAX_OBS, hvo.MR_MAX_FEATURES, hvo.MR_MAX_OBS_TOTAL) == (ref.DESCRIPTOR, ref.GEOMETRY, ref.MAX_OBS, ref.MAX_FEATURES, ref.MAX_OBS_TOTAL)
    assert hvo.MR_UNTOUCHED == ref.UNTOUCHED and len(hvo.MR_STATUS) == 5
    hdr = open(os.path.join(ROOT, "include", "hvo.h")).read()
    for n in NEW: assert n + "(" in hdr, n
    assert "#define HVO_ABI_VERSION 3 " in hdr


def test_example_compiles():
    """examples/map_refresh.cpp against the C++ mirror (it runs in tests/test_map_refresh_gpu.py)"""
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx: pytest.skip("no host compiler")
    subprocess.check_call([cxx, "-std=c++14", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-fsyntax-only", os.path.join(ROOT, "examples", "map_refresh.cpp")])


def test_the_median_rank():
    assert [ref.rank(N) for N in (1, 2, 3, 4)] == [0, 0, 1, 1]
    assert all(ref.rank(N) == (N - 1) // 2 for N in range(1, 258))


def test_crafted_medians():
    assert [int(x) for x in ref.distance_matrix(ref.on_a_line([0, 5, 20]))[0]] == [0, 5, 20]
    # N = 1: the only row; N = 2: rank 0 is the self-distance of either row, the first wins
    for values, best, median in (([7], 0, 0), ([7, 100], 0, 0),
                                 ([0, 10, 20], 0, 10),             # rank 1 of [0 10 20], [0 10 10], [0 10 20]: all 10, the first is kept
                                 ([0, 50, 60], 1, 10),             # [0 50 60], [0 10 50], [0 10 60]: rows 1 and 2 tie at 10
                                 ([0, 5, 20, 21], 2, 1),           # rank 1 of four: 5, 5, 1, 1
                                 ([30, 0, 29, 31], 0, 1),          # 1, 29, 1, 1: rows 0, 2 and 3 tie
                                 ([9, 9, 9, 9, 9], 0, 0)):         # all identical
        r = one(values)
        assert (r["best_obs"][0], r["best_median"][0], r["status"][0]) == (best, median, ref.REFRESHED), (values, r["best_obs"], r["best_median"])
        assert np.array_equal(r["desc"][0], ref.bits(values[best]))
    assert one([0, 10, 20])["tie"][0] and not one([0, 10, 21, 50, 51])["tie"][0] and not one([7])["tie"][0]


def test_a_bad_observer_leaves_the_matrix_and_stays_in_the_normal():
    values = [0, 50, 60]
    n = len(values)
    Ow = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 0]], F32)
    obs = dict(obs_start=[0, n], obs_desc=ref.on_a_line(values), obs_Ow=Ow, kf_bad=[0, 1, 0], ref_Ow=np.zeros((1, 3), F32), ref_level=[2], skip=None)
    P = np.array([[0, 0, 2]], F32)
    r = ref.refresh_points(P, obs)
    assert (r["best_obs"][0], r["best_median"][0]) == (0, 0)                 # rows 0 and 2 are left: N = 2, rank 0; the index counts the bad one
    obs_all = dict(obs, kf_bad=None)
    assert ref.refresh_points(P, obs_all)["best_obs"][0] == 1
    assert np.array_equal(r["normal"], ref.refresh_points(P, obs_all)["normal"])
    two = dict(obs, obs_start=[0, 2], obs_desc=obs["obs_desc"][[0, 2]], obs_Ow=Ow[[0, 2]], kf_bad=None)
    assert not np.array_equal(r["normal"], ref.refresh_points(P, two)["normal"])
    assert r["max_dist"][0] == F32(2) * ref.pm.SF[2] and r["min_dist"][0] == r["max_dist"][0] / ref.pm.SF[7]


def test_every_status_code_and_what_it_leaves():
    U = ref.UNTOUCHED
    d = ref.on_a_line([3, 4])
    obs = dict(obs_start=[0, 2, 2, 4, 6, 8, 10], obs_desc=np.concatenate([d] * 5), obs_Ow=np.ones((10, 3), F32), kf_bad=[0, 0, 0, 0, 1, 1, 0, 0, 1, 1],
               ref_Ow=np.zeros((6, 3), F32), ref_level=[0, 0, 0, 0, 8, -1], skip=[0, 0, 1, 0, 0, 0])
    pos = np.tile(np.array([0, 0, 2], F32), (6, 1))
    r = ref.refresh_points(pos, obs)
    assert r["status"].tolist() == [ref.REFRESHED, ref.NO_OBS, ref.SKIPPED, ref.DESC_KEPT, ref.BAD_LEVEL, ref.DESC_KEPT]
    assert r["best_obs"].tolist() == [0, -1, -1, -1, 0, -1]
    assert [(r["desc"][f] == U).all() for f in range(6)] == [False, True, True, True, False, True]
    assert [(r["normal"][f] == U).all() for f in range(6)] == [False, True, True, False, False, False]
    assert [r["max_dist"][f] == U for f in range(6)] == [False, True, True, False, True, True]
    g = ref.refresh_points(pos, obs, what=ref.GEOMETRY)                      # without the descriptor half nobody's descriptor is kept or written
    assert g["status"].tolist() == [0, ref.NO_OBS, ref.SKIPPED, 0, ref.BAD_LEVEL, ref.BAD_LEVEL] and (g["desc"] == U).all() and (g["best_obs"] == -1).all()
    h = ref.refresh_points(pos, obs, what=ref.DESCRIPTOR)
    assert h["status"].tolist() == [0, ref.NO_OBS, ref.SKIPPED, ref.DESC_KEPT, 0, ref.DESC_KEPT] and (h["normal"] == U).all() and (h["max_dist"] == U).all()
    lp = np.tile(np.array([0, 0, 2, 0, 0, 2], np.float64), (6, 1))          # a zero-length line: the world vector stays zero
    l = ref.refresh_lines(lp, obs)
    assert l["status"].tolist() == r["status"].tolist() and (l["wvec"][0] == 0).all() and (l["wvec"][1] == U).all()


def test_the_line_readings():
    assert ref.world_vector([1, 2, 3, 1, 2, 1]) == [0.0, 0.0, 1.0] and ref.world_vector([1, 2, 3, 1, 2, 3]) == [0.0, 0.0, 0.0]
    assert ref.line_scale_factors(3, 1.2) == [1.0, float(F32(1.2)), float(F32(1.2) * F32(1.2))]
    # the midpoint for the distance is a float one: a coordinate beyond float precision moves it
    P = [1.0 + 2.0 ** -30, 0, 0, 1.0 + 2.0 ** -30, 0, 0]
    assert ref.line_dist(P, [0.0, 0.0, 0.0]) == 1.0
    assert ref.line_geometry([0, 0, 1, 0, 0, 3], [[0.0, 0.0, 0.0]]) == [0.0, 0.0, 1.0]


def test_point_normal_against_float64():
    """the float sum's error: every term is a unit vector's component rounded to float (2^-24 relative, and the reciprocal's and the
    product's roundings: at most 4 * 2^-24 absolute per term before the mean), and each of the n adds rounds a partial sum of magnitude at most
    k once; after the division by n that is within (n + 8) * 2^-24 per component for n <= 64"""
    rng = np.random.RandomState(5)
    worst = 0.0
    for n in (1, 2, 3, 7, 30, 64):
        for _ in range(20):
            P = ref.point_positions(1, rng)[0]; Ow = rng.uniform(-1.5, 1.5, (n, 3)).astype(F32)
            got = ref.point_geometry([float(v) for v in P], [[float(v) for v in O] for O in Ow])
            d = P.astype(np.float64)[None, :] - Ow.astype(np.float64)
            want = (d / np.linalg.norm(d, axis=1)[:, None]).sum(axis=0) / n
            err = np.abs(np.array(got) - want).max()
            worst = max(worst, err / ((n + 8) * 2.0 ** -24))
            assert err <= (n + 8) * 2.0 ** -24, (n, err)
    print("worst error / bound: %.3f" % worst)


@pytest.mark.parametrize("which", ["points", "lines"])
def test_random_scene_is_not_vacuous(which):
    pos, obs, r = scene(which)
    assert len(pos) == which_args(which)["n"]
    assert sorted(set(r["status"].tolist())) == [0, 1, 2, 3, 4]
    assert int(r["tie"].sum()) >= 20
    cnt = np.diff(obs["obs_start"])
    assert cnt.max() <= 40 and cnt.min() == 0 and obs["kf_bad"].sum() > 0


def test_binding_refuses_the_limits_without_a_device(hvo):
    for st in ([0, 257], [0, 3, 300], np.zeros(65538, np.int64), [0] + [256 * (i + 1) for i in range(4097)]):
        with pytest.raises(hvo.HvoError) as e:
            hvo.map_refresh_check(st)
        assert e.value.status == -4 if hasattr(e.value, "status") else "-4" in str(e.value)
    hvo.map_refresh_check([0, 256]); hvo.map_refresh_check([0]); hvo.map_refresh_check(np.arange(65537) * 16)


def test_host_tool_gives_the_same_answers(tmp_path):
    """tools/map_refresh_host.cpp, the single-thread loops that tools/map_refresh_timing.py times beside the device: bit for bit the
    restatement on both random scenes"""
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx: pytest.skip("no host compiler")
    exe = str(tmp_path / "map_refresh_host")
    subprocess.run([cxx, "-O2", "-std=c++17", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tools", "map_refresh_host.cpp")], check=True)
    for which in ("points", "lines"):
        pos, obs, r = scene(which)
        line = which == "lines"
        f = str(tmp_path / (which + ".bin"))
        n = len(pos)
        sf = np.array(ref.line_scale_factors(8, 1.2) if line else ref.pm.SF, F32)
        with open(f, "wb") as fh:
            np.array([1 if line else 0, n, int(obs["obs_start"][-1]), 8, 3], np.int32).tofile(fh)
            for a, dt in ((sf, F32), (obs["obs_start"], np.int32), (obs["obs_desc"], np.uint8), (obs["obs_Ow"], F32), (obs["kf_bad"], np.uint8), (obs["ref_Ow"], F32),
                          (obs["ref_level"], np.int32), (obs["skip"], np.uint8), (pos, np.float64 if line else F32)):
                np.ascontiguousarray(a, dt).tofile(fh)
        o = str(tmp_path / (which + ".out"))
        subprocess.run([exe, f, o, "1"], check=True, stdout=subprocess.DEVNULL)
        rdt = np.float64 if line else F32
        raw = open(o, "rb").read(); at = 0
        for k, dt, w in (("best_obs", np.int32, 1), ("best_median", np.int32, 1), ("desc", np.uint8, 32), ("normal", rdt, 3), ("wvec", np.float64, 3 if line else 0),
                         ("max_dist", F32, 1), ("min_dist", F32, 1), ("status", np.uint8, 1)):
            if w == 0: continue
            nb = n * w * np.dtype(dt).itemsize
            got = np.frombuffer(raw[at:at + nb], dt).reshape(r[k].shape); at += nb
            assert got.tobytes() == np.ascontiguousarray(r[k], dt).tobytes(), (which, k)
        assert at == len(raw)
