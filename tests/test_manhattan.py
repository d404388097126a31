"""Known answers of the CPU restatement of Tracking::TrackManhattanFrame (tests/manhattan_ref.py; reference src/Tracking.cc:1172-1348) on
crafted inputs.  No GPU."""
import math

import numpy as np

import manhattan_ref as ref

F32 = np.float32


def _pert(R, deg, axis=(1.0, 1.0, 0.0)):
    return (ref.rot(axis, deg) @ R).astype(F32)


def test_three_families_recovered():
    n, Rt = ref.three_families(seed=1)
    o = ref.track_manhattan(n, None, Rt.astype(F32))
    assert o["n_found"] == 3 and o["tracked"] == 1 and o["n_in_cone"] == [600, 600, 600]
    assert np.abs(o["R"] - Rt).max() < 1e-3
    # from a 3 degree error: axis 1 reads R_last as given and lands on the true axis in one call; axes 2 and 3 read the column axis 1
    # replaced (R_cm aliases R_cm_update), so one call halves the error and a tracker's chain of calls converges
    R0 = _pert(Rt, 3.0)
    o = ref.track_manhattan(n, None, R0)
    assert np.abs(o["axis_vec"][0] - Rt[:, 0]).max() < 1e-3
    e0 = np.abs(R0 - Rt).max(); e1 = np.abs(o["R"] - Rt).max()
    assert 0.4 * e0 < e1 < 0.6 * e0
    R = R0
    for _ in range(8):
        R = ref.track_manhattan(n, None, R)["R"]
    assert np.abs(R - Rt).max() < 1e-3
    assert abs(np.linalg.det(R.astype(np.float64)) - 1.0) < 1e-5


def test_axes_read_updated_columns():
    """the mean shift of axis 2 uses R_cm_update's new column 0 (shallow cv::Mat copy at Tracking.cc:1181)"""
    n, Rt = ref.three_families(seed=2)
    R0 = _pert(Rt, 3.0)
    o = ref.track_manhattan(n, None, R0)
    Rc = R0.copy(); Rc[:, 0] = o["axis_vec"][0]
    mn, ml = ref.cone_masks(R0, 2, n, np.zeros((0, 3)), np.zeros(0, bool))
    aliased = ref.mean_shift_axis(Rc, 2, n[mn], np.zeros((0, 3)), o["min_num_sn"])[0]
    fresh = ref.mean_shift_axis(R0, 2, n[mn], np.zeros((0, 3)), o["min_num_sn"])[0]
    assert np.array_equal(o["axis_vec"][1], aliased) and not np.array_equal(aliased, fresh)


def _two_axes(pair, R_true, seed=3):
    rng = np.random.RandomState(seed)
    parts = [ref.family(rng, R_true[:, c], 400, 0.5) for c in pair] + [ref.scatter(rng, 100, R_true)]
    return np.concatenate(parts).astype(F32)


def test_two_axes_each_pair_and_det_flip():
    for handed in (1.0, -1.0):
        Rt = ref.rot((0.3, 0.1, -0.6), 17.0); Rt[:, 2] *= handed            # right- and left-handed R_last
        for pair, missing in (((0, 1), 2), ((1, 2), 0), ((0, 2), 1)):
            n = _two_axes(pair, Rt)
            o = ref.track_manhattan(n, None, Rt.astype(F32))
            assert o["n_found"] == 2 and o["tracked"] == 1, (handed, pair)
            assert [o["found"][k] for k in range(3)] == [int(k in pair) for k in range(3)]
            # the code's cross product (v1 x v2, v3 x v2, v1 x v3), negated when the determinant is about -1
            u, v = {(0, 1): (0, 1), (1, 2): (2, 1), (0, 2): (0, 2)}[pair]
            c = np.cross(Rt[:, u], Rt[:, v])
            M = Rt.copy(); M[:, missing] = c
            flip = abs(np.linalg.det(M) + 1.0) < 0.5
            want = -c if flip else c
            assert np.abs(o["R"][:, missing] - want).max() < 1e-3, (handed, pair)
            assert np.abs(np.delete(o["R"], missing, 1) - np.delete(Rt, missing, 1)).max() < 1e-3
            assert np.linalg.det(o["R"].astype(np.float64)) > 0
    # both branches of the flip occur: right-handed (0, 2) flips, right-handed (0, 1) does not
    Rt = ref.rot((0.3, 0.1, -0.6), 17.0)
    assert abs(np.linalg.det(np.stack([Rt[:, 0], np.cross(Rt[:, 0], Rt[:, 2]), Rt[:, 2]], 1)) + 1) < 0.5
    assert abs(np.linalg.det(np.stack([Rt[:, 0], Rt[:, 1], np.cross(Rt[:, 0], Rt[:, 1])], 1)) - 1) < 1e-9


def test_fewer_than_two_axes():
    Rt = ref.rot((0.5, 0.5, 0.2), 11.0)
    R0 = _pert(Rt, 2.0)
    o = ref.track_manhattan(np.zeros((0, 3), F32), None, R0)          # nothing: R_last comes back unchanged
    assert o["n_found"] == 0 and o["tracked"] == 0 and o["min_num_sn"] == 0 and np.array_equal(o["R"], R0)
    rng = np.random.RandomState(4)
    n = np.concatenate([ref.family(rng, Rt[:, 1], 500, 0.5), ref.scatter(rng, 100, Rt)]).astype(F32)
    o = ref.track_manhattan(n, None, R0)                               # one axis: no SVD, R_last with that column replaced
    assert o["n_found"] == 1 and o["found"] == [0, 1, 0] and o["tracked"] == 0
    want = R0.copy(); want[:, 1] = o["axis_vec"][1]
    assert np.array_equal(o["R"], want)


def test_threshold_fallback():
    Rt = ref.rot((0.1, 0.9, 0.3), 31.0)
    rng = np.random.RandomState(5)
    n = np.concatenate([ref.family(rng, Rt[:, 0], 1000, 0.5), ref.family(rng, Rt[:, 1], 30, 0.5), ref.family(rng, Rt[:, 2], 10, 0.5),
                        ref.scatter(rng, 500, Rt)]).astype(F32)
    o = ref.track_manhattan(n, None, Rt.astype(F32))
    assert o["n_in_cone"] == [1000, 30, 10]
    assert len(n) // 20 == 77 and o["min_num_sn"] == (30 + 10) // 2
    assert o["n_selected"] == [1000, 30, 10] and o["found"] == [1, 1, 0] and o["n_found"] == 2


def test_nan_normals_count_in_size_only():
    n, Rt = ref.three_families(seed=6, n=100)
    o = ref.track_manhattan(n, None, Rt.astype(F32))
    assert o["n_found"] == 3 and o["min_num_sn"] == len(n) // 20
    nan = np.full((6000, 3), np.nan, F32)
    o = ref.track_manhattan(np.concatenate([n, nan]), None, Rt.astype(F32))
    assert o["n_in_cone"] == [100, 100, 100]                           # NaN normals fail the cone test
    assert o["min_num_sn"] == 100 and o["n_selected"] == [100, 100, 100]   # but count in size / 20, and 100 > 100 fails
    assert o["n_found"] == 0 and np.array_equal(o["R"], Rt.astype(F32))


def test_axis_from_lines_alone():
    Rt = ref.rot((0.7, -0.2, 0.4), 14.0)
    rng = np.random.RandomState(7)
    n = np.concatenate([ref.family(rng, Rt[:, 0], 200, 0.5), ref.family(rng, Rt[:, 1], 200, 0.5)]).astype(F32)
    d = ref.family(rng, Rt[:, 2], 30, 1.0)
    bad = ref.family(rng, Rt[:, 2], 40, 1.0)
    l3d = np.concatenate([ref.lines_along(rng, d), ref.lines_along(rng, bad, good=np.zeros(40))])[np.r_[0:15, 30:70, 15:30]]
    o, = [ref.track_manhattan(n, l3d, Rt.astype(F32))]
    assert o["n_in_cone"] == [200, 200, 0] and o["min_num_sn"] == 20
    assert o["n_selected"][2] == 30 and o["found"] == [1, 1, 1]
    assert np.abs(o["R"] - Rt).max() < 1e-3
    assert o["line_axes"].sum() == 30 * 4 and np.all(o["line_axes"][15:55] == 0)
    o = ref.track_manhattan(n, l3d[:0], Rt.astype(F32))
    assert o["found"] == [1, 1, 0]


def test_cone_boundary_one_ulp():
    n, s_in, s_out = ref.boundary_normals()
    assert float(s_in) < ref.SIN_N <= float(s_out) and np.nextafter(s_in, F32(1)) == s_out
    o = ref.track_manhattan(n, None, np.eye(3, dtype=F32))
    assert o["n_in_cone"][0] == 1
    assert list(o["normal_axes"]) == [1, 0]
    assert abs(math.asin(float(s_in)) - 0.2018) < 1e-6


def test_example_compiles():
    import os
    import subprocess
    from conftest import ROOT
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-fsyntax-only",
                           os.path.join(ROOT, "examples", "manhattan_track.cpp")])
