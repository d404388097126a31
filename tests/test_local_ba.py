"""Optimizer::LocalMapOptimization without a device: the restatement tests/local_ba_ref.py pinned by known answers, the readings it
takes, and the new symbols of every layer (header, library, binding, C++ mirror, example)."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import local_ba_ref as ref
from conftest import ROOT, PKG_DIR

NEW = ("hvo_local_ba_create", "hvo_local_ba_destroy", "hvo_local_ba_last_error", "hvo_local_ba_last_ms", "hvo_local_ba_last_profile", "hvo_local_ba_default_params", "hvo_local_ba_optimize")


@pytest.fixture(scope="module")
def small():
    return ref.shape_window("S", 5)


def line_distance(ends, truth):
    """largest distance of the estimated end points from the true infinite lines (an end point slides along its line unobserved)"""
    d = truth[:, 3:] - truth[:, :3]; d = d / np.linalg.norm(d, axis=1)[:, None]
    out = 0.0
    for k in (0, 3):
        v = ends[:, k:k + 3] - truth[:, :3]
        out = max(out, float(np.linalg.norm(v - (v * d).sum(axis=1)[:, None] * d, axis=1).max()))
    return out


def test_a_noise_free_window_converges_to_the_truth():
    """(a) poses and landmarks, the fixed key frames as the gauge; iterations raised so that the check is of the minimum, not of the budget"""
    W, T = ref.shape_window("S", 5, noise=0.0, outliers=0.0, skip_cases=False, off=(0.003, 0.01), lm_off=0.02)
    R = ref.local_map_optimization(W, params=dict(iterations=(30, 30)))
    free = W.fixed == 0
    before = np.abs(W.Tcw.astype(np.float64) - T["Tcw"])[free].max(); after = np.abs(R.Tcw_d - T["Tcw"])[free].max()
    print("poses %.2e -> %.2e, points %.2e -> %.2e, lines %.2e -> %.2e, chi2 %s" % (before, after, np.abs(W.pt_pos - T["points"]).max(), np.abs(R.pt_d - T["points"]).max(),
                                                                                 line_distance(W.ln_pos, T["lines"]), line_distance(R.ln_d, T["lines"]), R.chi2))
    assert before > 1e-3 and after < 2e-5
    assert np.abs(R.pt_d - T["points"]).max() < 2e-3 and np.abs(W.pt_pos - T["points"]).max() > 2e-2      # float pixels: a few 1e-5 px at metres of depth
    # a line that fewer than two key frames observe is held by its Manhattan edge alone and is left out
    seen = np.diff(W.ln_obs_start) >= 2
    assert seen.sum() >= 8
    assert line_distance(R.ln_d[seen], T["lines"][seen]) < 2e-4 and line_distance(W.ln_pos[seen], T["lines"][seen]) > 1e-2
    assert R.chi2[1] < 1e-4 and not R.pt_erase.any() and not R.ln_erase.any() and not R.par_erase.any() and not R.perp_erase.any() and not R.manh_erase.any()
    assert np.array_equal(R.Tcw_d[~free], np.array([ref.se3_to_Tcw(ref.se3_from_Tcw(t)) for t in W.Tcw[~free]]))     # the gauge did not move
    assert np.array_equal(R.Tcw_f, R.Tcw_d.astype(np.float32)) and np.array_equal(R.ln_f, R.ln_d.astype(np.float32))


def test_the_eliminated_step_is_the_dense_solve(small):
    """(b) what licenses treating a line as one landmark: the step from the landmark-eliminated system equals numpy.linalg.solve on the
    full system over (free key frames, point coordinates, line coordinates), to a relative 1e-9"""
    W, _ = small
    g = ref._Graph(W, ref.default_params())
    assert g.counts[ref.MANH] and g.counts[ref.PAR] and g.counts[ref.PERP] and g.counts[ref.START]
    for robust, ops in ((True, ref.Ops()), (False, ref.Ops("tree", 3))):
        lin = ref.Linearisation(g, g.pose0, g.lm0, np.ones(g.E, bool), robust, ops)
        lam = 1e-5 * lin.max_diag
        dx, dl, ok, scale = lin.step(lam, ops)
        H, b, idx = lin.full_system()
        x = np.linalg.solve(H + lam * np.eye(len(b)), b)
        mine = np.concatenate([dx.reshape(-1), dl.reshape(-1)[idx]])
        rel = np.abs(mine - x).max() / np.abs(x).max()
        print("unknowns %d, largest relative difference %.2e" % (len(b), rel))
        assert ok and rel < 1e-9
        assert abs(scale - float(x @ (lam * x + b))) < 1e-9 * abs(scale)


def test_jacobians(small):
    """(c) the numeric rule reproduces the analytic point Jacobian, and perturbs exactly the non-fixed vertices of every edge"""
    W, _ = small
    g = ref._Graph(W, ref.default_params()); ops = ref.Ops()
    R, t, X = g.gather(g.pose0, g.lm0)
    Nl, Np = g.numeric_jacobians(g.pose0, g.lm0, ops)
    Al, Ap = g.point_jacobians(R, t, X)
    pt = g.is_pt; free = g.ef >= 0
    assert np.abs(Nl[pt] - Al[pt]).max() < 2e-4 * np.abs(Al[pt]).max()          # delta 1e-9 on pixel values of a few hundred: about 1e-5 of rounding
    assert np.abs(Np[pt & free] - Ap[pt & free]).max() < 2e-4 * np.abs(Ap[pt]).max()
    assert (pt & ~free).any() and not Np[~free].any()                            # a fixed observer: no pose columns
    k = g.kind
    assert Nl[k == ref.START][:, 0, :3].any() and not Nl[k == ref.START][:, :, 3:].any()       # start vertex only
    assert Nl[k == ref.END][:, 0, 3:].any() and not Nl[k == ref.END][:, :, :3].any()           # end vertex only
    for kind in (ref.MANH, ref.PAR, ref.PERP):
        J = Nl[k == kind]
        assert np.abs(J[:, 0, :3]).max() > 0 and np.abs(J[:, 0, 3:]).max() > 0 and not J[:, 1].any()
    assert not Np[k == ref.MANH].any()                                           # no pose vertex
    tern = ((k == ref.PAR) | (k == ref.PERP))
    assert (tern & free).any() and np.all(np.abs(Np[tern & free][:, 0]).max(axis=1) > 0) and not Np[tern & ~free].any()


def test_reading_1_the_current_key_frames_camera(small):
    W, _ = small
    cam = W.cam.copy(); cam[1:, 0] *= 1.05; cam[1:, 2] += 7.0
    V = W.copy(cam=cam)
    a = ref._Graph(V, ref.default_params()); b = ref._Graph(V, ref.default_params(), end_cam_current=False)
    k = a.kind
    for kind in (ref.END, ref.PAR, ref.PERP):
        assert np.all(a.cam[k == kind] == cam[0].astype(np.float64)) and np.all(b.cam[k == kind] == cam[b.kf[k == kind]].astype(np.float64))
    assert np.all(a.cam[k == ref.START] == cam[a.kf[k == ref.START]].astype(np.float64)) and np.array_equal(a.cam[k == ref.PT], b.cam[k == ref.PT])
    ra = ref.local_map_optimization(V); rb = ref.local_map_optimization(V, end_cam_current=False)
    assert np.abs(ra.ln_d - rb.ln_d).max() > 1e-4                               # the end points are pulled to where key frame 0's camera puts them


def test_reading_2_the_error_an_edge_holds():
    W, _ = ref.shape_window("S", 100, noise=0.5, outliers=0.1)
    a = ref.local_map_optimization(W); b = ref.local_map_optimization(W, stored_error=False)
    d = np.flatnonzero(a.pt_erase != b.pt_erase)
    assert len(d)
    e = a.graph.pt_edge[d]
    # every difference is an edge put on level 1 after round 1: its held error (round 1's) is over the gate, at the final estimate it is not
    assert a.level[e].all() and np.all(a.held[e] > 5.991) and np.all(b.held[e] <= 5.991) and a.pt_erase[d].all() and not b.pt_erase[d].any()
    assert np.array_equal(a.Tcw_d, b.Tcw_d)                                     # the reading changes the flags, not the estimate


def test_reading_3_the_final_test_reads_the_start_edge_twice(small):
    W, _ = small
    o = int(W.ln_obs_start[0]) + 1; k = int(W.ln_obs_kf[o])
    g = ref._Graph(W, ref.default_params())
    R, t, X = g.gather(g.pose0, g.lm0)
    es = g.ln_start_edge[o]
    ps = g._project(R, t, X[:, :3])[es]; pe = g._project(R, t, X[:, 3:])[g.ln_end_edge[o]]
    d = pe - ps; d = d / np.linalg.norm(d); c, s = np.cos(0.12), np.sin(0.12)
    d = np.array([c * d[0] - s * d[1], s * d[0] + c * d[1]])                   # the observed line turned about the start point's projection
    fn = np.array([-d[1], d[0], 0.0]); fn[2] = -(fn[0] * ps[0] + fn[1] * ps[1])
    f = W.ln_obs_fn.copy(); f[o] = fn
    V = W.copy(ln_obs_fn=f)
    # one iteration in round 1: the end point has not yet slid along its line to where the turned line crosses it
    a = ref.local_map_optimization(V, params=dict(iterations=(1, 10))); b = ref.local_map_optimization(V, params=dict(iterations=(1, 10)), final_start_twice=False)
    ee = a.graph.ln_end_edge[o]
    assert a.level[es] and a.level[ee] and a.held[ee] > 3.84 >= a.held[es]       # classified out by its END edge
    assert not a.ln_erase[o] and b.ln_erase[o]                                  # and not erased, because the final test never reads it
    assert k == W.ln_obs_kf[o]


def test_readings_4_and_5_the_walk():
    W, _ = ref.shape_window("S", 5)
    R = ref.local_map_optimization(W)
    R.ln_erase[:] = 0
    made = [o for o in range(len(W.ln_obs_kf)) if R.line_made[np.searchsorted(W.ln_obs_start, o, side="right") - 1]]
    i = 5; R.ln_erase[made[i]] = 1
    owner = int(np.searchsorted(W.ln_obs_start, made[i], side="right") - 1)
    _, lines_w, _, _ = ref.walk_erased(W, R)
    _, lines_a, _, _ = ref.walk_erased(W, R, pairing="aligned")
    assert lines_w == [(int(W.ln_obs_kf[made[i // 2]]), owner)] and lines_a == [(int(W.ln_obs_kf[made[i]]), owner)] and lines_w != lines_a
    # reading 5: a line on the wrong axis is flagged, and the walk has no list for it
    idx = W.ln_manh_idx.copy(); l = int(np.flatnonzero(idx == 1)[0]); idx[l] = 2
    R2 = ref.local_map_optimization(W.copy(ln_manh_idx=idx))
    assert R2.manh_erase[l] and len(ref.walk_erased(W, R2)) == 4
    pts, _, par, perp = ref.walk_erased(W, R2)
    assert len(pts) == int(R2.pt_erase.sum()) and len(par) == int(R2.par_erase.sum()) and len(perp) == int(R2.perp_erase.sum())
    for line, kf, k in par:
        first = W.par_start[line] + int(np.flatnonzero(W.par_kf[W.par_start[line]:W.par_start[line + 1]] == kf)[0])
        assert R2.par_erase[first + k]


def test_graph_rules_and_polls(small):
    W, _ = small
    R = ref.local_map_optimization(W)
    assert R.status == ref.OPTIMISED and R.rounds == 2 and R.stopped_at == -1
    assert 0 < R.par_made.sum() < len(R.par_made) and 0 < R.perp_made.sum() < len(R.perp_made)          # the skip cases are in the window
    bad = (W.par_idx < 0) | (W.par_fn[:, 0] == 0.0) | (W.par_fn[:, 0] == -1.0) | np.isnan(W.par_fn).any(axis=1)
    assert np.array_equal(R.par_made == 0, bad)
    info = R.graph.info[R.graph.kind == ref.PAR]
    assert set(np.round(info, 6)) <= {round(0.5 + k / 10.0, 6) for k in range(1, 4)}                     # 0.5 + keys / 10
    assert ref.default_params()["huber_delta"][0] == float(np.float32(np.sqrt(5.991)))
    r0 = ref.local_map_optimization(W, params=dict(stop_at_poll=0))
    assert r0.status == ref.STOPPED and r0.stopped_at == 0 and np.array_equal(r0.Tcw_f, W.Tcw) and np.array_equal(r0.ln_d, W.ln_pos) and not r0.pt_erase.any()
    r1 = ref.local_map_optimization(W, params=dict(stop_at_poll=1))
    assert r1.status == ref.OPTIMISED and r1.rounds == 1 and r1.iterations == [0, 0] and not r1.pt_erase.any()     # no edge was ever evaluated: chi2() == 0
    between = 1 + R.iterations[0] + (R.trials[0] - R.iterations[0]) + (1 if R.iterations[0] < 5 else 0)
    rb = ref.local_map_optimization(W, params=dict(stop_at_poll=between))
    assert rb.rounds == 1 and rb.iterations == [R.iterations[0], 0] and rb.stopped_at == between and rb.pt_erase.any()
    none = ref.local_map_optimization(W.copy(fixed=np.ones(W.n_kf)))
    assert none.status == ref.NOTHING and np.array_equal(none.pt_f, W.pt_pos)
    sc, gen = ref.accepted_scenes("S", 3)
    assert 2 * len(sc) >= gen
    D = ref.measured_D(sc)
    print("D (poses, points, lines) on %d of %d windows: %s" % (len(sc), gen, D))
    assert np.all(D > 0) and D[0] < 1e-3


def test_symbols_declared_exported_bound_and_sized(hvo):
    """(e)"""
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hvo.h")).read(), flags=re.S)
    lib = ctypes.CDLL(os.path.join(PKG_DIR, "csrc", "libhvo.so"))
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert hasattr(lib, n), n
        assert n in hvo.EXPORTS, n
    # the header's layouts: 2 + 1 + 1 int32 and 9 doubles; 4 int32 and 24 pointers; 14 pointers, 4 int32, 4 doubles, 10 int32
    assert ctypes.sizeof(hvo.LocalBAParams) == 16 + 72 and ctypes.sizeof(hvo.LocalBAGraph) == 16 + 24 * 8 and ctypes.sizeof(hvo.LocalBAResult) == 14 * 8 + 16 + 32 + 40
    fields = re.search(r"typedef struct \{([^}]*)\} hvo_local_ba_graph;", hdr).group(1)
    names = re.findall(r"\*\s*(\w+)", fields)
    assert names == [n for n, _ in hvo.LOCAL_BA_GRAPH_ARRAYS]
    fields = re.search(r"typedef struct \{([^}]*)\} hvo_local_ba_result;", hdr).group(1)
    assert re.findall(r"\*\s*(\w+)", fields) == list(hvo.LOCAL_BA_RESULT_ARRAYS)
    lib.hvo_abi_version.restype = ctypes.c_int
    assert lib.hvo_abi_version() == 3
    p = hvo.LocalBA.default_params()
    d = ref.default_params()
    assert list(p.iterations) == [5, 10] and p.max_trials == 10 and p.stop_at_poll == -1
    assert tuple(p.huber_delta) == d["huber_delta"] and tuple(p.chi2_gate) == d["chi2_gate"] and tuple(p.inv_sigma) == d["inv_sigma"]
    for k, v in ref.LIMITS.items():
        assert hvo.LBA_LIMITS[k] == v
    for name, macro in (("free_kf", "MAX_FREE_KF"), ("kf", "MAX_KF"), ("points", "MAX_POINTS"), ("lines", "MAX_LINES")):
        assert int(re.search(r"#define HVO_LBA_%s\s+(\d+)" % macro, hdr).group(1)) == ref.LIMITS[name]
    with pytest.raises(hvo.HvoError, match="hvo_local_ba_create"):
        hvo.LocalBA(device=1023)
    mirror = open(os.path.join(ROOT, "include", "hvo.hpp")).read()
    for name in ("class LocalBA", "struct LocalMapGraph", "struct LocalMapResult", "walkErased", "static int LocalMapOptimization(LocalBA &ba, const LocalMapGraph &g, const int *stop, LocalMapResult &r)"):
        assert name in mirror, name


def test_example_compiles():
    """(f) examples/local_map_optimization.cpp against the C++ mirror (tests/test_local_ba_gpu.py builds and runs it)"""
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx: pytest.skip("no host compiler")
    subprocess.check_call([cxx, "-std=c++14", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-fsyntax-only", os.path.join(ROOT, "examples", "local_map_optimization.cpp")])


def test_the_binding_refuses_every_limit_without_a_device(hvo, small):
    """(g) the checks that need no device are made before the library is entered, with the library's reasons"""
    S, _ = small
    z = np.zeros

    def st(n_lm, n): a = z(n_lm + 1, np.int64); a[1:] = n; return a
    kf_out = S.pt_obs_kf.copy(); kf_out[3] = S.n_kf
    twice = S.pt_obs_kf.copy(); twice[S.pt_obs_start[1] + 1] = twice[S.pt_obs_start[1]]
    twice_l = S.ln_obs_kf.copy(); twice_l[S.ln_obs_start[1] + 1] = twice_l[S.ln_obs_start[1]]
    nl = S.n_lines
    empty_lines = dict(ln_manh_idx=z(16385), ln_obs_start=z(16386), ln_obs_kf=[], ln_obs_fn=z((0, 3)), par_start=z(16386), par_kf=[], par_idx=[], par_fn=z((0, 3)),
                       par_map_size=z(16385), perp_start=z(16386), perp_kf=[], perp_idx=[], perp_fn=z((0, 3)), perp_map_size=z(16385))
    cases = [("1024 key frames", S.copy(Tcw=np.tile(S.Tcw[-1:], (1025, 1, 1)), fixed=np.ones(1025), cam=np.tile(S.cam[:1], (1025, 1)))),
             ("64 free", S.copy(Tcw=np.tile(S.Tcw[:1], (65, 1, 1)), fixed=z(65), cam=np.tile(S.cam[:1], (65, 1)))),
             ("65536 points", S.copy(pt_pos=z((65537, 3)), pt_obs_start=z(65538), pt_obs_kf=[], pt_obs_uv=z((0, 2)), pt_obs_inv_sigma2=[])),
             ("16384 lines", S.copy(ln_pos=z((16385, 6)), **empty_lines)),
             ("2\\^20 point observations", S.copy(pt_obs_start=st(S.n_points, (1 << 20) + 1), pt_obs_kf=z((1 << 20) + 1), pt_obs_uv=z(((1 << 20) + 1, 2)), pt_obs_inv_sigma2=z((1 << 20) + 1))),
             ("2\\^18 line observations", S.copy(ln_obs_start=st(nl, (1 << 18) + 1), ln_obs_kf=z((1 << 18) + 1), ln_obs_fn=z(((1 << 18) + 1, 3)))),
             ("2\\^18 par plus perp", S.copy(par_start=st(nl, (1 << 17) + 1), par_kf=z((1 << 17) + 1), par_idx=z((1 << 17) + 1), par_fn=z(((1 << 17) + 1, 3)),
                                            perp_start=st(nl, 1 << 17), perp_kf=z(1 << 17), perp_idx=z(1 << 17), perp_fn=z((1 << 17, 3)))),
             ("outside the call's list", S.copy(pt_obs_kf=kf_out)), ("one point twice", S.copy(pt_obs_kf=twice)), ("one line twice", S.copy(ln_obs_kf=twice_l))]
    for what, W in cases:
        with pytest.raises(hvo.HvoError, match=what) as e:
            hvo.local_ba_graph_arrays(ref.to_binding(W))
        assert e.value.status == -4
        with pytest.raises(ref.Refused, match=what):
            ref.check_limits(W)
    a, n_kf, n_pts, n_ln = hvo.local_ba_graph_arrays(ref.to_binding(S))
    assert (n_kf, n_pts, n_ln) == (S.n_kf, S.n_points, S.n_lines) and a["Tcw"].dtype == np.float32 and a["ln_pos"].dtype == np.float64
    with pytest.raises(ValueError):
        hvo.local_ba_graph_arrays(dict(ref.to_binding(S), pt_obs_inv_sigma2=S.pt_obs_inv_sigma2[:-1]))
