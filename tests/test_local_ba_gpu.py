"""LocalBA.optimize (csrc/local_ba.hip) against the restatement tests/local_ba_ref.py on the device.

Shapes (local_ba_ref.SHAPES): S = 5 local key frames (the last of them fixed as id 0) + 2 outside observers, 60 points, 10 lines carrying
all four line edge kinds; M = 24 free + 8 fixed key frames, 1500 points, 120 lines (more than one workgroup of edges, more than 64 edges
per observer); W = 64 free key frames with 30 points each and 16 lines (the reduced system at its largest, 384 unknowns).

D is measured on the CPU (local_ba_ref.measured_D), one figure each for poses, points and lines; the device must lie within 8 D, the
margin pose_opt and line_opt use.  The references are computed once per module."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import local_ba_ref as ref
from conftest import ROOT, PKG_DIR

pytestmark = pytest.mark.gpu
FLAGS = ("pt_erase", "ln_erase", "manh_erase", "par_erase", "perp_erase", "par_made", "perp_made", "line_made")
COUNTS = ("n_free_kf", "n_pt_edges", "n_line_obs", "n_manh_edges", "n_par_edges", "n_perp_edges", "n_lines_made", "rounds", "stopped_at", "status")
ARRAYS = ("Tcw_f", "Tcw_d", "pt_f", "pt_d", "ln_f", "ln_d") + FLAGS
W_SEED = 1001        # the first seed from 1000 on whose W window is accepted (checked below)


@pytest.fixture(scope="module")
def ba(hvo):
    b = hvo.LocalBA()
    yield b
    b.close()


@pytest.fixture(scope="module")
def scenes():
    out = {}
    for shape, n in (("S", 4), ("M", 2)):
        sc, gen = ref.accepted_scenes(shape, n)
        assert 2 * len(sc) >= gen, (shape, len(sc), gen)
        out[shape] = (sc, ref.measured_D(sc))
    sc, gen = ref.accepted_scenes("W", 1, seed0=W_SEED)
    assert gen == 1
    out["W"] = (sc, ref.measured_D(sc))
    return out


def run(ba, W, **kw):
    return ba.optimize(ref.to_binding(W), **kw)


def same_flags(o, R):
    for k in FLAGS:
        assert np.array_equal(getattr(o, k), getattr(R, k)), k
    for k in COUNTS:
        assert getattr(o, k) == getattr(R, k), (k, getattr(o, k), getattr(R, k))


def diffs(o, R):
    return np.array([np.abs(o.Tcw_d - R.Tcw_d).max(), np.abs(o.pt_d - R.pt_d).max() if o.pt_d.size else 0.0, np.abs(o.ln_d - R.ln_d).max() if o.ln_d.size else 0.0])


def same_bytes(a, b):
    for k in ARRAYS:
        assert getattr(a, k).tobytes() == getattr(b, k).tobytes(), k
    for k in COUNTS + ("iterations", "trials", "lam", "chi2"):
        assert getattr(a, k) == getattr(b, k), k


def check_floats(o):
    """the float write-back is the double estimate rounded (Converter::toCvMat)"""
    assert np.array_equal(o.Tcw_f, o.Tcw_d.astype(np.float32)) and np.array_equal(o.pt_f, o.pt_d.astype(np.float32)) and np.array_equal(o.ln_f, o.ln_d.astype(np.float32))


@pytest.mark.parametrize("shape", ["S", "M"])
def test_accepted_scenes_agree_with_the_restatement(ba, scenes, shape):
    sc, D = scenes[shape]
    print("%s: D (poses, points, lines) = %s over %d accepted windows" % (shape, D, len(sc)))
    assert np.all(D > 0)
    for W, R, _, _ in sc:
        o = run(ba, W)
        d = diffs(o, R)
        print("  iterations %s / %s trials %s / %s lambda %s / %s chi2 %s / %s diff %s  %.2f ms" % (o.iterations, R.iterations, o.trials, R.trials, o.lam, R.lam, o.chi2, R.chi2, d, o.ms))
        same_flags(o, R)
        assert np.all(d <= 8 * D), (d, D)
        check_floats(o)
        assert int(o.pt_erase.sum()) > 0 and o.status == 0


def test_trial_counts_on_a_crafted_window(ba):
    """no outlier, an exact start of the landmarks and poses well off: every trial changes chi2 by more than 1e-4 of itself, so iterations,
    trials and lambda are compared too"""
    W, _ = ref.shape_window("S", 31, outliers=0.0, lm_off=0.0, off=(0.01, 0.03), structural=False)
    W = W.copy(manh_available=0)
    R = ref.local_map_optimization(W, params=dict(iterations=(4, 3)))
    assert min(abs(s) for s in R.steps) > 1e-4, R.steps
    o = run(ba, W, params=dict(iterations=(4, 3)))
    print("iterations", o.iterations, "trials", o.trials, "lambda", o.lam, R.lam)
    assert o.iterations == R.iterations and o.trials == R.trials
    assert np.allclose(o.lam, R.lam, rtol=1e-6) and np.allclose(o.chi2, R.chi2, rtol=1e-6)
    same_flags(o, R)


def test_the_largest_reduced_system(hvo, ba, scenes):
    sc, D = scenes["W"]
    W, R = sc[0][0], sc[0][1]
    assert R.n_free_kf == 64
    o = run(ba, W)
    d = diffs(o, R)
    print("W: D", D, "diff", d, "iterations", o.iterations, "trials", o.trials, "%.2f ms" % o.ms)
    same_flags(o, R)
    assert np.all(d <= 8 * D), (d, D)
    same_bytes(o, run(ba, W))


def test_same_bytes_twice_and_a_dirty_workspace(hvo, ba, scenes):
    S = scenes["S"][0][0][0]; M = scenes["M"][0][0][0]
    a = run(ba, S)
    same_bytes(a, run(ba, S))
    run(ba, M)
    b = run(ba, S)                                        # after M the workspace holds M's blocks
    fresh = hvo.LocalBA()
    try:
        same_bytes(b, run(fresh, S))
    finally:
        fresh.close()
    same_bytes(a, b)


def variant(W, **kw):
    return W.copy(**kw)


def test_zero_points_zero_lines_and_every_line_skipped(ba, scenes):
    S = scenes["S"][0][0][0]
    nl = S.n_lines
    no_pts = variant(S, pt_pos=np.zeros((0, 3)), pt_obs_start=[0], pt_obs_kf=[], pt_obs_uv=np.zeros((0, 2)), pt_obs_inv_sigma2=[])
    empty = dict(ln_pos=np.zeros((0, 6)), ln_manh_idx=[], ln_obs_start=[0], ln_obs_kf=[], ln_obs_fn=np.zeros((0, 3)), par_start=[0], par_kf=[], par_idx=[],
                 par_fn=np.zeros((0, 3)), par_map_size=[], perp_start=[0], perp_kf=[], perp_idx=[], perp_fn=np.zeros((0, 3)), perp_map_size=[])
    no_lines = variant(S, **empty)
    pos = S.ln_pos.copy(); pos[::2, 1] = np.nan; pos[1::2, 3] = pos[1::2, 0] + 5e-6
    skipped = variant(S, ln_pos=pos)
    for name, W in (("zero points", no_pts), ("zero lines", no_lines), ("every line skipped", skipped)):
        R = ref.local_map_optimization(W)
        o = run(ba, W)
        d = diffs(o, R) if name != "every line skipped" else np.array([np.abs(o.Tcw_d - R.Tcw_d).max(), np.abs(o.pt_d - R.pt_d).max(), 0.0])
        print(name, "diff", d, "iterations", o.iterations, R.iterations, "trials", o.trials, R.trials)
        for k in ("n_free_kf", "n_pt_edges", "n_line_obs", "n_manh_edges", "n_par_edges", "n_perp_edges", "n_lines_made", "status"):
            assert getattr(o, k) == getattr(R, k), (name, k)
        for k in ("par_made", "perp_made", "line_made"):
            assert np.array_equal(getattr(o, k), getattr(R, k)), (name, k)
        assert o.status == 0 and o.rounds == 2
    o = run(ba, skipped)
    assert o.n_lines_made == 0 and not o.line_made.any() and not o.ln_erase.any() and not o.par_made.any()
    assert o.ln_d.tobytes() == skipped.ln_pos.tobytes()          # a skipped line comes back as it went in, NaN included
    assert run(ba, no_lines).n_lines_made == 0 and run(ba, no_pts).n_pt_edges == 0


def test_no_manhattan_edges_without_axes_or_index(ba, scenes):
    S = scenes["S"][0][0][0]
    assert run(ba, S).n_manh_edges > 0
    for W in (variant(S, manh_available=0), variant(S, ln_manh_idx=np.zeros(S.n_lines))):
        o = run(ba, W); R = ref.local_map_optimization(W)
        assert o.n_manh_edges == 0 == R.n_manh_edges and not o.manh_erase.any()
        assert o.n_par_edges == R.n_par_edges > 0 and o.status == 0


def test_a_point_whose_observers_all_turn_level_1(ba, scenes):
    """every observation of point 0 is a gross outlier: after round 1 it has no active edge, keeps round 1's estimate through round 2
    and all its observations are flagged"""
    S = scenes["S"][0][0][0]
    uv = S.pt_obs_uv.copy(); a, b = S.pt_obs_start[0], S.pt_obs_start[1]
    uv[a:b] += np.array([[150.0, -120.0], [-140.0, 130.0]] * 8, np.float32)[:b - a]
    W = variant(S, pt_obs_uv=uv)
    R = ref.local_map_optimization(W); o = run(ba, W)
    assert R.pt_erase[a:b].all() and R.level[R.graph.pt_edge[a:b]].all()
    assert o.pt_erase[a:b].all()
    one = ref.local_map_optimization(W, params=dict(iterations=(5, 0)))
    assert np.abs(R.pt_d[0] - one.pt_d[0]).max() == 0.0          # the restatement: round 2 does not move it
    o1 = run(ba, W, params=dict(iterations=(5, 0)))
    assert o.pt_d[0].tobytes() == o1.pt_d[0].tobytes()             # the device: neither


def test_a_free_key_frame_without_edges_and_no_free_key_frame(ba, scenes):
    S = scenes["S"][0][0][0]
    T = np.concatenate([S.Tcw, S.Tcw[:1] + 0], axis=0); lone = S.n_kf
    fixed = np.concatenate([S.fixed, [0]]); cam = np.concatenate([S.cam, S.cam[:1]], axis=0)
    W = variant(S, Tcw=T, fixed=fixed, cam=cam)
    o = run(ba, W); R = ref.local_map_optimization(W)
    assert o.n_free_kf == R.n_free_kf == int((S.fixed == 0).sum()) + 1 and o.status == 0
    assert np.abs(o.Tcw_d[lone] - R.Tcw_d[lone]).max() < 1e-15 and np.abs(o.Tcw_d[lone] - T[lone]).max() < 1e-6      # kept: only the quaternion round trip
    base = run(ba, S)
    assert o.Tcw_d[:lone].tobytes() == base.Tcw_d.tobytes()      # and the others do not notice it
    none = variant(S, fixed=np.ones(S.n_kf))
    o = run(ba, none)
    assert o.status == 1 and o.rounds == 0 and o.iterations == [0, 0]
    assert o.Tcw_f.tobytes() == none.Tcw.tobytes() and o.pt_f.tobytes() == none.pt_pos.tobytes() and o.ln_d.tobytes() == none.ln_pos.tobytes()
    assert not o.pt_erase.any() and not o.ln_erase.any()


def test_stop_flag_and_polls(hvo, ba, scenes):
    S, R0 = scenes["S"][0][0][0], scenes["S"][0][0][1]
    stop = ctypes.c_int(1)
    o = run(ba, S, stop=stop)
    assert o.status == 2 and o.stopped_at == 0 and o.rounds == 0
    assert o.Tcw_f.tobytes() == S.Tcw.tobytes() and o.pt_f.tobytes() == S.pt_pos.tobytes() and o.ln_d.tobytes() == S.ln_pos.tobytes() and not o.pt_erase.any()
    # the polls of an undisturbed run: 0 the test before round 1; then one before each iteration, one after each rejected trial that
    # allows another; one between the rounds
    between = 1 + R0.iterations[0] + (R0.trials[0] - R0.iterations[0])
    if R0.iterations[0] < 5: between += 1
    cases = {"before an iteration": 3, "between the rounds": between, "first poll of round 2": between + 1}
    W2, _ = ref.shape_window("S", 73, off=(0.02, 0.08))     # a window whose first round rejects a trial: the poll after it exists
    R2 = ref.local_map_optimization(W2, params=dict(iterations=(5, 0)))
    assert R2.trials[0] > R2.iterations[0]
    for name, k in cases.items():
        R = ref.local_map_optimization(S, params=dict(stop_at_poll=k))
        o = run(ba, S, params=dict(stop_at_poll=k))
        print(name, "poll", k, "rounds", o.rounds, "iterations", o.iterations, "trials", o.trials)
        assert R.stopped_at == k, (name, R.stopped_at)
        same_flags(o, R)
        assert o.iterations == R.iterations and o.trials == R.trials
        assert np.all(diffs(o, R) <= 8 * scenes["S"][1])
    assert ref.local_map_optimization(S, params=dict(stop_at_poll=between)).rounds == 1
    j = next(i for i, s in enumerate(R2.steps) if s < 0)    # the first rejected trial; it is the (j + 1)-th iteration's second-to-last
    k = 1 + (j + 1)                                         # polls before it: the entry test and one before each of j + 1 iterations
    R = ref.local_map_optimization(W2, params=dict(stop_at_poll=k)); o = run(ba, W2, params=dict(stop_at_poll=k))
    print("after a trial: poll", k, "iterations", o.iterations, "trials", o.trials)
    assert R.trials[0] == j + 1 and R.iterations[0] == j + 1 and R.rounds == 1          # the restatement stopped right after that trial
    assert o.stopped_at == R.stopped_at == k and o.iterations == R.iterations and o.trials == R.trials and o.rounds == R.rounds
    for f in FLAGS: assert np.array_equal(getattr(o, f), getattr(R, f)), f


def test_every_limit_is_refused_whole(hvo, ba, scenes):
    S = scenes["S"][0][0][0]
    nkf = S.n_kf

    def grown(n, kind):
        z = np.zeros
        if kind == "kf":
            return variant(S, Tcw=np.tile(S.Tcw[-1:], (n, 1, 1)), fixed=np.ones(n), cam=np.tile(S.cam[:1], (n, 1)), **{k: getattr(S, k) for k in ()})
        if kind == "free":
            return variant(S, Tcw=np.tile(S.Tcw[:1], (n, 1, 1)), fixed=z(n), cam=np.tile(S.cam[:1], (n, 1)))
        if kind == "points":
            return variant(S, pt_pos=z((n, 3)), pt_obs_start=z(n + 1), pt_obs_kf=[], pt_obs_uv=z((0, 2)), pt_obs_inv_sigma2=[])
        if kind == "lines":
            return variant(S, ln_pos=z((n, 6)), ln_manh_idx=z(n), ln_obs_start=z(n + 1), ln_obs_kf=[], ln_obs_fn=z((0, 3)), par_start=z(n + 1), par_kf=[], par_idx=[],
                           par_fn=z((0, 3)), par_map_size=z(n), perp_start=z(n + 1), perp_kf=[], perp_idx=[], perp_fn=z((0, 3)), perp_map_size=z(n))
        if kind == "pt_obs":
            st = z(S.n_points + 1, np.int64); st[1:] = n
            return variant(S, pt_obs_start=st, pt_obs_kf=z(n), pt_obs_uv=z((n, 2)), pt_obs_inv_sigma2=z(n))
        if kind == "ln_obs":
            st = z(S.n_lines + 1, np.int64); st[1:] = n
            return variant(S, ln_obs_start=st, ln_obs_kf=z(n), ln_obs_fn=z((n, 3)))
        if kind == "struct":
            st = z(S.n_lines + 1, np.int64); st[1:] = n
            return variant(S, par_start=st, par_kf=z(n), par_idx=z(n), par_fn=z((n, 3)), perp_start=st, perp_kf=z(n), perp_idx=z(n), perp_fn=z((n, 3)))
    kf_out = S.pt_obs_kf.copy(); kf_out[3] = nkf
    par_out = S.par_kf.copy(); par_out[0] = -1
    twice = S.pt_obs_kf.copy(); twice[S.pt_obs_start[1] + 1] = twice[S.pt_obs_start[1]]
    twice_l = S.ln_obs_kf.copy(); twice_l[S.ln_obs_start[1] + 1] = twice_l[S.ln_obs_start[1]]
    cases = [("1024 key frames", grown(1025, "kf")), ("64 free", grown(65, "free")), ("65536 points", grown(65537, "points")), ("16384 lines", grown(16385, "lines")),
             ("2^20 point observations", grown((1 << 20) + 1, "pt_obs")), ("2^18 line observations", grown((1 << 18) + 1, "ln_obs")),
             ("2^18 par plus perp", grown((1 << 17) + 1, "struct")), ("outside the call's list", variant(S, pt_obs_kf=kf_out)),
             ("outside the call's list", variant(S, par_kf=par_out)), ("one point twice", variant(S, pt_obs_kf=twice)), ("one line twice", variant(S, ln_obs_kf=twice_l))]
    for what, W in cases:
        with pytest.raises(hvo.HvoError, match=re.escape(what)) as e:
            run(ba, W, limits=False)
        assert e.value.status == -4, what
        out = e.value.output
        for k in ("Tcw_d", "pt_d", "ln_d", "Tcw_f", "pt_f", "ln_f"):
            assert np.isnan(getattr(out, k)).all(), (what, k)
        for k in FLAGS:
            assert (getattr(out, k) == 0xEE).all(), (what, k)
        with pytest.raises(ref.Refused, match=re.escape(what)):
            ref.local_map_optimization(W)
    run(ba, S)                                            # and the object is as usable as before


def test_the_example_builds_and_runs(tmp_path):
    exe = str(tmp_path / "local_map_optimization")
    lib = os.path.join(PKG_DIR, "csrc")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-std=c++17", "-O1", "-x", "c++", os.path.join(ROOT, "examples", "local_map_optimization.cpp"), "-I", os.path.join(ROOT, "include"),
                           "-L", lib, "-lhvo", "-Wl,-rpath," + lib, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0 and "local map optimization ok" in out.stdout
