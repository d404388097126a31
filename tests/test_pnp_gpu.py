"""The relocalisation PnP solver on the GPU (csrc/pnp.hip) against tests/pnp_ref.py.  Everything is + - * / sqrt in a fixed order without
contraction, so every comparison is exact: samples, counts, masks, hyp_event and the float32 Tcw bits.  tests/test_pnp.py asserts on the CPU
that each crafted case reaches the path it is meant for (and that no error2 sits within 1e-6 relative of its threshold).

Planted poses: max |Tcw - planted| of the RESTATEMENT over the planted scenes used here is 1.2e-7 (float32 inputs dominate; measured on the
CPU by tests/test_pnp.py::test_planted_pose_error_of_the_restatement); with the margin of 4 for scenes not yet seen the bound is 4.8e-7."""
import numpy as np
import pytest

import pnp_ref as ref

pytestmark = pytest.mark.gpu
_cache = {}
POSE_TOL = 4.8e-7


def ctx_of(hvo):
    if "ctx" not in _cache:
        _cache["ctx"] = hvo.Context(max_batch=1)
    return _cache["ctx"]


def want_of(name):
    """the restatement's answer of a crafted case, computed once"""
    if name not in _cache:
        c = ref.cases()[name]
        _cache[name] = (c, [ref.solve(p, ref.CAM, c["P"], j=j) for j, p in enumerate(c["problems"])])
    return _cache[name]


def params_of(hvo, P):
    return hvo.pnp_params(**{k: v for k, v in P.items()})


def same(got, want, what=""):
    for k in ("N", "n_features", "min_inliers", "max_its", "T", "no_more", "status"):
        assert got[k] == want[k], (what, k, got[k], want[k])
    assert np.float32(got["epsilon"]).tobytes() == np.float32(want["epsilon"]).tobytes(), what
    assert np.array_equal(got["hyp_sample"], want["hyp_sample"]), (what, "hyp_sample")
    assert np.array_equal(got["hyp_inliers"], want["hyp_inliers"]), (what, "hyp_inliers")
    assert np.array_equal(got["hyp_event"], want["hyp_event"]), (what, "hyp_event")
    assert len(got["events"]) == len(want["events"]), (what, "events")
    for e, (g, w) in enumerate(zip(got["events"], want["events"])):
        assert g["iteration"] == w["iteration"] and g["n_inliers"] == w["n_inliers"] and g["success"] == w["success"], (what, e)
        assert g["Tcw"].tobytes() == w["Tcw"].tobytes(), (what, e, "Tcw", g["Tcw"], w["Tcw"])
        assert np.array_equal(g["inliers"], w["inliers"]), (what, e, "inliers")
        # the record's own hypothesis: what iterate() returns with bNoMore when the loop ends between this record and the next
        assert g["hyp_n_inliers"] == w["hyp_n_inliers"] == want["hyp_inliers"][w["iteration"] - 1], (what, e)
        assert g["hyp_Tcw"].tobytes() == w["hyp_Tcw"].tobytes(), (what, e, "hyp_Tcw")
        assert np.array_equal(g["hyp_inliers"], w["hyp_inliers"]), (what, e, "hyp_inliers")
    untouched(got, what)
    assert got["best_n_inliers"] == want["best_n_inliers"] and got["best_valid"] == want["best_valid"] and got["best_iteration"] == want["best_iteration"], what
    assert got["best_Tcw"].tobytes() == want["best_Tcw"].tobytes(), (what, "best_Tcw")
    assert np.array_equal(got["best_inliers"], want["best_inliers"]), (what, "best_inliers")
    if want["events"] and want["status"] == 0:                    # the last record's own hypothesis is the best of all T
        assert got["events"][-1]["hyp_Tcw"].tobytes() == want["best_Tcw"].tobytes() and np.array_equal(got["events"][-1]["hyp_inliers"], want["best_inliers"]), what


def untouched(got, what=""):
    """everything past T, past n_events and past n_features is as it was before the call (hvo_amd.PNP_SENTINEL bytes, iteration -99)"""
    raw, T, ne, nf = got["raw"], got["T"], len(got["events"]), got["n_features"]
    S = 0xA5
    for k in ("hyp_inliers", "hyp_event", "hyp_sample"):
        assert (raw[k][T:].view(np.uint8) == S).all(), (what, k, "past T")
    for k in ("ev_inliers", "ev_hyp_inliers"):
        assert (raw[k][ne:] == S).all() and (raw[k][:, nf:] == S).all(), (what, k, "past n_events / n_features")
    assert (raw["best_inliers"][nf:] == S).all(), what
    for e in range(ne, len(raw["events"])):
        v = raw["events"][e]
        assert v.iteration == -99 and v.n_inliers == 0 and v.success == 0 and v.hyp_n_inliers == 0 and not any(v.Tcw) and not any(v.hyp_Tcw), (what, e)


def run_case(hvo, name, check=True, spare_events=2):
    c, want = want_of(name)
    got = ctx_of(hvo).pnp_ransac(ref.CAM, c["problems"], params_of(hvo, c["P"]), want_sample=True, check=check, spare_events=spare_events)
    for j in range(len(want)):
        same(got[j], want[j], "%s[%d]" % (name, j))
    return c, got, want


def test_clean_scene_recovers_the_planted_pose(hvo):
    """one candidate, N = 40, all inliers"""
    c, got, want = run_case(hvo, "clean40")
    ev = got[0]["events"][0]
    assert ev["success"] and ev["n_inliers"] == 40
    assert np.abs(ev["Tcw"] - c["problems"][0]["Tcw"]).max() < POSE_TOL
    res, state = got[0], {}
    T, no_more, inl, n = hvo.pnp_iterate(res, state, 5)
    assert T is not None and not no_more and n == 40 and inl.sum() == 40 and state["mnIterations"] == ev["iteration"]


@pytest.mark.parametrize("n", [9, 10, 15, 63, 64, 65, 130])
def test_lane_and_ballot_edges(hvo, n):
    """N = 9 (no hypotheses), 10 (one iteration), 15, 63, 64, 65, 130 with 40 % gross outliers"""
    run_case(hvo, "edge%d" % n)


@pytest.mark.parametrize("n_kf", [1, 3, 17])
def test_many_candidates_in_one_call(hvo, n_kf):
    """candidates of different N in ONE call: every candidate equals itself alone (the same position, the others empty), bit for bit"""
    probs = ref.multi_problems(n_kf); P = ref.default_params(seed=11)
    got = ctx_of(hvo).pnp_ransac(ref.CAM, probs, params_of(hvo, P), want_sample=True)
    empty = dict(p3d=np.zeros((0, 3)), p2d=np.zeros((0, 2)), sigma2=np.zeros(0), feature_index=np.zeros(0, np.int32), n_features=1)
    for j in range(n_kf):                                         # EVERY candidate: the addressing by j * capN, j * Tcap, j * E is what this is about
        if j in (0, n_kf // 2, n_kf - 1):
            same(got[j], ref.solve(probs[j], ref.CAM, P, j=j), "candidate %d of %d" % (j, n_kf))
        alone = ctx_of(hvo).pnp_ransac(ref.CAM, [empty] * j + [probs[j]] + [empty] * (n_kf - 1 - j), params_of(hvo, P), want_sample=True)[j]
        for k in ("hyp_sample", "hyp_inliers", "hyp_event", "best_inliers", "best_Tcw"):
            assert alone[k].tobytes() == got[j][k].tobytes(), (j, k)
        assert len(alone["events"]) == len(got[j]["events"]), j
        for a, b in zip(alone["events"], got[j]["events"]):
            for k in ("Tcw", "inliers", "hyp_Tcw", "hyp_inliers"):
                assert a[k].tobytes() == b[k].tobytes(), (j, k)
            assert (a["iteration"], a["n_inliers"], a["hyp_n_inliers"]) == (b["iteration"], b["n_inliers"], b["hyp_n_inliers"]), j


@pytest.mark.parametrize("name", ["coplanar", "duplicates"])
def test_degenerate_geometry_is_finite_and_equal(hvo, name):
    c, got, want = run_case(hvo, name)
    for e in got[0]["events"]:
        assert np.isfinite(e["Tcw"]).all()
    assert np.isfinite(got[0]["best_Tcw"]).all()


def test_refine_fails_then_succeeds(hvo):
    c, got, want = run_case(hvo, "two_pose")
    ev = got[0]["events"]
    assert [e["success"] for e in ev] == [False, True]
    # the replay returns nothing at the first record and the second record's pose at its iteration, in chunks like Relocalization's
    state, seen = {}, []
    for _ in range(20):
        T, no_more, inl, n = hvo.pnp_iterate(got[0], state, 5)
        if T is not None or no_more:
            seen.append((state["mnIterations"], n)); break
    assert seen == [(ev[1]["iteration"], ev[1]["n_inliers"])]


def test_max_events_overflow(hvo):
    """two records, room for one: the status is HVO_ERR_CAPACITY, the kept event is complete, nothing past the cap is written"""
    c, want = want_of("overflow")
    with pytest.raises(hvo.HvoError):
        ctx_of(hvo).pnp_ransac(ref.CAM, c["problems"], params_of(hvo, c["P"]))
    for spare in (0, 3):                                          # cap_events == max_events, and room for three more that must stay as they were
        c, got, want = run_case(hvo, "overflow", check=False, spare_events=spare)      # same() ends with untouched(): the tails are the sentinel bytes
        assert got[0]["status"] == -5 and len(got[0]["events"]) == 1
        raw = got[0]["raw"]
        assert len(raw["events"]) == 1 + spare and raw["events"][0].iteration == want[0]["events"][0]["iteration"]
        assert (got[0]["hyp_event"] == -1).all()                  # the second record was not kept: no iteration names it


@pytest.mark.parametrize("name", ["refine280", "rows32", "rows33", "rows64", "rows65"])
def test_refine_tree_order(hvo, name):
    """a Refine over 280 inliers (the tree), and over exactly 32 / 33 (64 / 66 rows of M) and 64 / 65 correspondences: both sides of the rule"""
    c, got, want = run_case(hvo, name)
    assert got[0]["events"] and got[0]["events"][-1]["success"]
    assert np.abs(got[0]["events"][-1]["Tcw"] - c["problems"][0]["Tcw"]).max() < POSE_TOL


@pytest.mark.parametrize("name", ["clean40", "minset5", "minset64"])
def test_min_set(hvo, name):
    """min_set = 4, 5 and 64 (128 rows of M: the tree inside the hypothesis kernel)"""
    run_case(hvo, name)


def test_same_call_twice_and_another_seed(hvo):
    c, want = want_of("edge130")
    a = ctx_of(hvo).pnp_ransac(ref.CAM, c["problems"], params_of(hvo, c["P"]), want_sample=True)[0]
    b = ctx_of(hvo).pnp_ransac(ref.CAM, c["problems"], params_of(hvo, c["P"]), want_sample=True)[0]
    for k in ("hyp_sample", "hyp_inliers", "hyp_event", "best_Tcw", "best_inliers"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert [e["Tcw"].tobytes() + e["inliers"].tobytes() for e in a["events"]] == [e["Tcw"].tobytes() + e["inliers"].tobytes() for e in b["events"]]
    o = ctx_of(hvo).pnp_ransac(ref.CAM, c["problems"], params_of(hvo, dict(c["P"], seed=c["P"]["seed"] + 1)), want_sample=True)[0]
    assert not np.array_equal(o["hyp_sample"], a["hyp_sample"])
    ms = ctx_of(hvo).pnp_last_kernel_ms()
    assert ms[0] > 0 and ms[1] > 0


def test_invalid_arguments_and_limits(hvo):
    c, _ = want_of("clean40")
    p = c["problems"]
    for kw, status in ((dict(extra_iterations=1000), -4), (dict(min_set=3), -1), (dict(min_set=65), -4), (dict(max_events=0), -1)):
        with pytest.raises(hvo.HvoError) as e:
            ctx_of(hvo).pnp_ransac(ref.CAM, p, params_of(hvo, dict(c["P"], **kw)))
        assert e.value.status == status, kw
    big = dict(p3d=np.zeros((4097, 3)), p2d=np.zeros((4097, 2)), sigma2=np.ones(4097), feature_index=np.arange(4097), n_features=4097)
    with pytest.raises(hvo.HvoError) as e:
        ctx_of(hvo).pnp_ransac(ref.CAM, [big])
    assert e.value.status == -4
    bad = dict(p[0], feature_index=np.full(40, 99999, np.int32))
    with pytest.raises(hvo.HvoError) as e:
        ctx_of(hvo).pnp_ransac(ref.CAM, [bad])
    assert e.value.status == -1
    assert ctx_of(hvo).pnp_ransac(ref.CAM, p, params_of(hvo, c["P"]))[0]["events"]      # the context still works


def test_stream_form_equals_the_host_form(hvo, synth):
    """the frame side resident: match_kf with -1 entries and bad points, features at every octave; the device's compaction in ascending
    frame-feature index gives the host-array form's result bit for bit"""
    g = synth.make_frame("std", 0x5EED0101)[0]
    st = hvo.Stream(depth=2, stages=hvo.STAGE_ORB, bf=0.0)
    try:
        tk = st.submit(g); fr = st.collect(tk)
        kp = fr["kp_un"]; nf = len(kp)
        assert set(np.unique(kp["octave"]).tolist()) >= set(range(8)) and nf > 300
        rng = np.random.RandomState(5)
        scale = np.ones(8, np.float32)
        for i in range(1, 8):
            scale[i] = scale[i - 1] * np.float32(1.2)
        sides, probs = [], []
        for j, (nk, keep) in enumerate(((400, 0.5), (150, 0.9))):
            sc = ref.planted_scene(40 + j, nk)                     # a pose and a depth per key-frame feature
            R = sc["Tcw"].reshape(3, 4)[:, :3]; t = sc["Tcw"].reshape(3, 4)[:, 3]
            match = np.full(nf, -1, np.int32)
            who = np.sort(rng.permutation(nf)[:nk]); match[who] = rng.permutation(nk)
            match[who[rng.rand(nk) > keep]] = -1
            z = rng.uniform(1.0, 4.0, nk); pos = np.zeros((nk, 3), np.float32)
            for i in np.nonzero(match >= 0)[0]:
                m = match[i]
                pc = np.array([(kp["x"][i] - ref.CAM[2]) / ref.CAM[0] * z[m], (kp["y"][i] - ref.CAM[3]) / ref.CAM[1] * z[m], z[m]])
                pos[m] = (R.T @ (pc - t)).astype(np.float32)
            bad = (rng.rand(nk) < 0.1)
            outl = rng.rand(nk) < 0.2; pos[outl] += rng.randn(int(outl.sum()), 3).astype(np.float32)
            sides.append(dict(match_kf=match, pos=pos, bad=bad))
            idx = np.array([i for i in range(nf) if match[i] >= 0 and not bad[match[i]]], np.int32)       # the constructor (:78-101)
            probs.append(dict(p3d=pos[match[idx]], p2d=np.stack([kp["x"][idx], kp["y"][idx]], 1), sigma2=scale[kp["octave"][idx]] * scale[kp["octave"][idx]],
                              feature_index=idx, n_features=nf))
        assert (sides[0]["match_kf"] < 0).any() and sides[0]["bad"].any()
        P = params_of(hvo, ref.default_params(seed=21))
        host = ctx_of(hvo).pnp_ransac(ref.CAM, probs, P, want_sample=True)
        strm = st.pnp_ransac(tk, ref.CAM, sides, P, want_sample=True)
        for j in range(2):
            h, s = host[j], strm[j]
            assert h["N"] == s["N"] == len(probs[j]["p3d"]) and h["T"] == s["T"] > 0 and h["events"]
            for k in ("hyp_sample", "hyp_inliers", "hyp_event", "best_Tcw"):
                assert h[k].tobytes() == s[k].tobytes(), (j, k)
            assert np.array_equal(h["best_inliers"], s["best_inliers"]) and s["n_features"] == nf
            untouched(s, "stream %d" % j)                         # the arrays have the stream's key-point capacity: nothing past the frame's count is written
            assert len(h["events"]) == len(s["events"])
            for a, b in zip(h["events"], s["events"]):
                assert a["Tcw"].tobytes() == b["Tcw"].tobytes() and a["n_inliers"] == b["n_inliers"] and np.array_equal(a["inliers"], b["inliers"])
                assert a["hyp_Tcw"].tobytes() == b["hyp_Tcw"].tobytes() and np.array_equal(a["hyp_inliers"], b["hyp_inliers"])
        assert st.pnp_last_kernel_ms(tk)[0] > 0
    finally:
        st.close()


def test_example_runs(hvo, synth, tmp_path):
    """examples/relocalization_pnp.cpp linked against the library and run on a synthetic sequence: two candidate key frames and the frame to
    relocalise; ComputeBoW, SearchByBoW of both candidates in one call, ONE PnP call, the round-robin iterate(5) replay and PoseOptimization"""
    import os
    import re
    import subprocess
    from conftest import ROOT, PKG_DIR
    csrc = os.path.join(PKG_DIR, "csrc"); exe = str(tmp_path / "relocalization_pnp")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "relocalization_pnp.cpp"),
                           "-L" + csrc, "-lhvo", "-Wl,-rpath," + csrc, "-o", exe])
    g, d, _ = synth.make_sequence("std", 0x5EED7100, 3)
    args = []
    for i in range(3):
        g[i].tofile(tmp_path / ("g%d.u8" % i)); d[i].tofile(tmp_path / ("d%d.u16" % i))
        args += [str(tmp_path / ("g%d.u8" % i)), str(tmp_path / ("d%d.u16" % i))]
    out = subprocess.check_output([exe] + args).decode()
    print(out)
    m = re.search(r"candidate (\d+) at iteration (\d+): PnP (\d+) inliers, PoseOptimization (\d+) good", out)
    assert m and re.search(r"relocalised against candidate \d+", out), out
    assert int(m.group(3)) > 10 and int(m.group(4)) >= 10, out
