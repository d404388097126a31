"""The guided ORB search (csrc/match.hip: k_search_by_projection, k_sbp_epilogue) on crafted windows, ties and overflow paths.

The inputs come from tests/guided_cases.py: key points written by hand, descriptors at chosen Hamming distances.  Each case is compared bit
for bit -- match count, match_idx, and match_dist where match_idx >= 0 -- with the CPU oracle (oracle/match.c) through every host-array
entry point that can express it (hvo_search_by_projection with and without the rotation check, hvo_search_by_projection_map,
hvo_search_by_projection_tracked).  The oracle's answer is first checked against the expectation the case states by hand, so oracle and
kernel cannot be wrong together; test_cases_hold_without_a_gpu does that, and checks the path properties, without a device.

What the cases reach that ORB features of a shifted synthetic frame do not: the claim chain through the 16 ranked keys into the rescan (both
modes, with t_occupied and non-blocking queries), list compaction (first at nt = 513, twice at nt = 1000), distance ties whose index order
and grid traversal order disagree, bounds with a negative minimum and windows off every edge, non-finite queries, every boundary value of
the window / stereo / threshold / ratio / level tests, ComputeThreeMaxima's ratios and tie rules, and the size limits."""
import ctypes as C

import numpy as np
import pytest

import guided_cases as gc

gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases(hvo):
    return gc.build_all(hvo.KEYPOINT_DT)                      # the builders assert their own path properties


def _modes(c):
    return [m for m in ("last", "rot", "map") if m in c.expect]


def _oracle(orc, c, mode):
    sel = c.oracle_mask
    if mode == "map":
        return orc.search_by_projection_map(*gc.args_map(c, sel), th_high=c.th_high, nn_ratio=c.nn_ratio)
    return orc.search_by_projection(*gc.args_last(c, sel), th_high=c.th_high, check_orientation=(mode == "rot"))


@pytest.fixture(scope="module")
def oracle_results(orc, cases):
    """every case through the oracle, once, checked against what the case states by hand"""
    out = {}
    for name, c in cases.items():
        for mode in _modes(c):
            n, idx, dist = _oracle(orc, c, mode)
            en, eidx, edist = c.expect[mode]
            sel = c.oracle_mask
            assert np.all(eidx[~sel] == -1), name                         # by hand: a non-finite or huge query matches nothing
            assert np.array_equal(idx, eidx[sel]), (name, mode, np.flatnonzero(idx != eidx[sel])[:8])
            assert np.array_equal(dist[idx >= 0], edist[sel][idx >= 0]) and n == en == int((idx >= 0).sum()), (name, mode)
            out[name, mode] = (n, idx, dist)
    return out


def test_cases_hold_without_a_gpu(orc, cases, oracle_results):
    """path properties and hand-stated expectations of every case, on the oracle alone"""
    assert {c.props["ncomp"] for n, c in cases.items() if len(c.t.kp) == 100} == {0}
    for nt in gc.CHAIN_NT:
        for best in ("first64", "last64", "spread"):
            c = cases["chain%d_%s" % (nt, best)]
            assert c.props["ncomp"] == gc.NCOMP[nt] and len(c.t.kp) == nt
            S = np.sort(c.props["order"][:16])
            if best == "first64":
                assert S.max() < 64
            elif best == "last64":
                assert S.min() >= nt - 64
            elif nt > 512:
                assert S.min() < 512 <= S.max() and (nt < 1000 or (S < 960).sum() in range(9, 16))
            d16 = gc.ham(c.q.desc[:1], c.t.desc[S])[0]
            assert len(set(d16.tolist())) < 16                            # ties among the best keys
    # where the chain leaves the ranked keys: the model counts the free ranked keys at each query's turn
    for name, first_last, first_map in (("chain100", 16, 15), ("chain100_marks", 2 + 14, 2 + 13)):
        c = cases[name]
        for mode, first in (("last", first_last), ("map", first_map)):
            n, idx, dist, st = gc.model_search(c, mode)
            assert np.array_equal(idx, c.expect[mode][1]) and np.array_equal(idx, oracle_results[name, mode][1])
            assert int(np.flatnonzero(st.rescan)[0]) == first and st.rescan[first:].all() and not st.rescan[:first].any()
    c = cases["chain100"]; idx = c.expect["map"][1]
    assert c.props["same_at"] == (21, 37) and idx[20] == c.props["order"][20] and np.all(idx[15:36] >= 0) and np.all(idx[36:] == -1)   # rescanned: ratio test passes and fails
    assert np.array_equal(c.expect["last"][1], c.props["order"][:40])
    c = cases["chain100_free3"]; idx = c.expect["last"][1]
    assert np.array_equal(idx[2::3], idx[3::3][: len(idx[2::3])]) and len(set(idx.tolist())) == 40 - 13
    c = cases["chain100_occupied"]
    assert not set(c.expect["last"][1].tolist()) & set(c.props["order"][[0, 3, 4, 17]].tolist())
    # the model agrees with the oracle on every other modelled case too
    for name in ("ties", "grid_bounds", "boundaries", "complement", "dense", "dense_tracked_1", "dense_tracked_4", "chain1000_spread", "chain513_first64"):
        c = cases[name]
        for mode in (m for m in _modes(c) if m != "rot"):
            n, idx, dist, st = gc.model_search(c, mode)
            assert n == oracle_results[name, mode][0] and np.array_equal(idx[c.oracle_mask], oracle_results[name, mode][1]), (name, mode)
    for name in ("dense_tracked_1", "dense_tracked_4"):                   # the windows are what the tracked prologue derives
        c = cases[name]; k = c.tracked
        r, lo, hi = orc.track_windows(k.level, k.view_cos, k.th, gc.SF)
        assert np.array_equal(r, c.q.r) and np.array_equal(lo, c.q.lo) and np.array_equal(hi, c.q.hi)
        assert (k.view_cos.astype(np.float64) > 0.998).any() and (k.view_cos.astype(np.float64) <= 0.998).any()
    for r in gc.ROTATION:                                                 # the cull removed something, the unculled run keeps everything
        assert oracle_results[r[0], "rot"][0] < oracle_results[r[0], "last"][0] == len(cases[r[0]].q.u) - 1
    assert cases["rot_20_2_1"].expect["rot"][0] == 22 and cases["rot_20_1_1"].expect["rot"][0] == 20


CASES = (["chain100", "chain100_marks", "chain100_occupied", "chain100_free3", "chain100_occupied_free3"]
         + ["chain%d_%s" % (nt, b) for nt in gc.CHAIN_NT for b in ("first64", "last64", "spread")]
         + ["ties", "grid_bounds", "boundaries", "complement"] + [r[0] for r in gc.ROTATION]
         + ["nq1_nt1", "nq1_nt0", "dense", "dense_tracked_1", "dense_tracked_4", "nq_16384", "nt_65535"])


def test_case_list_is_complete(cases):
    assert sorted(CASES) == sorted(cases)


@gpu
@pytest.mark.parametrize("name", CASES)
def test_guided_case(gpu_ctx, cases, oracle_results, name):
    c = cases[name]
    sel = c.oracle_mask
    runs = []
    for mode in _modes(c):
        if mode == "map":
            runs.append((mode, "map", gpu_ctx.search_by_projection_map(*gc.args_map(c), th_high=c.th_high, nn_ratio=c.nn_ratio)))
            if c.tracked is not None:
                runs.append((mode, "tracked", gpu_ctx.search_by_projection_tracked(*gc.args_tracked(c), th_high=c.th_high, nn_ratio=c.nn_ratio)))
        else:
            runs.append((mode, mode, gpu_ctx.search_by_projection(*gc.args_last(c), th_high=c.th_high, check_orientation=(mode == "rot"))))
    for mode, entry, (n, idx, dist) in runs:
        no, io, do = oracle_results[name, mode]
        bad = np.flatnonzero(idx[sel] != io)
        assert len(bad) == 0, (entry, bad[:8], idx[sel][bad[:8]], io[bad[:8]])
        assert np.array_equal(dist[sel][io >= 0], do[io >= 0]), entry
        assert np.all(idx[~sel] == -1) and n == no, (entry, n, no)         # non-finite and huge queries: nothing, and nobody else disturbed
        assert np.array_equal(idx, c.expect[mode][1]), entry


def _raw_call(hvo, ctx, c, nq, nt):
    """hvo_search_by_projection / _map on the first nq queries and nt features of c, into caller-owned outputs pre-filled with 77"""
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    q, t = c.q, c.t
    rep = lambda a, n: np.ascontiguousarray(np.resize(a, (n,) + a.shape[1:]))
    qa = [rep(a, nq) for a in (q.desc, q.u, q.v, q.r, q.lo, q.hi, q.ur, q.angle, q.blocks)]
    ta = [rep(a, nt) for a in (t.kp, t.uright, t.occ, t.desc)]
    out = []
    for map_mode in (False, True):
        mi = np.full(nq, 77, np.int32); md = np.full(nq, 77, np.int32); n = C.c_int(77)
        b = [float(v) for v in c.bounds]
        if map_mode:
            rc = hvo.lib().hvo_search_by_projection_map(ctx.h, p(qa[0]), nq, *[p(a) for a in qa[1:7]], p(qa[8]), p(ta[0]), p(ta[1]), p(ta[2]), p(ta[3]), nt,
                                                        *b, 100, 0.8, p(mi), p(md), C.byref(n))
        else:
            rc = hvo.lib().hvo_search_by_projection(ctx.h, p(qa[0]), nq, *[p(a) for a in qa[1:9]], p(ta[0]), p(ta[1]), p(ta[2]), p(ta[3]), nt,
                                                    *b, 100, 1, p(mi), p(md), C.byref(n))
        out.append((rc, mi, md))
    return out


@gpu
def test_one_past_the_limits_is_refused(hvo, gpu_ctx, cases):
    """nq = 16385 and nt = 65536: the library's unsupported error, before anything is written to the caller's arrays"""
    UNSUPPORTED = -4
    c = cases["nq_16384"]
    for nq, nt in ((gc.MAX_Q + 1, 8), (4, gc.MAX_T + 1), (gc.MAX_Q + 1, gc.MAX_T + 1)):
        for rc, mi, md in _raw_call(hvo, gpu_ctx, c, nq, nt):
            assert rc == UNSUPPORTED and np.all(mi == 77) and np.all(md == 77), (nq, nt, rc)
    for rc, mi, md in _raw_call(hvo, gpu_ctx, c, gc.MAX_Q, 8):               # the same call at the limit runs
        assert rc == 0 and np.array_equal(mi, np.arange(gc.MAX_Q) % 8)
    c = cases["dense_tracked_1"]; t = c.t                                   # the tracked form, through the binding
    big = [np.resize(a, (gc.MAX_T + 1,) + a.shape[1:]) for a in (t.kp, t.uright, t.occ, t.desc)]
    with pytest.raises(hvo.HvoError) as e:
        gpu_ctx.search_by_projection_tracked(*gc.args_tracked(c)[:8], *big, c.bounds)
    assert e.value.status == UNSUPPORTED
