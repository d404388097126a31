"""The three guided line searches on the device (csrc/line_track.inc: k_lsbp_keys + k_lsbp_epilogue, k_lines_geom_gate; csrc/line_map.inc:
k_lsbp_map_keys + k_lsbp_map_epilogue; csrc/local_lines.hip on top of the latter) on the hand-built cases of tests/line_search_cases.py.

Each case goes through every entry point that can express it -- hvo_search_lines_by_projection_map, hvo_search_lines_by_projection,
hvo_match_lines_geom, and hvo_search_local_lines for the crowded-window, claim-chain and 2048-line cases -- and is compared, integers with
array_equal and no tolerance anywhere, with the CPU restatement / the oracle AND with the expectation the case states by hand (which
tests/test_line_search_edges.py has checked against those references without a device).  Every call is made twice and must return the same bytes.

What the cases reach that lines extracted from synthetic frames do not: the fallback of k_lsbp_map_epilogue with the ratio rule passing and
rejecting inside it, the four smallest keys of k_lsbp_map_keys in one lane / four lanes / across the 64-line chunks at 0 .. 130 candidates,
ties whose visit order disagrees with their index order, lines that pass only at a later sample point, repeated grid items, the last
occupancy word at 2048 lines, t_occupied on the last of 63 / 64 / 65 lines, 64 / 65 / 129 / 16384 queries, windows off every edge and under
non-zero minimum bounds, zero-length lines, and the boundary value of every gate."""
import ctypes as C

import numpy as np
import pytest

import line_map_ref as lmr
import line_search_cases as lc
import local_map_lines_ref as ref

gpu = pytest.mark.gpu
UNSUPPORTED = -4


@pytest.fixture(scope="module")
def cases(hvo):
    return lc.build_all(hvo)


@pytest.fixture(scope="module")
def references(orc, cases):
    """every case through its CPU reference, once (tests/test_line_search_edges.py checks these against the hand-stated expectations)"""
    out = {}
    for name, c in cases.items():
        for mode in c.expect:
            if mode == "map": out[name, mode] = ref.search_lines_by_projection_map(*lc.args_map(c))
            elif mode == "last": out[name, mode] = orc.search_lines_by_projection(*lc.args_last(c))
            else:
                a = lc.args_geom(c)
                out[name, mode] = orc.lines_geom_match(*a[:5], desc_th=a[5], last_has_mapline=a[6])
    return out


def device(ctx, c, mode):
    if mode == "map":
        a = lc.args_map(c)
        return ctx.search_lines_by_projection_map(*a[:13], th=a[13], nn_ratio=a[14])
    if mode == "last":
        return ctx.search_lines_by_projection(*lc.args_last(c))
    a = lc.args_geom(c)
    return ctx.match_lines_geom(*a[:5], desc_th=a[5], last_has_mapline=a[6])


def as_bytes(r):
    return (int(r[0]), r[1].tobytes(), r[2].tobytes())


@gpu
@pytest.mark.parametrize("name", lc.CASES)
def test_line_search_case(gpu_ctx, cases, references, name):
    c = cases[name]
    for mode, (en, e1, e2) in c.expect.items():
        r = device(gpu_ctx, c, mode)
        n, a1, a2 = r
        no, o1, o2 = references[name, mode]
        bad = np.flatnonzero(a1 != o1)
        assert len(bad) == 0, (mode, bad[:8], a1[bad[:8]], o1[bad[:8]])
        assert np.array_equal(a2, o2) and n == no, (mode, n, no, np.flatnonzero(a2 != o2)[:8])
        assert np.array_equal(a1, e1) and np.array_equal(a2, e2) and n == en, mode          # and what the case states by hand
        assert as_bytes(device(gpu_ctx, c, mode)) == as_bytes(r), mode                       # the second run returns the same bytes


def upload(hvo, M):
    lm = hvo.LineMap(slots=0)
    lm.set_many(0, M["pos"], M["wvec"], M["normal"], M["max_dist"], M["min_dist"], M["desc"], M["observed"], M["bad"])
    return lm


@gpu
@pytest.mark.parametrize("name", lc.LOCAL)
def test_line_search_case_on_the_resident_map(hvo, gpu_ctx, cases, name):
    """hvo_search_local_lines over the crafted current frame: a resident map made of the frame's own 3-D lines (lc.local_map), against the
    restatement of the whole call; and that restatement's queries through the host-array core give the same matches"""
    c = cases[name]; t = c.t; th = c.local.th
    M, T, held = lc.local_map(c)
    o = lmr.search_local_lines(M, lmr.CAM, T, lmr.BOUNDS, lmr.LOG_SF, th, 0.95, t.kl, t.fn, t.l3d, t.desc, c.cs, c.ci, held)
    lm = upload(hvo, M)
    try:
        run = lambda: gpu_ctx.search_local_lines(lm, lmr.CAM, T, t.kl, t.fn, t.l3d, t.desc, c.cs, c.ci, lmr.BOUNDS, held=held, log_scale_factor=lmr.LOG_SF, th=th)
        r = run()
        assert (r.n_slots_tested, r.n_in_view, r.n_matches, r.n_gated, r.status) == (o["n_slots_tested"], o["n_in_view"], o["n_matches"], o["n_gated"], 0)
        assert r.n_in_view == c.local.nslots and r.n_matches >= 3
        assert np.array_equal(r.in_view_slot, o["in_view_slot"])
        assert np.array_equal(r.proj.view(np.uint32), o["proj"].view(np.uint32)) and np.array_equal(r.view_cos.view(np.uint32), o["view_cos"].view(np.uint32))
        assert np.array_equal(r.match_idx, o["match_idx"]) and np.array_equal(r.match_dist, o["match_dist"]), np.flatnonzero(r.match_idx != o["match_idx"])[:8]
        assert np.array_equal(r.held, o["held"]) and np.array_equal(r.level, o["level"])
        r2 = run()
        for key in ("held", "in_view_slot", "proj", "view_cos", "level", "match_idx", "match_dist"):
            assert getattr(r2, key).tobytes() == getattr(r, key).tobytes(), key
        fp = lmr.frustum_pass(M, lmr.CAM, T, lmr.BOUNDS, lmr.LOG_SF, held); q = lmr.queries(M, fp)
        nm, mi, md = gpu_ctx.search_lines_by_projection_map(q[0], q[1], q[2], q[3], q[4], t.kl, t.fn, t.l3d, t.desc, fp["t_occupied"], c.cs, c.ci,
                                                            np.array(lmr.BOUNDS, np.float32), th=th)
        assert nm == r.n_matches and np.array_equal(mi, r.match_idx) and np.array_equal(md, r.match_dist)
    finally:
        lm.close()


def raw_call(hvo, ctx, c, mode, nq, nt):
    """the C entry point on the case's first nq queries and nt lines (repeated round and round past the end), into caller arrays pre-filled with 77"""
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    rep = lambda a, n: None if a is None else np.ascontiguousarray(np.resize(a, (n,) + a.shape[1:]))
    t = c.t
    mi = np.full(nq, 77, np.int32); md = np.full(nq, 77, np.int32); n = C.c_int(77)
    b = np.ascontiguousarray(c.bounds, np.float32)
    if mode == "map":
        m = c.map
        qa = [rep(a, nq) for a in (m.q, m.vc, m.wvec, m.desc, m.blocks)]; ta = [rep(a, nt) for a in (t.kl, t.fn, t.l3d, t.desc, t.occ)]
        rc = hvo.lib().hvo_search_lines_by_projection_map(ctx.h, nq, *[p(a) for a in qa], *[p(a) for a in ta], nt, p(c.cs), p(c.ci), p(b), m.th, m.nn_ratio,
                                                          p(mi), p(md), C.byref(n))
    else:
        m = c.last
        occ = np.zeros(len(t.kl), np.uint8) if t.occ is None else t.occ
        qa = [rep(a, nq) for a in (m.q, m.kl, m.desc, m.blocks)]; ta = [rep(a, nt) for a in (t.kl, t.fn, t.desc, occ)]
        rc = hvo.lib().hvo_search_lines_by_projection(ctx.h, nq, *[p(a) for a in qa], *[p(a) for a in ta], nt, p(c.cs), p(c.ci), p(b), m.th,
                                                      p(mi), p(md), C.byref(n))
    return rc, n.value, mi, md


@gpu
def test_one_past_the_limits_is_refused(hvo, gpu_ctx, cases):
    """2049 current lines (both searches) and 16385 queries (the local-map search): the library's unsupported error before anything is written
    to the caller's arrays; the same calls at the limits run and give what the cases state"""
    wide, many = cases["nt_2048_last"], cases["nq_16384"]
    for c, mode, nq, nt in ((wide, "map", 2, lc.MAXT + 1), (wide, "last", 2, lc.MAXT + 1), (many, "map", lc.MAXQ + 1, 8), (many, "map", lc.MAXQ + 1, lc.MAXT + 1)):
        rc, n, mi, md = raw_call(hvo, gpu_ctx, c, mode, nq, nt)
        assert rc == UNSUPPORTED and n == 77 and np.all(mi == 77) and np.all(md == 77), (mode, nq, nt, rc)
    for c, mode, nq, nt in ((wide, "map", 2, lc.MAXT), (wide, "last", 2, lc.MAXT), (many, "map", lc.MAXQ, 8)):
        rc, n, mi, md = raw_call(hvo, gpu_ctx, c, mode, nq, nt)
        en, eidx, edist = c.expect[mode]
        assert rc == 0 and n == en and np.array_equal(mi, eidx) and np.array_equal(md, edist), (mode, nq, nt, rc)
