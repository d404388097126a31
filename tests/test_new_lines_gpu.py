"""LocalMapping::CreateNewMapLinesConstraint on the GPU (csrc/line_triang.hip) against tests/new_lines_ref.py.  Integers are compared exactly,
floats by their bits (a NaN by being one).  tests/test_new_lines.py asserts on the CPU that every crafted case says what it is meant to say
and that the random scene (seed new_lines_ref.SCENE_SEED) is not vacuous.  The restatement runs the sequential loops; the device evaluates
independent triples and resolves."""
import numpy as np
import pytest

import new_lines_ref as ref

pytestmark = pytest.mark.gpu
PAIR_INT = ("outcome", "created_idx0", "created_idx1", "created_idx2")
PAIR_SCALAR = ("kf2", "kf3", "mv2", "mv3", "n_created", "status")
_cache = {}


def ctx_of(hvo):
    if "ctx" not in _cache:
        _cache["ctx"] = hvo.Context(max_batch=1)
    return _cache["ctx"]


def scene():
    """the random scene, 200 lines x 4 neighbours, and the restatement's answer, computed once"""
    if "scene" not in _cache:
        cur, kfs = ref.random_scene()
        _cache["scene"] = (cur, kfs, ref.full(cur, kfs))
    return _cache["scene"]


def same_bits(a, b):
    a = np.asarray(a, np.float32); b = np.asarray(b, np.float32)
    n = np.isnan(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), n) and np.array_equal(a[~n].view(np.uint32), b[~n].view(np.uint32))


def same(got, want, what=""):
    (gm, gp, gs), (wm, wp, ws) = got, want
    assert len(gm) == len(wm) and len(gp) == len(wp), (what, len(gm), len(wm), len(gp), len(wp))
    for j, (g, w) in enumerate(zip(gm, wm)):
        assert np.array_equal(g["match_idx"], w["match_idx"]), (what, "match_idx", j, np.flatnonzero(np.asarray(g["match_idx"]) != w["match_idx"])[:8])
        assert (g["n_matched"], g["gate"]) == (w["n_matched"], w["gate"]), (what, j, g["n_matched"], w["n_matched"], g["gate"], w["gate"])
    for p, (g, w) in enumerate(zip(gp, wp)):
        for k in PAIR_SCALAR:
            assert g[k] == w[k], (what, p, k, g[k], w[k])
        for k in PAIR_INT:
            assert np.array_equal(g[k], w[k]), (what, p, k, np.flatnonzero(np.asarray(g[k]) != np.asarray(w[k]))[:8] if len(g[k]) == len(w[k]) else (len(g[k]), len(w[k])),
                                                [ (int(a), int(b)) for a, b in zip(g[k], w[k]) if a != b ][:8])
        assert same_bits(g["line3d"], w["line3d"]), (what, p, "line3d", np.flatnonzero((g["line3d"] != w["line3d"]).any(axis=1))[:8])
    assert np.array_equal(gs["owner_pair"], ws["owner_pair"]) and gs["n_new"] == ws["n_new"] and gs["n_pairs"] == ws["n_pairs"], (what, "summary")


def identical(a, b, what=""):
    (am, ap, asum), (bm, bp, bsum) = a, b
    assert len(am) == len(bm) and len(ap) == len(bp), what
    for x, y in zip(am, bm):
        assert x["match_idx"].tobytes() == y["match_idx"].tobytes() and (x["n_matched"], x["gate"]) == (y["n_matched"], y["gate"]), what
    for x, y in zip(ap, bp):
        for k in PAIR_INT + ("line3d",):
            assert x[k].tobytes() == y[k].tobytes(), (what, k)
        assert all(x[k] == y[k] for k in PAIR_SCALAR), what
    assert asum["owner_pair"].tobytes() == bsum["owner_pair"].tobytes() and (asum["n_new"], asum["n_pairs"]) == (bsum["n_new"], bsum["n_pairs"]), what


def untouched(hvo, m, p, s):
    U = hvo.NL_UNTOUCHED
    for x in m:
        assert len(x["match_idx"]) > 0 and (x["match_idx"] == U).all() and x["n_matched"] == x["gate"] == U
    for x in p:
        for k in PAIR_INT + ("line3d",):
            assert len(x[k]) > 0 and (x[k] == U).all(), k
        assert all(x[k] == U for k in PAIR_SCALAR)
    assert (s["owner_pair"] == U).all() and s["n_new"] == s["n_pairs"] == U


def run(hvo, cur, kfs, **kw):
    return ctx_of(hvo).create_new_map_lines(cur, kfs, **kw)


def both(hvo, cur, kfs, what, **kw):
    got = run(hvo, cur, kfs, **kw)
    same(got, ref.full(cur, kfs, **kw), what)
    return got


@pytest.mark.parametrize("pairing", [ref.AS_WRITTEN, ref.ALIGNED])
def test_crafted_cases(hvo, pairing):
    seen = set()
    for name, cur, kfs, want in ref.full_call_cases() + ref.bound_cases():
        m, p, s = both(hvo, cur, kfs, name, pairing=pairing)
        assert int(p[0]["outcome"][0]) == want, (name, int(p[0]["outcome"][0]))
        seen.add(want)
    m, p, s = both(hvo, *ref.nan_overlap_scene(), "NaN overlap ratios", pairing=pairing)
    assert int(p[0]["outcome"][0]) == ref.CREATED and s["n_new"] == 1
    for sc in (ref.gated_middle_scene, ref.idx_range_scene):
        cur, kfs = sc()
        m, p, s = both(hvo, cur, kfs, sc.__name__, pairing=pairing)
        assert (p[0]["kf2"], p[0]["kf3"], p[0]["mv2"], p[0]["mv3"]) == ((0, 1, 0, 2) if pairing == ref.AS_WRITTEN else (0, 2, 0, 2))
        assert s["n_new"] == (0 if pairing == ref.AS_WRITTEN else 1)
    assert int(run(hvo, *ref.idx_range_scene(), pairing=ref.AS_WRITTEN)[1][0]["outcome"][0]) == ref.IDX_RANGE
    seen.add(int(run(hvo, *ref.idx_range_scene(), pairing=pairing)[1][0]["outcome"][0]))
    for cur, kfs, want in ref.occupied_shift_scenes():
        m, p, s = both(hvo, cur, kfs, "occupied, shifted", pairing=pairing)
        assert int(p[0]["outcome"][0]) == (want if pairing == ref.AS_WRITTEN else ref.CREATED)
        seen.add(int(p[0]["outcome"][0]))
    # the exact set of codes the DEVICE returned: every code but the two that no call reaches; the three a shifted pair alone reaches need AS_WRITTEN
    shifted = {ref.IDX_RANGE, ref.OCCUPIED_2, ref.OCCUPIED_3}
    assert seen == set(range(ref.N_CODES)) - {ref.OCCUPIED_1, ref.W_ZERO_E} - (set() if pairing == ref.AS_WRITTEN else shifted), sorted(seen)


def test_crafted_searches(hvo):
    """the search cases through the whole call: the same descriptors on both neighbours, lines that triangulate to nothing"""
    cases = [(n, d1, d2, h1, h2, th, nr, w) for n, d1, d2, h1, h2, th, nr, w in ref.search_cases()]
    d1, d2, th, w = ref.ratio_case(); cases.append(("ratio", d1, d2, np.zeros(3, np.uint8), np.zeros(6, np.uint8), th, 0.85, w))
    for d1, d2, w in ref.mad_cases(): cases.append(("mad", d1, d2, np.zeros(5, np.uint8), np.zeros(10, np.uint8), 80, 0.85, w))
    for name, d1, d2, h1, h2, th, nr, want in cases:
        rows = lambda ds, hs: [(10.0 + 9 * i, 20.0, 60.0 + 9 * i, 200.0, 0, d, int(h)) for i, (d, h) in enumerate(zip(ds, hs))]
        cur = ref.side(rows(d1, h1)); kfs = [ref.side(rows(d2, h2), Tcw=ref.T_R), ref.side(rows(d2, h2), Tcw=ref.T_L)]
        m, p, s = both(hvo, cur, kfs, name, th_high=th, nn_ratio=nr)
        assert m[0]["match_idx"].tolist() == want == m[1]["match_idx"].tolist(), (name, m[0]["match_idx"])


def test_random_scene_and_stream_form(hvo, synth):
    cur, kfs, want = scene()
    got = run(hvo, cur, kfs)
    same(got, want, "random scene")
    assert got[2]["n_new"] > 50 and sum(k > 0 for k in got[2]["kernel_ms"]) == 3
    same(run(hvo, cur, kfs, pairing=ref.ALIGNED), ref.full(cur, kfs, pairing=ref.ALIGNED), "random scene, aligned")
    # the current key frame resident: a streamed frame's lines against neighbours made from them
    cam = (535.4, 539.2, 320.1, 247.6)
    g, d = synth.make_frame("std", 0x5EED0171)
    st = hvo.Stream(depth=2, stages=hvo.STAGE_LSD)
    try:
        tk = st.submit(g, d); fr = st.collect(tk)
        n = len(fr["kl"])
        assert n > 60
        has = (np.arange(n) % 5 == 0).astype(np.uint8)
        kfs2 = ref.neighbours_of_frame(fr["kl"], fr["ldesc"], ref.SCENE_POSES[:3], cam, 171)
        cur2 = dict(kl=fr["kl"], linefn=fr["linefn"], desc=fr["ldesc"], has_map_line=has, Tcw=ref.IDENTITY, cam=cam)
        w2 = ref.full(cur2, kfs2)
        assert w2[2]["n_new"] > 5 and w2[2]["n_pairs"] == 3
        strm = st.create_new_map_lines(tk, cam, ref.IDENTITY, has, kfs2)
        host = run(hvo, cur2, kfs2)
        identical(strm, host, "stream")
        same(strm, w2, "stream")
        identical(strm, st.create_new_map_lines(tk, cam, ref.IDENTITY, has, kfs2), "stream twice")
        rc, msg, m, p, s = st.create_new_map_lines(tk, cam, ref.IDENTITY, has, kfs2, th_high=256, check=False)
        assert rc == -1 and "th_high" in msg
        untouched(hvo, m, p, s)
    finally:
        st.close()
    st = hvo.Stream(depth=2, stages=hvo.STAGE_ORB)
    try:
        tk = st.submit(g, d); st.collect(tk)
        rc, msg, m, p, s = st.create_new_map_lines(tk, cam, ref.IDENTITY, np.zeros(4, np.uint8), kfs[:2], check=False)
        assert rc == -1 and "create new map lines" in msg and "LSD stage" in msg, msg
        untouched(hvo, m, p, s)
    finally:
        st.close()


@pytest.mark.parametrize("n1", [1, 2, 63, 64, 65, 255, 256, 257])
def test_current_line_counts(hvo, n1):
    """a wave, and the epilogue's block, on either side"""
    cur, kfs = ref.random_scene(n=max(n1, 2) if n1 < 60 else n1, seed=40 + n1, poses=ref.SCENE_POSES[:3])
    cur = ref.cut(cur, n1)
    m, p, s = both(hvo, cur, kfs, "n1 = %d" % n1)
    assert s["n_pairs"] == 3 and (n1 < 60 or s["n_new"] > 0)


def test_neighbour_line_counts_and_neighbour_counts(hvo):
    cur, kfs = ref.random_scene(n=40, seed=51, poses=ref.SCENE_POSES)
    rag = [ref.cut(kfs[0], 0), ref.cut(kfs[1], 1), ref.cut(kfs[2], 2), kfs[3]]
    m, p, s = both(hvo, cur, rag, "neighbours of 0, 1, 2 and 40 lines")
    assert [x["n_matched"] for x in m[:2]] == [0, 0] and s["n_pairs"] == 6
    m, p, s = both(hvo, cur, kfs[:2], "exactly 2 neighbours")
    assert s["n_pairs"] == 1 and s["n_new"] > 0
    m, p, s = both(hvo, cur, kfs[:1], "one neighbour")
    assert s["n_pairs"] == 0 and s["n_new"] == 0 and m[0]["gate"] == 0 and (m[0]["match_idx"] == -1).all()
    gated = [dict(k, skip=1) for k in kfs[:3]] + [kfs[3]]
    m, p, s = both(hvo, cur, gated, "all gated but one")
    assert s["n_pairs"] == 0 and s["n_new"] == 0 and [x["gate"] for x in m] == [1, 1, 1, 0] and (s["owner_pair"] == -1).all()
    m, p, s = both(hvo, ref.cut(cur, 0), kfs, "no current lines")
    assert s["n_pairs"] == 0 and s["n_new"] == 0
    # 16 neighbours of 8 lines: 120 pairs
    poses = [(ref.yaw(0.01 * (k % 3)), (0.2 * np.cos(k * 0.39), 0.2 * np.sin(k * 0.39), 0.01 * k)) for k in range(16)]
    cur8, kfs8 = ref.random_scene(n=8, seed=52, poses=poses, occupied=0.0, spare=0.0)
    m, p, s = both(hvo, cur8, kfs8, "16 neighbours")
    assert s["n_pairs"] == 120 and len(p) == 120 and s["n_new"] > 0 and (p[119]["kf2"], p[119]["kf3"]) == (14, 15)


def test_refusals_leave_the_outputs_untouched(hvo):
    cur, kfs = ref.random_scene(n=16, seed=53, poses=ref.SCENE_POSES[:2])
    ctx = ctx_of(hvo)
    fat = ref.side([(1.0, 2.0, 3.0, 4.0, 0, ref.BASE, 0)] * (ref.MAX_LINES + 1), Tcw=ref.T_R)
    for c, k, kw, code, word in ((cur, [kfs[0]] * 17, {}, -4, "17 neighbours"), (cur, [kfs[0], fat], {}, -4, "2049"), (fat, kfs, {}, -4, "2049"),
                                 (cur, kfs, dict(th_high=256), -1, "th_high"), (cur, kfs, dict(n_levels=0), -1, "n_levels"), (cur, kfs, dict(pairing=2), -1, "pairing"),
                                 (cur, kfs * 2, dict(n_pairs_cap=5), -1, "6 pairs")):
        rc, msg, m, p, s = ctx.create_new_map_lines(c, k, check=False, **kw)
        assert rc == code and word in msg, (word, rc, msg)
        untouched(hvo, m, p, s)
    for missing in ("kl", "linefn", "desc", "has_map_line"):
        rc, msg, m, p, s = ctx.create_new_map_lines(cur, [kfs[0], dict(kfs[1], n=len(kfs[1]["kl"]), **{missing: None})], check=False)
        assert rc == -1 and "neighbour 1" in msg, (missing, msg)
        untouched(hvo, m, p, s)
    rc, msg, m, p, s = ctx.create_new_map_lines(dict(cur, n=len(cur["kl"]), desc=None), kfs, check=False)
    assert rc == -1 and "current key frame" in msg
    untouched(hvo, m, p, s)
    assert run(hvo, cur, kfs)[1][0]["status"] == 0                      # and the context goes on working


def _leftovers(hvo, ctx):
    """a frame_bf_match and a local-map line search on the same context: their staging is what the next call finds"""
    rng = np.random.RandomState(3)
    d1 = rng.randint(0, 256, (300, 32)).astype(np.uint8); d2 = rng.randint(0, 256, (280, 32)).astype(np.uint8)
    ctx.frame_bf_match(d1, d2, 80.0, 0.85, True)
    nq, nt = 6, 12
    ctx.search_lines_by_projection_map(rng.uniform(0, 400, (nq, 4)), np.ones(nq, np.float32), rng.normal(size=(nq, 3)), d1[:nq], None, np.zeros(nt, hvo.KEYLINE_DT),
                                       np.zeros((nt, 3)), np.zeros(nt, hvo.LINE3D_DT), d2[:nt], None, np.zeros(64 * 48 + 1, np.int32), np.zeros(0, np.int32), (0.0, 640.0, 0.0, 480.0))


@pytest.mark.parametrize("fill", [0x00, 0xFF, 0x7F])
def test_dirty_matching_arena(hvo, fill):
    """the census's three conditions for this site: a pre-filled arena (proven by peeking), the same call's and other calls' leftovers (the
    older matchers of match.hip among them, which share the context's call arena), a regrowth"""
    ctx = hvo.Context(max_batch=1)
    try:
        cur, kfs, want = scene()
        S = (ref.cut(cur, 50), [ref.cut(k, 60) for k in kfs[:3]])
        wS = ref.full(*S)
        assert wS[2]["n_new"] > 0
        cap = ctx.debug_call_arena(fill, 120000)
        assert cap >= 120000 and (ctx.debug_call_arena_peek(0, cap) == fill).all()
        first = ctx.create_new_map_lines(*S)
        same(first, wS, "S on a filled arena")
        assert ctx.debug_call_arena(None) == cap                      # S fits: no regrowth so far
        for k in range(2):
            identical(ctx.create_new_map_lines(*S), first, "S again")
        ctx.debug_call_arena(fill)
        L = ctx.create_new_map_lines(cur, kfs)                          # grows the arena
        same(L, want, "L")
        cap2 = ctx.debug_call_arena(None)
        assert cap2 > cap
        identical(ctx.create_new_map_lines(*S), first, "S after L")
        identical(ctx.create_new_map_lines(cur, kfs), L, "L after S")
        _leftovers(hvo, ctx)
        identical(ctx.create_new_map_lines(*S), first, "S after other calls")
        ctx.debug_call_arena(fill)
        assert (ctx.debug_call_arena_peek(cap2 - 4096, 4096) == fill).all()
        identical(ctx.create_new_map_lines(*S), first, "S on the regrown, filled arena")
    finally:
        ctx.close()


def test_example_runs(hvo, tmp_path):
    """examples/create_map_lines.cpp linked against the library: the call and the host walk on its toy map print the created list the
    restatement gives for the same toy map"""
    import os
    import re
    import subprocess
    from conftest import ROOT, PKG_DIR
    csrc = os.path.join(PKG_DIR, "csrc"); exe = str(tmp_path / "create_map_lines")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "create_map_lines.cpp"),
                           "-L" + csrc, "-lhvo", "-Wl,-rpath," + csrc, "-o", exe])
    out = subprocess.check_output([exe]).decode()
    print(out)
    got = [tuple(int(v) for v in t) for t in re.findall(r"pair (\d+) \(key frames (\d+), (\d+)\): line (\d+) with (\d+) and (\d+)", out)]
    cur, kfs = ref.toy_map()
    m, p, s = ref.full(cur, kfs)
    want = [(q, x["kf2"], x["kf3"], int(a), int(b), int(c)) for q, x in enumerate(p) for a, b, c in zip(x["created_idx0"], x["created_idx1"], x["created_idx2"])]
    assert got == want and len(want) >= 3 and len({w[0] for w in want}) >= 2, (got, want)
    assert re.search(r"created %d new map lines" % s["n_new"], out)
