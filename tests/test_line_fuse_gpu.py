"""LSDmatcher::Fuse on the GPU (csrc/line_fuse.hip) against tests/line_fuse_ref.py, the definition.  Every returned field is compared: integers
exactly, floats by their bits (a NaN by being one).  tests/test_line_fuse.py asserts on the CPU that every crafted case says what it is
meant to say and that the random scene is not vacuous.  The restatement runs the sequential loop per entry and per key line and normalises
a key line's direction for every entry; the device forms it once per key frame and sweeps LDS chunks with 16 lanes per entry."""
import numpy as np
import pytest

import line_fuse_ref as ref

pytestmark = pytest.mark.gpu
ARRAYS = ("best_idx", "best_dist", "gate", "level", "fused_entry", "fused_idx", "behind_entry")
SCALARS = ("n_fused", "n_behind", "n_searched", "status")
_cache = {}


def ctx_of(hvo):
    if "ctx" not in _cache:
        _cache["ctx"] = hvo.Context(max_batch=1)
    return _cache["ctx"]


def call(ctx, kfs, mp, **kw):
    """Context.fuse_lines with the restatement's default of three levels (the binding's default is the one octave of the line extractor)"""
    kw.setdefault("n_levels", 3)
    return ctx.fuse_lines(kfs, mp, **kw)


def call_slots(ctx, m, slots, kfs, **kw):
    kw.setdefault("n_levels", 3)
    return ctx.fuse_lines_slots(m, slots, kfs, **kw)


def scene(hvo):
    """the random scene and the restatement's answers under both level rules, computed once"""
    if "scene" not in _cache:
        kfs, mp = ref.random_scene(hvo.KEYLINE_DT)
        _cache["scene"] = (kfs, mp, {rule: [ref.fuse(kf, mp, level_rule=rule) for kf in kfs] for rule in (ref.CLAMPED, ref.AS_WRITTEN)})
    return _cache["scene"]


def same_bits(a, b):
    a = np.asarray(a, np.float32); b = np.asarray(b, np.float32)
    n = np.isnan(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), n) and np.array_equal(a[~n].view(np.uint32), b[~n].view(np.uint32))


def same(got, want, what=""):
    assert len(got) == len(want), (what, len(got), len(want))
    for j, (g, w) in enumerate(zip(got, want)):
        for k in SCALARS:
            assert g[k] == w[k], (what, j, k, g[k], w[k])
        for k in ARRAYS:
            assert len(g[k]) == len(w[k]) and np.array_equal(g[k], w[k]), (what, j, k, len(g[k]), len(w[k]),
                                                                          [(i, int(a), int(b)) for i, (a, b) in enumerate(zip(g[k], w[k])) if a != b][:8])
        assert same_bits(g["proj"], w["proj"]), (what, j, "proj", np.flatnonzero((np.asarray(g["proj"]) != w["proj"]).any(axis=1))[:8])


def identical(a, b, what=""):
    assert len(a) == len(b), what
    for x, y in zip(a, b):
        for k in ARRAYS + ("proj",):
            assert x[k].tobytes() == y[k].tobytes(), (what, k)
        assert all(x[k] == y[k] for k in SCALARS), what


def untouched(hvo, res):
    for r in res if isinstance(res, list) else [res]:
        for k in ARRAYS + ("proj",):
            assert (r[k] == hvo.FUSE_UNTOUCHED).all(), k
        assert all(r[k] == hvo.FUSE_UNTOUCHED for k in SCALARS)


def both(hvo, kfs, mp, what="", **kw):
    """the device call on kfs against the shared map side mp, compared with the restatement"""
    got = call(ctx_of(hvo), kfs, mp, **kw)
    same(got, [ref.fuse(kf, mp, **kw) for kf in kfs], what)
    return got


def test_crafted_gates(hvo):
    kf, mp, want, names = ref.crafted_gates(hvo.KEYLINE_DT)
    g = both(hvo, [kf], mp, "gates", level_rule=ref.CLAMPED)[0]
    assert g["gate"].tolist() == want
    # as written, a searched row whose mfMaxDistance puts its level above the table is gated by the level; the other gates come first
    g = both(hvo, [kf], mp, "gates, as written", level_rule=ref.AS_WRITTEN)[0]
    assert all(a == b or (b == ref.SEARCHED and a == ref.LEVEL) for a, b in zip(g["gate"].tolist(), want))


@pytest.mark.parametrize("n_levels", [1, 3])
def test_crafted_levels(hvo, n_levels):
    kf, mp, lv = ref.crafted_levels(hvo.KEYLINE_DT, n_levels)
    c = both(hvo, [kf], mp, "levels, clamped", log_scale_factor=ref.LOG_11, n_levels=n_levels, level_rule=ref.CLAMPED)[0]
    a = both(hvo, [kf], mp, "levels, as written", log_scale_factor=ref.LOG_11, n_levels=n_levels, level_rule=ref.AS_WRITTEN)[0]
    assert a["level"].tolist() == lv and (c["gate"] == 0).all() and (a["gate"] == ref.LEVEL).sum() == 3


@pytest.mark.parametrize("n_levels", [1, 3])
def test_crafted_searches(hvo, n_levels):
    kf, mp, bi, bd, names = ref.crafted_search(hvo.KEYLINE_DT, n_levels)
    g = both(hvo, [kf], mp, "searches", n_levels=n_levels)[0]
    assert g["best_idx"].tolist() == bi.tolist() and g["best_dist"].tolist() == bd.tolist()
    kf, mp, bi, bd = ref.short_rows(hvo.KEYLINE_DT)
    g = both(hvo, [kf], mp, "short rows")[0]
    assert g["best_idx"].tolist() == bi.tolist()


@pytest.mark.parametrize("n_lines", [0, 1, 63, 64, 65, 200, 2048])
def test_line_counts(hvo, n_lines):
    """a wave's worth, an LDS chunk's worth and the limit, on the key-frame side"""
    kfs, mp = ref.random_scene(hvo.KEYLINE_DT, n_kf=1, n_lines=n_lines, n=40, seed=100 + n_lines)
    g = both(hvo, kfs, mp, "%d lines" % n_lines)[0]
    assert g["n_searched"] > 5 and (n_lines < 63 or g["n_fused"] > 5)


def test_2049_lines_are_refused(hvo):
    kfs, mp = ref.random_scene(hvo.KEYLINE_DT, n_kf=1, n_lines=16, n=8, seed=3)
    fat = dict(kfs[0], kl=np.zeros(ref.MAX_LINES + 1, hvo.KEYLINE_DT), desc_rows=np.zeros((4, 32), np.uint8))
    rc, msg, res = call(ctx_of(hvo), [kfs[0], fat], mp, check=False)
    assert rc == -4 and "2049 lines" in msg, (rc, msg)
    untouched(hvo, res)


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257])
def test_entry_counts(hvo, n):
    kfs, mp = ref.random_scene(hvo.KEYLINE_DT, n_kf=1, n_lines=48, n=n, seed=200 + n)
    g = both(hvo, kfs, mp, "%d entries" % n)[0]
    assert len(g["best_idx"]) == n and (n < 255 or g["n_fused"] > 20)


@pytest.mark.parametrize("n_kf", [1, 3, 31])
def test_keyframe_counts_with_ragged_line_counts(hvo, n_kf):
    kfs, mp = ref.random_scene(hvo.KEYLINE_DT, n_kf=n_kf, n_lines=48, n=40, seed=300 + n_kf)
    rag = [ref.cut(kf, 48 if j == 0 else (j * 7) % 49) for j, kf in enumerate(kfs)]
    g = both(hvo, rag, mp, "%d key frames" % n_kf)
    assert sum(r["n_fused"] for r in g) > 5 * n_kf


@pytest.mark.parametrize("rule", [ref.CLAMPED, ref.AS_WRITTEN])
def test_random_scene(hvo, rule):
    kfs, mp, want = scene(hvo)
    got = call(ctx_of(hvo), kfs, mp, level_rule=rule)
    same(got, want[rule], "random scene, " + rule)
    assert sum(k > 0 for k in got[0]["kernel_ms"]) == 3
    # one map side per key frame = the shared one
    identical(call(ctx_of(hvo), kfs, [mp] * len(kfs), level_rule=rule), got, "per key frame")


def test_slots_are_arrays(hvo):
    """the entries as slots of a resident line map: the slot list out of order, a slot nobody names, a bad slot among the named"""
    kfs, mp, want = scene(hvo)
    n = len(mp["pos"])
    perm = np.random.RandomState(9).permutation(n + 5)[:n].astype(np.int32)          # entry i lives in slot perm[i]
    m = hvo.LineMap(slots=16)
    try:
        z = lambda *s: np.zeros(s)
        pos, nrm, mx, mn, desc = z(n + 5, 6), z(n + 5, 3), np.ones(n + 5, np.float32), np.ones(n + 5, np.float32), np.zeros((n + 5, 32), np.uint8)
        pos[perm] = mp["pos"]; nrm[perm] = mp["normal"]; mx[perm] = mp["max_distance"]; mn[perm] = mp["min_distance"]; desc[perm] = mp["desc"]
        m.set_many(0, pos, pos[:, 3:] - pos[:, :3], nrm, mx, mn, desc)
        got = call_slots(ctx_of(hvo), m, perm, kfs)
        same(got, want[ref.CLAMPED], "slots")
        bad_entry = int(want[ref.CLAMPED][0]["fused_entry"][3])
        m.set_bad(int(perm[bad_entry]))
        kb = [dict(kf, skip=np.where(np.arange(n) == bad_entry, 1, kf["skip"]).astype(np.uint8)) for kf in kfs]
        same(call_slots(ctx_of(hvo), m, perm, kfs), [ref.fuse(kf, mp) for kf in kb], "a bad slot counts as skipped")
        rc, msg, res = call_slots(ctx_of(hvo), m, np.array([0, n + 5], np.int32), [dict(kf, skip=None) for kf in kfs], check=False)
        assert rc == -1 and "slot %d" % (n + 5) in msg, msg
        untouched(hvo, res)
    finally:
        m.close()


def test_stream_form(hvo, synth):
    cam = (535.4, 539.2, 320.1, 247.6)
    g, d = synth.make_frame("std", 0x5EED0171)
    st = hvo.Stream(depth=2, stages=hvo.STAGE_LSD)
    try:
        tk = st.submit(g, d); fr = st.collect(tk)
        n = len(fr["kl"])
        assert 60 < n <= ref.MAX_LINES
        mp = ref.map_from_frame(fr["kl"], fr["ldesc"], cam, 171)
        skip = (np.arange(n) % 11 == 0).astype(np.uint8)
        kf = ref.make_kf(fr["kl"], fr["ldesc"], Tcw=ref.IDENTITY, cam=cam, skip=skip)
        kw = dict(n_levels=2, level_rule=ref.AS_WRITTEN)
        want = ref.fuse(kf, mp, **kw)
        assert want["n_fused"] * 4 >= n and want["n_behind"] > 5
        strm = st.fuse_lines(tk, cam + (40.0,), ref.IDENTITY, maps=mp, skip=skip, **kw)
        same([strm], [want], "stream")
        identical([strm], call(ctx_of(hvo), [kf], mp, **kw), "stream = host")
        m = hvo.LineMap(slots=n)
        try:
            m.set_many(0, mp["pos"], mp["pos"][:, 3:] - mp["pos"][:, :3], mp["normal"], mp["max_distance"], mp["min_distance"], mp["desc"])
            identical([st.fuse_lines(tk, cam + (40.0,), ref.IDENTITY, line_map=m, slots=np.arange(n, dtype=np.int32), skip=skip, **kw)], [strm], "stream on slots")
        finally:
            m.close()
        rc, msg, res = st.fuse_lines(tk, cam + (40.0,), ref.IDENTITY, maps=mp, skip=skip, th_low=256, check=False)
        assert rc == -1 and "th_low" in msg
        untouched(hvo, res)
    finally:
        st.close()
    st = hvo.Stream(depth=2, stages=hvo.STAGE_ORB)
    try:
        tk = st.submit(g, d); st.collect(tk)
        rc, msg, res = st.fuse_lines(tk, cam + (40.0,), ref.IDENTITY, maps=mp, check=False)
        assert rc == -1 and "fuse lines" in msg and "LSD stage" in msg, msg
        untouched(hvo, res)
    finally:
        st.close()


def test_refusals_leave_the_outputs_untouched(hvo):
    kfs, mp = ref.random_scene(hvo.KEYLINE_DT, n_kf=2, n_lines=16, n=12, seed=53)
    ctx = ctx_of(hvo)
    for kw, word in ((dict(th_low=256), "th_low"), (dict(n_levels=0), "n_levels"), (dict(n_levels=17), "n_levels"), (dict(level_rule=2), "level_rule")):
        rc, msg, res = call(ctx, kfs, mp, check=False, **kw)
        assert rc == -1 and word in msg, (word, rc, msg)
        untouched(hvo, res)
    for k2, word in ((dict(kfs[1], bounds=(0.0, 0.0, 0.0, 480.0)), "bounds"), (dict(kfs[1], kl=None, n=16), "null array"), (dict(kfs[1], desc_rows=None, n_desc_rows=16), "null array")):
        rc, msg, res = call(ctx, [kfs[0], k2], mp, check=False)
        assert rc == -1 and word in msg, (word, rc, msg)
        untouched(hvo, res)
    big = ref.make_map([(np.zeros(6), (1.0, 0.0, 0.0), 1.0, 1.0, ref.BASE)] * 1)
    big = {k: np.repeat(v, ref.MAX_ENTRIES + 1, axis=0) for k, v in big.items()}
    rc, msg, res = call(ctx, [dict(kfs[0], skip=None)], big, check=False)
    assert rc == -4 and "65537 entries" in msg, msg
    untouched(hvo, res)
    # 2^24 padded pairs: 257 key frames x 65536 entries.  Room for that many results is not made: the call is refused before it writes, so
    # every result shares one best_idx cell, which must stay as it is
    import ctypes as C
    big = {k: v[:ref.MAX_ENTRIES] for k, v in big.items()}
    M, mk, ns = hvo._lf_maps([big]); K, kk = hvo._lf_keyframes([dict(kfs[0], skip=None)] * 257, [ref.MAX_ENTRIES] * 257)
    R = (hvo.LfResult * 257)(); cell = np.full(1, hvo.FUSE_UNTOUCHED, np.int32)
    for j in range(257): R[j].best_idx = cell.ctypes.data; R[j].status = hvo.FUSE_UNTOUCHED
    P = hvo._lf_params(3.0, 50, ref.LOG_SF, 3, 1.2, ref.CLAMPED, False)
    rc = hvo.lib().hvo_fuse_lines(ctx.h, C.byref(P), M, 257, K, R)
    msg = hvo.lib().hvo_last_error(ctx.h).decode()
    assert rc == -4 and "%d padded entries" % (257 * ref.MAX_ENTRIES) in msg, msg
    assert cell[0] == hvo.FUSE_UNTOUCHED and all(R[j].status == hvo.FUSE_UNTOUCHED for j in range(257))
    assert both(hvo, kfs, mp, "after the refusals")[0]["status"] == 0          # and the context goes on working


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
        kfs, mp, want = scene(hvo)
        kS, mS = ref.random_scene(hvo.KEYLINE_DT, n_kf=1, n_lines=40, n=50, seed=61)
        wS = [ref.fuse(kf, mS) for kf in kS]
        assert wS[0]["n_fused"] > 10 and wS[0]["n_behind"] > 0
        cap = ctx.debug_call_arena(fill, 60000)
        assert cap >= 60000 and (ctx.debug_call_arena_peek(0, cap) == fill).all()
        first = call(ctx, kS, mS)
        same(first, wS, "S on a filled arena")
        assert ctx.debug_call_arena(None) == cap                      # S fits: no regrowth so far
        for k in range(2):
            identical(call(ctx, kS, mS), first, "S again")
        ctx.debug_call_arena(fill)
        L = call(ctx, kfs, mp)                                     # grows the arena
        same(L, want[ref.CLAMPED], "L")
        cap2 = ctx.debug_call_arena(None)
        assert cap2 > cap
        identical(call(ctx, kS, mS), first, "S after L")
        identical(call(ctx, kfs, mp), L, "L after S")
        _leftovers(hvo, ctx)
        identical(call(ctx, kS, mS), first, "S after other calls")
        ctx.debug_call_arena(fill)
        assert (ctx.debug_call_arena_peek(cap2 - 4096, 4096) == fill).all()
        identical(call(ctx, kS, mS), first, "S on the regrown, filled arena")
    finally:
        ctx.close()


def test_example_runs(hvo, tmp_path):
    """examples/fuse_line_neighbors.cpp linked against the library: both calls (the second on slots) and the host walks on its toy map print
    what the restatement's walk gives on the same toy map, under stop_on_behind true and false"""
    import os
    import subprocess
    from conftest import ROOT, PKG_DIR
    csrc = os.path.join(PKG_DIR, "csrc"); exe = str(tmp_path / "fuse_line_neighbors")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "fuse_line_neighbors.cpp"),
                           "-L" + csrc, "-lhvo", "-Wl,-rpath," + csrc, "-o", exe])
    out = subprocess.check_output([exe]).decode()
    print(out)
    want = ref.toy_run(hvo.KEYLINE_DT, True) + ref.toy_run(hvo.KEYLINE_DT, False)
    assert out.splitlines() == want
    assert "stopped_at 5" in want[1] and "stopped_at -1" in want[6] and "replaced 1" in want[1]
    # and the same toy map through the Python binding
    dev = lambda kfs, mp: call(ctx_of(hvo), kfs, mp, n_levels=1)
    assert ref.toy_run(hvo.KEYLINE_DT, True, dev) + ref.toy_run(hvo.KEYLINE_DT, False, dev) == want
