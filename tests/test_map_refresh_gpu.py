"""MapPoint / MapLine ComputeDistinctiveDescriptors + UpdateNormalAndDepth / UpdateAverageDir on the GPU (csrc/map_refresh.hip) against
tests/map_refresh_ref.py.  Integers are compared exactly, floats by their bits (a NaN by being one); an entry the status says is not written
must hold what the caller put there.  tests/test_map_refresh.py asserts on the CPU that the crafted cases say what they are meant to say and
that the random scenes (map_refresh_ref.SCENE_*) meet every status code and at least 20 ties."""
import numpy as np
import pytest

import arena_cases as ac
import line_map_ref
import map_refresh_ref as ref
import point_map_ref as pm

pytestmark = pytest.mark.gpu
F32 = np.float32
_cache = {}
COUNTS = (1, 2, 3, 4, 63, 64, 65, 255, 256)


def ctx_of(hvo):
    if "ctx" not in _cache:
        _cache["ctx"] = hvo.Context(max_batch=1)
    return _cache["ctx"]


def keys(line):
    return ref.KEYS_LINE if line else ref.KEYS_POINT


def same(got, want, line, what=""):
    for k in keys(line):
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape, g.dtype, w.dtype)
        eq = (g == w) | (np.isnan(g) & np.isnan(w)) if g.dtype.kind == "f" else g == w
        if g.dtype.kind == "f": eq &= np.signbit(g) == np.signbit(w)
        bad = np.flatnonzero(~eq.reshape(len(g), -1).all(axis=1))
        assert len(bad) == 0, (what, k, bad[:8], g[bad[:2]], w[bad[:2]])


def identical(a, b, line, what=""):
    for k in keys(line):
        assert a[k].tobytes() == b[k].tobytes(), (what, k)


def run(hvo, line, pos, obs, **kw):
    c = ctx_of(hvo)
    return c.refresh_map_lines(pos, obs, **kw) if line else c.refresh_map_points(pos, obs, **kw)


def want_of(line, pos, obs, **kw):
    return (ref.refresh_lines if line else ref.refresh_points)(pos, obs, **kw)


def both(hvo, line, pos, obs, tag="", **kw):
    got, want = run(hvo, line, pos, obs, **kw), want_of(line, pos, obs, **kw)
    same(got, want, line, tag)
    return got, want


def positions(line, n, rng):
    return ref.line_positions(n, rng) if line else ref.point_positions(n, rng)


def scene(line):
    k = ("scene", line)
    if k not in _cache:
        pos, obs = ref.random_scene(**(ref.SCENE_LINES if line else ref.SCENE_POINTS))
        _cache[k] = (pos, obs, want_of(line, pos, obs))
    return _cache[k]


@pytest.mark.parametrize("line", [False, True])
def test_observation_counts(hvo, line):
    """1 .. 4 (the ranks 0 0 1 1), 63 / 64 / 65 (the distances leave LDS) and 255 / 256 (four rows per lane), alone with every observer good and
    together with a fifth of them bad, so that the descriptor list's length differs from the observation count"""
    rng = np.random.RandomState(11)
    for N in COUNTS:
        obs = ref.make_obs([N], rng, flips=40)
        got, want = both(hvo, line, positions(line, 1, rng), obs, "N = %d" % N)
        assert want["status"][0] == 0 and 0 <= want["best_obs"][0] < N
    obs = ref.make_obs(COUNTS, rng, flips=40, bad_rate=0.2)
    both(hvo, line, positions(line, len(COUNTS), rng), obs, "all counts, a fifth bad")


@pytest.mark.parametrize("line", [False, True])
def test_257_observations_are_refused_whole(hvo, line):
    rng = np.random.RandomState(12)
    obs = ref.make_obs([3, 257, 2], rng)
    pos = positions(line, 3, rng)
    c = ctx_of(hvo)
    with pytest.raises(hvo.HvoError):                                        # the binding refuses before the library
        run(hvo, line, pos, obs)
    P, I, O, o, n, keep = hvo._mr_args(line, obs["obs_start"], obs["obs_desc"], obs["obs_Ow"], obs["ref_Ow"], obs["ref_level"], obs["kf_bad"], obs["skip"], 8, 1.2, 3, None)
    import ctypes as C
    p = np.ascontiguousarray(pos)
    f = getattr(hvo.lib(), "hvo_refresh_map_lines" if line else "hvo_refresh_map_points"); f.restype = C.c_int; f.argtypes = [C.c_void_p] * 5
    rc = f(c.h, C.addressof(P), C.addressof(I), p.ctypes.data, C.addressof(O))
    assert rc == -4 and "257 observations of one feature" in hvo.lib().hvo_last_error(c.h).decode()
    assert all((v == hvo.MR_UNTOUCHED).all() for v in o.values())
    # the other refusals: a decreasing list, a first entry that is not 0, a missing array, an empty mask; and the empty call
    for change, code in ((dict(obs_start=[0, 3, 2, 5]), -1), (dict(obs_start=[1, 3, 4, 5]), -1), (dict(ref_Ow=None), -1), (dict(obs_desc=None), -1)):
        rc, msg, r = run(hvo, line, pos, dict(ref.make_obs([3, 1, 1], rng), **change), check=False)
        assert rc == code and msg and all((r[k] == hvo.MR_UNTOUCHED).all() for k in keys(line)), (change, rc, msg)
    rc, msg, r = run(hvo, line, pos, ref.make_obs([3, 1, 1], rng), what=0, check=False)
    assert rc == -1
    rc, msg, r = run(hvo, line, pos[:0], dict(ref.make_obs([], rng), obs_start=[0]), check=False)
    assert rc == 0 and len(r["status"]) == 0


@pytest.mark.parametrize("line", [False, True])
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_ragged_lists(hvo, line, n):
    rng = np.random.RandomState(13 + n)
    counts = rng.randint(0, 6, n); counts[::5] = 0
    got, want = both(hvo, line, positions(line, n, rng), ref.make_obs(counts, rng, bad_rate=0.15), "n = %d" % n)
    if n > 1: assert (want["status"] == ref.NO_OBS).sum() >= n // 5


@pytest.mark.parametrize("line", [False, True])
def test_every_status_code_and_each_half(hvo, line):
    U = ref.UNTOUCHED
    d = ref.on_a_line([3, 4])
    obs = dict(obs_start=[0, 2, 2, 4, 6, 8, 10], obs_desc=np.concatenate([d] * 5), obs_Ow=np.ones((10, 3), F32), kf_bad=[0, 0, 0, 0, 1, 1, 0, 0, 1, 1],
               ref_Ow=np.zeros((6, 3), F32), ref_level=[0, 0, 0, 0, 8, -1], skip=[0, 0, 1, 0, 0, 0])
    pos = np.tile(np.array([0, 0, 2, 0, 0, 2], np.float64), (6, 1)) if line else np.tile(np.array([0, 0, 2], F32), (6, 1))
    got, want = both(hvo, line, pos, obs, "statuses")
    assert got["status"].tolist() == [0, 2, 1, 3, 4, 3]
    assert (got["normal"][1] == U).all() and (got["normal"][3] != U).any() and got["max_dist"][4] == U and (got["desc"][3] == U).all()
    g, w = both(hvo, line, pos, obs, "geometry alone", what=ref.GEOMETRY)
    assert (g["desc"] == U).all() and g["status"].tolist() == [0, 2, 1, 0, 4, 4]
    g, w = both(hvo, line, pos, obs, "descriptor alone", what=ref.DESCRIPTOR)
    assert (g["normal"] == U).all() and (g["max_dist"] == U).all() and g["status"].tolist() == [0, 2, 1, 3, 0, 3]
    # only the outputs asked for are written
    r = run(hvo, line, pos, obs, want=("status", "desc"))
    assert np.array_equal(r["status"], want["status"]) and np.array_equal(r["desc"], want["desc"]) and (r["normal"] == U).all() and (r["best_obs"] == U).all()


@pytest.mark.parametrize("line", [False, True])
def test_ties_in_the_median(hvo, line):
    cases = ([7], [7, 100], [0, 10, 20], [0, 50, 60], [0, 5, 20, 21], [30, 0, 29, 31], [9, 9, 9, 9, 9], [40] * 64, [40] * 65, list(range(0, 200, 2)) + [0] * 156)
    rng = np.random.RandomState(14)
    counts = [len(c) for c in cases]
    obs = ref.make_obs(counts, rng)
    obs["obs_desc"] = np.concatenate([ref.on_a_line(c) for c in cases])
    got, want = both(hvo, line, positions(line, len(cases), rng), obs, "ties")
    assert got["best_obs"][:9].tolist() == [0, 0, 0, 1, 2, 0, 0, 0, 0] and got["best_median"][:9].tolist() == [0, 0, 10, 10, 1, 1, 0, 0, 0]
    assert want["tie"].sum() >= 8


@pytest.mark.parametrize("line", [False, True])
def test_random_scene(hvo, line):
    pos, obs, want = scene(line)
    assert len(pos) == (100 if line else 300) and sorted(set(want["status"].tolist())) == [0, 1, 2, 3, 4] and int(want["tie"].sum()) >= 20
    same(run(hvo, line, pos, obs), want, line, "scene")


def make_map(hvo, line, pos, rng):
    """a map of len(pos) slots with arbitrary contents; every seventh slot bad"""
    n = len(pos)
    M = dict(pos=pos, normal=rng.uniform(-1, 1, (n, 3)).astype(np.float64 if line else F32), max_dist=rng.uniform(5, 9, n).astype(F32),
             min_dist=rng.uniform(0.1, 1, n).astype(F32), desc=rng.randint(0, 256, (n, 32)).astype(np.uint8), observed=rng.randint(0, 2, n).astype(np.uint8),
             bad=(np.arange(n) % 7 == 3).astype(np.uint8))
    if line:
        M["wvec"] = rng.uniform(-1, 1, (n, 3))
        m = hvo.LineMap(slots=0); m.set_many(0, M["pos"], M["wvec"], M["normal"], M["max_dist"], M["min_dist"], M["desc"], M["observed"], M["bad"])
    else:
        m = hvo.PointMap(slots=0); m.set_many(0, M["pos"], M["normal"], M["max_dist"], M["min_dist"], M["desc"], M["observed"], M["bad"])
    return m, M


def slot_bytes(m, j):
    s = m.slot(j)
    return {k: (np.asarray(v).tobytes() if isinstance(v, np.ndarray) else v) for k, v in s.items()}


@pytest.mark.parametrize("line", [False, True])
def test_slot_form(hvo, line):
    """the slot form equals the array form on the slots' positions bit for bit; the map reads back exactly the outputs; untouched, bad and
    skipped slots are unchanged byte for byte, and so are observed and bad of every slot"""
    pos, obs, _ = scene(line)
    rng = np.random.RandomState(15)
    n = len(pos)
    nm = n + 50
    mpos = positions(line, nm, rng)
    slots = rng.permutation(nm)[:n].astype(np.int32)
    mpos[slots] = pos
    m, M = make_map(hvo, line, mpos, rng)
    before = [slot_bytes(m, j) for j in range(nm)]
    arr = run(hvo, line, pos, dict(obs, skip=np.maximum(obs["skip"], M["bad"][slots])))     # a bad slot counts as skipped
    got = m.refresh(ctx_of(hvo), slots, obs)
    identical(got, arr, line, "slot form against array form")
    assert (M["bad"][slots] == 1).sum() > 5 and (got["status"][M["bad"][slots] == 1] == ref.SKIPPED).all()
    U = ref.UNTOUCHED
    listed = set(int(s) for s in slots)
    for j in range(nm):
        now = slot_bytes(m, j)
        assert (now["bad"], now["observed"], now["pos"]) == (before[j]["bad"], before[j]["observed"], before[j]["pos"]), j
        if j not in listed: assert now == before[j], j
    for i, j in enumerate(slots):
        now, was, st = m.slot(int(j)), before[int(j)], got["status"][i]
        if st in (ref.SKIPPED, ref.NO_OBS):
            assert slot_bytes(m, int(j)) == was, (i, j); continue
        assert now["desc"].tobytes() == (got["desc"][i].tobytes() if got["best_obs"][i] >= 0 else was["desc"]), (i, j)
        assert now["normal"].tobytes() == got["normal"][i].tobytes()
        if line: assert now["wvec"].tobytes() == got["wvec"][i].tobytes()
        rng_written = 0 <= obs["ref_level"][i] < 8
        for k in ("max_dist", "min_dist"):
            assert F32(now[k]).tobytes() == (got[k][i] if rng_written else F32(was[k])).tobytes(), (i, j, k)
            assert (got[k][i] != U) == rng_written, (i, j, k)
    # a slot outside the map and a slot listed twice are refused whole; the text is the map's too
    for bad_slots in (np.concatenate([slots[:-1], [nm]]), np.concatenate([slots[:-1], slots[:1]])):
        rc, msg, r = m.refresh(ctx_of(hvo), bad_slots.astype(np.int32), obs, check=False)
        assert rc == -1 and msg and (r["status"] == U).all()
        assert m._f("last_error")(m.h).decode() == msg
    m.close()


def test_end_to_end_points(hvo):
    """refresh, then search_local_points, equals set_many with the restatement's values, then the same search"""
    e = ac.env()
    i, _ = ac.inputs(e, "search_local_points", "S")
    M = {k: np.array(v) for k, v in i["M"].items()}
    n = len(M["pos"])
    rng = np.random.RandomState(16)
    slots = np.flatnonzero(np.arange(n) % 3 != 0).astype(np.int32)
    R, t, Ow = pm.pose_parts(i["T"])
    obs = ref.make_obs(rng.randint(1, 12, len(slots)), rng)
    cnt = np.diff(obs["obs_start"])
    obs["obs_desc"] = np.repeat(M["desc"][slots], cnt, axis=0); obs["obs_desc"][::3, 5] ^= 0x11
    obs["obs_Ow"] = (Ow[None, :] + rng.uniform(-0.05, 0.05, (len(obs["obs_desc"]), 3))).astype(F32)
    obs["ref_Ow"] = np.tile(Ow, (len(slots), 1)).astype(F32); obs["ref_level"][:] = rng.randint(0, 3, len(slots))
    prior = dict(desc=M["desc"][slots], normal=M["normal"][slots], max_dist=M["max_dist"][slots], min_dist=M["min_dist"][slots])
    want = ref.refresh_points(M["pos"][slots], dict(obs, skip=M["bad"][slots]), prior=prior)
    M2 = dict(M)
    for k in prior: M2[k] = M[k].copy(); M2[k][slots] = want[k]
    search = lambda mp: ctx_of(hvo).search_local_points(mp, pm.CAM, i["T"], i["kp"], i["ur"], i["desc"], ac.B4, held=i["held"].copy(), seen_extra=i["extra"], th=1.0,
                                                        log_scale_factor=pm.LOG_SF, n_levels=pm.N_LEVELS)
    a = ac._pmap_of(e, M); a.refresh(ctx_of(hvo), slots, obs)
    b = ac._pmap_of(e, M2)
    ra, rb = search(a), search(b)
    ac.identical(ra, rb, "points end to end")
    assert ra.n_matches > 5 and not all(np.array_equal(M2[k], M[k]) for k in prior)
    a.close(); b.close()


def test_end_to_end_lines(hvo):
    e = ac.env()
    i, _ = ac.inputs(e, "search_local_lines", "S")
    M = {k: np.array(v) for k, v in i["M"].items()}
    n = len(M["pos"])
    rng = np.random.RandomState(17)
    slots = np.flatnonzero(np.arange(n) % 3 != 0).astype(np.int32)
    R, t, Ow = pm.pose_parts(i["T"])
    obs = ref.make_obs(rng.randint(1, 12, len(slots)), rng)
    cnt = np.diff(obs["obs_start"])
    obs["obs_desc"] = np.repeat(M["desc"][slots], cnt, axis=0); obs["obs_desc"][::3, 5] ^= 0x11
    obs["obs_Ow"] = (Ow[None, :] + rng.uniform(-0.05, 0.05, (len(obs["obs_desc"]), 3))).astype(F32)
    obs["ref_Ow"] = np.tile(Ow, (len(slots), 1)).astype(F32); obs["ref_level"][:] = rng.randint(0, 3, len(slots))
    prior = dict(desc=M["desc"][slots], normal=M["normal"][slots], wvec=M["wvec"][slots], max_dist=M["max_dist"][slots], min_dist=M["min_dist"][slots])
    want = ref.refresh_lines(M["pos"][slots], dict(obs, skip=M["bad"][slots]), prior=prior)
    M2 = dict(M)
    for k in prior: M2[k] = M[k].copy(); M2[k][slots] = want[k]
    search = lambda lm: ctx_of(hvo).search_local_lines(lm, ac.LCAM, i["T"], i["kl"], i["fn"], i["l3"], i["ld"], i["cs"], i["ci"], line_map_ref.BOUNDS, held=i["held"].copy(),
                                                       seen_extra=i["extra"], log_scale_factor=line_map_ref.LOG_SF, th=5.0, rel_map=True)
    a = ac._lmap_open(e, dict(M=M))["map"]; a.refresh(ctx_of(hvo), slots, obs)
    b = ac._lmap_open(e, dict(M=M2))["map"]
    ra, rb = search(a), search(b)
    ac.identical(ra, rb, "lines end to end")
    assert ra.n_in_view > 5 and not all(np.array_equal(M2[k], M[k]) for k in prior)
    a.close(); b.close()


@pytest.mark.parametrize("line", [False, True])
def test_dirty_arena(hvo, line):
    """the same call on a clean arena, on an arena filled with 0xFF and 0x5A, and after another call's leftovers (a larger refresh of the other kind):
    identical bytes; what the call reads past its uploads it has cleared itself"""
    c = ctx_of(hvo)
    rng = np.random.RandomState(18)
    counts = rng.randint(0, 9, 70); counts[5] = 70
    obs = ref.make_obs(counts, rng, bad_rate=0.2); ref.plant_statuses(obs, rng)
    pos = positions(line, 70, rng)
    first = run(hvo, line, pos, obs)
    same(first, want_of(line, pos, obs), line, "dirty arena: the case itself")
    for fill in (0xFF, 0x5A):
        cap = c.debug_call_arena(fill=fill, min_bytes=1 << 20)
        assert cap >= 1 << 20 and (c.debug_call_arena_peek(cap - 64, 64) == fill).all()
        identical(run(hvo, line, pos, obs), first, line, "fill %#x" % fill)
    spos, sobs, swant = scene(not line)
    run(hvo, not line, spos, sobs)                                           # another call's leftovers, larger than this one
    identical(run(hvo, line, pos, obs), first, line, "after a larger call")


def test_example_runs(hvo, tmp_path):
    """examples/map_refresh.cpp linked against the library: hvo::PointMap::refresh on its toy map prints what the restatement gives for the
    same map, read back from the slots"""
    import os
    import re
    import subprocess
    from conftest import ROOT, PKG_DIR
    csrc = os.path.join(PKG_DIR, "csrc"); exe = str(tmp_path / "map_refresh")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "map_refresh.cpp"),
                           "-L" + csrc, "-lhvo", "-Wl,-rpath," + csrc, "-o", exe])
    out = subprocess.check_output([exe]).decode()
    print(out)
    pos = np.array([[0, 0, 2], [0.5, 0, 2], [-0.5, 0.25, 2], [0, 0.5, 2]], F32)
    Ow = np.zeros((9, 3), F32); Ow[:, 0] = np.tile([0, 0.25, 0.5], 3)
    obs = dict(obs_start=[0, 3, 6, 9, 9], obs_desc=ref.on_a_line([0, 10, 20, 0, 50, 60, 5, 6, 7]), obs_Ow=Ow, kf_bad=[0] * 6 + [1] * 3,
               ref_Ow=np.array([[0, 0, 0], [0.25, 0, 0], [0, 0, 0], [0, 0, 0]], F32), ref_level=[0, 2, 1, 0], skip=None)
    prior = dict(desc=np.full((4, 32), 0xAA, np.uint8), normal=np.zeros((4, 3), F32), max_dist=np.full(4, 9, F32), min_dist=np.full(4, 1, F32))
    w = ref.refresh_points(pos, obs, prior=prior)
    assert w["status"].tolist() == [0, 0, 3, 2] and w["best_obs"].tolist() == [0, 1, -1, -1]
    rows = re.findall(r"point (\d+): status (\d+) best (-?\d+) median (-?\d+) descriptor bits (\d+) normal (\S+) (\S+) (\S+) range (\S+) (\S+)", out)
    assert len(rows) == 4
    for p, r in enumerate(rows):
        assert [int(v) for v in r[:5]] == [p, w["status"][p], w["best_obs"][p], w["best_median"][p], int(np.unpackbits(w["desc"][p]).sum())], r
        assert np.array([float(v) for v in r[5:]], F32).tobytes() == np.concatenate([w["normal"][p], [w["max_dist"][p], w["min_dist"][p]]]).astype(F32).tobytes(), r
