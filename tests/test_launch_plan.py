"""Which kernels a batch takes is decided by its size: peac_select (csrc/peac.hip), lsd_select (csrc/lsd.hip), hvo_batch_select and
hvo_prio_select (csrc/api.hip) are plain host functions, the launches read their result, and hvo_debug_plan_select evaluates them without
a device.  This file holds their thresholds AS DATA (TABLE): the selection is walked over every batch size from 1 to 8200 at three
geometries and must change where the table says and nowhere else.  Someone who moves a threshold changes it here, on purpose.

tests/test_batch_boundaries_gpu.py imports expected_report() and compares it with what a context says it launched."""
import os

import pytest

from conftest import PKG_DIR

N_MAX = 8200
GEOMS = [(640, 480), (200, 160), (1280, 960)]
ALL = None          # "every n above the last bound"

# (stage, field): where the threshold is written (file under csrc/, the text of the deciding expression -- it must occur exactly once in
# that file --, its line when this table was written) and the value per range of n: [(largest n of the range, value), ..., (ALL, value)].
# A callable value is evaluated on n.
TABLE = {
    # ---- LSD: growing form --------------------------------------------------------------------------------------------------------
    ("lsd", "async_w"): dict(file="lsd.hip", line=2014, text="int aw = n <= 8 ? 32 : n <= 16 ? 16 : 0;",
                             steps=[(8, 32), (16, 16), (ALL, 0)]),
    ("lsd", "grow"): dict(file="lsd.hip", line=2002, text="bool dense = n > 5 * 1024;",       # and `bool lat = n <= 64 && ...` two lines below
                          steps=[(16, "async"), (64, "lat"), (5120, "grow"), (ALL, "dense")]),
    ("lsd", "async_fallback"): dict(file="lsd.hip", line=2023, text="s.grow = LSD_GROW_ASYNC; s.async_w = aw; s.async_fallback = 1;",
                                    steps=[(16, 1), (ALL, 0)]),
    ("lsd", "async_lds"): dict(file="lsd.hip", line=2026, text="size_t alds = (n > 2 && n <= 16) ? 56 * 1024 : 0;",
                               steps=[(2, 0), (16, 56 * 1024), (ALL, 0)]),
    ("lsd", "async_early"): dict(file="lsd.hip", line=2023, text="s.async_early = kn.async_early.or_(1);", steps=[(16, 1), (ALL, 0)]),
    ("lsd", "lat_lds"): dict(file="lsd.hip", line=2033, text="size_t lds = (size_t)g.nwords * 4, floor_ = 56 * 1024;",
                             steps=[(16, 0), (64, 56 * 1024), (ALL, 0)]),
    # ---- LSD: chunks of the preamble, LBD and culling loops -----------------------------------------------------------------------
    ("lsd", "chunk"): dict(file="lsd.hip", line=1983, text="s.chunk = (int)std::min<size_t>((size_t)plan_batch, 512);",
                           steps=[(512, lambda n: n), (ALL, 512)]),
    ("lsd", "chunks"): dict(file="lsd.hip", line=1995, text="s.chunks = (n + s.chunk - 1) / s.chunk;", steps=[(ALL, lambda n: (n + 511) // 512)]),
    ("lsd", "pre"): dict(file="lsd.hip", line=1997, text="s.pre_form = (readings & HVO_READING_LSD_8U) ? 2 : pre_fused ? 0 : 1;", steps=[(ALL, "fused")]),
    ("lsd", "compact"): dict(file="lsd.hip", line=1990, text="s.compact = kn.compact ? 1 : 0;", steps=[(ALL, 0)]),
    ("lsd", "lbd_gradient"): dict(file="lsd.hip", line=1998, text="s.lbd_split = lbd_split_form(readings, have_b5 || kn.lbd_split.set);", steps=[(ALL, "fused")]),
    ("lsd", "lbd_desc"): dict(file="lsd.hip", line=2000, text="s.lbd_desc = (!kn.lbd_desc.off() && std::max(g.w, g.h) <= LBD_SHORT_SAFE) ? 1 : 0;", steps=[(ALL, 1)]),
    ("lsd", "perm_items"): dict(file="lsd.hip", line=2001, text="s.perm_items = (n >= 2 && frame_perm_on) ? n : 0;", steps=[(1, 0), (ALL, lambda n: n)]),
    ("lsd", "n"): dict(file="lsd.hip", line=1979, text="s.n = n; s.plan_batch = plan_batch; s.cull = cull ? 1 : 0;", steps=[(ALL, lambda n: n)]),
    ("lsd", "plan_batch"): dict(file="lsd.hip", line=1979, text="s.n = n; s.plan_batch = plan_batch; s.cull = cull ? 1 : 0;", steps=[(ALL, lambda n: n)]),
    ("lsd", "cull"): dict(file="lsd.hip", line=1979, text="s.n = n; s.plan_batch = plan_batch; s.cull = cull ? 1 : 0;", steps=[(ALL, 0)]),
    # ---- PEAC: the AHC --------------------------------------------------------------------------------------------------------------
    ("peac", "cluster"): dict(file="peac.hip", line=2197, text="const int heads_max = kn.heads_maxn.or_(256);",     # heads up to 256 frames, then `n >= 3072 ? 16 : 64`
                              steps=[(256, "heads"), (3071, "c64"), (ALL, "slots")]),
    ("peac", "heads"): dict(file="peac.hip", line=2203, text="int heads = (gl <= 0 && n <= heads_max && (heads_fit || heads_big)) ? 3 : 0;",
                            steps=[(256, 3), (ALL, 0)]),
    ("peac", "heads_big"): dict(file="peac.hip", line=2209, text="bool big = heads_big || n > 128;", steps=[(128, 0), (256, 1), (ALL, 0)]),
    ("peac", "group"): dict(file="peac.hip", line=2186, text="const int use = gl > 0 ? gl : (n >= 3072 ? 16 : 64);", steps=[(3071, 64), (ALL, 16)]),
    ("peac", "cluster_wgs"): dict(file="peac.hip", line=2227, text="s.cluster_wgs = (n + 3) / 4;", steps=[(3071, lambda n: n), (ALL, lambda n: (n + 3) // 4)]),
    ("peac", "perm_items"): dict(file="peac.hip", line=2191, text="s.perm_items = (waves >= 2 && frame_perm_on && !kn.perm.off()) ? waves : 0;",
                                 steps=[(1, 0), (3071, lambda n: n), (ALL, lambda n: (n + 3) // 4)]),
    # the keys of k_peac_cluster<64> would sit in LDS up to 256 frames -- the batch sizes the queue heads take: never by default
    ("peac", "ldsq"): dict(file="peac.hip", line=2218, text="bool ldsq = n <= 256;", steps=[(ALL, 0)]),
    ("peac", "edges_done"): dict(file="peac.hip", line=2182, text="s.edges_done = ((size_t)g.nblk * 34 + 16 <= 150 * 1024 && !kn.edges.off()) ? 1 : 0;", steps=[(ALL, 1)]),
    ("peac", "poolcap"): dict(file="peac.hip", line=2211, text="const bool force_pool = kn.poolcap.set && kn.poolcap.v >= 7 * g.nblk && kn.poolcap.v < g.poolcap;", steps=[(ALL, 0)]),
    ("peac", "slots_fit"): dict(file="peac.hip", line=2194, text="const bool slots_fit = g.segcap <= 32768;", steps=[(ALL, 1)]),
    # ---- PEAC: block map and flood ------------------------------------------------------------------------------------------------
    ("peac", "blkmap_y"): dict(file="peac.hip", line=2229, text="s.blkmap_y = n <= 64 ? 32 : n <= 1024 ? 4 : 1;", steps=[(64, 32), (1024, 4), (ALL, 1)]),
    ("peac", "flood_t"): dict(file="peac.hip", line=2234, text="const int ft = flood_t > 0 ? flood_t : (n >= 6144 ? 64 : n <= 8 ? 512 : 256);",
                              steps=[(8, 512), (6143, 256), (ALL, 64)]),
    ("peac", "flood_epl"): dict(file="peac.hip", line=2237, text="s.flood_epl = (ft == 64 && fe == 2) ? 2 : 1;", steps=[(ALL, 1)]),
    ("peac", "flood_slim"): dict(file="peac.hip", line=2238, text="s.flood_slim = (ft == 64 && fe != 2 && !kn.flood_slim.off()) ? 1 : 0;", steps=[(6143, 0), (ALL, 1)]),
    ("peac", "flood_perm_items"): dict(file="peac.hip", line=2239, text="s.flood_perm_items = (n >= 2 && frame_perm_on && !kn.flood_perm.off()) ? n : 0;",
                                       steps=[(1, 0), (ALL, lambda n: n)]),
    ("peac", "n"): dict(file="peac.hip", line=2180, text="s.n = n;", steps=[(ALL, lambda n: n)]),
    # ---- what hvo_batch_run and hvo_create choose themselves ----------------------------------------------------------------------
    ("batch", "sched"): dict(file="api.hip", line=78, text="b.sched = sched_cfg >= 0 ? sched_cfg : (n >= 3072 ? (big_frames ? 7 : 5) : 1);", steps=[(3071, 1), (ALL, 5)]),
    ("batch", "orb_first"): dict(file="api.hip", line=80, text="b.orb_first = (b.sched == 5 || b.sched == 7) && !serialize && (stages & HVO_STAGE_ORB);", steps=[(3071, 0), (ALL, 1)]),
    ("batch", "lsd_first"): dict(file="api.hip", line=85, text="n >= 8 && n <= 64 && (stages & (HVO_STAGE_LSD | HVO_STAGE_LSD_CULL)) != 0;", steps=[(7, 0), (64, 1), (ALL, 0)]),
    ("batch", "peac_last"): dict(file="api.hip", line=79, text="b.peac_last = b.sched >= 3 && b.sched != 5 && b.sched != 7 && !serialize;", steps=[(ALL, 0)]),
    ("batch", "prio_orb"): dict(file="api.hip", line=64, text="pr[0] = 0; pr[1] = -1; pr[2] = 1;", steps=[(ALL, 0)]),
    ("batch", "prio_lsd"): dict(file="api.hip", line=65, text="if (max_batch >= 3072) pr[1] = pr[2] = 0;", steps=[(3071, -1), (ALL, 0)]),
    ("batch", "prio_peac"): dict(file="api.hip", line=65, text="if (max_batch >= 3072) pr[1] = pr[2] = 0;", steps=[(3071, 1), (ALL, 0)]),
    ("batch", "stages"): dict(file="api.hip", line=86, text="b.stages = stages; b.n = n;", steps=[(ALL, 7)]),
    ("batch", "n"): dict(file="api.hip", line=86, text="b.stages = stages; b.n = n;", steps=[(ALL, lambda n: n)]),
}

# What a geometry changes, written out: (w, h) -> {(stage, field): steps}.  Everything else is TABLE's.
GEOMETRY_EXCEPTIONS = {
    (1280, 960): {
        # 12 288 blocks: 24 704 node ids do not fit the queue heads' LDS form (peac.hip: heads_fit), the BIG form takes every batch size
        ("peac", "heads_big"): [(256, 1), (ALL, 0)],
        # ... and k_peac_edges' 34 bytes of LDS per block exceed 150 KB: initGraph's edges stay inside the clustering kernel
        ("peac", "edges_done"): [(ALL, 0)],
        # a lone large frame (scaled image >= 600 000 pixels) gets 64 workers (lsd.hip: `if (n <= 2 && nsp >= 600000) aw = 64;`)
        ("lsd", "async_w"): [(2, 64), (8, 32), (16, 16), (ALL, 0)],
        # the availability mask of k_lsd_grow_lat is 1024 / 32 * 768 words = 96 KB, above the 56 KB floor
        ("lsd", "lat_lds"): [(16, 0), (64, 32 * 768 * 4), (ALL, 0)],
        # frames of 2 x 640 x 480 pixels and more prefer policy 7 (api.hip: big_frames)
        ("batch", "sched"): [(3071, 1), (ALL, 7)],
    },
}


def _steps(w, h, key):
    return GEOMETRY_EXCEPTIONS.get((w, h), {}).get(key, TABLE[key]["steps"])


def _value(steps, n):
    for bound, v in steps:
        if bound is ALL or n <= bound:
            return v(n) if callable(v) else v
    raise AssertionError("no range for n = %d" % n)


def expected_report(w, h, n, stages=7, cull=False):
    """the launch report a batch of n frames of w x h (max_batch = n, no HVO_* variable set) must give, from TABLE"""
    r = {"peac": {}, "lsd": {}, "batch": {}}
    for (stage, field) in TABLE:
        r[stage][field] = _value(_steps(w, h, (stage, field)), n)
    r["batch"]["stages"] = stages
    r["lsd"]["cull"] = 1 if cull else 0
    if not stages & 1:
        r["batch"]["orb_first"] = 0
    if not stages & (2 | 8):
        r["batch"]["lsd_first"] = 0
    return r


def natural_thresholds(w, h):
    """every n at which some field's value range ends: the only places the selection may change form (fields that are a function of n
    within a range -- n itself, ceil(n / 4), ceil(n / 512) -- change inside it, as the table's callables say)"""
    t = set()
    for key in TABLE:
        t.update(b for b, _ in _steps(w, h, key) if b is not ALL)
    return sorted(t)


@pytest.fixture
def clean_env(monkeypatch):
    for k in list(os.environ):
        if k.startswith("HVO_"):
            monkeypatch.delenv(k)
    return monkeypatch


def test_the_table_points_at_the_code():
    """every row names the one place in csrc/ where its threshold is written"""
    src = {}
    for key, row in TABLE.items():
        path = os.path.join(PKG_DIR, "csrc", row["file"])
        lines = src.setdefault(path, open(path).read().split("\n"))
        hits = [i + 1 for i, l in enumerate(lines) if row["text"] in l]
        assert len(hits) == 1, "%s: %r occurs %d times in %s (lines %s; the table says line %d)" % (key, row["text"], len(hits), row["file"], hits, row["line"])


@pytest.mark.parametrize("w,h", GEOMS)
def test_forms_change_only_at_the_thresholds(hvo, clean_env, w, h):
    got = [None] + [hvo.plan_select(w, h, n) for n in range(1, N_MAX + 1)]
    # 1. every n: the table's row
    for n in range(1, N_MAX + 1):
        exp = expected_report(w, h, n)
        for stage in ("peac", "lsd", "batch"):
            assert got[n][stage] is not None, (stage, n)
            assert set(got[n][stage]) == set(exp[stage]), (stage, sorted(set(got[n][stage]) ^ set(exp[stage])))
            bad = {f: (got[n][stage][f], exp[stage][f]) for f in exp[stage] if got[n][stage][f] != exp[stage][f]}
            assert not bad, "%d x %d, n = %d, %s: (selected, table) %s" % (w, h, n, stage, bad)
    # 2. said the other way round, without the table's values: a field whose value is no function of n changes between n and n + 1 only
    #    where n is one of the thresholds
    th = set(natural_thresholds(w, h))
    for key in TABLE:
        steps = _steps(w, h, key)
        if any(callable(v) for _, v in steps):
            continue
        stage, field = key
        changes = [n for n in range(1, N_MAX) if got[n][stage][field] != got[n + 1][stage][field]]
        assert set(changes) <= th, (key, changes)
        assert changes == [b for b, _ in steps if b is not ALL], (key, changes)
    assert th <= {1, 2, 7, 8, 16, 64, 128, 256, 512, 1024, 3071, 5120, 6143}, sorted(th)


def test_max_batch_larger_than_the_batch(hvo, clean_env):
    """the chunk follows the plan (max_batch), the forms follow n; the stream priorities follow max_batch"""
    r = hvo.plan_select(640, 480, 40, max_batch=4096)
    assert r["lsd"]["chunk"] == 512 and r["lsd"]["chunks"] == 1 and r["lsd"]["plan_batch"] == 4096 and r["lsd"]["grow"] == "lat"
    assert r["peac"]["cluster"] == "heads" and r["batch"]["sched"] == 1
    assert (r["batch"]["prio_orb"], r["batch"]["prio_lsd"], r["batch"]["prio_peac"]) == (0, 0, 0)
    r = hvo.plan_select(640, 480, 700, max_batch=300)
    assert r["lsd"]["plan_batch"] == 700 and r["lsd"]["chunks"] == 2


def test_slot_form_is_refused_when_labels_do_not_fit_16_bits(hvo, clean_env):
    """segcap = 2 * blocks + 128 > 32768, i.e. more than 16 320 blocks: k_peac_cluster_slots packs a label into a signed 16-bit half
    (peac_slots.inc), such frames take the lending form.  1640 x 1000 has 16 400 blocks, 1630 x 1000 has 16 300."""
    assert (1640 // 10) * (1000 // 10) > 16320 >= (1630 // 10) * (1000 // 10)
    for n in (3072, 6144):
        big, fits = hvo.plan_select(1640, 1000, n)["peac"], hvo.plan_select(1630, 1000, n)["peac"]
        assert (big["slots_fit"], big["cluster"]) == (0, "c16_lend"), big
        assert (fits["slots_fit"], fits["cluster"]) == (1, "slots"), fits
    clean_env.setenv("HVO_PEAC_GL", "16")
    assert hvo.plan_select(1640, 1000, 5)["peac"]["cluster"] == "c16_lend"


def test_geometries_a_stage_refuses_leave_its_part_empty(hvo, clean_env):
    r = hvo.plan_select(16, 16, 4)                       # PEAC needs two 10 x 10 blocks each way
    assert r["peac"] is None and r["lsd"] is not None and r["batch"] is not None
    r = hvo.plan_select(8, 8, 4)                         # the scaled image of LSD must have 8 x 8 pixels
    assert r["peac"] is None and r["lsd"] is None


def bit_reversal_order(n):
    """the order hvo_frame_perm documents: the indices 0 .. 2^bits - 1 in bit-reversed order, those below n kept"""
    bits = 0
    while (1 << bits) < n:
        bits += 1
    out = []
    for i in range(1 << bits):
        r = int(format(i, "0%db" % bits)[::-1], 2) if bits else 0
        if r < n:
            out.append(r)
    return out


def test_frame_permutation(hvo):
    """every n from 1 to 300 and the batch sizes of test_batch_boundaries_gpu.py (and their wave counts): a permutation of 0 .. n - 1,
    the bit-reversal order, and for n >= 3 not the identity"""
    sizes = list(range(1, 301)) + [512, 513, 768, 1024, 1025, 1280, 1281, 1536, 3071, 3072, 5120, 5121, 6143, 6144, 8191, 8192]
    for n in sizes:
        p = hvo.frame_perm(n).tolist()
        assert sorted(p) == list(range(n)), n
        assert p == bit_reversal_order(n), n
        if n >= 3:
            assert p != list(range(n)), n
    assert hvo.frame_perm(5).tolist() == [0, 4, 2, 1, 3] and hvo.frame_perm(8).tolist() == [0, 4, 2, 6, 1, 5, 3, 7]


# Every knob a GPU test sets, at the geometry and batch size it sets it: (w, h, n, environment, stage, the fields it must select).
# A knob that went dead selects what the line without it selects, and fails here.
KNOBS = [
    # tests/test_peac_gpu.py: flood variants on a lone frame, on 16 frames
    (640, 480, 1, {}, "peac", dict(flood_t=512, flood_epl=1, flood_slim=0)),
    (640, 480, 1, {"HVO_FLOOD_T": "64", "HVO_FLOOD_EPL": "1"}, "peac", dict(flood_t=64, flood_epl=1, flood_slim=1)),
    (640, 480, 1, {"HVO_FLOOD_T": "64", "HVO_FLOOD_EPL": "2"}, "peac", dict(flood_t=64, flood_epl=2, flood_slim=0)),
    (640, 480, 1, {"HVO_FLOOD_T": "128", "HVO_FLOOD_EPL": "1"}, "peac", dict(flood_t=128, flood_epl=1, flood_slim=0)),
    (640, 480, 16, {"HVO_FLOOD_T": "256"}, "peac", dict(flood_t=256)),
    (640, 480, 16, {"HVO_FLOOD_T": "64"}, "peac", dict(flood_t=64, flood_slim=1)),
    # test_peac_flood_pmax_gpu.py
    (640, 480, 8, {"HVO_FLOOD_T": "64"}, "peac", dict(flood_t=64, flood_slim=1)),
    (640, 480, 8, {"HVO_FLOOD_T": "64", "HVO_FLOOD_SLIM": "0"}, "peac", dict(flood_t=64, flood_slim=0)),
    # four frames per wave: slots / lending / grouped, a forced pool, the edges inside the kernel (10 frames; 5 at 200 x 160; 6 at 1280 x 960)
    (640, 480, 10, {}, "peac", dict(cluster="heads", group=64)),
    (640, 480, 10, {"HVO_PEAC_GL": "16", "HVO_PEAC_SLOTS": "1", "HVO_PEAC_LEND": "1"}, "peac", dict(cluster="slots", group=16, cluster_wgs=3, perm_items=3, poolcap=0, edges_done=1)),
    (640, 480, 10, {"HVO_PEAC_GL": "16", "HVO_PEAC_SLOTS": "0", "HVO_PEAC_LEND": "1"}, "peac", dict(cluster="c16_lend", group=16, poolcap=0)),
    (640, 480, 10, {"HVO_PEAC_GL": "16", "HVO_PEAC_SLOTS": "0", "HVO_PEAC_LEND": "0"}, "peac", dict(cluster="c16", group=16, poolcap=0)),
    (640, 480, 10, {"HVO_PEAC_GL": "16", "HVO_PEAC_SLOTS": "1", "HVO_PEAC_LEND": "1", "HVO_PEAC_POOLCAP": "22000"}, "peac", dict(cluster="slots", poolcap=22000)),
    (640, 480, 10, {"HVO_PEAC_GL": "16", "HVO_PEAC_SLOTS": "0", "HVO_PEAC_LEND": "1", "HVO_PEAC_POOLCAP": "22000"}, "peac", dict(cluster="c16_lend", poolcap=22000)),
    (640, 480, 10, {"HVO_PEAC_GL": "16", "HVO_PEAC_SLOTS": "0", "HVO_PEAC_LEND": "0", "HVO_PEAC_POOLCAP": "22000"}, "peac", dict(cluster="c16", poolcap=22000)),
    (640, 480, 10, {"HVO_PEAC_GL": "16", "HVO_PEAC_SLOTS": "1", "HVO_PEAC_LEND": "1", "HVO_PEAC_EDGES": "0"}, "peac", dict(cluster="slots", edges_done=0)),
    (640, 480, 10, {"HVO_PEAC_GL": "16", "HVO_PEAC_SLOTS": "0", "HVO_PEAC_LEND": "1", "HVO_PEAC_EDGES": "0"}, "peac", dict(cluster="c16_lend", edges_done=0)),
    (640, 480, 4, {"HVO_PEAC_GL": "16", "HVO_PEAC_SLOTS": "1", "HVO_PEAC_POOLCAP": "22000"}, "peac", dict(cluster="slots", poolcap=22000)),
    (640, 480, 4, {"HVO_PEAC_GL": "16", "HVO_PEAC_SLOTS": "0", "HVO_PEAC_POOLCAP": "22000"}, "peac", dict(cluster="c16_lend", poolcap=22000)),
    (200, 160, 5, {"HVO_PEAC_GL": "16", "HVO_PEAC_SLOTS": "1"}, "peac", dict(cluster="slots")),
    (200, 160, 5, {"HVO_PEAC_GL": "16", "HVO_PEAC_SLOTS": "0"}, "peac", dict(cluster="c16_lend")),
    (1280, 960, 6, {"HVO_PEAC_GL": "16"}, "peac", dict(cluster="slots", edges_done=0, slots_fit=1)),
    # grouped paths on six frames
    (640, 480, 6, {"HVO_PEAC_GL": "16", "HVO_FLOOD_T": "64"}, "peac", dict(cluster="slots", cluster_wgs=2, flood_t=64, flood_slim=1)),
    (640, 480, 6, {"HVO_PEAC_GL": "16", "HVO_FLOOD_T": "128"}, "peac", dict(cluster="slots", flood_t=128)),
    (640, 480, 6, {"HVO_PEAC_GL": "32", "HVO_FLOOD_T": "128"}, "peac", dict(cluster="c32", group=32, cluster_wgs=3, perm_items=3, flood_t=128)),
    (640, 480, 6, {"HVO_PEAC_GL": "64", "HVO_FLOOD_T": "256"}, "peac", dict(cluster="c64", group=64, cluster_wgs=6, ldsq=1, flood_t=256)),
    # queue heads on seven frames
    (640, 480, 7, {"HVO_PEAC_HEADS": "4"}, "peac", dict(cluster="heads", heads=4, heads_big=0, poolcap=0)),
    (640, 480, 7, {"HVO_PEAC_HEADS": "3"}, "peac", dict(cluster="heads", heads=3, heads_big=0, poolcap=0)),
    (640, 480, 7, {"HVO_PEAC_HEADS": "2"}, "peac", dict(cluster="heads", heads=2, heads_big=0, poolcap=0)),
    (640, 480, 7, {"HVO_PEAC_HEADS": "0"}, "peac", dict(cluster="c64", heads=0, ldsq=1)),
    (640, 480, 1, {"HVO_PEAC_HEADS": "0"}, "peac", dict(cluster="c64", heads=0, ldsq=1)),
    (640, 480, 7, {"HVO_PEAC_HEADS": "4", "HVO_PEAC_POOLCAP": "22000"}, "peac", dict(cluster="heads", heads=4, poolcap=22000)),
    (640, 480, 7, {"HVO_PEAC_HEADS": "3", "HVO_PEAC_POOLCAP": "22000"}, "peac", dict(cluster="heads", heads=3, poolcap=22000)),
    (640, 480, 7, {"HVO_PEAC_HEADS": "3", "HVO_PEAC_HEADS_BIG": "1"}, "peac", dict(cluster="heads", heads=3, heads_big=1)),
    (640, 480, 7, {"HVO_PEAC_HEADS": "2", "HVO_PEAC_HEADS_BIG": "1"}, "peac", dict(cluster="heads", heads=2, heads_big=1)),
    (640, 480, 7, {"HVO_PEAC_HEADS": "4", "HVO_PEAC_POOLCAP": "22000", "HVO_PEAC_HEADS_BIG": "1"}, "peac", dict(cluster="heads", heads=4, heads_big=1, poolcap=22000)),
    # one frame per wave, keys in global memory / in LDS
    (640, 480, 6, {"HVO_PEAC_HEADS_MAXN": "1", "HVO_PEAC_LDSQ": "0"}, "peac", dict(cluster="c64", ldsq=0)),
    (640, 480, 6, {"HVO_PEAC_HEADS_MAXN": "1", "HVO_PEAC_LDSQ": "1"}, "peac", dict(cluster="c64", ldsq=1)),
    # tests/test_lsd_gpu.py: both growing kernels (the async and the latency forms, which small batches take first, switched off)
    (640, 480, 3, {}, "lsd", dict(grow="async", async_w=32)),
    (640, 480, 3, {"HVO_LSD_ASYNC": "0", "HVO_LSD_LAT": "0", "HVO_LSD_DENSE": "0"}, "lsd", dict(grow="grow", async_w=0, async_fallback=0)),
    (640, 480, 3, {"HVO_LSD_ASYNC": "0", "HVO_LSD_LAT": "0", "HVO_LSD_DENSE": "1"}, "lsd", dict(grow="dense", async_w=0, async_fallback=0)),
    (640, 480, 3, {"HVO_LSD_ASYNC": "0"}, "lsd", dict(grow="lat", lat_lds=56 * 1024)),
    # compact records
    (640, 480, 5, {"HVO_LSD_COMPACT": "1", "HVO_LSD_DENSE": "0"}, "lsd", dict(compact=1, grow="grow_c", chunk=5, chunks=1)),
    (640, 480, 5, {"HVO_LSD_COMPACT": "1", "HVO_LSD_DENSE": "1", "HVO_LSD_CHUNK": "2"}, "lsd", dict(compact=1, grow="dense_c", chunk=2, chunks=3)),
    (501, 397, 5, {"HVO_LSD_COMPACT": "1", "HVO_LSD_DENSE": "1", "HVO_LSD_CHUNK": "2"}, "lsd", dict(compact=1, grow="dense_c", chunk=2, chunks=3)),
    # preamble, LBD gradient and descriptor forms
    (640, 480, 2, {"HVO_LSD_PRE_SPLIT": "0"}, "lsd", dict(pre="fused")),
    (640, 480, 2, {"HVO_LSD_PRE_SPLIT": "1"}, "lsd", dict(pre="split", grow="async")),
    (1280, 960, 2, {"HVO_LSD_PRE_SPLIT": "1"}, "lsd", dict(pre="split", grow="async", async_w=64)),
    (640, 480, 3, {"HVO_LBD_SPLIT": "1"}, "lsd", dict(lbd_gradient="split")),
    (640, 480, 3, {"HVO_LSD_PRE_SPLIT": "1", "HVO_LBD_SPLIT": "1"}, "lsd", dict(pre="split", lbd_gradient="split")),
    (160, 120, 1, {}, "lsd", dict(lbd_desc=1)),
    (160, 120, 1, {"HVO_LBD_DESC": "0"}, "lsd", dict(lbd_desc=0)),
    # async growing: workers, the early drop, beyond 16 frames
    (640, 480, 5, {"HVO_LSD_ASYNC": "4", "HVO_LSD_ASYNC_EARLY": "1"}, "lsd", dict(grow="async", async_w=4, async_early=1, async_fallback=1)),
    (640, 480, 5, {"HVO_LSD_ASYNC": "16", "HVO_LSD_ASYNC_EARLY": "0"}, "lsd", dict(grow="async", async_w=16, async_early=0)),
    (640, 480, 5, {"HVO_LSD_ASYNC": "32", "HVO_LSD_ASYNC_EARLY": "1"}, "lsd", dict(grow="async", async_w=32, async_early=1)),
    (640, 480, 5, {"HVO_LSD_ASYNC": "7", "HVO_LSD_ASYNC_EARLY": "0"}, "lsd", dict(grow="async", async_w=7, async_early=0)),
    (1280, 960, 1, {"HVO_LSD_ASYNC": "32"}, "lsd", dict(grow="async", async_w=32)),
    (638, 479, 16, {"HVO_LSD_ASYNC": "8"}, "lsd", dict(grow="async", async_w=8)),
    (640, 480, 40, {}, "lsd", dict(grow="lat", async_w=0)),
    (640, 480, 40, {"HVO_LSD_ASYNC": "3"}, "lsd", dict(grow="async", async_w=3, async_fallback=1)),
    (640, 480, 12, {"HVO_LSD_ASYNC": "3"}, "lsd", dict(grow="async", async_w=3)),
    # tests/test_batch_boundaries_gpu.py: a second chunk without the compact layout
    (200, 160, 17, {"HVO_LSD_CHUNK": "5"}, "lsd", dict(chunk=5, chunks=4, compact=0, grow="lat")),
    # launch orders
    (640, 480, 16, {"HVO_FRAME_PERM": "0"}, "peac", dict(perm_items=0, flood_perm_items=0)),
    (640, 480, 16, {"HVO_FRAME_PERM": "0"}, "lsd", dict(perm_items=0)),
    (640, 480, 16, {"HVO_PEAC_PERM": "0"}, "peac", dict(perm_items=0, flood_perm_items=16)),
    (640, 480, 16, {"HVO_FLOOD_PERM": "0"}, "peac", dict(perm_items=16, flood_perm_items=0)),
    # the overlap policy
    (640, 480, 16, {"HVO_SCHED": "5"}, "batch", dict(sched=5, orb_first=1, lsd_first=0)),
    (640, 480, 16, {"HVO_SCHED": "3"}, "batch", dict(sched=3, peac_last=1, lsd_first=0)),
    (640, 480, 16, {"HVO_PRIO": "2,1,0"}, "batch", dict(prio_orb=2, prio_lsd=1, prio_peac=0)),
]


# settings of the GPU tests that spell out what the batch would take anyway (the other values of the same parametrisation differ)
VALUES_THAT_ARE_THE_DEFAULT = [{"HVO_LSD_PRE_SPLIT": "0"}, {"HVO_LSD_ASYNC": "32", "HVO_LSD_ASYNC_EARLY": "1"}, {"HVO_FLOOD_T": "256"}, {"HVO_PEAC_HEADS": "3"}]


@pytest.mark.parametrize("case", range(len(KNOBS)))
def test_knobs_select_what_the_gpu_tests_mean_them_to(hvo, clean_env, case):
    w, h, n, env, stage, want = KNOBS[case]
    for k, v in env.items():
        clean_env.setenv(k, v)
    got = hvo.plan_select(w, h, n)[stage]
    bad = {f: (got[f], v) for f, v in want.items() if got[f] != v}
    assert not bad, "%s, %d frames of %d x %d, %s: (selected, wanted) %s" % (env, n, w, h, stage, bad)


def test_every_knob_changes_something(hvo, clean_env):
    """each variable of KNOBS, alone or in the combination a test uses it in, selects something the clean environment does not"""
    for w, h, n, env, stage, want in KNOBS:
        if not env or env in VALUES_THAT_ARE_THE_DEFAULT:
            continue
        base = hvo.plan_select(w, h, n)[stage]
        for k, v in env.items():
            clean_env.setenv(k, v)
        got = hvo.plan_select(w, h, n)[stage]
        for k in env:
            clean_env.delenv(k)
        assert got != base, (env, n, stage)
