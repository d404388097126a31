"""The key-frame database on the GPU (csrc/kf_db.hip) against tests/kf_db_ref.py, the literal inverted file.  Every comparison is exact:
candidate lists, common words, pBestKF and the counts as integers, the scores, accScore and bestAccScore by their bits (.view(np.uint32)).
tests/test_kf_db.py asserts on the CPU that each crafted case and the random scripts reach the paths they are meant for.

(The 125-word vocabulary holds bags of at most 125 distinct words; the 200-word bags run on the 1000-word vocabulary.)"""
import numpy as np
import pytest

import bow_ref
import kf_db_ref as ref

pytestmark = pytest.mark.gpu
_cache = {}
INT_KEYS = ("candidates", "words", "best")
BIT_KEYS = ("score", "acc")
COUNT_KEYS = ("n_sharing", "max_common", "min_common", "n_scored")


def vocab(hvo, k, L, scoring=ref.L1_NORM):
    """an uploaded vocabulary of k^L words; the host side is generated once per shape"""
    if (k, L) not in _cache:
        _cache[(k, L)] = bow_ref.make_vocabulary(k, L, 300 + k + L)
    voc = dict(_cache[(k, L)]); voc["scoring"] = scoring
    return voc, hvo.Vocabulary(voc["k"], voc["L"], voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"], voc["scoring"], voc["weighting"])


class Dev:
    """the device database behind the methods a script plays"""

    def __init__(self, hvo, v):
        self.db = hvo.KeyFrameDatabase(v)

    def add(self, slot, w, v):
        self.db.add(slot, w, v)

    def erase(self, slot):
        self.db.erase(slot)

    def clear(self):
        self.db.clear()

    def set_covisible(self, slot, slots):
        self.db.set_covisible(slot, slots)

    def query(self, w, v, mode, min_score, connected):
        return self.db.query(w, v, mode, min_score, connected, views=True)


def bits(a):
    return np.asarray(a, np.float32).reshape(-1).view(np.uint32)


def same(got, want, what=""):
    for k in INT_KEYS:
        assert np.array_equal(got[k], want[k]), (what, k, got[k], want[k])
    for k in COUNT_KEYS:
        assert got[k] == want[k], (what, k, got[k], want[k])
    for k in BIT_KEYS:
        assert np.array_equal(bits(got[k]), bits(want[k])), (what, k)
    assert bits(got["best_acc_score"])[0] == bits(want["best_acc_score"])[0], (what, "best_acc_score", got["best_acc_score"], want["best_acc_score"])


def same_kept(dev, rdb, what=""):
    for s in rdb.kf:
        w, v, sc = dev.db.get(s)
        assert np.array_equal(w, np.array(rdb.kf[s].words, np.int32)) and np.array_equal(v.view(np.uint64), np.array(rdb.kf[s].values).view(np.uint64)), (what, s)
        assert np.array_equal(bits(sc), bits(rdb.kept(s))), (what, s, sc, rdb.kept(s))


def play(hvo, v, n_words, scoring, script, what="", check_kept=False):
    dev = Dev(hvo, v); rdb = ref.Database(n_words, scoring)
    try:
        got = ref.run_script(dev, script); want = ref.run_script(rdb, script)
        assert len(got) == len(want) > 0
        for i, (g, w) in enumerate(zip(got, want)):
            same(g, w, "%s query %d" % (what, i))
        if check_kept:
            same_kept(dev, rdb, what)
        assert dev.db.info()["n_live"] == len(rdb.kf)
        return got
    finally:
        dev.db.close()


def slots_for(n):
    """n + holes non-contiguous slot numbers, the last one 16383 once there are two"""
    holes = min(5, n // 3)
    s = [3 * i + 1 for i in range(n + holes)]
    if n >= 2:
        s[-1] = 16383
    return s, holes


@pytest.mark.parametrize("mode", [ref.RELOC, ref.LOOP])
@pytest.mark.parametrize("n", [0, 1, 2, 63, 64, 65, 300])
def test_database_sizes(hvo, n, mode):
    """0 .. 300 live slots with erased ones between them, bags of 1, 63, 64, 65 and 125 words on the 125-word vocabulary, three queries in sequence"""
    voc, v = vocab(hvo, 5, 3)
    s, holes = slots_for(n)
    script = ref.random_script(1000 + 7 * n + mode, 125, s, [1, 63, 64, 65, 125], n_queries=3, mode=mode, holes=holes)
    got = play(hvo, v, 125, ref.L1_NORM, script, "n=%d mode=%d" % (n, mode), check_kept=True)
    if n == 0:
        assert all(len(g["candidates"]) == 0 and g["n_sharing"] == 0 for g in got)
    if n >= 63:
        assert any(len(g["candidates"]) > 0 for g in got) and len(got[0]["words"]) == 16384
    v.close()


def test_chunks_cross_several_rounds(hvo):
    """1000-word vocabulary, bags of 500 and 200 words, a query of 700: the slot chunks, the LDS table and the ordered sum span several 64-lane rounds"""
    voc, v = vocab(hvo, 10, 3)
    for mode in (ref.RELOC, ref.LOOP):
        script = ref.random_script(77 + mode, 1000, list(range(2, 82, 2)), [500, 200], n_queries=2, query_size=700, mode=mode, holes=3)
        got = play(hvo, v, 1000, ref.L1_NORM, script, "1000 words mode=%d" % mode, check_kept=True)
        assert got[0]["max_common"] > 128 and got[0]["n_scored"] > 1
    v.close()


def test_bag_of_4096_words(hvo):
    voc, v = vocab(hvo, 8, 4)
    assert v.info()["n_words"] == 4096
    rng = np.random.RandomState(3)
    full = np.arange(4096, dtype=np.int32)
    val = lambda n: (lambda x: x / x.sum())(0.05 + rng.rand(n))
    script = [ref.A(0, full, val(4096)), ref.A(1, full[::2], val(2048)), ref.A(5, full[:4000], val(4000)), ref.A(6, full[100:], val(3996)),
              ("cov", 0, [5, 6]), ("cov", 5, [0]), ref.Q(full, val(4096)), ref.Q(full[7:], val(4089))]
    got = play(hvo, v, 4096, ref.L1_NORM, script, "4096", check_kept=True)
    assert got[0]["max_common"] == 4096 and got[0]["n_scored"] == 3 and got[0]["words"].tolist()[:7] == [4096, 2048, 0, 0, 0, 4000, 3996]
    v.close()


@pytest.mark.parametrize("name", sorted(ref.CRAFTED))
def test_crafted_cases(hvo, name):
    voc, v = vocab(hvo, 5, 3)
    play(hvo, v, ref.N_CRAFT_WORDS, ref.L1_NORM, ref.CRAFTED[name](), name, check_kept=True)
    v.close()


@pytest.mark.parametrize("scoring", [ref.L1_NORM, ref.L2_NORM, ref.CHI_SQUARE, ref.BHATTACHARYYA, ref.DOT_PRODUCT])
def test_scoring_types(hvo, scoring):
    """each scoring on a vocabulary of that type, bags normalised by its norm; bit for bit, L1 like the others"""
    voc, v = vocab(hvo, 10, 3, scoring)
    for mode in (ref.RELOC, ref.LOOP):
        script = ref.random_script(500 + scoring, 1000, list(range(70)), [130, 64, 200], scoring=scoring, n_queries=3, query_size=300, mode=mode, holes=4)
        got = play(hvo, v, 1000, scoring, script, "scoring %d mode %d" % (scoring, mode), check_kept=True)
        assert any(g["n_scored"] > 1 for g in got)
    v.close()


def test_chi_square_guard_and_l2_clamp(hvo):
    """values of 0 on both sides (vi + wi == 0: nothing is added, no 0 / 0) and an L2 sum >= 1 (the clamp)"""
    w = np.arange(10, 15, dtype=np.int32)
    for scoring, kv, qv in ((ref.CHI_SQUARE, [0.0, 0.5, 0.0, 0.25, 0.25], [0.0, 0.5, 0.25, 0.0, 0.25]), (ref.L2_NORM, [1.0, 1.0, 0.5, 0.5, 0.5], [1.0, 0.5, 0.5, 0.5, 0.5])):
        voc, v = vocab(hvo, 5, 3, scoring)
        got = play(hvo, v, 125, scoring, [ref.A(0, w, kv), ref.A(1, w, qv), ref.Q(w, qv)], "guard %d" % scoring)
        assert not np.isnan(got[0]["score"][:2]).any()
        if scoring == ref.L2_NORM:
            assert got[0]["score"][0] == 1.0
        v.close()


def test_kl_is_refused(hvo):
    voc, v = vocab(hvo, 5, 3, ref.KL)
    db = hvo.KeyFrameDatabase(v)
    db.add(0, [1, 2], [0.5, 0.5])
    with pytest.raises(hvo.HvoError) as e:
        db.query([1, 2], [0.5, 0.5])
    assert e.value.status == -4 and "KL" in db.last_error()
    db.close(); v.close()


def test_pool_growth_and_a_slot_that_moves(hvo):
    """300 bags into a database created empty (the pool doubles once its first 65536 words are used: one device copy), then a slot erased and added
    again with a larger bag (a new room at the pool's end); the bags read back and the answers are those of the restatement throughout"""
    voc, v = vocab(hvo, 10, 3)
    script = ref.random_script(91, 1000, list(range(300)), [200, 250], n_queries=1, query_size=300)
    adds = [op for op in script if op[0] == "add"]; rest = [op for op in script if op[0] != "add"]
    dev = Dev(hvo, v); rdb = ref.Database(1000)
    assert dev.db.info()["pool_capacity"] == 0
    ref.run_script(dev, adds[:200]); ref.run_script(rdb, adds[:200])
    cap0 = dev.db.info()["pool_capacity"]
    ref.run_script(dev, adds[200:]); ref.run_script(rdb, adds[200:])
    i = dev.db.info()
    assert i["pool_capacity"] == 2 * cap0 and i["pooled_words"] == 300 * 256 > cap0 and i["next_sequence"] == 300
    same_kept(dev, rdb, "after growth")
    same(ref.run_script(dev, rest)[0], ref.run_script(rdb, rest)[0], "after growth")
    rng = np.random.RandomState(4)
    big = ref.near_bag(rng, 1000, rdb.kf[10].words, 600, 0.9, "L1")
    small = ref.near_bag(rng, 1000, rdb.kf[11].words, 100, 0.9, "L1")
    more = [("erase", 10), ref.A(10, *big), ("erase", 11), ref.A(11, *small), ("cov", 10, [0, 20, 30]), rest[-1]]
    g = ref.run_script(dev, more); w = ref.run_script(rdb, more)
    same(g[0], w[0], "after the move")
    j = dev.db.info()
    assert j["pooled_words"] == i["pooled_words"] + 640 and j["n_live"] == 300      # slot 10 moved to a room of 640, slot 11 stayed in its own
    same_kept(dev, rdb, "after the move")
    dev.db.clear(); rdb.clear()
    assert dev.db.info()["n_live"] == 0 and dev.db.info()["n_slots"] == 0 and dev.db.info()["pooled_words"] == 0
    same(ref.run_script(dev, [adds[0], adds[1], rest[-1]])[0], ref.run_script(rdb, [adds[0], adds[1], rest[-1]])[0], "after clear")
    dev.db.close(); v.close()


def test_more_candidates_than_the_lds_sort_holds(hvo):
    """2100 one-word slots added in a shuffled order all become candidates: the select kernel sorts in global scratch (above 2048 entries) and the
    list is the add order, not the slot order"""
    voc, v = vocab(hvo, 5, 3)
    order = np.random.RandomState(8).permutation(2100).tolist()
    script = [ref.A(s, [7], [1.0]) for s in order] + [ref.Q([7, 9], [0.5, 0.5])]
    got = play(hvo, v, 125, ref.L1_NORM, script, "2100")
    assert got[0]["candidates"].tolist() == order
    v.close()


def frames(synth):
    if "fr" not in _cache:
        _cache["fr"] = np.stack([synth.make_frame("std", 0x5EED0101)[0], synth.make_frame("lowtex", 0x5EED0102)[0], synth.make_frame("std", 0x5EED0103)[0]])
    return _cache["fr"]


def test_stream_and_batch_forms(hvo, synth):
    """on resident 640 x 480 frames: the stream query equals the host query on the downloaded bag, hvo_stream_keyframe_db_add equals add of the
    downloaded bag, the batch form of three frames equals three stream calls in order, a frame with another vocabulary's bag is refused"""
    g = frames(synth)
    voc, v = vocab(hvo, 4, 6)
    st = hvo.Stream(depth=4, stages=hvo.STAGE_ORB, bf=0.0); c = hvo.Context(max_batch=4)
    dbs = []
    try:
        tk = [st.submit(g[i]) for i in range(3)]
        for t in tk:
            st.collect(t)
        bow = [st.compute_bow(t, v, levelsup=4) for t in tk]
        nw = [len(b["bow_word"]) for b in bow]
        assert min(nw) >= 8 and max(nw) > 300, nw                   # (the low-texture frame holds few words)
        rng = np.random.RandomState(21)
        base = [("add", 2 + i, *ref.near_bag(rng, 4096, bow[i % 3]["bow_word"], nw[i % 3] - (nw[i % 3] // 40) * (i // 3), 0.9, "L1")) for i in range(12)]
        cov = [("cov", 2 + i, [2 + (i + 3) % 12, 2 + (i + 6) % 12, 40]) for i in range(12)] + [("cov", 40, [2, 3])]

        def make(stream_add):
            d = Dev(hvo, v); dbs.append(d)
            ref.run_script(d, base)
            if stream_add:
                d.db.add(40, st, ticket=tk[0])
            else:
                d.add(40, bow[0]["bow_word"], bow[0]["bow_value"])
            ref.run_script(d, cov)
            return d

        a, b = make(True), make(False)
        rdb = ref.Database(4096); ref.run_script(rdb, base + [ref.A(40, bow[0]["bow_word"], bow[0]["bow_value"])] + cov)
        ga, gb = a.db.get(40), b.db.get(40)                         # the device-to-device add holds the downloaded bag
        assert np.array_equal(ga[0], gb[0]) and np.array_equal(ga[1].view(np.uint64), gb[1].view(np.uint64)) and np.array_equal(ga[0], bow[0]["bow_word"])
        for i in (1, 0, 2):                                         # three queries in sequence on each: stream, host, restatement
            s = st.keyframe_db_query(tk[i], a.db, views=True)
            h = b.query(bow[i]["bow_word"], bow[i]["bow_value"], ref.RELOC, 0.0, None)
            w = rdb.query(bow[i]["bow_word"], bow[i]["bow_value"])
            same(s, h, "stream vs host %d" % i); same(s, w, "stream vs restatement %d" % i)
            assert len(s["candidates"]) > 0 and a.db.DetectRelocalizationCandidates(st, tk[i]) is not None
        lp = st.keyframe_db_query(tk[1], a.db, mode=ref.LOOP, min_score=0.01, connected=[3, 40], views=True)
        same(lp, b.query(bow[1]["bow_word"], bow[1]["bow_value"], ref.LOOP, 0.01, [3, 40]), "stream loop")
        # the batch form: frames 0, 1, 2 in that order on a fresh database = three stream calls on another
        c.batch_upload(g); c.batch_run(hvo.STAGE_ORB)
        bb = c.batch_compute_bow(v, 3, levelsup=4)
        assert all(np.array_equal(bb[i]["bow_word"], bow[i]["bow_word"]) for i in range(3))
        p, q = make(False), make(False)
        rb = c.batch_keyframe_db_query(v, p.db, 3, views=True)
        for i in range(3):
            same(rb[i], st.keyframe_db_query(tk[i], q.db, views=True), "batch frame %d" % i)
        same_kept_pair = [np.array_equal(bits(p.db.get(s)[2]), bits(q.db.get(s)[2])) for s in list(range(2, 14)) + [40]]
        assert all(same_kept_pair)
        # refusals: a frame whose bag belongs to another vocabulary, a frame that has none, a database of another vocabulary
        voc2, v2 = vocab(hvo, 5, 3)
        st.compute_bow(tk[2], v2, levelsup=1)
        before = a.db.info()
        for call in (lambda: st.keyframe_db_query(tk[2], a.db), lambda: st.keyframe_db_add(tk[2], a.db, 100), lambda: st.keyframe_db_query(tk[2], a.db, voc=v2),
                     lambda: c.batch_keyframe_db_query(v2, a.db, 3)):
            with pytest.raises(hvo.HvoError) as e:
                call()
            assert e.value.status == -1 and "vocabulary" in a.db.last_error()
        assert a.db.info() == before
        v2.close()
    finally:
        for d in dbs:
            d.db.close()
        st.close(); c.close(); v.close()


def test_limits_refuse_whole_with_a_reason(hvo):
    voc, v = vocab(hvo, 5, 3)
    script = ref.CRAFTED["best_differs"]()
    dev = Dev(hvo, v); rdb = ref.Database(125)
    ref.run_script(dev, script[:-1]); ref.run_script(rdb, script[:-1])
    db = dev.db
    before = db.info(); kept = [db.get(s) for s in (0, 1, 2)]
    w5 = np.arange(5, dtype=np.int32); v5 = np.full(5, 0.2)
    bad = [
        (lambda: db.add(-1, w5, v5), -1, "outside"), (lambda: db.add(16384, w5, v5), -1, "outside"),
        (lambda: db.add(1, w5, v5), -1, "live"),
        (lambda: db.add(7, np.arange(4097), np.full(4097, 0.1)), -4, "4096"),
        (lambda: db.add(7, [3, 2, 5], [0.1, 0.1, 0.1]), -1, "ascending"), (lambda: db.add(7, [3, 3], [0.1, 0.1]), -1, "ascending"),
        (lambda: db.add(7, [3, 125], [0.1, 0.1]), -1, "vocabulary"), (lambda: db.add(7, [-1, 3], [0.1, 0.1]), -1, "vocabulary"),
        (lambda: db.add(7, [3, 4], [0.1, -0.1]), -1, "negative"), (lambda: db.add(7, [3, 4], [0.1, np.nan]), -1, "finite"),
        (lambda: db.set_covisible(0, list(range(11))), -1, "10"), (lambda: db.set_covisible(7, [0]), -1, "not live"), (lambda: db.set_covisible(16384, [0]), -1, "outside"),
        (lambda: db.get(7), -1, "not live"), (lambda: db.erase(-1), -1, "outside"),
        (lambda: db.query(w5, v5, mode=2), -1, "mode"), (lambda: db.query([4, 3], [0.5, 0.5]), -1, "ascending"),
        (lambda: db.query(np.arange(4097), np.full(4097, 0.1)), -4, "4096"),
        (lambda: db.query(script[-1][1], script[-1][2], cap=1), -5, "candidates"),     # two candidates: refused, and the kept scores stay as they were
    ]
    for call, status, word in bad:
        with pytest.raises(hvo.HvoError) as e:
            call()
        assert e.value.status == status and word in db.last_error(), (status, word, e.value.status, db.last_error())
        assert db.info() == before
    for s, k in zip((0, 1, 2), kept):
        g = db.get(s)
        assert np.array_equal(g[0], k[0]) and np.array_equal(g[1].view(np.uint64), k[1].view(np.uint64)) and np.array_equal(bits(g[2]), bits(k[2]))
    db.erase(9); db.erase(9)                                            # erasing what is not there does nothing
    assert db.info() == before
    same(dev.query(*script[-1][1:]), rdb.query(*script[-1][1:]), "after the refusals")
    host_only = hvo.Vocabulary(voc["k"], voc["L"], voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"], device=-1)
    with pytest.raises(hvo.HvoError):
        hvo.KeyFrameDatabase(host_only)
    host_only.close(); db.close(); v.close()


def test_kernel_time_is_reported(hvo):
    voc, v = vocab(hvo, 10, 3)
    dev = Dev(hvo, v)
    ref.run_script(dev, ref.random_script(5, 1000, list(range(64)), [200], n_queries=1, query_size=300))
    assert 0 < dev.db.last_kernel_ms() < 50                          # device ms of the four kernels: measured, and sane
    dev.db.close(); v.close()


def test_example_runs(hvo, synth, tmp_path):
    """examples/keyframe_db.cpp linked against the library and run on a synthetic sequence: three key frames added device to device, the
    fourth frame finds candidates among them and matches them by bag of words"""
    import os
    import re
    import subprocess
    from conftest import ROOT, PKG_DIR
    csrc = os.path.join(PKG_DIR, "csrc"); exe = str(tmp_path / "keyframe_db")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "keyframe_db.cpp"),
                           "-L" + csrc, "-lhvo", "-Wl,-rpath," + csrc, "-o", exe])
    g, d, _ = synth.make_sequence("std", 0x5EED7100, 4)
    args = []
    for i in range(4):
        g[i].tofile(tmp_path / ("g%d.u8" % i)); d[i].tofile(tmp_path / ("d%d.u16" % i))
        args += [str(tmp_path / ("g%d.u8" % i)), str(tmp_path / ("d%d.u16" % i))]
    out = subprocess.check_output([exe] + args).decode()
    m = re.search(r"frame: (\d+) points \((\d+) words\), (\d+) of 3 key frames are candidates", out)
    assert m and int(m.group(1)) > 500 and int(m.group(3)) >= 1, out
    assert re.search(r"candidate \d: SearchByBoW (\d+) matches", out) and max(int(x) for x in re.findall(r"SearchByBoW (\d+) matches", out)) >= 50, out


def test_loop_candidates_through_the_class(hvo):
    voc, v = vocab(hvo, 5, 3)
    script = ref.CRAFTED["loop_connected"]()
    dev = Dev(hvo, v); ref.run_script(dev, script[:-1])
    q = script[-1]
    assert dev.db.DetectLoopCandidates((q[1], q[2]), [0], 0.3) == [1] and dev.db.DetectLoopCandidates(dict(bow_word=q[1], bow_value=q[2]), [], 0.3) == [0]
    dev.db.close(); v.close()
