"""The resident vocabulary, ComputeBoW and SearchByBoW on the GPU (csrc/bow.hip) against tests/bow_ref.py.  Everything is integer arithmetic
or reproducible double arithmetic in a fixed order, so every comparison is exact: integers with array_equal, doubles bit for bit through
.view(np.uint64).  tests/test_bow.py asserts on the CPU that each crafted case reaches the path it is meant for."""
import numpy as np
import pytest

import bow_ref as ref

pytestmark = pytest.mark.gpu
_cache = {}


def ctx_of(hvo):
    if "ctx" not in _cache:
        _cache["ctx"] = hvo.Context(max_batch=4)
    return _cache["ctx"]


def upload(hvo, voc, device=0):
    return hvo.Vocabulary(voc["k"], voc["L"], voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"], voc["scoring"], voc["weighting"], device=device)


def same_bow(got, want, what=""):
    for k in ("word_id", "node_id", "bow_word", "fv_node", "fv_start", "fv_index"):
        assert np.array_equal(got[k], want[k]), (what, k)
    assert np.array_equal(got["bow_value"].view(np.uint64), want["bow_value"].view(np.uint64)), (what, "bow_value")
    assert got["n_short"] == want["n_short"], what


def descs(n, seed, voc=None, near_leaves=False):
    rng = np.random.RandomState(seed)
    d = rng.randint(0, 256, (n, 32)).astype(np.uint8)
    if near_leaves and voc is not None and n:                      # noisy copies of the words' own descriptors: repeated words
        leaves = voc["desc"][voc["is_leaf"] == 1]
        d = leaves[rng.randint(0, len(leaves), n)].copy()
        d[:, rng.randint(0, 32)] ^= rng.randint(0, 256, n).astype(np.uint8)
    return d


def vocab(key, *a, **kw):
    if key not in _cache:
        _cache[key] = ref.make_vocabulary(*a, **kw)
    return _cache[key]


@pytest.mark.parametrize("shape", [(3, 3, 1), (4, 6, 4)])
def test_transform_sizes(hvo, shape):
    """k = 3, L = 3 and k = 4, L = 6 (5461 nodes) at N = 0, 1, 63, 64, 65, 1000: all six frames in ONE call (frames of different counts)"""
    k, L, up = shape
    voc = vocab(shape, k, L, 100 + k)
    v = upload(hvo, voc)
    assert v.info()["n_nodes"] == sum(k ** i for i in range(L + 1)) and v.info()["n_words"] == k ** L
    ds = [descs(n, 7 + n, voc, near_leaves=n == 1000) for n in (0, 1, 63, 64, 65, 1000)]
    got = ctx_of(hvo).compute_bow(v, ds, levelsup=up)
    for d, g in zip(ds, got):
        same_bow(g, ref.transform(voc, d, up), "N=%d" % len(d))
        assert g["computed"]
    one = ctx_of(hvo).compute_bow(v, ds[4], levelsup=up)           # a frame alone equals the frame inside the call of six
    same_bow(one, got[4])
    v.close()


def test_transform_k20_and_levelsup(hvo):
    voc = vocab("k20", 20, 2, 31)
    v = upload(hvo, voc); d = descs(300, 5, voc)
    for up in (0, 1, 2, 5):
        g = ctx_of(hvo).compute_bow(v, d, levelsup=up)
        same_bow(g, ref.transform(voc, d, up), "levelsup=%d" % up)
        if up >= 2:
            assert (g["node_id"] == 0).all() and g["fv_node"].tolist() == [0]      # levelsup >= L: every node id is the root
    v.close()


@pytest.mark.parametrize("weighting", [ref.TF_IDF, ref.TF, ref.IDF, ref.BINARY])
@pytest.mark.parametrize("scoring", [ref.L1_NORM, ref.L2_NORM, ref.DOT_PRODUCT])
def test_weightings_and_norms(hvo, weighting, scoring):
    voc = dict(vocab("w", 3, 3, 17)); voc["weighting"] = weighting; voc["scoring"] = scoring
    v = upload(hvo, voc); d = descs(400, 3, voc, near_leaves=True)
    w = ref.transform(voc, d, 1)
    assert len(w["bow_word"]) < 400                                 # words repeat: the sums have several terms
    same_bow(ctx_of(hvo).compute_bow(v, d, levelsup=1), w)
    v.close()


def test_repeated_sum_is_not_a_product(hvo):
    voc, count = ref.tfidf_case()
    v = upload(hvo, voc); d = np.repeat(voc["desc"][:1], count, axis=0)
    g = ctx_of(hvo).compute_bow(v, d, levelsup=0)
    same_bow(g, ref.transform(voc, d, 0))
    assert g["bow_value"][0] != 0.1 * count
    v.close()


@pytest.mark.parametrize("which", ["root", "leaf"])
def test_duplicate_children_first_wins(hvo, which):
    voc = ref.make_vocabulary(3, 3, 21, dup_root=which == "root", dup_leaf=which == "leaf")
    v = upload(hvo, voc); d = descs(200, 4)
    for up in (0, 2):
        same_bow(ctx_of(hvo).compute_bow(v, d, levelsup=up), ref.transform(voc, d, up), which)
    v.close()


def test_stopped_words_unbalanced_tree_one_word_distinct_words_empty(hvo):
    c = ctx_of(hvo)
    voc = ref.make_vocabulary(3, 2, 6, zero_weight_every=2)         # weight-0 words: absent from both vectors, ids -1
    v = upload(hvo, voc); d = np.concatenate([voc["desc"][voc["is_leaf"] == 1], descs(50, 8)])
    g = c.compute_bow(v, d, levelsup=0); w = ref.transform(voc, d, 0)
    same_bow(g, w); assert (g["word_id"] == -1).sum() >= 3 and np.array_equal(g["word_id"] == -1, g["node_id"] == -1)
    v.close()
    voc = ref.make_vocabulary(3, 3, 5, leaf_at_level1=True)         # a leaf at level 1: n_short and the defined node id
    v = upload(hvo, voc); d = np.concatenate([np.repeat(voc["desc"][:1], 5, axis=0), descs(120, 9)])
    for up in (0, 1, 2):
        g = c.compute_bow(v, d, levelsup=up); w = ref.transform(voc, d, up)
        same_bow(g, w, "unbalanced levelsup=%d" % up)
        assert (g["n_short"] >= 5) == (up < 2) and (up == 2 or (g["node_id"][:5] == 1).all())
    v.close()
    voc = vocab("w", 3, 3, 17); v = upload(hvo, voc)
    leaves = voc["desc"][voc["is_leaf"] == 1]
    g = c.compute_bow(v, np.repeat(leaves[:1], 300, axis=0), levelsup=1)                 # all N features in one word
    same_bow(g, ref.transform(voc, np.repeat(leaves[:1], 300, axis=0), 1)); assert len(g["bow_word"]) == 1
    dw = ref.distinct_word_descriptors(voc)                                              # N distinct words
    g = c.compute_bow(v, dw, levelsup=1); w = ref.transform(voc, dw, 1)
    same_bow(g, w); assert len(g["bow_word"]) == len(dw) >= 20
    v.close()
    voc = ref.empty_vocabulary(); v = upload(hvo, voc)                                  # the empty vocabulary: empty vectors
    g = c.compute_bow(v, descs(10, 1), levelsup=0)
    same_bow(g, ref.transform(voc, descs(10, 1), 0)); assert len(g["bow_word"]) == 0 and len(g["fv_node"]) == 0 and (g["word_id"] == -1).all()
    v.close()


def test_validation_refusals_on_the_device(hvo):
    bad = ref.make_vocabulary(2, 2, 1); bad["parent"][2] = 3
    with pytest.raises(hvo.HvoError):
        upload(hvo, bad)
    bad = ref.make_vocabulary(2, 2, 1); bad["is_leaf"][-1] = 0
    with pytest.raises(hvo.HvoError):
        upload(hvo, bad)
    host_only = upload(hvo, ref.make_vocabulary(2, 2, 1), device=-1)
    with pytest.raises(hvo.HvoError):
        ctx_of(hvo).compute_bow(host_only, descs(4, 1), levelsup=0)
    v = upload(hvo, vocab("w", 3, 3, 17))
    with pytest.raises(hvo.HvoError):
        ctx_of(hvo).compute_bow(v, descs(4097, 1), levelsup=0)       # beyond 4096 features: refused, not truncated
    v.close()


def frames(hvo, synth):
    """three synthetic frames of different feature counts (std, low texture, std), shared and never modified"""
    if "fr" not in _cache:
        g = np.stack([synth.make_frame("std", 0x5EED0101)[0], synth.make_frame("lowtex", 0x5EED0102)[0], synth.make_frame("std", 0x5EED0103)[0]])
        _cache["fr"] = g
    return _cache["fr"]


def test_forms_agree_and_second_call_is_a_noop(hvo, synth):
    g = frames(hvo, synth)
    voc = vocab((4, 6, 4), 4, 6, 104); v = upload(hvo, voc)
    st = hvo.Stream(depth=4, stages=hvo.STAGE_ORB, bf=0.0); c = ctx_of(hvo)
    try:
        tk = [st.submit(g[i]) for i in range(3)]
        fr = [st.collect(t) for t in tk]
        assert len({len(f["desc"]) for f in fr}) == 3                  # three different feature counts
        host = c.compute_bow(v, [f["desc"] for f in fr], levelsup=4)
        for i in range(3):
            same_bow(host[i], ref.transform(voc, fr[i]["desc"], 4), "frame %d" % i)
            s = st.compute_bow(tk[i], v, levelsup=4)
            assert s["computed"]; same_bow(s, host[i], "stream %d" % i)
        again = st.compute_bow(tk[1], v, levelsup=4)                   # `if (mBowVec.empty())`: nothing runs, the same result
        assert not again["computed"]; same_bow(again, host[1])
        other = st.compute_bow(tk[1], v, levelsup=2)                   # another levelsup recomputes
        assert other["computed"]; same_bow(other, ref.transform(voc, fr[1]["desc"], 2))
        c.batch_upload(g); c.batch_run(hvo.STAGE_ORB)
        b = c.batch_compute_bow(v, 3, levelsup=4)
        for i in range(3):
            assert b[i]["computed"]; same_bow(b[i], host[i], "batch %d" % i)
        b2 = c.batch_compute_bow(v, 2, levelsup=4)
        assert not b2[0]["computed"]; same_bow(b2[1], host[1])
        c.batch_run(hvo.STAGE_ORB)
        assert c.batch_compute_bow(v, 3, levelsup=4)[2]["computed"]      # a new run drops the kept result
        # SearchByBoW on the resident frame equals the host-array form
        s0 = st.compute_bow(tk[0], v, levelsup=4)
        # key frames: frame 0 itself in reversed feature order (every feature has its twin), and frame 2
        kfs = [dict(desc=fr[j]["desc"][::o], node_id=host[j]["node_id"][::o], has_map_point=(np.arange(len(fr[j]["desc"])) % 5 != 0), angle=fr[j]["kp"]["angle"][::o])
               for j, o in ((0, -1), (2, 1))]
        frame = dict(desc=fr[0]["desc"], node_id=s0["node_id"], angle=fr[0]["kp"]["angle"])
        n0 = len(fr[0]["desc"])
        for orient in (True, False):
            hs = c.search_by_bow(frame, kfs, nnratio=0.9, check_orientation=orient, th_low=80)
            ss = st.search_by_bow(tk[0], v, kfs, nnratio=0.9, check_orientation=orient, th_low=80)
            for j in range(2):
                want = ref.search_by_bow(kfs[j], frame, 0.9, orient, 80)
                assert np.array_equal(hs[j][0], want[0]) and hs[j][1] == want[1] and (j == 1 or want[1] > 100)
                assert np.array_equal(ss[j][0][:n0], want[0]) and ss[j][1] == want[1] and (ss[j][0][n0:] == -1).all()
        v2 = upload(hvo, vocab("w", 3, 3, 17))
        with pytest.raises(hvo.HvoError):
            st.search_by_bow(tk[2], v2, kfs)                           # frame 2 holds a bag of words of ANOTHER vocabulary
        v2.close()
    finally:
        st.close(); v.close()


def run_search(hvo, kf, fr, **kw):
    got = ctx_of(hvo).search_by_bow(fr, [kf], **kw)[0]
    want = ref.search_by_bow(kf, fr, kw.get("nnratio", 0.7), kw.get("check_orientation", True), kw.get("th_low", 50))
    assert np.array_equal(got[0], want[0]) and got[1] == want[1]
    return got


@pytest.mark.parametrize("n", [100, 1000])
def test_search_random_pairs(hvo, n):
    kf, fr = ref.random_pair(n, n, 40 + n, n_nodes=12 if n == 100 else 60)
    for orient in (True, False):
        m, nm = run_search(hvo, kf, fr, check_orientation=orient)
        assert nm > n // 10


def test_search_big_node_and_claim_chain(hvo):
    kf, fr = ref.big_node_case()                                    # 130 candidates, 70 key-frame features in one node: the wave loops
    m, nm = run_search(hvo, kf, fr, check_orientation=False)
    assert m[129] == 0 and nm >= 10
    kf, fr = ref.chain_case()
    m, nm = run_search(hvo, kf, fr, check_orientation=False)
    assert m.tolist() == [0, -1, 1, -1, 2, -1]


def test_search_thresholds_ties_and_single_candidate(hvo):
    assert run_search(hvo, *ref.pair_at(50, 200), check_orientation=False)[1] == 1          # best = 50 = TH_LOW is accepted
    assert run_search(hvo, *ref.pair_at(51, 200), check_orientation=False)[1] == 0
    assert run_search(hvo, *ref.pair_at(28, 40), nnratio=0.7, check_orientation=False)[1] == 0   # (float)28 == 0.7f * 40.f: not below
    assert run_search(hvo, *ref.pair_at(27, 40), nnratio=0.7, check_orientation=False)[1] == 1
    m, nm = run_search(hvo, *ref.pair_at(10, 10, n_extra=2), nnratio=1.5, check_orientation=False)
    assert m.tolist() == [0, -1, -1, -1]                             # a tie for best at positions 0 and 1: the first
    assert run_search(hvo, *ref.pair_at(30, None), check_orientation=False)[1] == 1         # a single candidate: second = 256


def test_search_map_points_one_sided_nodes_orientation_and_empties(hvo):
    kf, fr = ref.random_pair(200, 200, 3)
    kf["has_map_point"][:] = 0
    assert run_search(hvo, kf, fr)[1] == 0                           # no key-frame feature has a map point
    kf, fr = ref.random_pair(200, 200, 3)
    kf["node_id"][kf["node_id"] >= 0] += 1000
    assert run_search(hvo, kf, fr)[1] == 0                           # no node on both sides
    kf, fr = ref.random_pair(200, 200, 3)
    kf["node_id"][::2] = 777; fr["node_id"][::3] = 888              # nodes on one side only beside shared ones
    assert run_search(hvo, kf, fr, check_orientation=False)[1] > 5
    kf, fr = ref.bin30_case()                                       # angle differences in bin 30 -> 0: only membership of bin 0 decides
    m, nm = run_search(hvo, kf, fr, check_orientation=True)
    assert nm == 16 and (m[:16] >= 0).all() and (m[16:] == -1).all()
    assert run_search(hvo, kf, fr, check_orientation=False)[1] == 21
    kf, fr = ref.random_pair(50, 60, 8)
    empty = dict(desc=np.zeros((0, 32), np.uint8), node_id=np.zeros(0, np.int32), has_map_point=np.zeros(0, np.uint8), angle=np.zeros(0, np.float32))
    m, nm = ctx_of(hvo).search_by_bow(fr, [empty])[0]
    assert nm == 0 and (m == -1).all() and len(m) == 60
    m, nm = ctx_of(hvo).search_by_bow(empty, [kf])[0]
    assert nm == 0 and len(m) == 0


def test_search_three_keyframes_stay_independent(hvo):
    """n_kf = 3 in one launch: the three key frames want the same frame features; each result equals its own single call"""
    kf0, fr = ref.random_pair(300, 300, 12)
    rng = np.random.RandomState(2)
    kfs = [kf0]
    for s in (1, 2):
        k = {a: b.copy() for a, b in kf0.items()}
        p = rng.permutation(300)[: 300 - 40 * s]                     # the same features in another order and number: other indices, the same claims
        kfs.append({a: b[p] for a, b in k.items()})
    got = ctx_of(hvo).search_by_bow(fr, kfs, check_orientation=True)
    for j in range(3):
        want = ref.search_by_bow(kfs[j], fr)
        assert np.array_equal(got[j][0], want[0]) and got[j][1] == want[1] and want[1] > 30
    assert ((got[0][0] >= 0) & (got[1][0] >= 0)).sum() > 20           # overlapping claims


def test_kernel_times_are_reported(hvo):
    c = ctx_of(hvo)
    voc = vocab("w", 3, 3, 17); v = upload(hvo, voc)
    kf, fr = ref.random_pair(200, 200, 3)
    b = c.compute_bow(v, fr["desc"], levelsup=1)
    c.search_by_bow(dict(desc=fr["desc"], node_id=b["node_id"], angle=fr["angle"]), [kf])
    t_bow, t_search = c.bow_last_kernel_ms()
    assert 0 < t_bow < 50 and 0 < t_search < 50                     # device ms of the two launch groups: measured, and sane
    v.close()


def test_example_runs(hvo, synth, tmp_path):
    """examples/track_reference_kf.cpp linked against the library and run on two frames of a synthetic sequence: ComputeBoW, SearchByBoW, the
    line and plane matchers and PoseOptimization on the resident frame"""
    import os
    import re
    import subprocess
    from conftest import ROOT, PKG_DIR
    csrc = os.path.join(PKG_DIR, "csrc"); exe = str(tmp_path / "track_reference_kf")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "track_reference_kf.cpp"),
                           "-L" + csrc, "-lhvo", "-Wl,-rpath," + csrc, "-o", exe])
    g, d, _ = synth.make_sequence("std", 0x5EED7100, 2)
    args = []
    for i in range(2):
        g[i].tofile(tmp_path / ("g%d.u8" % i)); d[i].tofile(tmp_path / ("d%d.u16" % i))
        args += [str(tmp_path / ("g%d.u8" % i)), str(tmp_path / ("d%d.u16" % i))]
    out = subprocess.check_output([exe] + args).decode()
    k = re.search(r"key frame 0: (\d+) points \((\d+) words, (\d+) nodes\)", out)
    t = re.search(r"frame 1: (\d+) points \((\d+) words\), SearchByBoW (\d+) matches, (\d+) line matches, (\d+) planes -> inliers (\d+)", out)
    assert k and t, out
    assert int(k.group(1)) > 500 and 100 < int(k.group(2)) <= 512 and 32 < int(k.group(3)) <= 64     # k = 8, L = 3, levelsup 1: at most 64 nodes at level 2
    assert int(t.group(3)) >= 100 and int(t.group(6)) >= 100, out                                # consecutive frames: matches, and a pose they support
