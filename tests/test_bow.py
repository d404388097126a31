"""The bag-of-words restatement (tests/bow_ref.py) on answers worked by hand, the generators of the crafted cases tests/test_bow_gpu.py runs
(each must reach the path it is meant for -- that cannot be asserted on the GPU), and the parts of the feature that need no device: the text
loader, the host-side validation, the binding's names."""
import math
import re

import numpy as np
import pytest

import bow_ref as ref
from conftest import ROOT


def _fnv(b):
    h = 0xcbf29ce484222325
    for x in b:
        h = ((h ^ x) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return h


def test_hand_vocabulary_transform():
    """k = 2, L = 2, four descriptors: words 0, 1, 0, 2 with weights 1, 2, 1, 4.  TF_IDF: word 0 = 1 + 1 = 2, word 1 = 2, word 2 = 4; L1 norm 8"""
    voc, d = ref.hand_vocabulary(), ref.hand_descriptors()
    r = ref.transform(voc, d, 0)
    assert r["word_id"].tolist() == [0, 1, 0, 2]
    assert r["node_id"].tolist() == [3, 4, 3, 5]                   # levelsup 0: the word's own node (level 2)
    assert r["bow_word"].tolist() == [0, 1, 2] and r["bow_value"].tolist() == [0.25, 0.25, 0.5]
    assert r["fv_node"].tolist() == [3, 4, 5] and r["fv_start"].tolist() == [0, 2, 3, 4] and r["fv_index"].tolist() == [0, 2, 1, 3]
    r1 = ref.transform(voc, d, 1)
    assert r1["node_id"].tolist() == [1, 1, 1, 2]                  # level 1
    assert r1["fv_node"].tolist() == [1, 2] and r1["fv_start"].tolist() == [0, 3, 4] and r1["fv_index"].tolist() == [0, 1, 2, 3]
    for up in (2, 3):
        assert ref.transform(voc, d, up)["node_id"].tolist() == [0, 0, 0, 0]     # level <= 0: the root
    assert r1["bow_value"].tolist() == r["bow_value"].tolist() and r["n_short"] == 0


def test_hand_search_claim_chain():
    kf, fr = ref.chain_case()
    tr = []
    m, n = ref.search_by_bow(kf, fr, nnratio=0.7, check_orientation=False, trace=tr)
    assert m.tolist() == [0, -1, 1, -1, 2, -1] and n == 3
    assert [(t[1], t[3]) for t in tr] == [(3, 0), (13, 2), (21, 4)]       # distances 2+1, 12+1, 20+1 to frame features 0, 2, 4
    m2, n2 = ref.search_by_bow(kf, fr, nnratio=0.7, check_orientation=False, ignore_claims=True)
    assert m2.tolist() != m.tolist() and m2.tolist() == [2, -1, -1, -1, -1, -1]


def test_tfidf_case_sum_differs_from_product():
    voc, count = ref.tfidf_case()
    d = np.repeat(voc["desc"][:1], count, axis=0)                  # six features in word 0
    r = ref.transform(voc, d, 0)
    s = 0.0
    for _ in range(count):
        s += 0.1
    assert r["bow_word"].tolist() == [0]
    assert s != 0.1 * count and abs(s - 0.1 * count) < 2e-16       # the last bit
    assert r["bow_value"][0] == s / 1.0 and r["bow_value"][0] != 0.1 * count


@pytest.mark.parametrize("which", ["root", "leaf"])
def test_tie_case_has_equal_children(which):
    voc = ref.make_vocabulary(3, 3, 21, dup_root=which == "root", dup_leaf=which == "leaf")
    T = ref.tree(voc)
    if which == "root":
        kids = T[0][0]
        assert np.array_equal(voc["desc"][kids[0] - 1], voc["desc"][kids[1] - 1])
        assert ref.descend(voc, T, voc["desc"][kids[1] - 1], 2)[2:] == (kids[0], False, True)     # node at level 1: the first of the equal two
        return
    firsts = {c[0] for c in T[0] if c and T[1][c[0]]}; seconds = {c[1] for c in T[0] if c and T[1][c[0]]}
    for a, b in zip(sorted(firsts), sorted(seconds)):
        assert np.array_equal(voc["desc"][a - 1], voc["desc"][b - 1])
    rng = np.random.RandomState(4); hit = 0
    for _ in range(60):                                            # the two equal children are equally far from ANY query: when they are the
        word, w, nid, short, tie = ref.descend(voc, T, rng.randint(0, 256, 32).astype(np.uint8), 0)      # nearest, the first must win
        assert nid not in seconds
        hit += int(nid in firsts and tie)
    assert hit >= 10


def test_ratio_boundary_case_is_exact():
    kf, fr = ref.pair_at(28, 40)
    tr = []
    m, n = ref.search_by_bow(kf, fr, nnratio=0.7, check_orientation=False, trace=tr)
    assert tr[0][1:3] == (28, 40) and np.float32(28) == np.float32(0.7) * np.float32(40)     # (float)best == nnratio * (float)second
    assert n == 0
    m, n = ref.search_by_bow(*ref.pair_at(27, 40), nnratio=0.7, check_orientation=False)
    assert n == 1 and m[0] == 0


def test_threshold_tie_single_and_bin30_cases():
    assert ref.search_by_bow(*ref.pair_at(50, 200), check_orientation=False)[1] == 1
    assert ref.search_by_bow(*ref.pair_at(51, 200), check_orientation=False)[1] == 0
    tr = []
    m, n = ref.search_by_bow(*ref.pair_at(10, 10, n_extra=2), nnratio=1.5, check_orientation=False, trace=tr)
    assert tr[0][1:4] == (10, 10, 0) and n == 1 and m.tolist() == [0, -1, -1, -1]          # tie for best: the first in list order, second = the same distance
    tr = []
    m, n = ref.search_by_bow(*ref.pair_at(30, None), check_orientation=False, trace=tr)
    assert tr[0][1:3] == (30, 256) and n == 1                                            # a single candidate: second stays 256
    assert ref.rot_bin(359.0, 2.0) == 12 and ref.rot_bin(1.0, 2.0) == 12 and ref.rot_bin(0.0, 14.0) == 12
    assert ref.rot_bin(359.9, 0.0) == 12 and int(math.floor(float(np.float32(885.0) * (np.float32(1) / np.float32(30))) + 0.5)) == 30
    assert ref.rot_bin(890.0, 0.0) == 0                            # an angle difference that lands in bin 30 -> 0 (angles are not reduced by the matcher)


def test_bin30_case_is_decided_by_the_fold():
    kf, fr = ref.bin30_case()
    assert [ref.rot_bin(a, 0.0) for a in (0.0, 890.0, 60.0, 120.0, 180.0)] == [0, 0, 2, 4, 6] and ref.rot_bin(890.0, 0.0, fold30=False) == 30
    m, n = ref.search_by_bow(kf, fr)
    assert n == 16 and (m[:16] == np.arange(16)).all() and (m[16:] == -1).all()      # bins 0 (six of them), 2, 4 stay; bin 6 goes
    m2, n2 = ref.search_by_bow(kf, fr, fold30=False)
    assert (m2[:3] == -1).all() and (m2[16:] >= 0).all() and not np.array_equal(m, m2)   # without the fold bin 0 goes and bin 6 stays


def test_example_compiles():
    """examples/track_reference_kf.cpp, the only caller of hvo::ORBVocabulary / BowVectors / Frame::ComputeBoW / Frame::SearchByBoW, against the
    C++ mirror, as the other examples are checked (tests/test_cpp_adaptor.py); tests/test_bow_gpu.py links and runs it"""
    import subprocess
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I" + ROOT + "/include", "-fsyntax-only", ROOT + "/examples/track_reference_kf.cpp"])


def test_big_node_and_random_cases_reach_their_paths():
    kf, fr = ref.big_node_case()
    assert (fr["node_id"] == 4).sum() == 130 and (kf["node_id"] == 4).sum() == 70
    m, n = ref.search_by_bow(kf, fr, check_orientation=False)
    got = np.nonzero(m >= 0)[0]
    assert n >= 10 and got.min() < 64 and m[129] == 0            # claims in the first and in the third chunk of 64
    m2, _ = ref.search_by_bow(kf, fr, check_orientation=False, ignore_claims=True)
    assert not np.array_equal(m, m2)
    kf, fr = ref.random_pair(100, 100, 1)
    a, na = ref.search_by_bow(kf, fr, check_orientation=True); b, nb = ref.search_by_bow(kf, fr, check_orientation=False)
    assert 0 < na < nb                                             # the rotation filter removes some


def test_unbalanced_and_stopped_generators():
    voc = ref.make_vocabulary(3, 3, 5, leaf_at_level1=True)
    T = ref.tree(voc)
    assert T[1][1] and T[3][1] == 1                               # node 1 is a word at level 1
    word, w, nid, short, _ = ref.descend(voc, T, voc["desc"][0], 1)     # nid level 2, leaf at level 1
    assert short and nid == 1 and word == 0
    assert not ref.descend(voc, T, voc["desc"][0], 2)[3]          # nid level 1: reached
    voc = ref.make_vocabulary(3, 2, 6, zero_weight_every=2)
    d = voc["desc"][voc["is_leaf"] == 1]
    r = ref.transform(voc, d, 0)
    assert (r["word_id"] == -1).sum() >= 3 and np.array_equal(r["word_id"] == -1, r["node_id"] == -1)
    assert 0 not in r["bow_word"] and len(r["fv_index"]) == (r["word_id"] >= 0).sum()


def test_distinct_word_generator_gives_one_word_per_feature():
    voc = ref.make_vocabulary(3, 3, 17)
    d = ref.distinct_word_descriptors(voc)
    r = ref.transform(voc, d, 1)
    assert len(d) >= 20 and len(r["bow_word"]) == len(d) and sorted(r["word_id"].tolist()) == r["bow_word"].tolist()
    assert r["word_id"].tolist() != sorted(r["word_id"].tolist())       # not already in word order


def test_text_loader_validation_and_binding(hvo, tmp_path):
    """fails on a tree without the feature: the binding has Vocabulary, the five calls, and EXPORTS names the C functions.  The loader and the
    validation run on a host-only vocabulary (device -1): no device is needed."""
    for name in ("hvo_vocabulary_create", "hvo_vocabulary_load_text", "hvo_vocabulary_destroy", "hvo_vocabulary_info", "hvo_compute_bow",
                 "hvo_stream_compute_bow", "hvo_batch_compute_bow", "hvo_search_by_bow", "hvo_stream_search_by_bow"):
        assert name in hvo.EXPORTS
    assert all(hasattr(hvo.Context, m) for m in ("compute_bow", "batch_compute_bow", "search_by_bow"))
    assert all(hasattr(hvo.Stream, m) for m in ("compute_bow", "search_by_bow"))
    hdr = open(ROOT + "/include/hvo.h").read()
    assert re.search(r"#define HVO_ABI_VERSION\s+3\b", hdr)
    voc = ref.make_vocabulary(4, 3, 11, scoring=ref.L2_NORM, weighting=ref.IDF)
    p = tmp_path / "voc.txt"
    ref.write_text(voc, str(p))
    with open(p, "a") as f:
        f.write("\n")                                               # a trailing empty line is not a node
    v = hvo.Vocabulary.load_text(str(p), device=-1)
    assert v.info() == dict(k=4, L=3, n_nodes=4 + 16 + 64 + 1, n_words=64, scoring=ref.L2_NORM, weighting=ref.IDF, device=-1)
    v.close()
    mk = lambda voc, **kw: hvo.Vocabulary(voc["k"], voc["L"], voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"], voc["scoring"], voc["weighting"], device=-1, **kw)
    assert mk(ref.empty_vocabulary()).info()["n_words"] == 0       # no words: legal
    assert mk(ref.make_vocabulary(3, 3, 5, leaf_at_level1=True)).info()["n_words"] == 1 + 2 * 9
    def refused(voc):
        with pytest.raises(hvo.HvoError) as e:
            mk(voc)
        return e.value.status
    bad = ref.make_vocabulary(2, 2, 1); bad["parent"][2] = 3       # a parent id >= its child's id (row 2 is node 3)
    assert refused(bad) == -1
    bad = ref.make_vocabulary(2, 2, 1); bad["parent"][3] = 5
    assert refused(bad) == -1
    bad = ref.make_vocabulary(2, 2, 1); bad["is_leaf"][-1] = 0     # a non-leaf without children
    assert refused(bad) == -1
    bad = ref.make_vocabulary(2, 2, 1); bad["parent"][-1] = 1      # node 1 gets a third child with k = 2
    assert refused(bad) == -1
    for k, L in ((1, 2), (21, 2), (3, 0), (3, 11)):
        bad = ref.make_vocabulary(2, 2, 1); bad["k"], bad["L"] = k, L
        assert refused(bad) == -1
    junk = tmp_path / "junk.txt"; junk.write_text("10 6 0 0\n0 0 1 2 3\n")
    with pytest.raises(hvo.HvoError):
        hvo.Vocabulary.load_text(str(junk), device=-1)
    with pytest.raises(hvo.HvoError):
        hvo.Vocabulary.load_text(str(tmp_path / "missing.txt"), device=-1)


def test_host_restatement_tool_agrees_with_the_reference_restatement(tmp_path):
    """tools/bow_host.cpp (the host path tools/bow_timing.py times) gives the same BowVector and the same match vector as bow_ref on one case"""
    import subprocess
    exe = str(tmp_path / "bow_host")
    subprocess.check_call(["g++", "-O1", "-std=c++14", ROOT + "/tools/bow_host.cpp", "-o", exe])
    voc = ref.make_vocabulary(4, 3, 8)
    kf, fr = ref.random_pair(150, 160, 6, n_nodes=1)
    kf["node_id"] = ref.transform(voc, kf["desc"], 1)["node_id"]; t = ref.transform(voc, fr["desc"], 1); fr["node_id"] = t["node_id"]
    m, nm = ref.search_by_bow(kf, fr)
    with open(tmp_path / "case.bin", "wb") as f:
        np.array([4, 3, voc["scoring"], voc["weighting"], len(voc["parent"]), 1, 160, 150, 1], np.int32).tofile(f)
        for a in (voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"], fr["desc"], kf["desc"], kf["has_map_point"], kf["angle"], fr["angle"]):
            np.ascontiguousarray(a).tofile(f)
    out = subprocess.check_output([exe, str(tmp_path / "case.bin")]).split()
    assert int(out[2]) == len(t["bow_word"]) and int(out[3]) == nm and nm > 5
    # the match vector and the BowVector themselves, not only their sizes: FNV-1a over match (int32), the words (int32) and the values' bits
    assert int(out[4], 16) == _fnv(m.astype(np.int32).tobytes())
    assert int(out[5], 16) == _fnv(t["bow_word"].astype(np.int32).tobytes() + t["bow_value"].tobytes())
