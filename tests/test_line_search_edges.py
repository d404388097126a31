"""The hand-built cases of tests/line_search_cases.py on the CPU: every case through the restatement of the local-map line search
(tests/local_map_lines_ref.py) or the oracle (oracle/match.c: the frame-to-frame search and SearchByGeomNApearance), checked against the
expectation the case states by hand FIRST -- so that reference and kernel cannot be wrong together when tests/test_line_search_edges_gpu.py
compares them -- and the path properties the cases are built for, counted by the cases' own model: the fallback of k_lsbp_map_epilogue
taken and not taken, the ratio rule passing and rejecting inside it, ties decided by the visit position against the index order, claims in
the last occupancy word.  No GPU."""
import numpy as np
import pytest

import line_map_ref as lmr
import line_search_cases as lc
import local_map_lines_ref as ref


@pytest.fixture(scope="module")
def cases(hvo):
    return lc.build_all(hvo)                                      # the builders assert their own path properties


def reference(orc, c, mode):
    if mode == "map": return ref.search_lines_by_projection_map(*lc.args_map(c))
    if mode == "last": return orc.search_lines_by_projection(*lc.args_last(c))
    a = lc.args_geom(c)
    return orc.lines_geom_match(*a[:5], desc_th=a[5], last_has_mapline=a[6])


@pytest.fixture(scope="module")
def references(orc, cases):
    """every case through its reference, once, checked against what the case states by hand"""
    out = {}
    for name, c in cases.items():
        for mode, (en, e1, e2) in c.expect.items():
            n, a1, a2 = reference(orc, c, mode)
            assert np.array_equal(a1, e1), (name, mode, np.flatnonzero(a1 != e1)[:8], a1[:16], e1[:16])
            assert np.array_equal(a2, e2) and n == en, (name, mode, n, en)
            out[name, mode] = (n, a1, a2)
    return out


CASES, CHAINS, LOCAL = lc.CASES, lc.CHAINS, lc.LOCAL


def test_case_list_is_complete(cases):
    assert sorted(CASES) == sorted(cases)
    assert sorted(LOCAL) == sorted(n for n, c in cases.items() if c.local is not None)


def test_every_case_holds_on_its_reference(cases, references):
    assert {m for (_, m) in references} == {"map", "last", "geom"}
    for name in CASES:
        assert any(k[0] == name for k in references), name


def test_the_models_agree_with_the_references(cases, references):
    for name, c in cases.items():
        if c.map is not None and len(c.map.q) <= 200:
            n, idx, dist, _ = lc.model_map(c)
            assert n == references[name, "map"][0] and np.array_equal(idx, references[name, "map"][1]) and np.array_equal(dist, references[name, "map"][2]), name
        if "last" in c.expect and len(c.last.q) <= 200:
            n, idx, dist, _ = lc.model_last(c)
            assert n == references[name, "last"][0] and np.array_equal(idx, references[name, "last"][1]) and np.array_equal(dist, references[name, "last"][2]), name


def test_path_properties(cases, references):
    st = {n: lc.model_map(cases[n])[3] for n in CHAINS}
    # the fallback: taken for at least three queries and not taken for at least three, in every blocking chain
    for n in ("chain_all1", "chain_exhaust", "chain_alt", "chain_all1_occupied", "chain_alt_occupied"):
        assert st[n].fallback.sum() >= 3 and (~st[n].fallback).sum() >= 3, n
        assert np.all(st[n].nfree[st[n].fallback] < 2) and np.all(st[n].ncand > lc.TOPK)
    assert not st["chain_all0"].fallback.any()
    # inside it the ratio rule passes on the octaves alone (read from the key lines there) and rejects
    for n in ("chain_all1", "chain_all1_occupied"):
        assert "pass" in st[n].inside and "reject" in st[n].inside and "accept" in st[n].inside, n
        i = st[n].inside.index("pass"); idx = references[n, "map"][1]
        assert idx[i] == 7 and np.all(idx[i + 1:] == -1)
    # a chain that ends with every candidate claimed: the queries after that get -1 / 256 out of the fallback
    n, idx, dist = references["chain_exhaust", "map"]
    assert n == 12 and sorted(idx[:12].tolist()) == list(range(12)) and np.all(idx[12:] == -1) and np.all(dist[12:] == 256) and st["chain_exhaust"].fallback[12:].all()
    assert dist[11] == 95
    # candidate counts; the four smallest keys in one lane, in four lanes of one chunk, across chunks; five candidates are enough for the fallback
    for place, best in lc.PLACE.items():
        for cnt in lc.COUNTS:
            c = cases["count_%d_%s" % (cnt, place)]; s = lc.model_map(c)[3]
            assert np.all(s.ncand == cnt) and sorted(s.top[0].tolist()) == sorted(best)
            assert s.top[0].tolist() == sorted(best, reverse=True)                       # ties: the visit order, which is the reverse of the index order
            assert s.fallback.tolist() == [False] * 3 + [cnt > lc.TOPK] * 3
            lanes = [b % 64 for b in s.top[0]]; chunks = [b // 64 for b in s.top[0]]
            assert (len(set(lanes)), len(set(chunks))) == {"lane": (1, 4), "chunk": (4, 1), "across": (2, 3)}[place]
    assert references["count_5_lane", "map"][0] == 5 and references["count_4_lane", "map"][0] == 4
    for n, cnt in (("count_0", 0), ("count_1", 1), ("count_2", 2)):
        assert np.all(lc.model_map(cases[n])[3].ncand == cnt) and references[n, "map"][0] == cnt
    # ties that the visit position decides against the index order
    for n in ("visit_tie_later_index_first", "visit_passes_from_middle", "visit_passes_at_end_only", "visit_three_cells", "visit_twice_in_a_cell"):
        for mode in ("map", "last"):
            idx, dist = references[n, mode][1:]
            assert idx[0] == 1 and idx[1] == 0 and dist[0] == dist[1], (n, mode)
    # claims in the last occupancy word (lines 2016 .. 2047, bit 31 first), and t_occupied on the last line of a count that is no multiple of 32
    idx = references["nt_2048_last_word", "map"][1]
    assert idx[0] == 2047 and set(idx[:32].tolist()) == set(range(2016, 2048)) and np.all(idx[32:] == -1)
    for nt in (63, 64, 65, 2048):
        for mode in ("map", "last"):
            assert references["nt_%d_last" % nt, mode][1][0] == nt - 1 and references["nt_%d_last_occupied" % nt, mode][0] == 0
    # every `continue` of the window walk
    q = cases["window_off_each_edge"].map.q
    assert sorted(lc.window_cells(lc.B0, q_[0], q_[1], 8.0) for q_ in q[:4]) == [1, 2, 3, 4]


def test_local_form_restatement_reaches_the_same_paths(cases):
    """the resident map of lc.local_map() over the crafted frames: the frustum pass keeps every crafted slot, and its queries drive the search
    core into the fallback as well"""
    for name in LOCAL:
        c = cases[name]; t = c.t
        M, T, held = lc.local_map(c)
        fp = lmr.frustum_pass(M, lmr.CAM, T, lmr.BOUNDS, lmr.LOG_SF, held)
        assert len(fp["slots"]) == c.local.nslots and int(fp["t_occupied"].sum()) == len(c.local.occ), name
        q = lmr.queries(M, fp)
        n, idx, dist, st = lc.model_map_arrays(q[0], q[1], q[2], q[3], q[4], t.kl, t.fn, t.l3d, t.desc, fp["t_occupied"], c.cs, c.ci, lmr.BOUNDS, c.local.th, 0.95)
        o = lmr.search_local_lines(M, lmr.CAM, T, lmr.BOUNDS, lmr.LOG_SF, c.local.th, 0.95, t.kl, t.fn, t.l3d, t.desc, c.cs, c.ci, held)
        assert o["n_matches"] == n and np.array_equal(o["match_idx"], idx) and np.array_equal(o["match_dist"], dist), name
        assert n >= 3 and np.all(st.ncand > lc.TOPK), name
        if c.map.blocks.any(): assert st.fallback.sum() >= 3, name
