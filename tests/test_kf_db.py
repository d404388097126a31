"""The key-frame database (csrc/kf_db.hip) on the CPU: the boundary it adds is declared, exported and bound; the crafted cases of
tests/kf_db_ref.py reach the paths they are meant for (tests/test_kf_db_gpu.py runs the same scripts on the device); the example compiles;
the host program tools/kf_db_timing.py times gives the restatement's candidate lists."""
import ctypes
import os
import re
import subprocess

import numpy as np

import kf_db_ref as ref
from conftest import ROOT, PKG_DIR

NAMES = ("hvo_keyframe_db_create", "hvo_keyframe_db_destroy", "hvo_keyframe_db_last_error", "hvo_keyframe_db_add", "hvo_stream_keyframe_db_add",
         "hvo_keyframe_db_erase", "hvo_keyframe_db_clear", "hvo_keyframe_db_set_covisible", "hvo_keyframe_db_get", "hvo_keyframe_db_info",
         "hvo_keyframe_db_query", "hvo_stream_keyframe_db_query", "hvo_batch_keyframe_db_query", "hvo_keyframe_db_last_kernel_ms")


def test_boundary_is_declared_exported_and_bound(hvo):
    """fails on a tree without the feature"""
    hdr = open(os.path.join(ROOT, "include", "hvo.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = ctypes.CDLL(os.path.join(PKG_DIR, "csrc", "libhvo.so"))
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert hasattr(lib, n), n
        assert n in hvo.EXPORTS, n
    for m in ("add", "erase", "clear", "set_covisible", "setCovisible", "get", "info", "query", "DetectRelocalizationCandidates", "DetectLoopCandidates", "last_kernel_ms"):
        assert callable(getattr(hvo.KeyFrameDatabase, m)), m
    assert callable(hvo.Context.keyframe_db_query) and callable(hvo.Context.batch_keyframe_db_query)
    assert callable(hvo.Stream.keyframe_db_query) and callable(hvo.Stream.keyframe_db_add)
    assert ctypes.sizeof(hvo.KfdbParams) == 24 and ctypes.sizeof(hvo.KfdbResult) == 80 and ctypes.sizeof(hvo.KeyframeDbDesc) == 40
    assert (hvo.KFDB_RELOC, hvo.KFDB_LOOP, hvo.KFDB_MAX_SLOTS, hvo.KFDB_MAX_COVISIBLE) == (ref.RELOC, ref.LOOP, 16384, 10)
    assert lib.hvo_keyframe_db_create(None, None) == -1            # refused before any device is touched


def run(name):
    return ref.run_script(ref.Database(ref.N_CRAFT_WORDS), ref.CRAFTED[name]())


def test_score_functions_on_hand_values():
    w1, v1, w2, v2 = [1, 3, 5, 9], [0.5, 0.25, 0.125, 0.125], [0, 3, 4, 5, 7], [0.25, 0.25, 0.25, 0.125, 0.125]
    assert ref.score(ref.L1_NORM, w1, v1, w2, v2) == 0.375          # min(0.25, 0.25) + min(0.125, 0.125)
    assert ref.score(ref.DOT_PRODUCT, w1, v1, w2, v2) == 0.25 * 0.25 + 0.125 * 0.125
    assert ref.score(ref.L2_NORM, w1, v1, w2, v2) == 1.0 - (1.0 - 0.078125) ** 0.5
    assert ref.score(ref.L2_NORM, [1], [2.0], [1], [1.0]) == 1.0    # the >= 1 clamp
    assert ref.score(ref.CHI_SQUARE, w1, v1, w2, v2) == 2. * (0.0625 / 0.5 + 0.015625 / 0.25)
    assert ref.score(ref.CHI_SQUARE, [1], [0.0], [1], [0.0]) == 0.0  # the vi + wi != 0 guard: no 0 / 0
    assert ref.score(ref.BHATTACHARYYA, w1, v1, w2, v2) == 0.25 + 0.125
    assert ref.score(ref.L1_NORM, [1, 2], [0.5, 0.5], [3], [1.0]) == 0.0 and ref.score(ref.L1_NORM, [], [], [3], [1.0]) == 0.0


def test_best_differs_and_entries_collapse():
    r, = run("best_differs")
    assert r["discovery"] == [1, 0, 2] and r["n_scored"] == 3
    assert r["best"].tolist() == [0, 0, 2]                          # slot 1's entry names slot 0: pBestKF != pKFi
    assert r["acc"][0] == r["acc"][1] == np.float32(0.9375) and (r["acc"] > np.float32(0.75) * r["best_acc_score"]).all()
    assert r["candidates"].tolist() == [0, 2]                       # three entries above the threshold, two candidates


def test_discovery_order_is_not_slot_order():
    first, second = run("discovery_order")
    assert first["candidates"].tolist() == [9, 5, 2] and first["discovery"] == [9, 5, 2]
    assert second["candidates"].tolist() == [9, 2, 5]                # slot 5 erased and added again: behind slot 2 on their first common word
    assert sorted(first["candidates"]) != first["candidates"].tolist() and sorted(second["candidates"]) != second["candidates"].tolist()


def test_min_common_boundary():
    r, = run("min_common_boundary")
    assert (r["max_common"], r["min_common"], r["n_sharing"], r["n_scored"]) == (10, 8, 3, 2)
    assert r["words"].tolist() == [10, 9, 8]
    assert not np.isnan(r["score"][1]) and np.isnan(r["score"][2])  # 9 > 8 is scored, 8 > 8 is not
    assert int(np.float32(5) * np.float32(0.8)) == 4 and int(np.float32(15) * np.float32(0.8)) == 12     # the float product, truncated


def test_stale_score_changes_the_candidates():
    q1, q2 = run("stale_with")
    only, = run("stale_without")
    assert q1["candidates"].tolist() == [1] and q1["score"][1] == np.float32(0.875)
    for r in (q2, only):
        assert r["words"].tolist() == [10, 1, 10] and np.isnan(r["score"][1]) and r["n_scored"] == 2      # slot 1: in the query, not scored
    assert q2["acc"][0] == np.float32(0.3125 + 0.875) and q2["best"][0] == 1 and q2["candidates"].tolist() == [1]
    assert only["acc"][0] == np.float32(0.3125) and only["best"][0] == 0 and only["candidates"].tolist() == [0, 2]


def test_loop_connected_and_min_score():
    with_c, = run("loop_connected")
    without, = run("loop_unconnected")
    high, = run("loop_high_min_score")
    assert without["candidates"].tolist() == [0]                    # the connected key frame would win ...
    assert with_c["candidates"].tolist() == [1] and with_c["words"][0] == 0 and np.isnan(with_c["score"][0])    # ... and is not even discovered
    assert with_c["n_scored"] == 3 and with_c["score"][3] == np.float32(0.25) and np.isnan(with_c["acc"][3])     # scored, below min_score: no entry
    assert with_c["acc"][1] == np.float32(0.75)                     # ... but a neighbour: 0.5 + 0.25, and not the connected slot 0's 1.0
    assert with_c["best_acc_score"] == np.float32(0.75)
    assert high["candidates"].tolist() == [] and high["n_scored"] == 3 and high["best_acc_score"] == np.float32(0.9)   # bestAccScore starts at minScore
    db = ref.Database(ref.N_CRAFT_WORDS); ref.run_script(db, ref.CRAFTED["loop_high_min_score"]())
    assert db.kept(3).tolist() == [0.0, 0.25]                       # mLoopScore is written either way


def test_075_is_strict():
    r, = run("strict_075")
    assert r["acc"].tolist() == [1.0, 0.75, np.float32(0.75 + 2.0 ** -20)] and r["best_acc_score"] == 1.0
    assert r["candidates"].tolist() == [0, 2]


def test_random_scripts_reach_their_paths():
    """the random databases of the GPU file: several slots pass the min-common test, neighbours add up, entries collapse, some slots are dropped by
    the 0.75 threshold, and in the loop form min_score removes scored slots"""
    s = ref.random_script(11, 125, list(range(0, 600, 2)), [1, 63, 64, 65, 125], n_queries=3, holes=20)
    rs = ref.run_script(ref.Database(125), s)
    assert any(r["n_scored"] > 3 for r in rs) and any(len(r["candidates"]) >= 2 for r in rs)
    assert any((r["best"][r["best"] >= 0] != np.nonzero(r["best"] >= 0)[0]).any() for r in rs)
    assert any((~np.isnan(r["acc"])).sum() > len(r["candidates"]) for r in rs)
    s = ref.random_script(12, 125, list(range(65)), [64, 65, 125], n_queries=3, mode=ref.LOOP)
    rs = ref.run_script(ref.Database(125), s)
    assert any((~np.isnan(r["score"])).sum() > (~np.isnan(r["acc"])).sum() > 0 for r in rs)


def test_example_compiles():
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I" + ROOT + "/include", "-fsyntax-only", ROOT + "/examples/keyframe_db.cpp"])


def test_example_links(tmp_path):
    csrc = os.path.join(PKG_DIR, "csrc")
    subprocess.check_call(["g++", "-std=c++14", "-O1", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "keyframe_db.cpp"),
                           "-L" + csrc, "-lhvo", "-Wl,-rpath," + csrc, "-o", str(tmp_path / "keyframe_db")])


def test_host_tool_agrees_with_the_restatement(tmp_path):
    """tools/kf_db_host.cpp (the host path tools/kf_db_timing.py times: an inverted file of std::list) returns the restatement's candidate lists"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import kf_db_timing as tm
    finally:
        sys.path.pop(0)
    exe = str(tmp_path / "kf_db_host")
    subprocess.check_call(["g++", "-O1", "-std=c++14", ROOT + "/tools/kf_db_host.cpp", "-o", exe])
    for mode, seed in ((ref.RELOC, 5), (ref.LOOP, 6)):
        script = ref.random_script(seed, 1000, list(range(120)), [200, 150], n_queries=3, mode=mode, query_size=300)
        want = ref.run_script(ref.Database(1000), script)
        path = str(tmp_path / ("case%d.bin" % mode))
        tm.write_case(path, 1000, ref.L1_NORM, script)
        out = subprocess.check_output([exe, path, "1"]).decode().splitlines()
        got = [[int(x) for x in ln.split()[2:]] for ln in out if ln.startswith("candidates ")]
        assert got == [r["candidates"].tolist() for r in want] and any(len(g) for g in got)
