"""The local-map line search, LSDmatcher::SearchByProjection(F, vpMapLines, eval_orient, th) (reference src/LSDmatcher.cpp:709-801): the
C ABI declares and exports it, the C++ mirror's example compiles, and the CPU restatement (tests/local_map_lines_ref.py) gives the known
answers of hand-built scenes for every detail that decides bits.  No GPU here: tests/line_search_cases.py holds the scenes (Scene, desc_bits)
and states each of them again as a named case, which tests/test_line_search_edges_gpu.py runs on the device."""
import ctypes
import os
import re
import subprocess

import numpy as np

from conftest import ROOT, PKG_DIR
import local_map_lines_ref as ref
from line_search_cases import Scene, desc_bits

NAMES = ("hvo_search_lines_by_projection_map", "hvo_stream_search_lines_by_projection_map")


def test_header_library_and_binding_carry_the_call(hvo):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hvo.h")).read(), flags=re.S)
    lib = ctypes.CDLL(os.path.join(PKG_DIR, "csrc", "libhvo.so"))
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert hasattr(lib, n), n
        assert n in hvo.EXPORTS, n
    assert hasattr(hvo.Context, "search_lines_by_projection_map") and hasattr(hvo.Stream, "search_lines_by_projection_map")


def test_example_compiles():
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           "-fsyntax-only", os.path.join(ROOT, "examples", "local_map_lines.cpp")])


def test_window_uses_the_0998_direction_gate(hvo):
    # a line 5 degrees off the query's direction: inside the Cur/Last call's 0.96, outside GetFeaturesInAreaForLine's default 0.998
    s = Scene(hvo, [100.0])
    s.kl["ey"] = np.float32(100.0 + 100.0 * np.tan(np.radians(5.0)))
    assert s.run(100.0)[0] == 0
    s.kl["ey"] = np.float32(100.0 + 100.0 * np.tan(np.radians(3.0)))            # cos 3 degrees = 0.99863 passes
    assert s.run(100.0)[0] == 1


def test_nan_gate_passes(hvo):
    s = Scene(hvo, [100.0])
    s.l3d["A"][:] = 0.0                                                      # no fitted 3-D line: 0 / 0
    n, mi, md = s.run(100.0)
    assert n == 1 and mi[0] == 0 and md[0] == 0
    s = Scene(hvo, [100.0])
    n, mi, _ = s.run(100.0, wvec=(0.0, 0.0, 0.0))                            # zero world vector
    assert n == 1 and mi[0] == 0


def test_3d_gate_14_passes_16_fails(hvo):
    s = Scene(hvo, [100.0])
    for deg, want in ((14.0, 1), (16.0, 0), (170.0, 1), (90.0, 0)):   # (|cos| : the opposite direction passes)
        a = np.radians(deg)
        n, mi, _ = s.run(100.0, wvec=(np.cos(a), np.sin(a), 0.0))
        assert n == want and mi[0] == (0 if want else -1), deg
    # the frame's direction is compared in the CAMERA frame with the WORLD vector, as the reference does: a tilt out of the image plane counts too
    a = np.radians(20.0)
    assert s.run(100.0, wvec=(np.cos(a), 0.0, np.sin(a)))[0] == 0


def test_radius_at_0998f_and_the_float_below(hvo):
    s = Scene(hvo, [106.5])                                                  # 6.5 pixels from the query: inside 8, outside 5
    v = np.float32(0.998)
    below = np.nextafter(v, np.float32(0.0))
    assert float(v) > 0.998 and float(below) < 0.998
    assert ref.radius_by_viewing_cos(v, 1.0) == 5.0 and ref.radius_by_viewing_cos(below, 1.0) == 8.0
    assert s.run(100.0, view_cos=v)[0] == 0
    assert s.run(100.0, view_cos=below)[0] == 1


def test_th_1_and_5(hvo):
    s = Scene(hvo, [120.0])                                                  # 20 pixels away
    assert ref.radius_by_viewing_cos(1.0, 5.0) == 25.0 and ref.radius_by_viewing_cos(0.5, 5.0) == 40.0
    assert s.run(100.0, th=1.0)[0] == 0
    n, mi, _ = s.run(100.0, th=5.0)
    assert n == 1 and mi[0] == 0


def test_best_distance_95_and_96(hvo):
    for k, want in ((95, 1), (96, 0)):
        s = Scene(hvo, [100.0], descs=[desc_bits(k)])
        n, mi, md = s.run(100.0)
        assert n == want and md[0] == (95 if want else 256), k


def test_ratio_rule_same_and_different_octaves(hvo):
    # best 50, second 52: 50 > 0.95 * 52 = 49.4 -> rejected in the same octave, accepted across octaves
    for octs, want in (([0, 0], 0), ([0, 1], 1), ([2, 2], 0)):
        s = Scene(hvo, [100.0, 101.0], octaves=octs, descs=[desc_bits(50), desc_bits(52)])
        assert s.run(100.0)[0] == want, octs
    # best 50, second 60: 50 > 57 is false -> accepted even in the same octave
    s = Scene(hvo, [100.0, 101.0], descs=[desc_bits(50), desc_bits(60)])
    n, mi, md = s.run(100.0)
    assert n == 1 and mi[0] == 0 and md[0] == 50
    # one candidate: bestLevel2 stays -1, no ratio test
    s = Scene(hvo, [100.0], descs=[desc_bits(50)])
    assert s.run(100.0)[0] == 1
    # ties go to the earlier visit, and the later tie is the second: 40 > 0.95 * 40 -> rejected in the same octave
    s = Scene(hvo, [100.0, 101.0], descs=[desc_bits(40), desc_bits(40, 100)])
    assert s.run(100.0)[0] == 0
    s = Scene(hvo, [100.0, 101.0], octaves=[1, 0], descs=[desc_bits(40), desc_bits(40, 100)])
    n, mi, _ = s.run(100.0)
    assert n == 1 and mi[0] == 0


def test_claims_block_or_get_overwritten(hvo):
    s = Scene(hvo, [100.0])
    # two map lines after the same current line: with observations the first one's claim blocks the second ...
    n, mi, _ = s.run([100.0, 100.0], blocks=np.array([1, 0], np.uint8))
    assert n == 1 and list(mi) == [0, -1]
    # ... without, the second overwrites it (both acceptances are counted, the caller's assignment in query order keeps the second)
    n, mi, _ = s.run([100.0, 100.0], blocks=np.array([0, 1], np.uint8))
    assert n == 2 and list(mi) == [0, 0]
    n, mi, _ = s.run([100.0, 100.0, 100.0], blocks=np.array([0, 1, 1], np.uint8))
    assert n == 2 and list(mi) == [0, 0, -1]
    # a line that held an observed map line before the call is passed over; the next candidate wins
    s = Scene(hvo, [100.0, 102.0], octaves=[0, 1], descs=[desc_bits(10), desc_bits(20)])
    n, mi, md = s.run(100.0, occ=np.array([1, 0], np.uint8))
    assert n == 1 and mi[0] == 1 and md[0] == 20
    # a claimed best leaves the next query the remaining line
    n, mi, md = s.run([100.0, 100.0], blocks=np.array([1, 1], np.uint8))
    assert n == 2 and list(mi) == [0, 1] and list(md) == [10, 20]
