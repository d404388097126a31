"""CPU tests of the line-structure restatement (tests/line_opt_ref.py) by known answers worked by hand, its behaviour on generated scenes,
and the presence of the new entry points in the header, the library and the binding."""
import ctypes
import math
import os
import re

import numpy as np

import line_opt_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
X, Y, Z = np.eye(3)


def test_thresholds_and_constants():
    p = ref.default_params()
    assert p["cos_par"] == math.cos(3 * 0.0174533) and abs(p["cos_par"] - 0.998629) < 1e-6            # 3 degrees with the reference's 0.0174533
    assert p["cos_perp"] == math.cos(87.0 * 0.0174533) and abs(p["cos_perp"] - 0.052336) < 1e-6
    # const float thHuberLine = sqrt(0.02): the double square root rounded to float, one ulp above the float square root of 0.02f
    assert p["huber_delta"] == float(np.float32(math.sqrt(0.02))) == 0.1414213627576828 != float(np.sqrt(np.float32(0.02)))
    assert p["chi2_round"] == (np.float32(0.02), np.float32(0.01)) and p["chi2_reject"] == 0.02


def _dir2(deg):
    return np.array([math.cos(math.radians(deg)), math.sin(math.radians(deg)), 0.0])


def test_pairs_parallel_perpendicular_and_the_band_between():
    # line functions (a, b, c): the 2-D vector is (a / c, b / c)
    fn = np.array([[1, 0, 1], [2, 0, 1], [0, 3, 1], _dir2(2.9) * 2, _dir2(3.1), _dir2(87.1), [1, 0, 1]], np.float64)
    fn[3:6, 2] = 1.0
    eq = np.array([X, X, Y, _dir2(2.9), _dir2(3.1), _dir2(87.1), Z], np.float32)
    rel = ref.struct_constraints(fn, eq)
    assert rel[0].tolist() == [0, 1, 2, 1, 0, 2, 0]       # 2.9 degrees parallel, 3.1 neither, 87.1 perpendicular; line 6: parallel in 2-D, perpendicular in 3-D
    assert rel[2].tolist() == [2, 2, 0, 2, 0, 1, 2]       # Y: 87.1 degrees from line 3 (perpendicular), 86.9 from line 4 (neither), 2.9 from line 5; line 6: perpendicular both ways
    assert np.array_equal(rel, rel.T)                     # the arithmetic is symmetric; only the row rule is not
    assert ref.lists_of(rel[0]) == ([1, 3], [2, 5])


def test_invalid_partner_enters_a_list_and_rows_follow_the_rule():
    s = 1 / math.sqrt(3)
    fn = np.array([[1, 1, 1], [1, 1, 2], [3, 3, 1], [1, 1, 0], [1, 1, 1]], np.float64)
    eq = np.array([[s, s, s], [-1, -1, -1], [s, s, s], [s, s, s], [s, s, 0]], np.float32)
    eq[4] = np.float32([1 / math.sqrt(2), 1 / math.sqrt(2), 0])
    rel = ref.struct_constraints(fn, eq)
    # line 1 was never fitted: its row is skipped, but as a partner its (-1,-1,-1) is parallel to (s,s,s): |cos| = 1
    assert rel[1].tolist() == [0, 0, 0, 0, 0] and rel[0, 1] == 1 and rel[2, 1] == 1
    # line 3: c == 0 gives inf / inf = NaN, every comparison false: in no list and with no list
    assert not rel[3].any() and not rel[:, 3].any()
    # line 4 (a direction in the image plane) keeps its row under the active rule and loses it under GrabImageRGBD's
    assert rel[0, 4] == 0                                  # cos = 0.816: neither
    eq2 = eq.copy(); eq2[4] = np.float32([1, 0, 0]); eq2[0] = np.float32([1, 0, 0]); eq2[2] = np.float32([1, 0, 0])
    r0 = ref.struct_constraints(fn, eq2); r1 = ref.struct_constraints(fn, eq2, ref.default_params(row_rule=1))
    assert r0[4].tolist() == [1, 0, 1, 0, 0] and r1[4].tolist() == [0, 0, 0, 0, 0]
    assert r1[0].tolist() == [0, 0, 0, 0, 0] and r1[1].tolist() == r0[1].tolist() == [0] * 5     # z == 0 skips rows 0, 2, 4; (-1,-1,-1) has z != 0 ...
    # ... so under GrabImageRGBD's rule the unfitted line 1 is NOT skipped: (-1,-1,-1) against (1,0,0) is 0.577, neither
    # part 2 gives the invalid partner no edge: line 0 with five entries, two of them to line 1-like partners
    S = ref.crafted([X, X, X, X, X, X], [(0, i, 1) for i in range(1, 6)])
    S["line_eq"][1] = -1.0; S["line_eq"][3, 2] = 0.0
    R = ref.run_scene(S)
    assert R.n_lines_to_opt == 1 and R.n_edges == 3 and R.n_par_edges == 3     # partner 1 is (-1,-1,-1), partner 3 has z == 0: both dropped; 2, 4, 5 stay


def test_fewer_than_five_counts_dropped_partners():
    S = ref.crafted([X] * 6, [(0, i, 1) for i in range(1, 6)] + [(1, i, 1) for i in (0, 2, 3, 4)])
    for i in (2, 3, 4): S["line_eq"][i] = -1.0
    R = ref.run_scene(S)
    # line 0: five entries, three to dropped partners: it enters with two edges.  line 1: four entries: it does not
    assert R.n_lines_to_opt == 1 and R.n_edges == 2 and R.graph.entered.tolist() == [True] + [False] * 5
    # a slot that already holds -1 counts for the size and gives no edge
    S["rel"][0, 5] = -1
    R = ref.run_scene(S)
    assert R.n_lines_to_opt == 1 and R.n_edges == 1 and R.rel[0, 5] == -1
    # the end-point conditions: z == 0, x == -1, |dx| and |dy| below 1e-5
    for edit in (lambda A, B: A.__setitem__((0, 2), 0.0), lambda A, B: B.__setitem__((0, 0), -1.0),
                 lambda A, B: (B.__setitem__((0, 0), A[0, 0] + 5e-6), B.__setitem__((0, 1), A[0, 1]))):
        T = ref.crafted([X] * 6, [(0, i, 1) for i in range(1, 6)]); edit(T["A"], T["B"])
        assert ref.run_scene(T).n_lines_to_opt == 0


def _angle_to(lines, axes):
    d = ref.directions(lines)
    return np.degrees(np.arccos(np.clip(np.abs((d * axes).sum(axis=1)), 0, 1)))


def test_two_families_move_to_their_axes():
    S = ref.crafted_families()
    R = ref.run_scene(S)
    n = len(S["A"])
    assert R.n_lines_to_opt == n and R.n_edges == n * (n - 1) and R.rounds == 2 and R.written_back == 1
    before = _angle_to(np.concatenate([S["A"], S["B"]], axis=1), S["axes"]); after = _angle_to(R.lines, S["axes"])
    # the measurements lie within about 0.3 degrees of the axes and there are 15 per line; the lines start about 2 degrees off
    # and every one ends nearer to its axis.  What remains is the rotation about the other family's axis, which the perpendicular edges do
    # not see and the parallel error 1 - cos, quadratic in the angle, at best halves per step
    assert before.mean() > 2.0 and np.all(after < before) and after.max() < 1.5 and after.mean() < 0.4 * before.mean(), (before, after)
    R1 = ref.run_scene(S, params=ref.default_params(iterations=0))
    chi0 = float((R1.round_chi2[0]).sum())
    assert R.chi2[0] < 0.05 * chi0 and R.chi2[1] <= R.chi2[0] and R.n_flagged == [0, 0] and not (R.rel < 0).any()
    # mid points are not constrained: they stay within the step noise
    mid0 = 0.5 * (S["A"] + S["B"]); mid1 = 0.5 * (R.lines[:, :3] + R.lines[:, 3:])
    assert np.abs(mid1 - mid0).max() < 1e-3


def test_fewer_than_ten_edges_break_after_round_one():
    S = ref.crafted([X] * 10, [(0, i, 1) for i in range(1, 10)])           # nine edges
    R = ref.run_scene(S)
    assert R.n_edges == 9 and R.rounds == 1 and R.iterations[1] == 0
    S = ref.crafted([X] * 11, [(0, i, 1) for i in range(1, 11)])           # ten
    assert ref.run_scene(S).rounds == 2


def _perp_partner(c):
    return np.array([c, math.sqrt(1 - c * c), 0.0])


def test_classification_thresholds_and_final_rejection_at_rest():
    """iterations = 0: nothing moves, so every chi2 is the geometry's.  Line 0 along X with perpendicular partners whose cosine against X is
    0.05 (chi2 0.0025), 0.12 (0.0144: flagged by round 2's 0.01 only, kept by the final <= 0.02) and 0.15 (0.0225: flagged twice, rejected)"""
    cs = [0.05] * 8 + [0.12, 0.15]
    S = ref.crafted([X] + [_perp_partner(c) for c in cs], [(0, i, 2) for i in range(1, 11)])
    R = ref.run_scene(S, params=ref.default_params(iterations=0))
    assert R.n_edges == 10 and R.rounds == 2 and R.iterations == [0, 0] and R.n_flagged == [1, 2]
    assert R.rel[0].tolist() == [0] + [2] * 9 + [-2]
    assert ref.lists_of(R.rel[0]) == ([], list(range(1, 10)) + [-1])
    assert np.array_equal(R.lines, np.concatenate([S["A"], S["B"]], axis=1))
    # parallel edges: error 1 - c.  A partner 30 degrees off: (1 - 0.866)^2 = 0.01795: flagged in round 2, kept; 35 degrees: 0.0327: rejected
    S = ref.crafted([X] + [X] * 8 + [_dir2(30), _dir2(35)], [(0, i, 1) for i in range(1, 11)])
    R = ref.run_scene(S, params=ref.default_params(iterations=0))
    assert R.n_flagged == [1, 2] and R.rel[0].tolist() == [0] + [1] * 9 + [-1]


def test_round_two_excludes_flagged_edges_and_their_line_rests():
    """line 0 must be parallel to five lines along Y and five along Z: the best it can do is 45 degrees from each, chi2 = (1 - 0.707)^2 =
    0.086, so round 1 flags all ten; in round 2 no vertex is active, nothing is computed, and the final rejection takes all ten"""
    d0 = np.array([1.0, 1.0, 0.8]); d0 /= np.linalg.norm(d0)
    S = ref.crafted([d0] + [Y] * 5 + [Z] * 5, [(0, i, 1) for i in range(1, 11)])
    R = ref.run_scene(S)
    assert R.rounds == 2 and R.iterations[0] >= 1 and R.n_flagged == [10, 10]
    assert R.iterations[1] == 0 and R.trials[1] == 0 and R.lam[1] == 0.0
    assert R.rel[0, 1:].tolist() == [-1] * 10
    d1 = ref.directions(R.lines)[0] @ ref.TILT                  # back in the frame the directions were written in
    assert abs(d1[1] - d1[2]) < 0.05 and abs(d1[0]) < 0.5 * abs(d0[0]) + 0.3     # it moved towards the Y-Z diagonal in round 1
    # with one satisfiable family beside the conflict only the satisfiable edges stay in round 2
    S = ref.crafted([ref.rot_vec([0, 0, 0.03]) @ Y] + [Y] * 7 + [Z] * 3, [(0, i, 1) for i in range(1, 11)])
    R = ref.run_scene(S)
    assert R.n_flagged == [3, 3] and R.rel[0, 1:].tolist() == [1] * 7 + [-1] * 3 and R.iterations[1] >= 1


def test_vertex0_write_back_quirk_both_ways():
    S = ref.crafted_families(line0=True); R = ref.run_scene(S)
    init = np.concatenate([S["A"], S["B"]], axis=1)
    assert R.written_back == 1 and np.abs(R.lines - init).max() > 1e-3 and np.array_equal(R.lines, R.est)
    S = ref.crafted_families(line0=False); R = ref.run_scene(S)
    n = len(init)
    # line 0 has no vertices: optimizer.vertex(0) == 0 holds for every i, nothing is written back although 15 lines were optimised
    assert R.n_lines_to_opt == n - 1 and R.written_back == 0 and np.array_equal(R.lines, init) and np.abs(R.est - init).max() > 1e-3
    # the rejections are written all the same
    S["rel"][1, 2] = 2                                       # a parallel neighbour declared perpendicular: error about 1
    R = ref.run_scene(S)
    assert R.written_back == 0 and R.rel[1, 2] == -2 and np.array_equal(R.lines, init)


def test_tree_order_and_ulp_nudges_stay_close():
    S = ref.crafted_families(); a = ref.run_scene(S); b = ref.run_scene(S, ref.Ops("tree", 3))
    assert np.array_equal(a.rel, b.rel) and 0 < np.abs(a.lines - b.lines).max() < 1e-3
    c = ref.run_scene(S, ref.Ops("tree"))
    assert np.array_equal(ref.run_scene(S, ref.Ops("tree")).lines, c.lines)


def test_generator_stays_inside_the_rejection_cap():
    nat, g1 = ref.accepted_scenes(4, seed0=2000)
    cor, g2 = ref.accepted_scenes(4, seed0=3000, corrupt=0.01)
    print("natural scenes: generated %d accepted %d; corrupted lists: generated %d accepted %d" % (g1, len(nat), g2, len(cor)))
    assert len(nat) * 2 >= g1 and len(cor) * 2 >= g2
    S, R = nat[0]
    assert (S["line_eq"][:, 0] == -1).any() and (S["linefn"][:, 2] == 0).any() and R.n_lines_to_opt > 50 and R.n_edges > 2000
    assert sum(R.n_flagged[0] for _, R in cor) > 50 and {R.written_back for _, R in cor + nat} == {0, 1}


def test_entry_points_declared_exported_and_bound(hvo):
    hdr = open(os.path.join(ROOT, "include", "hvo.h")).read()
    L = hvo.lib()
    for sym in ("hvo_line_struct_default_params", "hvo_line_struct_optimize", "hvo_stream_line_struct_optimize", "hvo_batch_line_struct_optimize",
                "hvo_line_opt_last_kernel_ms", "hvo_stream_line_opt_last_kernel_ms"):
        assert re.search(r"\bint\s+%s\s*\(" % sym, hdr), sym
        assert hasattr(L, sym), sym
    assert ctypes.sizeof(hvo.LineStructParams) == 4 * 8 + 2 * 4 + 4 * 4 == 56
    assert ctypes.sizeof(hvo.LineStructProblem) == 2 * 4 + 2 * 8 == 24
    assert ctypes.sizeof(hvo.LineOptResult) == 14 * 4 + 4 * 8 == 88
    # the library's defaults are the reference's, formed with libm on the host
    p = hvo.line_struct_params(); q = ref.default_params()
    assert p.cos_par == q["cos_par"] and p.cos_perp == q["cos_perp"] and p.huber_delta == q["huber_delta"] and p.chi2_reject == 0.02
    assert (np.float32(p.chi2_round[0]), np.float32(p.chi2_round[1])) == q["chi2_round"] and p.min_constraints == 5 and p.iterations == 5
    assert p.row_rule == hvo.LINE_STRUCT_ROW_UNSET and p.mode == hvo.LINE_STRUCT_CONSTRAINTS | hvo.LINE_STRUCT_OPTIMIZE
    assert hvo.rel_lists(np.array([0, 1, -2, 2, -1], np.int8)) == ([1, -1], [-1, 3])
    for m in ("line_struct_optimize", "batch_line_struct_optimize", "line_opt_last_kernel_ms"): assert hasattr(hvo.Context, m), m
    for m in ("line_struct_optimize", "line_opt_last_kernel_ms"): assert hasattr(hvo.Stream, m), m
