"""Map-plane association, PlaneMatcher::SearchMapByCoefficients (reference src/PlaneMatcher.cpp:10-81; csrc/plane_assoc.hip), without a GPU:
known answers on the restatement tests/plane_assoc_ref.py for every rule that decides bits, the generated scenes' coverage, and the new
symbols' declarations, exports and struct sizes."""
import ctypes
import os
import re

import numpy as np

import plane_assoc_ref as ref
from conftest import ROOT, PKG_DIR

F32 = np.float32
NEW = ["hvo_plane_map_create", "hvo_plane_map_destroy", "hvo_plane_map_set", "hvo_plane_map_set_bad", "hvo_plane_map_counts",
       "hvo_plane_map_slot", "hvo_plane_map_last_error", "hvo_match_planes", "hvo_stream_match_planes", "hvo_batch_match_planes"]


def test_crafted_known_answers():
    """ties (first wins) for the three roles, the fall-through and its removal, every threshold met exactly (strict), negative angles, bad
    slots, empty and NaN clouds: the hand-written answers on poses where the 4 x 4 product is exact in float and double alike"""
    assert np.array_equal(ref.world_coeff(ref.T_EXACT, ref.exact_frame_plane()), np.array([1, 0, 0, 0], F32))
    assert np.array_equal(ref.world_coeff(ref.T_EXACT, ref.exact_frame_plane(-0.375)), np.array([1, 0, 0, -0.375], F32))
    for name, coef, Tcw, slots, th, exp in ref.crafted_cases():
        o = ref.search_map(coef, Tcw, slots, th)
        got = (int(o["match"][0]), int(o["vertical"][0]), int(o["parallel"][0]))
        assert got == tuple(exp[:3]), (name, got, exp)
        assert o["dist"][0] == F32(exp[3]), (name, o["dist"][0], exp[3])
        assert o["n_matches"] == int(exp[0] >= 0), name


def test_fall_through_depends_on_the_prefix_minimum():
    """the one order-dependent rule: slot 1 is consumed or not depending on the distances before it"""
    c = ref.exact_frame_plane().reshape(1, 4)
    a, b = ref.slot(1.0, [0.03125]), ref.slot(0.9990234375, [0.0625])
    o = ref.search_map(c, ref.T_EXACT, [a, b])
    assert (o["match"][0], o["parallel"][0], o["fell_through"][0]) == (0, 1, [1])
    o = ref.search_map(c, ref.T_EXACT, [b, a])                               # the other order: both consumed in turn
    assert (o["match"][0], o["parallel"][0], o["fell_through"][0], o["dist"][0]) == (1, -1, [], F32(0.03125))
    o = ref.search_map(c, ref.T_EXACT, [b])
    assert (o["match"][0], o["parallel"][0]) == (0, -1)


def test_several_frame_planes_and_offsets():
    """each frame plane runs its own thresholds; pM3 enters the distance"""
    c = np.stack([ref.exact_frame_plane(), ref.exact_frame_plane(-0.5)])
    slots = [ref.slot(1.0, [0.0625]), ref.slot(1.0, [0.5 + 0.03125])]
    o = ref.search_map(c, ref.T_EXACT, slots)
    assert list(o["match"]) == [0, 1] and list(o["dist"]) == [F32(0.0625), F32(0.03125)] and o["n_matches"] == 2
    assert list(o["parallel"]) == [1, 0]                                       # the other slot is gated, too far, and parallel
    assert np.array_equal(o["dist_mat"], np.array([[0.0625, 0.53125], [0.4375, 0.03125]], F32))


def test_world_coeff_against_float64():
    rng = np.random.RandomState(5)
    for _ in range(200):
        T = ref.pose(ref.rot(rng.normal(size=3), rng.uniform(0, 180)), rng.uniform(-3, 3, 3))
        c = rng.normal(size=4).astype(F32)
        T4 = np.vstack([T.astype(np.float64), [0, 0, 0, 1]])
        exact = T4.T @ c.astype(np.float64)
        got = ref.world_coeff(T, c)
        # the double sums carry at most three roundings of 2^-53 relative each before the one rounding to float
        assert np.all(np.abs(got.astype(np.float64) - exact) <= np.abs(exact) * 2.0 ** -24 + 4 * 2.0 ** -50 * np.abs(T4.T).dot(np.abs(c)))
    T = ref.pose(np.eye(3), (0, 0, 0))
    assert np.array_equal(ref.world_coeff(T, [0.5, -0.25, 0.125, 3.0]), np.array([0.5, -0.25, 0.125, 3.0], F32))


def test_generated_scenes_are_not_vacuous():
    """a condition on the inputs of the GPU tests: each role, the fall-through (also one that ends as the parallel plane) and an unmatched
    frame plane occur, under both threshold sets"""
    for th in (ref.DEFAULT_TH, ref.TUM3_TH):
        tot = dict(match=0, vertical=0, parallel=0, fell=0, unmatched=0, fell_parallel=0)
        for sc in ref.SCENES + [ref.BIG_SCENE]:
            coef, Tcw, slots = ref.make_scene(*sc)
            for k, v in ref.scene_stats(ref.search_map(coef, Tcw, slots, th)).items():
                tot[k] += v
        assert all(v > 0 for v in tot.values()), (th, tot)
    coef, Tcw, slots = ref.make_scene(*ref.BIG_SCENE)
    sizes = np.array([len(s[1]) for s in slots])
    assert len(slots) > 2000 and sizes.sum() >= 1000000 and sizes.max() > 0.25 * sizes.sum() and len(slots) % 64 and np.all(sizes[sizes > 0] % 64 != 0)
    assert any(s[2] for s in slots) and any(len(s[1]) == 0 for s in slots) and any(np.isnan(s[1]).any() for s in slots)


def test_new_symbols_declared_exported_and_sized(hvo):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hvo.h")).read(), flags=re.S)
    lib = ctypes.CDLL(os.path.join(PKG_DIR, "csrc", "libhvo.so"))
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert hasattr(lib, n), n
        assert n in hvo.EXPORTS, n
    assert ctypes.sizeof(hvo.PlaneMatch) == 2312                          # 2 + 5 x 64 ints / floats + 64 x 4 floats
    assert hvo.PlaneMatch.pM.offset == 8 + 5 * 256 and hvo.PlaneMatch.dist.offset == 8 + 4 * 256
    assert hvo.PLANE_CLOUD_DT.itemsize == 40
    lib.hvo_abi_version.restype = ctypes.c_int
    assert lib.hvo_abi_version() == 3
    assert tuple(F32(v) for v in hvo.PLANE_MATCH_DEFAULT_TH) == tuple(F32(v) for v in ref.DEFAULT_TH)
