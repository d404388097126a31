"""The census and the vacuity conditions of tests/arena_cases.py, on the CPU.

Every host-array entry point stages through one grow-only device buffer per context (hvo_call_arena, csrc/arena.hip), directly or through
the runner of a staged call (StagedCall::begin, csrc/staged_call.hpp); the two resident slot maps add a grow-only scratch of their own
(sm_grow on d_a / d_b).  Each call site carves its own layout and decides by hand what it uploads, what it clears and what it trusts a
kernel to write.  tests/test_call_arena_gpu.py runs every such entry point on a dirty arena; this file
makes sure that a new call site cannot stay out of that test: the sites are counted in the sources and every one must be claimed by a case."""
import glob
import os
import re

import numpy as np
import pytest

import arena_cases as ac
from conftest import PKG_DIR

# what is not an entry point's call site: the function itself and the test door that grows the arena the way a call would (both in arena.hip),
# and arena_begin of match.hip's older matchers, which share the arena but are not run dirty yet ("not covered yet")
NOT_A_SITE = {"arena.hip": 2, "match.hip": 1}
# a site reaches the arena by calling hvo_call_arena itself or through the runner's begin(dev_bytes, ..) (a container's begin() has no argument)
ARENA_SITE = r"\bhvo_call_arena\s*\(|\.begin\s*\(\s*\w"
ENTRY_POINTS = ("lines_3d", "vanishing_points", "plane_clouds", "normals_lpvo", "surface_normals", "track_manhattan", "batch_track_manhattan",
                "undistort_keypoints", "assign_features_to_grid", "assign_lines_to_grid", "compute_bow", "search_by_bow", "line_struct_optimize",
                "pose_optimize", "pnp_ransac", "search_by_projection_keyframe", "fuse_points", "fuse_points_slots", "create_new_map_points",
                "search_local_points", "search_local_lines", "create_new_map_lines", "fuse_lines", "fuse_lines_slots", "refresh_map_points",
                "refresh_map_lines")


@pytest.fixture(scope="module")
def env():
    return ac.env()


def _count(pattern):
    found = {}
    for path in sorted(glob.glob(os.path.join(PKG_DIR, "csrc", "*.hip"))):
        src = re.sub(r"//[^\n]*", "", open(path).read())                 # a comment that names the function is not a call
        n = len(re.findall(pattern, src))
        if n: found[os.path.basename(path)] = n
    return found


def test_every_arena_call_site_is_claimed_by_a_case():
    found = _count(ARENA_SITE)
    for f, n in NOT_A_SITE.items():
        assert found.get(f, 0) == n, (f, found.get(f))
        del found[f]
    claimed = {}
    for c in ac.CASES:
        for f, tag in c.sites:
            if tag not in ("d_a", "d_b"): claimed.setdefault(f, set()).add(tag)
    assert {f: len(t) for f, t in claimed.items()} == found, ({f: sorted(t) for f, t in claimed.items()}, found)
    assert sum(found.values()) == 22


def test_every_slot_map_scratch_is_claimed_by_a_case():
    found = _count(r"\bsm_grow\s*\(\s*m\s*,")                              # the calls; the definition's first parameter has a type
    claimed = {}
    for c in ac.CASES:
        for f, tag in c.sites:
            if tag in ("d_a", "d_b"): claimed.setdefault(f, set()).add(tag)
    assert {f: len(t) for f, t in claimed.items()} == found == {"local_points.hip": 2, "local_lines.hip": 2}
    assert sorted(c.name for c in ac.CASES if c.uses_map) == ["search_local_lines", "search_local_points"]


def test_design_md_has_a_row_for_every_site():
    """DESIGN.md section 8 is the reading the device run confirms: one row per call site, naming its file and the function that carves it"""
    from conftest import ROOT
    doc = open(os.path.join(ROOT, "DESIGN.md")).read()
    sec = doc[doc.index("## 8. The call arena"):]
    rows = [r for r in sec.splitlines() if r.startswith("| `")]
    for c in ac.CASES:
        for f, tag in c.sites:
            assert any(r.startswith("| `%s` " % f) and "`%s`" % tag in r.split("|")[1] for r in rows), (f, tag)
    assert len(rows) == 22 + 4                                           # the arena's call sites, and four rows for the two maps' scratch
    for word in ("plane map", "key-frame database", "bag-of-words blocks"):
        assert word in sec, word                                         # named as not covered yet


def test_the_case_table_names_every_entry_point_once(env):
    names = [c.name for c in ac.CASES]
    assert sorted(names) == sorted(ENTRY_POINTS) and len(set(names)) == len(names)
    for n in names:
        assert callable(getattr(env.hvo.Context, n)), n


@pytest.mark.parametrize("name", ENTRY_POINTS)
def test_inputs_are_not_vacuous_and_l_needs_more_than_s(env, name):
    c = ac.BY_NAME[name]
    need = {}
    for size in ("S", "L"):
        i, w = ac.inputs(env, name, size)
        if c.want:
            assert w is not None
            c.vacuous(env, i, w)
        if c.arena: need[size] = c.arena(env, i)
    if c.arena:
        assert 0 < need["S"] < need["L"], need
        assert ac.arena_capacity(need["S"]) >= need["S"] and ac.arena_capacity(need["S"]) % 4096 == 0


def test_l_is_larger_than_s_where_the_layout_is_not_restated(env):
    """the layouts that are a page of carving are not restated here; their size grows with the counts, and those grow"""
    size = {"vanishing_points": lambda i: len(i["kl"]), "plane_clouds": lambda i: i["depth"].size, "surface_normals": lambda i: i["depth"].size,
            "search_by_bow": lambda i: len(i["fr"]["desc"]) + len(i["kf"]["desc"]), "line_struct_optimize": lambda i: len(i["S"]["linefn"]),
            "pose_optimize": lambda i: sum(len(P.kp_xy) + len(P.linefn) for P in i["P"]), "pnp_ransac": lambda i: sum(len(p["p3d"]) for p in i["problems"]),
            "search_by_projection_keyframe": lambda i: len(i["kp"]) + len(i["cand"]["pos"]), "fuse_points": lambda i: len(i["kf"]["kp_un"]) + len(i["mp"]["pos"]),
            "fuse_points_slots": lambda i: len(i["kf"]["kp_un"]) + len(i["slots"]), "create_new_map_points": lambda i: len(i["cur"]["kp_un"]),
            "search_local_lines": lambda i: len(i["kl"]) + len(i["M"]["pos"]),
            "create_new_map_lines": lambda i: len(i["cur"]["kl"]) * len(i["kfs"]), "fuse_lines": lambda i: sum(len(k["kl"]) for k in i["kfs"]) + len(i["mp"]["pos"]),
            "fuse_lines_slots": lambda i: sum(len(k["kl"]) for k in i["kfs"]) + len(i["slots"]),
            "refresh_map_points": lambda i: len(i["pos"]) + len(i["obs"]["obs_desc"]), "refresh_map_lines": lambda i: len(i["pos"]) + len(i["obs"]["obs_desc"])}
    for c in ac.CASES:
        assert (c.arena is not None) != (c.name in size), c.name
    for name, f in size.items():
        assert f(ac.inputs(env, name, "S")[0]) < f(ac.inputs(env, name, "L")[0]), name


def test_the_comparison_helpers():
    a = dict(x=np.array([1.0, np.nan], np.float32), n=3, r=[np.arange(3)], kernel_ms=(1.0, 2.0))
    b = dict(x=np.array([1.0, np.nan], np.float32), n=3, r=[np.arange(3)], kernel_ms=(5.0, 6.0))
    ac.identical(a, b)                                                    # timings are not results
    with pytest.raises(AssertionError):
        ac.identical(a, dict(b, n=4))
    with pytest.raises(AssertionError):
        ac.identical(a, dict(b, x=np.array([1.0, -np.nan], np.float32)))   # byte identity sees a NaN's sign
    assert ac.same_bits(a["x"], np.array([1.0, -np.nan], np.float32)) and not ac.same_bits(a["x"], np.array([1.0, 2.0], np.float32))
    assert ac.arena_capacity(1) == 4096 and ac.arena_capacity(4096) == 8192 and ac.arena_capacity(3276) == 4096
