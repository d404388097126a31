"""The crafted ramps of tests/lsd_cases.py do reach the paths they are there for -- asserted on the oracle alone, with its path counters
(oracle.lsd_path_counts), so that tests/test_lsd_crafted_gpu.py compares the kernels with the oracle where it matters:

  * regions larger than a worker's private list (LA_CAP, lsd_async.inc): the `over` path of k_lsd_grow_async, the held-pixel list
    (LA_BCAP) of the younger workers inside such a region;
  * refine of a region of more than LA_CAP / 2 points: first growth and re-growth together overflow the list;
  * reduce_region_radius rounds that start above the closed form's limit (`reg_size <= 4096`): lane 0 walks the list, in refine_wave and
    in la_refine;
  * a re-growth with tau <= 0; the 0 / 2 pi wrap of isAligned; more than 200 segments (the keep-200 sort).

The preconditions are inequalities against the limits read from the kernel sources; the measured counters are printed (run with -s), they
are the record.  If an image misses its path, change the image -- never the inequality.

Not reached by any of these images (8-bit input bounds a region's extent along its gradient to 48 scaled pixels, so its front stays short
and its radius reduction never runs out of points):
  * reduce_region_radius ending with fewer than 2 points (`reject_reduce` stays 0);
  * more than LSD_RING pending points, i.e. the read-back of an expanded point from reg[] instead of the LDS ring (`max_pending`
    stays far below it).
Both are asserted below as they stand, so that an image that does reach one of them is noticed and moved into the table.
"""
import numpy as np
import pytest

import lsd_cases

LIM = lsd_cases.limits()


@pytest.fixture(scope="module")
def counts(orc):
    out = {}
    for name in lsd_cases.CASES:
        g = lsd_cases.make(name)
        out[name] = (orc.lsd_path_counts(g, big=LIM["REDUCE_CLOSED"]), len(orc.line_extract(g)[0]))
    return out


def test_limits_are_read_from_the_kernel_sources():
    print(LIM)
    assert LIM["LA_CAP"] >= 2 * LIM["REDUCE_CLOSED"] > 0 and 0 < LIM["LA_BCAP"] <= LIM["LA_CAP"]
    assert LIM["LSD_RING"] >= 64 and LIM["LSD_RING"] & (LIM["LSD_RING"] - 1) == 0


def test_generators_are_deterministic_and_sized():
    sizes = lsd_cases.by_size()
    assert set(sizes) == {(lsd_cases.H, lsd_cases.W), (lsd_cases.H_BIG, lsd_cases.W_BIG)}, sizes
    assert lsd_cases.W % 4 and lsd_cases.H % 4 and lsd_cases.W % 32 and lsd_cases.H % 32
    for name in lsd_cases.CASES:
        assert np.array_equal(lsd_cases.make(name), lsd_cases.make(name)), name
    assert int(lsd_cases.saw(np.array([-1.0]))[0]) == 255 and int(lsd_cases.saw(np.array([256.5]))[0]) == 0


@pytest.mark.parametrize("name", list(lsd_cases.CASES))
def test_image_reaches_its_paths(counts, name):
    c, nkl = counts[name]
    paths = lsd_cases.CASES[name][1]
    print("\n%-12s key lines %3d  paths %s\n             %s" % (name, nkl, ",".join(paths) or "-", " ".join("%s=%d" % kv for kv in c.items())))
    for p in paths:
        if p == "region_gt_la_cap": assert c["max_region"] > LIM["LA_CAP"], (name, p, c["max_region"])
        elif p == "refine_gt_half_la_cap": assert c["max_refine"] > LIM["LA_CAP"] // 2, (name, p, c["max_refine"])
        elif p == "reduce_gt_closed": assert c["max_reduce_start"] > LIM["REDUCE_CLOSED"] and c["reduce_rounds_big"] >= 1, (name, p, c["max_reduce_start"])
        elif p == "tau_le_0": assert c["tau_le_0"] >= 1, (name, p)
        elif p == "segments_gt_200": assert c["segments"] > 200, (name, p, c["segments"])
        elif p == "wrap": assert c["wrap_growths"] >= 1 and c["wrap_points"] >= 1, (name, p)
        else: raise AssertionError("unknown path %r" % p)
    assert c["segments"] < 16384 and nkl >= 10, (name, c["segments"], nkl)
    assert nkl == min(c["segments"], 200)


@pytest.mark.parametrize("form", list(lsd_cases.FORMS))
def test_knobs_force_the_forms_on_the_crafted_batches(hvo, monkeypatch, form):
    """the batches of tests/test_lsd_crafted_gpu.py (the frames of one size each) are grown by the form its knobs name: evaluated by
    the plan's own selection, without a device"""
    import os
    for k in list(os.environ):
        if k.startswith("HVO_"): monkeypatch.delenv(k)
    env, want = lsd_cases.FORMS[form]
    for k, v in env.items(): monkeypatch.setenv(k, v)
    for (h, w), names in lsd_cases.by_size().items():
        got = hvo.plan_select(w, h, len(names))["lsd"]
        bad = {f: (got[f], v) for f, v in want.items() if got[f] != v}
        assert not bad, "%s, %d frames of %d x %d: (selected, wanted) %s" % (env, len(names), w, h, bad)


def test_paths_no_image_reaches(counts):
    """see the module docstring: named here so that they are not forgotten"""
    for name, (c, _) in counts.items():
        assert c["reject_reduce"] == 0, name
        assert c["max_pending"] <= LIM["LSD_RING"], (name, c["max_pending"])


def test_counters_observe_only(orc, synth):
    """orc_lsd_detect gives the same segments before, between and after counted runs, and the counters agree with what it returns"""
    for g in (lsd_cases.make("holes_diag"), synth.make_gray("std", 0x5EED0002)):
        s0 = orc.lsd_detect(g)
        c = orc.lsd_path_counts(g)
        s1 = orc.lsd_detect(g)
        assert np.array_equal(s0, s1) and c["segments"] == len(s0)
        assert c == orc.lsd_path_counts(g)
        assert c["regions"] >= c["refines"] >= c["reject_regrow"] and c["max_region"] >= c["max_refine"] and c["max_first_plus_regrow"] >= c["max_refine"]
        assert orc.lsd_path_counts(g, big=0)["regions_big"] == c["regions"]


def test_the_1280_frame_of_the_async_test_stays_below_a_private_list(orc, synth):
    """test_lines_async_1280 (test_lsd_gpu.py) runs the async kernel on this frame: its regions fit a worker's private list, so it does
    NOT take the `over` path -- the crafted ramps are what does"""
    c = orc.lsd_path_counts(synth.make_gray("std", 0x5EED0003, 1280, 960))
    print(c)
    assert 0 < c["max_first_plus_regrow"] and c["max_region"] < LIM["LA_CAP"] and c["max_first_plus_regrow"] < LIM["LA_CAP"]
