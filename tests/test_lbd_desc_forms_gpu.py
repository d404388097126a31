"""The two formulations of the LBD descriptor kernels, byte for byte.

HVO_LBD_DESC=0 selects k_lbd_desc_v1 (one kernel from the key line to the 32 bytes); the default is k_lbd_line_setup (one line per lane:
direction, length, the 63 band rows' starts) + k_lbd_desc (blocks of positions without a per-position test, a float median as the clamp,
max / min accumulation, 72 band-sum chains, ordered sums read from LDS).  Context.lbd_desc hands crafted key lines to whichever form
the context's plan selected, so lengths, angles and positions the detector does not produce on a small image are reached:

  num_pixels   1, 2, 3 (halfWidth 0 and 1), 31 / 32 / 33 and 63 / 64 / 65 (the edges of the 8-position blocks of the steep branch and of
               the 32-position tile of the along-rows branch), 97 (more than three tiles, a remainder of one)
  angles       both branches (|cos| > |sin| and not), both signs, pi/4 where the float cos / sin decide the branch, pi and -pi + 1e-3
  centres      mid-image and the four corners: band rows and positions clamp on every border
  images       96 x 80 and 98 x 82 (w % 4 != 0: the other Sobel instantiation); seeded noise plus two ramps, gradients of both signs

and 200 seeded random lines with end points inside the image.  A second test runs the detector with and without cullingLine on a
160 x 120 frame under both settings: the set-up kernel's two launch sites."""
import contextlib
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LENGTHS = (1, 2, 3, 31, 32, 33, 63, 64, 65, 97)
ANGLES = (0.0, 1e-3, np.pi / 4, -np.pi / 4, np.pi / 2, -np.pi / 2, 3 * np.pi / 4, np.pi, -np.pi + 1e-3)
SIZES = ((96, 80), (98, 82))


@contextlib.contextmanager
def lbd_desc_setting(value):
    old = os.environ.get("HVO_LBD_DESC")
    if value is None:
        os.environ.pop("HVO_LBD_DESC", None)
    else:
        os.environ["HVO_LBD_DESC"] = value
    try:
        yield
    finally:
        if old is None:
            os.environ.pop("HVO_LBD_DESC", None)
        else:
            os.environ["HVO_LBD_DESC"] = old


def image(w, h):
    rng = np.random.default_rng(7000 + w)
    x, y = np.meshgrid(np.arange(w), np.arange(h))
    g = rng.integers(0, 96, (h, w)) + 150.0 * x / (w - 1) * (y < h // 2) + 150.0 * (h - 1 - y) / (h - 1) * (y >= h // 2)
    return np.ascontiguousarray(np.clip(g, 0, 255).astype(np.uint8))


def keylines(hvo, w, h):
    rows = []
    centres = ((w / 2.0, h / 2.0), (0.0, 0.0), (w - 1.0, 0.0), (0.0, h - 1.0), (w - 1.0, h - 1.0))
    for n in LENGTHS:
        for a in ANGLES:
            for cx, cy in centres:
                dx, dy = 0.5 * n * np.cos(a), 0.5 * n * np.sin(a)
                rows.append((a, cx - dx, cy - dy, cx + dx, cy + dy, n))
    rng = np.random.default_rng(9000 + w)
    for _ in range(200):
        sx, ex = rng.uniform(0, w - 1, 2); sy, ey = rng.uniform(0, h - 1, 2)
        rows.append((np.arctan2(ey - sy, ex - sx), sx, sy, ex, ey, int(max(abs(ex - sx), abs(ey - sy))) + 1))
    kl = np.zeros(len(rows), hvo.KEYLINE_DT)
    for i, (a, sx, sy, ex, ey, n) in enumerate(rows):
        kl[i]["angle"] = a; kl[i]["class_id"] = i; kl[i]["num_pixels"] = n
        for f, v in (("sx", sx), ("sy", sy), ("ex", ex), ("ey", ey), ("sox", sx), ("soy", sy), ("eox", ex), ("eoy", ey)):
            kl[i][f] = v
        kl[i]["pt_x"] = 0.5 * (sx + ex); kl[i]["pt_y"] = 0.5 * (sy + ey); kl[i]["length"] = np.hypot(ex - sx, ey - sy); kl[i]["size"] = 1.0
    return kl


def describe(hvo, setting, g, kl):
    """a new context per setting: the plan reads the switch once, when it is built"""
    with lbd_desc_setting(setting):
        assert hvo.plan_select(g.shape[1], g.shape[0], 1)["lsd"]["lbd_desc"] == (0 if setting == "0" else 1)      # the switch selects the other form
        ctx = hvo.Context(max_batch=1, orb_nlevels=1)
        try:
            first = ctx.lbd_desc(g, kl)
            again = ctx.lbd_desc(g, kl)                 # the same plan and scratch once more
        finally:
            ctx.close()
    assert first.tobytes() == again.tobytes()
    return first


@pytest.fixture(scope="module")
def cases(hvo, orc):
    out = []
    for w, h in SIZES:
        g = image(w, h); kl = keylines(hvo, w, h)
        out.append((w, h, kl, orc.lbd_compute(g, kl), describe(hvo, None, g, kl), describe(hvo, "0", g, kl)))
    return out


def differing(a, b):
    return np.flatnonzero((a != b).any(axis=1))


def test_crafted_lines_cover_both_branches_and_borders(cases):
    for w, h, kl, _, _, _ in cases:
        assert len(kl) == len(LENGTHS) * len(ANGLES) * 5 + 200
        c, s = np.cos(kl["angle"].astype(np.float64)).astype(np.float32), np.sin(kl["angle"].astype(np.float64)).astype(np.float32)
        along = np.abs(c) > np.abs(s)
        assert along.sum() > 100 and (~along).sum() > 100


def test_new_form_equals_the_one_kernel_form(cases):
    for w, h, kl, _, new, old in cases:
        bad = differing(new, old)
        assert len(bad) == 0, "%d x %d: %d lines differ, first %s" % (w, h, len(bad), [(int(kl["num_pixels"][i]), float(kl["angle"][i])) for i in bad[:5]])


def test_both_forms_equal_the_oracle(cases):
    for w, h, kl, ref, new, old in cases:
        for name, d in (("HVO_LBD_DESC unset", new), ("HVO_LBD_DESC=0", old)):
            bad = differing(d, ref)
            assert len(bad) == 0, "%s, %d x %d: %d lines differ from the oracle, first %s" % (
                name, w, h, len(bad), [(int(kl["num_pixels"][i]), float(kl["angle"][i])) for i in bad[:5]])


def test_descriptors_are_not_degenerate(cases):
    """the comparison above would also pass on constant output: the lines see gradients, so their descriptors differ from each other"""
    for w, h, kl, ref, new, _ in cases:
        assert len(np.unique(new, axis=0)) > len(kl) // 2


def run_detector(hvo, setting, g):
    """ldesc after the first descriptor pass (STAGE_LSD) and after cullingLine's second pass, each with its key lines"""
    n, h, w = g.shape
    with lbd_desc_setting(setting):
        ctx = hvo.Context(max_batch=n, orb_nlevels=1)
        try:
            ctx.batch_upload(g, np.zeros((n, h, w), np.uint16))
            out = []
            for stages in (hvo.STAGE_LSD, hvo.STAGE_LSD | hvo.STAGE_LSD_CULL):
                ctx.batch_run(stages)
                res = ctx.batch_download(stages)
                rep = ctx.launch_report()["lsd"]
                assert (rep["lbd_desc"], rep["cull"]) == (0 if setting == "0" else 1, int(stages != hvo.STAGE_LSD)), rep
                assert all(r["status"] == 0 for r in res)
                out.append([(r["kl"].copy(), r["ldesc"].copy()) for r in res])
        finally:
            ctx.close()
    return out


def test_both_launch_sites_on_a_detector_run(hvo, orc, synth):
    g = np.ascontiguousarray(synth.make_gray("std", 0x5EED1000, 160, 120)[None])
    new, old = run_detector(hvo, None, g), run_detector(hvo, "0", g)
    for p, what in enumerate(("first pass", "second pass")):
        (kl_n, d_n), (kl_o, d_o) = new[p][0], old[p][0]
        assert len(kl_n) > 5, what
        assert kl_n.tobytes() == kl_o.tobytes(), what
        assert d_n.tobytes() == d_o.tobytes(), what
        assert np.array_equal(d_n, orc.lbd_compute(g[0], kl_n)), what
    assert len(new[1][0][0]) <= len(new[0][0][0])
