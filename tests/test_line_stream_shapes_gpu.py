"""The two streaming kernels of the line chain at the edges of their tiling.

k_lsd_pre walks a band of 192 scaled columns over a segment of 96 scaled rows in chunks of 4 scaled rows; k_lbd_blur_sobel gives a
thread 4 columns and R = 32 output rows.  Both have a second, simpler formulation behind an environment switch (HVO_LSD_PRE_SPLIT=1:
k_lsd_blur + k_lsd_resize_grad, HVO_LBD_SPLIT=1: k_lbd_blur5 + k_lbd_sobel), so every pixel of what they leave -- the defined mask, the
records of the defined pixels, the gradient image, read back with Context.lsd_images -- is compared byte for byte, and the key lines
are compared with the CPU oracle as in test_lsd_gpu.py.

Geometries (w, h) -> scaled (sw, sh) = (round(0.8 w), round(0.8 h)).  The contexts run one ORB level: the default eight refuse images
below ~137 pixels, one level accepts 64.  The issue's rows-per-block cases h = R - 1, R, R + 1 are below that limit too, so the same
three positions are taken one and two blocks further down (h = 2R, 2R + 1, 3R - 1, 3R, 3R + 1), and 64 x 64 is the smallest image the
chain accepts.  A segment starts at a multiple of 96 scaled rows, which is a multiple of the chunk: no segment starts in mid-period."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-4
R = 32          # LBD_FUSED_ROWS
CH = 4          # PRE_CH

# (w, h, special frame)                      sw   sh   what the case is there for
CASES = [
    (200, 121, "const"),    # 160   97   one band, sw % 32 == 0; sh - 1 == 96: the segment's last chunk has one row ((sh - 1) % 4 == 0)
    (240, 122, "noise"),    # 192   98   exactly one band; sh - 1 == 97: the second segment has one gradient row ((sh - 1) % 4 == 1)
    (241, 125, "corner"),   # 193  100   the last band is a single scaled column, sw % 32 == 1; (sh - 1) % 4 == 3; w % 4 == 1
    (239, 64, "noise"),     # 191   51   sw % 32 == 31; w % 4 == 3; h == 2R; (sh - 1) % 4 == 2
    (242, 65, "corner"),    # 194   52   two columns in the last band; w % 4 == 2; h == 2R + 1: the last block holds image row h - 1 only
    (64, 95, "const"),      #  51   76   the narrowest image; h == 3R - 1
    (66, 96, "noise"),      #  53   77   w % 4 == 2; h == 3R
    (65, 97, "corner"),     #  52   78   w % 4 == 1; h == 3R + 1
    (64, 64, "noise"),      #  51   51   the smallest image the chain accepts: top and bottom reflection two blocks apart
]


def check(kl_g, d_g, fn_g, kl_o, d_o, fn_o):
    assert len(kl_g) == len(kl_o), (len(kl_g), len(kl_o))
    for f in ("class_id", "octave", "num_pixels"):
        assert np.array_equal(kl_g[f], kl_o[f]), f
    for f in ("angle", "pt_x", "pt_y", "response", "sx", "sy", "ex", "ey", "sox", "soy", "eox", "eoy", "length"):
        assert np.allclose(kl_g[f], kl_o[f], rtol=0, atol=TOL), f
    assert np.allclose(kl_g["size"], kl_o["size"], rtol=1e-6, atol=1e-2)
    assert np.array_equal(d_g, d_o), int((d_g != d_o).sum())
    assert np.allclose(fn_g, fn_o, rtol=1e-9, atol=1e-7)


@pytest.fixture(scope="module")
def big(synth):
    return synth.make_gray("std", 11, 704, 480)


def frames_of(big, w, h, special):
    """a crop and its flipud, as test_lines_odd_geometry takes them, and one crafted frame"""
    crop = np.ascontiguousarray(big[:h, :w])
    rng = np.random.default_rng(1000 * w + h)
    if special == "noise":          # nearly every pixel has an angle: the queue of a chunk is full
        s = rng.integers(0, 256, (h, w), dtype=np.uint8)
    elif special == "const":        # no pixel has one: an empty queue, zero lines on both sides
        s = np.full((h, w), 90, np.uint8)
    else:                           # flat but for the corner that lies in the last band and the last segment
        s = np.full((h, w), 90, np.uint8)
        s[h - 24:, w - 24:] = rng.integers(0, 256, (24, 24), dtype=np.uint8)
    return np.ascontiguousarray(np.stack([crop, crop[::-1], s]))


def run(hvo, g, twice):
    """key lines and images of every frame; twice: the same again on the same context, which must give the same bytes"""
    n, h, w = g.shape
    ctx = hvo.Context(max_batch=n, orb_nlevels=1)
    try:
        ctx.batch_upload(g, np.zeros((n, h, w), np.uint16))
        out = []
        for _ in range(2 if twice else 1):
            ctx.batch_run(hvo.STAGE_LSD)
            res = ctx.batch_download(hvo.STAGE_LSD)
            rep = ctx.launch_report()["lsd"]
            split = os.environ.get("HVO_LSD_PRE_SPLIT") == "1"                 # the forms the caller asked for are the ones that ran
            assert (rep["pre"], rep["lbd_gradient"]) == (("split", "split") if split else ("fused", "fused")), rep
            out.append(([(r["status"], r["kl"].copy(), r["ldesc"].copy(), r["linefn"].copy()) for r in res], [ctx.lsd_images(b) for b in range(n)]))
    finally:
        ctx.close()
    if twice:
        (l0, i0), (l1, i1) = out
        for b in range(n):
            assert l0[b][0] == l1[b][0]
            for a, c in zip(l0[b][1:], l1[b][1:]):
                assert a.tobytes() == c.tobytes(), "second run differs, frame %d" % b
            for k in ("mask", "records", "dxy"):
                assert i0[b][k].tobytes() == i1[b][k].tobytes(), "second run differs: %s of frame %d" % (k, b)
    return out[0]


@pytest.mark.parametrize("w,h,special", CASES)
def test_line_stream_shapes(hvo, orc, big, monkeypatch, w, h, special):
    g = frames_of(big, w, h, special)
    sw, sh = int(round(w * 0.8)), int(round(h * 0.8))
    monkeypatch.delenv("HVO_LSD_PRE_SPLIT", raising=False)
    monkeypatch.delenv("HVO_LBD_SPLIT", raising=False)
    lines, imgs = run(hvo, g, twice=True)                       # the fused kernels
    monkeypatch.setenv("HVO_LSD_PRE_SPLIT", "1")
    monkeypatch.setenv("HVO_LBD_SPLIT", "1")
    _, ref = run(hvo, g, twice=False)                           # the two-kernel formulations
    for b in range(len(g)):
        assert imgs[b]["mask"].shape == (sh, (sw + 31) // 32) and imgs[b]["dxy"].shape == (h, w, 2)
        for k in ("mask", "records", "dxy"):
            a, c = imgs[b][k], ref[b][k]
            assert a.shape == c.shape, (k, b, a.shape, c.shape)
            if a.tobytes() != c.tobytes():
                bad = np.argwhere(a != c)
                raise AssertionError("%s of frame %d differs from the split kernels' at %d places, first %s" % (k, b, len(bad), bad[:4].tolist()))
        if special == "const" and b == 2:
            assert len(imgs[b]["records"]) == 0 and not imgs[b]["mask"].any() and not imgs[b]["dxy"].any()
        if special == "noise" and b == 2:
            assert len(imgs[b]["records"]) > 0.5 * (sw - 1) * (sh - 1)      # most of a chunk's queue places are taken, several wave-passes per chunk
        status, kl, d, fn = lines[b]
        assert status == 0
        kl_o, d_o, fn_o = orc.line_extract(g[b])
        check(kl, d, fn, kl_o, d_o, fn_o)
        if special == "const" and b == 2:
            assert len(kl) == 0 and len(kl_o) == 0
