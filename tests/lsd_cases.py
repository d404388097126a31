"""Crafted images for line growing: sawtooth ramps whose aligned regions are thousands of points large.

The gradient magnitude of a pixel must exceed rho = 2 / sin(22.5 deg) = 5.22 grey levels per scaled pixel to carry a level-line angle.
An 8-bit sawtooth of slope 6 per pixel (7.5 per scaled pixel) does, everywhere but at its 255 -> 0 steps: between two steps lies a strip
about 34 scaled pixels wide and as long as the image, one aligned region.  Bending, tilting or piercing the strips makes the rectangle of
such a region sparse, which sends it through refine and reduce_region_radius.

The limits these regions are meant to pass are read from the kernel sources, so a moved limit moves the preconditions of
tests/test_lsd_crafted.py with it (or fails there loudly).  CASES names, per image, the paths it is there for; the CPU test asserts with
the oracle's path counters (oracle.lsd_path_counts) that the image does reach them.
"""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "a-low-texture-robust-hybrid-feature-based-visual-odometry_amd", "csrc")

W, H = 322, 397                 # odd geometry: no multiple of 4 or 32, scaled 258 x 318
W_BIG, H_BIG = 640, 480


def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _define(text, name, where):
    m = re.findall(r"^\s*#\s*define\s+%s\s+(\d+)\b" % name, text, re.M)
    assert len(m) == 1, "%s: expected one '#define %s <number>', found %d" % (where, name, len(m))
    return int(m[0])


def limits():
    """LA_CAP, LA_BCAP (lsd_async.inc), LSD_RING and the largest list the closed-form reduce_radius_wave takes (`reg_size <= N`, stated
    once in refine_wave of lsd.hip and once in la_refine of lsd_async.inc: the two must agree)"""
    a, l = _read("lsd_async.inc"), _read("lsd.hip")
    closed = [re.findall(r"if\s*\(\s*reg_size\s*<=\s*(\d+)\s*\)", t) for t in (l, a)]
    assert len(closed[0]) == 1 and len(closed[1]) == 1 and closed[0] == closed[1], "closed-form limit of reduce_region_radius: %r" % (closed,)
    return dict(LA_CAP=_define(a, "LA_CAP", "lsd_async.inc"), LA_BCAP=_define(a, "LA_BCAP", "lsd_async.inc"),
                LSD_RING=_define(l, "LSD_RING", "lsd.hip"), REDUCE_CLOSED=int(closed[0][0]))


def saw(v):
    """uint8(v mod 256) of a real-valued ramp"""
    return (np.floor(v).astype(np.int64) % 256).astype(np.uint8)


def _xy(w, h):
    y, x = np.mgrid[0:h, 0:w]
    return x.astype(np.float64), y.astype(np.float64)


def _holes(g, frac, patch, seed):
    """overwrite about `frac` of the area with flat patch x patch squares at positions of RandomState(seed); a patch takes the grey of
    its top-left pixel, so it is a hole in the strip (no gradient inside) without a strong edge around it"""
    g = g.copy(); h, w = g.shape
    rng = np.random.RandomState(seed)
    for _ in range(int(frac * w * h / (patch * patch))):
        x0 = int(rng.randint(0, w - patch)); y0 = int(rng.randint(0, h - patch))
        g[y0:y0 + patch, x0:x0 + patch] = g[y0, x0]
    return g


def ramp_v(w=W, h=H):
    x, y = _xy(w, h)
    return saw(6 * x)


def ramp_h_down(w=W_BIG, h=H_BIG):
    x, y = _xy(w, h)
    return saw(-6 * y)


def shallow(w=W, h=H):
    x, y = _xy(w, h)
    return saw(6 * (x * np.cos(0.3) + y * np.sin(0.3)))


def chevron(deg, w=W, h=H):
    x, y = _xy(w, h)
    return saw(6 * (x + np.tan(np.deg2rad(deg)) * np.abs(y - h / 2)))


def wavy(w=W, h=H):
    x, y = _xy(w, h)
    return saw(6 * (x + 12 * np.sin(2 * np.pi * y / 300)))


def cone(w=W, h=H):
    x, y = _xy(w, h)
    return saw(6 * np.hypot(x - w / 2, y - h / 2))


def holes25(w=W, h=H):
    return _holes(ramp_v(w, h), 0.25, 5, 2)


def holes_diag(w=W, h=H):
    x, y = _xy(w, h)
    return _holes(saw(4.3 * (x + y)), 0.15, 4, 3)


# name -> (generator, the paths the image is there for); tests/test_lsd_crafted.py turns every path into an inequality on the counters
CASES = {
    "ramp_v":      (ramp_v,                 ("region_gt_la_cap",)),
    "ramp_h_down": (ramp_h_down,            ("region_gt_la_cap", "wrap")),
    "shallow":     (shallow,                ("region_gt_la_cap", "reduce_gt_closed")),
    "chevron10":   (lambda: chevron(10.0),  ("region_gt_la_cap", "refine_gt_half_la_cap")),
    "chevron18":   (lambda: chevron(18.0),  ("tau_le_0",)),
    "wavy":        (wavy,                   ("region_gt_la_cap",)),
    "cone":        (cone,                   ()),                       # many refinements and reduce rounds of mid-size regions, the longest pending front
    "holes25":     (holes25,                ("reduce_gt_closed",)),
    "holes_diag":  (holes_diag,             ("reduce_gt_closed", "segments_gt_200")),
}


# The growing forms and the knobs that force each onto a small batch (the ones tests/test_lsd_gpu.py uses):
# id -> (environment, launch_report()["lsd"] fields it must show).  tests/test_lsd_crafted.py checks the selection without a device.
_ONE_WAVE = {"HVO_LSD_ASYNC": "0", "HVO_LSD_LAT": "0"}
FORMS = {
    "grow":         (dict(_ONE_WAVE, HVO_LSD_DENSE="0"), dict(grow="grow", async_w=0, compact=0)),
    "dense":        (dict(_ONE_WAVE, HVO_LSD_DENSE="1"), dict(grow="dense", async_w=0, compact=0)),
    "lat":          ({"HVO_LSD_ASYNC": "0"}, dict(grow="lat", async_w=0, compact=0)),
    "grow_c":       ({"HVO_LSD_COMPACT": "1", "HVO_LSD_DENSE": "0"}, dict(grow="grow_c", compact=1)),
    "dense_c":      ({"HVO_LSD_COMPACT": "1", "HVO_LSD_DENSE": "1"}, dict(grow="dense_c", compact=1)),
    "grow_c_small": ({"HVO_LSD_COMPACT": "1", "HVO_LSD_DENSE": "0", "HVO_LSD_COMPACT_FRAC": "0.01"}, dict(grow="grow_c", compact=1)),   # the pool regrows
}
for _w in (3, 8, 32):
    for _e in (0, 1):
        FORMS["async%d_early%d" % (_w, _e)] = ({"HVO_LSD_ASYNC": str(_w), "HVO_LSD_ASYNC_EARLY": str(_e)},
                                               dict(grow="async", async_w=_w, async_early=_e, async_fallback=1))


def make(name):
    g = np.ascontiguousarray(CASES[name][0]())
    assert g.dtype == np.uint8 and g.ndim == 2
    return g


def by_size():
    """{(h, w): [names]} -- frames of one size go into one batch"""
    out = {}
    for name in CASES:
        out.setdefault(make(name).shape, []).append(name)
    return out
