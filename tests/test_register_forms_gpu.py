"""The two kernels whose register allocation is pinned (k_orb_level at 80, k_peac_cluster_slots at 168: DESIGN 4, "The register file as
a budget") against their independent formulations and the CPU oracle, byte for byte.

ORB: the fused per-level pass against the separate resize / FAST / blur kernels (HVO_ORB_FUSED=0) and the oracle, on the geometries
and crafted images at which the fused kernel takes its other paths (candidate-list overflow, NMS ties, border fix-up, margin tiles,
the minThFAST fallback, an XCD slot without a frame).  AHC: the slot form against the lending form (HVO_PEAC_SLOTS=0) and the
oracle on idle and partly filled waves, mixed waves, a compacted pool and a small depth geometry."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


# ----------------------------------------------------------------------------------------------------------------------------
# ORB
# ----------------------------------------------------------------------------------------------------------------------------
KP_FIELDS = ("x", "y", "size", "angle", "response", "octave", "class_id")


def same_orb(tag, kp_a, d_a, kp_b, d_b):
    assert len(kp_a) == len(kp_b), (tag, len(kp_a), len(kp_b))
    for f in KP_FIELDS:
        a, b = np.ascontiguousarray(kp_a[f]), np.ascontiguousarray(kp_b[f])
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (tag, f, int((a != b).sum()))
    assert d_a.tobytes() == d_b.tobytes(), (tag, "descriptors")


def _orb_plan(hvo, ctx):
    out = (ctypes.c_int * 4)()
    L = hvo.lib(); L.hvo_debug_orb_plan.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    assert L.hvo_debug_orb_plan(ctx.h, out) == 0
    return list(out)


def orb_three_ways(hvo, orc, monkeypatch, g, min_keys):
    """one image: fused, separate kernels, oracle"""
    got = {}
    for fused in ("1", "0"):
        monkeypatch.setenv("HVO_ORB_FUSED", fused)
        ctx = hvo.Context()
        try:
            got[fused] = ctx.extract_orb(g)
            assert _orb_plan(hvo, ctx)[0] == int(fused)        # the path that was asked for is the one that ran
        finally:
            ctx.close()
    kp_o, d_o = orc.Orb().extract(g)
    print("keys fused %d separate %d oracle %d" % (len(got["1"][0]), len(got["0"][0]), len(kp_o)))
    assert len(kp_o) >= min_keys, len(kp_o)
    same_orb("fused vs separate", got["1"][0], got["1"][1], got["0"][0], got["0"][1])
    same_orb("fused vs oracle", got["1"][0], got["1"][1], kp_o, d_o)


@pytest.mark.parametrize("hh,ww", [(397, 501), (479, 638), (479, 639)])
def test_orb_level_odd_widths(hvo, orc, synth, monkeypatch, hh, ww):
    """the smallest geometry the fused pass takes (397 x 501, w % 4 = 1) and one width each for w % 4 = 2 and 3: the last owned
    dword of a row is partly outside the level (right border fix-up, the (s + 32768) >> 16 rounding of the last w % 4 columns)"""
    big = synth.make_gray("std", 11, 704, 480)
    orb_three_ways(hvo, orc, monkeypatch, np.ascontiguousarray(big[:hh, :ww]), 20)


def noise_image():
    return np.random.default_rng(0xFA57).integers(0, 256, (480, 640), dtype=np.uint8)


def checker_image():
    y, x = np.mgrid[0:480, 0:640]
    return np.where(((x >> 2) + (y >> 2)) & 1, 200, 60).astype(np.uint8)


def sparks_image():
    """a flat image with single bright pixels: on a lattice whose pitch (13 x 11) is coprime to every tile size, so that some fall on
    the first and last column / row a tile owns and in its halo; along all four borders inside the 19-pixel margin the FAST grid does
    not cover (blur / resize input only, REFLECT_101 sources) and just inside it; and weak ones only (above minThFAST, below
    iniThFAST) in the left half of every other band of rows, so that cells with only weak corners lie beside cells with strong ones"""
    g = np.full((480, 640), 90, np.uint8)
    for y in range(20, 460, 11):
        for x in range(20, 620, 13):
            weak = x < 320 and (y // 60) % 2 == 0
            g[y, x + (y // 11) % 3] = 100 if weak else 190
    for k, p in enumerate((0, 1, 2, 3, 5, 15, 16, 17, 18, 19)):
        for q in range(24 + 3 * k, 440, 37):
            g[q, p] = 200; g[q + 5, 639 - p] = 200                 # left / right margin
            g[p, q + 100] = 200; g[479 - p, q + 105] = 200         # top / bottom margin
    return g


@pytest.mark.parametrize("make,min_keys", [(noise_image, 900), (checker_image, 0), (sparks_image, 100)], ids=["noise", "checker4", "sparks"])
def test_orb_level_crafted_images(hvo, orc, monkeypatch, make, min_keys):
    """uniform noise: more than half of a cell's pixels pass the pair test, the candidate list of every tile overflows and the
    full-raster score / NMS / emission path runs; a 4-pixel checkerboard: every corner's score ties with neighbours (strict NMS);
    single bright pixels: see sparks_image"""
    orb_three_ways(hvo, orc, monkeypatch, make(), min_keys)


def test_orb_level_batch_with_empty_xcd_slots(hvo, orc, synth, monkeypatch):
    """three frames under max_batch 4: the grid is rounded up to eight frame slots (one per XCD), five of them have no frame"""
    gray = np.stack([synth.make_gray("std", 0x5EED6000), sparks_image(), synth.make_gray("lowtex", 0x5EED0001)])
    res = {}
    for fused in ("1", "0"):
        monkeypatch.setenv("HVO_ORB_FUSED", fused)
        ctx = hvo.Context(max_batch=4)
        try:
            ctx.batch_upload(gray, np.zeros((3, 480, 640), np.uint16))
            ctx.batch_run(hvo.STAGE_ORB)
            res[fused] = ctx.batch_download(hvo.STAGE_ORB)
            assert _orb_plan(hvo, ctx)[0] == int(fused)
        finally:
            ctx.close()
    o = orc.Orb()
    for b in range(3):
        kp_o, d_o = o.extract(gray[b])
        assert res["1"][b]["status"] == 0 and res["0"][b]["status"] == 0
        same_orb("frame %d fused vs separate" % b, res["1"][b]["kp"], res["1"][b]["desc"], res["0"][b]["kp"], res["0"][b]["desc"])
        same_orb("frame %d fused vs oracle" % b, res["1"][b]["kp"], res["1"][b]["desc"], kp_o, d_o)


# ----------------------------------------------------------------------------------------------------------------------------
# AHC
# ----------------------------------------------------------------------------------------------------------------------------
PL_FIELDS = ("n_points", "rid", "normal", "center", "mse")


def same_planes(tag, lab_a, pl_a, lab_b, pl_b):
    assert len(pl_a) == len(pl_b), (tag, len(pl_a), len(pl_b))
    for f in PL_FIELDS:
        a, b = np.ascontiguousarray(pl_a[f]), np.ascontiguousarray(pl_b[f])
        assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), (tag, f)
    assert lab_a.dtype == lab_b.dtype and np.array_equal(lab_a, lab_b), (tag, int((lab_a != lab_b).sum()))


def plane_scene(seed, nplanes, w=640, h=480, K=(535.4, 539.2, 320.1, 247.6), q=1):
    """piecewise-planar depth as in tools/soak_planes.py: nplanes exact planes on a grid of rectangles, quantised to q sensor units
    (coarse steps = many equal depths = ties); no noise"""
    rng = np.random.default_rng(seed)
    u, v = np.meshgrid(np.arange(w), np.arange(h))
    rx, ry = (u - K[2]) / K[0], (v - K[3]) / K[1]
    nx = int(np.ceil(np.sqrt(nplanes * 4 / 3))); ny = int(np.ceil(nplanes / nx))
    region = np.minimum((v * ny // h) * nx + (u * nx // w), nplanes - 1)
    z = np.zeros((h, w))
    for k in range(nplanes):
        n = rng.normal(0, 1, 3); n[2] = abs(n[2]) + 1.0; n /= np.linalg.norm(n)
        zk = rng.uniform(0.8, 4.5) / (n[0] * rx + n[1] * ry + n[2])
        z[region == k] = zk[region == k]
    d = np.clip(np.round(z * 5000.0), 0, 65535)
    return np.clip(np.round(d / q) * q, 0, 65535).astype(np.uint16)


def ahc_three_ways(hvo, orc, monkeypatch, depth, poolcap=None, K=None):
    """a batch through the four-frames-per-wave AHC: slot form, lending form, oracle"""
    monkeypatch.setenv("HVO_PEAC_GL", "16")
    if poolcap: monkeypatch.setenv("HVO_PEAC_POOLCAP", str(poolcap))
    n, h, w = depth.shape
    kw = dict(fx=K["fx"], fy=K["fy"], cx=K["cx"], cy=K["cy"]) if K else {}
    res, rep = {}, {}
    for slots in ("1", "0"):
        monkeypatch.setenv("HVO_PEAC_SLOTS", slots)
        ctx = hvo.Context(max_batch=n, **kw)
        try:
            ctx.batch_upload(np.zeros((n, h, w), np.uint8), depth)
            ctx.batch_run(hvo.STAGE_PLANES)
            res[slots] = ctx.batch_download(hvo.STAGE_PLANES)
            rep[slots] = ctx.launch_report()["peac"]
        finally:
            ctx.close()
    # two different kernels were compared: the slot form and the lending form, each with the pool that was asked for
    assert rep["1"]["cluster"] == "slots" and rep["0"]["cluster"] == "c16_lend", (rep["1"], rep["0"])
    for r in rep.values():
        assert (r["group"], r["cluster_wgs"], r["poolcap"], r["n"]) == (16, (n + 3) // 4, int(poolcap or 0), n), r
    okw = {k: np.float32(v) for k, v in kw.items()}
    counts = []
    for b in range(n):
        lo, po = orc.peac(depth[b], **okw)
        counts.append(len(po))
        assert res["1"][b]["status"] == 0 and res["0"][b]["status"] == 0
        same_planes("frame %d slots vs lending" % b, res["1"][b]["labels"], res["1"][b]["planes"], res["0"][b]["labels"], res["0"][b]["planes"])
        same_planes("frame %d slots vs oracle" % b, res["1"][b]["labels"], res["1"][b]["planes"], lo, po)
    print("planes per frame", counts)
    return counts


@pytest.fixture(scope="module")
def ahc_frames(synth):
    """no valid block / one exact plane / 35 exact planes in coarse depth steps (ties everywhere) / two textured rooms"""
    return np.stack([np.zeros((480, 640), np.uint16), plane_scene(1, 1), plane_scene(2, 35, q=25), synth.make_depth(0x5EED1000), synth.make_depth(77)])


@pytest.mark.parametrize("n", [1, 3, 4, 5])
def test_slot_ahc_batches(hvo, orc, monkeypatch, ahc_frames, n):
    """1, 3, 4 and 5 frames at 640 x 480: a wave with three idle groups, with one, a full wave, a full wave and a nearly idle one.  The
    first wave mixes a frame with no valid block, a single-plane frame and a tie-heavy many-plane frame"""
    counts = ahc_three_ways(hvo, orc, monkeypatch, ahc_frames[:n])
    assert counts[0] == 0
    if n >= 3: assert counts[1] == 1 and counts[2] >= 12


def test_slot_ahc_pool_compaction(hvo, orc, monkeypatch, ahc_frames):
    """a list pool of 22 000 entries (the smallest the launch accepts is 7 x 3072): compacted inside the merge loop, more than once"""
    ahc_three_ways(hvo, orc, monkeypatch, ahc_frames[1:5], poolcap=22000)


def test_slot_ahc_small_depth_geometry(hvo, orc, synth, monkeypatch):
    """200 x 160 depth: 320 blocks, a queue of two 256-slot pages, five frames"""
    w, h = 200, 160
    K = synth.intrinsics(w, h)
    Kt = (K["fx"], K["fy"], K["cx"], K["cy"])
    depth = np.stack([synth.make_depth(0x5EED6100, w, h), plane_scene(3, 1, w, h, Kt), np.zeros((h, w), np.uint16), plane_scene(4, 6, w, h, Kt, q=5), synth.make_depth(0x5EED6101, w, h)])
    counts = ahc_three_ways(hvo, orc, monkeypatch, depth, K=K)
    assert counts[1] >= 1 and counts[2] == 0 and counts[3] >= 2
