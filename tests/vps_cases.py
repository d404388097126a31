"""Case builders for tests/test_vps_edges_gpu.py and a numpy restatement of the pair stage of the vanishing-point path (k_vp_lines + k_vp_pairs of
csrc/vps.hip = orc_vp_line_params + the pair loop of orc_vp_sphere_grid in oracle/vps.c).

The restatement is CPU-only test infrastructure.  It exists to state preconditions -- how many pairs each sphere cell holds (which of
k_vp_grid's three ordering paths a cell takes) and how far every pair lies from a cell border (whether the device's acos / atan2 may
legitimately choose the neighbouring cell) -- and it is validated against the oracle's smoothed grid, never against the device."""
import numpy as np

PI = 3.1415926535897932384626433832795
ACC = 1.0 / 180.0 * PI
TOL = 60.0 / 180.0 * PI
LA, LO = 90, 360
VP_BIG, VP_BIGMAX, VP_MAX_LINES, VP_GROUPS = 48, 2048, 1024, 105
K_DEFAULT = (535.4, 539.2, 320.1, 247.6)
K_512 = (512.0, 512.0, 320.0, 240.0)
BORDER_MARGIN = 1e-9                                                  # in cells (= degrees)


def keylines(orc, sx, sy, ex, ey):
    kl = np.zeros(len(sx), orc.KEYLINE_DT)
    kl["sx"], kl["sy"], kl["ex"], kl["ey"] = sx, sy, ex, ey
    return kl


def random_segments(orc, n, seed, box=(20.0, 620.0, 20.0, 460.0), half=(10.0, 40.0)):
    """n segments: midpoints uniform in box = (x0, x1, y0, y1), direction uniform, half-length uniform in `half`"""
    rng = np.random.RandomState(seed)
    mx = rng.uniform(box[0], box[1], n); my = rng.uniform(box[2], box[3], n)
    a = rng.uniform(0.0, np.pi, n); L = rng.uniform(half[0], half[1], n)
    dx, dy = np.cos(a) * L, np.sin(a) * L
    return keylines(orc, mx - dx, my - dy, mx + dx, my + dy)


def pencil(orc, n, seed, vp=(900.0, 120.0)):
    """n segments that all point at one vanishing point: every pair meets in the same few cells"""
    rng = np.random.RandomState(seed)
    mx = rng.uniform(40, 600, n); my = rng.uniform(40, 440, n)
    dx, dy = vp[0] - mx, vp[1] - my
    s = rng.uniform(15, 50, n) / np.hypot(dx, dy)
    return keylines(orc, mx - dx * s, my - dy * s, mx + dx * s, my + dy * s)


def tiled_rectangles(w=1280, h=960, pitch=40, seed=7):
    """a light image tiled with small dark rectangles, one per pitch x pitch tile, each tilted by its own angle: four short line
    segments per tile, thousands per frame"""
    rng = np.random.RandomState(seed)
    ty, tx = (h + pitch - 1) // pitch, (w + pitch - 1) // pitch
    ang = rng.uniform(0.0, np.pi, (ty, tx)); hu = rng.uniform(11.0, 15.0, (ty, tx)); hv = rng.uniform(6.0, 9.0, (ty, tx))
    yy, xx = np.mgrid[0:h, 0:w]
    iy, ix = yy // pitch, xx // pitch
    ly = yy - (iy * pitch + pitch / 2.0); lx = xx - (ix * pitch + pitch / 2.0)
    c, s = np.cos(ang[iy, ix]), np.sin(ang[iy, ix])
    u = lx * c + ly * s; v = -lx * s + ly * c
    # a two-pixel ramp at the sides keeps the gradient direction of an edge the same along it
    d = np.minimum(hu[iy, ix] - np.abs(u), hv[iy, ix] - np.abs(v))
    return (200.0 - 160.0 * np.clip(d / 2.0 + 0.5, 0.0, 1.0)).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------ the restatement
def pair_cells(kl, K=K_DEFAULT):
    """key lines, intrinsics -> dict over the pairs (i < j) in np.triu_indices order (= the reference's loop order = the rank p of
    k_vp_pairs): cell (-1: the pair contributes nothing), val, finite (pt[2] != 0), la_f / lo_f (latitude / acc, longitude / acc)"""
    fx, cx, cy = (float(np.float32(K[0])), float(np.float32(K[2])), float(np.float32(K[3])))      # Frame::fx, cx, cy are floats
    sx, sy, ex, ey = (kl[k].astype(np.float32) for k in ("sx", "sy", "ex", "ey"))
    dx = (ex - sx).astype(np.float64); dy = (ey - sy).astype(np.float64)          # Point2f differences are float subtractions
    sx, sy, ex, ey = (a.astype(np.float64) for a in (sx, sy, ex, ey))
    para = np.stack([sy - ey, ex - sx, sx * ey - sy * ex], axis=1)                # (sx, sy, 1) x (ex, ey, 1)
    length = np.sqrt(dx * dx + dy * dy)
    ori = np.arctan2(dy, dx); ori = np.where(ori < 0, ori + PI, ori)
    n = len(kl)
    i, j = np.triu_indices(n, 1)
    a, b = para[i], para[j]
    p0 = a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1]; p1 = a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2]; p2 = a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]
    finite = p2 != 0
    with np.errstate(divide="ignore", invalid="ignore"):
        X = p0 / p2 - cx; Y = p1 / p2 - cy
        N = np.sqrt(X * X + Y * Y + fx * fx)
        la_f = np.arccos(fx / N) / ACC; lo_f = (np.arctan2(X, Y) + PI) / ACC
    la_f = np.where(finite, la_f, 0.5); lo_f = np.where(finite, lo_f, 0.5)
    la = np.minimum(la_f.astype(np.int64), LA - 1); lo = np.minimum(lo_f.astype(np.int64), LO - 1)       # the two clamps
    dev = np.abs(ori[i] - ori[j]); dev = np.minimum(PI - dev, dev)
    ok = finite & ~(dev > TOL)
    cell = np.where(ok, la * LO + lo, -1)
    val = np.where(ok, np.sqrt(length[i] * length[j]) * (np.sin(2.0 * dev) + 0.2), 0.0)
    return dict(cell=cell, val=val, finite=finite, la_f=la_f, lo_f=lo_f, n=n)


def raw_grid(pc):
    """the unsmoothed sums, every cell's pairs added in pair order (np.bincount adds in index order)"""
    m = pc["cell"] >= 0
    return np.bincount(pc["cell"][m], weights=pc["val"][m], minlength=LA * LO).reshape(LA, LO)


def smooth(raw):
    """src/Frame.cc:629-649: new = old + (3 x 3 sum) / 9 in the interior, 0 on the border rows and columns"""
    g = np.zeros_like(raw)
    tot = np.zeros((LA - 2, LO - 2))
    for m in range(3):
        for q in range(3):
            tot += raw[m: m + LA - 2, q: q + LO - 2]
    g[1:-1, 1:-1] = raw[1:-1, 1:-1] + tot / 9
    return g


def counts(pc):
    """pairs per cell (90 x 360)"""
    return np.bincount(pc["cell"][pc["cell"] >= 0], minlength=LA * LO).reshape(LA, LO)


def border_distance(pc):
    """the smallest distance, in cells, of any finite pair's latitude / acc or longitude / acc from a whole number"""
    f = pc["finite"]
    if not f.any():
        return np.inf
    return float(min(np.abs(pc["la_f"][f] - np.rint(pc["la_f"][f])).min(), np.abs(pc["lo_f"][f] - np.rint(pc["lo_f"][f])).min()))


def lone_lane_steps(cnt, bigmax=VP_BIGMAX):
    """k_vp_grid's serial work: the expected moves of the owner lanes' insertion sorts (count^2 / 4 per cell) over the cells a lone lane
    orders -- every cell of at most VP_BIG pairs, and in the worst case the LARGEST cells beyond the table's bigmax entries"""
    c = np.sort(cnt.ravel())[::-1].astype(np.float64)
    big = c[c > VP_BIG]; small = c[c <= VP_BIG]
    return float((small ** 2 / 4).sum() + (big[: max(len(big) - bigmax, 0)] ** 2 / 4).sum())


# ------------------------------------------------------------------------------------------------------ the cases
SWEEP_N = (2, 3, 4, 63, 64, 65, 255, 256, 257, 1023, 1024)
SWEEP_SEED = {n: 100 + n for n in SWEEP_N}
OVERFLOW_SEED = 3
SEED_FIXUP = (0x9E3779B9, (0x9E3779B9 * VP_GROUPS) & 0xFFFFFFFF, 0)
SEED_FIXUP_SCENE = (23, 362, 77)
RESIDENT_NFEAT = 1280
RESIDENT_W, RESIDENT_H = 1280, 960


def overflow_lines(orc, n=1024, seed=OVERFLOW_SEED):
    """midpoints in the 80 x 80 px box x 280-360, y 210-290, half-lengths 10-40 px: the intersections crowd the cells round the principal point"""
    rng = np.random.RandomState(seed)
    mx = rng.uniform(280, 360, n); my = rng.uniform(210, 290, n)
    a = rng.uniform(0, np.pi, n); L = rng.uniform(10, 40, n)
    dx, dy = np.cos(a) * L, np.sin(a) * L
    return keylines(orc, mx - dx, my - dy, mx + dx, my + dy)


def boundary_lines(orc):
    """450 random segments in a small box (cells of every small population, 48 and 49 among them) and a pencil of 60 (1770 pairs in a few cells)"""
    return np.concatenate([overflow_lines(orc, 450, 3), pencil(orc, 60, 9)])


def redraw_lines(orc, k=40, oblique=1):
    """k exactly horizontal lines on integer coordinates (every pair of them has pt[2] == 0 exactly: integer products below 2^53) and
    `oblique` lines that cross them"""
    i = np.arange(k, dtype=np.float64)
    kl = keylines(orc, 10.0 + i, 40.0 + 10 * i, 200.0 + 3 * i, 40.0 + 10 * i)
    ob = keylines(orc, [301.25, 420.5][:oblique], [33.5, 60.25][:oblique], [380.75, 350.25][:oblique], [101.25, 150.5][:oblique])    # within 60 degrees of them
    return np.concatenate([kl, ob])


def gave_up(orc, kl, seed, K=K_DEFAULT):
    """per hypothesis group: did it use up its redraws (360 zero hypotheses)?"""
    return np.array([not orc.vp_hypothesis(kl, seed, i * 360, fx=K[0], cx=K[2], cy=K[3]).any() for i in range(VP_GROUPS)])


def redraws_of(kl, seed, i):
    """the draws group i makes before a pair with pt[2] != 0 comes up (65: gave up) -- the xorshift32 rule of oracle/vps.c restated on integers"""
    n = len(kl)
    sx, sy, ex, ey = (kl[k].astype(np.float64) for k in ("sx", "sy", "ex", "ey"))
    para = np.stack([sy - ey, ex - sx, sx * ey - sy * ex], axis=1)
    rs = (seed ^ ((0x9E3779B9 * (i + 1)) & 0xFFFFFFFF)) & 0xFFFFFFFF
    if rs == 0:
        rs = 0x6D2B79F5

    def xs():
        nonlocal rs
        x = rs; x ^= (x << 13) & 0xFFFFFFFF; x ^= x >> 17; x ^= (x << 5) & 0xFFFFFFFF; rs = x
        return (x & 0x7FFFFFFF) % n
    for tries in range(64):
        a = xs(); b = xs()
        while b == a:
            b = xs()
        if para[a][0] * para[b][1] - para[a][1] * para[b][0] != 0:
            return tries + 1
    return 65


def host_case(orc, kl, seed, K=K_DEFAULT, th=None, random=True):
    ref = orc.vanishing_points(kl, seed=seed, th_angle=th, fx=K[0], fy=K[1], cx=K[2], cy=K[3], want_scores=True)
    pc = pair_cells(kl, K)
    c = dict(kl=kl, seed=seed, K=K, th=th, ref=ref, cnt=counts(pc), border=border_distance(pc), random=random)
    # the restatement against the oracle: its raw sums through the interior-3x3 rule are the oracle's grid
    assert np.allclose(smooth(raw_grid(pc)), ref["grid"], rtol=1e-12, atol=1e-12), np.abs(smooth(raw_grid(pc)) - ref["grid"]).max()
    if random:
        assert c["border"] > BORDER_MARGIN, c["border"]
    return c


_CACHE = {}


def host_cases(orc):
    """name -> case; every precondition of the case list is asserted here, on the CPU"""
    if "host" in _CACHE:
        return _CACHE["host"]
    S = {}
    # overflow_1024: more cells above VP_BIG pairs than the table holds
    c = S["overflow_1024"] = host_case(orc, overflow_lines(orc), 7)
    assert (c["cnt"] > VP_BIG).sum() > VP_BIGMAX, (c["cnt"] > VP_BIG).sum()
    assert (c["cnt"] == VP_BIG).any() and (c["cnt"] == VP_BIG + 1).any()
    # boundary_48_49: both sides of the threshold, and a cell the workgroup needs a second trip for
    c = S["boundary_48_49"] = host_case(orc, boundary_lines(orc), 5)
    assert (c["cnt"] == VP_BIG).any() and (c["cnt"] == VP_BIG + 1).any() and c["cnt"].max() > 1024 and (c["cnt"] > VP_BIG).sum() <= VP_BIGMAX
    # count_sweep
    for n in SWEEP_N:
        S["sweep_%d" % n] = host_case(orc, random_segments(orc, n, SWEEP_SEED[n]), 3 + n)
    # redraw_mixed: some groups redraw and succeed, some give up
    kl = redraw_lines(orc); seed = 11
    c = S["redraw_40_1"] = host_case(orc, kl, seed)
    g = gave_up(orc, kl, seed); tries = np.array([redraws_of(kl, seed, i) for i in range(VP_GROUPS)])
    assert g.any() and not g.all() and np.array_equal(g, tries == 65), (g.sum(), tries)
    assert ((tries > 1) & (tries < 65)).sum() >= 20 and c["ref"]["score"] > 0
    assert 1 < tries[c["ref"]["best"] // 360] < 65                   # the best hypothesis comes from a group that redrew: the stream's use shows in the result
    c["gave_up"] = g
    i = np.arange(2, dtype=np.float64)
    kl = np.concatenate([keylines(orc, 10.0 + i, 40.0 + 25 * i, 200.0 + 3 * i, 40.0 + 25 * i), redraw_lines(orc, 1, 1)[1:]]); seed = 5
    c = S["redraw_3"] = host_case(orc, kl, seed)
    g = gave_up(orc, kl, seed); tries = np.array([redraws_of(kl, seed, i) for i in range(VP_GROUPS)])
    assert not g.all() and np.array_equal(g, tries == 65) and ((tries > 1) & (tries < 65)).sum() >= 20, tries
    assert 1 < tries[c["ref"]["best"] // 360] < 65, tries[c["ref"]["best"] // 360]
    c["gave_up"] = g
    # lo_clamp: an intersection exactly above the principal point.  X = +0 and Y < 0 exactly (integer coordinates), atan2(+0, Y < 0) is pi in
    # every IEEE libm, so longitude / acc = 2 pi / acc in every libm: the cell does not depend on the libm, whatever its distance from 360
    kl = keylines(orc, [320, 270], [300, 50], [320, 300], [400, 80])
    c = S["lo_clamp"] = host_case(orc, kl, 3, K=K_512, random=False)
    assert c["cnt"][15, 359] == 1 and c["cnt"].sum() == 1
    assert sorted(zip(*np.nonzero(c["ref"]["grid"]))) == [(14, 358), (15, 358), (16, 358)] and c["ref"]["score"] == 0 and c["ref"]["best"] == 0
    # its mirror image below the principal point: X = +0, Y > 0, atan2 = +0 exactly, longitude = pi exactly
    kl = keylines(orc, [320, 270], [0, 450], [320, 300], [100, 420])
    c = S["lo_mirror"] = host_case(orc, kl, 3, K=K_512, random=False)
    nz = np.nonzero(c["ref"]["grid"])
    assert c["cnt"][17, 180] == 1 and sorted(set(nz[0])) == [16, 17, 18] and sorted(set(nz[1])) == [179, 180, 181] and abs(c["ref"]["score"] - 86.85) < 0.01
    # no_score: two lines that cross exactly at the principal point, 90 degrees apart (the 60-degree gate drops the pair)
    kl = keylines(orc, [220, 320], [240, 100], [300, 320], [240, 200])
    c = S["no_score"] = host_case(orc, kl, 3, K=K_512, random=False)
    r = c["ref"]
    assert not r["grid"].any() and r["score"] == 0 and r["best"] == 0 and np.isfinite(r["vps"]).all() and r["vps"].any() and r["vp_idx"].tolist() == [0, 0]
    # seed_fixup: seeds that zero the xorshift state of group 0 / group 104
    # (only the best hypothesis leaves the device: each scene is one whose best hypothesis the oracle finds IN the fixed-up group, well ahead
    # of every other group's, so that a different stream for that group changes the result)
    for s, scene, grp in zip(SEED_FIXUP, SEED_FIXUP_SCENE, (0, VP_GROUPS - 1, None)):
        c = S["seed_%08x" % s] = host_case(orc, random_segments(orc, 40, scene), s)
        if grp is not None:
            assert (s ^ ((0x9E3779B9 * (grp + 1)) & 0xFFFFFFFF)) == 0
            other = c["ref"]["scores"].copy(); other[grp * 360: (grp + 1) * 360] = 0
            assert c["ref"]["best"] // 360 == grp and c["ref"]["score"] > other.max() + 10, (c["ref"]["best"], c["ref"]["score"], other.max())
    # line2vps_edges: a zero-length line (NaN direction) in a small scene, at three angles
    kl = np.concatenate([random_segments(orc, 24, 21), keylines(orc, [50], [50], [50], [50])])
    for name, th in (("default", None), ("pi", PI), ("1e-12", 1e-12)):
        S["l2v_" + name] = host_case(orc, kl, 9, th=th)
    assert S["l2v_default"]["ref"]["vp_idx"][-1] == 3 and S["l2v_pi"]["ref"]["vp_idx"][-1] == 3
    assert (S["l2v_pi"]["ref"]["vp_idx"][:-1] < 3).all() and (S["l2v_1e-12"]["ref"]["vp_idx"] == 3).all()
    assert 0 < (S["l2v_default"]["ref"]["vp_idx"] < 3).sum() < 24
    _CACHE["host"] = S
    return S


def resident_case(orc):
    """one 1280 x 960 frame of tiled tilted rectangles: the oracle extracts more key lines than the host form's 1024"""
    if "res" in _CACHE:
        return _CACHE["res"]
    g = tiled_rectangles(RESIDENT_W, RESIDENT_H)
    kl = orc.line_extract(g, nfeatures=RESIDENT_NFEAT)[0]
    assert VP_MAX_LINES < len(kl) <= RESIDENT_NFEAT, len(kl)
    pc = pair_cells(kl)
    cnt = counts(pc)
    c = dict(gray=g, kl=kl, cnt=cnt, steps=lone_lane_steps(cnt), border=border_distance(pc))
    ref = orc.vanishing_points(kl, seed=9)
    assert np.allclose(smooth(raw_grid(pc)), ref["grid"], rtol=1e-12, atol=1e-12)
    _CACHE["res"] = c
    return c
