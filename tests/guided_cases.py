"""Hand-written inputs for the guided ORB search (csrc/match.hip: k_search_by_projection + k_sbp_epilogue), plain numpy.

No ORB extraction and no GPU: key points are KEYPOINT_DT records written field by field, descriptors are a base descriptor with a chosen
number of bits flipped (so the Hamming distance to the base IS that number).  Every builder
  * asserts, on its inputs, the property that puts the case on the path it is meant for (`Case.props` keeps the figures),
  * states what it expects -- literal arrays, or a closed formula such as "query i takes the feature of rank i" -- in `Case.expect[mode]`
    = (n_matches, match_idx, match_dist); match_dist is only meaningful where match_idx >= 0.
tests/test_guided_edges_gpu.py runs the cases through the CPU oracle (oracle/match.c) and through the device entry points.

Modes: "last" = SearchByProjection(Cur, Last) without the rotation check, "rot" = the same with it, "map" = SearchByProjection(F, MapPoints).
`Case.tracked` (level, view_cos, th), when present, says that the map-mode windows are what the tracked entry point derives from those fields.
`Case.oracle_mask` marks the queries the oracle may see: a non-finite or huge coordinate makes its `(int)` conversion undefined in C.

model_search() is a second, sort-based statement of the search ("first free candidate in (distance, cellX, cellY, index) order") used as the
closed formula of the contention cases and to count, per query, how many ranked keys are still free when its turn comes."""
from types import SimpleNamespace as NS

import numpy as np

F = np.float32
COLS, ROWS = 64, 48                      # the frame grid
SBP_K, SBP_LCAP = 16, 512                # ranked keys per query, LDS list capacity of k_search_by_projection
MAX_Q, MAX_T = 16384, 65535
B0 = (0.0, 0.0, 640.0, 480.0)            # 10 x 10 px cells
B1 = (-11.5, -7.25, 651.75, 489.5)       # undistorted bounds with a negative minimum
BASE = np.random.default_rng(0xBA5E).integers(0, 256, 32, dtype=np.uint8)
SF = np.cumprod(np.concatenate([[F(1.0)], np.full(7, F(1.2), F)])).astype(F)     # mvScaleFactors of the default 8-level pyramid


def flip(k, start=0, base=BASE):
    """`base` with k distinct bits flipped (37 is coprime to 256): Hamming distance to base == k; k = 256 is the complement"""
    bits = np.unpackbits(base)
    bits[(start + 37 * np.arange(k)) % 256] ^= 1
    return np.packbits(bits)


def ham(a, b):
    return np.unpackbits(a[:, None, :] ^ b[None, :, :], axis=2).sum(axis=2).astype(np.int32)


def feats(kp_dt, x, y, dist, octave=0, angle=0.0, uright=-1.0, occ=0, desc=None):
    """train features; descriptor j = BASE with dist[j] bits flipped, starting at bit j (equal distances, different descriptors)"""
    n = len(x)
    kp = np.zeros(n, kp_dt)
    kp["x"] = np.asarray(x, F); kp["y"] = np.asarray(y, F); kp["size"] = 31; kp["octave"] = octave; kp["angle"] = angle; kp["class_id"] = -1
    if desc is None:
        desc = np.stack([flip(int(d), j) for j, d in enumerate(np.broadcast_to(dist, n))]) if n else np.zeros((0, 32), np.uint8)
    return NS(kp=kp, desc=np.ascontiguousarray(desc, np.uint8), uright=np.broadcast_to(F(uright), n).astype(F).copy(),
              occ=np.broadcast_to(np.uint8(occ), n).copy())


def queries(u, v, r, lo=0, hi=-1, ur=0.0, angle=0.0, blocks=1, desc=None):
    n = len(u)
    b = lambda a, dt: np.broadcast_to(np.asarray(a, dt), n).copy()
    return NS(desc=np.tile(BASE, (n, 1)) if desc is None else np.ascontiguousarray(desc, np.uint8), u=b(u, F), v=b(v, F), r=b(r, F),
              lo=b(lo, np.int32), hi=b(hi, np.int32), ur=b(ur, F), angle=b(angle, F), blocks=b(blocks, np.uint8))


def make(name, q, t, expect, bounds=B0, th_high=100, nn_ratio=0.8, oracle_mask=None, tracked=None, **props):
    nq = len(q.u)
    exp = {}
    for mode, (idx, dist) in expect.items():
        idx = np.asarray(idx, np.int32).reshape(nq); dist = np.broadcast_to(np.asarray(dist, np.int32), nq).copy()
        n = int((idx >= 0).sum())
        exp[mode] = (n, idx, dist)
    return NS(name=name, q=q, t=t, bounds=bounds, th_high=th_high, nn_ratio=nn_ratio, expect=exp, tracked=tracked, props=props,
              oracle_mask=np.ones(nq, bool) if oracle_mask is None else np.asarray(oracle_mask, bool))


# ------------------------------------------------------------------------------------------------ argument tuples of the entry points
def args_last(c, sel=slice(None)):
    q, t = c.q, c.t
    return (q.desc[sel], q.u[sel], q.v[sel], q.r[sel], q.lo[sel], q.hi[sel], q.ur[sel], q.angle[sel], q.blocks[sel], t.kp, t.uright, t.occ, t.desc, c.bounds)


def args_map(c, sel=slice(None)):
    q, t = c.q, c.t
    return (q.desc[sel], q.u[sel], q.v[sel], q.r[sel], q.lo[sel], q.hi[sel], q.ur[sel], q.blocks[sel], t.kp, t.uright, t.occ, t.desc, c.bounds)


def args_tracked(c):
    q, t, k = c.q, c.t, c.tracked
    return (q.desc, q.u, q.v, q.ur, k.level, k.view_cos, q.blocks, k.th, t.kp, t.uright, t.occ, t.desc, c.bounds)


# ------------------------------------------------------------------------------------------------ the grid, in the reference's float steps
def _round_away(v):
    v = v.astype(np.float64)                                     # exact; + 0.5 is exact in double for these magnitudes
    return (np.sign(v) * np.floor(np.abs(v) + 0.5)).astype(np.int64)


def cells(kp, bounds):
    """Frame::PosInGrid -> (cellX, cellY, in_grid)"""
    mnx, mny, mxx, mxy = (F(b) for b in bounds)
    invW = F(COLS) / (mxx - mnx); invH = F(ROWS) / (mxy - mny)
    px = _round_away((kp["x"] - mnx) * invW); py = _round_away((kp["y"] - mny) * invH)
    return px, py, (px >= 0) & (px < COLS) & (py >= 0) & (py < ROWS)


def window(c, i):
    """GetFeaturesInArea's cell range of query i -> (cx0, cx1, cy0, cy1) after clamping, or None when it returns early"""
    mnx, mny, mxx, mxy = (F(b) for b in c.bounds)
    invW = F(COLS) / (mxx - mnx); invH = F(ROWS) / (mxy - mny)
    x, y, r = c.q.u[i], c.q.v[i], c.q.r[i]
    cx0 = max(0, int(np.floor((x - mnx - r) * invW))); cx1 = min(COLS - 1, int(np.ceil((x - mnx + r) * invW)))
    cy0 = max(0, int(np.floor((y - mny - r) * invH))); cy1 = min(ROWS - 1, int(np.ceil((y - mny + r) * invH)))
    if cx0 >= COLS or cx1 < 0 or cy0 >= ROWS or cy1 < 0:
        return None
    return cx0, cx1, cy0, cy1


def candidates(c, i, grid=None):
    """mask of the train features that pass every test of query i but the occupancy"""
    px, py, _ = grid if grid is not None else cells(c.t.kp, c.bounds)
    w = window(c, i)
    if w is None:
        return np.zeros(len(c.t.kp), bool)
    kp, q = c.t.kp, c.q
    m = (px >= w[0]) & (px <= w[1]) & (py >= w[2]) & (py <= w[3])
    if q.lo[i] > 0 or q.hi[i] >= 0:
        m &= ~(kp["octave"] < q.lo[i])
        if q.hi[i] >= 0:
            m &= ~(kp["octave"] > q.hi[i])
    m &= (np.abs(kp["x"] - q.u[i]) < q.r[i]) & (np.abs(kp["y"] - q.v[i]) < q.r[i])
    m &= ~((c.t.uright > 0) & (np.abs(q.ur[i] - c.t.uright) > q.r[i]))
    return m


def model_search(c, mode):
    """sort-based statement of both searches (no rotation check) -> (n, idx, dist, stats); stats.ncand[i] = candidates not held by t_occ,
    stats.ranked_free[i] = how many of query i's SBP_K best keys are still free at its turn, stats.rescan[i] = the kernel's rescan condition"""
    grid = cells(c.t.kp, c.bounds); px, py, _ = grid
    nq, nt = len(c.q.u), len(c.t.kp)
    D = ham(c.q.desc, c.t.desc) if nq and nt else np.zeros((nq, nt), np.int32)
    occ0 = c.t.occ.astype(bool); occ = occ0.copy()
    idx = np.full(nq, -1, np.int32); dist = np.full(nq, 256, np.int32)
    ncand = np.zeros(nq, int); ranked_free = np.zeros(nq, int); rescan = np.zeros(nq, bool)
    for i in range(nq):
        if not c.oracle_mask[i]:
            continue
        cand = np.flatnonzero(candidates(c, i, grid))
        cand = cand[np.lexsort((cand, py[cand], px[cand], D[i, cand]))]
        ranked = cand[~occ0[cand]]
        ncand[i] = len(ranked); ranked_free[i] = int((~occ[ranked[:SBP_K]]).sum())
        rescan[i] = len(ranked) > SBP_K and (ranked_free[i] < 2 if mode == "map" else ranked_free[i] == 0)
        free = cand[~occ[cand]]
        free = free[D[i, free] < 256]                           # bestDist starts at 256, only strictly smaller distances enter
        if not len(free) or D[i, free[0]] > c.th_high:
            continue
        if mode == "map" and len(free) > 1 and c.t.kp["octave"][free[0]] == c.t.kp["octave"][free[1]] \
                and F(D[i, free[0]]) > F(c.nn_ratio) * F(D[i, free[1]]):
            continue
        idx[i] = free[0]; dist[i] = D[i, free[0]]
        if c.q.blocks[i]:
            occ[free[0]] = True
    return int((idx >= 0).sum()), idx, dist, NS(ncand=ncand, ranked_free=ranked_free, rescan=rescan)


# ================================================================================================ 1 + 2: the claim chain
def _lattice(rng, n):
    """n points on a jittered lattice of 10 px cells (bounds B0): a few hundred cells, so several points share one; point 0 lies in a late cell"""
    cx = 2 * rng.integers(1, 31, n); cy = 2 * rng.integers(1, 23, n)
    cx[0], cy[0] = 61, 45
    x = (10 * cx + rng.uniform(-3, 3, n)).astype(F); y = (10 * cy + rng.uniform(-3, 3, n)).astype(F)
    return x, y, cx, cy


def compactions(ncand_per_chunk):
    """how often k_search_by_projection compacts its list, from the candidate count of each 64-feature chunk"""
    nl = ncomp = 0
    for m in ncand_per_chunk:
        if nl + 64 > SBP_LCAP:
            nl = SBP_K; ncomp += 1
        nl += m
    return ncomp


def chain(kp_dt, name, nt, Q=40, best="perm", occupied=(), free_every=0, marks=False, map_octaves=True, seed=7):
    """Q identical queries over one window that holds all nt features.  Query i takes the i-th free feature in (distance, cellX, cellY,
    index) order; a query with q_blocks = 0 leaves its feature to the next one.  In map mode a same-octave runner-up at the same distance
    fails the ratio test (nn_ratio 0.9): the query stays empty, claims nothing, and so does every query after it."""
    rng = np.random.default_rng(seed + nt)
    x, y, cx, cy = _lattice(rng, nt)
    perm = rng.permutation(nt)
    d = 1 + (perm % 40)
    if best != "perm":                                                    # the 16 best keys at chosen indices, ties among them and among the rest
        if best == "first64":
            S = np.sort(rng.choice(64, 16, replace=False))
        elif best == "last64":
            S = nt - 64 + np.sort(rng.choice(64, 16, replace=False))
        elif nt >= 1000:                                                  # "spread": on either side of both compaction boundaries
            S = np.concatenate([np.arange(508, 516), np.arange(956, 964)])
        else:                                                             # ... of the one boundary (the last chunk boundary where there is none)
            b = 512 if nt > 512 else 448
            S = np.arange(b - 8, b + 8); S = S[S < nt]
            S = np.concatenate([np.arange(b - 8 - (16 - len(S)), b - 8), S])
        d = 5 + (perm % 36)
        d[S] = 1 + (np.arange(16) % 4)
    order = np.lexsort((np.arange(nt), cy, cx, d))
    if best != "perm":
        assert set(order[:16]) == set(S.tolist())
    octave = np.zeros(nt, np.int32)
    same_at = ()
    if map_octaves:                                                       # neighbours in rank order differ in octave, except where stated
        same_at = (21, 37) if nt == 100 else ()
        o = 0
        for rk in range(nt):
            o = o if rk in same_at else (o + 1) % 3
            octave[order[rk]] = o
    t = feats(kp_dt, x, y, d, octave=octave)
    for j in occupied:
        t.occ[order[j]] = 1
    blocks = np.ones(Q, np.uint8)
    if free_every:
        blocks[free_every - 1::free_every] = 0
    q = queries(np.full(Q, 320.0), np.full(Q, 240.0), 400.0, blocks=blocks)
    nmark = 0
    if marks:                                                             # two narrow queries first claim ranks 14 and 15 of the chain's ranked list
        tgt = order[[14, 15]]; nmark = 2
        mq = queries(t.kp["x"][tgt], t.kp["y"][tgt], 2.0, desc=t.desc[tgt])
        q = NS(**{k: np.concatenate([getattr(mq, k), getattr(q, k)]) for k in vars(q)})
    # ---- the closed formula
    free = [j for j in order if not t.occ[j]]
    exp = {}
    for mode in ("last", "map"):
        idx = []; claimed = set()
        if marks:
            idx += list(tgt); claimed |= set(tgt.tolist())
        for i in range(Q):
            av = [j for j in free if j not in claimed][:2]
            j = av[0]
            if mode == "map" and len(av) > 1 and octave[av[0]] == octave[av[1]] and F(d[av[0]]) > F(0.9) * F(d[av[1]]):
                idx.append(-1); continue
            idx.append(j)
            if blocks[i]:
                claimed.add(j)
        idx = np.array(idx); exp[mode] = (idx, np.where(idx >= 0, np.concatenate([np.zeros(nmark, int), d[idx[nmark:]]]), 256))
    c = make(name, q, t, exp, nn_ratio=0.9)
    # ---- path: every chain query has all nt features as candidates (same window, levels unchecked, t_uright = -1)
    grid = cells(t.kp, c.bounds)
    assert np.array_equal(grid[0], cx) and np.array_equal(grid[1], cy)
    assert all(candidates(c, i, grid).sum() == nt for i in (nmark, nmark + Q - 1)) and np.all(q.lo == 0) and np.all(q.hi == -1) and np.all(t.uright == -1)
    if marks:
        assert all(candidates(c, i, grid).sum() == 1 for i in (0, 1))
    c.props.update(ncomp=compactions([min(64, nt - b) for b in range(0, nt, 64)]), same_at=same_at, nmark=nmark,
                   shared_cells=int(nt - len(set(zip(cx.tolist(), cy.tolist())))), order=order)
    assert c.props["shared_cells"] > 0 and order[0] != 0 and (cx[0], cy[0]) == (61, 45)
    return c


# ================================================================================================ 3: ties and traversal order
def ties(kp_dt):
    """one query per island, identical distances (7) inside an island; the lower index lies in the later cell.  B0 cells are 10 px, so the
    cell of (10 a + 1, 10 b + 1) is (a, b).  Odd and even cell numbers (cell = 48 cellX + cellY) both occur among the winners."""
    isl = [  # (query centre cell), [(cellX, cellY, octave) per feature], winner, runner-up
        ((10, 20), [(10, 20, 0), (10, 20, 1), (10, 20, 2)], 0, 1),             # same cell: index order
        ((20, 20), [(22, 20, 0), (20, 20, 1)], 1, 0),                            # cells differ in X
        ((30, 21), [(30, 23, 0), (30, 21, 1)], 1, 0),                            # cells differ only in Y (winner in an odd cell)
        ((41, 11), [(43, 9, 0), (41, 13, 1), (41, 11, 2), (41, 11, 2)], 2, 3),  # all three; runner-up = same cell, next index, same octave
        ((51, 31), [(53, 29, 0), (51, 33, 2), (51, 31, 2), (51, 31, 1)], 2, 3),  # runner-up in another octave; the next in traversal shares it
    ]
    x, y, o, qu, qv, win, run = [], [], [], [], [], [], []
    for (qx, qy), fs, w, ru in isl:
        win.append(len(x) + w); run.append(len(x) + ru)
        for a, b, oc in fs:
            x.append(10 * a + 1.0); y.append(10 * b + 1.0); o.append(oc)
        qu.append(10 * qx + 1.0); qv.append(10 * qy + 1.0)
    t = feats(kp_dt, x, y, 7, octave=o)
    q = queries(qu, qv, 35.0, blocks=0)
    win = np.array(win); run = np.array(run)
    same = t.kp["octave"][win] == t.kp["octave"][run]                       # 7 > 0.9 * 7: a same-octave runner-up rejects
    assert same.tolist() == [False, False, False, True, False]
    c = make("ties", q, t, {"last": (win, 7), "map": (np.where(same, -1, win), 7)}, nn_ratio=0.9)
    px, py, _ = cells(t.kp, c.bounds)
    for i in range(len(isl)):
        m = np.flatnonzero(candidates(c, i))
        assert len(m) == len(isl[i][1]) and np.all(ham(q.desc[i:i + 1], t.desc[m]) == 7)
        k = m[np.lexsort((m, py[m], px[m]))]
        assert k[0] == win[i] and k[1] == run[i] and (win[i] != m.min() or i == 0)
    assert {int((px[w] * ROWS + py[w]) & 1) for w in win} == {0, 1}
    return c


# ================================================================================================ 4: grid and bounds
def _half_cell(mn, inv, k0):
    """a float x with (x - mn) * inv == k + 0.5 exactly, for the first k >= k0 that has one"""
    for k in range(k0, k0 + 30):
        x = F((k + 0.5) / float(inv) + float(mn))
        for _ in range(8):
            x = np.nextafter(x, F(-1e9))
        for _ in range(17):
            if (x - mn) * inv == F(k + 0.5):
                return x, k
            x = np.nextafter(x, F(1e9))
    raise AssertionError("no exact half-cell position")


def grid_bounds(kp_dt):
    mnx, mny, mxx, mxy = (F(b) for b in B1)
    invW = F(COLS) / (mxx - mnx); invH = F(ROWS) / (mxy - mny)
    X = lambda cell: F(float(mnx) + cell / float(invW)); Y = lambda cell: F(float(mny) + cell / float(invH))      # position of a fractional cell index
    hx, kx = _half_cell(mnx, invW, 20); hy, ky = _half_cell(mny, invH, 15)
    fs = [  # x, y, distance, expected cell (None: PosInGrid rejects it)
        (X(-0.4), Y(-0.4), 10, (0, 0)),          # 0  round(-0.4) = 0: in the grid
        (X(-0.8), Y(24.0), 1, None),             # 1  column -1
        (X(63.7), Y(24.0), 2, None),             # 2  column 64
        (X(32.0), Y(47.6), 3, None),             # 3  row 48
        (X(32.0), Y(-0.7), 4, None),             # 4  row -1
        (X(63.2), Y(47.3), 15, (63, 47)),        # 5
        (hx, hy, 16, (kx + 1, ky + 1)),          # 6  exact half cell in both axes: rounds away from zero
        (X(32.0), Y(30.0), 17, (32, 30)),        # 7
        (X(0.2), Y(24.0), 18, (0, 24)),          # 8
        (X(62.9), Y(24.0), 19, (63, 24)),        # 9
        (X(32.0), Y(0.1), 20, (32, 0)),          # 10
        (X(32.0), Y(46.8), 21, (32, 47)),        # 11
        (hx + F(2.0), hy - F(2.0), 16, (kx + 1, ky)),   # 12 ties with 6; earlier cell than 6 only because 6 rounds up in y
    ]
    t = feats(kp_dt, [f[0] for f in fs], [f[1] for f in fs], [f[2] for f in fs], octave=np.arange(len(fs)) % 8)
    px, py, ing = cells(t.kp, B1)
    for j, f in enumerate(fs):
        assert (f[3] is None and not ing[j]) or (f[3] is not None and ing[j] and (px[j], py[j]) == f[3]), (j, px[j], py[j])
    assert (t.kp["x"][6] - mnx) * invW == F(kx + 0.5) and (t.kp["y"][6] - mny) * invH == F(ky + 0.5)
    assert t.kp["x"][0] < mnx and t.kp["y"][0] < mny
    big = F(1e30); inf = F(np.inf); nan = F(np.nan)
    qs = [  # u, v, r, expected feature, seen by the oracle
        (320.0, 240.0, 1000.0, 0, True),                    # 0  the whole grid: 1..4 have the best distances and are no candidates
        (X(0.2), Y(24.0), 30.0, 8, True),                   # 1  cut by the left edge (feature 1 lies inside the pixel window)
        (X(62.9), Y(24.0), 30.0, 9, True),                  # 2  right edge (feature 2)
        (X(32.0), Y(0.1), 30.0, 10, True),                  # 3  top edge (feature 4)
        (X(32.0), Y(46.8), 30.0, 11, True),                 # 4  bottom edge (feature 3)
        (float(mnx) - 50.0, 240.0, 20.0, -1, True),         # 5  wholly outside, left
        (float(mxx) + 50.0, 240.0, 20.0, -1, True),         # 6  right
        (320.0, float(mny) - 50.0, 20.0, -1, True),         # 7  above
        (320.0, float(mxy) + 50.0, 20.0, -1, True),         # 8  below
        (X(32.0), Y(30.0), 0.0, -1, True),                  # 9  r = 0 on top of feature 7
        (X(32.0), Y(30.0), -5.0, -1, True),                 # 10 r < 0
        (hx, hy, 6.0, 12, True),                            # 11 the half-cell tie: 12 = (kx+1, ky) comes before 6 = (kx+1, ky+1)
        (X(-0.4), Y(-0.4), 3.0, 0, True),                   # 12 a window around the point outside the bounds that is in cell (0, 0)
        (inf, 240.0, 30.0, -1, False), (nan, 240.0, 30.0, -1, False), (320.0, nan, 30.0, -1, False), (320.0, -inf, 30.0, -1, False),
        (big, big, 0.0, -1, False),                         # 17 what k_project_last writes for a point that fails its tests
        (-big, 240.0, 30.0, -1, False), (big, 240.0, 30.0, -1, False),
        (320.0, 240.0, 1000.0, 0, True),                    # 20 as query 0: the queries above left no trace
    ]
    q = queries([s[0] for s in qs], [s[1] for s in qs], [s[2] for s in qs], blocks=0)
    idx = np.array([s[3] for s in qs])
    d = np.array([fs[j][2] if j >= 0 else 256 for j in idx])
    c = make("grid_bounds", q, t, {"last": (idx, d), "map": (idx, d)}, bounds=B1, oracle_mask=[s[4] for s in qs])
    assert len(set(t.kp["octave"][[6, 12]])) == 2                            # distinct octaves: the ratio test never applies, both modes agree
    ws = [window(c, i) for i in range(13)]
    assert ws[0] == (0, 63, 0, 47) and all(ws[i] is None for i in (5, 6, 7, 8))
    assert ws[1][0] == 0 and ws[2][1] == 63 and ws[3][2] == 0 and ws[4][3] == 47 and all(0 < a <= b < 63 for a, b in (ws[1][2:], ws[2][2:], ws[3][:2], ws[4][:2]))
    for i, rejected in ((1, 1), (2, 2), (3, 4), (4, 3)):                      # the rejected point is inside the pixel window, and closer in Hamming distance
        assert abs(t.kp["x"][rejected] - q.u[i]) < q.r[i] and abs(t.kp["y"][rejected] - q.v[i]) < q.r[i] and fs[rejected][2] < fs[idx[i]][2]
    assert set(np.flatnonzero(candidates(c, 11)).tolist()) == {6, 12} and ws[9] is not None and not candidates(c, 9).any() and not candidates(c, 10).any()
    return c


# ================================================================================================ 5: boundary values
def boundaries(kp_dt, complement=False):
    """islands 60 px apart, one query each (q_blocks = 0), every number exact in float.  Each island lists its features as
    (dx, dy, distance, octave, uright) relative to the query at (X, Y) with radius 8 and q_ur = X - 20, then the expected feature of the
    island in last-frame and in map mode (nn_ratio 0.5)."""
    below = lambda v: float(np.nextafter(F(v), F(-1e9))); above = lambda v: float(np.nextafter(F(v), F(1e9)))
    isl = []
    R = 8.0
    def island(fs, last, mp=None, lo=0, hi=-1, at=None, q_ur=None):
        isl.append((fs, last, last if mp is None else mp, lo, hi, at, q_ur))
    if not complement:
        th_high = 60
        island([(8.0, 0.0, 1, 0, -1), (1.0, 1.0, 50, 1, -1)], 1)                      # |dx| == r is rejected
        island([(-8.0, 0.0, 1, 0, -1), (1.0, 1.0, 50, 1, -1)], 1)
        island([(0.0, 8.0, 1, 0, -1), (1.0, 1.0, 50, 1, -1)], 1)                      # |dy| == r
        island([(below(R), 0.0, 1, 0, -1), (1.0, 1.0, 50, 1, -1)], 0, at=(0.0, 40.0))   # the next float below r is accepted (query at 0: dx is exact)
        island([(0.0, below(R), 1, 0, -1), (1.0, 1.0, 50, 1, -1)], 0, at=(40.0, 0.0))
        island([(1.0, 0.0, 1, 0, R), (1.0, 1.0, 50, 1, -1)], 0, q_ur=0.0)             # er == r is kept (q_ur = 0, t_uright = r)
        island([(1.0, 0.0, 1, 0, above(R)), (1.0, 1.0, 50, 1, -1)], 1, q_ur=0.0)      # the next float above r is rejected
        island([(1.0, 0.0, 1, 0, 0.0), (1.0, 1.0, 50, 1, -1)], 0)                     # t_uright == 0: no stereo check
        island([(1.0, 0.0, 1, 0, -3.0), (1.0, 1.0, 50, 1, -1)], 0)                    # t_uright < 0: none either
        island([(1.0, 0.0, 60, 0, -1)], 0)                                            # d == th_high is accepted
        island([(1.0, 0.0, 61, 0, -1)], -1)                                           # d == th_high + 1 is rejected
        island([(1.0, 0.0, 10, 2, -1), (2.0, 0.0, 20, 2, -1)], 0, 0)                  # map: d == nn_ratio * d2 is accepted
        island([(1.0, 0.0, 11, 2, -1), (2.0, 0.0, 20, 2, -1)], 0, -1)                 # one bit more is rejected
        island([(1.0, 0.0, 11, 2, -1), (2.0, 0.0, 20, 3, -1)], 0, 0)                  # a second best in another octave is accepted
        island([(1.0, 0.0, 11, 2, -1)], 0, 0)                                         # a single candidate is accepted
        island([(1.0, 0.0, 5, 7, -1)], 0, lo=0, hi=-1)                                # (0, -1) checks nothing
        island([(1.0, 0.0, 1, 2, -1), (2.0, 0.0, 5, 3, -1)], 1, lo=3, hi=-1)          # forward band (3, -1): 2 is outside, 3 is its end
        island([(1.0, 0.0, 5, 7, -1)], 0, lo=3, hi=-1)                                # ... and it has no upper end
        island([(1.0, 0.0, 1, 4, -1), (2.0, 0.0, 5, 3, -1)], 1, lo=0, hi=3)           # backward band (0, 3): 4 is outside, 3 is its end
        island([(1.0, 0.0, 5, 0, -1)], 0, lo=0, hi=3)
        island([(1.0, 0.0, 1, 1, -1), (2.0, 0.0, 5, 0, -1)], 1, lo=0, hi=0)           # (0, 0) does check
        island([(1.0, 0.0, 1, 1, -1), (2.0, 0.0, 5, 2, -1)], 1, lo=2, hi=4)           # a two-sided band: below, at the lower end,
        island([(1.0, 0.0, 1, 5, -1), (2.0, 0.0, 5, 4, -1)], 1, lo=2, hi=4)           # above, at the upper end
    else:
        th_high = 256
        island([(1.0, 0.0, 256, 0, -1)], -1)                                          # the complement alone: d = 256 never enters bestDist
        island([(1.0, 0.0, 256, 0, -1), (2.0, 0.0, 200, 1, -1)], 1)
        island([(1.0, 0.0, 200, 0, -1), (2.0, 0.0, 256, 0, -1)], 0, 0)                # ... and never becomes a second best: 200 > 0.5 * 256 would reject
        island([(1.0, 0.0, 200, 0, -1), (2.0, 0.0, 255, 0, -1)], 0, -1)               # d2 = 255 does
        island([(1.0, 0.0, 255, 0, -1)], 0, 0)
    x, y, d, o, ur, qu, qv, qur, lo, hi, el, em, own = ([] for _ in range(13))
    for k, (fs, last, mp, l, h, at, q_ur) in enumerate(isl):
        X, Y = at if at else (100.0 + 60.0 * (k % 8), 100.0 + 60.0 * (k // 8))
        base = len(x)
        for dx, dy, dist, oc, u in fs:
            x.append(X + dx); y.append(Y + dy); d.append(dist); o.append(oc); ur.append(u)
        qu.append(X); qv.append(Y); lo.append(l); hi.append(h); qur.append(X - 20.0 if q_ur is None else q_ur)
        el.append(base + last if last >= 0 else -1); em.append(base + mp if mp >= 0 else -1); own.append(range(base, len(x)))
    t = feats(kp_dt, x, y, d, octave=o)
    t.uright[:] = np.array(ur, F)
    q = queries(qu, qv, R, lo=lo, hi=hi, ur=qur, blocks=0)
    d = np.array(d); el = np.array(el); em = np.array(em)
    c = make("complement" if complement else "boundaries", q, t, {"last": (el, np.where(el >= 0, d[el], 256)), "map": (em, np.where(em >= 0, d[em], 256))},
             th_high=th_high, nn_ratio=0.5)
    if not complement:                                                          # the boundary values are what they claim to be, in float
        kp = t.kp
        assert kp["x"][0] - q.u[0] == F(R) and q.u[1] - kp["x"][2] == F(R) and kp["y"][4] - q.v[2] == F(R)
        assert kp["x"][6] - q.u[3] == np.nextafter(F(R), F(0)) and kp["y"][8] - q.v[4] == np.nextafter(F(R), F(0)) and kp["y"][6] == q.v[3]
        assert abs(q.ur[5] - t.uright[10]) == F(R) and abs(q.ur[6] - t.uright[12]) == np.nextafter(F(R), F(9)) and t.uright[14] == 0 and t.uright[16] < 0
        assert abs(q.ur[7] - t.uright[14]) > F(R) and abs(q.ur[8] - t.uright[16]) > F(R)          # far off: only the sign of t_uright spares them
        assert F(10) == F(0.5) * F(20) and F(11) > F(0.5) * F(20)
    for i in range(len(isl)):                                                   # islands do not see each other
        assert set(np.flatnonzero(candidates(c, i)).tolist()) <= set(own[i])
    assert np.array_equal(ham(np.tile(BASE, (1, 1)), t.desc)[0], d)
    return c


# ================================================================================================ 6: rotation consistency
def rotation(kp_dt, name, counts, tail=True):
    """isolated one-to-one pairs (query on top of its feature, distance 0, radius 2).  counts = [(bin, n), ...] in the order the pairs are
    laid out; pair k of a bin has q_angle - t_angle = 30 bin - 7 + k % 15 degrees, reached for every other pair through a negative difference
    that wraps by +360.  With factor = 1 / 30 the bin is round(rot / 30) for rot in [0, 360): ONLY BINS 0..12 EXIST, bins 13..29 of the
    30-bin histogram stay empty and `bin == 30` cannot happen.  `tail`: a pair in bin 12 alone (culled), then a second query on the same
    feature with an angle of the best bin -- the culled query's claim still blocks it."""
    bins = []; qa = []; ta = []
    for b, n in counts:
        for k in range(n):
            diff = 30.0 * b - 7.0 + (k % 15)
            if diff < 0:
                diff += 360.0                                             # bin 0 from below: rot in [353, 360) rounds to 12 -- not used, see assert
            tang = 40.0 + k if (k & 1) == 0 else 355.0 - k                 # odd pairs: t_angle > q_angle, so the raw difference is negative
            qang = tang + diff
            if qang >= 360.0:
                qang -= 360.0
            bins.append(b); qa.append(qang); ta.append(tang)
    assert all(b >= 1 for b, _ in counts)
    n = len(bins)
    tq = list(range(n))                                                    # query k sits on feature tq[k]
    if tail:
        bins += [12, counts[0][0]]; ta.append(10.0); qa += [0.0, 10.0 + 30.0 * counts[0][0]]          # 0 - 10 = -10 -> 350 -> bin 12
        tq += [n, n]
    nt = len(ta)
    x = 50.0 + 20.0 * (np.arange(nt) % 25); y = 50.0 + 20.0 * (np.arange(nt) // 25)
    t = feats(kp_dt, x, y, 0, angle=np.array(ta, F))
    tq = np.array(tq)
    q = queries(x[tq], y[tq], 2.0, angle=np.array(qa, F), desc=t.desc[tq])
    # the bins, in the kernel's float steps
    rot = q.angle - t.kp["angle"][tq]
    rot = np.where(rot < 0, rot + F(360.0), rot)
    got = _round_away(rot * (F(1.0) / F(30)))
    assert np.array_equal(got, bins) and got.max() <= 12 and (q.angle - t.kp["angle"][tq] < 0).sum() >= n // 3
    # ComputeThreeMaxima by hand: strict > keeps the first of equal bins ahead; a bin survives when its count is >= 0.1 * the best
    hist = {}
    matched = np.ones(len(tq), bool)
    if tail:
        matched[-1] = False                                                # its only candidate is claimed
    for b, m in zip(bins, matched):
        if m:
            hist[b] = hist.get(b, 0) + 1
    c = NS(bins=np.array(bins), hist=hist, matched=matched, tq=tq)
    return name, q, t, c


def rotation_case(kp_dt, name, counts, keep, tail=True):
    """`keep` is the hand-stated set of surviving bins"""
    name, q, t, r = rotation(kp_dt, name, counts, tail)
    all_idx = np.where(r.matched, r.tq, -1)
    rot_idx = np.where(r.matched & np.isin(r.bins, list(keep)), r.tq, -1)
    c = make(name, q, t, {"last": (all_idx, 0), "rot": (rot_idx, 0)}, hist=r.hist, keep=set(keep))
    assert (rot_idx < 0).sum() > (all_idx < 0).sum() or not tail
    return c


ROTATION = [  # name, [(bin, count) ...], surviving bins
    ("rot_20_2_1", [(3, 20), (7, 2), (10, 1)], {3, 7}),            # 2 < 0.1f * 20 is false: the second stays; 1 < 2: the third goes
    ("rot_20_1_1", [(3, 20), (7, 1), (10, 1)], {3}),               # 1 < 2: second and third go
    ("rot_5_5_2_2", [(2, 5), (9, 5), (4, 2), (11, 2)], {2, 9, 4}),   # equal firsts: both stay; equal thirds: strict > keeps bin 4, bin 11 goes
    ("rot_5_3_3_3", [(1, 5), (4, 3), (6, 3), (8, 3)], {1, 4, 6}),   # three equal bins behind the best: the first two in bin order stay
    ("rot_3_3_3", [(5, 3), (2, 3), (9, 3), (11, 1)], {2, 5, 9}),   # three equal bests; a fourth, smaller bin is culled
]


# ================================================================================================ 7: limits
def limit_nq(kp_dt, nq=MAX_Q):
    """nq queries on 8 features, windows 2 px: query i sits on feature i % 8 with its descriptor; nobody blocks, everybody matches"""
    x = 105.0 + 50.0 * np.arange(8); y = np.full(8, 205.0)
    t = feats(kp_dt, x, y, 3 + np.arange(8))
    k = np.arange(nq) % 8
    q = queries(x[k], y[k], 2.0, blocks=0, desc=t.desc[k])
    c = make("nq_%d" % nq, q, t, {"last": (k, 0), "rot": (k, 0), "map": (k, 0)})
    assert all(candidates(c, i).sum() == 1 for i in (0, 7, nq - 1))
    return c


def limit_nt(kp_dt, nt=MAX_T):
    """nt features, all but the last two crowded into the far cell (60, 44); the last two lie at (104, 104).  Feature nt - 2 is the closer one
    and is held (t_occupied), so the only match is index nt - 1: the top of the key's 16-bit index field and of the occupancy bitmap.  Four
    identical queries with a 3 px window: the first takes it, the others find it claimed."""
    x = np.full(nt, 601.0, F); y = np.full(nt, 441.0, F)
    x[-2:] = 104.0; y[-2:] = 104.0
    desc = np.tile(flip(9), (nt, 1)); desc[-2] = flip(1); desc[-1] = flip(2)
    t = feats(kp_dt, x, y, 0, desc=desc)
    t.occ[-2] = 1
    q = queries(np.full(4, 104.0), np.full(4, 104.0), 3.0)
    c = make("nt_%d" % nt, q, t, {"last": ([nt - 1, -1, -1, -1], 2), "map": ([nt - 1, -1, -1, -1], 2)})
    w = window(c, 0)
    assert (w[1] - w[0] + 1) * (w[3] - w[2] + 1) <= 4 and set(np.flatnonzero(candidates(c, 0)).tolist()) == {nt - 2, nt - 1}
    return c


def tiny(kp_dt, nt):
    t = feats(kp_dt, [100.0] * nt, [100.0] * nt, 4)
    q = queries([101.0], [99.0], 5.0)
    e = ([0], 4) if nt else ([-1], 256)
    return make("nq1_nt%d" % nt, q, t, {"last": e, "rot": e, "map": e})


# ================================================================================================ 8: dense contention
def dense(kp_dt, tracked_th=None):
    """300 features in a 100 x 100 px patch, 300 queries whose descriptors are up to 6 bit flips from 8 prototypes, as the features' are.  With
    tracked_th the windows are the tracked entry point's (2.5 or 4.0 by view_cos, times th when th != 1, times scale[level], band
    [level - 1, level]); otherwise radius 40 and no level check."""
    rng = np.random.default_rng(0xDE5E)
    n = 300
    protos = rng.integers(0, 256, (8, 32), dtype=np.uint8)
    def descs():
        out = np.empty((n, 32), np.uint8)
        for i in range(n):
            out[i] = flip(int(rng.integers(0, 7)), int(rng.integers(0, 256)), protos[rng.integers(0, 8)])
        return out
    t = feats(kp_dt, rng.uniform(270, 370, n), rng.uniform(190, 290, n), 0, octave=rng.integers(0, 4, n), desc=descs())
    t.uright[:] = np.where(rng.uniform(size=n) < 0.5, t.kp["x"] - rng.uniform(10, 14, n), -1).astype(F)
    t.occ[:] = rng.uniform(size=n) < 0.1
    u = rng.uniform(270, 370, n).astype(F); v = rng.uniform(190, 290, n).astype(F)
    ur = (u - rng.uniform(10, 14, n)).astype(F)
    blocks = (rng.uniform(size=n) < 0.9).astype(np.uint8)
    if tracked_th is None:
        q = queries(u, v, 40.0, ur=ur, blocks=blocks, desc=descs())
        c = make("dense", q, t, {}, nn_ratio=0.8)
    else:
        level = rng.integers(0, 5, n).astype(np.int32)
        vcos = np.where(rng.uniform(size=n) < 0.5, 0.9985, 0.9975).astype(F)         # both sides of 0.998
        r = np.where(vcos.astype(np.float64) > 0.998, F(2.5), F(4.0)).astype(F)
        if F(tracked_th) != F(1.0):
            r = r * F(tracked_th)
        q = queries(u, v, r * SF[level], lo=level - 1, hi=level, ur=ur, blocks=blocks, desc=descs())
        c = make("dense_tracked_%g" % tracked_th, q, t, {}, nn_ratio=0.8, tracked=NS(level=level, view_cos=vcos, th=float(tracked_th)))
        assert set(np.unique(r / (F(tracked_th) if tracked_th != 1.0 else F(1)))) == {F(2.5), F(4.0)}
    for mode in (("last", "map") if tracked_th is None else ("map",)):
        nm, idx, dist, st = model_search(c, mode)
        c.expect[mode] = (nm, idx, dist)
        c.props[mode] = NS(rescans=int(st.rescan.sum()), matched=nm, max_cand=int(st.ncand.max()),
                           contested=int(((st.ranked_free < np.minimum(st.ncand, SBP_K)) & (st.ncand > 0)).sum()))
        p = c.props[mode]
        if tracked_th is None:
            assert p.contested > 100 and p.matched > 100 and p.rescans > 0 and p.max_cand > SBP_K, vars(p)
        else:
            assert p.contested > 20 and p.matched > 20, vars(p)
        won = idx[(idx >= 0) & (blocks == 1)]
        assert len(set(won.tolist())) == len(won)                                      # a claimed feature is never given out twice
    return c


# ================================================================================================ the list
CHAIN_NT = (448, 449, 512, 513, 1000)
# `nl + 64 > SBP_LCAP` is first true with 512 entries in the list, i.e. at the chunk that starts at index 512: nt = 513 is the first size that
# compacts (not 449), nt = 1000 compacts again at index 960
NCOMP = {100: 0, 448: 0, 449: 0, 512: 0, 513: 1, 1000: 2}
COMPACT_AT = (512, 960)


def build_all(kp_dt, limits=True):
    cs = [chain(kp_dt, "chain100", 100),
          chain(kp_dt, "chain100_marks", 100, marks=True),
          chain(kp_dt, "chain100_occupied", 100, occupied=(0, 3, 4, 17)),
          chain(kp_dt, "chain100_free3", 100, free_every=3),
          chain(kp_dt, "chain100_occupied_free3", 100, occupied=(1, 2, 15, 16), free_every=3)]
    for nt in CHAIN_NT:
        for best in ("first64", "last64", "spread"):
            cs.append(chain(kp_dt, "chain%d_%s" % (nt, best), nt, best=best))
    cs += [ties(kp_dt), grid_bounds(kp_dt), boundaries(kp_dt), boundaries(kp_dt, complement=True)]
    cs += [rotation_case(kp_dt, *r) for r in ROTATION]
    cs += [tiny(kp_dt, 1), tiny(kp_dt, 0), dense(kp_dt), dense(kp_dt, 1.0), dense(kp_dt, 4.0)]
    if limits:
        cs += [limit_nq(kp_dt), limit_nt(kp_dt)]
    return {c.name: c for c in cs}
