"""Hand-written inputs for the three guided line searches (csrc/line_track.inc: k_lsbp_keys + k_lsbp_epilogue, k_lines_geom_gate; csrc/line_map.inc:
k_lsbp_map_keys + k_lsbp_map_epilogue; lsbp_window under all of them), plain numpy.

No line extraction and no GPU: key lines are KEYLINE_DT records written field by field (the window reads sx / sy / ex / ey and the line function,
the orientation gates read the in-octave end points sox .. eoy, the length gate reads length -- so every gate is set on its own), descriptors
are desc_bits(k): Hamming distance k from the zero descriptor every query carries, and the line grid is a CSR written from a {cell: [lines]}
dictionary, so a cell's insertion order -- the order of the reference's visits -- is chosen by hand.  Every builder
  * states what it expects by hand -- literal arrays, or a closed formula such as "query i takes the candidate of rank i in (distance, visit)
    order" -- in Case.expect[mode] = (n_matches, match_idx, match_dist) (mode "geom": (lmatches, matches12, accepted)),
  * asserts the property that puts the case on the path it is meant for, through model_map() / model_last() (Case.props keeps the figures).
Modes: "map" = SearchByProjection(F, vpMapLines) (hvo_search_lines_by_projection_map), "last" = SearchByProjection(Cur, Last)
(hvo_search_lines_by_projection), "geom" = SearchByGeomNApearance (hvo_match_lines_geom).  Case.local marks the cases that also go through the
resident map (hvo_search_local_lines): local_map() builds that map over the case's current-frame arrays.

model_map() is a second, sort-based statement of the local-map search ("the first two free keys in (distance, visit position) order, then
the acceptance rule") which also counts what the kernels' paths depend on: candidates per query, which of the LSBP_MAP_TOPK smallest keys are
claimed at each query's turn, hence whether k_lsbp_map_epilogue must fall back to the query's list, and the lane (index % 64) and 64-line
chunk (index // 64) of each of the smallest keys in k_lsbp_map_keys."""
from types import SimpleNamespace as NS

import numpy as np

import line_map_ref as lmr
import local_map_lines_ref as ref

F = np.float32
B0 = np.array([0.0, 640.0, 0.0, 480.0], np.float32)             # mnMinX, mnMaxX, mnMinY, mnMaxY: 10 x 10 pixel cells
B1 = np.array([-12.5, 652.5, -9.0, 489.0], np.float32)          # undistorted bounds with a negative minimum
BOUNDS = B0
MAXT, MAXQ, TOPK = 2048, 16384, 4                               # LSBP_MAXT, LSBP_MAP_MAXQ, LSBP_MAP_TOPK
VC_WIDE = np.float32(0.5)                                       # a viewing cosine below 0.998: radius 8
VC_AT = np.float32(0.998)                                       # float(0.998f) > 0.998: radius 5
VC_BELOW = np.nextafter(VC_AT, np.float32(0.0))                 # the float below: radius 8
COS10, COS20 = np.cos(10.0 / 180.0 * np.pi), np.cos(20.0 / 180.0 * np.pi)


def desc_bits(k, offset=0):
    """a descriptor at Hamming distance k from the zero descriptor (bits offset .. offset + k - 1 set)"""
    b = np.zeros(256, np.uint8); b[offset:offset + k] = 1
    return np.packbits(b)


def descs(dists):
    """descriptor j at distance dists[j] from zero; equal distances get different descriptors"""
    return np.stack([desc_bits(int(d), (7 * j) % (257 - int(d))) for j, d in enumerate(dists)]) if len(dists) else np.zeros((0, 32), np.uint8)


class Scene:
    """horizontal current lines from x = 100 to 200 at the given heights, each in the grid cell of its start point; line function y - y0;
    3-D line A - B = (1, 0, 0)"""

    def __init__(self, hvo, ys, octaves=None, descs=None):
        n = len(ys)
        self.kl = np.zeros(n, hvo.KEYLINE_DT)
        self.kl["sx"] = 100.0; self.kl["ex"] = 200.0; self.kl["sy"] = ys; self.kl["ey"] = ys
        self.kl["octave"] = 0 if octaves is None else octaves
        self.fn = np.stack([np.zeros(n), np.ones(n), -np.asarray(ys, np.float64)], axis=1)
        self.l3d = np.zeros(n, hvo.LINE3D_DT); self.l3d["A"][:, 0] = 1.0
        self.desc = np.zeros((n, 32), np.uint8) if descs is None else np.asarray(descs, np.uint8)
        cells = {}
        for j, y in enumerate(ys):
            cells.setdefault((10, int(y // 10)), []).append(j)
        self.cs, self.ci = ref.grid_from_cells(cells)

    def queries(self, q_y, view_cos=1.0, wvec=(1.0, 0.0, 0.0), qdesc=None):
        q_y = np.atleast_1d(np.asarray(q_y, np.float32)); nq = len(q_y)
        q = np.stack([np.full(nq, 100.0), q_y, np.full(nq, 200.0), q_y], axis=1).astype(np.float32)
        vc = np.broadcast_to(np.asarray(view_cos, np.float32), (nq,)).copy()
        wv = np.broadcast_to(np.asarray(wvec, np.float64), (nq, 3)).copy()
        qd = np.zeros((nq, 32), np.uint8) if qdesc is None else np.broadcast_to(np.asarray(qdesc, np.uint8), (nq, 32)).copy()
        return q, vc, wv, qd

    def run(self, q_y, view_cos=1.0, wvec=(1.0, 0.0, 0.0), qdesc=None, blocks=None, occ=None, th=1.0, nn_ratio=0.95):
        q, vc, wv, qd = self.queries(q_y, view_cos, wvec, qdesc)
        return ref.search_lines_by_projection_map(q, vc, wv, qd, blocks, self.kl, self.fn, self.l3d, self.desc, occ, self.cs, self.ci, BOUNDS, th, nn_ratio)


# ------------------------------------------------------------------------------------------------ cases and the entry points' argument tuples
def _exp(idx, dist, n=None):
    idx = np.asarray(idx, np.int32).reshape(-1); dist = np.broadcast_to(np.asarray(dist, np.int32), idx.shape).copy()
    dist[idx < 0] = 256
    return (int((idx >= 0).sum()) if n is None else n, idx, dist)


def make(name, t, cs, ci, bounds=B0, map=None, last=None, expect=None, local=None, **props):
    """t: NS(kl, fn, l3d, desc, occ); map: NS(q, vc, wvec, desc, blocks, th, nn_ratio); last: NS(q, kl, desc, blocks, th)"""
    return NS(name=name, t=t, cs=np.asarray(cs, np.int32), ci=np.asarray(ci, np.int32), bounds=np.asarray(bounds, np.float32), map=map, last=last, geom=None,
              expect=dict(expect), local=local, props=props)


def args_map(c):
    m, t = c.map, c.t
    return (m.q, m.vc, m.wvec, m.desc, m.blocks, t.kl, t.fn, t.l3d, t.desc, t.occ, c.cs, c.ci, c.bounds, m.th, m.nn_ratio)


def args_last(c):
    m, t = c.last, c.t
    occ = np.zeros(len(t.kl), np.uint8) if t.occ is None else t.occ
    return (m.q, m.kl, m.desc, m.blocks, t.kl, t.fn, t.desc, occ, c.cs, c.ci, c.bounds, m.th)


def args_geom(c):
    g = c.geom
    return (g.d_last, g.kl_last, g.d_cur, g.kl_cur, c.bounds, g.desc_th, g.has_ml)


def keylines(dt, sx, sy, ex, ey, octave=0, length=None):
    """key lines whose in-octave end points and length follow the image end points (a builder overwrites what it sets by hand)"""
    n = len(sx)
    kl = np.zeros(n, dt)
    for f, v in (("sx", sx), ("sy", sy), ("ex", ex), ("ey", ey), ("sox", sx), ("soy", sy), ("eox", ex), ("eoy", ey)):
        kl[f] = np.asarray(v, np.float32)
    kl["octave"] = octave
    kl["length"] = np.hypot(kl["ex"] - kl["sx"], kl["ey"] - kl["sy"]) if length is None else length
    kl["class_id"] = np.arange(n)
    return kl


def line_functions(kl):
    """mvKeyLineFunctions: the normalised line through the two end points, (a, b, c) with a x + b y + c = the signed distance"""
    sx, sy, ex, ey = (kl[f].astype(np.float64) for f in ("sx", "sy", "ex", "ey"))
    a, b = sy - ey, ex - sx
    n = np.hypot(a, b); n[n == 0] = 1.0
    a, b = a / n, b / n
    return np.stack([a, b, -(a * sx + b * sy)], axis=1)


def lines3d(dt, kl, z=2.0):
    """the key lines' end points at depth z under line_map_ref.CAM, in the camera frame; every line good"""
    l3 = np.zeros(len(kl), dt)
    fx, fy, cx, cy = lmr.CAM[:4]
    for f, (u, v) in (("A", ("sx", "sy")), ("B", ("ex", "ey"))):
        l3[f] = np.stack([(kl[u].astype(np.float64) - cx) / fx * z, (kl[v].astype(np.float64) - cy) / fy * z, np.full(len(kl), z)], axis=1)
    l3["good"] = 1; l3["line_eq"] = (1.0, 0.0, 0.0)
    return l3


def hframe(hvo, ys, dists, octaves=0, cells=None, occ=None, x0=100.0, x1=200.0):
    """horizontal current lines x0 .. x1 at heights ys, descriptor distances `dists`; cells: {(ix, iy): [lines]} (default: the start point's cell,
    index order) -> (t, cell_start, cell_items)"""
    n = len(ys); ys = np.asarray(ys, np.float32)
    kl = keylines(hvo.KEYLINE_DT, np.full(n, x0), ys, np.full(n, x1), ys, octave=octaves)
    fn = np.stack([np.zeros(n), np.ones(n), -ys.astype(np.float64)], axis=1)
    if cells is None:
        cells = {}
        for j, y in enumerate(ys):
            cells.setdefault((int(x0 // 10), int(y // 10)), []).append(j)
    cs, ci = ref.grid_from_cells(cells)
    t = NS(kl=kl, fn=fn, l3d=lines3d(hvo.LINE3D_DT, kl), desc=descs(dists), occ=None if occ is None else np.asarray(occ, np.uint8))
    return t, cs, ci


def hqueries(hvo, q_y, blocks, r, x0=100.0, x1=200.0, desc=None, vc=VC_WIDE):
    """horizontal queries x0 .. x1 at heights q_y for both modes with the SAME window radius r: map (view cosine vc: 8 th or 5 th) and last (r = th)"""
    q_y = np.asarray(q_y, np.float32); nq = len(q_y)
    q = np.stack([np.full(nq, x0), q_y, np.full(nq, x1), q_y], axis=1).astype(np.float32)
    blocks = np.broadcast_to(np.asarray(blocks, np.uint8), (nq,)).copy()
    qd = np.zeros((nq, 32), np.uint8) if desc is None else np.ascontiguousarray(desc, np.uint8)
    base = 8.0 if float(vc) <= 0.998 else 5.0
    wv = np.tile(np.array([1.0, 0.0, 0.0]), (nq, 1))
    m = NS(q=q, vc=np.full(nq, vc, np.float32), wvec=wv, desc=qd, blocks=blocks, th=float(r) / base, nn_ratio=0.95)
    assert float(ref.radius_by_viewing_cos(vc, m.th)) == float(r)
    qkl = keylines(hvo.KEYLINE_DT, q[:, 0], q[:, 1], q[:, 2], q[:, 3])
    return m, NS(q=q, kl=qkl, desc=qd, blocks=blocks, th=float(r))


# ------------------------------------------------------------------------------------------------ the models
def window_cells(bounds, x, y, r):
    """lsbp_window's cell range of one sample point -> (cx0, cx1, cy0, cy1) after clamping, or the number (1 .. 4) of the `continue` it takes"""
    minX, maxX, minY, maxY = (F(v) for v in bounds); x, y, r = F(x), F(y), F(r)
    invW = F(F(64) / F(maxX - minX)); invH = F(F(48) / F(maxY - minY))
    cx0 = max(0, int(np.floor(F(F(F(x - minX) - r) * invW))))
    if cx0 >= 64: return 1
    cx1 = min(63, int(np.ceil(F(F(F(x - minX) + r) * invW))))
    if cx1 < 0: return 2
    cy0 = max(0, int(np.floor(F(F(F(y - minY) - r) * invH))))
    if cy0 >= 48: return 3
    cy1 = min(47, int(np.ceil(F(F(F(y - minY) + r) * invH))))
    if cy1 < 0: return 4
    return cx0, cx1, cy0, cy1


def samples(q4):
    x1, y1, x2, y2 = (F(v) for v in q4)
    return ((x1, y1), (F(float(F(x1 + x2)) / 2.0), F(float(F(y1 + y2)) / 2.0)), (x2, y2))


def _ham_rows(qd, td):
    return np.unpackbits(qd[:, None, :] ^ td[None, :, :], axis=2).sum(axis=2).astype(np.int64)


def model_map_arrays(q, vc, wvec, qdesc, blocks, kl, fn, l3d, tdesc, occ, cs, ci, bounds, th, nn_ratio):
    nq, nt = len(q), len(kl)
    occ0 = np.zeros(nt, bool) if occ is None else np.asarray(occ).astype(bool)
    blocks = np.zeros(nq, bool) if blocks is None else np.asarray(blocks).astype(bool)
    claimed = np.zeros(nt, bool)
    D = _ham_rows(qdesc, tdesc) if nq and nt else np.zeros((nq, nt), np.int64)
    dirs = ref.line_directions(kl) if nt else None
    idx = np.full(nq, -1, np.int32); dist = np.full(nq, 256, np.int32)
    st = NS(ncand=np.zeros(nq, int), top=np.full((nq, TOPK), -1, int), nfree=np.zeros(nq, int), fallback=np.zeros(nq, bool), inside=[None] * nq)
    for i in range(nq):
        r = ref.radius_by_viewing_cos(vc[i], th)
        visit = ref.features_in_area_for_line(*q[i], r, kl, fn, cs, ci, bounds, dirs=dirs) if nt else []
        keys = sorted((int(D[i, j]), p, j) for p, j in enumerate(visit)
                      if not occ0[j] and not float(ref.angle_3d(l3d[j]["A"], l3d[j]["B"], wvec[i])) < ref.TH_NORMAL)
        st.ncand[i] = len(keys)
        for k, key in enumerate(keys[:TOPK]): st.top[i, k] = key[2]
        st.nfree[i] = sum(1 for key in keys[:TOPK] if not claimed[key[2]])
        st.fallback[i] = st.nfree[i] < 2 and len(keys) > TOPK
        free = [key for key in keys if not claimed[key[2]]]
        if not free or free[0][0] > 95: continue
        d1, j1 = free[0][0], free[0][2]
        if len(free) > 1 and int(kl["octave"][j1]) == int(kl["octave"][free[1][2]]) and F(d1) > F(F(nn_ratio) * F(free[1][0])):
            st.inside[i] = "reject" if st.fallback[i] else None
            continue
        st.inside[i] = "pass" if st.fallback[i] and len(free) > 1 and F(d1) > F(F(nn_ratio) * F(free[1][0])) else ("accept" if st.fallback[i] else None)
        idx[i] = j1; dist[i] = d1
        if blocks[i]: claimed[j1] = True
    return int((idx >= 0).sum()), idx, dist, st


def model_map(c):
    """-> (n, idx, dist, stats): stats.ncand[i] candidates of query i (t_occupied lines never enter), .top[i] the lines of its TOPK smallest keys,
    .nfree[i] how many of those are unclaimed at its turn, .fallback[i] the epilogue's rescan condition, .inside[i] what happened inside the
    fallback: "pass" = accepted although best > ratio x second (the octaves differ), "accept", "reject" = the ratio rule in equal octaves"""
    return model_map_arrays(*args_map(c))


def angle2d(a, b):
    ax, ay = float(F(a["eox"] - a["sox"])), float(F(a["eoy"] - a["soy"])); bx, by = float(F(b["eox"] - b["sox"])), float(F(b["eoy"] - b["soy"]))
    with np.errstate(invalid="ignore", divide="ignore"):
        return abs(np.float64(ax * bx + ay * by) / (np.sqrt(np.float64(ax * ax + ay * ay)) * np.sqrt(np.float64(bx * bx + by * by))))


def model_last(c):
    """the frame-to-frame search, sort-based: the smallest free key in (distance, visit position) order among the window's lines that pass the
    10-degree and the length gates -> (n, idx, dist, ncand)"""
    m, t = c.last, c.t
    nq, nt = len(m.q), len(t.kl)
    occ = np.zeros(nt, bool) if t.occ is None else np.asarray(t.occ).astype(bool).copy()
    D = _ham_rows(m.desc, t.desc) if nq and nt else np.zeros((nq, nt), np.int64)
    dirs = ref.line_directions(t.kl) if nt else None
    idx = np.full(nq, -1, np.int32); dist = np.full(nq, 256, np.int32); ncand = np.zeros(nq, int)
    for i in range(nq):
        visit = ref.features_in_area_for_line(*m.q[i], F(m.th), t.kl, t.fn, c.cs, c.ci, c.bounds, TH=F(0.96), dirs=dirs) if nt else []
        keys = []
        for p, j in enumerate(visit):
            ql, tl = m.kl[i], t.kl[j]
            mx = max(ql["length"], tl["length"]); mn = min(ql["length"], tl["length"])
            if angle2d(tl, ql) < COS10 or float(F(mn / mx)) < 0.75: continue
            keys.append((int(D[i, j]), p, j))
        ncand[i] = len(keys)
        free = sorted(k for k in keys if not occ[k[2]])
        if free and free[0][0] <= 95:
            idx[i] = free[0][2]; dist[i] = free[0][0]
            if m.blocks[i]: occ[free[0][2]] = True
    return int((idx >= 0).sum()), idx, dist, ncand


# ------------------------------------------------------------------------------------------------ the local-map scenes of test_local_map_lines.py
def scene_cases(hvo):
    out = []

    def add(name, s, q_y, idx, dist, blocks=None, occ=None, th=1.0, **kw):
        q, vc, wv, qd = s.queries(q_y, **kw)
        t = NS(kl=s.kl.copy(), fn=s.fn, l3d=s.l3d.copy(), desc=s.desc, occ=None if occ is None else np.asarray(occ, np.uint8))
        m = NS(q=q, vc=vc, wvec=wv, desc=qd, blocks=None if blocks is None else np.asarray(blocks, np.uint8), th=th, nn_ratio=0.95)
        out.append(make("scene_" + name, t, s.cs, s.ci, map=m, expect={"map": _exp(idx, dist)}))

    s = Scene(hvo, [100.0]); s.kl["ey"] = np.float32(100.0 + 100.0 * np.tan(np.radians(5.0)))
    add("dir_5deg", s, 100.0, [-1], 256)                        # inside the Cur/Last call's 0.96, outside the 0.998 of this search
    s = Scene(hvo, [100.0]); s.kl["ey"] = np.float32(100.0 + 100.0 * np.tan(np.radians(3.0)))
    add("dir_3deg", s, 100.0, [0], 0)
    s = Scene(hvo, [100.0]); s.l3d["A"][:] = 0.0
    add("nan_line3d", s, 100.0, [0], 0)                         # no fitted 3-D line: 0 / 0 passes
    add("nan_wvec", Scene(hvo, [100.0]), 100.0, [0], 0, wvec=(0.0, 0.0, 0.0))
    rad = np.radians([14.0, 16.0, 170.0, 90.0])
    wv = np.stack([np.cos(rad), np.sin(rad), np.zeros(4)], axis=1)
    wv = np.concatenate([wv, [[np.cos(np.radians(20.0)), 0.0, np.sin(np.radians(20.0))]]])       # tilted out of the image plane
    add("gate3d_14_16_170_90_tilt", Scene(hvo, [100.0]), [100.0] * 5, [0, -1, 0, -1, -1], 0, wvec=wv)
    add("radius_0998f_and_below", Scene(hvo, [106.5]), [100.0, 100.0], [-1, 0], 0, view_cos=[VC_AT, VC_BELOW])   # 6.5 px: inside 8, outside 5
    add("th_1", Scene(hvo, [120.0]), 100.0, [-1], 256, th=1.0)
    add("th_5", Scene(hvo, [120.0]), 100.0, [0], 0, th=5.0)
    add("best_95", Scene(hvo, [100.0], descs=[desc_bits(95)]), 100.0, [0], 95)
    add("best_96", Scene(hvo, [100.0], descs=[desc_bits(96)]), 100.0, [-1], 256)
    for octs, want in (([0, 0], -1), ([0, 1], 0), ([2, 2], -1)):                                 # 50 > 0.95 * 52: rejected in equal octaves only
        add("ratio_50_52_oct%d%d" % tuple(octs), Scene(hvo, [100.0, 101.0], octaves=octs, descs=[desc_bits(50), desc_bits(52)]), 100.0, [want], 50)
    add("ratio_50_60", Scene(hvo, [100.0, 101.0], descs=[desc_bits(50), desc_bits(60)]), 100.0, [0], 50)
    add("ratio_single", Scene(hvo, [100.0], descs=[desc_bits(50)]), 100.0, [0], 50)
    add("tie_same_octave", Scene(hvo, [100.0, 101.0], descs=[desc_bits(40), desc_bits(40, 100)]), 100.0, [-1], 256)
    add("tie_octaves_10", Scene(hvo, [100.0, 101.0], octaves=[1, 0], descs=[desc_bits(40), desc_bits(40, 100)]), 100.0, [0], 40)
    add("claim_blocks", Scene(hvo, [100.0]), [100.0, 100.0], [0, -1], 0, blocks=[1, 0])
    add("claim_overwritten", Scene(hvo, [100.0]), [100.0, 100.0], [0, 0], 0, blocks=[0, 1])
    add("claim_overwritten_then_blocks", Scene(hvo, [100.0]), [100.0] * 3, [0, 0, -1], 0, blocks=[0, 1, 1])
    two = lambda: Scene(hvo, [100.0, 102.0], octaves=[0, 1], descs=[desc_bits(10), desc_bits(20)])
    add("occupied_passed_over", two(), 100.0, [1], 20, occ=[1, 0])
    add("claimed_best_leaves_next", two(), [100.0, 100.0], [0, 1], [10, 20], blocks=[1, 1])
    return out


# ------------------------------------------------------------------------------------------------ candidate counts and where the smallest keys sit
CROWD_NT = 260
PLACE = {"lane": [5, 69, 133, 197], "chunk": [67, 81, 104, 127], "across": [63, 64, 127, 128]}
COUNTS = (4, 5, 64, 65, 130)


def crowd(hvo, name, nt, cand, best, nq, local=None):
    """nt lines of which `cand` lie in the one window (heights 100 .. 109.5, all listed in cell (10, 10) in DESCENDING index order: the
    visit order is the reverse of the index order); the others 200 px below.  The lines of `best` have distance 7 -- equal, so the visit
    position decides among them -- with octaves alternating along the visit order; one other candidate, in the middle of the visit order, has
    distance 20, the rest 22 + (visit position % 50), all in octave 2.  nq blocking queries, all the same.
    By hand: the queries take the best lines in visit order (7 against 7 in different octaves passes), then the 20 (20 <= 0.95 * 22), then
    nothing: 22 against 22 (or 23, 0.95 * 23 = 21.85) in equal octaves is rejected.  The frame-to-frame search has no ratio rule: rank after rank."""
    cand = sorted(cand); visit = cand[::-1]; n = len(cand)
    ys = 300.0 + (np.arange(nt) % 100); d = np.full(nt, 200); octv = np.full(nt, 2)
    for k, j in enumerate(cand): ys[j] = 100.0 + 9.5 * k / max(n, 1)
    bv = [j for j in visit if j in set(best)]; rest = [j for j in visit if j not in set(best)]
    for k, j in enumerate(bv): d[j] = 7; octv[j] = k % 2
    mid = rest[len(rest) // 2] if rest else None
    for p, j in enumerate(rest): d[j] = 20 if j == mid else 22 + p % 50
    cells = {(10, 10): visit}
    for j in range(nt):
        if j not in set(cand): cells.setdefault((10, int(ys[j] // 10)), []).append(j)
    t, cs, ci = hframe(hvo, ys, d, octv, cells)
    m, l = hqueries(hvo, [104.75] * nq, 1, 8.0)
    want = bv + ([mid] if rest else [])                          # map mode: then the ratio rule rejects (or nothing is left)
    e_map = _exp((want + [-1] * nq)[:nq], ([int(d[j]) for j in want] + [256] * nq)[:nq])
    order = sorted(visit, key=lambda j: d[j])                    # (stable: distance, then visit position)
    e_last = _exp((order + [-1] * nq)[:nq], ([int(d[j]) for j in order] + [256] * nq)[:nq])
    c = make(name, t, cs, ci, map=m, last=l, expect={"map": e_map, "last": e_last}, local=local, count=n, best=list(best))
    _, _, _, st = model_map(c)
    assert np.all(st.ncand == n), (name, st.ncand)
    assert [int(v) for v in st.top[0][: len(bv)]] == bv and (n <= TOPK or len(bv) == TOPK)
    fb = [(i >= 3 and n > TOPK) for i in range(nq)]              # one of four left at query 3, none from query 4 on
    assert st.fallback.tolist() == fb, (name, st.fallback)
    c.props["fallback"] = fb
    return c


def crowd_cases(hvo):
    out = [crowd(hvo, "count_0", 8, [], [], 2), crowd(hvo, "count_1", 8, [6], [6], 2), crowd(hvo, "count_2", 8, [2, 5], [2, 5], 3)]
    for place, best in PLACE.items():
        lanes = {b % 64 for b in best}; chunks = {b // 64 for b in best}
        assert {"lane": len(lanes) == 1 and len(chunks) == 4, "chunk": len(lanes) == 4 and len(chunks) == 1,
                "across": chunks == {0, 1, 2} and {63, 0} <= lanes}[place]
        others = [j for j in range(CROWD_NT) if j not in best]
        for n in COUNTS:
            step = len(others) // max(n - 4, 1)
            cand = best + others[::step][: n - 4] if n > 4 else list(best)
            assert len(cand) == n
            out.append(crowd(hvo, "count_%d_%s" % (n, place), CROWD_NT, cand, best, 6,
                             local=NS(th=2.0, nslots=6, occ=()) if place == "across" and n in (65, 130) else None))
    return out


# ------------------------------------------------------------------------------------------------ claim chains in one crowded window
CHAIN_D = [60, 10, 50, 20, 70, 30, 40, 80, 84, 85, 90, 95]       # by line; by rank: lines 1 3 5 6 2 0 4 7 8 9 10 11
CHAIN_RANK = [1, 3, 5, 6, 2, 0, 4, 7, 8, 9, 10, 11]
CHAIN_OCT_A = [0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0]               # line 7 (80) alone in octave 1: 80 > 0.95 * 84 passes only because the octaves differ
CHAIN_OCT_X = [1, 0, 0, 1, 0, 0, 1, 1, 0, 1, 0, 1]               # octave = rank % 2: neighbours in rank never share an octave, every query is accepted


def chain(hvo, name, octv, blocks, idx, occ=None, fallback=None, inside=None, last_idx=None, local_th=5.0):
    """twelve lines 0.25 px apart in one cell, distances CHAIN_D; len(blocks) identical queries with radius 8.  idx: by hand, as line numbers"""
    nq = len(blocks)
    t, cs, ci = hframe(hvo, 100.0 + 0.25 * np.arange(12), CHAIN_D, octv, occ=occ)
    m, l = hqueries(hvo, [101.5] * nq, blocks, 8.0)
    exp = {"map": _exp(idx, [CHAIN_D[j] if j >= 0 else 256 for j in idx])}
    if last_idx is not None: exp["last"] = _exp(last_idx, [CHAIN_D[j] if j >= 0 else 256 for j in last_idx])
    c = make(name, t, cs, ci, map=m, last=l if last_idx is not None else None, expect=exp,
             local=NS(th=local_th, nslots=nq, occ=() if occ is None else tuple(np.flatnonzero(occ))))
    _, _, _, st = model_map(c)
    assert np.all(st.ncand == 12 - (0 if occ is None else int(np.sum(occ)))) and st.ncand[0] >= 10          # a crowded window
    assert st.fallback.tolist() == fallback, (name, st.fallback.tolist())
    if inside is not None: assert st.inside == inside, (name, st.inside)
    c.props.update(fallback=fallback, inside=st.inside)
    return c


def chain_cases(hvo):
    R = CHAIN_RANK; T, Fa = True, False
    assert [CHAIN_D[j] for j in R] == sorted(CHAIN_D) and [CHAIN_OCT_X[j] for j in R] == [k % 2 for k in range(12)]
    out = []
    # every query blocks: rank after rank.  Three of the four smallest keys are gone at query 3: the fallback from there on.  Query 7: 80 > 79.8
    # but octaves 1 and 0 (read from t_kl inside the fallback) -> accepted.  Query 8: 84 > 0.95 * 85 in octave 0 both -> rejected, and again.
    out.append(chain(hvo, "chain_all1", CHAIN_OCT_A, [1] * 12, R[:8] + [-1] * 4, fallback=[Fa] * 3 + [T] * 9,
                     inside=[None] * 3 + ["accept"] * 4 + ["pass"] + ["reject"] * 4, last_idx=R))
    # octaves alternate by rank: all twelve are claimed, the last one alone (95, no second: accepted); the two queries after that find nothing
    out.append(chain(hvo, "chain_exhaust", CHAIN_OCT_X, [1] * 14, R + [-1, -1], fallback=[Fa] * 3 + [T] * 11, last_idx=R + [-1, -1]))
    # no query blocks: everybody gets the best line, nobody rescans
    out.append(chain(hvo, "chain_all0", CHAIN_OCT_A, [0] * 6, [1] * 6, fallback=[Fa] * 6, last_idx=[1] * 6))
    # blocking and free queries alternate: a free query takes what the next blocking one then claims
    out.append(chain(hvo, "chain_alt", CHAIN_OCT_X, [1, 0] * 6, [R[k] for k in (0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6)], fallback=[Fa] * 5 + [T] * 7,
                     last_idx=[R[k] for k in (0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6)]))
    # the best and the third best held before the call: ten candidates, ranks 1 3 4 5 | 6 7 8 ...
    occ = np.zeros(12, np.uint8); occ[[R[0], R[2]]] = 1
    out.append(chain(hvo, "chain_all1_occupied", CHAIN_OCT_A, [1] * 8, [R[k] for k in (1, 3, 4, 5, 6, 7)] + [-1, -1], occ=occ, fallback=[Fa] * 3 + [T] * 5,
                     inside=[None] * 3 + ["accept"] * 2 + ["pass"] + ["reject"] * 2, last_idx=[R[k] for k in (1, 3, 4, 5, 6, 7, 8, 9)]))
    out.append(chain(hvo, "chain_alt_occupied", CHAIN_OCT_X, [0, 1] * 5, [R[k] for k in (1, 1, 3, 3, 4, 4, 5, 5, 6, 6)], occ=occ,
                     fallback=[Fa] * 6 + [T] * 4, last_idx=[R[k] for k in (1, 1, 3, 3, 4, 4, 5, 5, 6, 6)]))
    return out


# ------------------------------------------------------------------------------------------------ visit order
def visit_cases(hvo):
    out = []
    dt = hvo.KEYLINE_DT

    def both(name, t, cs, ci, q_y, blocks, r, idx, dist, x1=200.0, vc=VC_WIDE, **props):
        m, l = hqueries(hvo, q_y, blocks, r, x1=x1, vc=vc)
        c = make(name, t, cs, ci, map=m, last=l, expect={"map": _exp(idx, dist), "last": _exp(idx, dist)}, **props)
        out.append(c)
        return c

    # a tie where the later index is visited first: the cell lists line 1 before line 0
    t, cs, ci = hframe(hvo, [100.0, 100.5], [30, 30], [0, 1], cells={(10, 10): [1, 0]})
    both("visit_tie_later_index_first", t, cs, ci, [100.0] * 3, 1, 8.0, [1, 0, -1], 30)

    # a line that fails at the start sample and passes at a later one: line 0 runs through the query's END point with slope `slope`, listed in the
    # cell of each sample point, and it is listed BEFORE line 1 at the start; line 1 lies on the query.  Equal distances: line 1 wins the tie, as
    # its first PASSING visit is the earlier one
    for name, slope, r, vc, first in (("visit_passes_from_middle", 0.05, 8.0, VC_WIDE, 1), ("visit_passes_at_end_only", 0.06, 5.0, np.float32(1.0), 2)):
        kl = keylines(dt, [100.0, 100.0], [100.0 - 200.0 * slope, 100.0], [300.0, 300.0], [100.0, 100.0], octave=[0, 1])
        kl["length"] = 200.0; kl["soy"] = kl["eoy"] = 0.0                               # the gates of the frame-to-frame search see two parallel lines
        tt = NS(kl=kl, fn=line_functions(kl), l3d=lines3d(hvo.LINE3D_DT, kl), desc=descs([30, 30]), occ=None)
        tt.l3d["A"][0] = tt.l3d["B"][0] + (tt.l3d["A"][1] - tt.l3d["B"][1])             # (the 3-D gate too)
        cs, ci = ref.grid_from_cells({(10, 10): [0, 1], (20, 10): [0], (30, 10): [0]})
        c = both(name, tt, cs, ci, [100.0, 100.0], 1, r, [1, 0], 30, x1=300.0, vc=vc)
        passes = [abs(float(F(tt.fn[0] @ np.array([float(x), float(y), 1.0])))) < r for x, y in samples(c.map.q[0])]
        assert passes == [False] * first + [True] * (3 - first), (name, passes)
        cs_ = F(abs(F(-1.0) * ref.line_directions(kl)[0][0]))
        assert cs_ >= F(0.998) and cs_ < F(0.9989)

    # a line listed in three cells of ONE sample's window: its first visit is in column 9, before line 0's only listing in column 10
    t, cs, ci = hframe(hvo, [100.0, 100.5], [30, 30], [0, 1], cells={(9, 10): [1], (10, 10): [0, 1], (11, 10): [1]})
    both("visit_three_cells", t, cs, ci, [100.0] * 2, 1, 8.0, [1, 0], 30)
    # a line listed twice in one cell (three items for two lines)
    t, cs, ci = hframe(hvo, [100.0, 100.5], [30, 30], [0, 1], cells={(10, 10): [1, 0, 1]})
    assert len(ci) == 3
    both("visit_twice_in_a_cell", t, cs, ci, [100.0] * 3, 1, 8.0, [1, 0, -1], 30)
    # a window over three grid columns, two rows each, every cell with a line: columns first, rows inside a column -- 5 4 3 2 1 0
    cells = {(11, 11): [0], (11, 10): [1], (10, 11): [2], (10, 10): [3], (9, 11): [4], (9, 10): [5]}
    t, cs, ci = hframe(hvo, [112.0, 104.0] * 3, [30] * 6, [1, 0] * 3, cells=cells)
    c = both("visit_three_columns", t, cs, ci, [108.0] * 7, 1, 8.0, [5, 4, 3, 2, 1, 0, -1], 30)
    assert window_cells(B0, 100.0, 108.0, 8.0) == (9, 11, 10, 12)
    assert model_map(c)[3].fallback.tolist() == [False] * 3 + [True] * 4
    return out


# ------------------------------------------------------------------------------------------------ sizes
def ladder(hvo, nt, good, occ_last=False):
    """nt horizontal lines at heights 30 + 400 j / nt, every descriptor at distance 200 except those of `good` {line: (distance, octave)}
    -> (t, cell_start, cell_items, heights)"""
    ys = (30.0 + 400.0 * np.arange(nt) / nt).astype(np.float32)
    d = np.full(nt, 200); octv = np.zeros(nt, int)
    for j, (dj, oj) in good.items(): d[j] = dj; octv[j] = oj
    occ = np.zeros(nt, np.uint8); occ[nt - 1] = 1
    t, cs, ci = hframe(hvo, ys, d, octv, occ=occ if occ_last else None)
    return t, cs, ci, ys


def ring(hvo, nq):
    """eight lines 50 px apart (distance from zero = line number), query i on line i % 8 with descriptor desc_bits(i % 5): each finds its line
    at distance |i % 5 - i % 8|; only the last eight queries block"""
    t, cs, ci = hframe(hvo, 25.0 + 50.0 * np.arange(8), [0] * 8)
    t.desc = np.stack([desc_bits(j) for j in range(8)])
    i = np.arange(nq)
    qd = np.stack([desc_bits(k) for k in range(5)])[i % 5] if nq else np.zeros((0, 32), np.uint8)
    m, l = hqueries(hvo, 25.0 + 50.0 * (i % 8), (i >= nq - 8).astype(np.uint8), 5.0, desc=qd, vc=np.float32(1.0))
    e = _exp(i % 8, np.abs(i % 5 - i % 8))
    return make("nq_%d" % nq, t, cs, ci, map=m, last=l, expect={"map": e, "last": e})


def size_cases(hvo):
    out = []
    for nt in (63, 64, 65, MAXT):
        for occ_last in (False, True):
            # the only acceptable line is the last one; held before the call, nothing is left (the others are 200 bits away)
            t, cs, ci, ys = ladder(hvo, nt, {nt - 1: (5, 0)}, occ_last)
            m, l = hqueries(hvo, [ys[nt - 1]] * 2, 1, 16.0)
            e = _exp([-1, -1] if occ_last else [nt - 1, -1], 5)
            c = make("nt_%d_last%s" % (nt, "_occupied" if occ_last else ""), t, cs, ci, map=m, last=l, expect={"map": e, "last": e})
            assert model_map(c)[3].ncand[0] >= (3 if nt < 100 else 65) - occ_last
            out.append(c)
    # claims on every line of the last occupancy word: lines 2016 .. 2047 at distances 10 + 2 (2047 - j), octaves alternating; 34 blocking
    # queries on line 2032 take 2047, 2046, ... 2016, then nothing
    good = {j: (10 + 2 * (MAXT - 1 - j), j % 2) for j in range(MAXT - 32, MAXT)}
    want = list(range(MAXT - 1, MAXT - 33, -1))
    t, cs, ci, ys = ladder(hvo, MAXT, good)
    m, l = hqueries(hvo, [ys[MAXT - 16]] * 34, 1, 16.0)
    e = _exp(want + [-1, -1], [good[j][0] for j in want] + [256, 256])
    c = make("nt_2048_last_word", t, cs, ci, map=m, last=l, expect={"map": e, "last": e}, local=NS(th=2.0, nslots=34, occ=(), good=sorted(good)))
    _, _, _, st = model_map(c)
    assert np.all(st.ncand >= 64) and st.fallback.tolist() == [False] * 3 + [True] * 31 and {j >> 5 for j in want} == {MAXT // 32 - 1}
    out.append(c)
    out += [ring(hvo, nq) for nq in (0, 1, 64, 65, 129, MAXQ)]
    return out


# ------------------------------------------------------------------------------------------------ windows
def window_cases(hvo):
    out = []
    dt = hvo.KEYLINE_DT

    def free(name, kl, fn, cells, q, idx, dist, r=8.0, bounds=B0, d=None, qkl=None, blocks=0, l3d=None):
        nq = len(q); q = np.asarray(q, np.float32)
        t = NS(kl=kl, fn=line_functions(kl) if fn is None else np.asarray(fn, np.float64), l3d=lines3d(hvo.LINE3D_DT, kl) if l3d is None else l3d,
               desc=descs(np.arange(len(kl)) + 1 if d is None else d), occ=None)
        cs, ci = ref.grid_from_cells(cells)
        blocks = np.broadcast_to(np.asarray(blocks, np.uint8), (nq,)).copy()
        m = NS(q=q, vc=np.full(nq, VC_WIDE), wvec=np.zeros((nq, 3)), desc=np.zeros((nq, 32), np.uint8), blocks=blocks, th=r / 8.0, nn_ratio=0.95)   # (zero world vector: the 3-D gate passes)
        l = NS(q=q, kl=keylines(dt, q[:, 0], q[:, 1], q[:, 2], q[:, 3]) if qkl is None else qkl, desc=m.desc, blocks=blocks, th=r)
        c = make(name, t, cs, ci, bounds=bounds, map=m, last=l, expect={"map": _exp(idx, dist), "last": _exp(idx, dist)})
        out.append(c)
        return c

    # each of lsbp_window's four `continue` branches, taken by the START sample of a query whose later samples find a line: left of the grid,
    # right of it (as the end sample), above, below; and a query with all three samples outside
    kl = keylines(dt, [-50.0, 590.0, 100.0, 300.0], [100.0, 200.0, -50.0, 430.0], [50.0, 700.0, 100.0, 300.0], [100.0, 200.0, 50.0, 530.0])
    kl["length"] = 100.0
    cells = {(0, 10): [0], (59, 20): [1], (10, 0): [2], (30, 43): [3]}
    q = [[-50.0, 100.0, 50.0, 100.0], [700.0, 200.0, 590.0, 200.0], [100.0, -50.0, 100.0, 50.0], [300.0, 530.0, 300.0, 430.0], [700.0, 530.0, 800.0, 530.0]]
    c = free("window_off_each_edge", kl, None, cells, q, [0, 1, 2, 3, -1], [1, 2, 3, 4, 256])
    c.last.kl["length"] = 100.0
    taken = [window_cells(B0, q_[0], q_[1], 8.0) for q_ in q]
    assert taken == [2, 1, 4, 3, 1], taken
    assert all(isinstance(window_cells(B0, *samples(q_)[2], 8.0), tuple) for q_ in q[:4])

    # bounds with a non-zero minimum: the window subtracts the minimum, the grid assignment (Frame::AssignFeaturesToGridForLine) does not.
    # Line 0 (distance 5) sits where that assignment puts x = 100 -- column 9 -- which the start sample's window, columns 10 .. 12, does not
    # reach; line 1 (distance 30) is listed in column 10 and is what the query finds
    kl = keylines(dt, [100.0, 100.0], [100.0, 100.0], [200.0, 200.0], [100.0, 100.0])
    invW = F(64) / F(B1[1] - B1[0]); invH = F(48) / F(B1[3] - B1[2])
    assert int(F(100.0) * invW) == 9 and int(F(100.0) * invH) == 9
    assert window_cells(B1, 100.0, 100.0, 8.0) == (10, 12, 9, 12) and window_cells(B1, 150.0, 100.0, 8.0)[0] > 10
    assert window_cells(np.array([0, B1[1] - B1[0], 0, B1[3] - B1[2]]), 100.0, 100.0, 8.0)[0] <= 9         # without the minimum it would be reached
    free("window_minimum_bounds", kl, None, {(9, 9): [0], (10, 9): [1]}, [[100.0, 100.0, 200.0, 100.0]], [1], [30], bounds=B1, d=[5, 30])

    # a radius that covers the whole grid: lines in the four corner cells and one in the middle, all parallel to the query; five blocking
    # queries take them by distance (octaves alternate)
    kl = keylines(dt, [0.0, 600.0, 0.0, 600.0, 300.0], [5.0, 5.0, 475.0, 475.0, 200.0], [40.0, 640.0, 40.0, 640.0, 340.0], [5.0, 5.0, 475.0, 475.0, 200.0],
                  octave=[0, 1, 1, 0, 1])
    kl["length"] = 100.0
    cells = {(0, 0): [0], (60, 0): [1], (0, 47): [2], (63, 47): [3], (30, 20): [4]}
    c = free("window_whole_grid", kl, None, cells, [[100.0, 100.0, 200.0, 100.0]] * 6, [3, 0, 4, 1, 2, -1], [10, 20, 30, 40, 50, 256], r=1600.0,
             d=[20, 40, 50, 10, 30], blocks=1)
    assert window_cells(B0, 100.0, 100.0, 1600.0) == (0, 63, 0, 47)

    # a zero-length CURRENT line: its direction is 0 / 0, the NaN passes the direction gate, and its line function decides.  Line 1 is at right
    # angles to the query and fails.  (Both pass the other gates: in-octave end points and lengths are written by hand.)
    kl = keylines(dt, [150.0, 150.0], [100.0, 100.0], [150.0, 150.0], [100.0, 200.0])
    for f, v in (("sox", 0.0), ("soy", 0.0), ("eox", 100.0), ("eoy", 0.0), ("length", 100.0)): kl[f] = v
    free("window_zero_length_line", kl, [[0.0, 1.0, -100.0], [0.0, 1.0, -100.0]], {(15, 10): [1, 0]}, [[100.0, 100.0, 200.0, 100.0]], [0], [1])
    # a zero-length QUERY: every current line passes the direction gate, the line at right angles to everything else included
    kl = keylines(dt, [150.0], [50.0], [150.0], [150.0])
    qkl = keylines(dt, [150.0], [50.0], [150.0], [150.0])
    free("window_zero_length_query", kl, None, {(15, 10): [0]}, [[150.0, 100.0, 150.0, 100.0]], [0], [1], qkl=qkl)
    return out


# ------------------------------------------------------------------------------------------------ the frame-to-frame search's boundary values
def last_boundaries(hvo):
    """independent pairs (one current line and its query, 30 px apart from the next pair), radius th = 4; then a claim chain in `args_last` form"""
    dt = hvo.KEYLINE_DT
    R = 4.0
    P = []                                                       # (current line fields, line function or None, query xyxy, query key line fields, distance, found)

    def pair(what, found, t=None, fn=None, q=None, qk=None, d=10):
        y = 53.0 + 30.0 * len(P)
        tk = dict(sx=300.0, sy=y, ex=400.0, ey=y, sox=0.0, soy=0.0, eox=100.0, eoy=0.0, length=100.0); tk.update(t(y) if t else {})
        qq = [300.0, y, 400.0, y] if q is None else q(y)
        qf = dict(sox=0.0, soy=0.0, eox=100.0, eoy=0.0, length=100.0); qf.update(qk or {})
        P.append(NS(what=what, t=tk, fn=fn, q=qq, qk=qf, d=d, found=found, y=y))

    pair("|dist| = r: outside", False, q=lambda y: [300.0, y + R, 400.0, y + R])
    pair("|dist| one float below r", True, q=lambda y: [300.0, float(np.nextafter(F(y + R), F(0.0))), 400.0, float(np.nextafter(F(y + R), F(0.0)))])
    pair("|cos| = 0.96f: inside", True, t=lambda y: dict(ex=324.0, ey=y + 7.0), q=lambda y: [300.0, y, 324.0, y])      # (24, 7) / 25
    cos_t = lambda dy: F(F(24.0) / np.sqrt(F(F(576.0) + F(F(F(150.0) + F(dy)) - F(143.0)) ** 2)))        # (this pair sits at y = 143)
    dy = next(k * 2.0 ** -16 for k in range(1, 400) if cos_t(k * 2.0 ** -16) < F(0.96))
    assert len(P) == 3
    pair("|cos| below 0.96f", False, t=lambda y: dict(ex=324.0, ey=float(F(F(y + 7.0) + F(dy)))), q=lambda y: [300.0, y, 324.0, y])
    pair("length ratio 0.75", True, t=lambda y: dict(length=75.0))
    pair("length ratio below 0.75", False, t=lambda y: dict(length=float(np.nextafter(F(75.0), F(0.0)))))
    pair("length ratio 0.75, query the shorter", True, qk=dict(length=75.0))
    for deg, found in ((9.99, True), (10.01, False)):
        a = np.radians(deg)
        pair("orientation %.2f degrees" % deg, found, t=lambda y: dict(eox=100.0 * np.cos(a), eoy=100.0 * np.sin(a)))
    pair("distance 95", True, d=95)
    pair("distance 96", False, d=96)
    # the start sample fails the distance test and the end sample passes, and the reverse: slope 0.1 through the query's end / start (long queries)
    pair("start fails, end passes", True, t=lambda y: dict(sy=y - 20.0, ex=500.0), q=lambda y: [300.0, y, 500.0, y])
    pair("start passes, end fails", True, t=lambda y: dict(ey=y + 20.0, ex=500.0), q=lambda y: [300.0, y, 500.0, y])
    n = len(P)
    kl = np.zeros(n, dt); qkl = np.zeros(n, dt)
    for i, p in enumerate(P):
        for f, v in p.t.items(): kl[f][i] = v
        for f, v in p.qk.items(): qkl[f][i] = v
    q = np.array([p.q for p in P], np.float32)
    fn = line_functions(kl)
    cells = {}
    for i, p in enumerate(P):
        for ix in {30, int(p.t["ex"] // 10)}: cells.setdefault((ix, int(p.y // 10)), []).append(i)
    cs, ci = ref.grid_from_cells(cells)
    d = [p.d for p in P]
    t = NS(kl=kl, fn=fn, l3d=np.zeros(n, hvo.LINE3D_DT), desc=descs(d), occ=None)
    l = NS(q=q, kl=qkl, desc=np.zeros((n, 32), np.uint8), blocks=np.zeros(n, np.uint8), th=R)
    idx = [i if p.found else -1 for i, p in enumerate(P)]
    c = make("last_boundaries", t, cs, ci, last=l, expect={"last": _exp(idx, d)}, what=[p.what for p in P])
    # the properties the names claim, in the kernel's arithmetic
    dirs = ref.line_directions(kl)
    assert F(abs(F(-1.0) * dirs[0][2])) == F(0.96) and F(abs(F(-1.0) * dirs[0][3])) < F(0.96) and F(abs(F(-1.0) * dirs[0][3])) > F(0.9599)
    dist = lambda i, s: abs(float(F(fn[i] @ np.array([float(samples(q[i])[s][0]), float(samples(q[i])[s][1]), 1.0]))))
    assert dist(0, 0) == R and R - 1e-5 < dist(1, 0) < R
    assert float(F(F(75.0) / F(100.0))) == 0.75 and float(F(kl["length"][5] / F(100.0))) < 0.75
    assert angle2d(kl[7], qkl[7]) > COS10 > angle2d(kl[8], qkl[8])
    assert [dist(11, s) < R for s in range(3)] == [False, False, True] and [dist(12, s) < R for s in range(3)] == [True, False, False]
    assert model_last(c)[3].tolist() == [int(p.found or p.d == 96) for p in P]
    return c


def last_chain(hvo):
    """the claim chain in the frame-to-frame search: the twelve lines of the chain cases, lines 1 and 5 held before the call, queries that block,
    do not block and block again; 95 is accepted, and a thirteenth line at 96 never is"""
    d = CHAIN_D + [96]
    occ = np.zeros(13, np.uint8); occ[[1, 5]] = 1
    t, cs, ci = hframe(hvo, 100.0 + 0.25 * np.arange(13), d, occ=occ)
    blocks = [1, 0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1]
    m, l = hqueries(hvo, [101.5] * len(blocks), blocks, 8.0)
    R = CHAIN_RANK
    idx = [R[k] for k in (1, 3, 3, 3, 4, 5, 6, 7, 8, 9, 10, 11)] + [-1, -1]
    return make("last_chain", t, cs, ci, last=l, expect={"last": _exp(idx, [d[j] if j >= 0 else 256 for j in idx])})


# ------------------------------------------------------------------------------------------------ hvo_match_lines_geom
def geom_case(hvo, n_last, with_has_ml):
    """pair i1 <-> i2 = n_cur - 1 - i1 fixed by hand: the current descriptor i2 is a copy of the last frame's i1 (distance 0), every other one at
    least 64 bits away.  Entries 0 .. 11 are the gate's boundary values, the rest alternate: i1 % 3 == 0 fails the position gate"""
    dt = hvo.KEYLINE_DT
    n_cur = n_last + 3
    pool = np.random.RandomState(0x11E5).randint(0, 256, (n_cur, 32)).astype(np.uint8)
    H = _ham_rows(pool, pool); H[np.arange(n_cur), np.arange(n_cur)] = 256
    assert H.min() >= 64
    part = n_cur - 1 - np.arange(n_last)
    d_cur = pool; d_last = pool[part].copy()
    kl_last = np.zeros(n_last, dt); kl_cur = np.zeros(n_cur, dt)
    for kl in (kl_last, kl_cur):
        kl["sx"] = 1.0; kl["sox"] = 100.0; kl["soy"] = 100.0; kl["eox"] = 200.0; kl["eoy"] = 100.0
    has_ml = np.ones(n_last, np.uint8)
    m12 = part.astype(np.int32).copy(); acc = np.ones(n_last, np.uint8)
    up = lambda v: float(np.nextafter(F(v), F(np.inf)))

    def cur(i1, **f):
        for k, v in f.items(): kl_cur[k][part[i1]] = v

    def rejected(i1): m12[i1] = -1; acc[i1] = 0

    def left(i1): acc[i1] = 0                                   # not accepted, and the entry stays as matchNNR set it

    for i1 in range(1, 7): kl_last[i1]["sox"], kl_last[i1]["soy"], kl_last[i1]["eox"], kl_last[i1]["eoy"] = 0.0, 0.0, 100.0, 0.0
    cur(1, sox=64.0, soy=0.0, eox=200.0, eoy=0.0)                # the start point dW = 64 off, at equality ('>' is strict), the end point 100 off: accepted
    cur(2, sox=up(64.0), soy=0.0, eox=200.0, eoy=0.0); rejected(2)
    cur(3, sox=-100.0, soy=10.0, eox=100.0, eoy=0.0)             # start 100 px off, end point the same: accepted (2.9 degrees)
    cur(4, sox=0.0, soy=0.0, eox=200.0, eoy=10.0)                # start the same, end 100 px off: accepted
    cur(5, sox=0.0, soy=48.0, eox=200.0, eoy=48.0)               # dH = 48 at equality at the start, the end point 100 off
    cur(6, sox=0.0, soy=up(48.0), eox=200.0, eoy=up(48.0)); rejected(6)
    for i1, deg in ((7, 19.99), (8, 20.01)):
        a = np.radians(deg)
        cur(i1, eox=100.0 + 100.0 * np.cos(a), eoy=100.0 + 100.0 * np.sin(a))   # start point the same: the position gate passes
    rejected(8)
    cur(9, sx=0.0); left(9)                                      # startPointX == 0: passed over
    cur(10, sx=0.0, sox=400.0, eox=500.0); left(10)              # ... before the gates that would have reset the entry
    has_ml[11] = 0
    if with_has_ml: left(11)                                     # a last-frame line without a map line: passed over
    for i1 in range(12, n_last):
        if i1 % 3 == 0: cur(i1, sox=200.0, eox=300.0); rejected(i1)
        if with_has_ml and i1 % 5 == 0:
            has_ml[i1] = 0; m12[i1] = part[i1]; acc[i1] = 0
    assert angle2d(kl_cur[part[7]], kl_last[7]) > COS20 > angle2d(kl_cur[part[8]], kl_last[8])
    assert float(F(640.0) - F(0.0)) * 0.1 == 64.0 and float(F(480.0) - F(0.0)) * 0.1 == 48.0 and up(64.0) > 64.0
    c = NS(name="geom_%d%s" % (n_last, "_has_mapline" if with_has_ml else ""), t=None, cs=None, ci=None, bounds=B0, map=None, last=None, local=None,
           geom=NS(d_last=d_last, kl_last=kl_last, d_cur=d_cur, kl_cur=kl_cur, desc_th=0.9, has_ml=has_ml if with_has_ml else None),
           expect={"geom": (int(acc.sum()), m12, acc)}, props={})
    return c


# ------------------------------------------------------------------------------------------------ the resident map over a case's current frame
LOCAL_T = np.hstack([np.eye(3), np.array([[0.3], [-0.2], [0.5]])]).astype(np.float32)      # no rotation: a world vector is its camera-frame vector


def local_map(c):
    """the `add_frame_lines` idiom of tests/test_line_map_gpu.py over the case's crafted current frame: a map of c.local.nslots lines made from
    the frame's own 3-D lines (c.local.good, default every line of the window, in index order), observed as the case's queries block, all with the zero descriptor --
    so the queries of the frustum pass are the case's queries but for the height they sit at -- plus one observed slot per line of
    c.local.occ, held by that line before the call.  -> (M, Tcw, held)"""
    L = c.local; t = c.t
    good = list(getattr(L, "good", None) or np.flatnonzero(t.desc.any(axis=1) & (np.unpackbits(t.desc, axis=1).sum(axis=1) < 200)))
    n = L.nslots + len(L.occ)
    M, _ = lmr.make_map(n, "none", LOCAL_T, seed=3)
    T = LOCAL_T.astype(np.float64); R, tt = T[:, :3], T[:, 3]
    for k in range(L.nslots):
        i = good[k % len(good)]
        A, B = R.T @ (t.l3d["A"][i] - tt), R.T @ (t.l3d["B"][i] - tt)
        mid = 0.5 * (A + B); ow = -R.T @ tt; d = np.linalg.norm(mid - ow)
        M["pos"][k] = np.concatenate([A, B]); M["wvec"][k] = A - B; M["normal"][k] = (mid - ow) / d
        M["max_dist"][k] = np.float32(d * 2.03); M["min_dist"][k] = np.float32(d * 0.5)
    M["desc"][:] = 0; M["observed"][:] = 1; M["bad"][:] = 0
    M["observed"][: L.nslots] = c.map.blocks[: L.nslots]
    held = np.full(len(t.kl), -1, np.int32)
    for k, i in enumerate(L.occ): held[i] = L.nslots + k
    return M, LOCAL_T, held


# every case by name, written out: tests/test_line_search_edges.py checks the list against what build_all() returns
SCENES = ["dir_5deg", "dir_3deg", "nan_line3d", "nan_wvec", "gate3d_14_16_170_90_tilt", "radius_0998f_and_below", "th_1", "th_5", "best_95", "best_96",
          "ratio_50_52_oct00", "ratio_50_52_oct01", "ratio_50_52_oct22", "ratio_50_60", "ratio_single", "tie_same_octave", "tie_octaves_10",
          "claim_blocks", "claim_overwritten", "claim_overwritten_then_blocks", "occupied_passed_over", "claimed_best_leaves_next"]
CHAINS = ["chain_all1", "chain_exhaust", "chain_all0", "chain_alt", "chain_all1_occupied", "chain_alt_occupied"]
CASES = (["scene_" + s for s in SCENES] + ["count_0", "count_1", "count_2"] + ["count_%d_%s" % (n, p) for p in PLACE for n in COUNTS] + CHAINS
         + ["visit_tie_later_index_first", "visit_passes_from_middle", "visit_passes_at_end_only", "visit_three_cells", "visit_twice_in_a_cell", "visit_three_columns"]
         + ["nt_%d_last%s" % (nt, o) for nt in (63, 64, 65, 2048) for o in ("", "_occupied")] + ["nt_2048_last_word"]
         + ["nq_%d" % nq for nq in (0, 1, 64, 65, 129, 16384)]
         + ["window_off_each_edge", "window_minimum_bounds", "window_whole_grid", "window_zero_length_line", "window_zero_length_query"]
         + ["last_boundaries", "last_chain"] + ["geom_%d%s" % (n, h) for n in (255, 256, 257) for h in ("", "_has_mapline")])
LOCAL = [n for n in CASES if n in CHAINS or n in ("count_65_across", "count_130_across", "nt_2048_last_word")]


def build_all(hvo):
    cs = scene_cases(hvo) + crowd_cases(hvo) + chain_cases(hvo) + visit_cases(hvo) + size_cases(hvo) + window_cases(hvo)
    cs += [last_boundaries(hvo), last_chain(hvo)]
    cs += [geom_case(hvo, n, h) for n in (255, 256, 257) for h in (False, True)]
    out = {c.name: c for c in cs}
    assert len(out) == len(cs)
    return out
