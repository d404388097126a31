"""CPU restatement of the local-map line search, LSDmatcher::SearchByProjection(F, vpMapLines, eval_orient, th) (reference
src/LSDmatcher.cpp:709-801, RadiusByViewingCos 1436-1442), over Frame::GetFeaturesInAreaForLine with its defaults (src/Frame.cc:1557-1627,
include/Frame.h:131: TH = 0.998).  Test infrastructure only: numpy float32 / float64, one step per step of the reference, written from its
semantics.  Eigen's dot product of two Vector3d is taken as ((x x') + (y y')) + z z'.

Inputs are those of hvo_search_lines_by_projection_map: per query q_xyxy (mTrackProjX1/Y1/X2/Y2), q_view_cos (mTrackViewCos), q_wvec
(GetWorldVector()), q_desc (GetDescriptor()), q_blocks (Observations() > 0); per current line t_kl (mvKeylinesUn), t_fn (mvKeyLineFunctions),
t_l3d (mvLines3D: fields A, B), t_desc (mLdesc), t_occupied (holds a map line with observations); the line grid as CSR (cell ix * 48 + iy)."""
import math

import numpy as np

F32 = np.float32
GRID_COLS, GRID_ROWS = 64, 48
TH_NORMAL = math.cos(15.0 / 180.0 * math.pi)        # th_normal of LSDmatcher.cpp:713-715, in double


def radius_by_viewing_cos(view_cos, th):
    """RadiusByViewingCos (a float against the double 0.998), times th only when th != 1.0 (LSDmatcher.cpp:731-734); not scaled by level"""
    r = F32(5.0) if float(F32(view_cos)) > 0.998 else F32(8.0)
    if float(F32(th)) != 1.0:
        r = F32(r * F32(th))
    return r


def line_directions(t_kl):
    """the unit directions (start - end) of the current lines in float32, as GetFeaturesInAreaForLine computes them per visit"""
    with np.errstate(invalid="ignore", divide="ignore"):
        dx = (t_kl["sx"].astype(np.float32) - t_kl["ex"].astype(np.float32)).astype(np.float32)
        dy = (t_kl["sy"].astype(np.float32) - t_kl["ey"].astype(np.float32)).astype(np.float32)
        n = np.sqrt((dx * dx + dy * dy).astype(np.float32)).astype(np.float32)
        return (dx / n).astype(np.float32), (dy / n).astype(np.float32)


def features_in_area_for_line(x1, y1, x2, y2, r, t_kl, t_fn, cell_start, cell_items, bounds4, TH=F32(0.998), dirs=None):
    """Frame::GetFeaturesInAreaForLine: the window's lines in the order of their first passing visit (sample points start / middle / end,
    cells ix-major, a cell's lines in insertion order).  minLevel / maxLevel are not read.  dirs: line_directions(t_kl), if already computed."""
    d2xs, d2ys = line_directions(t_kl) if dirs is None else dirs
    x1, y1, x2, y2, r = F32(x1), F32(y1), F32(x2), F32(y2), F32(r)
    minX, maxX, minY, maxY = (F32(v) for v in bounds4)
    xs = (x1, F32(float(F32(x1 + x2)) / 2.0), x2)
    ys = (y1, F32(float(F32(y1 + y2)) / 2.0), y2)
    invW = F32(F32(GRID_COLS) / F32(maxX - minX)); invH = F32(F32(GRID_ROWS) / F32(maxY - minY))
    out, seen = [], set()
    with np.errstate(invalid="ignore", divide="ignore"):
        d1x = F32(x1 - x2); d1y = F32(y1 - y2)
        n1 = F32(np.sqrt(F32(F32(d1x * d1x) + F32(d1y * d1y))))
        d1x = F32(d1x / n1); d1y = F32(d1y / n1)
        for i in range(3):
            x, y = xs[i], ys[i]
            cx0 = max(0, int(np.floor(F32(F32(F32(x - minX) - r) * invW))))
            if cx0 >= GRID_COLS: continue
            cx1 = min(GRID_COLS - 1, int(np.ceil(F32(F32(F32(x - minX) + r) * invW))))
            if cx1 < 0: continue
            cy0 = max(0, int(np.floor(F32(F32(F32(y - minY) - r) * invH))))
            if cy0 >= GRID_ROWS: continue
            cy1 = min(GRID_ROWS - 1, int(np.ceil(F32(F32(F32(y - minY) + r) * invH))))
            if cy1 < 0: continue
            for ix in range(cx0, cx1 + 1):
                for iy in range(cy0, cy1 + 1):
                    c = ix * GRID_ROWS + iy
                    for k in range(int(cell_start[c]), int(cell_start[c + 1])):
                        j = int(cell_items[k])
                        if j in seen: continue
                        d2x, d2y = d2xs[j], d2ys[j]
                        cs = F32(abs(F32(F32(d1x * d2x) + F32(d1y * d2y))))
                        if cs < TH: continue                              # a NaN passes
                        fn = t_fn[j]
                        dist = F32(float(fn[0]) * float(x) + float(fn[1]) * float(y) + float(fn[2]))
                        if abs(dist) < r:
                            out.append(j); seen.add(j)
    return out


def angle_3d(A, B, wvec):
    """|cos| between the frame line's A - B (camera frame) and the map line's world vector, as the reference rounds it (LSDmatcher.cpp:760-769)"""
    vx, vy, vz = float(A[0]) - float(B[0]), float(A[1]) - float(B[1]), float(A[2]) - float(B[2])
    wx, wy, wz = (float(v) for v in wvec)
    dot = F32((vx * wx + vy * wy) + vz * wz)
    mag_f = F32(math.sqrt(vx * vx + vy * vy + vz * vz)); mag_ml = F32(math.sqrt(wx * wx + wy * wy + wz * wz))
    with np.errstate(invalid="ignore", divide="ignore"):
        return F32(abs(F32(dot / F32(mag_f * mag_ml))))


def hamming(a, b):
    return int(np.unpackbits(np.bitwise_xor(np.asarray(a, np.uint8), np.asarray(b, np.uint8))).sum())


def search_lines_by_projection_map(q_xyxy, q_view_cos, q_wvec, q_desc, q_blocks, t_kl, t_fn, t_l3d, t_desc, t_occupied, cell_start, cell_items,
                                   bounds4, th=1.0, nn_ratio=0.95):
    """-> (nmatches, match_idx, match_dist), match_idx[q] = the line assigned F.mvpMapLines[idx] = pML, or -1"""
    q_xyxy = np.asarray(q_xyxy, np.float32).reshape(-1, 4); nq = len(q_xyxy); nt = len(t_kl)
    holder_obs = np.zeros(nt, bool) if t_occupied is None else np.asarray(t_occupied).astype(bool).copy()
    blocks = np.zeros(nq, bool) if q_blocks is None else np.asarray(q_blocks).astype(bool)
    idx = np.full(nq, -1, np.int32); dist_out = np.full(nq, 256, np.int32)
    nn_ratio = F32(nn_ratio); nm = 0
    dirs = line_directions(t_kl) if nt else None
    for q in range(nq):
        r = radius_by_viewing_cos(q_view_cos[q], th)
        cand = features_in_area_for_line(*q_xyxy[q], r, t_kl, t_fn, cell_start, cell_items, bounds4, dirs=dirs) if nt else []
        if not cand: continue
        bestDist, bestLevel, bestDist2, bestLevel2, bestIdx = 256, -1, 256, -1, -1
        for j in cand:
            if holder_obs[j]: continue                                    # F.mvpMapLines[idx]->Observations() > 0
            ang = angle_3d(t_l3d[j]["A"], t_l3d[j]["B"], q_wvec[q])
            if float(ang) < TH_NORMAL: continue                           # a NaN passes
            d = hamming(q_desc[q], t_desc[j])
            if d < bestDist:
                bestDist2, bestDist, bestLevel2, bestLevel, bestIdx = bestDist, d, bestLevel, int(t_kl[j]["octave"]), j
            elif d < bestDist2:
                bestLevel2, bestDist2 = int(t_kl[j]["octave"]), d
        if bestDist <= 95:
            if bestLevel == bestLevel2 and F32(bestDist) > F32(nn_ratio * F32(bestDist2)):
                continue
            idx[q] = bestIdx; dist_out[q] = bestDist
            holder_obs[bestIdx] = blocks[q]                               # F.mvpMapLines[bestIdx] = pML
            nm += 1
    return nm, idx, dist_out


def grid_from_cells(cells):
    """a line grid in CSR form from {(ix, iy): [line, ...]} (insertion order kept)"""
    start = np.zeros(GRID_COLS * GRID_ROWS + 1, np.int32); items = []
    for c in range(GRID_COLS * GRID_ROWS):
        start[c] = len(items)
        items += list(cells.get((c // GRID_ROWS, c % GRID_ROWS), []))
    start[-1] = len(items)
    return start, np.array(items, np.int32)
