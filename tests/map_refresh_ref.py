"""CPU restatement of MapPoint::ComputeDistinctiveDescriptors + MapPoint::UpdateNormalAndDepth (reference src/MapPoint.cc:240-305, 328-369) and
MapLine::ComputeDistinctiveDescriptors + MapLine::UpdateAverageDir (src/MapLine.cpp:331-396, 404-455).  Test infrastructure only, and THE
DEFINITION of the readings csrc/map_refresh.hip states at its head: Python floats are IEEE doubles, f32() rounds to float (a double result of
+ - * / sqrt of two floats rounds to the same float as the float operation: 53 >= 2 * 24 + 2), one step per step of the reference.  The
descriptor half builds the real N x N matrix, sorts every row and indexes it as written.

Two readings have no precedent in the project, and neither OpenCV nor Eigen is in the reference tree, so they are CHOSEN here:
  * `cv::Mat MP = 0.5*(SP+EP)` on CV_32F: the MatExpr (SP + EP) scaled by 0.5 is evaluated as addWeighted(SP, 0.5, EP, 0.5):
    f32(SP * 0.5 + EP * 0.5) with the products and the sum in double, ONE rounding.  f32(f32(SP + EP) * 0.5) is the same float unless SP + EP
    overflows or the result is subnormal (halving is exact otherwise), so the choice shows only there.
  * Eigen's `normalize()` on a zero vector: taken as Eigen 3.3's `z = squaredNorm(); if (z > 0) *this /= sqrt(z)`: the zero vector (and a
    vector with a NaN) is left as it is.  Eigen 3.2 divides by norm() unconditionally and would give NaN.
The other readings follow tests/new_points_ref.py and tests/new_lines_ref.py: cv::norm is a double sum of squares left to right; Mat / scalar
multiplies by the double reciprocal and rounds to float; Eigen's squaredNorm is (x x + y y) + z z; the line scale table is sf[0] = 1,
sf[l] = sf[l - 1] * scale_factor in float, and the point table is the context's (point_map_ref.SF for the default pyramid).

Status (the first that applies): 0 refreshed, 1 skipped, 2 no observations, 3 descriptor kept (DESCRIPTOR asked for, every observer bad),
4 ref_level outside [0, n_levels) (GEOMETRY asked for; the distance range is left as it was, also under status 3).  An output entry that is
not written keeps the value of `prior` (default: UNTOUCHED everywhere, what the Python binding puts there)."""
import math

import numpy as np

import point_map_ref as pm

F32 = np.float32
DESCRIPTOR, GEOMETRY = 1, 2
REFRESHED, SKIPPED, NO_OBS, DESC_KEPT, BAD_LEVEL = range(5)
MAX_OBS, MAX_FEATURES, MAX_OBS_TOTAL = 256, 65536, 1 << 20
UNTOUCHED = 119
INT_MAX = 2 ** 31 - 1
KEYS_POINT = ("best_obs", "best_median", "desc", "normal", "max_dist", "min_dist", "status")
KEYS_LINE = KEYS_POINT + ("wvec",)
_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)
_ERR = dict(all="ignore")


def f32(x):
    return float(F32(x))


def ddiv(a, b):
    return float(np.float64(a) / np.float64(b))


def dsqrt(a):
    return float(np.sqrt(np.float64(a)))


def rank(N):
    """vDists[0.5 * (N - 1)]: the double product converted to size_t"""
    return int(0.5 * (N - 1))


def line_scale_factors(n_levels, scale_factor):
    sf = [1.0]
    for _ in range(1, n_levels): sf.append(f32(sf[-1] * f32(scale_factor)))
    return sf


def distance_matrix(rows):
    rows = np.asarray(rows, np.uint8).reshape(-1, 32)
    return _POP[rows[:, None, :] ^ rows[None, :, :]].sum(axis=2)


def distinctive(rows):
    """(BestIdx, BestMedian, tie) over the descriptor list: the matrix, every row sorted, `median < BestMedian`.  tie: the least median is
    reached by more than one row"""
    D = distance_matrix(rows)
    N = len(D)
    best_median, best = INT_MAX, 0
    medians = []
    for i in range(N):
        v = sorted(int(x) for x in D[i])
        median = v[rank(N)]
        medians.append(median)
        if median < best_median:
            best_median, best = median, i
    return best, best_median, medians.count(best_median) > 1


def point_geometry(P, Ows):
    """mNormalVector of UpdateNormalAndDepth: P and Ows hold float values"""
    s = [0.0, 0.0, 0.0]
    for O in Ows:
        d = [f32(P[c] - O[c]) for c in range(3)]
        nn = dsqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
        inv = ddiv(1.0, nn)
        s = [f32(s[c] + f32(d[c] * inv)) for c in range(3)]
    inn = ddiv(1.0, float(len(Ows)))
    return [f32(s[c] * inn) for c in range(3)]


def point_dist(P, Or):
    d = [f32(P[c] - Or[c]) for c in range(3)]
    return f32(dsqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]))


def line_geometry(P, Ows):
    """mNormalVector of UpdateAverageDir: P holds doubles, Ows float values"""
    mid = [0.5 * (P[c] + P[3 + c]) for c in range(3)]
    s = [0.0, 0.0, 0.0]
    for O in Ows:
        d = [mid[c] - O[c] for c in range(3)]
        nn = dsqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        s = [s[c] + ddiv(d[c], nn) for c in range(3)]
    return [ddiv(s[c], float(len(Ows))) for c in range(3)]


def line_dist(P, Or):
    cm = []
    for c in range(3):
        sp, ep = f32(P[c]), f32(P[3 + c])
        cm.append(f32(f32(sp * 0.5 + ep * 0.5) - Or[c]))
    return f32(dsqrt(cm[0] * cm[0] + cm[1] * cm[1] + cm[2] * cm[2]))


def world_vector(P):
    w = [P[c] - P[3 + c] for c in range(3)]
    z = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
    if z > 0.0:
        r = dsqrt(z)
        w = [ddiv(v, r) for v in w]
    return w


def _refresh(line, pos, obs, n_levels, sf, what, prior):
    st = np.asarray(obs["obs_start"], np.int64)
    n = len(st) - 1
    assert n <= MAX_FEATURES and (n == 0 or (np.diff(st).max() <= MAX_OBS and st[-1] <= MAX_OBS_TOTAL and st[0] == 0 and np.diff(st).min() >= 0))
    rdt = np.float64 if line else F32
    out = dict(best_obs=np.full(n, UNTOUCHED, np.int32), best_median=np.full(n, UNTOUCHED, np.int32), desc=np.full((n, 32), UNTOUCHED, np.uint8),
               normal=np.full((n, 3), UNTOUCHED, rdt), max_dist=np.full(n, UNTOUCHED, F32), min_dist=np.full(n, UNTOUCHED, F32), status=np.zeros(n, np.uint8))
    if line: out["wvec"] = np.full((n, 3), UNTOUCHED, np.float64)
    for k, v in (prior or {}).items():
        if k in out and k != "status": out[k] = np.array(v, out[k].dtype).reshape(out[k].shape).copy()
    tie = np.zeros(n, bool)
    desc = np.asarray(obs["obs_desc"], np.uint8).reshape(-1, 32); Ow = np.asarray(obs["obs_Ow"], F32).reshape(-1, 3)
    bad = np.zeros(len(desc), np.uint8) if obs.get("kf_bad") is None else np.asarray(obs["kf_bad"]).astype(bool)
    skip = np.zeros(n, bool) if obs.get("skip") is None else np.asarray(obs["skip"]).astype(bool)
    rOw = np.asarray(obs["ref_Ow"], F32).reshape(-1, 3); lvl = np.asarray(obs["ref_level"], np.int64)
    pos = np.asarray(pos, rdt).reshape(n, 6 if line else 3)
    with np.errstate(**_ERR):
        for f in range(n):
            a, b = int(st[f]), int(st[f + 1])
            out["best_obs"][f] = out["best_median"][f] = -1
            if skip[f]: out["status"][f] = SKIPPED; continue
            if a == b: out["status"][f] = NO_OBS; continue
            status = REFRESHED
            if what & DESCRIPTOR:
                good = [i for i in range(a, b) if not bad[i]]
                if not good: status = DESC_KEPT
                else:
                    bi, bm, tie[f] = distinctive(desc[good])
                    out["best_obs"][f] = good[bi] - a; out["best_median"][f] = bm; out["desc"][f] = desc[good[bi]]
            if what & GEOMETRY:
                P = [float(v) for v in pos[f]]; Os = [[float(v) for v in O] for O in Ow[a:b]]; Or = [float(v) for v in rOw[f]]
                out["normal"][f] = line_geometry(P, Os) if line else point_geometry(P, Os)
                if line: out["wvec"][f] = world_vector(P)
                if 0 <= lvl[f] < n_levels:
                    dist = line_dist(P, Or) if line else point_dist(P, Or)
                    mx = f32(dist * sf[int(lvl[f])])
                    out["max_dist"][f] = mx; out["min_dist"][f] = f32(ddiv(mx, sf[n_levels - 1]))
                elif status == REFRESHED: status = BAD_LEVEL
            out["status"][f] = status
    out["tie"] = tie
    return out


def refresh_points(pos, obs, n_levels=pm.N_LEVELS, what=DESCRIPTOR | GEOMETRY, sf=pm.SF, prior=None):
    return _refresh(False, pos, obs, n_levels, [float(v) for v in sf], what, prior)


def refresh_lines(pos, obs, n_levels=8, scale_factor=1.2, what=DESCRIPTOR | GEOMETRY, prior=None):
    return _refresh(True, pos, obs, n_levels, line_scale_factors(n_levels, scale_factor), what, prior)


# ---------------------------------------------------------------------------------------------------------------- inputs
def bits(k):
    """a descriptor with the first k bits set: the distance of bits(a) and bits(b) is |a - b|"""
    d = np.zeros(32, np.uint8)
    for i in range(k): d[i >> 3] |= 1 << (i & 7)
    return d


def on_a_line(values):
    return np.stack([bits(v) for v in values])


def make_obs(counts, rng, flips=24, bad_rate=0.0, level_hi=8):
    """ragged observations: per feature a random descriptor with up to `flips` bits flipped per observer, observers around the origin"""
    counts = np.asarray(counts, np.int64)
    n, no = len(counts), int(counts.sum())
    st = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    base = rng.randint(0, 256, (n, 32)).astype(np.uint8)
    desc = np.repeat(base, counts, axis=0)
    for i in range(no):
        for b in rng.randint(0, 256, rng.randint(0, flips + 1)): desc[i, b >> 3] ^= np.uint8(1 << (b & 7))
    return dict(obs_start=st, obs_desc=desc, obs_Ow=rng.uniform(-1.5, 1.5, (no, 3)).astype(F32), kf_bad=(rng.uniform(size=no) < bad_rate).astype(np.uint8),
                ref_Ow=rng.uniform(-1.5, 1.5, (n, 3)).astype(F32), ref_level=rng.randint(0, level_hi, n).astype(np.int32), skip=np.zeros(n, np.uint8))


def point_positions(n, rng):
    return np.column_stack([rng.uniform(-3, 3, n), rng.uniform(-2, 2, n), rng.uniform(2, 8, n)]).astype(F32)


def line_positions(n, rng):
    s = np.column_stack([rng.uniform(-3, 3, n), rng.uniform(-2, 2, n), rng.uniform(2, 8, n)])
    return np.concatenate([s, s + rng.uniform(-1, 1, (n, 3))], axis=1)


def plant_statuses(obs, rng):
    """features 0 .. 11 of a scene with at least 12: three each of skipped, every observer bad, a level outside the table; the empty ones
    come from the counts"""
    st = obs["obs_start"]
    obs["skip"][[0, 1, 2]] = 1
    for f in (3, 4, 5): obs["kf_bad"][st[f]:st[f + 1]] = 1
    obs["ref_level"][[6, 7, 8]] = (-1, 8, 1000)
    return obs


def random_scene(line, n, seed, max_obs=40):
    """n features with 1 .. max_obs observations (every 29th none), a tenth of the observers bad, every status planted"""
    rng = np.random.RandomState(seed)
    counts = rng.randint(1, max_obs + 1, n); counts[9::29] = 0
    obs = plant_statuses(make_obs(counts, rng, bad_rate=0.1), rng)
    return (line_positions(n, rng) if line else point_positions(n, rng)), obs


SCENE_POINTS = dict(line=False, n=300, seed=71)
SCENE_LINES = dict(line=True, n=100, seed=72)
