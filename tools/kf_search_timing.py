#!/usr/bin/env python3
"""Times hvo_stream_search_by_projection_keyframe (ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist)) on one
resident synthetic 640 x 480 frame: 1000 key-frame entries per candidate, 1 and 5 candidates in one call, (th, ORBdist) = (10, 100): the two
kernel groups' device times (the projection prologue, the searches) and the whole call's wall time, each the median of repeated calls after
5 warm-up calls.  Seven entries in ten are the frame's own key points back-projected at 1 .. 4 m (camera = world) with up to 70 descriptor
bits flipped, searched under a pose a centimetre off; the rest are random points.

Beside it hvo_search_by_projection on host arrays with the six query arrays (u, v, radius, the level band, the angles) ALREADY computed and
the frame's key points and descriptors uploaded with the call: the path the call replaces with a host prologue that costs nothing, i.e. a
lower bound for it.

    python tools/kf_search_timing.py [--entries 1000] [--candidates 1,5] [--reps 50]
"""
import argparse
import importlib.util
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "a-low-texture-robust-hybrid-feature-based-visual-odometry_amd")
spec = importlib.util.spec_from_file_location("hvo_amd", os.path.join(PKG, "__init__.py"), submodule_search_locations=[PKG])
hvo = importlib.util.module_from_spec(spec); sys.modules["hvo_amd"] = hvo; spec.loader.exec_module(hvo)
from hvo_amd import synth  # noqa: E402

CAM = (535.4, 539.2, 320.1, 247.6, 40.0)
SF = np.cumprod(np.concatenate([[np.float32(1.0)], np.full(7, np.float32(1.2), np.float32)])).astype(np.float32)


def make_candidate(n, rng, kp, desc, dx):
    nt = len(kp)
    f = rng.permutation(nt)[np.arange(n) % nt]
    z = rng.uniform(1.0, 4.0, n)
    X = np.stack([(kp["x"][f] - CAM[2]) / CAM[0] * z, (kp["y"][f] - CAM[3]) / CAM[1] * z, z], 1)
    other = np.arange(n) % 10 >= 7
    X[other] = np.stack([rng.uniform(-2, 2, other.sum()), rng.uniform(-1.5, 1.5, other.sum()), rng.uniform(0.5, 4, other.sum())], 1)
    d = np.linalg.norm(X, axis=1)
    mx = d * 1.2 ** (kp["octave"][f] - 0.5)
    qd = desc[f].copy()
    for i in range(n):
        bits = np.unpackbits(qd[i]); bits[rng.choice(256, rng.randint(0, 71), replace=False)] ^= 1; qd[i] = np.packbits(bits)
    T = np.hstack([np.eye(3), [[dx], [0.0], [0.0]]]).astype(np.float32)
    occ = np.zeros(nt, np.uint8); occ[::17] = 1
    return dict(pos=X.astype(np.float32), skip=(np.arange(n) % 70 == 8).astype(np.uint8), max_dist=mx.astype(np.float32),
                min_dist=(mx / 1.2 ** 7).astype(np.float32), desc=qd, angle=((kp["angle"][f] + 40.0) % 360.0).astype(np.float32), Tcw=T, occupied=occ)


def median_ms(f, reps):
    for _ in range(5): f()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); f(); t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", type=int, default=1000); ap.add_argument("--candidates", default="1,5"); ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    g, _ = synth.make_frame("std", 0x5EED0002)
    st = hvo.Stream(depth=2, stages=hvo.STAGE_ORB, bf=0.0); ctx = hvo.Context()
    t = st.submit(g); out = st.collect(t); kp, desc = out["kp_un"], out["desc"]; nkp = len(kp)
    b = [float(v) for v in st.bounds]
    rng = np.random.RandomState(14)
    print("frame: %d key points, %d key-frame entries per candidate, (th, ORBdist) = (10, 100); times in ms, median of %d calls after 5 warm-up calls"
          % (nkp, a.entries, a.reps))
    print("%10s %8s %8s | %9s %9s | %8s || %22s" % ("candidates", "searched", "matches", "prologue", "search", "call", "hvo_search_by_projection"))
    for nc in (int(v) for v in a.candidates.split(",")):
        cs = [make_candidate(a.entries, rng, kp, desc, 0.01 * (j + 1)) for j in range(nc)]
        call = lambda: st.search_by_projection_keyframe(t, CAM, nkp, cs, th=10.0, orb_dist=100)
        r = call(); ks = []
        for _ in range(a.reps): ks.append(call()[0]["kernel_ms"])
        k = np.median(np.array(ks), axis=0)
        # the replaced path, its prologue free: the six query arrays as the new call's prologue decided them
        olds = []
        for c, rr in zip(cs, r):
            ok = rr["gate"] == 0; lv = np.where(ok, rr["level"], 0)
            olds.append((c["desc"], np.where(ok, rr["proj"][:, 0], np.float32(1e30)), np.where(ok, rr["proj"][:, 1], np.float32(1e30)),
                         np.where(ok, np.float32(10.0) * SF[lv], np.float32(0)), np.where(ok, lv - 1, 0), np.where(ok, lv + 1, -1), np.zeros(len(ok), np.float32),
                         c["angle"], np.ones(len(ok), np.uint8), kp, np.full(nkp, -1, np.float32), c["occupied"], desc, (b[0], b[2], b[1], b[3])))
        old = lambda: [ctx.search_by_projection(*o, th_high=100, check_orientation=True) for o in olds]
        o = old()
        for j in range(nc):
            if o[j][0] != r[j]["n_matches"] or not np.array_equal(o[j][1], r[j]["match_idx"]): print("# candidate %d: the replaced path matched %d" % (j, o[j][0]))
        print("%10d %8d %8d | %9.3f %9.3f | %8.3f || %22.3f" % (nc, sum(x["n_searched"] for x in r), sum(x["n_matches"] for x in r), k[0], k[1],
                                                           median_ms(call, a.reps), median_ms(old, a.reps)))
    st.close(); ctx.close()


if __name__ == "__main__":
    main()
