#!/usr/bin/env python3
"""Times hvo_stream_create_keyframe_features (Tracking::CreateNewKeyFrame's new map points and map lines, written into the resident point
map and line map) on one synthetic 640 x 480 frame extracted with 1000 and with 2000 ORB features and 200 key lines: the whole call's wall
time and the device time of its launches, each the median of repeated calls after warm-up.  Every call starts from empty maps of
sufficient capacity and nothing held, with thDepth above every depth, so every feature with depth is made.

Beside it, the path the call replaces, in its three parts: collect() of the finished frame (the copy of its arrays out of the stream's pinned
block into the caller's), the loops of Tracking::CreateNewKeyFrame on the host (tools/new_keyframe_host.cpp, plain single-thread C++,
g++ -O2, on the same arrays and pose) and set_many of both maps with what the loops made.

    python tools/new_keyframe_timing.py [--features 1000,2000] [--reps 50]
"""
import argparse
import importlib.util
import os
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "a-low-texture-robust-hybrid-feature-based-visual-odometry_amd")
spec = importlib.util.spec_from_file_location("hvo_amd", os.path.join(PKG, "__init__.py"), submodule_search_locations=[PKG])
hvo = importlib.util.module_from_spec(spec); sys.modules["hvo_amd"] = hvo; spec.loader.exec_module(hvo)
from hvo_amd import synth  # noqa: E402

CAM = (535.4, 539.2, 320.1, 247.6, 40.0)
TH = 100.0


def host_loops_ms(out, T, calls):
    exe = os.path.join(ROOT, "tools", "new_keyframe_host")
    if not os.path.exists(exe):
        subprocess.check_call(["g++", "-O2", "-std=c++14", os.path.join(ROOT, "tools", "new_keyframe_host.cpp"), "-o", exe])
    n_kp, n_kl = len(out["kp_un"]), len(out["kl"])
    P = np.zeros(n_kp, np.dtype([("u", "<f4"), ("v", "<f4"), ("z", "<f4"), ("octave", "<i4"), ("held", "<i4")]))
    P["u"] = out["kp_un"]["x"]; P["v"] = out["kp_un"]["y"]; P["z"] = out["zdepth"]; P["octave"] = out["kp_un"]["octave"]; P["held"] = -1
    L = np.zeros(n_kl, np.dtype([("A", "<f8", 3), ("B", "<f8", 3), ("held", "<i4"), ("pad", "<i4")]))
    L["A"] = out["lines3d"]["A"]; L["B"] = out["lines3d"]["B"]; L["held"] = -1
    with tempfile.NamedTemporaryFile(suffix=".bin") as f:
        f.write(struct.pack("<ii", n_kp, n_kl) + np.array(list(CAM[:4]) + [TH], np.float32).tobytes() + np.asarray(T, np.float32).tobytes() + P.tobytes() + L.tobytes())
        f.flush()
        ms, npt, nln = subprocess.check_output([exe, f.name, str(calls)]).decode().split()
    return float(ms), int(npt), int(nln)


def median_ms(f, reps, warm=5):
    for _ in range(warm): f()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); f(); t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--features", default="1000,2000"); ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    g, d = synth.make_frame("std", 0x5EED0002)
    T = np.array([[1, 0, 0, 0.25], [0, 1, 0, -0.125], [0, 0, 1, 0.5]], np.float32)
    stages = hvo.STAGE_ORB | hvo.STAGE_LSD | hvo.STAGE_LINES3D
    print("times in ms, median of %d calls after warm-up; thDepth above every depth, nothing held, empty maps" % a.reps)
    print("%8s %6s %6s %7s %7s | %8s %8s || %8s %10s %9s | %8s" % ("features", "points", "lines", "new pts", "new lns", "call", "kernels", "collect", "host loops", "set_many", "replaced"))
    for nf in (int(v) for v in a.features.split(",")):
        st = hvo.Stream(depth=2, stages=stages, bf=CAM[4], orb_nfeatures=nf, lsd_nfeatures=200)
        kfi = hvo.KeyFrameInsert(); pm = hvo.PointMap(slots=4096); lm = hvo.LineMap(slots=512)
        t = st.submit(g, d); out = st.collect(t); n_kp, n_kl = len(out["kp_un"]), len(out["kl"])
        kms = []

        def call():
            # empty maps each time: the slots are simply written again
            r = st.create_keyframe_features(kfi, pm, lm, t, CAM, T, n_kp, n_kl, th_depth=TH, first_point_slot=0, first_line_slot=0, line_n_levels=8)
            kms.append(r.kernel_ms)
            return r
        r = call()
        c_ms = median_ms(call, a.reps); k_ms = float(np.median(kms[-a.reps:]))
        # the replaced path
        col = []
        for _ in range(a.reps + 5):
            t2 = st.submit(g, d)
            while not st.poll(t2): pass
            t0 = time.perf_counter(); st.collect(t2); col.append((time.perf_counter() - t0) * 1e3)
        col_ms = float(np.median(col[5:]))
        h_ms, hp, hl = host_loops_ms(out, T, a.reps)
        if (hp, hl) != (r.n_points_created, r.n_lines_created): print("# host loops made %d points and %d lines" % (hp, hl))
        pm2 = hvo.PointMap(slots=4096); lm2 = hvo.LineMap(slots=512)
        desc = out["desc"][r.pt_index]; ld = out["ldesc"][r.ln_index]

        def set_many():
            pm2.set_many(0, r.pt_pos, r.pt_normal, r.pt_max_dist, r.pt_min_dist, desc)
            if len(r.ln_index): lm2.set_many(0, r.ln_pos, r.ln_wvec, r.ln_normal, r.ln_max_dist, r.ln_min_dist, ld)
        s_ms = median_ms(set_many, a.reps)
        print("%8d %6d %6d %7d %7d | %8.3f %8.3f || %8.3f %10.3f %9.3f | %8.3f" % (nf, n_kp, n_kl, r.n_points_created, r.n_lines_created, c_ms, k_ms, col_ms, h_ms, s_ms,
                                                                                 col_ms + h_ms + s_ms))
        for m in (pm, lm, pm2, lm2): m.close()
        kfi.close(); st.close()


if __name__ == "__main__":
    main()
