#!/usr/bin/env python3
"""Times ORBmatcher::Fuse on the device (csrc/fuse.hip) for the two calls of LocalMapping::SearchInNeighbors:

  arrays   hvo_fuse_points: 1000 entries (one shared map side) x 30 key frames of 1000 features, on host arrays
  slots    hvo_fuse_points_slots: the same, the map side as 1000 slots of a resident point map
  stream   hvo_stream_fuse_points: one resident frame as the key frame, 30 000 candidates as slots of a resident point map

Per case: the three kernel groups' device times (hipEvents: grid, projection, search + compaction) and the whole call's wall time, medians of
repeated calls after 5 warm-up calls.  Beside them tools/fuse_host.cpp, a plain single-thread host restatement with real cell lists and one
call per key frame, built with g++ -O2 here and run on the same inputs (the stream case on the downloaded frame); its answer is compared
with the device's.  The key frames are tests/fuse_ref.py's random scene (five entries in eight are a feature's point under a pose 2 mm off).

    python tools/fuse_timing.py [--reps 30] [--out profiles/fuse.txt]
"""
import argparse
import importlib.util
import os
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
sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))
import fuse_ref as ref  # noqa: E402
import point_map_ref as pm  # noqa: E402
import fuse_host_io as io  # noqa: E402


def median_ms(f, reps):
    for _ in range(5): f()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); f(); t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def kernel_ms(f, reps):
    return np.median(np.array([f()[0]["kernel_ms"] for _ in range(reps)]), axis=0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30); ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s); lines.append(s)
    tmp = tempfile.mkdtemp()
    exe = os.path.join(tmp, "fuse_host")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-ffp-contract=off", os.path.join(ROOT, "tools", "fuse_host.cpp"), "-o", exe])
    ctx = hvo.Context(max_batch=1)
    dt = hvo.KEYPOINT_DT
    say("%-8s %9s %9s %8s | %8s %10s %8s | %8s || %10s %10s  %s" % ("case", "keyframes", "entries", "fused", "grid", "projection", "search", "call", "host grid", "host fuse", "same answer"))

    def host(kfs, mp):
        t = []
        r = io.run(exe, tmp, kfs, mp, pm.CAM, pm.BOUNDS, pm.SF, ref.INV_SIGMA2, ref.TH, ref.TH_LOW, pm.LOG_SF, pm.N_LEVELS, reps=max(3, a.reps // 3), times=t)
        return r, t

    def row(name, call, kfs, mp):
        r = call()
        k = kernel_ms(call, a.reps)
        hr, ht = host(kfs, mp)
        ok = all(np.array_equal(r[j]["best_idx"], hr[j]["best_idx"]) and np.array_equal(r[j]["best_dist"], hr[j]["best_dist"]) for j in range(len(kfs)))
        say("%-8s %9d %9d %8d | %8.3f %10.3f %8.3f | %8.3f || %10.3f %10.3f  %s" % (name, len(kfs), len(mp["pos"]), sum(x["n_fused"] for x in r), k[0], k[1], k[2],
                                                                                   median_ms(call, a.reps), ht[0], ht[1], "yes" if ok else "NO"))

    # the first loop: one map side, 30 target key frames
    _, mp = ref.random_scene(dt, 1000, 1000, seed=40)
    kfs = []
    for j in range(30):
        kf, _ = ref.random_scene(dt, 1000, 1000, seed=40, pose_dx=0.0002 * j)
        kf["skip"] = ((np.arange(1000) + j) % 11 == 0).astype(np.uint8)
        kfs.append(kf)
    row("arrays", lambda: ctx.fuse_points(pm.CAM, kfs, mp, pm.BOUNDS), kfs, mp)
    m = hvo.PointMap(0, 1000)
    m.set_many(0, mp["pos"], mp["normal"], mp["max_dist"], mp["min_dist"], mp["desc"])
    row("slots", lambda: ctx.fuse_points_slots(m, np.arange(1000), pm.CAM, kfs, pm.BOUNDS), kfs, mp)
    m.close()
    # the second call: the resident frame against 30 000 candidates
    g, d = synth.make_frame("std", 0x5EED0002)
    st = hvo.Stream(depth=2, stages=hvo.STAGE_ORB, bf=pm.CAM[4])
    t = st.submit(g, d); fr = st.collect(t)
    kf, mp = ref.random_scene(dt, 0, 30000, seed=41, frame=(fr["kp_un"], fr["desc"], fr["uright"], fr["zdepth"]))
    m = hvo.PointMap(0, 30000)
    m.set_many(0, mp["pos"], mp["normal"], mp["max_dist"], mp["min_dist"], mp["desc"])
    sl = np.arange(30000)
    row("stream", lambda: [st.fuse_points(t, pm.CAM, kf["Tcw"], point_map=m, slots=sl, skip=kf["skip"])], [kf], mp)
    m.close(); st.close(); ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write(HEAD + "\n".join(lines) + "\n")


HEAD = """tools/fuse_timing.py, run once on one MI355X (gfx950): ORBmatcher::Fuse for the two calls of LocalMapping::SearchInNeighbors.
arrays: hvo_fuse_points, one shared map side of 1000 entries against 30 key frames of 1000 features on host arrays (everything goes up with
the call).  slots: hvo_fuse_points_slots, the same with the map side as slots of a resident point map.  stream: hvo_stream_fuse_points, one
resident 640 x 480 frame as the key frame against 30 000 candidates as slots of a resident point map.  Columns: key frames, entries per key
frame, fused entries of all key frames | device ms of k_fuse_grid, k_fuse_project, k_fuse_search + k_fuse_compact (hipEvents) | wall ms of the
whole call || tools/fuse_host.cpp (g++ -O2, one thread, real cell lists, one call per key frame) on the same inputs on the same machine's
host: building the key frames' grids, and the Fuse calls (ms) | whether its bestIdx / bestDist equal the device's.  Medians after 5 warm-up
calls.  The host restatement does not pay for the pointer walk either; it is the arithmetic of the replaced loop, not the reference's
ORBmatcher with its cv::Mat temporaries and mutexes.

"""

if __name__ == "__main__":
    main()
