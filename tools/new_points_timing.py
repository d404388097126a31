#!/usr/bin/env python3
"""Times LocalMapping::CreateNewMapPoints on the device (csrc/new_points.hip):

  arrays   hvo_create_new_map_points: a current key frame of 1000 features against 10 and 20 neighbours of about 1000 features on host arrays
  stream   hvo_stream_create_new_map_points: one resident 640 x 480 frame with its bag of words as the current key frame, 10 and 20
           neighbours that see its features

Per point: the three kernel groups' device times (hipEvents: rows + search, triangulation, resolve + compaction) and the whole call's wall
time, medians of `reps` calls after 5 warm-up calls.  Beside them tools/new_points_host.cpp, a plain single-thread host restatement of the
sequential loop with real per-node lists, built with g++ -O2 here and run on the same inputs (the stream points on the downloaded frame);
its created lists, points and owners are compared with the device's.  Every point runs in a process of its own under a time limit.

    python tools/new_points_timing.py [--reps 30] [--out profiles/new_points.txt]
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
POINTS = (("arrays", 10), ("arrays", 20), ("stream", 10), ("stream", 20))
LIMIT_S = 150
COLS = "%-7s %10s %9s %8s | %8s %13s %8s | %8s || %10s  %s"
ROW = "%-7s %10d %9d %8d | %8.3f %13.3f %8.3f | %8.3f || %10.3f  %s"


def median_ms(f, reps):
    for _ in range(5): f()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); f(); t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def point(form, n_kf, reps):
    """one measurement, one line on stdout"""
    spec = importlib.util.spec_from_file_location("hvo_amd", os.path.join(PKG, "__init__.py"), submodule_search_locations=[PKG])
    hvo = importlib.util.module_from_spec(spec); sys.modules["hvo_amd"] = hvo; spec.loader.exec_module(hvo)
    from hvo_amd import synth
    sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))
    import bow_ref
    import new_points_host_io as io
    import new_points_ref as ref
    import point_map_ref as pm
    tmp = tempfile.mkdtemp()
    exe = io.build(tmp, ROOT)
    poses = [(ref.yaw(0.004 * (j % 5)), (0.1 + 0.02 * j, 0.03 * (j % 3), 0.04 * (j % 4))) for j in range(n_kf)]
    cam = ref.CAM + (ref.MB,)
    ctx = hvo.Context(max_batch=1); st = v = None
    if form == "arrays":
        cur, kfs = ref.random_scene(n=1000, seed=70 + n_kf, poses=poses)
        call = lambda: ctx.create_new_map_points(ref.CAM, cur, kfs)
    else:
        g, d = synth.make_frame("std", 0x5EED0002)
        voc = bow_ref.make_vocabulary(6, 3, 7)
        v = hvo.Vocabulary(voc["k"], voc["L"], voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"], voc["scoring"], voc["weighting"], device=0)
        st = hvo.Stream(depth=2, stages=hvo.STAGE_ORB, bf=ref.CAM[4])
        t = st.submit(g, d); fr = st.collect(t)
        b = st.compute_bow(t, v, levelsup=1)
        has = (np.arange(len(fr["kp_un"])) % 4 == 0).astype(np.uint8)
        kfs = ref.neighbours_of_frame(fr["kp_un"], fr["uright"], fr["zdepth"], fr["desc"], b["node_id"], poses, ref.CAM, 71, ref.MB)
        cur = dict(kp_un=fr["kp_un"], kp=fr["kp"], uright=fr["uright"], depth=fr["zdepth"], desc=fr["desc"], node_id=b["node_id"], has_map_point=has, Tcw=ref.IDENTITY, mb=ref.MB)
        call = lambda: st.create_new_map_points(t, v, cam, ref.IDENTITY, has, kfs)
    res, summ = call()
    wall = median_ms(call, reps)
    k = np.median(np.array([call()[1]["kernel_ms"] for _ in range(reps)]), axis=0)
    ht = []
    host = io.run(exe, tmp, cur, kfs, ref.CAM, pm.SF, ref.SIGMA2, reps=max(3, reps // 3), times=ht)
    print(ROW % (form, n_kf, len(cur["kp_un"]), summ["n_new"], k[0], k[1], k[2], wall, ht[0], "yes" if io.same_answer(host, res, summ) else "NO"))
    if st is not None: st.close(); v.close()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30); ap.add_argument("--out", default=None)
    ap.add_argument("--point", nargs=2, default=None, help="form and neighbour count: run one measurement in this process")
    a = ap.parse_args()
    if a.point:
        point(a.point[0], int(a.point[1]), a.reps)
        return
    lines = [COLS % ("form", "neighbours", "features", "created", "search", "triangulation", "resolve", "call", "host loop", "same answer")]
    print(lines[0])
    for form, n_kf in POINTS:
        try:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--point", form, str(n_kf)], capture_output=True, text=True, timeout=LIMIT_S)
        except subprocess.TimeoutExpired:
            lines.append("%-7s %10d  no answer within %d s" % (form, n_kf, LIMIT_S)); print(lines[-1])
            break                                                    # nothing more is started on the device after a point that hung
        if out.returncode != 0:
            lines.append("%-7s %10d  failed with status %d: %s" % (form, n_kf, out.returncode, out.stderr.strip().splitlines()[-1:] or "")); print(lines[-1])
            break
        lines.append(out.stdout.strip().splitlines()[-1]); print(lines[-1])
    if a.out:
        with open(a.out, "w") as f:
            f.write(HEAD + "\n".join(lines) + "\n")


HEAD = """tools/new_points_timing.py, run once on one MI355X (gfx950): LocalMapping::CreateNewMapPoints, the epipolar search and the triangulation
of a current key frame against 10 and 20 neighbours in one call.  arrays: hvo_create_new_map_points, everything goes up with the call (a
neighbour is about 1000 key points, descriptors, node ids, mvuRight, mvDepth and occupancy bytes).  stream: hvo_stream_create_new_map_points,
the current key frame is a resident 640 x 480 frame with its bag of words; the neighbours go up.  Columns: neighbours, features of the
current key frame, points created | device ms of k_bow_csr + k_np_search, k_np_triangulate, k_np_resolve + k_np_compact (hipEvents) | wall
ms of the whole call || tools/new_points_host.cpp (g++ -O2, one thread, the sequential loop over real per-node lists with the same readings)
on the same inputs on the same machine's host (ms) | whether its created lists, points and owners equal the device's.  Medians of 30 calls
after 5 warm-up calls; every point is a process of its own.  The host restatement is the arithmetic of the replaced loop, not the
reference's LocalMapping with its cv::Mat temporaries, cv::SVD::compute and mutexes.  One run; no run-to-run spread was measured.

"""

if __name__ == "__main__":
    main()
