#!/usr/bin/env python3
"""Times hvo_stream_search_local_points (Tracking::SearchLocalPoints against a resident point map) on one synthetic 640 x 480 frame for maps
of several sizes: the three kernel groups' device times (mark + frustum + compaction, the search, the assignment) and the whole call's wall
time, each the median of repeated calls after warm-up.  A quarter of every map is the frame's own key points with depth, unprojected
(camera = world) with their descriptors, so that the search matches; the rest are generated points of which every third one faces the
camera; about half of a map is in view.

Beside it, the path the call replaces, in its three parts: the host frustum loop that builds the query arrays (tools/point_frustum_host.cpp,
plain single-thread C++, g++ -O2, on the same map and pose), gathering those arrays for the in-view points on the host (numpy), and
hvo_search_by_projection_tracked, which uploads them together with the frame's key points, mvuRight and descriptors and runs the same search.

    python tools/point_map_timing.py [--slots 1000,4000,16000] [--reps 50]
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
N_LEVELS = 8


def make_map(n, rng, out):
    """n points in front of the identity camera: the first quarter are the frame's own key points with depth (cycled), unprojected, with
    mfMaxDistance half a level inside their octave; of the generated rest two in three are turned away (normal reversed)"""
    uv = np.stack([rng.uniform(40, 600, n), rng.uniform(40, 440, n)], 1); z = rng.uniform(1, 4, n)
    desc = rng.randint(0, 256, (n, 32)).astype(np.uint8)
    octave = rng.randint(0, N_LEVELS, n)
    good = np.nonzero(out["zdepth"] > 0)[0]
    own = good[np.arange(n // 4) % len(good)] if len(good) else good
    k = len(own)
    uv[:k, 0] = out["kp_un"]["x"][own]; uv[:k, 1] = out["kp_un"]["y"][own]; z[:k] = out["zdepth"][own]; desc[:k] = out["desc"][own]; octave[:k] = out["kp_un"]["octave"][own]
    X = np.stack([(uv[:, 0] - CAM[2]) / CAM[0] * z, (uv[:, 1] - CAM[3]) / CAM[1] * z, z], 1)
    d = np.linalg.norm(X, axis=1)
    nrm = X / d[:, None]
    away = np.arange(n) >= k; away[k::3] = False
    nrm[away] *= -1
    mx = d * 1.2 ** (octave - 0.5)
    return dict(pos=X.astype(np.float32), normal=nrm.astype(np.float32), max_dist=mx.astype(np.float32), min_dist=(mx / 1.2 ** (N_LEVELS - 1)).astype(np.float32), desc=desc)


def host_loop_ms(M, T, bounds, log_sf, calls):
    """the replaced path's host frustum loop on the same map: (median ms, in view)"""
    exe = os.path.join(ROOT, "tools", "point_frustum_host")
    if not os.path.exists(exe):
        subprocess.check_call(["g++", "-O2", "-std=c++14", os.path.join(ROOT, "tools", "point_frustum_host.cpp"), "-o", exe])
    n = len(M["pos"])
    with tempfile.NamedTemporaryFile(suffix=".bin") as f:
        f.write(struct.pack("<ii", n, N_LEVELS) + np.array(list(CAM[:5]) + list(bounds) + [log_sf], np.float32).tobytes() + np.asarray(T, np.float32).tobytes())
        for k, dt in (("pos", np.float32), ("normal", np.float32), ("max_dist", np.float32), ("min_dist", np.float32), ("desc", np.uint8)):
            f.write(np.ascontiguousarray(M[k], dt).tobytes())
        f.write(np.full(n, 2, np.uint8).tobytes())
        f.flush()
        ms, nv, _ = subprocess.check_output([exe, f.name, str(calls)]).decode().split()
    return float(ms), int(nv)


def median_ms(f, reps):
    for _ in range(5): f()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); f(); t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", default="1000,4000,16000"); ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    g, d = synth.make_frame("std", 0x5EED0002)
    st = hvo.Stream(depth=2, stages=hvo.STAGE_ORB, bf=CAM[4]); ctx = hvo.Context()
    T = np.hstack([np.eye(3), np.zeros((3, 1))]).astype(np.float32)
    t = st.submit(g, d); out = st.collect(t); nkp = len(out["kp"])
    log_sf = float(np.float32(np.log(np.float32(1.2))))
    b = [float(v) for v in st.bounds]
    print("frame: %d key points; th = 3; times in ms, median of %d calls after warm-up" % (nkp, a.reps))
    print("%6s %7s %7s | %8s %8s %8s | %8s || %9s %8s %16s | %8s" % ("slots", "in view", "matches", "frustum", "search", "assign", "call",
                                                                   "host loop", "gather", "tracked (upload)", "replaced"))
    for ns in (int(v) for v in a.slots.split(",")):
        M = make_map(ns, np.random.RandomState(ns), out); pm = hvo.PointMap(slots=ns)
        pm.set_many(0, M["pos"], M["normal"], M["max_dist"], M["min_dist"], M["desc"])
        held = np.full(nkp, -1, np.int32)
        call = lambda: st.search_local_points(pm, t, CAM, T, nkp, held=held, log_scale_factor=log_sf, n_levels=N_LEVELS, th=3.0)
        r = call(); ks = []
        for _ in range(a.reps): ks.append(tuple(call().kernel_ms))
        k = np.median(np.array(ks), axis=0)
        s = r.in_view_slot
        gather = lambda: (M["desc"][s], r.proj[:, 0].copy(), r.proj[:, 1].copy(), r.proj[:, 2].copy(), r.level, r.view_cos, np.ones(len(s), np.uint8))
        q = gather(); occ = np.zeros(nkp, np.uint8)
        old = lambda: ctx.search_by_projection_tracked(q[0], q[1], q[2], q[3], q[4], q[5], q[6], 3.0, out["kp_un"], out["uright"], occ, out["desc"],
                                                       (b[0], b[2], b[1], b[3]))
        nm_old = old()[0]
        if nm_old != r.n_matches: print("# the replaced path matched %d" % nm_old)
        hl, nv = host_loop_ms(M, T, b, log_sf, a.reps)
        if nv != r.n_in_view: print("# host loop: %d in view (plain float arithmetic, not the library's readings)" % nv)
        c_ms, g_ms, o_ms = median_ms(call, a.reps), median_ms(gather, a.reps), median_ms(old, a.reps)
        print("%6d %7d %7d | %8.3f %8.3f %8.3f | %8.3f || %9.3f %8.3f %16.3f | %8.3f" % (ns, r.n_in_view, r.n_matches, k[0], k[1], k[2], c_ms, hl, g_ms, o_ms,
                                                                                      hl + g_ms + o_ms))
        pm.close()
    st.close(); ctx.close()


if __name__ == "__main__":
    main()
