#!/usr/bin/env python3
"""Times hvo_stream_search_local_lines (Tracking::SearchLocalLines + computeStructConstInMap against a resident line map) on one synthetic
640 x 480 frame for maps of several sizes: the three kernel groups' device times (mark + frustum + compaction, the search, assignment +
post-gate + constraints) and the whole call's wall time, each the median of repeated calls after warm-up.  The first slots of every map are
the frame's own good 3-D lines with their descriptors (every fourth tilted out of its key line's interpretation plane, so that the post-gate
fires), the rest generated lines of which every second one is turned away; about half of a map is in view.

Beside it, the path the call replaces, in its three parts: the host frustum loop that builds the query arrays (tools/line_frustum_host.cpp,
plain single-thread C++, g++ -O2, on the same map and pose), and the upload of those arrays plus hvo_stream_search_lines_by_projection_map
(through the same binding, fed with the in-view lines).  That path applies neither the post-gate nor the map constraints.

    python tools/line_map_timing.py [--slots 1000,4000,16000] [--reps 50] [--lines 200]
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

CAM = (535.4, 539.2, 320.1, 247.6, 0.0)


def make_map(n, rng, out):
    """n lines in front of the identity camera; every second generated one is turned away (normal reversed) and fails the viewing-angle
    test; the first slots are the frame's own good 3-D lines (camera = world)"""
    uv = np.stack([rng.uniform(40, 600, n), rng.uniform(40, 440, n)], 1); duv = rng.uniform(-40, 40, (n, 2)); z = rng.uniform(1, 4, n)
    back = lambda p, zz: np.stack([(p[:, 0] - CAM[2]) / CAM[0] * zz, (p[:, 1] - CAM[3]) / CAM[1] * zz, zz], 1)
    A, B = back(uv, z), back(np.clip(uv + duv, 5, 635 - 160), z * rng.uniform(0.95, 1.05, n))
    desc = rng.randint(0, 256, (n, 32)).astype(np.uint8)
    l3 = out["lines3d"]; good = np.nonzero(l3["good"] == 1)[0][: n // 2]
    A[: len(good)] = l3["A"][good]; B[: len(good)] = l3["B"][good]; desc[: len(good)] = out["ldesc"][good]
    mid = 0.5 * (A + B); d = np.linalg.norm(mid, axis=1)
    nrm = mid / d[:, None]; nrm[len(good) + 1::2] *= -1
    w = A - B
    # every fourth frame-made line: the world vector tilted 10 degrees towards the normal of the plane through the camera and the line
    # (inside the search's 15 degree gate, outside the post-gate's |cos| <= 0.09)
    for k in range(0, len(good), 4):
        u = w[k] / np.linalg.norm(w[k]); pl = np.cross(A[k], B[k]); pl /= np.linalg.norm(pl)
        w[k] = np.cos(np.radians(10)) * u + np.sin(np.radians(10)) * pl
    return dict(pos=np.concatenate([A, B], 1), wvec=w, normal=nrm, max_dist=(2 * d).astype(np.float32), min_dist=(0.5 * d).astype(np.float32), desc=desc)


def host_loop_ms(M, T, bounds, log_sf, calls):
    """the replaced path's host frustum loop on the same map: (median ms, in view)"""
    exe = os.path.join(ROOT, "tools", "line_frustum_host")
    if not os.path.exists(exe):
        subprocess.check_call(["g++", "-O2", "-std=c++14", os.path.join(ROOT, "tools", "line_frustum_host.cpp"), "-o", exe])
    n = len(M["pos"])
    with tempfile.NamedTemporaryFile(suffix=".bin") as f:
        f.write(struct.pack("<i", n) + np.array(list(CAM[:4]) + list(bounds) + [log_sf], np.float32).tobytes() + np.asarray(T, np.float32).tobytes())
        for k, dt in (("pos", np.float64), ("wvec", np.float64), ("normal", np.float64), ("max_dist", np.float32), ("min_dist", np.float32), ("desc", np.uint8)):
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
    ap.add_argument("--slots", default="1000,4000,16000"); ap.add_argument("--reps", type=int, default=50); ap.add_argument("--lines", type=int, default=200)
    a = ap.parse_args()
    g, d = synth.make_frame("std", 0x5EED0002)
    st = hvo.Stream(depth=2, stages=hvo.STAGE_LSD | hvo.STAGE_ORB | hvo.STAGE_GRIDS | hvo.STAGE_LINES3D, bf=0.0, lsd_nfeatures=a.lines)
    T = np.hstack([np.eye(3), np.zeros((3, 1))]).astype(np.float32)
    t = st.submit(g, d); out = st.collect(t); nkl = len(out["kl"])
    log_sf = float(np.float32(np.log(np.float32(1.2))))
    print("frame: %d key lines; times in ms, median of %d calls after warm-up" % (nkl, a.reps))
    print("%6s %7s %7s %6s | %8s %8s %8s | %8s || %9s %15s | %8s" % ("slots", "in view", "matches", "gated", "frustum", "search", "post", "call",
                                                                  "host loop", "upload + search", "replaced"))
    for ns in (int(v) for v in a.slots.split(",")):
        M = make_map(ns, np.random.RandomState(ns), out); lm = hvo.LineMap(slots=ns)
        lm.set_many(0, M["pos"], M["wvec"], M["normal"], M["max_dist"], M["min_dist"], M["desc"])
        held = np.full(nkl, -1, np.int32)
        call = lambda: st.search_local_lines(lm, t, CAM, T, nkl, held=held, log_scale_factor=log_sf)
        r = call(); ks = []
        for _ in range(a.reps): ks.append(tuple(call().kernel_ms))
        k = np.median(np.array(ks), axis=0)
        s = r.in_view_slot
        old = lambda: st.search_lines_by_projection_map(t, r.proj, r.view_cos, M["wvec"][s], M["desc"][s], q_blocks=np.ones(len(s), np.uint8))
        hl, nv = host_loop_ms(M, T, st.bounds, log_sf, a.reps)
        if nv != r.n_in_view: print("# host loop: %d in view (plain float arithmetic, not the library's readings)" % nv)
        c_ms, o_ms = median_ms(call, a.reps), median_ms(old, a.reps)
        print("%6d %7d %7d %6d | %8.3f %8.3f %8.3f | %8.3f || %9.3f %15.3f | %8.3f" % (ns, r.n_in_view, r.n_matches, r.n_gated, k[0], k[1], k[2], c_ms, hl, o_ms, hl + o_ms))
        lm.close()
    st.close()


if __name__ == "__main__":
    main()
