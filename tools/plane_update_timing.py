#!/usr/bin/env python3
"""Times MapPlane::UpdateCoefficientsAndPoints on the resident plane map (csrc/plane_update.hip, kernel k_pu_update) against the host route it
replaces, on the scene of tests/test_plane_update_gpu.py's sequence test scaled to a slot of 20000 points and a frame cloud of 2000 points:

  device   hvo_update_map_planes (the frame cloud goes up with the call) and hvo_stream_update_map_planes on a resident 640x480 synthetic
           frame (its own plane clouds, a few hundred points a plane, merged into the 20000-point slot): host clock around the call, which
           ends in a stream synchronise; the slot is set back before every timed call, outside the window
  kernel   with --kernels: one child under `rocprofv3 --kernel-trace` (a run of its own), the k_pu_update dispatches after the warm-up
  route    what a caller did before: Stream.collect (the tail's arrays come down), the merge as single-thread C++
           (tools/plane_update_host.cpp merge, g++ -O2, on the same clouds) and hvo_plane_map_set of the merged cloud

One JSON line per figure.    python tools/plane_update_timing.py [--calls 30] [--kernels]"""
import argparse
import csv
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import plane_assoc_ref as aref                                 # noqa: E402
import plane_update_ref as ref                                 # noqa: E402

WARM = 3
F32 = np.float32
N_SLOT, N_FRAME = 20000, 2000


def scene():
    """one world wall whose voxel cloud has N_SLOT points, and a frame cloud of N_FRAME points of it seen from a pose"""
    rng = np.random.RandomState(31)
    world = np.array((0, 0, 1, -2), F32)
    side = 16.0
    while True:
        slot = ref.voxel_grid(aref.plane_cloud(rng, world, 8 * N_SLOT, extent=side))
        if len(slot) >= N_SLOT:
            break
        side *= 1.2
    slot = slot[rng.permutation(len(slot))[:N_SLOT]]
    Tcw = np.asarray(aref.pose(aref.rot((0.2, 1.0, -0.1), 12.0), (0.3, -0.2, 0.4)), F32)
    T4 = np.vstack([Tcw.astype(np.float64), [0, 0, 0, 1]])
    pick = slot[rng.permutation(N_SLOT)[:4 * N_FRAME]].astype(np.float64) + rng.normal(scale=0.03, size=(4 * N_FRAME, 3))
    frame = ref.voxel_grid((np.hstack([pick, np.ones((len(pick), 1))]) @ T4.T)[:, :3].astype(F32))[:N_FRAME]
    return world, slot, Tcw, frame


def timed(fn, reset, calls):
    t = []
    for k in range(WARM + calls):
        reset()
        t0 = time.perf_counter(); fn(); dt = (time.perf_counter() - t0) * 1e3
        if k >= WARM:
            t.append(dt)
    return round(float(np.median(t)), 4), round(float(np.min(t)), 4)


def run(hvo, synth, calls):
    world, slot, Tcw, frame = scene()
    rec, cloud = ref.records_for([frame], [aref.camera_coef(Tcw, world)])
    ctx = hvo.Context(); m = hvo.PlaneMap()
    st = hvo.Stream(depth=2, stages=hvo.STAGE_PLANES | hvo.STAGE_PLANE_TAIL, seed=3)
    out = []
    try:
        reset = lambda: m.set(0, world, slot)
        ops = [(0, 0, hvo.PLANE_UPDATE_MERGE)]
        med, mn = timed(lambda: ctx.update_map_planes(m, rec, cloud, Tcw, ops), reset, calls)
        reset(); r = ctx.update_map_planes(m, rec, cloud, Tcw, ops)
        merged = m.points(0)
        assert np.array_equal(merged.view(np.uint32), ref.voxel_grid(np.concatenate([ref.transform(ref.transform_matrix(Tcw), frame), slot])).view(np.uint32))
        out.append(dict(form="host_form_device", n_slot=N_SLOT, n_frame=len(frame), n_after=int(r["n_after"][0]), call_ms_median=med, call_ms_min=mn))
        g, d, _ = synth.make_sequence("std", 0x5EED5100, 1)
        t = st.submit(g[0], d[0])
        med, mn = timed(lambda: st.update_map_planes(m, t, Tcw, ops), reset, calls)
        reset(); r = st.update_map_planes(m, t, Tcw, ops)
        out.append(dict(form="stream_form_device", n_slot=N_SLOT, n_frame=int(r["n_frame"][0]), n_after=int(r["n_after"][0]), call_ms_median=med, call_ms_min=mn))
        # the route it replaces, piece by piece
        tc = []
        for k in range(WARM + calls):
            if k:
                t = st.submit(g[0], d[0])
            while not st.poll(t):                                  # the frame has finished: the window holds the collect alone
                pass
            t0 = time.perf_counter(); st.collect(t); tc.append((time.perf_counter() - t0) * 1e3)
        out.append(dict(form="route_collect", call_ms_median=round(float(np.median(tc[WARM:])), 4), note="Stream.collect of a finished frame: every array of the frame comes down, the tail's among them"))
        med, mn = timed(lambda: m.set(0, world, merged), lambda: None, calls)
        out.append(dict(form="route_plane_map_set", points=len(merged), call_ms_median=med, call_ms_min=mn))
        exe = os.path.join(tempfile.gettempdir(), "plane_update_host_timing")
        subprocess.check_call(["g++", "-O2", "-std=c++14", "-ffp-contract=off", os.path.join(ROOT, "tools", "plane_update_host.cpp"), "-o", exe])
        with tempfile.TemporaryDirectory() as td:
            Tcw.tofile(td + "/t"); frame.tofile(td + "/f"); slot.tofile(td + "/s")
            us = float(subprocess.check_output([exe, "merge", td + "/t", td + "/f", td + "/s", td + "/o", str(max(calls, 11))]).decode())
            assert np.array_equal(np.fromfile(td + "/o", np.uint32), merged.view(np.uint32).reshape(-1))
        out.append(dict(form="route_host_merge_cpp", n_slot=N_SLOT, n_frame=len(frame), call_ms_median=round(us / 1e3, 4)))
    finally:
        st.close(); ctx.close(); m.close()
    return out


def kernel_times(calls):
    with tempfile.TemporaryDirectory() as td:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", td, "--", sys.executable, os.path.abspath(__file__), "--inner", "--calls", str(calls)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=300)
        rows = []
        for p in glob.glob(os.path.join(td, "**", "*kernel_trace.csv"), recursive=True):
            for r in csv.DictReader(open(p)):
                if r["Kernel_Name"].startswith("k_pu_update"):
                    rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    rows.sort()
    per = WARM + calls + 1
    assert len(rows) == 2 * per, (len(rows), per)
    return [dict(form=f, k_pu_update_us=round(float(np.median([d for _, d in rows[k * per + WARM:(k + 1) * per]])) / 1e3, 2))
            for k, f in enumerate(("host_form_device", "stream_form_device"))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--inner", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.kernels and not args.inner:
        for o in kernel_times(args.calls):
            print(json.dumps(o), flush=True)
        return
    import importlib
    import __graft_entry__ as G
    hvo = G.package(); synth = importlib.import_module("hvo_amd.synth")
    for o in run(hvo, synth, args.calls):
        print(json.dumps(o), flush=True)


if __name__ == "__main__":
    main()
