#!/usr/bin/env python3
"""Times Manhattan-frame tracking (Tracking::TrackManhattanFrame; csrc/manhattan.hip, kernel k_mf_track): the host-array form
(hvo_track_manhattan: normals and 3-D lines go up, the result comes down) and the stream form (hvo_stream_track_manhattan: they stay on the
device) at 640x480 (8 560 normals) and 1280x960 (34 080), and the batch chain (hvo_batch_track_manhattan) over 256 resident frames.  Prints
one JSON line per configuration with host-clock times (each call ends in a stream synchronise).  Run it under
`rocprofv3 --kernel-trace --stats` for the kernel's device time.

    python tools/manhattan_timing.py [--calls 50] [--batch 256]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as G                                    # noqa: E402
hvo = G.package()
import importlib                                              # noqa: E402
synth = importlib.import_module("hvo_amd.synth")

STAGES = hvo.STAGE_LSD | hvo.STAGE_PLANES | hvo.STAGE_LINES3D | hvo.STAGE_PLANE_TAIL


def timed(fn, calls):
    for _ in range(3):
        fn()
    t = []
    for _ in range(calls):
        t0 = time.perf_counter(); fn(); t.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(t)), 4), round(float(np.min(t)), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--batch", type=int, default=256)
    args = ap.parse_args()
    R = np.eye(3, dtype=np.float32)
    for w, h in ((640, 480), (1280, 960)):
        kw = dict(fx=535.4 * w / 640, fy=539.2 * h / 480, cx=320.1 * w / 640, cy=247.6 * h / 480) if w != 640 else {}
        g, d, _ = synth.make_sequence("std", 0x5EED4500, 1, w=w, h=h)
        st = hvo.Stream(width=w, height=h, depth=2, stages=STAGES, seed=3, **kw)
        ctx = hvo.Context(**kw)
        try:
            t = st.submit(g[0], d[0])
            res = st.track_manhattan(t, R)
            s_med, s_min = timed(lambda: st.track_manhattan(t, R), args.calls)
            r = st.collect(t)
            sn, l3d = r["normals"], r["lines3d"]
            h_med, h_min = timed(lambda: ctx.track_manhattan(sn, l3d, R), args.calls)
            print(json.dumps(dict(form="host", w=w, h=h, normals=len(sn), lines=len(l3d), n_found=res.n_found, call_ms_median=h_med, call_ms_min=h_min)), flush=True)
            print(json.dumps(dict(form="stream", w=w, h=h, normals=len(sn), lines=len(l3d), n_found=res.n_found, call_ms_median=s_med, call_ms_min=s_min)), flush=True)
        finally:
            st.close(); ctx.close()
    n = args.batch
    g, d, _ = synth.make_sequence("std", 0x5EED4600, min(n, 64))
    idx = np.arange(n) % len(g)
    ctx = hvo.Context(max_batch=n)
    try:
        ctx.batch_upload(g[idx], d[idx])
        ctx.batch_run(STAGES)
        b_med, b_min = timed(lambda: ctx.batch_track_manhattan(R), max(args.calls // 5, 5))
        out = ctx.batch_track_manhattan(R)
        print(json.dumps(dict(form="batch", frames=n, tracked=int(sum(o.tracked for o in out)), call_ms_median=b_med, call_ms_min=b_min,
                              per_frame_us=round(b_med * 1e3 / n, 2))), flush=True)
    finally:
        ctx.close()


if __name__ == "__main__":
    main()
