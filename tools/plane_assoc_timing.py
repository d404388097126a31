#!/usr/bin/env python3
"""Times the map-plane association (PlaneMatcher::SearchMapByCoefficients; csrc/plane_assoc.hip, kernels k_pa_prep / k_pa_gate / k_pa_dist /
k_pa_decide) against resident plane maps of 64, 512 and 4096 slots: the host-array form (hvo_match_planes), the stream form on a resident
640x480 frame (hvo_stream_match_planes) and the batch form over a resident batch (hvo_batch_match_planes).

Call times: host clock around the call (each ends in a stream synchronise), profiler off, warm-up first.  Kernel times: with --kernels the
tool starts one child per map size under `rocprofv3 --kernel-trace` (a run of its own, nothing else traced) and splits the k_pa_* dispatches
by order into the three forms.  The distance pass's share of the HBM peak is 12 bytes per point of the good slots per launch, computed from
the shapes, over its kernel time.  --host times the same loop as plain single-thread C++ (tools/plane_assoc_host.cpp, g++ -O2) on the same
inputs as the host form.  One JSON line per figure.

    python tools/plane_assoc_timing.py [--calls 30] [--batch 32] [--kernels] [--host]"""
import argparse
import csv
import glob
import json
import os
import struct
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import plane_assoc_ref as ref                                  # noqa: E402  (the seeded scene generator)

SIZES = ((64, 60000), (512, 400000), (4096, 3000000))          # (slots, points in all slots)
HBM_PEAK = 8.0e12                                              # bytes/s, the spec peak (6.3e12 measured for a float4 copy)
WARM = 3
STAGES = None


def timed(fn, calls):
    for _ in range(WARM):
        fn()
    t = []
    for _ in range(calls):
        t0 = time.perf_counter(); fn(); t.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(t)), 4), round(float(np.min(t)), 4)


def scene(ns, pts):
    coef, Tcw, slots = ref.make_scene(1000 + ns, ns, pts, n_frame=12, big_share=0.2)
    good = int(sum(len(s[1]) for s in slots if not s[2]))
    return coef, Tcw, slots, good


def run_forms(hvo, synth, ns, pts, calls, batch):
    """the three forms at one map size; returns the figures (and leaves 3 x (WARM + calls) groups of k_pa_* dispatches in a trace)"""
    coef, Tcw, slots, good = scene(ns, pts)
    m = hvo.PlaneMap()
    for j, (w, xyz, bad) in enumerate(slots):
        m.set(j, w, xyz)
        if bad:
            m.set_bad(j)
    stages = hvo.STAGE_PLANES | hvo.STAGE_PLANE_TAIL
    g, d, _ = synth.make_sequence("std", 0x5EED5700, batch)
    ctx = hvo.Context(max_batch=batch)
    st = hvo.Stream(depth=2, stages=stages, seed=3)
    out = []
    try:
        base = dict(slots=ns, points=good, need_bytes=12 * good)
        med, mn = timed(lambda: ctx.match_planes(m, coef, Tcw), calls)
        r = ctx.match_planes(m, coef, Tcw)
        out.append(dict(base, form="host", frames=1, planes=r.n_planes, matches=r.n_matches, call_ms_median=med, call_ms_min=mn))
        t = st.submit(g[0], d[0])
        med, mn = timed(lambda: st.match_planes(m, t, Tcw), calls)
        r = st.match_planes(m, t, Tcw)
        st.collect(t)
        out.append(dict(base, form="stream", frames=1, planes=r.n_planes, matches=r.n_matches, call_ms_median=med, call_ms_min=mn))
        ctx.batch_upload(g, d); ctx.batch_run(stages)
        T = np.tile(Tcw.reshape(1, 12), (batch, 1))
        med, mn = timed(lambda: ctx.batch_match_planes(m, T), calls)
        rs = ctx.batch_match_planes(m, T)
        out.append(dict(base, form="batch", frames=batch, planes=int(sum(x.n_planes for x in rs)), matches=int(sum(x.n_matches for x in rs)),
                        call_ms_median=med, call_ms_min=mn, per_frame_us=round(med * 1e3 / batch, 2)))
    finally:
        st.close(); ctx.close(); m.close()
    return out


def kernel_times(ns, pts, calls, batch):
    """one child under rocprofv3 --kernel-trace; the k_pa_* dispatches in start order, four per call, WARM + calls calls per form"""
    with tempfile.TemporaryDirectory() as td:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", td, "--", sys.executable, os.path.abspath(__file__), "--inner", str(ns), str(pts),
               "--calls", str(calls), "--batch", str(batch)]
        subprocess.run(cmd, check=True, stdout=subprocess.DEVNULL, timeout=300)
        rows = []
        for p in glob.glob(os.path.join(td, "**", "*kernel_trace.csv"), recursive=True):
            for r in csv.DictReader(open(p)):
                if r["Kernel_Name"].startswith("k_pa_"):
                    rows.append((int(r["Start_Timestamp"]), r["Kernel_Name"].split("(")[0], int(r["End_Timestamp"]) - int(r["Start_Timestamp"])))
    rows.sort()
    per_form = (WARM + calls + 1) * 4
    assert len(rows) == 3 * per_form, (len(rows), per_form)
    out = []
    for k, form in enumerate(("host", "stream", "batch")):
        grp = rows[k * per_form + WARM * 4: (k + 1) * per_form]
        d = {}
        for _, name, ns_ in grp:
            d.setdefault(name, []).append(ns_)
        out.append(dict(form=form, **{name + "_us": round(float(np.median(v)) / 1e3, 2) for name, v in d.items()}))
    return out


def host_loop(ns, pts, calls):
    coef, Tcw, slots, good = scene(ns, pts)
    exe = os.path.join(ROOT, "tools", "plane_assoc_host")
    if not os.path.exists(exe):
        subprocess.check_call(["g++", "-O2", "-std=c++14", os.path.join(ROOT, "tools", "plane_assoc_host.cpp"), "-o", exe])
    with tempfile.NamedTemporaryFile(suffix=".bin") as f:
        f.write(struct.pack("<ii", len(coef), len(slots)) + np.asarray(ref.DEFAULT_TH, np.float32).tobytes() + Tcw.astype(np.float32).tobytes() + coef.tobytes())
        for w, xyz, bad in slots:
            f.write(w.astype(np.float32).tobytes() + struct.pack("<ii", int(bad), len(xyz)) + np.ascontiguousarray(xyz, np.float32).tobytes())
        f.flush()
        ms, nm, _ = subprocess.check_output([exe, f.name, str(calls)]).decode().split()
    return dict(form="host_cpu_loop", slots=ns, points=good, planes=len(coef), matches=int(nm), call_ms_median=float(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=30)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--host", action="store_true")
    ap.add_argument("--inner", nargs=2, type=int, default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.inner or not (args.kernels or args.host):
        import importlib
        import __graft_entry__ as G
        hvo = G.package(); synth = importlib.import_module("hvo_amd.synth")
        for ns, pts in ([tuple(args.inner)] if args.inner else SIZES):
            for o in run_forms(hvo, synth, ns, pts, args.calls, args.batch):
                print(json.dumps(o), flush=True)
        return
    for ns, pts in SIZES:
        if args.host:
            print(json.dumps(host_loop(ns, pts, 11)), flush=True)
        if args.kernels:
            good = scene(ns, pts)[3]
            for o in kernel_times(ns, pts, args.calls, args.batch):
                us = o.get("k_pa_dist_us")
                if us:
                    o["dist_need_bytes"] = 12 * good; o["dist_share_of_hbm_peak"] = round(12 * good / (us * 1e-6) / HBM_PEAK, 4)
                print(json.dumps(dict(o, slots=ns, points=good)), flush=True)


if __name__ == "__main__":
    main()
