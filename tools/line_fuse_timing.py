#!/usr/bin/env python3
"""Times LSDmatcher::Fuse on the device (csrc/line_fuse.hip) for the two line calls of LocalMapping::SearchInNeighbors:

  arrays         hvo_fuse_lines: 200 entries (one shared map side) x 30 key frames of 200 lines, on host arrays
  slots          hvo_fuse_lines_slots: the same, the map side as 200 slots of a resident line map
  stream         hvo_stream_fuse_lines: one resident frame as the key frame, 6000 candidates on host arrays
  stream slots   the same, the candidates as slots of a resident line map

Per case: the three kernel groups' device times (hipEvents: records + projection, search, count + compaction) and the whole call's wall time,
medians of repeated calls after 5 warm-up calls.  Beside them tools/line_fuse_host.cpp, a plain single-thread host restatement of the loop
(every key line tested for every entry, one call per key frame), built with g++ -O2 here and run on the same inputs (the stream cases on the
downloaded frame); its answer is compared with the device's.  The key frames are tests/line_fuse_ref.py's random scene with the 30 poses
drawn from three.

    python tools/line_fuse_timing.py [--reps 30] [--out profiles/line_fuse.txt]
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
import line_fuse_ref as ref  # noqa: E402

KW = dict(n_levels=3, scale_factor=1.2)


def write_case(path, kfs, mp, th, th_low, log_scale_factor, n_levels, scale_factor, level_rule):
    """the case file of tools/line_fuse_host.cpp (its head comment has the layout)"""
    n = len(mp["pos"])
    with open(path, "wb") as f:
        np.array([len(kfs), n, n_levels, th_low, level_rule], np.int32).tofile(f)
        np.array([th, log_scale_factor, scale_factor], np.float32).tofile(f)
        for k, dt in (("pos", np.float64), ("normal", np.float64), ("max_distance", np.float32), ("min_distance", np.float32), ("desc", np.uint8)):
            np.ascontiguousarray(mp[k], dt).tofile(f)
        for kf in kfs:
            kl = kf["kl"]; rows = np.ascontiguousarray(kf["desc_rows"], np.uint8).reshape(-1, 32)
            np.array([len(kl), len(rows)], np.int32).tofile(f)
            np.asarray(kf["Tcw"], np.float32).reshape(12).tofile(f)
            np.array(list(kf["cam"][:4]) + list(kf["bounds"]), np.float32).tofile(f)
            for k in ("pt_x", "pt_y", "sx", "sy", "ex", "ey"): np.ascontiguousarray(kl[k], np.float32).tofile(f)
            np.ascontiguousarray(kl["octave"], np.int32).tofile(f)
            rows.tofile(f)
            (np.zeros(n, np.uint8) if kf.get("skip") is None else np.ascontiguousarray(np.asarray(kf["skip"]).astype(bool), np.uint8)).tofile(f)


def run_host(exe, workdir, kfs, mp, reps, n_levels):
    """-> (one dict(best_idx, best_dist, gate) per key frame, the median ms of reps runs of all key frames)"""
    case, res = os.path.join(workdir, "line_fuse_case.bin"), os.path.join(workdir, "line_fuse_result.bin")
    write_case(case, kfs, mp, ref.TH, ref.TH_LOW, ref.LOG_SF, n_levels, 1.2, 0)
    ms = float(subprocess.check_output([exe, case, res, str(reps)]).decode().split()[0])
    n = len(mp["pos"]); out = []
    with open(res, "rb") as f:
        for _ in kfs:
            out.append(dict(best_idx=np.fromfile(f, np.int32, n), best_dist=np.fromfile(f, np.int32, n), gate=np.fromfile(f, np.int8, n)))
    return out, ms


def median_ms(f, reps):
    for _ in range(5): f()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); f(); t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30); ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)
    tmp = tempfile.mkdtemp()
    exe = os.path.join(tmp, "line_fuse_host")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-ffp-contract=off", os.path.join(ROOT, "tools", "line_fuse_host.cpp"), "-o", exe])
    ctx = hvo.Context(max_batch=1)
    dt = hvo.KEYLINE_DT
    say("%-12s %9s %6s %8s %6s | %10s %8s %8s | %8s || %10s  %s" % ("case", "keyframes", "lines", "entries", "fused", "projection", "search", "compact", "call", "host loop", "same answer"))

    def row(name, call, kfs, mp, n_levels):
        r = call()
        for _ in range(5): call()
        k = np.median(np.array([call()[0]["kernel_ms"] for _ in range(a.reps)]), axis=0)
        hr, hms = run_host(exe, tmp, kfs, mp, max(3, a.reps // 3), n_levels)
        ok = all(np.array_equal(r[j][f], hr[j][f]) for j in range(len(kfs)) for f in ("best_idx", "best_dist", "gate"))
        say("%-12s %9d %6d %8d %6d | %10.3f %8.3f %8.3f | %8.3f || %10.3f  %s" % (name, len(kfs), max(len(kf["kl"]) for kf in kfs), len(mp["pos"]), sum(x["n_fused"] for x in r),
                                                                             k[0], k[1], k[2], median_ms(call, a.reps), hms, "yes" if ok else "NO"))

    # the first call: one map side, 30 target key frames
    kfs, mp = ref.random_scene(dt, n_kf=30, n_lines=200, n=200, seed=40, pose_ids=[j % 3 for j in range(30)])
    row("arrays", lambda: ctx.fuse_lines(kfs, mp, **KW), kfs, mp, 3)
    m = hvo.LineMap(0, 200)
    m.set_many(0, mp["pos"], mp["pos"][:, 3:] - mp["pos"][:, :3], mp["normal"], mp["max_distance"], mp["min_distance"], mp["desc"])
    sl = np.arange(200, dtype=np.int32)
    row("slots", lambda: ctx.fuse_lines_slots(m, sl, kfs, **KW), kfs, mp, 3)
    m.close()
    # the second call: the resident frame against 6000 candidates
    cam = (535.4, 539.2, 320.1, 247.6, 40.0)
    g, d = synth.make_frame("std", 0x5EED0002)
    st = hvo.Stream(depth=2, stages=hvo.STAGE_LSD, lsd_nfeatures=200)
    t = st.submit(g, d); fr = st.collect(t)
    n_kl = len(fr["kl"]); copies = max(1, 6000 // max(n_kl, 1))
    mp = ref.map_from_frame(fr["kl"], fr["ldesc"], cam, 41, copies=copies)
    n = len(mp["pos"])
    kf = ref.make_kf(fr["kl"], fr["ldesc"], Tcw=ref.IDENTITY, cam=cam, skip=(np.arange(n) % 11 == 0).astype(np.uint8))
    K2 = dict(n_levels=2, scale_factor=1.2)
    row("stream", lambda: [st.fuse_lines(t, cam, ref.IDENTITY, maps=mp, skip=kf["skip"], **K2)], [kf], mp, 2)
    m = hvo.LineMap(0, n)
    m.set_many(0, mp["pos"], mp["pos"][:, 3:] - mp["pos"][:, :3], mp["normal"], mp["max_distance"], mp["min_distance"], mp["desc"])
    sl = np.arange(n, dtype=np.int32)
    row("stream slots", lambda: [st.fuse_lines(t, cam, ref.IDENTITY, line_map=m, slots=sl, skip=kf["skip"], **K2)], [kf], mp, 2)
    m.close(); st.close(); ctx.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write(HEAD + "\n".join(lines) + "\n")


HEAD = """tools/line_fuse_timing.py, run once on one MI355X (gfx950): LSDmatcher::Fuse for the two line calls of LocalMapping::SearchInNeighbors.
arrays: hvo_fuse_lines, one shared map side of 200 entries against 30 key frames of 200 lines on host arrays (everything goes up with the
call).  slots: hvo_fuse_lines_slots, the same with the map side as slots of a resident line map.  stream: hvo_stream_fuse_lines, one resident
640 x 480 frame as the key frame against its candidates on host arrays; stream slots: the candidates as slots of a resident line map.
Columns: key frames, lines per key frame, entries per key frame, fused entries of all key frames | device ms of k_lf_lines + k_lf_project,
k_lf_search, k_lf_count + k_lf_compact (hipEvents) | wall ms of the whole call || tools/line_fuse_host.cpp (g++ -O2, one thread, every key
line tested for every entry, one call per key frame) on the same inputs on the same machine's host (ms) | whether its bestIdx / bestDist /
gate equal the device's.  Medians of 30 calls after 5 warm-up calls.  The host restatement does not pay for the pointer walk either; it is
the arithmetic of the replaced loop, not the reference's LSDmatcher with its cv::Mat temporaries, its copy of mvKeyLines per entry and its
mutexes.

"""

if __name__ == "__main__":
    main()
