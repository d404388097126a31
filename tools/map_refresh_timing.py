#!/usr/bin/env python3
"""Times the map refresh on the device (csrc/map_refresh.hip): MapPoint / MapLine ComputeDistinctiveDescriptors + UpdateNormalAndDepth /
UpdateAverageDir for every feature of a key frame in one call.

  arrays   hvo_refresh_map_points / hvo_refresh_map_lines: the positions go up with the observations
  slots    hvo_point_map_refresh / hvo_line_map_refresh: the same features as slots of a resident map, rewritten in place

Per point: the kernel's device time (hipEvents) and the whole call's wall time, medians of `reps` calls after 5 warm-up calls.  Beside them
tools/map_refresh_host.cpp, a plain single-thread host program with the loops as written, built with g++ -O2 here and run on the same
inputs; its answers are compared with the device's.  Every point runs in a process of its own under a time limit.

    python tools/map_refresh_timing.py [--reps 30] [--out profiles/map_refresh.txt]
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
POINTS = (("points", "arrays", 1000, 10), ("points", "slots", 1000, 10), ("points", "arrays", 1000, 30), ("points", "slots", 1000, 30),
          ("lines", "arrays", 200, 10), ("lines", "slots", 200, 10))
LIMIT_S = 120
COLS = "%-7s %-7s %9s %13s | %8s | %8s || %10s  %s"
ROW = "%-7s %-7s %9d %13d | %8.3f | %8.3f || %10.3f  %s"
F32 = np.float32


def build_host(workdir, root=ROOT):
    exe = os.path.join(workdir, "map_refresh_host")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", os.path.join(root, "tools", "map_refresh_host.cpp"), "-o", exe])
    return exe


def run_host(exe, workdir, line, pos, obs, sf, n_levels=8, what=3, reps=1, times=None):
    """-> the result dict of the library's shape; times receives the median ms (the case file's layout: the tool's head comment)"""
    case, res = os.path.join(workdir, "mr_case.bin"), os.path.join(workdir, "mr_result.bin")
    n = len(pos)
    with open(case, "wb") as f:
        np.array([1 if line else 0, n, int(obs["obs_start"][-1]), n_levels, what], np.int32).tofile(f)
        for a, dt in ((sf, F32), (obs["obs_start"], np.int32), (obs["obs_desc"], np.uint8), (obs["obs_Ow"], F32), (obs["kf_bad"], np.uint8), (obs["ref_Ow"], F32),
                      (obs["ref_level"], np.int32), (obs["skip"], np.uint8), (pos, np.float64 if line else F32)):
            np.ascontiguousarray(a, dt).tofile(f)
    t = subprocess.check_output([exe, case, res, str(reps)]).decode().split()
    if times is not None: times.extend(float(v) for v in t)
    rdt = np.float64 if line else F32
    out = {}
    with open(res, "rb") as f:
        for k, dt, w in (("best_obs", np.int32, 1), ("best_median", np.int32, 1), ("desc", np.uint8, 32), ("normal", rdt, 3), ("wvec", np.float64, 3 if line else 0),
                         ("max_dist", F32, 1), ("min_dist", F32, 1), ("status", np.uint8, 1)):
            if w: out[k] = np.fromfile(f, dt, n * w).reshape((n, w) if w > 1 else (n,))
    return out


def same_answer(host, got):
    return all(np.asarray(got[k]).tobytes() == v.tobytes() for k, v in host.items())


def median_ms(f, reps):
    for _ in range(5): f()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter(); f(); t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def point(kind, form, n, n_obs, reps):
    """one measurement, one line on stdout"""
    spec = importlib.util.spec_from_file_location("hvo_amd", os.path.join(PKG, "__init__.py"), submodule_search_locations=[PKG])
    hvo = importlib.util.module_from_spec(spec); sys.modules["hvo_amd"] = hvo; spec.loader.exec_module(hvo)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import map_refresh_ref as ref
    line = kind == "lines"
    tmp = tempfile.mkdtemp()
    exe = build_host(tmp)
    rng = np.random.RandomState(90 + n_obs)
    obs = ref.make_obs(np.full(n, n_obs), rng, bad_rate=0.05)
    pos = ref.line_positions(n, rng) if line else ref.point_positions(n, rng)
    ctx = hvo.Context(max_batch=1)
    if form == "arrays":
        call = lambda: (ctx.refresh_map_lines if line else ctx.refresh_map_points)(pos, obs)
    else:
        z3, z1 = np.zeros((n, 3)), np.zeros(n, F32)
        if line: m = hvo.LineMap(slots=0); m.set_many(0, pos, z3, z3, z1, z1, np.zeros((n, 32), np.uint8))
        else: m = hvo.PointMap(slots=0); m.set_many(0, pos, z3, z1, z1, np.zeros((n, 32), np.uint8))
        slots = np.arange(n, dtype=np.int32)
        call = lambda: m.refresh(ctx, slots, obs)
    got = call()
    wall = median_ms(call, reps)
    k = float(np.median([call()["kernel_ms"] for _ in range(reps)]))
    ht = []
    sf = np.array(ref.line_scale_factors(8, 1.2) if line else ref.pm.SF, F32)
    host = run_host(exe, tmp, line, pos, obs, sf, reps=max(3, reps // 3), times=ht)
    print(ROW % (kind, form, n, int(obs["obs_start"][-1]), k, wall, ht[0], "yes" if same_answer(host, got) else "NO"))
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30); ap.add_argument("--out", default=None)
    ap.add_argument("--point", nargs=4, default=None, help="kind, form, features, observations per feature: run one measurement in this process")
    a = ap.parse_args()
    if a.point:
        point(a.point[0], a.point[1], int(a.point[2]), int(a.point[3]), a.reps)
        return
    lines = [COLS % ("kind", "form", "features", "observations", "kernel", "call", "host loop", "same answer")]
    print(lines[0])
    for kind, form, n, n_obs in POINTS:
        try:
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--point", kind, form, str(n), str(n_obs)], capture_output=True, text=True,
                                 timeout=LIMIT_S)
        except subprocess.TimeoutExpired:
            lines.append("%-7s %-7s %9d  no answer within %d s" % (kind, form, n, LIMIT_S)); print(lines[-1])
            break                                                    # nothing more is started on the device after a point that hung
        if out.returncode != 0:
            lines.append("%-7s %-7s %9d  failed with status %d: %s" % (kind, form, n, out.returncode, out.stderr.strip().splitlines()[-1:] or "")); print(lines[-1])
            break
        lines.append(out.stdout.strip().splitlines()[-1]); print(lines[-1])
    if a.out:
        with open(a.out, "w") as f:
            f.write(HEAD % dict(reps=a.reps) + "\n".join(lines) + "\n")


HEAD = """tools/map_refresh_timing.py: MapPoint / MapLine ComputeDistinctiveDescriptors + UpdateNormalAndDepth / UpdateAverageDir for every feature of a
key frame in one call (k_mr_points / k_mr_lines, one wave per feature).  arrays: hvo_refresh_map_points / hvo_refresh_map_lines, the
positions go up with the observations.  slots: hvo_point_map_refresh / hvo_line_map_refresh, the same features as slots of a resident map,
rewritten in place (the mirror on the host is updated from the same download).  Every feature has the same number of observations, a
twentieth of the observers bad.  Columns: features, observations in all | device ms of the kernel (hipEvents) | wall ms of the whole call
from Python || tools/map_refresh_host.cpp (g++ -O2, one thread, the loops as written with the same readings) on the same inputs on the same
machine's host (ms) | whether its answers equal the device's bit for bit.  Medians of %(reps)d calls after 5 warm-up calls; every point is a
process of its own.  The host program is the arithmetic of the replaced loops, not the reference's MapPoint with its cv::Mat temporaries,
std::map copies and mutexes.

"""

if __name__ == "__main__":
    main()
