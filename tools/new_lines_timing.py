#!/usr/bin/env python3
"""Times LocalMapping::CreateNewMapLinesConstraint on the device (csrc/line_triang.hip):

  stream   hvo_stream_create_new_map_lines: one resident 640 x 480 frame as the current key frame, 5 and 10 neighbours that see its lines
  arrays   hvo_create_new_map_lines: the same frame downloaded and the same neighbours, everything on host arrays (the same work)

Per point: the three kernel groups' device times (hipEvents: the searches, the triangulation, resolve + compaction) and the whole call's wall
time, medians of `reps` calls after 5 warm-up calls.  Beside them tools/new_lines_host.cpp, a plain single-thread host restatement of the
sequential loops, built with g++ -O2 here and run on the same inputs (the stream points on the downloaded frame); its created lists, end
points and owners are compared with the device's.  Every point runs in a process of its own under a time limit.

    python tools/new_lines_timing.py [--reps 30] [--out profiles/new_lines.txt]
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
POINTS = (("arrays", 5), ("arrays", 10), ("stream", 5), ("stream", 10))
LIMIT_S = 150
COLS = "%-7s %10s %6s %6s %8s | %8s %13s %8s | %8s || %10s  %s"
ROW = "%-7s %10d %6d %6d %8d | %8.3f %13.3f %8.3f | %8.3f || %10.3f  %s"


# ---- the case and result files of tools/new_lines_host.cpp (its head comment has the layout) ----
def _write_kf(f, kf):
    n = len(kf["kl"])
    np.array([n, 1 if kf.get("skip") else 0], np.int32).tofile(f)
    np.asarray(kf["Tcw"], np.float32).reshape(12).tofile(f)
    np.array(list(kf["cam"][:4]) + [kf.get("mb", 0.0), kf.get("median_depth", 1.0)], np.float32).tofile(f)
    np.ascontiguousarray(kf["kl"]).tofile(f); np.ascontiguousarray(kf["linefn"], np.float64).tofile(f)
    np.ascontiguousarray(kf["desc"], np.uint8).tofile(f); np.ascontiguousarray(np.asarray(kf["has_map_line"]).astype(bool), np.uint8).tofile(f)


def build_host(workdir, root=ROOT):
    exe = os.path.join(workdir, "new_lines_host")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-ffp-contract=off", "-I" + os.path.join(root, "include"), os.path.join(root, "tools", "new_lines_host.cpp"), "-o", exe])
    return exe


def run_host(exe, workdir, cur, kfs, th_high=80, nn_ratio=0.85, n_levels=8, scale_factor=1.2, pairing=0, reps=1, times=None):
    """-> (one dict(kf2, kf3, mv2, mv3, created_idx0 / 1 / 2, line3d of the created) per pair, owner_pair); times receives the median ms"""
    case, res = os.path.join(workdir, "nl_case.bin"), os.path.join(workdir, "nl_result.bin")
    with open(case, "wb") as f:
        np.array([len(kfs), n_levels, th_high, pairing], np.int32).tofile(f); np.array([nn_ratio, scale_factor], np.float32).tofile(f)
        _write_kf(f, cur)
        for kf in kfs: _write_kf(f, kf)
    t = subprocess.check_output([exe, case, res, str(reps)]).decode().split()
    if times is not None: times.extend(float(v) for v in t)
    out = []
    with open(res, "rb") as f:
        for _ in range(int(np.fromfile(f, np.int32, 1)[0])):
            kf2, kf3, mv2, mv3, n = (int(v) for v in np.fromfile(f, np.int32, 5))
            out.append(dict(kf2=kf2, kf3=kf3, mv2=mv2, mv3=mv3, created_idx0=np.fromfile(f, np.int32, n), created_idx1=np.fromfile(f, np.int32, n),
                            created_idx2=np.fromfile(f, np.int32, n), line3d=np.fromfile(f, np.float32, 6 * n).reshape(n, 6)))
        owner = np.fromfile(f, np.int32, len(cur["kl"]))
    return out, owner


def same_answer(host, pairs, summ):
    """the host tool's lists, end points and owners against a result of the library's shape"""
    hres, howner = host
    ok = len(hres) == len(pairs) and np.array_equal(howner, summ["owner_pair"])
    for h, r in zip(hres, pairs):
        i0 = r["created_idx0"]
        ok = ok and all(h[k] == r[k] for k in ("kf2", "kf3", "mv2", "mv3")) and all(np.array_equal(h[k], r[k]) for k in ("created_idx0", "created_idx1", "created_idx2"))
        ok = ok and h["line3d"].tobytes() == np.ascontiguousarray(r["line3d"][i0], np.float32).tobytes()
    return bool(ok)


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
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import new_lines_ref as ref
    tmp = tempfile.mkdtemp()
    exe = build_host(tmp)
    poses = [(ref.yaw(0.01 * (j % 5)), (0.3 * np.cos(0.63 * j), 0.3 * np.sin(0.63 * j), 0.02 * (j % 4))) for j in range(n_kf)]
    cam = (535.4, 539.2, 320.1, 247.6)
    ctx = hvo.Context(max_batch=1)
    g, d = synth.make_frame("std", 0x5EED0002)
    st = hvo.Stream(depth=2, stages=hvo.STAGE_LSD)
    t = st.submit(g, d); fr = st.collect(t)
    has = (np.arange(len(fr["kl"])) % 5 == 0).astype(np.uint8)
    kfs = ref.neighbours_of_frame(fr["kl"], fr["ldesc"], poses, cam, 81)
    cur = dict(kl=fr["kl"], linefn=fr["linefn"], desc=fr["ldesc"], has_map_line=has, Tcw=ref.IDENTITY, cam=cam)
    if form == "arrays": call = lambda: ctx.create_new_map_lines(cur, kfs)
    else: call = lambda: st.create_new_map_lines(t, cam, ref.IDENTITY, has, kfs)
    m, p, s = call()
    wall = median_ms(call, reps)
    k = np.median(np.array([call()[2]["kernel_ms"] for _ in range(reps)]), axis=0)
    ht = []
    host = run_host(exe, tmp, cur, kfs, reps=max(3, reps // 3), times=ht)
    print(ROW % (form, n_kf, len(cur["kl"]), s["n_pairs"], s["n_new"], k[0], k[1], k[2], wall, ht[0], "yes" if same_answer(host, p, s) else "NO"))
    st.close(); ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30); ap.add_argument("--out", default=None)
    ap.add_argument("--point", nargs=2, default=None, help="form and neighbour count: run one measurement in this process")
    a = ap.parse_args()
    if a.point:
        point(a.point[0], int(a.point[1]), a.reps)
        return
    lines = [COLS % ("form", "neighbours", "lines", "pairs", "created", "search", "triangulation", "resolve", "call", "host loop", "same answer")]
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
            f.write(HEAD % dict(reps=a.reps) + "\n".join(lines) + "\n")


HEAD = """tools/new_lines_timing.py: LocalMapping::CreateNewMapLinesConstraint, SearchForTriangulation of a current key frame against 5 and 10
neighbours and the three-view triangulation of every pair of them (10 and 45 pairs) in one call.  stream: hvo_stream_create_new_map_lines,
the current key frame is a resident 640 x 480 frame; the neighbours (key lines, line functions, descriptors and occupancy bytes of as many
lines) go up.  arrays: hvo_create_new_map_lines on the same frame downloaded and the same neighbours, so the two forms do the same work and
differ in what goes up.  Columns: neighbours, lines of the current key frame, pairs, lines created | device ms of the searches (per
neighbour k_hamming_knn2 + k_frame_bf_epilogue both ways, k_mutual_check, k_nl_occupancy), k_nl_triangulate, k_nl_resolve + k_nl_compact
(hipEvents) | wall ms of the whole call || tools/new_lines_host.cpp (g++ -O2, one thread, the sequential loops with the same readings) on
the same inputs on the same machine's host (ms) | whether its created lists, end points and owners equal the device's.  Medians of
%(reps)d calls after 5 warm-up calls; every point is a process of its own.  The host restatement is the arithmetic of the replaced loops, not
the reference's LocalMapping with its cv::Mat temporaries, cv::SVD::compute, BFMatcher, two threads per search and mutexes.

"""

if __name__ == "__main__":
    main()
