"""Times the relocalisation PnP solver on a RESIDENT stream frame beside the host path it replaces, per candidate count and correspondence count:

    n_kf N | device: hypothesis kernels, refine kernels, whole call (ms) || host: match vectors down, PnPsolver x n_kf single-threaded, pose up,
    their sum (ms) | accepted candidates device / host

Device side: one synthetic frame goes through a Stream with the ORB stage.  Each candidate key frame matches N of its features (the others
are -1); the matched key-frame points are the frame's key points unprojected at a random depth through a planted pose, 30 % of them displaced
(gross outliers).  `kernels` are the device times between hipEvents (hvo_stream_pnp_last_kernel_ms: hypotheses + scan, refine + events), `call`
is the wall time of Stream.pnp_ransac with its uploads, the compaction, the result download and the synchronisation; medians of 15 after a
warm-up call.  The reference's parameters: SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991), 8 extra iterations, 8 events.
Host side: what a tracker without this call does between SearchByBoW and PoseOptimization on resident frames -- hipMemcpy of the n_kf match
vectors down, one PnPsolver per candidate run to its end by tools/pnp_host.cpp (single thread; the same restatement, so the same hypotheses
and the same number of Refine calls -- a tracker that stops at the first accepted candidate does less), hipMemcpy of the 48 pose bytes up.
Every (n_kf, N) point is a process of its own under its own time limit (`--one n_kf N`, started by the sweep with `timeout`): a point that
raises, is killed at its limit or dies ends the sweep there, with a line that says which and how, and nothing more is started on the device.
Run on an MI355X, after __graft_entry__.build():  python tools/pnp_timing.py > profiles/r13_pnp.txt"""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))
import __graft_entry__ as entry      # noqa: E402
import pnp_ref as ref                # noqa: E402
from bow_timing import med, hip_runtime, copy_ms      # noqa: E402


POINT_LIMIT_S = 90                    # one point: a Stream, 31 device calls of a few ms each, 15 host solves; torch is not imported


def one(n_kf, N):
    hvo = entry.package()
    synth = __import__("importlib").import_module("hvo_amd.synth")
    exe = os.path.join(ROOT, "tools", "pnp_host")
    g = synth.make_frame("std", 0x5EED0101)[0]
    st = hvo.Stream(depth=2, stages=hvo.STAGE_ORB, bf=0.0)
    tk = st.submit(g); fr = st.collect(tk)
    kp = fr["kp_un"]; nf = len(kp)
    hip = hip_runtime()
    scale = np.ones(8, np.float32)
    for i in range(1, 8):
        scale[i] = scale[i - 1] * np.float32(1.2)
    Pd = ref.default_params(seed=1); P = hvo.pnp_params(**Pd)
    N = min(N, nf)
    rng = np.random.RandomState(n_kf * 1000 + N)
    sides, probs = [], []
    for j in range(n_kf):
        sc = ref.planted_scene(900 + j, 4)
        R = sc["Tcw"].reshape(3, 4)[:, :3]; t = sc["Tcw"].reshape(3, 4)[:, 3]
        who = np.sort(rng.permutation(nf)[:N])
        match = np.full(nf, -1, np.int32); match[who] = rng.permutation(N)
        z = rng.uniform(1.0, 4.0, N)
        pc = np.stack([(kp["x"][who] - ref.CAM[2]) / ref.CAM[0] * z, (kp["y"][who] - ref.CAM[3]) / ref.CAM[1] * z, z], 1)
        pw = (pc - t) @ R
        out = rng.rand(N) < 0.3; pw[out] += rng.randn(int(out.sum()), 3)
        pos = np.zeros((N, 3), np.float32); pos[match[who]] = pw.astype(np.float32)
        sides.append(dict(match_kf=match, pos=pos, bad=np.zeros(N, np.uint8)))
        probs.append(dict(p3d=pos[match[who]], p2d=np.stack([kp["x"][who], kp["y"][who]], 1), sigma2=scale[kp["octave"][who]] ** 2, feature_index=who, n_features=nf))
    # check=False: a candidate with more than max_events records keeps its status instead of ending the point (none is expected: records are rare)
    call, res = med(lambda: st.pnp_ransac(tk, ref.CAM, sides, P, check=False))
    kh, kr = [], []
    for _ in range(15):
        st.pnp_ransac(tk, ref.CAM, sides, P, check=False); a, b = st.pnp_last_kernel_ms(tk); kh.append(a); kr.append(b)
    with tempfile.TemporaryDirectory() as d:
        ref.write_problem_file(os.path.join(d, "p.bin"), probs, ref.CAM, Pd)
        host_ms = float(subprocess.check_output([exe, os.path.join(d, "p.bin"), os.path.join(d, "r.bin"), "15"], timeout=60).decode().split()[0])
        hres = ref.read_host_result(os.path.join(d, "r.bin"), n_kf, Pd["min_set"])
    dn, up = copy_ms(hip, n_kf * nf * 4, True), copy_ms(hip, 48, False)
    acc_d = sum(any(e["success"] for e in r["events"]) for r in res)
    acc_h = sum(any(rec["count"] > h["min_inliers"] for rec in h["records"]) for h in hres)
    over = sum(r["status"] != 0 for r in res)
    print("%d %d (%d features) | %.3f %.3f %.3f || %.3f %.3f %.3f %.3f | %d/%d%s" % (n_kf, N, nf, float(np.median(kh)), float(np.median(kr)), call, dn, host_ms, up,
                                                                                 dn + host_ms + up, acc_d, acc_h, "  (%d candidates past max_events)" % over if over else ""))
    st.close()


def main():
    if len(sys.argv) == 4 and sys.argv[1] == "--one":
        return one(int(sys.argv[2]), int(sys.argv[3]))
    exe = os.path.join(ROOT, "tools", "pnp_host")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-ffp-contract=off", os.path.join(ROOT, "tools", "pnp_host.cpp"), "-o", exe])
    print("# tools/pnp_timing.py: SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991), 30 % gross outliers; ms, medians of 15 after a warm-up call")
    print("# n_kf N | hypothesis kernels  refine kernels  call || host: matches down  PnPsolver x n_kf  pose up  sum | candidates with an accepted pose dev/host")
    sys.stdout.flush()
    for n_kf in (1, 5, 20):
        for N in (30, 100, 400):
            rc = subprocess.call(["timeout", "-k", "10", str(POINT_LIMIT_S), sys.executable, os.path.abspath(__file__), "--one", str(n_kf), str(N)])
            if rc != 0:
                print("# %d %d: the point ended with status %d (124 / 137: its time limit of %d s); the sweep stops here" % (n_kf, N, rc, POINT_LIMIT_S))
                return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
