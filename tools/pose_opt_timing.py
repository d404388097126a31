"""Device time of Optimizer::PoseOptimization on the GPU (csrc/pose_opt.hip) for profiles/r09_pose_opt.txt, from the hipEvents around the
launch (hvo_pose_last_kernel_ms): one call on a resident stream frame with the benchmark's feature counts, batches of 256 and 8192 problems
in one launch, the iterations and trials run, and for orientation the single-threaded numpy restatement of one problem (NOT g2o)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import conftest  # noqa: E402
import pose_opt_ref as ref  # noqa: E402


def main():
    hvo = conftest.load_pkg(); synth = conftest.load_synth()
    ctx = hvo.Context()
    # a resident frame: the synthetic benchmark frame, its own features back-projected as the map under a pose a little off
    s = hvo.Stream(640, 480, depth=2, stages=hvo.STAGE_FRAME, bf=40.0)
    g, d = synth.make_frame("std", 0x5EED0002)
    t = s.submit(g, d); fr = s.collect(t)
    fx, fy, cx, cy, bf = ref.CAM
    n, nl = len(fr["kp_un"]), len(fr["linefn"])
    pc = fr["plane_clouds"]; coef = pc["coef"][pc["valid"] != 0]; m = len(coef)
    z = np.where(fr["zdepth"] > 0, fr["zdepth"], 2.0).astype(np.float64)
    X = np.stack([(fr["kp_un"]["x"] - cx) / fx * z, (fr["kp_un"]["y"] - cy) / fy * z, z], axis=1).astype(np.float32)
    l3 = fr["lines3d"]
    pl_w = np.repeat(coef[:, None, :], 3, axis=1).astype(np.float32); pl_has = np.zeros((m, 3), np.uint8); pl_has[:, 0] = 1
    Tcw = np.concatenate([ref.rot_vec([0.01, -0.02, 0.015]), [[0.02], [-0.01], [0.03]]], axis=1).astype(np.float32)
    ms = dict(pt_has=(fr["zdepth"] > 0).astype(np.uint8), pt_xyz=X, ln_has=(l3["good"] != 0).astype(np.uint8),
              ln_xyz=np.concatenate([l3["A"], l3["B"]], axis=1), pl_has=pl_has, pl_coef_w=pl_w)
    r = s.pose_optimize(t, ref.CAM, Tcw, (n, nl, m), **ms)
    ts = []
    for _ in range(20):
        s.pose_optimize(t, ref.CAM, Tcw, (n, nl, m), **ms); ts.append(s.pose_last_kernel_ms(t))
    passes = sum(r.iterations); trials = sum(r.trials)
    print("resident frame: %d points (%d matched), %d lines (%d matched), %d planes; %d edges; iterations %s trials %s"
          % (n, int(ms["pt_has"].sum()), nl, int(ms["ln_has"].sum()), m, r.n_edges, list(r.iterations), list(r.trials)))
    print("one call on the resident frame, device time of the launch: median %.3f ms (min %.3f) = %.1f us per pass over %d system + %d trial passes"
          % (np.median(ts), min(ts), np.median(ts) * 1e3 / (passes + trials), passes, trials))
    s.close()
    P, _ = ref.make_scene(1001, n_pts=1000, n_lines=200, n_planes=8)
    k = ref.to_binding(P, hvo.KEYPOINT_DT, hvo.LINE3D_DT)
    r = ctx.pose_optimize(ref.CAM, k); one = ctx.pose_last_kernel_ms()
    print("generated problem, 1000 points, 200 lines, 8 planes x 3 roles: %d edges, iterations %s trials %s, device time %.3f ms"
          % (r.n_edges, list(r.iterations), list(r.trials), one))
    for nb in (256, 8192):
        probs = [k] * nb
        ctx.pose_optimize(ref.CAM, probs)
        t0 = time.perf_counter(); ctx.pose_optimize(ref.CAM, probs); wall = time.perf_counter() - t0
        dev = ctx.pose_last_kernel_ms()
        print("%d problems in one launch: device time %.2f ms = %.2f us per frame (wall with the binding's packing and the copies: %.1f ms)"
              % (nb, dev, dev / nb * 1e3, wall * 1e3))
    t0 = time.perf_counter(); ref.pose_optimization(P); dt = time.perf_counter() - t0
    print("numpy restatement of the generated problem on this host, one thread (not g2o): %.1f ms" % (dt * 1e3))
    ctx.close()


if __name__ == "__main__":
    main()
