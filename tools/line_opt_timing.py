"""Device time of the line structural constraints and Optimizer::LineOptStruct on the GPU (csrc/line_opt.hip) for
profiles/r10_line_opt.txt, from the hipEvents around the two launches (hvo_line_opt_last_kernel_ms): one generated frame of 200 lines,
batches of 256 and 8192 such frames in one launch sequence, split into the pair pass and the optimisation, and for orientation the
single-threaded numpy restatement of the same frame (NOT g2o: the reference cannot be built here)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import conftest  # noqa: E402
import line_opt_ref as ref  # noqa: E402


def main():
    hvo = conftest.load_pkg()
    ctx = hvo.Context()
    S = ref.make_scene(2000)
    k = dict(linefn=S["linefn"], lines3d=ref.to_records(S, hvo.LINE3D_DT))
    r = ctx.line_struct_optimize(k)
    ts = []
    for _ in range(20):
        ctx.line_struct_optimize(k); ts.append(ctx.line_opt_last_kernel_ms())
    ts = np.array(ts)
    print("one frame: %d lines, %d to optimise, %d edges (%d parallel, %d perpendicular), iterations %s trials %s"
          % (r.n_lines, r.n_lines_to_opt, r.n_edges, r.n_par_edges, r.n_perp_edges, list(r.iterations), list(r.trials)))
    print("one frame, device time, median of 20 (min): pair pass %.3f ms (%.3f), optimisation %.3f ms (%.3f)"
          % (np.median(ts[:, 0]), ts[:, 0].min(), np.median(ts[:, 1]), ts[:, 1].min()))
    t0 = time.perf_counter(); ref.struct_constraints(S["linefn"], S["line_eq"]); t1 = time.perf_counter(); ref.run_scene(S); t2 = time.perf_counter()
    print("numpy restatement of the same frame on this host, one thread (not g2o): pair pass %.1f ms, optimisation %.1f ms" % ((t1 - t0) * 1e3, (t2 - t1) * 1e3))
    for nb in (256, 8192):
        probs = [k] * nb
        ctx.line_struct_optimize(probs)
        t0 = time.perf_counter(); ctx.line_struct_optimize(probs); wall = time.perf_counter() - t0
        a, b = ctx.line_opt_last_kernel_ms()
        print("%d frames in one launch sequence: pair pass %.2f ms = %.2f us per frame, optimisation %.2f ms = %.2f us per frame (wall with packing and copies: %.0f ms)"
              % (nb, a, a / nb * 1e3, b, b / nb * 1e3, wall * 1e3), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
