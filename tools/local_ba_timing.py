"""Device time of Optimizer::LocalMapOptimization on the GPU (csrc/local_ba.hip) for profiles/local_ba.txt: per linearisation (poses,
edges, pairs, blocks, sums), per trial (landmark inverses, reduced system, factorisation, update, evaluation), of the trials the
one-workgroup factorisation, and the whole call, from the hipEvents the call records (hvo_local_ba_last_profile), for the test shapes S
and M and a window of 40 key frames / 6000 points / 600 lines; for orientation the single-threaded numpy restatement (NOT g2o)."""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import conftest  # noqa: E402
import local_ba_ref as ref  # noqa: E402


def main():
    hvo = conftest.load_pkg()
    ba = hvo.LocalBA()
    for shape, what, cpu in (("S", "5 local + 2 outside key frames, 60 points, 10 lines", True), ("M", "24 free + 8 fixed key frames, 1500 points, 120 lines", True),
                             ("T", "32 free + 8 fixed key frames, 6000 points, 600 lines", False), ("W", "64 free + 2 fixed key frames, 1920 points, 16 lines", False)):
        W, _ = ref.shape_window(shape, 1000)
        g = ref.to_binding(W)
        o = ba.optimize(g)
        rows = []
        for _ in range(5):
            t0 = time.perf_counter(); o = ba.optimize(g); wall = (time.perf_counter() - t0) * 1e3
            p = ba.last_profile(); p["wall"] = wall; rows.append(p)
        p = {k: float(np.median([r[k] for r in rows])) for k in rows[0]}
        nl, nt = int(p["linearisations"]), int(p["trials"])
        edges = o.n_pt_edges + 2 * o.n_line_obs + o.n_manh_edges + o.n_par_edges + o.n_perp_edges
        print("%s: %s; %d edges (%d point, %d line observations, %d Manhattan, %d par, %d perp); iterations %s trials %s"
              % (shape, what, edges, o.n_pt_edges, o.n_line_obs, o.n_manh_edges, o.n_par_edges, o.n_perp_edges, o.iterations, o.trials))
        print("   per linearisation %.3f ms (%d of them), per trial %.3f ms (%d), of a trial the factorisation %.3f ms; launches %.2f ms, whole call on the stream %.2f ms, "
              "wall with the binding %.2f ms" % (p["linearise_ms"] / max(nl, 1), nl, p["trials_ms"] / max(nt, 1), nt, p["factor_ms"] / max(nt, 1),
                                                p["linearise_ms"] + p["trials_ms"], p["call_ms"], p["wall"]))
        if cpu:
            t0 = time.perf_counter(); ref.local_map_optimization(W); dt = time.perf_counter() - t0
            print("   numpy restatement on this host, one thread (not g2o): %.0f ms" % (dt * 1e3))
    ba.close()


if __name__ == "__main__":
    main()
