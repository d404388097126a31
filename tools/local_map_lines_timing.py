#!/usr/bin/env python3
"""Times the local-map line search (hvo_search_lines_by_projection_map: k_lsbp_map_keys + k_lsbp_map_epilogue) for nq map lines against nt
current lines, nq in {500, 2000, 8192} x nt in {200, 2000}.  Current lines: a synthetic sequence's LSD lines (640x480 for 200, 1280x960 at
2000 features for 2000, topped up with the next frame's lines) with their 3-D lines and line grid; queries: the previous frame's lines
shifted into the frame (tests/test_local_map_lines_gpu.py's map_queries), repeated up to nq.  Prints one JSON line per configuration with the
host-clock time of the whole call (uploads, both kernels, the download; it ends in a stream synchronise).  Run it under
`rocprofv3 --kernel-trace --stats` for the kernels' device time.

    python tools/local_map_lines_timing.py [--calls 20]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as G                                    # noqa: E402
hvo = G.package()
import importlib                                              # noqa: E402
synth = importlib.import_module("hvo_amd.synth")
from test_local_map_lines_gpu import map_queries               # noqa: E402


def scene(ctx, w, h, nt, seed):
    g, d, off = synth.make_sequence("std", seed, 3, w=w, h=h)
    fr = []
    for k in range(3):
        kl, ld, fn = ctx.extract_lsd(g[k])
        fr.append((kl, ld, fn, ctx.lines_3d(kl, d[k], seed=3 + k)))
    cat = lambda i: np.concatenate([fr[1][i], fr[2][i]])[:nt]
    klt, dt, fnt, l3t = cat(0), cat(1), cat(2), cat(3)
    assert len(klt) == nt, (len(klt), nt)
    b4 = np.array([0.0, w, 0.0, h], np.float32)
    cs, ci = ctx.assign_lines_to_grid(klt, b4)
    q, vc, wv, qd = map_queries(fr[0][0], fr[0][3], fr[0][1], (off[1] - off[0]).astype(np.float32), 1)
    return (klt, fnt, l3t, dt, cs, ci, b4), (q, vc, wv, qd)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args()
    for nt, (w, h, nfeat) in ((200, (640, 480, 200)), (2000, (1280, 960, 2000))):
        kw = dict(fx=535.4 * w / 640, fy=539.2 * h / 480, cx=320.1 * w / 640, cy=247.6 * h / 480) if w != 640 else {}
        ctx = hvo.Context(lsd_nfeatures=nfeat, **kw)
        try:
            (klt, fnt, l3t, dt, cs, ci, b4), (q, vc, wv, qd) = scene(ctx, w, h, nt, 0x5EED6A00 + nt)
            for nq in (500, 2000, 8192):
                idx = np.tile(np.arange(len(q)), -(-nq // len(q)))[:nq]
                a = (q[idx], vc[idx], wv[idx], qd[idx], (np.arange(nq) % 3 != 0).astype(np.uint8), klt, fnt, l3t, dt, None, cs, ci, b4)
                for _ in range(3):
                    n, _, _ = ctx.search_lines_by_projection_map(*a, th=1.0)
                t = []
                for _ in range(args.calls):
                    t0 = time.perf_counter()
                    ctx.search_lines_by_projection_map(*a, th=1.0)
                    t.append((time.perf_counter() - t0) * 1e3)
                print(json.dumps(dict(nq=nq, nt=nt, n_items=int(cs[-1]), n_matches=n, calls=args.calls, call_ms_median=round(float(np.median(t)), 4),
                                      call_ms_min=round(float(np.min(t)), 4))), flush=True)
        finally:
            ctx.close()


if __name__ == "__main__":
    main()
