"""CPU checks of the relocalisation PnP solver: the restatement tests/pnp_ref.py against known answers, numpy.linalg and planted poses; the
events formulation against the literal iterate() / Refine() loop; tools/pnp_host.cpp (the text the kernels are compiled from, with a group of
one lane) against the restatement bit for bit; every crafted GPU case reaches the path it is meant for; the new ABI's declarations and layouts."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import pnp_ref as ref
from conftest import ROOT

_cache = {}


def solved(name):
    if name not in _cache:
        c = ref.cases()[name]
        _cache[name] = (c, [ref.solve(p, ref.CAM, c["P"], j=j, want_err=True) for j, p in enumerate(c["problems"])])
    return _cache[name]


# ---------------------------------------------------------------------------------------------- SetRansacParameters
@pytest.mark.parametrize("N, min_inl, max_its, T", [(100, 50, 35, 43), (20, 10, 35, 43), (15, 10, 14, 22), (10, 10, 1, 9), (9, 10, None, 0)])
def test_set_ransac_known_answers(N, min_inl, max_its, T):
    """(0.99, 10, 300, 4, 0.5, 5.991), src/Tracking.cc:3805: ceil(log(0.01) / log(1 - 0.5^3)) = 35; N = 15: epsilon = 10/15, 14; N == minInliers: 1"""
    S = ref.set_ransac(ref.default_params(), N)
    assert S["min_inliers"] == min_inl and S["T"] == T and S["no_more"] == (N == 9)
    if max_its is not None:
        assert S["max_its"] == max_its
    if N == 15:
        assert S["epsilon"] == np.float32(10) / np.float32(15)


# ---------------------------------------------------------------------------------------------- the Jacobi eigen-solver
@pytest.mark.parametrize("n, rank", [(3, 3), (3, 2), (12, 12), (12, 8)])
def test_jacobi_against_eigh(n, rank):
    """random symmetric PSD matrices, also of rank 8 (the four-point case: a null space of dimension 4).  Measured here: eigenvalues agree
    within 3e-15 of the largest, the projector onto the four smallest eigenvectors within 2e-13 (rank 8: the null space is exact; full
    rank: gaps of random spectra).  The bounds below carry a margin of about 10."""
    rng = np.random.RandomState(n * 100 + rank)
    B = rng.randn(64, rank, n)
    A = np.einsum("hri,hrj->hij", B, B)
    d, ut = ref.jacobi_eig(A)
    w, v = np.linalg.eigh(A)
    scale = w[:, -1:]
    assert np.abs(d - np.abs(w[:, ::-1])).max() / scale.max() < 3e-14
    assert (np.diff(d, axis=1) <= 1e-12 * scale).all()                      # descending
    assert np.abs(np.einsum("hik,hjk->hij", ut, ut) - np.eye(n)).max() < 1e-13  # orthonormal rows
    k = min(4, n - 1) if rank == n else n - rank
    P1 = np.einsum("hki,hkj->hij", ut[:, n - k:], ut[:, n - k:])
    P2 = np.einsum("hik,hjk->hij", v[:, :, :k], v[:, :, :k])
    assert np.abs(P1 - P2).max() < 2e-12


# ---------------------------------------------------------------------------------------------- EPnP alone
@pytest.mark.parametrize("n, coplanar", [(4, False), (5, False), (6, False), (50, False), (50, True), (300, False)])
def test_epnp_on_planted_poses(n, coplanar):
    """no noise: from five points on the planted pose comes back.  The bound: the float32 rounding of a 600-pixel coordinate is 3e-5 pixel,
    6e-8 rad over the focal length, and a five-point set may amplify that by a few hundred: 2e-5.  n = 4 is held to what EPnP promises there:
    M is 8 x 12, its null space has dimension >= 4, the three beta approximations plus Gauss-Newton may end in another stationary point (the
    reason PnPsolver wraps it in RANSAC), so only a finite proper rotation is asserted and the errors are printed.  The same holds for the
    exactly coplanar set: the fourth control point coincides with the centroid there (this EPnP has no planar case) and ABt loses rank, so its cut singular value leaves a finite matrix that is no rotation."""
    worst = 0.0
    for seed in range(6):
        sc = ref.planted_scene(700 + seed, n, coplanar=coplanar)
        R, t = ref.epnp(sc["p3d"][None].astype(np.float64), sc["p2d"][None].astype(np.float64), sc["cam"])
        assert np.isfinite(R).all() and np.isfinite(t).all()
        assert coplanar or (np.abs(R[0] @ R[0].T - np.eye(3)).max() < 1e-12 and abs(np.linalg.det(R[0]) - 1) < 1e-12)
        worst = max(worst, np.abs(np.concatenate([R[0], t[0][:, None]], 1).reshape(12) - sc["Tcw"]).max())
    print("n = %d coplanar = %s: max |Tcw - planted| = %.3g" % (n, coplanar, worst))
    assert n == 4 or coplanar or worst < 2e-5


def test_planted_pose_error_of_the_restatement():
    """max |Tcw - planted| of the restatement's refined pose over the planted scenes of the GPU tests: 1.2e-7 measured; the GPU tests' bound
    is that with a margin of 4 (POSE_TOL = 4.8e-7)"""
    worst = 0.0
    for name in ("clean40", "refine280", "rows32", "rows33", "rows64", "rows65"):
        c, s = solved(name)
        worst = max(worst, np.abs(s[0]["events"][-1]["Tcw"] - c["problems"][0]["Tcw"]).max())
    print("max |Tcw - planted| = %.3g" % worst)
    assert worst <= 1.2e-7


# ---------------------------------------------------------------------------------------------- the events formulation against the literal loop
def crafted_runs():
    """(name, counts per iteration, refined count per record iteration0) with min_inliers = 10, max_its = 12"""
    return [
        ("no passing iteration", [3, 9, 0, 5, 9, 9, 2, 1, 0, 4, 5, 6, 7, 8, 9, 9], {}),
        ("one record", [3, 12, 0, 5, 9, 9, 2, 1, 0, 4, 5, 6, 7, 8, 9, 9], {1: 14}),
        ("several records", [10, 3, 12, 12, 15, 2, 11, 20, 1, 1, 1, 1, 1, 1, 1, 1], {0: 10, 2: 10, 4: 9, 7: 10}),
        ("a record whose Refine fails, then one that succeeds", [3, 10, 4, 10, 13, 2, 11, 0, 0, 0, 0, 0, 0, 0, 0, 0], {1: 10, 4: 13}),
        ("a passing non-record after a success", [11, 0, 11, 10, 0, 0, 12, 11, 0, 0, 0, 0, 0, 0, 0, 0], {0: 11, 6: 9}),
        ("overrun past maxIts", [0, 0, 0, 0, 0, 0, 0, 0, 0, 11, 0, 0, 0, 15, 0, 16, 0, 0, 0, 0], {9: 11, 13: 16, 15: 10}),
        ("a record of exactly min_inliers only", [0, 10, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0], {1: 10}),
    ]


@pytest.mark.parametrize("chunk", [1, 5, 7])
@pytest.mark.parametrize("run", crafted_runs(), ids=lambda r: r[0])
def test_events_formulation_against_the_literal_loop(hvo, run, chunk):
    """drive both with the same crafted counts / masks / refine outcomes: the sequences of returns are identical, call by call"""
    name, counts, refined = run
    T, N, nf, min_inl, max_its = len(counts), 24, 30, 10, 12
    fi = np.arange(N) + 3
    mask_of = lambda it0: ((np.arange(N) * 7 + it0 * 3) % N < counts[it0]).astype(np.uint8)
    tcw_of = lambda it0, refined_: np.full(12, it0 + (0.5 if refined_ else 0.0), np.float32)
    rmask_of = lambda it0: ((np.arange(N) * 5 + it0) % N < refined[it0]).astype(np.uint8)
    by_feature = lambda m: np.bincount(fi[m != 0], minlength=nf).astype(np.uint8)

    def hyp(it):
        return None if it > T else (counts[it - 1], ("h", it - 1), tcw_of(it - 1, False))

    def refine(best):
        it0 = best[1]
        return refined[it0], ("r", it0), tcw_of(it0, True)
    lit = ref.LiteralSolver(N, min_inl, max_its, hyp, refine)
    ev = ref.events_from_counts(counts, min_inl, lambda it0: refined[it0], 8)
    assert sorted(refined) == ev["records"], "the crafted refine table names exactly the records"
    res = dict(N=N, min_inliers=min_inl, max_its=max_its, T=T, hyp_inliers=np.array(counts, np.int32), hyp_event=ev["hyp_event"],
               events=[dict(iteration=it0 + 1, n_inliers=refined[it0], success=refined[it0] > min_inl, Tcw=tcw_of(it0, True), inliers=by_feature(rmask_of(it0)),
                            hyp_n_inliers=counts[it0], hyp_Tcw=tcw_of(it0, False), hyp_inliers=by_feature(mask_of(it0))) for it0 in ev["records"]])
    state, n_returns = {}, 0
    for call in range(40):
        a = lit.iterate(chunk)
        b = hvo.pnp_iterate(res, state, chunk)
        assert state["mnIterations"] == lit.mnIterations, (name, call)
        assert (a[0] is None) == (b[0] is None) and a[1] == b[1] and a[3] == b[3], (name, call, a, b)
        if a[0] is not None:
            n_returns += 0 if a[1] else 1
            assert np.array_equal(a[0], b[0])
            kind, it0 = a[2]
            assert np.array_equal(b[2], by_feature(rmask_of(it0) if kind == "r" else mask_of(it0))), (name, call)
        if a[1]:
            break
    else:
        raise AssertionError("the loop never reported bNoMore")
    if name == "overrun past maxIts":                             # the call after the return at 10 starts before maxIts = 12: a chunk > 2 runs past it to the record at 14
        assert n_returns == (1 if chunk == 1 else 2)


# ---------------------------------------------------------------------------------------------- tools/pnp_host.cpp
def test_host_restatement_equals_pnp_ref(tmp_path):
    """tools/pnp_host.cpp compiles csrc/pnp_core.inc, the text of the kernels, for one lane: SetRansacParameters (N = 100, 20, 15, 10, 9 among the
    candidates), samples, counts, masks, the records, their refined counts and the float32 poses equal the numpy restatement's bit for bit"""
    exe = str(tmp_path / "pnp_host")
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-ffp-contract=off", ROOT + "/tools/pnp_host.cpp", "-o", exe])
    for P, probs in ((ref.default_params(seed=3), [ref.planted_scene(50 + n, n, 0.3 if n > 20 else 0.0) for n in (100, 20, 15, 10, 9, 300)]),
                     (ref.default_params(seed=4, min_set=40, extra_iterations=1), [ref.planted_scene(61, 90)])):
        ref.write_problem_file(str(tmp_path / "p.bin"), probs, ref.CAM, P)
        subprocess.check_output([exe, str(tmp_path / "p.bin"), str(tmp_path / "r.bin")])
        got = ref.read_host_result(str(tmp_path / "r.bin"), len(probs), P["min_set"])
        for j, (g, p) in enumerate(zip(got, probs)):
            w = ref.solve(p, ref.CAM, P, j=j)
            for k in ("N", "min_inliers", "max_its", "T", "no_more"):
                assert g[k] == w[k], (j, k)
            assert np.float32(g["epsilon"]).tobytes() == np.float32(w["epsilon"]).tobytes()
            if w["T"] == 0:
                continue
            assert np.array_equal(g["hyp_sample"], w["hyp_sample"]) and np.array_equal(g["hyp_inliers"], w["hyp_inliers"]) and np.array_equal(g["hyp_mask"], w["hyp_mask"]), j
            assert len(g["records"]) == len(w["events"])
            for r, e in zip(g["records"], w["events"]):
                assert r["it0"] + 1 == e["iteration"] and r["count"] == e["n_inliers"] and r["Tcw"].tobytes() == e["Tcw"].tobytes(), j
            if w["best_iteration"]:
                assert g["hyp_Tcw"][w["best_iteration"] - 1].tobytes() == w["best_Tcw"].tobytes()
    S = [g for g in got]
    assert S[0]["T"] > 0


# ---------------------------------------------------------------------------------------------- the crafted GPU cases reach their paths
def test_no_error_sits_on_its_threshold():
    """in every crafted case no correspondence's error2 lies within 1e-6 relative of its threshold, in any hypothesis or Refine: a last-bit
    difference in a pose could not flip an inlier"""
    for name, c in ref.cases().items():
        _, s = solved(name)
        for p, r in zip(c["problems"], s):
            me = np.asarray(p["sigma2"], np.float32) * np.float32(c["P"]["th2"])
            for e2 in r["err2"]:
                rel = np.abs(e2.astype(np.float64) - me[None, :]) / me[None, :]
                assert not (rel[np.isfinite(rel)] < 1e-6).any(), name


def test_crafted_cases_reach_their_paths():
    s = solved("clean40")[1][0]
    assert s["events"][0]["success"] and s["events"][0]["n_inliers"] == 40
    assert solved("edge9")[1][0]["T"] == 0 and solved("edge9")[1][0]["no_more"]
    assert solved("edge10")[1][0]["max_its"] == 1 and solved("edge10")[1][0]["min_inliers"] == 10
    assert solved("edge15")[1][0]["max_its"] == 14
    for n in (63, 64, 65, 130):
        r = solved("edge%d" % n)[1][0]
        assert r["T"] == 43 and r["events"] and r["events"][-1]["success"], n
    for name in ("coplanar", "duplicates"):
        r = solved(name)[1][0]
        assert r["events"] and all(np.isfinite(e["Tcw"]).all() for e in r["events"]), name
    c, s = solved("coplanar")
    pw = c["problems"][0]["p3d"].astype(np.float64); pw = pw - pw.mean(0)
    assert np.linalg.svd(pw, compute_uv=False)[2] < 1e-5 * np.linalg.svd(pw, compute_uv=False)[0]      # the points are coplanar: cvInvert's pseudo-inverse path
    r = solved("two_pose")[1][0]
    assert [(e["n_inliers"], e["success"]) for e in r["events"]] == [(10, False), (11, True)]
    assert (r["hyp_event"][:r["events"][1]["iteration"] - 1] == -1).all() and (r["hyp_event"] == 1).sum() >= 2      # a passing non-record after the success
    r = solved("overflow")[1][0]
    assert r["status"] == -5 and len(r["events"]) == 1 and (r["hyp_event"] == -1).all()
    r = solved("refine280")[1][0]
    assert r["events"][0]["n_inliers"] > 256 and r["hyp_inliers"][r["events"][0]["iteration"] - 1] > 256
    for n in (32, 33, 64, 65):
        r = solved("rows%d" % n)[1][0]
        it0 = r["events"][-1]["iteration"] - 1
        assert r["hyp_inliers"][it0] == n and r["events"][-1]["n_inliers"] == n, n      # the Refine ran on exactly n correspondences
    assert solved("minset5")[1][0]["events"] and solved("minset64")[1][0]["events"]
    assert solved("minset64")[1][0]["hyp_sample"].shape[1] == 64
    for n_kf in (1, 3, 17):
        assert len({len(p["p3d"]) for p in ref.multi_problems(n_kf)}) == n_kf


# ---------------------------------------------------------------------------------------------- the new ABI
def test_header_declares_the_pnp_boundary():
    hdr = open(os.path.join(ROOT, "include", "hvo.h")).read()
    for n in ("hvo_pnp_default_params", "hvo_pnp_ransac", "hvo_stream_pnp_ransac", "hvo_pnp_last_kernel_ms", "hvo_stream_pnp_last_kernel_ms"):
        assert re.search(r"\b%s\s*\(" % n, hdr), n
    for t in ("hvo_pnp_params", "hvo_pnp_problem", "hvo_pnp_event", "hvo_pnp_result", "hvo_pnp_keyframe_side"):
        assert re.search(r"\}\s*%s;" % t, hdr), t
    assert re.search(r"#define HVO_ABI_VERSION 3\b", hdr)


def test_pnp_struct_layouts(hvo, tmp_path):
    """sizes and field offsets of the ctypes mirrors equal the C compiler's"""
    structs = {"hvo_pnp_params": hvo.PnpParams, "hvo_pnp_problem": hvo.PnpProblem, "hvo_pnp_event": hvo.PnpEvent, "hvo_pnp_result": hvo.PnpResult,
               "hvo_pnp_keyframe_side": hvo.PnpKeyframeSide}
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "hvo.h"', 'int main(void) {']
    for cn, st in structs.items():
        src.append('printf("%s %%zu", sizeof(%s));' % (cn, cn))
        for f, _ in st._fields_:
            src.append('printf(" %%zu", offsetof(%s, %s));' % (cn, f))
        src.append('printf("\\n");')
    src.append("return 0; }")
    (tmp_path / "l.c").write_text("\n".join(src))
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(tmp_path / "l.c"), "-o", str(tmp_path / "l")])
    for line in subprocess.check_output([str(tmp_path / "l")]).decode().splitlines():
        w = line.split(); st = structs[w[0]]
        assert ctypes.sizeof(st) == int(w[1]), w[0]
        assert [getattr(st, f).offset for f, _ in st._fields_] == [int(v) for v in w[2:]], w[0]
    P = hvo.pnp_params()
    assert (P.probability, P.min_inliers, P.max_iterations, P.min_set, P.extra_iterations, P.max_events) == (0.99, 10, 300, 4, 8, 8)
    assert P.epsilon == np.float32(0.5) and P.th2 == np.float32(5.991)


def test_example_compiles_against_the_mirror():
    """examples/relocalization_pnp.cpp, the caller of hvo::PnPsolver, against the C++ mirror, as the other examples are checked;
    tests/test_pnp_gpu.py links and runs it"""
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I" + ROOT + "/include", "-fsyntax-only", ROOT + "/examples/relocalization_pnp.cpp"])
