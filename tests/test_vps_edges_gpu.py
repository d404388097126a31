"""Vanishing-point clustering (csrc/vps.hip) on crowded sphere grids and crafted edges: the paths tests/test_vps.py never reaches.

    path of vps.hip                                             case that reaches it (precondition asserted on the CPU, tests/vps_cases.py)
    k_vp_grid, owner lane's sort, cell of <= 48 pairs           every case
    k_vp_grid, workgroup rank, cell of > 48 pairs               overflow_1024, boundary_48_49 (one trip and, above 1024 pairs, two)
    k_vp_grid, table full -> back to the owner lane's sort      overflow_1024 (more than 2048 cells above 48 pairs), resident_above_1024
    the threshold itself                                        boundary_48_49 (cells of exactly 48 and of exactly 49 pairs)
    k_vp_lines / k_vp_pairs tiles of 256, pair rank, % n        count_sweep (n = 2 .. 1024; 1025 refused)
    more than 1024 lines (resident forms only)                  resident_above_1024 (stream and batch, lsd_nfeatures = 1280)
    k_vp_hyp redraws that succeed beside groups that give up    redraw_mixed
    LO >= 360 -> 359, "no score above 0 -> best = 0", rs == 0   lo_clamp, no_score, seed_fixup
    line2Vps on a NaN direction, th_angle = pi and 1e-12        line2vps_edges
    arrival order of the LDS atomics must not show              determinism

The reference is the CPU oracle (oracle/vps.c) with the comparison rules of tests/test_vps.py, unchanged: grid rtol 1e-10 / atol 1e-9, score
1e-9 relative, vps 1e-12, vp_idx equal, 37 800 hypotheses, and the twin rule when the best index differs.  The numpy restatement in
tests/vps_cases.py states the preconditions: pairs per cell, and that no pair of a random case lies within 1e-9 cell of a cell border (where
the device's acos / atan2 could legitimately pick the neighbour).  It is checked against the oracle's grid and never sees device output."""
import numpy as np
import pytest

import vps_cases as vc

LSD, VP = 2, 32


@pytest.fixture(scope="module")
def cases(orc):
    return vc.host_cases(orc)


@pytest.fixture(scope="module")
def resident(orc):
    return vc.resident_case(orc)


@pytest.fixture(scope="module")
def ctx512(hvo):
    fx, fy, cx, cy = vc.K_512
    ctx = hvo.Context(fx=fx, fy=fy, cx=cx, cy=cy)
    yield ctx
    ctx.close()


def check_vp(orc, got, kl, seed, ref, K=vc.K_DEFAULT, th=None):
    """the rules of tests/test_vps.py::test_vp_gpu_vs_oracle (got has no "grid" in the resident forms)"""
    assert got["n_hypotheses"] == 37800
    if "grid" in got:
        assert np.allclose(got["grid"], ref["grid"], rtol=1e-10, atol=1e-9), \
            (np.abs(got["grid"] - ref["grid"]).max(), np.argwhere(~np.isclose(got["grid"], ref["grid"], rtol=1e-10, atol=1e-9))[:8].tolist())
    assert abs(got["score"] - ref["score"]) <= 1e-9 * max(1.0, ref["score"]), (got["score"], ref["score"])
    if got["best"] != ref["best"]:
        assert abs(ref["scores"][got["best"]] - ref["score"]) <= 1e-9 * max(1.0, ref["score"]), (got["best"], ref["best"])
        twin = orc.vp_hypothesis(kl, seed, got["best"], fx=K[0], cx=K[2], cy=K[3])
        assert np.allclose(got["vps"], twin, atol=1e-12)
        assert np.array_equal(got["vp_idx"], orc.vp_line2vps(kl, twin, th_angle=th, fx=K[0], fy=K[1], cx=K[2], cy=K[3]))
    else:
        assert np.allclose(got["vps"], ref["vps"], atol=1e-12)
        assert np.array_equal(got["vp_idx"], ref["vp_idx"])


def run_case(orc, ctx, c):
    got = ctx.vanishing_points(c["kl"], seed=c["seed"], th_angle=c["th"], want_grid=True)
    check_vp(orc, got, c["kl"], c["seed"], c["ref"], c["K"], c["th"])
    return got


def test_vp_preconditions_hold_without_a_gpu(cases, resident):
    """every precondition of the case list (asserted where the cases are built), the restatement against the oracle's grid of every case,
    the border margin of every random case; nothing here touches a device"""
    assert {"overflow_1024", "boundary_48_49", "redraw_40_1", "redraw_3", "lo_clamp", "lo_mirror", "no_score", "l2v_default", "l2v_pi", "l2v_1e-12"} <= set(cases)
    assert all("sweep_%d" % n in cases for n in vc.SWEEP_N) and all("seed_%08x" % s in cases for s in vc.SEED_FIXUP)
    for name, c in cases.items():
        assert c["random"] == (name not in ("lo_clamp", "lo_mirror", "no_score")) and (not c["random"] or c["border"] > vc.BORDER_MARGIN), name
    assert len(resident["kl"]) > vc.VP_MAX_LINES and resident["border"] > vc.BORDER_MARGIN
    # k_vp_grid's serial work on the resident frame, were every lone-lane cell sorted by ONE lane: a few million dependent moves, seconds at most
    print("resident frame: %d lines, %d cells above %d pairs (largest %d), lone-lane moves <= %.3g" %
          (len(resident["kl"]), (resident["cnt"] > vc.VP_BIG).sum(), vc.VP_BIG, resident["cnt"].max(), resident["steps"]))
    assert resident["steps"] < 2e7


@pytest.mark.gpu
def test_overflow_1024_fills_the_big_cell_table(orc, gpu_ctx, cases):
    """gap 1, the k_vp_grid overflow fallback: 1024 segments in an 80 x 80 px box put more than VP_BIGMAX = 2048 cells above VP_BIG = 48
    pairs (precondition: 2242, the largest 339), so some of them find the table full and keep the owner lane's sort; which ones depends
    on arrival order, the sums must not"""
    c = cases["overflow_1024"]
    assert (c["cnt"] > vc.VP_BIG).sum() > vc.VP_BIGMAX
    run_case(orc, gpu_ctx, c)


@pytest.mark.gpu
def test_boundary_48_49_and_a_cell_of_two_trips(orc, gpu_ctx, cases):
    """gap 3, the threshold between the two orderings: cells of exactly 48 pairs (owner lane) and of exactly 49 (workgroup) both occur, and a
    cell of more than 1024 pairs takes the workgroup's rank loop into a second trip (precondition: 5, 7 and 1924 pairs)"""
    c = cases["boundary_48_49"]
    assert (c["cnt"] == 48).any() and (c["cnt"] == 49).any() and c["cnt"].max() > 1024
    run_case(orc, gpu_ctx, c)


@pytest.mark.gpu
@pytest.mark.parametrize("n", vc.SWEEP_N)
def test_count_sweep(orc, gpu_ctx, cases, n):
    """gap 5, small and block-edge counts: the pair rank p = i (2n - i - 1) / 2 + (j - i - 1), the 256-wide tiles of k_vp_lines and
    k_vp_pairs and the `% n` draws at n = 2, 3, 4, around 64 and 256, and at the host form's limit"""
    c = cases["sweep_%d" % n]
    assert len(c["kl"]) == n
    run_case(orc, gpu_ctx, c)


@pytest.mark.gpu
def test_1025_lines_are_refused_by_the_host_form(hvo, orc, gpu_ctx, cases):
    """gap 2, the host form's side of it: hvo_vanishing_points takes at most 1024 lines; the context goes on working"""
    with pytest.raises(hvo.HvoError):
        gpu_ctx.vanishing_points(vc.random_segments(orc, 1025, 1))
    run_case(orc, gpu_ctx, cases["sweep_4"])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["redraw_40_1", "redraw_3"])
def test_redraw_mixed(orc, gpu_ctx, cases, name):
    """gap 4, redraws that succeed: 40 exactly parallel lines and one oblique one -- a draw is non-parallel with probability 0.05, so most
    groups redraw (pt[2] == 0 -> continue) a few times and succeed while some use up their 64 draws and give up (precondition: both kinds
    occur, by orc.vp_hypothesis over the 105 groups) -- and 3 lines of which two are parallel (many short redraws).  The device must
    consume the xorshift stream exactly as oracle/vps.c does: the score and the best hypothesis depend on every group's pair"""
    c = cases[name]
    assert not c["gave_up"].all() and (name != "redraw_40_1" or c["gave_up"].any())
    got = run_case(orc, gpu_ctx, c)
    assert got["score"] > 0 and not c["gave_up"][got["best"] // 360]


@pytest.mark.gpu
def test_lo_clamp_and_its_mirror(orc, ctx512, cases):
    """gap 6, the LO >= 360 -> 359 clamp: with fx = fy = 512, cx = 320, cy = 240 the two segments meet exactly at (320, 100), X = +0,
    Y < 0, longitude 2 pi -- raw cell (15, 359), which the border-zeroing smooth shows as (14..16, 358), score 0, best 0.  The mirror
    image meets at (320, 400): longitude pi, a 3 x 3 block round (17, 180).  Both cells are libm-independent: atan2(+0, y) is exactly
    pi or +0.  The device's non-zero support must be the oracle's"""
    for name in ("lo_clamp", "lo_mirror"):
        c = cases[name]
        got = run_case(orc, ctx512, c)
        assert np.array_equal(got["grid"] != 0, c["ref"]["grid"] != 0), (name, np.argwhere(got["grid"] != 0).tolist())
    assert np.argwhere(got["grid"] != 0).tolist() == [[i, j] for i in (16, 17, 18) for j in (179, 180, 181)]
    assert run_case(orc, ctx512, cases["lo_clamp"])["best"] == 0


@pytest.mark.gpu
def test_no_score_keeps_hypothesis_zero(orc, ctx512, cases):
    """gap 6, "no score above 0 -> best = 0" with n >= 2: two lines crossing at the principal point 90 degrees apart fill no cell; the result
    is hypothesis 0 (finite), score 0, both lines in cluster 0"""
    got = run_case(orc, ctx512, cases["no_score"])
    assert not got["grid"].any() and got["score"] == 0 and got["best"] == 0 and np.isfinite(got["vps"]).all() and got["vp_idx"].tolist() == [0, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("seed", vc.SEED_FIXUP)
def test_seed_fixup(orc, gpu_ctx, cases, seed):
    """gap 6, the rs == 0 fix-up: seed 0x9E3779B9 zeroes the xorshift state of group 0, 0x9E3779B9 * 105 mod 2^32 that of group 104; seed 0"""
    run_case(orc, gpu_ctx, cases["seed_%08x" % seed])


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["default", "pi", "1e-12"])
def test_line2vps_edges(orc, gpu_ctx, cases, name):
    """gap 6, line2Vps on a zero-length line (NaN direction: no angle compares below 1000, cluster 3 at every th_angle) and at th_angle = pi
    (every other line joins a cluster) and 1e-12 (none does)"""
    got = run_case(orc, gpu_ctx, cases["l2v_" + name])
    assert got["vp_idx"][-1] == 3


@pytest.mark.gpu
def test_determinism_on_a_crowded_grid(hvo, orc, gpu_ctx, cases):
    """gap 7: k_vp_grid fills order[] by LDS atomics in arrival order and decides by arrival which crowded cells the workgroup orders; on
    overflow_1024 (all three ordering paths mixed: precondition as above) two calls on one context and one on a fresh context agree byte
    for byte in grid, vps, score, best and vp_idx"""
    c = cases["overflow_1024"]
    assert (c["cnt"] > vc.VP_BIG).sum() > vc.VP_BIGMAX and (c["cnt"] <= vc.VP_BIG).any()
    runs = [gpu_ctx.vanishing_points(c["kl"], seed=c["seed"], want_grid=True) for _ in range(2)]
    fresh = hvo.Context()
    try:
        runs.append(fresh.vanishing_points(c["kl"], seed=c["seed"], want_grid=True))
    finally:
        fresh.close()
    blob = [b"".join([r["grid"].tobytes(), r["vps"].tobytes(), np.float64(r["score"]).tobytes(), np.int32(r["best"]).tobytes(), r["vp_idx"].tobytes()]) for r in runs]
    assert blob[0] == blob[1] == blob[2]


def check_resident(orc, r, seed):
    kl = r["kl"]
    assert r["status"] == 0 and r["tail_status"] == 0 and len(kl) > vc.VP_MAX_LINES
    cnt = vc.counts(vc.pair_cells(kl))                                # of the frame's own key lines: the precondition, not a comparison
    assert (cnt > vc.VP_BIG).sum() > vc.VP_BIGMAX
    check_vp(orc, r["vp"], kl, seed, orc.vanishing_points(kl, seed=seed, want_scores=True))


@pytest.mark.gpu
def test_resident_above_1024_stream(hvo, orc, resident):
    """gap 2, more than 1024 key lines: only the resident forms take them (vp_enqueue sizes everything by lsd_nfeatures).  One 1280 x 960
    frame of tiled tilted rectangles through hvo_stream_* with lsd_nfeatures = 1280, stages LSD + VP (precondition: the oracle extracts
    1280 lines from it, and the frame's own lines put more than 2048 cells above 48 pairs: gap 1 on a real image); vp against the oracle
    on the frame's own key lines"""
    st = hvo.Stream(width=vc.RESIDENT_W, height=vc.RESIDENT_H, depth=2, stages=LSD | VP, seed=9, lsd_nfeatures=vc.RESIDENT_NFEAT)
    try:
        t = st.submit(resident["gray"])
        check_resident(orc, st.collect(t), 9 + t)
    finally:
        st.close()


@pytest.mark.gpu
def test_resident_above_1024_batch(hvo, orc, resident):
    """gap 2 in the batch form (hvo_batch_run with HVO_STAGE_VP): the same frame, the same rules"""
    ctx = hvo.Context(max_batch=1, lsd_nfeatures=vc.RESIDENT_NFEAT)
    try:
        ctx.batch_upload(resident["gray"][None])
        ctx.set_tail_params(seed=9)
        ctx.batch_run(LSD | VP)
        res = ctx.batch_download(LSD)
        ctx.batch_download_tail(LSD | VP, res)
        check_resident(orc, res[0], 9)
    finally:
        ctx.close()
