"""Whole batches at the sizes where the launch plans change form (tests/test_launch_plan.py holds the thresholds): every frame of every
batch is downloaded and looked at.

Geometry 200 x 160 with the camera of synth.intrinsics(200, 160) and the default extractor parameters; sixteen distinct frames, frame f
of a batch is distinct frame f % 16.  For every batch size, with max_batch = n, no HVO_* variable set and every stage:
  1. the context's launch report equals the table's row for n (imported, not copied);
  2. every frame's status is 0;
  3. the first occurrence of each distinct frame equals the CPU oracle under the rules of test_orb_gpu.check_orb, test_lsd_gpu.check and
     test_peac_gpu.check, unchanged;
  4. every later occurrence is byte-equal to the first in every array and count (each stage is bit-reproducible; a difference that depends
     on the position in the batch is a race, a chunk offset, a permutation slot or a ragged last wave).
For 65 and 513 frames the whole Frame constructor runs as well (culling and the tail stages walk the same chunks); the tail stages that draw
random numbers (3-D lines, vanishing points) are seeded per frame index, so there every frame is compared with the oracle at its own seed
(check_tail says how) and the seed-free arrays byte for byte as above."""
import os
import time

import numpy as np
import pytest

from test_launch_plan import expected_report

W, H = 200, 160
NDISTINCT = 16
SIZES = [8, 9, 16, 17, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 3071, 3072, 5120, 5121, 6143, 6144]
TAIL_SIZES = [65, 513]
TAIL_SEED = 9
STD_SEEDS = (0x5EEDB008, 0x5EEDB013, 0x5EEDB020, 0x5EEDB021, 0x5EEDB02D, 0x5EEDB036)
LOWTEX_SEEDS = (0x5EEDB000, 0x5EEDB001, 0x5EEDB003, 0x5EEDB006, 0x5EEDB00A, 0x5EEDB00B)
FLAT, NOISE, TIES, CORNER = 12, 13, 14, 15


def camera(synth):
    K = synth.intrinsics(W, H)
    return {k: K[k] for k in ("fx", "fy", "cx", "cy")}


def frame_set(synth):
    """twelve synth frames (std and lowtex alternating), flat grey without depth, noise over one exact plane, a checkerboard over 35 exact
    planes in coarse depth steps (ties everywhere), a textured frame over a three-plane corner"""
    from test_register_forms_gpu import plane_scene
    K = camera(synth); Kt = (K["fx"], K["fy"], K["cx"], K["cy"])
    gs, ds = [], []
    for a, b in zip(STD_SEEDS, LOWTEX_SEEDS):
        for kind, seed in (("std", a), ("lowtex", b)):
            g, d = synth.make_frame(kind, seed, W, H)
            gs.append(g); ds.append(d)
    j = (np.arange(W)[None, :] - Kt[2]) / Kt[0]; i = (np.arange(H)[:, None] - Kt[3]) / Kt[1]
    gs.append(np.full((H, W), 128, np.uint8)); ds.append(np.zeros((H, W), np.uint16))
    gs.append(np.random.default_rng(0xB0DE).integers(0, 256, (H, W), dtype=np.uint8)); ds.append(np.rint(2.0 / (0.1 * j + 0.2 * i + 1.0) * 5000).astype(np.uint16))
    y, x = np.mgrid[0:H, 0:W]
    gs.append(np.where(((x >> 3) + (y >> 3)) & 1, 200, 60).astype(np.uint8)); ds.append(plane_scene(7, 35, W, H, Kt, q=25))
    zs = [2.0 / (a * j + b * i + 1.0) for a, b in ((0.9, 0.5), (-0.9, 0.5), (0.0, -1.0))]          # a box corner pointing at the camera
    corner = np.rint(np.minimum(np.minimum(zs[0], zs[1]), zs[2]) * 5000).astype(np.int32) + np.random.default_rng(3).integers(-6, 7, (H, W))
    gs.append(synth.make_gray("std", 0x5EEDB063, W, H)); ds.append(corner.clip(1, 65535).astype(np.uint16))
    return np.ascontiguousarray(np.stack(gs)), np.ascontiguousarray(np.stack(ds))


@pytest.fixture(scope="module")
def reference(orc, synth):
    """the sixteen frames and the oracle's results for them, computed once; asserts that the set is not degenerate"""
    gray, depth = frame_set(synth)
    K = camera(synth); okw = {k: np.float32(v) for k, v in K.items()}
    o = orc.Orb()
    ref = []
    for f in range(NDISTINCT):
        kp, desc = o.extract(gray[f])
        kl, ld, fn = orc.line_extract(gray[f])
        labels, planes = orc.peac(depth[f], **okw)
        ref.append(dict(kp=kp, desc=desc, kl=kl, ldesc=ld, linefn=fn, labels=labels, planes=planes))
    assert len(gray) == NDISTINCT and len({g.tobytes() for g in gray}) == NDISTINCT and len({d.tobytes() for d in depth}) == NDISTINCT
    assert sum(len(r["planes"]) >= 1 for r in ref) >= 10, [len(r["planes"]) for r in ref]
    assert sum(len(r["kl"]) >= 5 for r in ref) >= 10, [len(r["kl"]) for r in ref]
    assert sum(len(r["kp"]) >= 50 for r in ref) >= 10, [len(r["kp"]) for r in ref]
    e = ref[FLAT]
    assert len(e["kp"]) == 0 and len(e["kl"]) == 0 and len(e["planes"]) == 0 and (e["labels"] == -1).all()
    assert len(ref[NOISE]["planes"]) == 1 and len(ref[CORNER]["planes"]) == 3 and len(ref[TIES]["kl"]) == 200
    return dict(gray=gray, depth=depth, K=K, okw=okw, ref=ref, culled={})


def test_preconditions_hold_without_a_gpu(reference):
    """nothing here touches a device: the fixture runs the sixteen frames through the oracle and asserts what makes the cases non-vacuous
    (at least ten frames with a plane, ten with five key lines, ten with fifty key points, and the empty frame giving none of each)"""
    assert len(reference["ref"]) == NDISTINCT
    assert sorted(set(SIZES)) == SIZES and set(TAIL_SIZES) <= set(SIZES)


def where(n, f):
    """frame f of a batch of n: the places whose arithmetic depends on its position"""
    return "frame %d of %d (distinct frame %d; LSD chunk %d, place %d; AHC wave %d, group %d; occurrence %d)" % (
        f, n, f % NDISTINCT, f // 512, f % 512, f // 4, f % 4, f // NDISTINCT)


def slab(res, key):
    """the (n, capacity, ...) array batch_download made for `key`: the per-frame results are views of it"""
    a = res[0][key].base
    assert a is not None and a.shape[0] == len(res), key
    return a


def assert_occurrences_equal(n, name, a):
    """a: one row per frame; row f must hold the bytes of row f % 16"""
    rows = np.ascontiguousarray(a).reshape(n, -1).view(np.uint8)
    first = rows[:NDISTINCT]
    for c in range(NDISTINCT, n, NDISTINCT):
        blk = rows[c:c + NDISTINCT]
        if not np.array_equal(blk, first[:len(blk)]):
            bad = np.flatnonzero((blk != first[:len(blk)]).any(axis=1))
            f = c + int(bad[0])
            raise AssertionError("%s: %s differs from its first occurrence in %d bytes (%d frames of this array differ in all)" % (
                name, where(n, f), int((rows[f] != rows[f % NDISTINCT]).sum()),
                sum(int((rows[k:k + NDISTINCT] != first[:len(rows[k:k + NDISTINCT])]).any(axis=1).sum()) for k in range(NDISTINCT, n, NDISTINCT))))


def check_primary(n, res, reference, culled):
    from test_orb_gpu import check_orb
    from test_lsd_gpu import check as check_lsd
    from test_peac_gpu import check as check_peac
    ref = reference["ref"]
    # 2. every frame's status
    bad = [f for f in range(n) if res[f]["status"] != 0]
    assert not bad, "status %d, %s (%d frames in all)" % (res[bad[0]]["status"], where(n, bad[0]), len(bad))
    # 3. the first occurrences against the oracle
    for f in range(min(n, NDISTINCT)):
        r, o = res[f], ref[f]
        try:
            check_orb(r["kp"], r["desc"], o["kp"], o["desc"])
            if not culled:
                check_lsd(r["kl"], r["ldesc"], r["linefn"], o["kl"], o["ldesc"], o["linefn"])
            check_peac(r["labels"], r["planes"], o["labels"], o["planes"])
        except AssertionError as e:
            raise AssertionError("against the oracle, %s: %s" % (where(n, f), e))
    # 4. the later occurrences against the first: counts, then whole slabs (what lies beyond a frame's count is the zero it was made with)
    for key in ("kp", "kl", "planes"):
        counts = np.array([len(r[key]) for r in res])
        assert_occurrences_equal(n, "number of " + key, counts)
    for key in ("kp", "desc", "kl", "ldesc", "linefn", "planes", "labels"):
        assert_occurrences_equal(n, key, slab(res, key))


def run_case(hvo, reference, n, stages):
    t0 = time.perf_counter()
    ctx = hvo.Context(max_batch=n, **reference["K"])
    try:
        ctx.batch_upload(reference["gray"], reference["depth"], repeat=(n + NDISTINCT - 1) // NDISTINCT, n=n)
        if stages != hvo.STAGE_ALL:
            ctx.set_tail_params(seed=TAIL_SEED)
        t1 = time.perf_counter()
        ctx.batch_run(stages)
        t2 = time.perf_counter()
        report = ctx.launch_report()
        res = ctx.batch_download(hvo.STAGE_ALL, labels8=True)
        if stages != hvo.STAGE_ALL:
            ctx.batch_download_tail(stages, res)
    finally:
        ctx.close()
    t3 = time.perf_counter()
    return report, res, (t1 - t0, t2 - t1, t3 - t2)


def report_line(n, report, times, total):
    p, l, b = report["peac"], report["lsd"], report["batch"]
    return ("n=%d | AHC %s%s wgs=%d perm=%d | blkmap y=%d | flood %d thr slim=%d | LSD grow=%s%s chunk=%d x%d | sched %d prio %d,%d,%d | "
            "upload %.2f run %.2f download %.2f check %.2f s" % (
                n, p["cluster"], "(H=%d big=%d)" % (p["heads"], p["heads_big"]) if p["cluster"] == "heads" else "", p["cluster_wgs"], p["perm_items"],
                p["blkmap_y"], p["flood_t"], p["flood_slim"], l["grow"], "(W=%d)" % l["async_w"] if l["grow"] == "async" else "", l["chunk"], l["chunks"],
                b["sched"], b["prio_orb"], b["prio_lsd"], b["prio_peac"], times[0], times[1], times[2], total - sum(times)))


@pytest.fixture
def clean_env(monkeypatch):
    for k in list(os.environ):
        if k.startswith("HVO_"):
            monkeypatch.delenv(k)
    return monkeypatch


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_whole_batch_at_a_plan_boundary(hvo, reference, clean_env, n):
    t0 = time.perf_counter()
    report, res, times = run_case(hvo, reference, n, hvo.STAGE_ALL)
    assert len(res) == n
    try:
        assert report == expected_report(W, H, n, stages=hvo.STAGE_ALL), {s: {f: (report[s][f], v) for f, v in e.items() if report[s][f] != v}
                                                                           for s, e in expected_report(W, H, n, stages=hvo.STAGE_ALL).items()}
        check_primary(n, res, reference, culled=False)
    finally:
        print(report_line(n, report, times, time.perf_counter() - t0))


@pytest.mark.gpu
def test_small_chunks_without_compact_records(hvo, reference, clean_env):
    """HVO_LSD_CHUNK below the batch size with one record per pixel (the suite had it only beside HVO_LSD_COMPACT=1): 17 frames in
    chunks of 5 -- three full chunks and one of two frames, every chunk after the first at an offset into the record image"""
    clean_env.setenv("HVO_LSD_CHUNK", "5")
    n = 17
    report, res, times = run_case(hvo, reference, n, hvo.STAGE_ALL)
    want = expected_report(W, H, n, stages=hvo.STAGE_ALL)
    want["lsd"].update(chunk=5, chunks=4)
    assert report == want, report["lsd"]
    check_primary(n, res, reference, culled=False)


def culled_reference(orc, reference, f):
    """Frame::cullingLine + the second LBD pass on the oracle's lines of distinct frame f (computed once)"""
    c = reference["culled"]
    if f not in c:
        o = reference["ref"][f]
        c[f] = orc.cull_lines(reference["gray"][f], o["kl"], o["linefn"])
    return c[f]


def check_tail(r, d, orc, seed, okw, full):
    """test_tail_gpu.check_tail's rules, unchanged, with this geometry's camera handed to the oracle.  full: the oracle scores all 37 800
    hypotheses (12 ms a frame); otherwise the hypothesis the device chose is formed again by the oracle and must give the device's
    vanishing points and line classes (0.1 ms a frame) -- that the choice has the best score is then not checked for this frame"""
    kl = r["kl"]
    o3 = orc.lines_3d(kl, d, seed=seed, **okw)
    assert r["lines3d"].tobytes() == o3.tobytes(), [f for f in o3.dtype.names if not np.array_equal(r["lines3d"][f], o3[f])]
    vg = r["vp"]
    assert r["tail_status"] == 0
    if not full:
        if vg["n_hypotheses"] == 0:
            assert (vg["vp_idx"] == 3).all()
        else:
            assert vg["n_hypotheses"] == 37800
            twin = orc.vp_hypothesis(kl, seed, vg["best"], fx=okw["fx"], cx=okw["cx"], cy=okw["cy"])
            assert np.allclose(vg["vps"], twin, atol=1e-12) and np.array_equal(vg["vp_idx"], orc.vp_line2vps(kl, twin, **okw))
        return
    vo = orc.vanishing_points(kl, seed=seed, want_scores=True, **okw)
    if vo is None:
        assert vg["n_hypotheses"] == 0 and (vg["vp_idx"] == 3).all()
    else:
        assert vg["n_hypotheses"] == 37800
        assert abs(vg["score"] - vo["score"]) <= 1e-9 * max(1.0, vo["score"])
        if vg["best"] != vo["best"]:
            assert abs(vo["scores"][vg["best"]] - vo["score"]) <= 1e-9 * max(1.0, vo["score"])
            twin = orc.vp_hypothesis(kl, seed, vg["best"], fx=okw["fx"], cx=okw["cx"], cy=okw["cy"])
            assert np.allclose(vg["vps"], twin, atol=1e-12) and np.array_equal(vg["vp_idx"], orc.vp_line2vps(kl, twin, **okw))
        else:
            assert np.allclose(vg["vps"], vo["vps"], atol=1e-12) and np.array_equal(vg["vp_idx"], vo["vp_idx"])


def check_tail_seed_free(r, d, orc, okw):
    po, co = orc.plane_clouds(d, r["labels"].astype(np.int32), r["planes"], dist_th=0.05, **okw)
    pg, cg = r["plane_clouds"], r["cloud_xyz"]
    assert len(pg) == len(po)
    for f in ("valid", "gate_ok", "first", "n_points", "n_pixels"):
        assert np.array_equal(pg[f], po[f]), f
    assert np.array_equal(cg, co)
    assert np.allclose(pg["coef"], po["coef"], rtol=0, atol=1e-5)
    so = orc.surface_normals(d, **okw)
    assert r["normals"].tobytes() == so.tobytes()
    bounds = (0.0, float(W), 0.0, float(H))
    ps, pi = orc.assign_features_to_grid(r["kp"], bounds)
    assert np.array_equal(r["pt_grid"][0], ps) and np.array_equal(r["pt_grid"][1], pi)
    ls, li, ln = orc.assign_lines_to_grid(r["kl"], bounds)
    assert np.array_equal(r["ln_grid"][0], ls) and np.array_equal(r["ln_grid"][1], li)


@pytest.mark.gpu
@pytest.mark.parametrize("n", TAIL_SIZES)
def test_whole_frame_constructor_at_a_plan_boundary(hvo, orc, reference, clean_env, n):
    """STAGE_FRAME = every stage with Frame::cullingLine and the tail: the culling loop and the tail kernels walk the batch in the chunks of
    the line stage.  Culled lines: the oracle's culling of the oracle's lines, with the rules of test_lsd_gpu.test_culling_with_a_large_line_quota."""
    t0 = time.perf_counter()
    report, res, times = run_case(hvo, reference, n, hvo.STAGE_FRAME)
    try:
        assert report == expected_report(W, H, n, stages=hvo.STAGE_FRAME, cull=True)
        check_primary(n, res, reference, culled=True)
        for f in range(NDISTINCT):
            r = res[f]
            klc, ldc, fnc = culled_reference(orc, reference, f)
            assert len(r["kl"]) == len(klc) and np.array_equal(r["ldesc"], ldc), where(n, f)
            for k in ("sx", "sy", "ex", "ey"):
                assert np.array_equal(r["kl"][k], klc[k]), (k, where(n, f))
            try:
                check_tail_seed_free(r, reference["depth"][f], orc, reference["okw"])
            except AssertionError as e:
                raise AssertionError("tail against the oracle, %s: %s" % (where(n, f), e))
        # the seeded stages: every frame against the oracle at its own seed (the key lines of frame f are those of f % 16, byte for byte, by
        # now).  All hypotheses are scored for every frame of the small case; in the large one for the first occurrences and for the
        # sixteen frames on either side of the chunk boundary, where a chunk offset would show
        for f in range(n):
            full = n <= 65 or f < NDISTINCT or abs(f - 512 + 0.5) < NDISTINCT
            try:
                check_tail(res[f], reference["depth"][f % NDISTINCT], orc, TAIL_SEED + f, reference["okw"], full)
                assert res[f]["vp"]["n_hypotheses"] == res[f % NDISTINCT]["vp"]["n_hypotheses"]
            except AssertionError as e:
                raise AssertionError("seeded tail against the oracle, %s: %s" % (where(n, f), e))
        # the seed-free tail arrays: every later occurrence against the first
        for f in range(NDISTINCT, n):
            a, b = res[f], res[f % NDISTINCT]
            for k in ("plane_clouds", "cloud_xyz", "normals"):
                assert a[k].tobytes() == b[k].tobytes(), "%s: %s differs from its first occurrence" % (k, where(n, f))
            for k in ("pt_grid", "ln_grid"):
                assert a[k][0].tobytes() == b[k][0].tobytes() and a[k][1].tobytes() == b[k][1].tobytes(), "%s: %s differs from its first occurrence" % (k, where(n, f))
    finally:
        print(report_line(n, report, times, time.perf_counter() - t0))
