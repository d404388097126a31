"""GPU tests of the line structural constraints and LineOptStruct (csrc/line_opt.hip) against tests/line_opt_ref.py, and of the three
forms against each other.

Measured on an MI355X (profiles/r10_line_opt.txt): D = 7.98e-5 m, 8 D = 6.39e-4 m, largest end-point difference 7.27e-5 m; median turn of
the optimised lines 2.44e-2 rad against 1.67e-3 rad for the angular equivalent of 8 D; 6 / 6 natural and 6 / 8 corrupted scenes accepted."""
import numpy as np
import pytest

import line_opt_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def natural():
    return ref.accepted_scenes(6, seed0=2000)


@pytest.fixture(scope="module")
def corrupted():
    return ref.accepted_scenes(6, seed0=3000, corrupt=0.01)


def prob(hvo, S, with_rel=False):
    d = dict(linefn=S["linefn"], lines3d=ref.to_records(S, hvo.LINE3D_DT))
    if with_rel: d["rel"] = S["rel"]
    return d


def test_part1_equals_restatement_on_every_scene(hvo, gpu_ctx):
    scenes = [ref.make_scene(s) for s in range(2000, 2008)] + [ref.make_scene(2100, n_lines=333, invalid=0.3), ref.make_scene(2101, n_lines=7)]
    for rule in (hvo.LINE_STRUCT_ROW_UNSET, hvo.LINE_STRUCT_ROW_Z0):
        out = gpu_ctx.line_struct_optimize([prob(hvo, S) for S in scenes], mode=hvo.LINE_STRUCT_CONSTRAINTS, row_rule=rule)
        for S, r in zip(scenes, out):
            want = ref.struct_constraints(S["linefn"], S["line_eq"], ref.default_params(row_rule=rule))
            assert r.rounds == 0 and r.n_lines == len(want)
            assert np.array_equal(r.rel, want), (S["seed"], rule, int((r.rel != want).sum()))
            assert np.array_equal(r.lines, np.concatenate([S["A"], S["B"]], axis=1))
        print("row rule %d: %d scenes, %d pairs equal, %d parallel %d perpendicular entries" % (
            rule, len(scenes), sum(r.rel.size for r in out), sum(int((r.rel == 1).sum()) for r in out), sum(int((r.rel == 2).sum()) for r in out)))


def _same_counts(r, R):
    assert np.array_equal(r.rel, R.rel), int((r.rel != R.rel).sum())
    got = (r.n_lines_to_opt, r.n_edges, r.n_par_edges, r.n_perp_edges, r.rounds, r.written_back, list(r.n_flagged))
    assert got == (R.n_lines_to_opt, R.n_edges, R.n_par_edges, R.n_perp_edges, R.rounds, R.written_back, list(R.n_flagged)), got


def test_part2_against_restatement(hvo, gpu_ctx, natural, corrupted):
    (nat, g1), (cor, g2) = natural, corrupted
    print("scenes generated / accepted: natural %d / %d, corrupted lists %d / %d" % (g1, len(nat), g2, len(cor)))
    assert 2 * len(nat) >= g1 and 2 * len(cor) >= g2
    D = ref.measured_D(nat + cor)
    out = gpu_ctx.line_struct_optimize([prob(hvo, S) for S, _ in nat]) + \
        gpu_ctx.line_struct_optimize([prob(hvo, S, True) for S, _ in cor], mode=hvo.LINE_STRUCT_OPTIMIZE)
    worst, turn, equiv = 0.0, [], []
    for (S, R), r in zip(nat + cor, out):
        _same_counts(r, R)
        worst = max(worst, float(np.abs(r.lines - R.lines).max()))
        if R.written_back:
            init = np.concatenate([S["A"], S["B"]], axis=1); e = R.graph.entered
            d0, d1 = ref.directions(init[e]), ref.directions(r.lines[e])
            turn += np.arccos(np.clip((d0 * d1).sum(axis=1), -1, 1)).tolist()
            equiv += (2 * 8 * D / np.linalg.norm(init[e, 3:] - init[e, :3], axis=1)).tolist()    # both end points off by 8 D, against each other
    print("D = %.3e, 8 D = %.3e, largest end-point difference %.3e; median turn %.3e rad, median angular equivalent of 8 D %.3e rad" % (
        D, 8 * D, worst, np.median(turn), np.median(equiv)))
    print("iterations / trials per round, device:", [(list(r.iterations), list(r.trials)) for r in out])
    assert worst <= 8 * D
    assert np.median(turn) >= 10 * np.median(equiv)          # the bound is not vacuous: the optimisation turns the lines far more than 8 D could
    assert sum(r.n_flagged[0] for r in out) > 50 and {r.written_back for r in out} == {0, 1}
    assert any(r.trials[0] > r.iterations[0] for r in out)   # rejected Levenberg trials occur


def test_same_bytes_twice_and_batch_equals_singles(hvo, gpu_ctx, natural, corrupted):
    P = [prob(hvo, S, True) for S, _ in natural[0][:3] + corrupted[0][:3]]
    a = gpu_ctx.line_struct_optimize(P); b = gpu_ctx.line_struct_optimize(P)
    for x, y in zip(a, b):
        assert bytes(x) == bytes(y) and np.array_equal(x.rel, y.rel) and np.array_equal(x.lines, y.lines)
    for i in (0, 4):
        s = gpu_ctx.line_struct_optimize(P[i])
        assert bytes(s) == bytes(a[i]) and np.array_equal(s.rel, a[i].rel) and np.array_equal(s.lines, a[i].lines)
    # part 2 alone on part 1's own output = both parts in one call
    r1 = gpu_ctx.line_struct_optimize(P[0], mode=hvo.LINE_STRUCT_CONSTRAINTS)
    r2 = gpu_ctx.line_struct_optimize(dict(P[0], rel=r1.rel), mode=hvo.LINE_STRUCT_OPTIMIZE)
    assert np.array_equal(r2.rel, a[0].rel) and np.array_equal(r2.lines, a[0].lines)
    print("kernel ms (pair pass, optimisation) of the last call: %.3f %.3f" % gpu_ctx.line_opt_last_kernel_ms())


def test_known_answers_on_the_device(hvo, gpu_ctx):
    X, Y, Z = np.eye(3)
    pp = lambda c: np.array([c, np.sqrt(1 - c * c), 0.0])
    S = ref.crafted([X] + [pp(c) for c in [0.05] * 8 + [0.12, 0.15]], [(0, i, 2) for i in range(1, 11)])
    r = gpu_ctx.line_struct_optimize(prob(hvo, S, True), mode=hvo.LINE_STRUCT_OPTIMIZE, params=dict(iterations=0))
    assert list(r.n_flagged) == [1, 2] and r.rel[0].tolist() == [0] + [2] * 9 + [-2] and r.rounds == 2 and list(r.iterations) == [0, 0]
    assert np.array_equal(r.lines, np.concatenate([S["A"], S["B"]], axis=1))
    d0 = np.array([1.0, 1.0, 0.8]); d0 /= np.linalg.norm(d0)
    S = ref.crafted([d0] + [Y] * 5 + [Z] * 5, [(0, i, 1) for i in range(1, 11)])
    r = gpu_ctx.line_struct_optimize(prob(hvo, S, True), mode=hvo.LINE_STRUCT_OPTIMIZE)
    assert list(r.n_flagged) == [10, 10] and r.iterations[1] == 0 and r.trials[1] == 0 and r.rel[0, 1:].tolist() == [-1] * 10
    S = ref.crafted([X] * 10, [(0, i, 1) for i in range(1, 10)])
    assert gpu_ctx.line_struct_optimize(prob(hvo, S, True), mode=hvo.LINE_STRUCT_OPTIMIZE).rounds == 1
    # the vertex(0) quirk both ways
    for line0 in (True, False):
        S = ref.crafted_families(line0=line0); R = ref.run_scene(S)
        r = gpu_ctx.line_struct_optimize(prob(hvo, S, True), mode=hvo.LINE_STRUCT_OPTIMIZE)
        init = np.concatenate([S["A"], S["B"]], axis=1)
        assert r.written_back == int(line0) == R.written_back and r.n_lines_to_opt == R.n_lines_to_opt
        assert np.array_equal(r.lines, init) != line0
        assert np.abs(r.lines - R.lines).max() < 1e-3
    # a slot that holds -1 on entry counts for the size, gives no edge and stays
    S = ref.crafted([X] * 6, [(0, i, 1) for i in range(1, 6)]); S["rel"][0, 5] = -1
    r = gpu_ctx.line_struct_optimize(prob(hvo, S, True), mode=hvo.LINE_STRUCT_OPTIMIZE)
    assert r.n_lines_to_opt == 1 and r.n_edges == 4 and r.rel[0, 5] == -1


def test_refusals_and_empty_frames(hvo, gpu_ctx, synth):
    l3 = np.zeros(0, hvo.LINE3D_DT)
    r = gpu_ctx.line_struct_optimize(dict(linefn=np.zeros((0, 3)), lines3d=l3))                # an empty frame
    assert r.n_lines == 0 and r.n_edges == 0 and r.written_back == 0 and r.rounds == 1 and r.status == 0
    S = ref.crafted([np.eye(3)[0]] * 6, [(k, i, 1) for k in range(6) for i in range(6) if i != k and i < 4])   # at most four entries per row
    r = gpu_ctx.line_struct_optimize(prob(hvo, S, True), mode=hvo.LINE_STRUCT_OPTIMIZE)
    assert r.n_lines_to_opt == 0 and r.n_edges == 0 and r.written_back == 0 and np.array_equal(r.lines, np.concatenate([S["A"], S["B"]], axis=1))
    assert np.array_equal(r.rel, S["rel"])
    big = np.zeros(4097, hvo.LINE3D_DT)
    with pytest.raises(hvo.HvoError) as e:                                                    # more than 4096 lines
        gpu_ctx.line_struct_optimize(dict(linefn=np.ones((4097, 3)), lines3d=big), mode=hvo.LINE_STRUCT_CONSTRAINTS)
    assert e.value.status == -4
    with pytest.raises(hvo.HvoError):                                                         # part 1 without line functions: NULL where not allowed
        gpu_ctx.line_struct_optimize(dict(lines3d=ref.to_records(S, hvo.LINE3D_DT)))
    with pytest.raises(hvo.HvoError):                                                         # a rel value outside -2 .. 2
        gpu_ctx.line_struct_optimize(dict(lines3d=ref.to_records(S, hvo.LINE3D_DT), rel=np.full((6, 6), 3, np.int8)), mode=hvo.LINE_STRUCT_OPTIMIZE)
    with pytest.raises(hvo.HvoError):
        gpu_ctx.line_struct_optimize(prob(hvo, S, True), mode=0)                             # neither part
    g, d = synth.make_frame("std", 0x5EED0002)
    s = hvo.Stream(640, 480, depth=2, stages=hvo.STAGE_ORB | hvo.STAGE_LSD)                   # missing HVO_STAGE_LINES3D
    try:
        with pytest.raises(hvo.HvoError):
            s.line_struct_optimize(s.submit(g), 0)
    finally:
        s.close()
    c = hvo.Context(max_batch=2)
    try:
        gg, dd = synth.make_batch("std", 0x5EED0002, 2)
        c.batch_upload(gg, dd); c.batch_run(hvo.STAGE_ALL)                                    # no tail stages
        with pytest.raises(hvo.HvoError):
            c.batch_line_struct_optimize([0])
        c.batch_run(hvo.STAGE_FRAME)
        with pytest.raises(hvo.HvoError):                                                     # n beyond the batch
            c.batch_line_struct_optimize([0, 0, 0])
        assert len(c.batch_line_struct_optimize([0, 0])) == 2
        with pytest.raises(hvo.HvoError):                                                     # a second optimising call on the same resident lines
            c.batch_line_struct_optimize([0, 0])
        assert len(c.batch_line_struct_optimize([0, 0], mode=hvo.LINE_STRUCT_CONSTRAINTS)) == 2     # constraints alone may be asked again
    finally:
        c.close()


def test_stream_batch_host_forms_and_the_chain(hvo, synth):
    """the stream form equals the host form on the downloaded records; frame k of a batch equals the stream form; after the call the resident
    frame's pose optimisation equals hvo_pose_optimize on host arrays carrying the optimised A, B, and differs from the un-optimised one"""
    import pose_opt_ref as pref
    s = hvo.Stream(640, 480, depth=2, stages=hvo.STAGE_FRAME, bf=40.0)
    ctx = hvo.Context(); bc = hvo.Context(max_batch=3)
    try:
        # the first frame for which the restatement, on the downloaded records, says that the end points are written back and turn
        for k in range(8):
            g, d = synth.make_frame("std", 0x5EED0002 + k)
            t = s.submit(g, d); out = s.collect(t)
            l3d, linefn = out["lines3d"], out["linefn"]; nl = len(linefn)
            R = ref.run_both(linefn, l3d["A"], l3d["B"], l3d["line_eq"])
            init = np.concatenate([l3d["A"], l3d["B"]], axis=1)
            print("frame %d: %d lines, %d to optimise, %d edges, written back %d, largest move %.3e" % (
                k, nl, R.n_lines_to_opt, R.n_edges, R.written_back, np.abs(R.lines - init).max()))
            if R.written_back and np.abs(R.lines - init).max() > 1e-3 and ref.accepted(R): break
        else:
            pytest.fail("no synthetic frame whose line 0 enters the graph")
        assert nl > 20
        # the chain's pose problem: every good line matched to a map line at its own (un-optimised) position, moved a little
        Tcw = np.concatenate([pref.rot_vec([0.01, -0.02, 0.015]), [[0.02], [-0.01], [0.03]]], axis=1).astype(np.float32)
        R_, t_ = Tcw[:, :3].astype(np.float64), Tcw[:, 3].astype(np.float64)
        r0 = np.random.RandomState(5)
        ln_has = (l3d["good"] != 0).astype(np.uint8)
        ln_xyz = np.concatenate([(l3d["A"] - t_) @ R_, (l3d["B"] - t_) @ R_], axis=1) + r0.normal(0, 0.004, (nl, 6))
        ms = dict(ln_has=ln_has, ln_xyz=ln_xyz)
        # three line-only correspondences do not reach nInitialCorrespondences >= 3 (points and planes count): add points
        kp_un = out["kp_un"]; n = len(kp_un); fx, fy, cx, cy, bf = pref.CAM
        z = np.where(out["zdepth"] > 0, out["zdepth"], 2.0).astype(np.float64)
        Xc = np.stack([(kp_un["x"] - cx) / fx * z, (kp_un["y"] - cy) / fy * z, z], axis=1)
        ms.update(pt_has=(r0.uniform(size=n) < 0.3).astype(np.uint8), pt_xyz=((Xc - t_) @ R_ + r0.normal(0, 0.004, Xc.shape)).astype(np.float32))
        before = s.pose_optimize(t, pref.CAM, Tcw, (n, nl, 0), **ms)
        rs = s.line_struct_optimize(t, nl)
        rh = ctx.line_struct_optimize(dict(linefn=linefn, lines3d=l3d))
        assert bytes(rs) == bytes(rh) and np.array_equal(rs.rel, rh.rel) and np.array_equal(rs.lines, rh.lines)
        assert rs.written_back == 1 and rs.n_lines == nl
        _same_counts(rs, R)
        print("stream form: %d lines, %d to optimise, %d edges, its %s trials %s; kernel ms %.3f %.3f" % (
            nl, rs.n_lines_to_opt, rs.n_edges, list(rs.iterations), list(rs.trials), *s.line_opt_last_kernel_ms(t)))
        with pytest.raises(hvo.HvoError):                                                     # a second call would optimise optimised lines
            s.line_struct_optimize(t, nl)
        with pytest.raises(hvo.HvoError):
            s.line_struct_optimize(t + 5, nl)                                                 # no such frame
        after = s.pose_optimize(t, pref.CAM, Tcw, (n, nl, 0), **ms)
        l3o = l3d.copy(); l3o["A"] = rs.lines[:, :3]; l3o["B"] = rs.lines[:, 3:]
        host = lambda rec: ctx.pose_optimize(pref.CAM, dict(Tcw=Tcw, kp_un=kp_un, uright=out["uright"], linefn=linefn, lines3d=rec,
                                                            plane_coef=np.zeros((0, 4), np.float32), **ms))
        h_after, h_before = host(l3o), host(l3d)
        assert bytes(after) == bytes(h_after) and bytes(before) == bytes(h_before)
        assert bytes(after) != bytes(before) and not np.array_equal(np.array(after.Tcw_d), np.array(before.Tcw_d))
        print("chain: pose translation moved by %.3e through the optimised lines" % np.abs(np.array(after.Tcw_d) - np.array(before.Tcw_d)).max())
        # the resident batch: frame 1 = the stream's frame (the batch's 3-D line seeds run seed + f, the stream's ticket + 1)
        g2, d2 = synth.make_frame("std", 0x5EED0001)
        bc.set_tail_params(seed=t)
        bc.batch_upload(np.stack([g2, g, g2]), np.stack([d2, d, d2])); bc.batch_run(hvo.STAGE_FRAME)
        rb = bc.batch_line_struct_optimize([0, nl, 0])
        assert bytes(rb[1]) == bytes(rs) and np.array_equal(rb[1].rel, rs.rel) and np.array_equal(rb[1].lines, rs.lines)
        assert rb[0].n_lines == 0 and rb[2].n_lines == 0
    finally:
        s.close(); ctx.close(); bc.close()
