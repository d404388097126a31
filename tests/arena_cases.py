"""One entry per entry point that stages through the context's call arena (hvo_call_arena, csrc/arena.hip) or through a slot map's call
scratch (hvo_slot_map::d_a / d_b, csrc/slot_map.hpp).  tests/test_call_arena.py counts the call sites in csrc/*.hip against the sites the
cases claim and asserts on the CPU that no input is vacuous; tests/test_call_arena_gpu.py runs every case on a dirty arena, on its own
leftovers, on the other cases' leftovers and across a regrowth.

A case has
    sites      the call sites it reaches, as (file, tag): the census compares the distinct tags per file with the calls the file holds
    build      (env, "S" | "L") -> the inputs, plain host arrays: S small, L larger (more arena, or more scratch for the two map calls)
    open       (env, inputs) -> the device objects the call needs beside the context (a vocabulary, a map), or None; .close() each
    run        (env, ctx, inputs, objs) -> anything made of dicts, lists, tuples, arrays, ctypes structures and numbers
    want       (env, inputs) -> the restatement's answer, or None where none is importable
    check      (env, got, want) -> asserts, with the comparison of the module's own GPU test
    vacuous    (env, inputs, want) -> asserts that the input reaches what it is meant to reach (on the restatement's answer, on the CPU)
    arena      (env, inputs) -> the bytes the call asks the arena for, where the layout is a line of arithmetic; else None
env is the namespace of the three loaders (hvo, orc, synth)."""
import ctypes
import types

import numpy as np

import bow_ref
import fuse_ref
import kf_search_ref
import line_fuse_ref
import line_map_ref
import line_opt_ref
import manhattan_ref
import map_refresh_ref
import new_lines_ref
import new_points_ref
import pnp_ref
import point_map_ref as pm
import pose_opt_ref

F32 = np.float32
B4 = pm.BOUNDS
TUM1_DIST = [0.262383, -0.953104, -0.005358, 0.002628, 1.163314]      # Examples/RGB-D/TUM1.yaml: a distortion that is not zero reaches the kernel
K0 = (535.4, 539.2, 320.1, 247.6)                                      # the context's default camera (TUM3.yaml)
SIZES = {"S": (247, 322), "L": (480, 640)}                             # h, w of the depth calls


def env():
    from conftest import load_oracle, load_pkg, load_synth
    e = types.SimpleNamespace(hvo=load_pkg(), orc=load_oracle(), synth=load_synth())
    e.orc.lib()
    return e


def al(v, a=256):
    return (v + a - 1) // a * a


def arena_capacity(request):
    """the capacity hvo_call_arena allocates when `request` bytes exceed what it holds"""
    return (request + (request >> 2) + 4095) & ~4095


# ---------------------------------------------------------------------------------------------------------------- comparing results
SKIP_KEYS = ("kernel_ms", "raw")


def flatten(x, prefix="", out=None):
    """every array, number and ctypes structure of a result under a path name -> {path: ndarray}; timings and the binding's raw views are left out"""
    out = {} if out is None else out
    if isinstance(x, dict):
        for k in sorted(x):
            if k not in SKIP_KEYS: flatten(x[k], prefix + "/" + str(k), out)
    elif isinstance(x, (list, tuple)):
        for i, v in enumerate(x): flatten(v, prefix + "/%d" % i, out)
    elif isinstance(x, ctypes.Structure):
        for name, _ in x._fields_:
            if name in SKIP_KEYS: continue
            v = getattr(x, name)
            out[prefix + "." + name] = np.array(v[:] if hasattr(v, "__len__") else v)
        for name in ("rel", "lines", "pt_outlier", "ln_outlier", "pl_outlier", "vp_outlier", "held", "in_view_slot", "proj", "view_cos", "level", "match_idx",
                     "match_dist", "n_par", "n_perp", "rel_map"):
            if name in x.__dict__ and x.__dict__[name] is not None: out[prefix + "." + name] = np.asarray(x.__dict__[name])
    elif x is None:
        out[prefix] = np.zeros(0, np.uint8)
    else:
        out[prefix] = np.asarray(x)
    return out


def identical(a, b, what=""):
    """byte identity of two results of the same call"""
    fa, fb = flatten(a), flatten(b)
    assert sorted(fa) == sorted(fb), (what, sorted(set(fa) ^ set(fb)))
    for k in fa:
        assert fa[k].dtype == fb[k].dtype and fa[k].shape == fb[k].shape and fa[k].tobytes() == fb[k].tobytes(), (what, k)


def same_bits(a, b):
    """floats by their bits, a NaN by being one"""
    a = np.asarray(a); b = np.asarray(b, a.dtype)
    n = np.isnan(b)
    return a.shape == b.shape and np.array_equal(np.isnan(a), n) and a[~n].tobytes() == b[~n].tobytes()


# ---------------------------------------------------------------------------------------------------------------- input pieces
def plane_depth(n, d, w, h, K=K0, units=5000.0):
    """u16 depth image of the plane n . X = d seen through K"""
    j = np.arange(w)[None, :]; i = np.arange(h)[:, None]
    z = d / (n[0] * (j - K[2]) / K[0] + n[1] * (i - K[3]) / K[1] + n[2])
    return np.clip(np.rint(z * units), 0, 65535).astype(np.uint16)


def plane_record(orc, n, d):
    r = np.zeros(1, orc.PLANE_DT)
    nn = np.asarray(n, np.float64); s = np.linalg.norm(nn); nn = nn / s
    r["center"][0] = nn * (d / s); r["normal"][0] = nn
    return r


def keylines(orc, w, h, n, seed):
    """random key lines inside and around the image, none shorter than 12 pixels, with the fields the searches read"""
    rng = np.random.default_rng(seed)
    kl = np.zeros(n, orc.KEYLINE_DT)
    ext = 200.0 * min(w, h) / 480.0
    kl["sx"] = rng.uniform(-10, w + 10, n); kl["sy"] = rng.uniform(-10, h + 10, n)
    a = rng.uniform(0, 2 * np.pi, n); r = rng.uniform(12.0, ext, n)
    kl["ex"] = kl["sx"] + (r * np.cos(a)).astype(F32); kl["ey"] = kl["sy"] + (r * np.sin(a)).astype(F32)
    kl["sox"], kl["soy"], kl["eox"], kl["eoy"] = kl["sx"], kl["sy"], kl["ex"], kl["ey"]
    kl["pt_x"] = (kl["sx"] + kl["ex"]) / 2; kl["pt_y"] = (kl["sy"] + kl["ey"]) / 2
    kl["angle"] = np.arctan2(kl["ey"] - kl["sy"], kl["ex"] - kl["sx"]); kl["length"] = np.hypot(kl["ex"] - kl["sx"], kl["ey"] - kl["sy"])
    kl["class_id"] = np.arange(n); kl["num_pixels"] = kl["length"].astype(np.int32); kl["response"] = kl["length"] / max(w, h); kl["size"] = 1
    return kl


def inside(kl, w, h, m=8):
    return kl[(kl["sx"] > m) & (kl["sx"] < w - m) & (kl["ex"] > m) & (kl["ex"] < w - m) & (kl["sy"] > m) & (kl["sy"] < h - m) & (kl["ey"] > m) & (kl["ey"] < h - m)]


def line_functions(kl):
    """mvKeyLineFunctions: the line through the end points, (a, b) a unit vector"""
    s = np.stack([kl["sx"], kl["sy"], np.ones(len(kl))], axis=1).astype(np.float64); e = np.stack([kl["ex"], kl["ey"], np.ones(len(kl))], axis=1).astype(np.float64)
    f = np.cross(s, e)
    return f / np.hypot(f[:, 0], f[:, 1])[:, None]


def depth_of(e, size, seed):
    h, w = SIZES[size]
    return e.synth.make_depth(seed, w, h)


class Case:
    def __init__(self, name, sites, build, run, want=None, check=None, vacuous=None, arena=None, open=None, uses_map=False):
        self.name, self.sites, self.build, self.run, self.want, self.check = name, tuple(sites), build, run, want, check
        self.vacuous, self.arena, self.open, self.uses_map = vacuous, arena, open, uses_map


CASES = []


def case(**kw):
    CASES.append(Case(**kw))


# ---------------------------------------------------------------------------------------------------------------- the depth calls
def _l3_build(e, size):
    h, w = SIZES[size]
    return dict(depth=depth_of(e, size, 0x5EED5101), kl=keylines(e.orc, w, h, 64 if size == "S" else 200, 51))


def _l3_vac(e, i, w):
    assert 5 < w["good"].sum() < len(i["kl"])


case(name="lines_3d", sites=[("line3d.hip", "hvo_lines_3d")], build=_l3_build,
     run=lambda e, c, i, o: c.lines_3d(i["kl"], i["depth"], seed=7), want=lambda e, i: e.orc.lines_3d(i["kl"], i["depth"], seed=7),
     check=lambda e, g, w: _bytes_equal(g, w), vacuous=_l3_vac,
     arena=lambda e, i: al(len(i["kl"]) * 68) + al(i["depth"].size * 2) + len(i["kl"]) * 104)


def _bytes_equal(g, w):
    assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), [f for f in w.dtype.names if not np.array_equal(g[f], w[f], equal_nan=True)]


def _vp_build(e, size):
    h, w = SIZES[size]
    return dict(kl=inside(keylines(e.orc, w, h, 120 if size == "S" else 260, 52), w, h))


def _vp_check(e, g, w):
    """the sums follow the reference's order but sin and acos are the device's (tests/test_tail_gpu.py compares the score at 1e-9): what is exact
    is the hypothesis count and, where the same hypothesis won, the structure-line labels"""
    assert g["n_hypotheses"] == 37800
    if g["best"] == w["best"]: assert np.array_equal(g["vp_idx"], w["vp_idx"])


def _vp_vac(e, i, w):
    assert w is not None and w["score"] > 0 and (w["vp_idx"] < 3).sum() >= 3 and (w["vp_idx"] == 3).any() and len(i["kl"]) >= 40


case(name="vanishing_points", sites=[("vps.hip", "hvo_vanishing_points")], build=_vp_build,
     run=lambda e, c, i, o: c.vanishing_points(i["kl"], seed=9, want_grid=True), want=lambda e, i: e.orc.vanishing_points(i["kl"], seed=9),
     check=_vp_check, vacuous=_vp_vac)


def _pc_build(e, size):
    """left half a slanted plane (label 0), right half another (label 1), a strip without a label between them"""
    h, w = SIZES[size]
    na, da, nb, db = (0.1, 0.2, 1.0), 2.0, (-0.3, 0.1, 1.0), 2.5
    d = plane_depth(na, da, w, h); d[:, w // 2:] = plane_depth(nb, db, w, h)[:, w // 2:]
    lab = np.zeros((h, w), np.int32); lab[:, w // 2:] = 1; lab[:, w // 2 - 3: w // 2 + 3] = -1
    return dict(depth=d, labels=lab, planes=np.concatenate([plane_record(e.orc, na, da), plane_record(e.orc, nb, db)]))


def _pc_check(e, g, w):
    (pg, cg), (po, co) = g, w
    for f in ("valid", "gate_ok", "first", "n_points", "n_pixels"):
        assert np.array_equal(pg[f], po[f]), f
    assert np.array_equal(cg, co)                                     # the voxel centroids bit for bit (the refit goes through float libm: not compared here)


def _pc_vac(e, i, w):
    po, co = w
    assert po["valid"].tolist() == [1, 1] and len(co) > 100 and po["first"][1] == po["n_points"][0]


case(name="plane_clouds", sites=[("planes_tail.hip", "hvo_plane_clouds")], build=_pc_build,
     run=lambda e, c, i, o: c.plane_clouds(i["depth"], i["labels"], i["planes"]), want=lambda e, i: e.orc.plane_clouds(i["depth"], i["labels"], i["planes"], dist_th=0.05),
     check=_pc_check, vacuous=_pc_vac)


def _lpvo_check(e, g, w):
    assert len(g[0]) == len(w[0])
    for a, b in zip(g, w): assert a.tobytes() == b.tobytes()


def _lpvo_arena(e, i):
    h, w = i["depth"].shape; N = w * h
    full = ((h - 1 - 10 + 14) // 15) * ((w - 1 - 10 + 14) // 15)
    return al(N * 2) + al(full * 24) + al(full * 4) + al(full * 8) + 256 + al(N * 4) + al(7 * N * 4) + al(7 * N * 8) + 256


def _lpvo_vac(e, i, w):
    assert len(w[0]) > 100


case(name="normals_lpvo", sites=[("lpvo.hip", "hvo_normals_lpvo")], build=lambda e, s: dict(depth=depth_of(e, s, 0x5EED5102)),
     run=lambda e, c, i, o: c.normals_lpvo(i["depth"]), want=lambda e, i: e.orc.normals_lpvo(i["depth"]), check=_lpvo_check, vacuous=_lpvo_vac, arena=_lpvo_arena)


def _sn_vac(e, i, w):
    fin = np.isfinite(w["normal"][:, 0])
    assert fin.sum() > 200 and (~fin).sum() > 200


case(name="surface_normals", sites=[("planes_tail.hip", "hvo_surface_normals")], build=lambda e, s: dict(depth=depth_of(e, s, 0x5EED5103)),
     run=lambda e, c, i, o: c.surface_normals(i["depth"]), want=lambda e, i: e.orc.surface_normals(i["depth"]),
     check=lambda e, g, w: _bytes_equal(g, w), vacuous=_sn_vac)


# ---------------------------------------------------------------------------------------------------------------- Manhattan tracking
def _mf_build(e, size):
    n, Rt = manhattan_ref.three_families(seed=8, n=100 if size == "S" else 900)
    rng = np.random.RandomState(11)
    l3d = manhattan_ref.lines_along(rng, np.concatenate([manhattan_ref.family(rng, Rt[:, c], 7 if size == "S" else 40, 2.0) for c in range(3)]))
    R = (manhattan_ref.rot((1.0, 1.0, 0.0), 5.0) @ Rt).astype(F32)
    return dict(normals=np.asarray(n, F32).reshape(-1, 3), l3d=l3d, R=R)


def _mf_check(e, g, w):
    res, na, la = g
    r = res.to_dict()
    for k in ("found", "n_found", "n_in_cone", "n_selected", "min_num_sn", "tracked"):
        assert np.array_equal(r[k], w[k]), (k, r[k], w[k])
    assert r["status"] == 0 and np.array_equal(na, w["normal_axes"]) and np.array_equal(la, w["line_axes"])


def _mf_vac(e, i, w):
    assert w["n_found"] == 3 and w["tracked"] and w["line_axes"].any() and w["normal_axes"].any()


case(name="track_manhattan", sites=[("api.hip", "hvo_track_manhattan")], build=_mf_build,
     run=lambda e, c, i, o: c.track_manhattan(i["normals"], i["l3d"], i["R"], axes=True),
     want=lambda e, i: manhattan_ref.track_manhattan(i["normals"], i["l3d"], i["R"]), check=_mf_check, vacuous=_mf_vac,
     arena=lambda e, i: al(len(i["normals"]) * 32) + al(len(i["l3d"]) * 104) + al(ctypes.sizeof(e.hvo.MfResult)) + al(len(i["normals"])) + al(len(i["l3d"])))


def _bmf_build(e, size):
    n = 1 if size == "S" else 3
    g, d = e.synth.make_batch("std", 0x5EED5200, 3)
    return dict(gray=g, depth=d, n=n, R0=manhattan_ref.rot((0.2, 1.0, 0.1), 4.0).astype(F32))


def _bmf_run(e, c, i, o):
    """the resident batch is made once per context: three frames through the line, plane and tail stages"""
    hvo = e.hvo
    if not getattr(c, "_arena_batch", False):
        c.set_tail_params(seed=5)
        c.batch_upload(i["gray"], i["depth"])
        c.batch_run(hvo.STAGE_LSD | hvo.STAGE_PLANES | hvo.STAGE_LINES3D | hvo.STAGE_PLANE_TAIL)
        c._arena_batch = True
    return c.batch_track_manhattan(i["R0"], n=i["n"])


case(name="batch_track_manhattan", sites=[("api.hip", "hvo_batch_track_manhattan")], build=_bmf_build, run=_bmf_run,
     arena=lambda e, i: i["n"] * ctypes.sizeof(e.hvo.MfResult))


# ---------------------------------------------------------------------------------------------------------------- frame post-processing
def _kp_build(e, size):
    kp, _ = kf_search_ref.planted_frame(e.hvo.KEYPOINT_DT, seed=53, nt=65 if size == "S" else 1000)
    return dict(kp=kp)


def _un_want(e, i):
    return e.orc.undistort_keypoints(i["kp"], fx=K0[0], fy=K0[1], cx=K0[2], cy=K0[3], dist5=TUM1_DIST)


def _un_vac(e, i, w):
    assert (np.abs(w["x"] - i["kp"]["x"]) > 0.5).sum() > len(i["kp"]) // 4


case(name="undistort_keypoints", sites=[("frame.hip", "frame_undistort")], build=_kp_build,
     run=lambda e, c, i, o: c.undistort_keypoints(i["kp"], TUM1_DIST), want=_un_want, check=lambda e, g, w: _bytes_equal(g, w), vacuous=_un_vac,
     arena=lambda e, i: 2 * al(len(i["kp"]) * 28))


def _grid_check(e, g, w):
    assert np.array_equal(g[0], w[0]) and np.array_equal(g[1], w[1])


def _grid_arena(n, item, per, cap):
    return al(n * item) + al(n * per * 4) + al((64 * 48 + 1) * 4) + al(max(cap, 1) * 4) + 256


case(name="assign_features_to_grid", sites=[("frame.hip", "grid_host")], build=_kp_build,
     run=lambda e, c, i, o: c.assign_features_to_grid(i["kp"], np.array(B4, F32)), want=lambda e, i: e.orc.assign_features_to_grid(i["kp"], np.array(B4, F32)),
     check=_grid_check, vacuous=lambda e, i, w: _true(len(w[1]) > len(i["kp"]) * 0.9 and w[0][-1] == len(w[1])),
     arena=lambda e, i: _grid_arena(len(i["kp"]), 28, 1, len(i["kp"])))


def _true(v):
    assert v


def _lg_build(e, size):
    return dict(kl=keylines(e.orc, 640, 480, 20 if size == "S" else 200, 54))


case(name="assign_lines_to_grid", sites=[("frame.hip", "grid_host")], build=_lg_build,
     run=lambda e, c, i, o: c.assign_lines_to_grid(i["kl"], np.array(B4, F32)), want=lambda e, i: e.orc.assign_lines_to_grid(i["kl"], np.array(B4, F32))[:2],
     check=_grid_check, vacuous=lambda e, i, w: _true(len(w[1]) > 4 * len(i["kl"])),
     arena=lambda e, i: _grid_arena(len(i["kl"]), 68, 128, len(i["kl"]) * 128))


# ---------------------------------------------------------------------------------------------------------------- bag of words
def _voc():
    return bow_ref.make_vocabulary(4, 4, 104)


def _voc_open(e, i):
    v = i["voc"]
    return dict(voc=e.hvo.Vocabulary(v["k"], v["L"], v["parent"], v["is_leaf"], v["desc"], v["weight"], v["scoring"], v["weighting"], device=0))


def _bow_build(e, size):
    voc = _voc(); rng = np.random.RandomState(55)
    n = 65 if size == "S" else 1000
    leaves = voc["desc"][voc["is_leaf"] == 1]
    d = leaves[rng.randint(0, len(leaves), n)].copy(); d[:, rng.randint(0, 32)] ^= rng.randint(0, 256, n).astype(np.uint8)
    return dict(voc=voc, desc=d)


def _bow_check(e, g, w):
    for k in ("word_id", "node_id", "bow_word", "fv_node", "fv_start", "fv_index"):
        assert np.array_equal(g[k], w[k]), k
    assert np.array_equal(g["bow_value"].view(np.uint64), w["bow_value"].view(np.uint64)) and g["n_short"] == w["n_short"]


case(name="compute_bow", sites=[("bow.hip", "hvo_compute_bow")], build=_bow_build, open=_voc_open,
     run=lambda e, c, i, o: c.compute_bow(o["voc"], i["desc"], levelsup=2), want=lambda e, i: bow_ref.transform(i["voc"], i["desc"], 2), check=_bow_check,
     vacuous=lambda e, i, w: _true(8 < len(w["bow_word"]) <= len(i["desc"]) and len(w["fv_node"]) > 4),
     arena=lambda e, i: al(max(len(i["desc"]), 1) * 32) + al(4))


def _sbow_build(e, size):
    kf, fr = bow_ref.random_pair(100, 100, 140, n_nodes=12) if size == "S" else bow_ref.random_pair(1000, 1000, 1040, n_nodes=60)
    return dict(kf=kf, fr=fr)


def _sbow_check(e, g, w):
    assert np.array_equal(g[0][0], w[0]) and g[0][1] == w[1]


case(name="search_by_bow", sites=[("bow.hip", "bow_search")], build=_sbow_build,
     run=lambda e, c, i, o: c.search_by_bow(i["fr"], [i["kf"]]), want=lambda e, i: bow_ref.search_by_bow(i["kf"], i["fr"]), check=_sbow_check,
     vacuous=lambda e, i, w: _true(w[1] > len(i["fr"]["desc"]) // 10))


# ---------------------------------------------------------------------------------------------------------------- the optimisers and the solver
def _ls_build(e, size):
    sc, _ = line_opt_ref.accepted_scenes(1, seed0=2200, n_lines=40) if size == "S" else line_opt_ref.accepted_scenes(1, seed0=2000)
    return dict(S=sc[0][0], R=sc[0][1])


def _ls_run(e, c, i, o):
    S = i["S"]
    return c.line_struct_optimize(dict(linefn=S["linefn"], lines3d=line_opt_ref.to_records(S, e.hvo.LINE3D_DT)))


def _ls_check(e, r, R):
    """the decisions are equal on a scene the generator accepted; the end points agree within a measured bound in tests/test_line_opt_gpu.py, not here"""
    assert np.array_equal(r.rel, R.rel)
    got = (r.n_lines_to_opt, r.n_edges, r.n_par_edges, r.n_perp_edges, r.rounds, r.written_back, list(r.n_flagged))
    assert got == (R.n_lines_to_opt, R.n_edges, R.n_par_edges, R.n_perp_edges, R.rounds, R.written_back, list(R.n_flagged)), got


case(name="line_struct_optimize", sites=[("line_opt.hip", "ls_run")], build=_ls_build, run=_ls_run, want=lambda e, i: i["R"], check=_ls_check,
     vacuous=lambda e, i, w: _true(w.n_edges > 20 and w.n_lines_to_opt > 3 and w.rounds >= 1))


def _po_build(e, size):
    if size == "S":
        sc, _ = pose_opt_ref.accepted_scenes(1, seed0=1100, n_pts=80, n_lines=20, n_planes=3)
    else:
        sc, _ = pose_opt_ref.accepted_scenes(3)
    return dict(P=[s[0] for s in sc], R=[s[1] for s in sc])


def _po_run(e, c, i, o):
    return c.pose_optimize(pose_opt_ref.CAM, [pose_opt_ref.to_binding(P, e.hvo.KEYPOINT_DT, e.hvo.LINE3D_DT) for P in i["P"]])


def _po_check(e, g, w):
    """flags, counts and the return value are equal on accepted scenes; the pose agrees within a measured bound in tests/test_pose_opt_gpu.py, not here"""
    assert len(g) == len(w)
    for r, R in zip(g, w):
        assert (r.ret, r.n_initial, r.n_bad, r.n_line_bad, r.n_edges, r.rounds) == (R.ret, R.n_initial, R.n_bad, R.n_line_bad, R.n_edges, R.rounds)
        assert np.array_equal(r.pt_outlier, R.pt_outlier) and np.array_equal(r.ln_outlier, R.ln_outlier)
        assert np.array_equal(r.vp_outlier, R.vp_outlier) and np.array_equal(r.pl_outlier, R.pl_outlier)


case(name="pose_optimize", sites=[("pose_opt.hip", "po_run")], build=_po_build, run=_po_run, want=lambda e, i: i["R"], check=_po_check,
     vacuous=lambda e, i, w: _true(all(R.ret > 10 and R.rounds == 4 for R in w) and any(R.n_bad > 0 for R in w)))


PNP_P = pnp_ref.default_params(seed=11)


def _pnp_run(e, c, i, o):
    return c.pnp_ransac(pnp_ref.CAM, i["problems"], e.hvo.pnp_params(**PNP_P), want_sample=True, spare_events=2)


def _pnp_check(e, g, w):
    import test_pnp_gpu
    for j in range(len(w)): test_pnp_gpu.same(g[j], w[j], "candidate %d" % j)


case(name="pnp_ransac", sites=[("pnp.hip", "pnp_run")], build=lambda e, s: dict(problems=pnp_ref.multi_problems(1 if s == "S" else 3)), run=_pnp_run,
     want=lambda e, i: [pnp_ref.solve(p, pnp_ref.CAM, PNP_P, j=j) for j, p in enumerate(i["problems"])], check=_pnp_check,
     vacuous=lambda e, i, w: _true(len(w[0]["events"]) >= 1 and w[0]["events"][0]["success"] and w[0]["T"] > 4))


# ---------------------------------------------------------------------------------------------------------------- the searches over map entries
def _kfs_build(e, size):
    nt, n = (65, 64) if size == "S" else (1004, 1000)
    kp, desc = kf_search_ref.planted_frame(e.hvo.KEYPOINT_DT, seed=56, nt=nt)
    return dict(kp=kp, desc=desc, cand=kf_search_ref.planted_candidate(kp, desc, pm.scene_pose(0), seed=56, n=n))


def _kfs_check(e, g, w):
    import test_kf_search_gpu
    test_kf_search_gpu.same(g[0], w)


case(name="search_by_projection_keyframe", sites=[("kf_search.hip", "kfs_run")], build=_kfs_build,
     run=lambda e, c, i, o: c.search_by_projection_keyframe(pm.CAM, i["kp"], i["desc"], B4, [i["cand"]], th=10.0, orb_dist=100),
     want=lambda e, i: kf_search_ref.search(i["cand"], pm.CAM, i["kp"], i["desc"], B4, 10.0, 100), check=_kfs_check,
     vacuous=lambda e, i, w: _true(w["n_matches"] * 4 > len(i["cand"]["pos"]) and w["n_searched"] > w["n_matches"]))


def _fuse_build(e, size):
    kf, mp = fuse_ref.random_scene(e.hvo.KEYPOINT_DT, 65, 17) if size == "S" else fuse_ref.random_scene(e.hvo.KEYPOINT_DT, 300, 257)
    return dict(kf=kf, mp=mp)


def _fuse_check(e, g, w):
    import test_fuse_gpu
    test_fuse_gpu.same(g[0], w)


def _fuse_vac(e, i, w):
    assert w["n_fused"] >= 3 and w["n_searched"] > w["n_fused"] and (w["gate"] != 0).any()


case(name="fuse_points", sites=[("fuse.hip", "fuse_run")], build=_fuse_build,
     run=lambda e, c, i, o: c.fuse_points(pm.CAM, [i["kf"]], i["mp"], B4), want=lambda e, i: fuse_ref.fuse(i["kf"], i["mp"], pm.CAM), check=_fuse_check,
     vacuous=_fuse_vac)


def _pmap_of(e, mp, n=None):
    n = len(mp["pos"]) if n is None else n
    m = e.hvo.PointMap(0, 16)
    m.set_many(0, mp["pos"][:n], mp["normal"][:n], mp["max_dist"][:n], mp["min_dist"][:n], mp["desc"][:n], mp.get("observed"), mp.get("bad"))
    return m


def _fslot_build(e, size):
    i = _fuse_build(e, size)
    n = len(i["mp"]["pos"])
    i["slots"] = np.random.RandomState(4).permutation(n)[: n - 2].astype(np.int32)          # a permuted subset of the slots
    return i


def _fslot_want(e, i):
    sl = i["slots"]
    sub = {k: np.asarray(v)[sl] for k, v in i["mp"].items()}
    return fuse_ref.fuse(dict(i["kf"], skip=i["kf"]["skip"][sl]), sub, pm.CAM)


case(name="fuse_points_slots", sites=[("fuse.hip", "fuse_run")], build=_fslot_build, open=lambda e, i: dict(map=_pmap_of(e, i["mp"])),
     run=lambda e, c, i, o: c.fuse_points_slots(o["map"], i["slots"], pm.CAM, [dict(i["kf"], skip=i["kf"]["skip"][i["slots"]])], B4),
     want=_fslot_want, check=_fuse_check, vacuous=_fuse_vac)


def _np_build(e, size):
    cur, kfs = new_points_ref.random_scene(n=64 if size == "S" else 300, seed=9, poses=new_points_ref.SCENE_POSES[:2], twins=0 if size == "S" else 5)
    return dict(cur=cur, kfs=kfs)


def _np_check(e, g, w):
    import test_new_points_gpu
    test_new_points_gpu.same(g, w)


case(name="create_new_map_points", sites=[("new_points.hip", "np_run")], build=_np_build,
     run=lambda e, c, i, o: c.create_new_map_points(new_points_ref.CAM, i["cur"], i["kfs"]),
     want=lambda e, i: new_points_ref.full(i["cur"], i["kfs"], new_points_ref.CAM, new_points_ref.CAM[4]), check=_np_check,
     vacuous=lambda e, i, w: _true(w[1]["n_new"] >= 5 and all(r["gate"] == 0 for r in w[0]) and sum((r["match_idx2"] >= 0).sum() for r in w[0]) > w[1]["n_new"]))


# ---------------------------------------------------------------------------------------------------------------- the two resident maps
def _lp_build(e, size):
    nt, n = (65, 100) if size == "S" else (1000, 1500)
    kp, desc = kf_search_ref.planted_frame(e.hvo.KEYPOINT_DT, seed=57, nt=nt)
    rng = np.random.RandomState(57)
    z = rng.uniform(1.0, 4.0, nt).astype(F32); z[::9] = -1                       # every ninth key point without depth
    ur = np.where(z > 0, kp["x"] - F32(pm.CAM[4]) / np.where(z > 0, z, 1), -1).astype(F32)
    T = pm.scene_pose()
    M, _ = pm.make_map(n, "alt", T, seed=57)
    pm.add_frame_points(M, kp, desc, z, T, range(1, n, 2))
    M["bad"][::7] = 1
    held = np.full(nt, -1, np.int32); held[3] = 9; held[5] = 14               # slot 14 is bad
    return dict(kp=kp, desc=desc, ur=ur, T=T, M=M, held=held, extra=np.arange(3, n, 11).astype(np.int32))


def _lp_check(e, r, o):
    import test_point_map_gpu
    test_point_map_gpu.same(r, o)


case(name="search_local_points", sites=[("api.hip", "hvo_search_local_points"), ("local_points.hip", "d_a"), ("local_points.hip", "d_b")], build=_lp_build,
     open=lambda e, i: dict(map=_pmap_of(e, i["M"])), uses_map=True,
     run=lambda e, c, i, o: c.search_local_points(o["map"], pm.CAM, i["T"], i["kp"], i["ur"], i["desc"], B4, held=i["held"], seen_extra=i["extra"], th=1.0,
                                                  log_scale_factor=pm.LOG_SF, n_levels=pm.N_LEVELS),
     want=lambda e, i: pm.search_local_points(i["M"], pm.CAM, i["T"], B4, pm.LOG_SF, pm.N_LEVELS, pm.SF, 1.0, i["kp"], i["ur"], i["desc"], i["held"], i["extra"]),
     check=_lp_check, vacuous=lambda e, i, w: _true(w["n_matches"] > 10 and w["n_in_view"] > w["n_matches"] and w["n_slots_tested"] < len(i["M"]["pos"])),
     arena=lambda e, i: al(len(i["kp"]) * 28) + al(len(i["kp"]) * 4) + al(len(i["kp"]) * 32) + 256)


LCAM = line_map_ref.CAM


def _ll_build(e, size):
    from test_line_map_gpu import add_frame_lines
    nl, n = (40, 100) if size == "S" else (200, 300)
    d = e.synth.make_depth(0x5EED5104, 640, 480)
    kl = inside(keylines(e.orc, 640, 480, 3 * nl, 58), 640, 480)[:nl]
    assert len(kl) == nl
    l3 = e.orc.lines_3d(kl, d, seed=3, fx=LCAM[0], fy=LCAM[1], cx=LCAM[2], cy=LCAM[3])
    rng = np.random.RandomState(58)
    ld = rng.randint(0, 256, (nl, 32)).astype(np.uint8)
    cs, ci, _ = e.orc.assign_lines_to_grid(kl, np.array(line_map_ref.BOUNDS, F32))
    T = line_map_ref.scene_pose()
    M, _ = line_map_ref.make_map(n, "alt", T, seed=5)
    add_frame_lines(M, kl, ld, l3, T, range(1, n, 2), tilt_every=3)
    M["bad"][::7] = 1
    held = np.full(nl, -1, np.int32); held[0], held[1] = 14, 9                  # slot 14 is bad
    return dict(kl=kl, fn=line_functions(kl), l3=l3, ld=ld, cs=cs, ci=ci, T=T, M=M, held=held, extra=np.arange(3, n, 11).astype(np.int32))


def _lmap_open(e, i):
    M = i["M"]
    lm = e.hvo.LineMap(slots=0)
    lm.set_many(0, M["pos"], M["wvec"], M["normal"], M["max_dist"], M["min_dist"], M["desc"], M["observed"], M["bad"])
    return dict(map=lm)


def _ll_check(e, r, o):
    import test_line_map_gpu
    test_line_map_gpu.same(r, o)


case(name="search_local_lines", sites=[("api.hip", "hvo_search_local_lines"), ("local_lines.hip", "d_a"), ("local_lines.hip", "d_b")], build=_ll_build,
     open=_lmap_open, uses_map=True,
     run=lambda e, c, i, o: c.search_local_lines(o["map"], LCAM, i["T"], i["kl"], i["fn"], i["l3"], i["ld"], i["cs"], i["ci"], line_map_ref.BOUNDS, held=i["held"],
                                                 seen_extra=i["extra"], log_scale_factor=line_map_ref.LOG_SF, th=5.0, rel_map=True),
     want=lambda e, i: line_map_ref.search_local_lines(i["M"], LCAM, i["T"], line_map_ref.BOUNDS, line_map_ref.LOG_SF, 5.0, 0.95, i["kl"], i["fn"], i["l3"], i["ld"],
                                                       i["cs"], i["ci"], i["held"], i["extra"]),
     check=_ll_check, vacuous=lambda e, i, w: _true(w["n_matches"] > 2 and w["n_in_view"] > 20 and (i["l3"]["good"] == 1).sum() >= 5))


# ---------------------------------------------------------------------------------------------------------------- the line calls and the map refresh
# S stays below one block of 256 with ragged counts; L crosses the 256 boundaries (an entry block, an LDS chunk of LF_CHUNK records, a wave's
# four rows per lane).  The seeds are chosen so that the vacuity conditions hold; they are no part of them.
def _nl_build(e, size):
    n, poses, cuts = (40, new_lines_ref.SCENE_POSES[:2], (33, 40)) if size == "S" else (300, new_lines_ref.SCENE_POSES[:3], (300, 257, 190))
    cur, kfs = new_lines_ref.random_scene(n=n, seed=35, poses=poses)
    return dict(cur=cur, kfs=[new_lines_ref.cut(k, m) for k, m in zip(kfs, cuts)])


def _nl_check(e, g, w):
    import test_new_lines_gpu
    test_new_lines_gpu.same(g, w)


def _nl_vac(e, i, w):
    """every neighbour is searched, and every pair creates a line and rejects a triple it evaluated (an outcome past 'no match on a side')"""
    m, p, s = w
    assert len(p) == len(i["kfs"]) * (len(i["kfs"]) - 1) // 2 and all(x["gate"] == 0 for x in m)
    for x in p:
        assert x["n_created"] >= 1 and (np.asarray(x["outcome"]) > new_lines_ref.NO_MATCH).any(), np.unique(x["outcome"])


case(name="create_new_map_lines", sites=[("line_triang.hip", "nl_run")], build=_nl_build,
     run=lambda e, c, i, o: c.create_new_map_lines(i["cur"], i["kfs"]), want=lambda e, i: new_lines_ref.full(i["cur"], i["kfs"]), check=_nl_check, vacuous=_nl_vac)


def _lf_build(e, size):
    if size == "S":
        kfs, mp = line_fuse_ref.random_scene(e.hvo.KEYLINE_DT, n_kf=2, n_lines=70, n=37, seed=83)
        kfs = [kfs[0], line_fuse_ref.cut(kfs[1], 3)]
    else:
        kfs, mp = line_fuse_ref.random_scene(e.hvo.KEYLINE_DT, n_kf=3, n_lines=300, n=300, seed=84)
        kfs = [kfs[0], line_fuse_ref.cut(kfs[1], 257), line_fuse_ref.cut(kfs[2], 130)]
    return dict(kfs=kfs, mp=mp)


def _lf_want(e, i):
    return [line_fuse_ref.fuse(kf, i["mp"]) for kf in i["kfs"]]


def _lf_check(e, g, w):
    import test_line_fuse_gpu
    test_line_fuse_gpu.same(g, w)


def _lf_vac(e, i, w):
    """every key frame fuses an entry and rejects one: at a gate, and among the searched"""
    for x in w:
        assert x["n_fused"] >= 1 and (x["gate"] != 0).any() and x["n_searched"] > x["n_fused"], (x["n_fused"], x["n_searched"])


case(name="fuse_lines", sites=[("line_fuse.hip", "lf_run")], build=_lf_build,
     run=lambda e, c, i, o: c.fuse_lines(i["kfs"], i["mp"], n_levels=3), want=_lf_want, check=_lf_check, vacuous=_lf_vac)


def _lfs_build(e, size):
    i = _lf_build(e, size)
    n = len(i["mp"]["pos"])
    i["slots"] = np.random.RandomState(9).permutation(n + 5)[:n].astype(np.int32)             # entry k lives in slot slots[k]; five slots nobody names
    return i


def _lfs_open(e, i):
    mp, sl = i["mp"], i["slots"]; n = len(sl) + 5
    pos, nrm, mx, mn, desc = np.zeros((n, 6)), np.zeros((n, 3)), np.ones(n, F32), np.ones(n, F32), np.zeros((n, 32), np.uint8)
    pos[sl] = mp["pos"]; nrm[sl] = mp["normal"]; mx[sl] = mp["max_distance"]; mn[sl] = mp["min_distance"]; desc[sl] = mp["desc"]
    m = e.hvo.LineMap(slots=16)
    m.set_many(0, pos, pos[:, 3:] - pos[:, :3], nrm, mx, mn, desc)
    return dict(map=m)


case(name="fuse_lines_slots", sites=[("line_fuse.hip", "lf_run")], build=_lfs_build, open=_lfs_open,
     run=lambda e, c, i, o: c.fuse_lines_slots(o["map"], i["slots"], i["kfs"], n_levels=3), want=_lf_want, check=_lf_check, vacuous=_lf_vac)


def _mr_build(line):
    def build(e, size):
        rng = np.random.RandomState(91 if line else 90)
        if size == "S":
            counts = rng.randint(0, 6, 33)                                # at most 5 observations
        else:
            counts = rng.randint(0, 12, 300); counts[77] = 256            # one feature at the limit: four rows per lane
        counts[:12] = np.maximum(counts[:12], 2)                          # the features plant_statuses works on have observers
        obs = map_refresh_ref.plant_statuses(map_refresh_ref.make_obs(counts, rng, bad_rate=0.15), rng)
        return dict(pos=map_refresh_ref.line_positions(len(counts), rng) if line else map_refresh_ref.point_positions(len(counts), rng), obs=obs)
    return build


def _mr_check(line):
    def check(e, g, w):
        import test_map_refresh_gpu
        test_map_refresh_gpu.same(g, w, line)
    return check


def _mr_vac(e, i, w):
    assert len(set(w["status"].tolist())) >= 3 and (w["status"] == 0).sum() > len(w["status"]) // 2, np.unique(w["status"])
    assert np.diff(i["obs"]["obs_start"]).max() == (256 if len(w["status"]) > 256 else 5)


case(name="refresh_map_points", sites=[("map_refresh.hip", "mr_run")], build=_mr_build(False),
     run=lambda e, c, i, o: c.refresh_map_points(i["pos"], i["obs"]), want=lambda e, i: map_refresh_ref.refresh_points(i["pos"], i["obs"]),
     check=_mr_check(False), vacuous=_mr_vac)

case(name="refresh_map_lines", sites=[("map_refresh.hip", "mr_run")], build=_mr_build(True),
     run=lambda e, c, i, o: c.refresh_map_lines(i["pos"], i["obs"]), want=lambda e, i: map_refresh_ref.refresh_lines(i["pos"], i["obs"]),
     check=_mr_check(True), vacuous=_mr_vac)

BY_NAME = {c.name: c for c in CASES}
_inputs = {}


def inputs(e, name, size):
    """a case's S or L input and the restatement's answer, built once per process and never modified"""
    k = (name, size)
    if k not in _inputs:
        c = BY_NAME[name]
        i = c.build(e, size)
        _inputs[k] = (i, c.want(e, i) if c.want else None)
    return _inputs[k]
