"""CPU checks of tests/new_keyframe_ref.py, the restatement csrc/new_keyframe.hip is compared with on the device: hand-stated cases first, then
the closed forms of the selection (what the kernels count) against the sequential loops on every scene, with the conditions that make the
scenes worth running asserted one by one.  The last tests need the built library: the new symbols and the binding's methods."""
import ctypes
import os

import numpy as np
import pytest

import new_keyframe_ref as kr
from conftest import PKG_DIR

F32 = np.float32
OBS = np.array([1, 0, 1, 0, 1, 0, 1, 0], bool)               # the observed flag of the eight slots the hand cases hold


def _loops_equal_closed(depth, held, obs, th):
    a = kr.point_loop(depth, held, obs, th); b = kr.point_closed(depth, held, obs, th)
    assert a == b, (a, b)
    return a


# ---------------------------------------------------------------------------------------------------------------- hand-stated cases
def test_hand_three_points_all_near():
    """depths 2, 1, 0, 3 under th 5: candidates in order 1, 0, 3; nothing breaks; feature 3 holds an observed slot and is kept"""
    ents, proc = _loops_equal_closed(np.array([2, 1, 0, 3], F32), [-1, -1, -1, 0], OBS, 5.0)
    assert proc == [1, 0, 3] and ents == [1, 0]


def test_hand_break_after_the_increment():
    """150 candidates at depths 1 .. 150, th 0.5: c = 0, so 100 entries do not break (nPoints > 100 is false at 100) and the 101st does"""
    z = np.arange(1, 151).astype(F32)
    ents, proc = _loops_equal_closed(z, np.full(150, -1), OBS, 0.5)
    assert proc == list(range(101)) and ents == proc


def test_hand_one_beyond_the_near_ones():
    """120 near candidates and 30 far: the loop runs through the near ones and processes exactly one far entry"""
    z = np.concatenate([np.linspace(1, 2, 120), np.linspace(4, 5, 30)]).astype(F32)
    ents, proc = _loops_equal_closed(z, np.full(150, -1), OBS, 3.0)
    assert proc == list(range(121))


def test_hand_equal_depths_go_by_index():
    z = np.full(130, 2.5, F32)
    ents, proc = _loops_equal_closed(z, np.full(130, -1), OBS, 1.0)
    assert proc == list(range(101))


def test_hand_held_values():
    """-1 and an unobserved slot and FOREIGN_UNOBSERVED create; an observed slot and FOREIGN_OBSERVED keep"""
    held = [-1, 1, 0, kr.FOREIGN_UNOBSERVED, kr.FOREIGN_OBSERVED]
    ents, proc = _loops_equal_closed(np.array([1, 2, 3, 4, 5], F32), held, OBS, 9.0)
    assert proc == [0, 1, 2, 3, 4] and ents == [0, 1, 3]


def test_hand_lines_count_created_only():
    """200 line candidates, every second one held and observed, th below all: the line loop creates 101 (it counts created entries only and
    walks 201 candidates to find them) where the point rule would stop after 101 candidates with 51 created"""
    n = 260
    A = np.zeros((n, 3)); B = np.zeros((n, 3)); A[:, 2] = np.arange(1, n + 1); B[:, 2] = A[:, 2] - 0.5; A[:, 0] = 1.0
    held = np.where(np.arange(n) % 2 == 0, -1, 0)
    ents = kr.line_loop(A, B, held, OBS, 0.5)
    assert ents == list(range(0, 202, 2)) and ents == kr.line_closed(A, B, held, OBS, 0.5)
    as_points = kr.point_loop(A[:, 2].astype(F32), held, OBS, 0.5)[0]
    assert len(as_points) == 51 and set(as_points) < set(ents)


def test_hand_line_candidates_and_key():
    """both end-point z must be != 0 (a negative one is a candidate); the key is the larger z as a float"""
    A = np.array([[1, 0, 2.0], [1, 0, 0.0], [1, 0, -1.0], [0, 0, 3.0]]); B = np.array([[1, 0, 1.0], [1, 0, 4.0], [1, 0, -2.0], [0, 0, 3.5]])
    assert kr.line_loop(A, B, [-1] * 4, OBS, 9.0) == [2, 0, 3]
    assert kr.line_key(A[2], B[2]) == -1.0 and kr.line_key(A[3], B[3]) == 3.5


def test_hand_nan_line_depth_is_refused():
    A = np.array([[1, 0, 2.0], [1, 0, np.nan]]); B = np.array([[1, 0, 1.0], [1, 0, np.nan]])
    for f in (kr.line_loop, kr.line_closed):
        with pytest.raises(kr.Refused): f(A, B, [-1, -1], OBS, 3.0)
    # sz > ez is false for a NaN sz: the key is ez, the order is defined and the frame is taken
    A[1, 2] = np.nan; B[1, 2] = 1.5
    assert kr.line_loop(A, B, [-1, -1], OBS, 3.0) == [1, 0]


def test_hand_unproject_identity_pose():
    """the identity pose: x3D = ((u - cx) z / fx, (v - cy) z / fy, z); the normal is x3D / |x3D| and the range is |x3D| sf[level] down to / sf[7]"""
    T = np.eye(4, dtype=F32)[:3]
    Rwc, Ow = kr.camera_parts(T)
    P = kr.unproject(420.0, 240.0, 2.0, (500.0, 500.0, 320.0, 240.0), Rwc, Ow)
    assert np.array_equal(P, np.array([F32(F32(100.0) * F32(2.0)) * (F32(1.0) / F32(500.0)), 0.0, 2.0], F32))
    n, mx, mi = kr.point_entry(P, Ow, 2, 8, kr.pm.SF, False)
    d = float(np.sqrt(np.float64(P[0]) ** 2 + 4.0))
    assert abs(float(mx) - d * 1.44) < 1e-5 and abs(float(mi) - float(mx) / float(kr.pm.SF[7])) < 1e-6 and abs(float(n[2]) - 2.0 / d) < 1e-6


def test_hand_negative_zero_normal():
    """a point straight ahead of a camera at the origin: d = (-0.0, 0, z) when x = -0.0.  The sole-observer sum gives +0.0, the Frame
    constructor's quotient keeps -0.0"""
    P = np.array([-0.0, 0.0, 2.0], F32); Ow = np.zeros(3, F32)
    kf = kr.point_entry(P, Ow, 0, 8, kr.pm.SF, False)[0]; tmp = kr.point_entry(P, Ow, 0, 8, kr.pm.SF, True)[0]
    assert not np.signbit(kf[0]) and np.signbit(tmp[0]) and kf[2] == tmp[2] == 1.0


def test_hand_struct_row():
    T = np.eye(4, dtype=F32)[:3]
    Rwc, Ow = kr.camera_parts(T)
    A = np.array([[1.0, 0, 2], [1.0, 0, 2], [1.0, 0, 2], [0.0, 1, 2]]); B = A + np.array([[1.0, 0, 0], [0, 1.0, 0], [1.0, 1.0, 0], [1.0, 0, 0]])
    row = kr.struct_row(np.array([0, 0, 3.0, 2, 0, 3.0]), A, B, Rwc, Ow)
    assert row.tolist() == [1, 2, 0, 0]                              # parallel, perpendicular, 45 degrees, gated out by first[0] == 0


# ---------------------------------------------------------------------------------------------------------------- scenes
def _scene(n, seed, th, z_lo=0.5, z_hi=6.0, pattern="mixed", n_slots=40):
    kp, z, desc = kr.make_points(n, seed, z_lo, z_hi)
    rng = np.random.RandomState(seed + 1000)
    obs = (np.arange(n_slots) % 2 == 0)
    held = kr.held_pattern(n, pattern, n_slots, rng)
    return dict(kp=kp, z=z, desc=desc, held=held, obs=obs, th=th)


SCENES = dict(few=(60, 1, 3.0), exact=(400, 2, 0.6), near=(400, 3, 3.0), ties=(300, 4, 2.0), far=(300, 5, 0.4))


@pytest.mark.parametrize("name", sorted(SCENES))
def test_closed_forms_equal_the_loops_points(name):
    n, seed, th = SCENES[name]
    s = _scene(n, seed, th)
    if name == "ties": s["z"][s["z"] > 0] = F32(2.5)
    ents, proc = _loops_equal_closed(s["z"], s["held"], s["obs"], th)
    M = int((s["z"] > 0).sum()); c = int(((s["z"] > 0) & (s["z"] <= F32(th))).sum())
    assert len(proc) == min(M, max(c, 100) + 1)
    if name == "few": assert M < 100 and len(proc) == M
    if name == "exact": assert c < 100 <= M and len(proc) == 101
    if name == "near": assert c > 100 and len(proc) == c + 1 < M
    if name == "ties": assert proc == sorted(proc) and len(proc) == 101
    if name in ("exact", "far"):
        far = [i for i in proc if s["z"][i] > F32(th)]
        assert any(i in ents for i in far) and any(i not in ents for i in far)      # a processed far entry created, and one held
    held_kinds = {int(s["held"][i]) if s["held"][i] < 0 else ("obs" if s["obs"][s["held"][i]] else "unobs") for i in proc}
    assert held_kinds >= {-1, kr.FOREIGN_OBSERVED, kr.FOREIGN_UNOBSERVED, "obs", "unobs"}, held_kinds
    assert any(s["held"][i] >= 0 and not s["obs"][s["held"][i]] for i in ents)          # an unobserved held slot is re-created


def test_depth_equal_to_the_threshold_counts_as_near():
    """z == thDepth exactly: `first > mThDepth` is false, the entry is near; 110 such entries and 50 far ones process 111"""
    z = np.concatenate([np.full(110, F32(3.0)), np.linspace(4, 5, 50)]).astype(F32)
    ents, proc = _loops_equal_closed(z, np.full(160, -1), OBS, 3.0)
    assert len(proc) == 111 and (z[proc[:110]] == F32(3.0)).all()


@pytest.mark.parametrize("seed,th", [(11, 0.6), (12, 3.0), (13, 9.0)])
def test_closed_forms_equal_the_loops_lines(seed, th):
    kl, ldesc, A, B = kr.make_lines(500, seed)
    rng = np.random.RandomState(seed)
    obs = (np.arange(40) % 2 == 0)
    held = kr.held_pattern(500, "mixed", 40, rng)
    ents = kr.line_loop(A, B, held, obs, th)
    assert ents == kr.line_closed(A, B, held, obs, th) and len(ents) > 0
    z = np.array([kr.line_key(A[i], B[i]) for i in range(500)], F32); z[(A[:, 2] == 0) | (B[:, 2] == 0)] = 0
    as_points = kr.point_loop(z, held, obs, th)[0]
    if th < 1: assert set(as_points) < set(ents)                   # the created-only counter gives a different set than the point rule would


def test_init_gates():
    kl, ldesc, A, B = kr.make_lines(64, 21)
    A[5] = [0.0, 0.3, 2.0]; B[5] = [0.5, 0.3, 2.0]                 # x == 0 with z != 0: a key-frame candidate, not an init one
    A[6] = [0.4, 0.3, 0.0]; B[6] = [0.5, 0.3, 2.0]                 # z == 0 with x != 0: an init entry, not a key-frame candidate
    kl["sx"][7] = 0.0                                              # startPointX > 0.0 fails
    ini = kr.init_lines(kl["sx"], A); kf = kr.line_loop(A, B, np.full(64, -1), OBS, 9.0)
    assert 5 in kf and 5 not in ini and 6 in ini and 6 not in kf and 7 in kf and 7 not in ini
    assert ini == sorted(ini)
    assert kr.init_points(np.array([1, 0, -1, 2], F32)) == [0, 3]


def test_create_closed_and_loop_agree_and_bad_level():
    """the whole call by both selections; a planted level outside the table is reported, takes no slot and shifts no other entry's data"""
    T = kr.scene_pose(0); cam = kr.pm.CAM
    s = _scene(300, 31, 1.0)
    kl, ldesc, A, B = kr.make_lines(150, 32)
    obs = s["obs"]
    hl = kr.held_pattern(150, "mixed", 40, np.random.RandomState(5))
    first = kr.point_loop(s["z"], s["held"], obs, 1.0)[0][4]
    s["kp"]["octave"][first] = 9
    kw = dict(kp_un=s["kp"], depth=s["z"], desc=s["desc"], keylines=kl, ldesc=ldesc, l3d_A=A, l3d_B=B, th_depth=1.0, held_points=s["held"], held_lines=hl,
              pt_observed=obs, ln_observed=obs, first_point_slot=40, first_line_slot=40)
    a = kr.create(kr.KEYFRAME, cam, T, **kw); b = kr.create(kr.KEYFRAME, cam, T, closed=True, **kw)
    assert not kr.compare(a, b)
    assert a["pt_status"][4] == kr.BAD_LEVEL and a["pt_slot"][4] == -1 and a["held_points"][first] == -1
    made = a["pt_status"] == kr.CREATED
    assert a["pt_slot"][made].tolist() == list(range(40, 40 + int(made.sum()))) and a["n_points_created"] == made.sum() == len(made) - 1
    assert a["ln_rel"].shape == (len(a["ln_index"]), 150) and set(np.unique(a["ln_rel"])) == {0, 1, 2}
    t = kr.create(kr.TEMPORAL, cam, T, **kw)
    assert (t["held_points"][t["pt_index"][made]] == kr.FOREIGN_UNOBSERVED).all() and len(t["ln_index"]) == 0 and (t["pt_slot"] == -1).all()
    assert t["held_points"][first] == s["held"][first]


# ---------------------------------------------------------------------------------------------------------------- the library
NEW_SYMBOLS = ("hvo_kfi_default_params", "hvo_kf_insert_create", "hvo_kf_insert_destroy", "hvo_kf_insert_last_error", "hvo_create_keyframe_features",
               "hvo_stream_create_keyframe_features")


def test_example_compiles():
    """examples/create_keyframe.cpp against the C++ mirror (it runs in tests/test_new_keyframe_gpu.py); the header stays plain C"""
    import shutil
    import subprocess
    from conftest import ROOT
    cxx = shutil.which("g++") or shutil.which("c++")
    if not cxx: pytest.skip("no host compiler")
    subprocess.check_call([cxx, "-std=c++14", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-fsyntax-only", os.path.join(ROOT, "examples", "create_keyframe.cpp")])
    hdr = open(os.path.join(ROOT, "include", "hvo.h")).read()
    assert "#define HVO_ABI_VERSION 3 " in hdr and "hvo_create_keyframe_features" in hdr


def test_library_exports_and_binding(hvo):
    lib = ctypes.CDLL(os.path.join(PKG_DIR, "csrc", "libhvo.so"))
    assert not [n for n in NEW_SYMBOLS if not hasattr(lib, n)]
    assert set(NEW_SYMBOLS) <= set(hvo.EXPORTS)
    assert callable(hvo.Context.create_keyframe_features) and callable(hvo.Stream.create_keyframe_features) and hasattr(hvo, "KeyFrameInsert")
    p = hvo.KfiParams(); hvo.lib().hvo_kfi_default_params(ctypes.byref(p))
    assert (p.mode, p.line_geometry, p.first_point_slot, p.first_line_slot) == (hvo.KFI_KEYFRAME, 1, -1, -1)
    assert p.cos_par == kr.COS_PAR and p.cos_perp == kr.COS_PERP
    assert (hvo.KFI_MAX_FEATURES, hvo.KFI_MAX_LINES) == (kr.MAX_FEATURES, kr.MAX_LINES)
    assert ctypes.sizeof(hvo.KfiParams) == 48 and ctypes.sizeof(hvo.KfiResult) == 40 and ctypes.sizeof(hvo.KfiIO) == 8 + 18 * 8
