"""MapPlane::UpdateCoefficientsAndPoints on the resident plane map (reference src/MapPlane.cc:300-368; csrc/plane_update.hip), without a GPU:
the restatement tests/plane_update_ref.py pinned to the oracle's voxel grid and to known answers, hvo_plane_update_transform (host arithmetic,
no device) through ctypes and from the stand-alone tools/plane_update_host.cpp, that program under the address and undefined-behaviour
sanitizers, and the new symbols' declarations, exports and struct sizes.  Every comparison is bit-equal."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import plane_update_ref as ref
from conftest import ROOT, PKG_DIR

F32 = np.float32
NEW = ["hvo_update_map_planes", "hvo_stream_update_map_planes", "hvo_plane_map_get_points", "hvo_plane_update_transform"]


def same_bits(a, b):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint32 if a.itemsize == 4 else np.uint64), b.view(np.uint32 if b.itemsize == 4 else np.uint64))


@pytest.mark.parametrize("seed", [0x5EED0002, 11, 12])
def test_restatement_voxel_grid_against_the_oracle(orc, synth, seed):
    """every labelled pixel's float point as pixel_point forms it, the restatement's voxel_grid per plane, against orc.plane_clouds' slice"""
    d = synth.make_depth(seed)
    labels, planes = orc.peac(d)
    rec, cloud = orc.plane_clouds(d, labels, planes)
    assert len(planes) >= 2
    fx, fy, cx, cy = (float(F32(v)) for v in (535.4, 539.2, 320.1, 247.6))
    dfac = float(F32(1.0) / F32(5000.0))
    for pl in range(len(planes)):
        i, j = np.nonzero(labels == pl)
        z = d[i, j].astype(np.float64) * dfac
        p = np.stack([((j.astype(np.float64) - cx) * z / fx), ((i.astype(np.float64) - cy) * z / fy), z], axis=1).astype(F32)
        got = ref.voxel_grid(p)
        want = cloud[rec["first"][pl]:rec["first"][pl] + rec["n_points"][pl]]
        assert len(got) > 0 and same_bits(got, want), (seed, pl, len(got), len(want))


def _lib():
    lib = ctypes.CDLL(os.path.join(PKG_DIR, "csrc", "libhvo.so"))
    lib.hvo_plane_update_transform.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    return lib


def test_transform_through_ctypes():
    lib = _lib()
    for name, T in ref.transform_cases():
        T = np.ascontiguousarray(T, F32); M = np.zeros((3, 4))
        assert lib.hvo_plane_update_transform(T.ctypes.data, M.ctypes.data) == 0
        assert same_bits(M, ref.transform_matrix(T)), name
    assert lib.hvo_plane_update_transform(None, None) == -1
    rng = np.random.RandomState(3)
    for _ in range(200):
        T = np.ascontiguousarray(ref.random_pose(rng)); M = np.zeros((3, 4))
        assert lib.hvo_plane_update_transform(T.ctypes.data, M.ctypes.data) == 0
        assert same_bits(M, ref.transform_matrix(T))


def test_transform_cases_cover_the_branches():
    """a condition on the inputs: each branch of Quaterniond(Matrix3d), and the w < 0 flip, occurs"""
    seen = set()
    for name, T in ref.transform_cases():
        m = T[:, :3].astype(np.float64)
        if m[0, 0] + m[1, 1] + m[2, 2] > 0:
            seen.add("trace")
        else:
            i = 0
            if m[1, 1] > m[0, 0]: i = 1
            if m[2, 2] > m[i, i]: i = 2
            seen.add(i)
        import pose_opt_ref
        if pose_opt_ref.quat_from_R(m)[0] < 0:
            seen.add("flip")
    assert seen == {"trace", 0, 1, 2, "flip"}, seen
    M = ref.transform_matrix(ref.transform_cases()[0][1])
    assert np.array_equal(M, np.eye(4)[:3])


def _host_program(tmp_path, flags, name):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-O1", "-std=c++14", "-ffp-contract=off"] + flags + [ROOT + "/tools/plane_update_host.cpp", "-o", exe])
    return exe


def _run_host_cases(exe, tmp_path):
    cases = ref.transform_cases()
    rng = np.random.RandomState(4)
    T = np.stack([c[1] for c in cases] + [ref.random_pose(rng) for _ in range(50)]).astype(F32)
    T.tofile(str(tmp_path / "T.bin"))
    subprocess.check_call([exe, "transform", str(tmp_path / "T.bin"), str(tmp_path / "M.bin")])
    M = np.fromfile(str(tmp_path / "M.bin"), np.float64).reshape(-1, 3, 4)
    assert len(M) == len(T)
    for k in range(len(T)):
        assert same_bits(M[k], ref.transform_matrix(T[k])), k
    # the whole merge on the host against the restatement: a slot's cloud, a frame cloud, a NaN point in each
    frame = ref.wall(rng, 300); slot = ref.voxel_grid(ref.wall(rng, 1500))
    frame[7, 1] = np.nan; slot[11, 2] = np.inf
    Tcw = ref.random_pose(rng, 0.5)
    Tcw.tofile(str(tmp_path / "t.bin")); frame.tofile(str(tmp_path / "f.bin")); slot.tofile(str(tmp_path / "s.bin"))
    subprocess.check_call([exe, "merge", str(tmp_path / "t.bin"), str(tmp_path / "f.bin"), str(tmp_path / "s.bin"), str(tmp_path / "o.bin")])
    want = ref.voxel_grid(np.concatenate([ref.transform(ref.transform_matrix(Tcw), frame), slot]))
    assert same_bits(np.fromfile(str(tmp_path / "o.bin"), F32).reshape(-1, 3), want)
    np.array([[0, 0, 0], [1e9, 0, 0]], F32).tofile(str(tmp_path / "f.bin"))
    assert subprocess.call([exe, "merge", str(tmp_path / "t.bin"), str(tmp_path / "f.bin"), str(tmp_path / "s.bin"), str(tmp_path / "o.bin")]) == 3


def test_transform_from_the_host_program(tmp_path):
    """tools/plane_update_host.cpp includes csrc/plane_update_xform.inc, the text the library compiles, under g++ -ffp-contract=off"""
    _run_host_cases(_host_program(tmp_path, [], "plane_update_host"), tmp_path)


def test_host_program_under_sanitizers(tmp_path):
    """the same run with -fsanitize=address,undefined: host code with its own main"""
    exe = _host_program(tmp_path, ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"], "plane_update_host_san")
    _run_host_cases(exe, tmp_path)


def test_two_points_in_one_voxel_give_one_mean():
    """(coordinates in 64ths: the 2^-24 m fixed point holds them exactly, so the expected means are exact too)"""
    out = ref.voxel_grid(np.array([[1, 2, 3], [3, 4, 5]], F32) / 64)
    assert same_bits(out, np.array([[2, 3, 4]], F32) / 64)
    out = ref.voxel_grid(np.array([[1, 2, 3], [3, 4, 5], [3, 4, 6]], F32) / 64)   # a mean that is not a float: rounded once
    assert same_bits(out, (np.array([[7, 10, 14]], np.float64) / (3 * 64)).astype(F32))
    # below 2^-24 m the fixed point rounds: the documented deviation of the plane tail's voxel grid
    assert same_bits(ref.voxel_grid(np.array([[0.05, 0.05, 0.05]], F32)), (np.rint(np.full((1, 3), F32(0.05), np.float64) * 2 ** 24) / 2 ** 24).astype(F32))
    out = ref.voxel_grid(np.array([[0.25, 0.5, 0.75]] * 3, F32))
    assert same_bits(out, np.array([[0.25, 0.5, 0.75]], F32))


def test_voxel_edges_follow_floorf():
    """points at k * 0.1f and one ulp to either side, on both signs: the voxel is where floorf(p * 10.0f) in float says"""
    inv = F32(1.0) / F32(0.1)
    for k in (-7, -3, -1, 1, 2, 3, 7, 10, 33):
        c = F32(k) * F32(0.1)
        for x in (np.nextafter(c, F32(-np.inf)), c, np.nextafter(c, F32(np.inf))):
            lo = F32(np.floor(c * inv)) - F32(2)                              # an anchor two voxels below pins min_b
            anchor = (lo + F32(0.5)) * F32(0.1)
            assert np.floor(anchor * inv) == lo
            out = ref.voxel_grid(np.array([[anchor, 0, 0], [x, 0, 0]], F32))
            want_voxel = int(np.floor(F32(x) * inv) - lo)
            assert want_voxel in (1, 2, 3) and len(out) == 2
            # a probe in the middle of the voxel floorf names fuses with x; one in a neighbouring voxel does not
            for v in (1, 2, 3):
                probe = (lo + F32(v) + F32(0.5)) * F32(0.1)
                assert int(np.floor(probe * inv) - lo) == v
                n = len(ref.voxel_grid(np.array([[anchor, 0, 0], [x, 0, 0], [probe, 0, 0]], F32)))
                assert n == (2 if v == want_voxel else 3), (k, x, v)


def test_lower_bound_that_moves_down_keeps_the_order():
    a = np.array([[3, 3, 3], [15, 3, 3], [3, 9, 3], [3, 3, 23]], F32) / 64            # voxels (0,0,0) (2,0,0) (0,1,0) (0,0,3)
    out = ref.voxel_grid(a)
    assert same_bits(out, a)                                                  # ascending i + j div0 + k div0 div1
    b = np.concatenate([a, np.array([[-35, -15, -9]], F32) / 64])             # min_b moves down on every axis: to (-6, -3, -2)
    out = ref.voxel_grid(b[::-1])
    assert same_bits(out, b[[4, 0, 1, 2, 3]])
    assert same_bits(ref.voxel_grid(b[[2, 4, 0, 3, 1]]), out)                # the order of the points does not show


def test_overflow_and_dropped_points():
    assert ref.voxel_grid(np.array([[0, 0, 0], [1e9, 0, 0]], F32)) is None
    assert ref.voxel_grid(np.array([[0, 0, 0], [2000, 2000, 2000]], F32)) is None     # 20001^3 cells
    out = ref.voxel_grid(np.array([[3 / 64, 3 / 64, 3 / 64], [np.nan, 0, 0], [0, np.inf, 0], [15 / 64, 3 / 64, 3 / 64]], F32))
    assert same_bits(out, np.array([[3, 3, 3], [15, 3, 3]], F32) / 64)
    assert len(ref.voxel_grid(np.zeros((0, 3), F32))) == 0
    # apply: the refused operation leaves the slot, the others are done
    rec, cloud = ref.records_for([[[0, 0, 1]], [[0, 0, 1], [1e9, 0, 1]], [[0.5, 0, 1]]])
    slots = [[np.array([0, 0, 1, -1], F32), np.array([[0, 0, 1.01]], F32), False] for _ in range(3)]
    I = np.eye(4, dtype=F32)[:3]
    r = ref.apply(slots, rec, cloud, I, None, [(0, 0, ref.MERGE), (1, 1, ref.MERGE), (2, 2, ref.MERGE)])
    assert list(r["status"]) == [0, -4, 0] and r["n_done"] == 2 and list(r["n_after"]) == [1, 1, 2]
    assert same_bits(slots[1][1], np.array([[0, 0, 1.01]], F32))


def test_example_compiles():
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), "-fsyntax-only",
                           os.path.join(ROOT, "examples", "plane_map_update.cpp")])


NEW_PLANE_CPP = r"""
#include <cstdio>
#include <cstring>
#include "hvo.hpp"
// hvo::PlaneMap::trackUpdateList, the host half of PlaneMap::UpdateCoefficientsAndPoints: the loop of Tracking.cc:796-804
static int run(const int *match, int n, const unsigned char *outlier, int stride, int *n_ops, int *first_slot)
{
    hvo_plane_match pm; memset(&pm, 0, sizeof(pm));
    pm.n_planes = n;
    for (int i = 0; i < 64; i++) pm.match[i] = i < n ? match[i] : -1;
    hvo_plane_update u; bool newPlane = true;
    hvo::PlaneMap::trackUpdateList(pm, outlier, stride, u, newPlane);
    *n_ops = u.n; *first_slot = u.n ? u.slot[0] : -1;
    for (int k = 0; k < u.n; k++) if (u.op[k] != HVO_PLANE_UPDATE_MERGE || match[u.plane[k]] != u.slot[k]) return -1;
    return newPlane ? 1 : 0;
}
int main()
{
    int n_ops, s0;
    const int match[2] = { 7, -1 };                       // plane 0 matched to slot 7, plane 1 unmatched
    // the optimiser's layout, three bytes a plane [match, parallel, vertical]: plane 1 is no outlier in its match role, its other roles
    // and plane 0's are flagged -> newPlane
    const unsigned char a[6] = { 1, 1, 1, 0, 1, 1 };
    printf("%d", run(match, 2, a, 3, &n_ops, &s0)); printf(" %d %d\n", n_ops, s0);
    // plane 1 is an outlier in its match role only, nothing else is flagged -> no newPlane
    const unsigned char b[6] = { 0, 0, 0, 1, 0, 0 };
    printf("%d\n", run(match, 2, b, 3, &n_ops, &s0));
    // one byte a plane
    const unsigned char c[2] = { 1, 0 }, d[2] = { 0, 1 };
    printf("%d %d\n", run(match, 2, c, 1, &n_ops, &s0), run(match, 2, d, 1, &n_ops, &s0));
    // no flags: an unmatched plane is a new plane; all matched: none
    const int both[2] = { 3, 4 };
    printf("%d %d\n", run(match, 2, nullptr, 1, &n_ops, &s0), run(both, 2, nullptr, 1, &n_ops, &s0));
    return 0;
}
"""


def test_cpp_mirror_new_plane_flag_reads_the_match_role(tmp_path):
    """hvo::PlaneMap::UpdateCoefficientsAndPoints reads mvbPlaneOutlier[i] at outlier[i * stride]: with the pose optimiser's n x 3 buffer
    (stride 3) one matched and one unmatched plane whose parallel / vertical flags differ from the match flag give the reference's newPlane"""
    src = tmp_path / "new_plane.cpp"; src.write_text(NEW_PLANE_CPP)
    csrc = os.path.join(PKG_DIR, "csrc"); exe = str(tmp_path / "new_plane")
    subprocess.check_call(["g++", "-std=c++14", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src), "-L" + csrc, "-lhvo", "-Wl,-rpath," + csrc, "-o", exe])
    out = subprocess.check_output([exe]).decode().split("\n")
    assert out[:4] == ["1 1 7", "0", "1 0", "1 0"], out


def test_new_symbols_declared_exported_and_sized(hvo):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hvo.h")).read(), flags=re.S)
    lib = _lib()
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert hasattr(lib, n), n
        assert n in hvo.EXPORTS, n
    assert ctypes.sizeof(hvo.PlaneUpdate) == 4 + 3 * 256 and ctypes.sizeof(hvo.PlaneUpdateResult) == 4 * 256 + 4
    assert (hvo.PLANE_UPDATE_MERGE, hvo.PLANE_UPDATE_INSERT, hvo.PLANE_UPDATE_MAX_POINTS) == (ref.MERGE, ref.INSERT, ref.MAX_POINTS)
    for name, val in (("HVO_PLANE_UPDATE_MERGE", "0"), ("HVO_PLANE_UPDATE_INSERT", "1")):
        assert re.search(r"#define\s+%s\s+%s\b" % (name, val), hdr), name
    lib.hvo_abi_version.restype = ctypes.c_int
    assert lib.hvo_abi_version() == 3
    assert same_bits(hvo.plane_update_transform(ref.transform_cases()[1][1]), ref.transform_matrix(ref.transform_cases()[1][1]))
