"""Raw C-ABI calls of the Frame-tail entry points (hvo_surface_normals, hvo_plane_clouds, hvo_lines_3d, hvo_normals_lpvo) with an explicit
`stride`, for tests/test_tail_edges_gpu.py.  The Python bindings make the depth image contiguous first, so a row stride other than 2 * w
and the status codes of the refusals are only reachable this way.  Every function returns the status code first and raises nothing."""
import ctypes as C

import numpy as np

OK, INVALID_ARG, UNSUPPORTED, CAPACITY = 0, -1, -4, -5


def padded(depth, pad_bytes, fill=0xFFFF):
    """`depth` as a view into a parent whose rows are pad_bytes longer; the padding columns hold `fill`"""
    assert pad_bytes % 2 == 0
    h, w = depth.shape
    parent = np.full((h, w + pad_bytes // 2), fill, np.uint16)
    parent[:, :w] = depth
    view = parent[:, :w]
    assert view.strides == (2 * w + pad_bytes, 2)
    return view


def _depth(depth, stride):
    assert depth.dtype == np.uint16 and depth.ndim == 2 and depth.strides[1] == 2
    return depth.ctypes.data_as(C.c_void_p), depth.shape[1], depth.shape[0], depth.strides[0] if stride is None else stride


def surface_normals(hvo, ctx, depth, stride=None, cap=None, fill=0):
    """-> (rc, records, n); the records keep `fill` bytes where the call wrote nothing"""
    p, w, h, stride = _depth(depth, stride)
    full = (((h + 2) // 3) // 2) * (((w + 2) // 3) // 2)
    cap = full if cap is None else cap
    out = np.frombuffer(bytearray([fill]) * (max(cap, 1) * hvo.SURFACE_NORMAL_DT.itemsize), hvo.SURFACE_NORMAL_DT).copy()
    n = C.c_int(-1)
    rc = hvo.lib().hvo_surface_normals(ctx.h, p, w, h, stride, hvo._p(out), cap, C.byref(n))
    return rc, out, n.value


def plane_clouds(hvo, ctx, depth, labels, planes, n_planes=None, dist_th=0.05, cap=200000, stride=None):
    """-> (rc, plane records (n_planes), cloud rows (min(n_total, cap), 3), n_total)"""
    p, w, h, stride = _depth(depth, stride)
    labels = np.ascontiguousarray(labels, np.int32); planes = np.ascontiguousarray(planes)
    assert labels.shape == (h, w) and planes.dtype == hvo.PLANE_DT
    n_planes = len(planes) if n_planes is None else n_planes
    assert n_planes <= len(planes)
    out = np.zeros(max(n_planes, 1), hvo.PLANE_CLOUD_DT); cloud = np.zeros((max(cap, 1), 3), np.float32); n = C.c_int(-1)
    rc = hvo.lib().hvo_plane_clouds(ctx.h, p, w, h, stride, hvo._p(labels), hvo._p(planes), n_planes, dist_th, hvo._p(cloud), cap, hvo._p(out), C.byref(n))
    return rc, out[:n_planes], cloud[: max(min(n.value, cap), 0)].copy(), n.value


def lines_3d(hvo, ctx, kl, depth, seed=1, stride=None):
    """-> (rc, LINE3D_DT records)"""
    p, w, h, stride = _depth(depth, stride)
    kl = np.ascontiguousarray(kl)
    out = np.zeros(len(kl), hvo.LINE3D_DT)
    rc = hvo.lib().hvo_lines_3d(ctx.h, hvo._p(kl), len(kl), p, w, h, stride, seed, hvo._p(out))
    return rc, out


def normals_lpvo(hvo, ctx, depth, stride=None):
    """-> (rc, normals (n, 3) f64, depth (n) f32, pixel (n, 2) i32)"""
    p, w, h, stride = _depth(depth, stride)
    cap = ((h + 14) // 15) * ((w + 14) // 15)
    nrm = np.zeros((cap, 3)); dz = np.zeros(cap, np.float32); px = np.zeros((cap, 2), np.int32); n = C.c_int(-1)
    rc = hvo.lib().hvo_normals_lpvo(ctx.h, p, w, h, stride, hvo._p(nrm), hvo._p(dz), hvo._p(px), cap, C.byref(n))
    m = max(min(n.value, cap), 0)
    return rc, nrm[:m], dz[:m], px[:m]
