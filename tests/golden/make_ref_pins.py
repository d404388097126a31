#!/usr/bin/env python3
"""Regenerates tests/golden/ref_pins_v1.npz.

PROVENANCE: unlike frontend_v1.npz, these vectors are outputs of the REFERENCE itself: the three pieces of it that
compile from their own files (include/peac/DisjointSet.hpp, include/peac/AHCParamSet.hpp, src/lineIterator.cpp),
called through oracle/ref_shim.cpp as oracle/_ref/libhvoref.so (`make -C oracle ref REF=<reference checkout>`).
The inputs are stored next to the outputs, so tests/test_ref_pins.py replays them through the oracle without the
reference or its library; where the library is built, the test also checks that it still gives these vectors.

    make -C oracle ref REF=<reference checkout> && python tests/golden/make_ref_pins.py
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle", "_ref", "libhvoref.so")

DS_SIZES = (1, 2, 17, 3072)


def ds_ops(n, rng):
    """4 n steps of (Union(x, y), Find(q), getSetSize(q)) on n elements"""
    ops = np.empty((4 * n, 3), np.int32)
    for k in range(4 * n):
        ops[k] = (int(rng.integers(n)), int(rng.integers(n)), int(rng.integers(n)))
    return ops


def threshold_depths():
    """metre-scale and millimetre-scale depths, with the breakpoints of the default ParamSet"""
    return np.concatenate([np.linspace(0.0, 13.2, 331), np.linspace(0.0, 70000.0, 701), [499.999, 500.0, 500.001, 3999.9, 4000.0, 4000.1]])


def line_segments(rng):
    """segments in grid coordinates (64 x 48): steep / reversed / degenerate ones and end points outside the grid"""
    segs = [(0, 0, 0, 0), (3.5, 2.5, 3.5, 2.5), (0, 0, 63.9, 47.9), (63.9, 0, 0, 47.9), (10, 40, 10, 2), (5.2, 7.9, 5.9, 30.1)]
    segs += [tuple(rng.uniform(-4, 70, 4)) for _ in range(2000)]
    return np.array(segs, np.float64)


def load_ref(path=REF):
    L = C.CDLL(path)
    L.ref_ds_create.restype = C.c_void_p; L.ref_ds_create.argtypes = [C.c_int]
    L.ref_ds_union.argtypes = [C.c_void_p, C.c_int, C.c_int]
    L.ref_ds_find.argtypes = [C.c_void_p, C.c_int]; L.ref_ds_set_size.argtypes = [C.c_void_p, C.c_int]
    L.ref_ds_free.argtypes = [C.c_void_p]; L.ref_ds_free.restype = None
    L.ref_T_mse.restype = C.c_double; L.ref_T_mse.argtypes = [C.c_int, C.c_double]
    L.ref_T_ang.restype = C.c_double; L.ref_T_ang.argtypes = [C.c_int, C.c_double]
    L.ref_T_dz.restype = C.c_double; L.ref_T_dz.argtypes = [C.c_double]
    L.ref_line_iterator.argtypes = [C.c_double] * 4 + [C.c_void_p, C.c_void_p, C.c_int]
    return L


def ds_outputs(L, n, ops):
    """per step (Union's returned root, Find, getSetSize), then Find of every element at the end"""
    out = np.empty_like(ops); final = np.empty(n, np.int32)
    d = L.ref_ds_create(n)
    try:
        for k, (x, y, q) in enumerate(ops.tolist()):
            out[k] = (L.ref_ds_union(d, x, y), L.ref_ds_find(d, q), L.ref_ds_set_size(d, q))
        for q in range(n):
            final[q] = L.ref_ds_find(d, q)
    finally:
        L.ref_ds_free(d)
    return out, final


def threshold_outputs(L, zs):
    """columns: T_mse(P_INIT), T_mse(P_MERGING), T_mse(P_REFINE), T_ang(P_INIT), T_dz(z), T_dz(-z)"""
    return np.array([[L.ref_T_mse(0, z), L.ref_T_mse(1, z), L.ref_T_mse(2, z), L.ref_T_ang(0, z), L.ref_T_dz(z), L.ref_T_dz(-z)]
                     for z in zs.tolist()], np.float64)


def line_outputs(L, segs, cap=512):
    """cells of every walk, concatenated in order, and the walk lengths"""
    ax, ay = np.zeros(cap, np.int32), np.zeros(cap, np.int32)
    counts, cells = [], []
    for s in segs.tolist():
        n = L.ref_line_iterator(*s, ax.ctypes.data, ay.ctypes.data, cap)
        assert n <= cap
        counts.append(n); cells.append(np.stack([ax[:n], ay[:n]], 1))
    return np.array(counts, np.int32), np.concatenate(cells).astype(np.int32)


def build(L):
    out = {}
    rng = np.random.default_rng(7)
    for n in DS_SIZES:
        ops = ds_ops(n, rng)
        out["ds%d_ops" % n] = ops
        out["ds%d_out" % n], out["ds%d_final" % n] = ds_outputs(L, n, ops)
    zs = threshold_depths()
    out["t_z"] = zs
    out["t_out"] = threshold_outputs(L, zs)
    out["t_ang_merging_refine"] = np.array([L.ref_T_ang(1, 1.0), L.ref_T_ang(2, 1.0)], np.float64)
    segs = line_segments(np.random.default_rng(11))
    out["line_segs"] = segs
    out["line_counts"], out["line_cells"] = line_outputs(L, segs)
    return out


if __name__ == "__main__":
    path = os.path.join(HERE, "ref_pins_v1.npz")
    np.savez_compressed(path, **build(load_ref()))
    print("wrote", path, os.path.getsize(path), "bytes")
