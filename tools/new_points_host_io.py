"""The case and result files of tools/new_points_host.cpp (its head comment has the layout), for tools/new_points_timing.py and
tests/test_new_points.py."""
import os
import subprocess

import numpy as np


def _write_kf(f, kf):
    kp = kf["kp_un"]; n = len(kp)
    raw = kp if kf.get("kp") is None else kf["kp"]
    stereo = kf.get("uright") is not None
    np.array([n, 1 if stereo else 0, 1 if kf.get("skip") else 0], np.int32).tofile(f)
    np.asarray(kf["Tcw"], np.float32).reshape(12).tofile(f)
    np.array([kf.get("mb", 0.0)], np.float32).tofile(f)
    for a in (kp["x"], kp["y"], raw["x"], raw["y"]): np.ascontiguousarray(a, np.float32).tofile(f)
    np.ascontiguousarray(kp["octave"], np.int32).tofile(f)
    for k in ("uright", "depth"): (np.ascontiguousarray(kf[k], np.float32) if stereo else np.full(n, -1.0, np.float32)).tofile(f)
    np.ascontiguousarray(kf["desc"], np.uint8).tofile(f)
    np.ascontiguousarray(kf["node_id"], np.int32).tofile(f)
    np.ascontiguousarray(np.asarray(kf["has_map_point"]).astype(bool), np.uint8).tofile(f)


def write_case(path, cur, kfs, cam, scale_factors, sigma2, th_low, n_levels, scale_factor):
    sf = np.ones(16, np.float32); sf[:len(scale_factors)] = scale_factors
    sg = np.ones(16, np.float32); sg[:len(sigma2)] = sigma2
    with open(path, "wb") as f:
        np.array([len(kfs), n_levels, th_low], np.int32).tofile(f)
        np.array(list(cam[:5]) + [scale_factor], np.float32).tofile(f)
        sf.tofile(f); sg.tofile(f)
        _write_kf(f, cur)
        for kf in kfs: _write_kf(f, kf)


def read_result(path, n_kf, n1):
    out = []
    with open(path, "rb") as f:
        for _ in range(n_kf):
            n = int(np.fromfile(f, np.int32, 1)[0])
            out.append(dict(created_idx1=np.fromfile(f, np.int32, n), created_idx2=np.fromfile(f, np.int32, n), x3d=np.fromfile(f, np.float32, 3 * n).reshape(n, 3)))
        owner = np.fromfile(f, np.int32, n1)
    return out, owner


def build(workdir, root):
    exe = os.path.join(workdir, "new_points_host")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-ffp-contract=off", os.path.join(root, "tools", "new_points_host.cpp"), "-o", exe])
    return exe


def run(exe, workdir, cur, kfs, cam, scale_factors, sigma2, th_low=50, n_levels=8, scale_factor=1.2, reps=1, times=None):
    """-> (one dict(created_idx1, created_idx2, x3d of the created) per neighbour, owner); times (a list) receives the median ms of reps runs"""
    case, res = os.path.join(workdir, "np_case.bin"), os.path.join(workdir, "np_result.bin")
    write_case(case, cur, kfs, cam, scale_factors, sigma2, th_low, n_levels, scale_factor)
    t = subprocess.check_output([exe, case, res, str(reps)]).decode().split()
    if times is not None: times.extend(float(v) for v in t)
    return read_result(res, len(kfs), len(cur["kp_un"]))


def same_answer(host, res, summ):
    """the host tool's lists, points and owner against a result of the library's shape"""
    hres, howner = host
    ok = np.array_equal(howner, summ["owner"])
    for h, r in zip(hres, res):
        i1 = r["created_idx1"]
        ok = ok and np.array_equal(h["created_idx1"], i1) and np.array_equal(h["created_idx2"], r["created_idx2"])
        ok = ok and h["x3d"].tobytes() == np.ascontiguousarray(r["x3d"][i1], np.float32).tobytes()
    return bool(ok)
