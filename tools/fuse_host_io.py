"""The case and result files of tools/fuse_host.cpp (its head comment has the layout), for tools/fuse_timing.py and tests/test_fuse.py."""
import os
import subprocess

import numpy as np


def write_case(path, kfs, mp, cam, bounds4, scale_factors, inv_sigma2, th, th_low, log_scale_factor, n_levels):
    n = len(mp["pos"])
    sf = np.ones(16, np.float32); sf[:len(scale_factors)] = scale_factors
    isg = np.ones(16, np.float32); isg[:len(inv_sigma2)] = inv_sigma2
    with open(path, "wb") as f:
        np.array([len(kfs), n, n_levels, th_low], np.int32).tofile(f)
        np.array(list(cam[:5]) + list(bounds4) + [th, log_scale_factor], np.float32).tofile(f)
        sf.tofile(f); isg.tofile(f)
        for k, dt in (("pos", np.float32), ("normal", np.float32), ("max_dist", np.float32), ("min_dist", np.float32), ("desc", np.uint8)):
            np.ascontiguousarray(mp[k], dt).tofile(f)
        for kf in kfs:
            kp = kf["kp_un"]; nt = len(kp)
            np.array([nt], np.int32).tofile(f)
            np.asarray(kf["Tcw"], np.float32).reshape(12).tofile(f)
            np.ascontiguousarray(kp["x"], np.float32).tofile(f); np.ascontiguousarray(kp["y"], np.float32).tofile(f)
            np.ascontiguousarray(kp["octave"], np.int32).tofile(f)
            (np.full(nt, -1.0, np.float32) if kf.get("uright") is None else np.ascontiguousarray(kf["uright"], np.float32)).tofile(f)
            np.ascontiguousarray(kf["desc"], np.uint8).tofile(f)
            (np.zeros(n, np.uint8) if kf.get("skip") is None else np.ascontiguousarray(np.asarray(kf["skip"]).astype(bool), np.uint8)).tofile(f)


def read_result(path, n_kf, n):
    out = []
    with open(path, "rb") as f:
        for _ in range(n_kf):
            out.append(dict(best_idx=np.fromfile(f, np.int32, n), best_dist=np.fromfile(f, np.int32, n), gate=np.fromfile(f, np.int8, n)))
    return out


def run(exe, workdir, kfs, mp, cam, bounds4, scale_factors, inv_sigma2, th, th_low, log_scale_factor, n_levels, reps=1, times=None):
    """-> one dict(best_idx, best_dist, gate) per key frame; times (a list) receives (grid ms, fuse ms), the medians of reps runs"""
    case, res = os.path.join(workdir, "fuse_case.bin"), os.path.join(workdir, "fuse_result.bin")
    write_case(case, kfs, mp, cam, bounds4, scale_factors, inv_sigma2, th, th_low, log_scale_factor, n_levels)
    t = subprocess.check_output([exe, case, res, str(reps)]).decode().split()
    if times is not None: times.extend(float(v) for v in t)
    return read_result(res, len(kfs), len(mp["pos"]))
