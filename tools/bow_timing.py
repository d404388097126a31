"""Times ComputeBoW + SearchByBoW on a RESIDENT stream frame beside the host path they replace, per vocabulary size and feature count:

    k L nodes | N | device: compute_bow kernels, call; search_by_bow kernels, call (ms) ||
    host: download of N descriptors, transform, search, upload of N matches, their sum (ms) | words dev/host, matches dev/host

Device side: two consecutive synthetic frames go through a Stream with the ORB stage; the first is the key frame (its node ids from
compute_bow, every feature has a map point), the second the current frame.  `kernels` is the device time between hipEvents around the
launches (hvo_stream_bow_last_kernel_ms), `call` the wall time of the whole call with its uploads, the result download and the
synchronisation; medians of 15.  compute_bow is recomputed every time by alternating levelsup with levelsup - 1 (a second call with the
same arguments launches nothing); only the calls at the listed levelsup are timed.
Host side: what a tracker without these calls does with a resident frame -- hipMemcpy of the N x 32 descriptor bytes down, the
single-thread tree walk and the sequential matcher (tools/bow_host.cpp, std::map vectors like DBoW2's), hipMemcpy of N x 4 match bytes up
for the resident pose optimisation.  The words and matches of both sides are printed and must agree.

The vocabularies have RANDOM node descriptors (no vocabulary file is needed): that understates the cache locality of a trained tree, where
descents of similar descriptors share their upper nodes -- for the host walk more than for the device.  Keep this note next to the numbers.
Run on an MI355X, after __graft_entry__.build():  python tools/bow_timing.py > profiles/r12_bow.txt"""
import ctypes as C
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as entry      # noqa: E402
import bow_ref as ref                # noqa: E402


def full_tree(k, L, seed):
    """rows level by level, vectorised (bow_ref.make_vocabulary is a Python loop: 1.1 M nodes take minutes)"""
    rng = np.random.RandomState(seed)
    parent, leaf = [], []
    first, count, rows = 0, 1, 0
    for level in range(1, L + 1):
        parent.append(np.repeat(np.arange(first, first + count, dtype=np.int32), k)); leaf.append(np.full(count * k, level == L, np.uint8))
        first, count, rows = rows + 1, count * k, rows + count * k
    parent = np.concatenate(parent); leaf = np.concatenate(leaf)
    desc = rng.randint(0, 256, (len(parent), 32)).astype(np.uint8)
    weight = np.where(leaf == 1, 0.5 + rng.rand(len(parent)) * 8, 0.0)
    return dict(k=k, L=L, scoring=ref.L1_NORM, weighting=ref.TF_IDF, parent=parent, is_leaf=leaf, desc=desc, weight=weight)


def med(fn, reps=15):
    fn(); t = []
    for _ in range(reps):
        t0 = time.perf_counter(); r = fn(); t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t)), r


def hip_runtime():
    """the HIP runtime this process already runs on (the one libhvo.so brought in)"""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            L = C.CDLL(line.split()[-1])
            L.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]; L.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]; L.hipFree.argtypes = [C.c_void_p]
            return L
    raise RuntimeError("libamdhip64 is not loaded")


def copy_ms(hip, nbytes, down):
    """median wall ms of one synchronous hipMemcpy of nbytes between the device and pageable host memory"""
    d = C.c_void_p(); assert hip.hipMalloc(C.byref(d), max(nbytes, 4)) == 0
    h = np.zeros(max(nbytes, 4), np.uint8)
    t, _ = med(lambda: hip.hipMemcpy(h.ctypes.data, d, nbytes, 2) if down else hip.hipMemcpy(d, h.ctypes.data, nbytes, 1), reps=31)
    hip.hipFree(d)
    return t


def main():
    hvo = entry.package()
    synth = __import__("importlib").import_module("hvo_amd.synth")
    exe = os.path.join(ROOT, "tools", "bow_host")
    subprocess.check_call(["g++", "-O2", "-std=c++14", os.path.join(ROOT, "tools", "bow_host.cpp"), "-o", exe])
    ctx = hvo.Context(); hip = hip_runtime()
    g, _, _ = synth.make_sequence("std", 0x5EED7100, 2)
    print("# tools/bow_timing.py: random node descriptors -- a trained tree has more cache locality than this, for the host walk more than for the device")
    print("# k L nodes | N | bow kernels  bow call  search kernels  search call || host: download  transform  search  upload  sum | words dev/host  matches dev/host")
    for k, L, up in ((4, 6, 4), (8, 5, 3), (10, 6, 4)):
        voc = full_tree(k, L, 5)
        v = hvo.Vocabulary(k, L, voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"], voc["scoring"], voc["weighting"])
        for nfeat in (500, 1000, 2000):
            st = hvo.Stream(depth=2, stages=hvo.STAGE_ORB, bf=0.0, orb_nfeatures=nfeat)
            t0, t1 = st.submit(g[0]), st.submit(g[1])
            f0, f1 = st.collect(t0), st.collect(t1)
            n = len(f1["desc"])
            kfb = ctx.compute_bow(v, f0["desc"], levelsup=up)
            kf = dict(desc=f0["desc"], node_id=kfb["node_id"], has_map_point=np.ones(len(f0["desc"]), np.uint8), angle=f0["kp_un"]["angle"])
            tb, kb = [], []
            for _ in range(15):
                st.compute_bow(t1, v, levelsup=up - 1)
                c0 = time.perf_counter(); b = st.compute_bow(t1, v, levelsup=up); tb.append((time.perf_counter() - c0) * 1e3)
                assert b["computed"]
                kb.append(st.bow_last_kernel_ms(t1)[0])
            ts, m = med(lambda: st.search_by_bow(t1, v, [kf]))
            ks = st.bow_last_kernel_ms(t1)[1]
            with tempfile.NamedTemporaryFile(suffix=".bin", delete=False) as f:
                np.array([k, L, voc["scoring"], voc["weighting"], len(voc["parent"]), up, n, len(f0["desc"]), 15], np.int32).tofile(f)
                for a in (voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"], f1["desc"], kf["desc"], kf["has_map_point"], kf["angle"].astype(np.float32),
                          f1["kp"]["angle"].astype(np.float32)):
                    np.ascontiguousarray(a).tofile(f)
            ht, hs, hw, hm = subprocess.check_output([exe, f.name]).decode().split()[:4]
            os.unlink(f.name)
            dn, upl = copy_ms(hip, n * 32, True), copy_ms(hip, n * 4, False)
            print("%d %d %d | %d | %.3f %.3f %.3f %.3f || %.3f %s %s %.3f %.3f | %d/%s %d/%s" % (
                k, L, len(voc["parent"]) + 1, n, float(np.median(kb)), float(np.median(tb)), ks, ts, dn, ht, hs, upl, dn + float(ht) + float(hs) + upl,
                len(b["bow_word"]), hw, m[0][1], hm))
            st.close()
        v.close()
    ctx.close()


if __name__ == "__main__":
    main()
