"""Times DetectRelocalizationCandidates on the resident key-frame database (hvo_stream_keyframe_db_query) beside the host path it replaces,
per database size:

    key frames | words in the query | device: query kernels, whole call (ms) || host: download of the bag, host query, their sum (ms) | candidates dev/host

Device side: one synthetic frame (about 1000 features) goes through a Stream with the ORB stage and gets its bag of words on a k = 10,
L = 5 vocabulary with random node descriptors (100 000 words: about 900 distinct words per frame, near ORBvoc's 800).  `kernels` is the
device time between hipEvents around the query's four kernels (hvo_keyframe_db_last_kernel_ms), `call` the wall time of the whole call with
its upload, its download and its one synchronisation; medians of 50 after 5 warm-up calls.
Host side: what a tracker without the call does with a resident frame: hipMemcpy of the bag (12 bytes per word) down, then the
single-thread query on an inverted file of std::list (tools/kf_db_host.cpp, the reference's shape); median of 50.

How the databases are drawn: 5 % of the key frames (at most 40) are views of the query's place and hold 60 % of the query's words; every
other key frame holds 3 % of them (words every indoor view has); the rest of each bag, up to the query's word count, are words drawn
uniformly from the vocabulary.  Every key frame has up to 10 neighbours among the 10 key frames added before it.  The candidates of both
sides are printed and must agree.

Run on an MI355X, after __graft_entry__.build():  python tools/kf_db_timing.py > profiles/kf_db.txt"""
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def write_case(path, n_voc_words, scoring, script):
    """a script of tests/kf_db_ref.py as the binary file tools/kf_db_host.cpp plays: int32 (words in the vocabulary, scoring, operations), then
    per operation int32 (type, slot or mode) and its arrays"""
    i32 = lambda *a: np.array(a, np.int32).tobytes()
    with open(path, "wb") as f:
        f.write(i32(n_voc_words, scoring, len(script)))
        for op in script:
            if op[0] == "add":
                f.write(i32(0, op[1], len(op[2]))); f.write(np.ascontiguousarray(op[2], np.int32).tobytes()); f.write(np.ascontiguousarray(op[3], np.float64).tobytes())
            elif op[0] == "erase":
                f.write(i32(1, op[1]))
            elif op[0] == "clear":
                f.write(i32(2, 0))
            elif op[0] == "cov":
                f.write(i32(3, op[1], len(op[2]))); f.write(np.ascontiguousarray(op[2], np.int32).tobytes())
            elif op[0] == "query":
                conn = np.ascontiguousarray([] if op[5] is None else op[5], np.int32)
                f.write(i32(4, op[3])); f.write(np.array([op[4]], np.float32).tobytes()); f.write(i32(len(conn))); f.write(conn.tobytes())
                f.write(i32(len(op[1]))); f.write(np.ascontiguousarray(op[1], np.int32).tobytes()); f.write(np.ascontiguousarray(op[2], np.float64).tobytes())
            else:
                raise ValueError(op[0])


def draw_database(rng, n_kf, n_voc_words, qw):
    """the adds and neighbour lists described at the head of this file"""
    script = []
    near = set(rng.choice(n_kf, min(max(n_kf // 20, 1), 40), replace=False).tolist())
    for s in range(n_kf):
        share = 0.6 if s in near else 0.03
        w = np.unique(np.concatenate([rng.choice(qw, int(share * len(qw)), replace=False), rng.randint(0, n_voc_words, len(qw) - int(share * len(qw)))])).astype(np.int32)
        v = 0.05 + rng.rand(len(w)); v /= v.sum()
        script.append(("add", s, w, v))
        script.append(("cov", s, list(range(max(0, s - 10), s))))
    return script


def main():
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, os.path.join(ROOT, "tools"))
    import __graft_entry__ as entry
    import kf_db_ref as ref
    from bow_timing import full_tree, med, hip_runtime, copy_ms
    hvo = entry.package()
    synth = __import__("importlib").import_module("hvo_amd.synth")
    exe = os.path.join(ROOT, "tools", "kf_db_host")
    subprocess.check_call(["g++", "-O2", "-std=c++14", os.path.join(ROOT, "tools", "kf_db_host.cpp"), "-o", exe])
    voc = full_tree(10, 5, 5)
    v = hvo.Vocabulary(10, 5, voc["parent"], voc["is_leaf"], voc["desc"], voc["weight"], voc["scoring"], voc["weighting"])
    st = hvo.Stream(depth=2, stages=hvo.STAGE_ORB, bf=0.0)
    t = st.submit(synth.make_frame("std", 0x5EED7100)[0]); fr = st.collect(t)
    bow = st.compute_bow(t, v, levelsup=3)
    qw, qv = bow["bow_word"], bow["bow_value"]
    hip = hip_runtime()
    print("# tools/kf_db_timing.py: %d features, %d words in the query; medians of 50 after 5 warm-up calls" % (len(fr["desc"]), len(qw)))
    print("# key frames | query words | query kernels  whole call || host: download  host query  sum | candidates dev/host")
    for n_kf in (100, 1000, 10000):
        script = draw_database(np.random.RandomState(n_kf), n_kf, 100000, qw)
        db = hvo.KeyFrameDatabase(v)
        for op in script:
            if op[0] == "add":
                db.add(op[1], op[2], op[3])
            else:
                db.set_covisible(op[1], op[2])
        for _ in range(5):
            r = st.keyframe_db_query(t, db)
        tc, kc = [], []
        for _ in range(50):
            c0 = time.perf_counter(); r = st.keyframe_db_query(t, db); tc.append((time.perf_counter() - c0) * 1e3)
            kc.append(db.last_kernel_ms())
        with tempfile.NamedTemporaryFile(suffix=".bin", delete=False) as f:
            pass
        write_case(f.name, 100000, ref.L1_NORM, script + [ref.Q(qw, qv)])
        out = subprocess.check_output([exe, f.name, "50"]).decode().splitlines()
        os.unlink(f.name)
        hc = [int(x) for x in out[0].split()[2:]]; hq = float(out[-1].split()[1])
        dn = copy_ms(hip, len(qw) * 12, True)
        same = "same" if hc == r["candidates"].tolist() else "DIFFERENT"
        print("%d | %d | %.3f %.3f || %.3f %.3f %.3f | %d/%d %s" % (n_kf, len(qw), float(np.median(kc)), float(np.median(tc)), dn, hq, dn + hq, len(r["candidates"]), len(hc), same))
        db.close()
    st.close(); v.close()


if __name__ == "__main__":
    main()
