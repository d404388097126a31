"""Every line-growing form against the oracle on the crafted ramps of tests/lsd_cases.py: regions of up to 16 000 points, larger than a
worker's private list (LA_CAP) and than the closed form of reduce_region_radius takes (tests/test_lsd_crafted.py asserts on the oracle
alone that each image reaches the paths it is listed for, and names the two paths none reaches).

Bar: test_lsd_gpu.check -- key-line structure and descriptor bytes exact, floats within the project's TOL; which float fields were
bit-equal is printed (run with -s).  Every form runs twice on the same context: the second run starts from the tags, lists and pools the
giant regions left behind.  For the async kernel the control block must show that the device did take the `over` path (st_over) on the
frames whose largest region exceeds LA_CAP, unless the frame was grown again after an expired wait (printed: a finding, not a failure)."""
import ctypes

import numpy as np
import pytest

import lsd_cases
from test_lsd_gpu import check

pytestmark = pytest.mark.gpu
LIM = lsd_cases.limits()
STREAMED = ("ramp_v", "chevron10", "holes_diag")


@pytest.fixture(scope="module")
def crafted(orc):
    """name -> image, the oracle's lines, its path counters: computed once, shared, never written"""
    out = {}
    for name in lsd_cases.CASES:
        g = lsd_cases.make(name)
        out[name] = dict(g=g, ref=orc.line_extract(g), cnt=orc.lsd_path_counts(g))
    return out


def groups(crafted):
    """[((h, w), [names])]: frames of one size go into one batch"""
    out = {}
    for name in lsd_cases.CASES:
        out.setdefault(crafted[name]["g"].shape, []).append(name)
    return sorted(out.items())


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def compare(tag, name, kl, d, fn, ref):
    """print which float fields are bit-equal, then the project's check"""
    kl_o, d_o, fn_o = ref
    if len(kl) == len(kl_o):
        ff = [f for f in kl_o.dtype.names if kl_o.dtype[f].kind == "f"]
        diff = [f for f in ff if not np.array_equal(bits(kl[f]), bits(kl_o[f]))] + ([] if np.array_equal(bits(fn), bits(fn_o)) else ["linefn"])
        print("%-22s %-12s %3d lines, float fields not bit-equal: %d of %d %s" % (tag, name, len(kl), len(diff), len(ff) + 1, diff or ""))
    else:
        print("%-22s %-12s %d lines, the oracle has %d" % (tag, name, len(kl), len(kl_o)))
    check(kl, d, fn, kl_o, d_o, fn_o)


def async_evidence(hvo, ctx, tag, names, crafted):
    """the control blocks k_lsd_grow_async left: a frame with a region larger than a private list, done and not aborted, has dropped at
    least one overflowed list and grown that region again at the frontier, with all its workers on one XCD"""
    L = hvo.lib(); L.hvo_debug_lsd_async.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
    regrown, foreign, wpf = ctx.lsd_async_report()
    big = seen = 0
    for b, name in enumerate(names):
        ac = (ctypes.c_uint * 256)()
        assert L.hvo_debug_lsd_async(ctx.h, b, ac) == 0
        ctl = list(ac)
        print("%-22s %-12s done %d abort %d regions %d spec %d valid %d fail %d swallowed %d front %d over %d  xcd %d foreign %d"
              % (tag, name, ctl[3], ctl[6], ctl[8], ctl[9], ctl[10], ctl[11], ctl[12], ctl[13], ctl[14], ctl[32], ctl[33]))
        if crafted[name]["cnt"]["max_region"] > LIM["LA_CAP"]:
            big += 1
            if ctl[3] == 1 and ctl[6] == 0:
                seen += 1
                assert ctl[14] > 0, (tag, name, "st_over", ctl[8:15])
                assert ctl[32] != 0 and ctl[33] == 0, (tag, name, ctl[32:35])
    print("%-22s frames grown again after an expired wait: %d, foreign workers %d, workers per frame %d" % (tag, regrown, foreign, wpf))
    assert 0 <= regrown <= len(names) and seen >= big - regrown, (tag, big, seen, regrown)
    return regrown


@pytest.mark.parametrize("form", list(lsd_cases.FORMS))
def test_crafted_batches(hvo, crafted, monkeypatch, form):
    env, want = lsd_cases.FORMS[form]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for (h, w), names in groups(crafted):
        n = len(names)
        g = np.ascontiguousarray(np.stack([crafted[k]["g"] for k in names]))
        ctx = hvo.Context(max_batch=n)
        try:
            ctx.batch_upload(g, np.zeros((n, h, w), np.uint16))
            for run in range(2):
                ctx.batch_run(hvo.STAGE_LSD)
                res = ctx.batch_download(hvo.STAGE_LSD)
                rep = ctx.launch_report()["lsd"]
                bad = {f: (rep[f], v) for f, v in want.items() if rep[f] != v}
                assert not bad and rep["n"] == n, (form, bad, rep)
                tag = "%s run %d" % (form, run)
                for b, name in enumerate(names):
                    assert res[b]["status"] == 0, (tag, name, res[b]["status"])
                    compare(tag, name, res[b]["kl"], res[b]["ldesc"], res[b]["linefn"], crafted[name]["ref"])
                if want["grow"] == "async":
                    async_evidence(hvo, ctx, tag, names, crafted)
        finally:
            ctx.close()


@pytest.mark.parametrize("workers", [None, "64"])
@pytest.mark.parametrize("size", ["%dx%d" % (lsd_cases.W, lsd_cases.H), "%dx%d" % (lsd_cases.W_BIG, lsd_cases.H_BIG)])
def test_crafted_lone_frames(hvo, crafted, monkeypatch, size, workers):
    """Context().extract_lsd, one image after the other on the same context: the default plan of a lone frame (the async kernel; 32 workers
    at these sizes, 64 only from 600 000 scaled pixels on), and 64 workers forced -- as many as a frame can have, most of them inside
    one giant region"""
    if workers: monkeypatch.setenv("HVO_LSD_ASYNC", workers)
    names = dict(("%dx%d" % (w, h), nm) for (h, w), nm in groups(crafted))[size]
    tag = "lone %s w%s" % (size, workers or "32")
    ctx = hvo.Context()
    try:
        for name in names:
            kl, d, fn = ctx.extract_lsd(crafted[name]["g"])
            rep = ctx.launch_report()
            assert rep["batch"] is None and (rep["lsd"]["grow"], rep["lsd"]["async_w"], rep["lsd"]["n"]) == ("async", int(workers or 32), 1), rep
            compare(tag, name, kl, d, fn, crafted[name]["ref"])
            async_evidence(hvo, ctx, tag, [name], crafted)
    finally:
        ctx.close()


def test_crafted_frames_streamed(hvo, crafted):
    """the streamed mode over three of the images in a row, twice round its ring of three slots"""
    st = hvo.Stream(width=lsd_cases.W, height=lsd_cases.H, depth=3, stages=hvo.STAGE_LSD, bf=0.0)
    try:
        for turn in range(2):
            t = [st.submit(crafted[name]["g"]) for name in STREAMED]
            for name, ticket in zip(STREAMED, t):
                r = st.collect(ticket)
                assert r["status"] == 0, (turn, name, r["status"])
                compare("stream turn %d" % turn, name, r["kl"], r["ldesc"], r["linefn"], crafted[name]["ref"])
    finally:
        st.close()
