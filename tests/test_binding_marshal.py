"""The marshalling core of the binding (_marshal) and the records the call families declare on it, without a device: what alloc() hands to
a call, what cut() returns, what fill() passes for None / empty / flags / ragged lengths, the quirks each family keeps, and which exports
have a declared signature."""
import ctypes as C
import importlib

import numpy as np
import pytest


@pytest.fixture(scope="module")
def calls(hvo):
    """the tables and argument builders live in the package itself"""
    return hvo


@pytest.fixture(scope="module")
def marshal(hvo):
    return importlib.import_module("hvo_amd._marshal")


def _output_tables(hvo, calls):
    """every Outputs table of the calls with the record it fills"""
    return dict(LL_OUT=(calls.LL_OUT, hvo.LocalLinesIO), LP_OUT=(calls.LP_OUT, hvo.LocalPointsIO), KFI_OUT=(calls.KFI_OUT, hvo.KfiIO),
                KFDB_OUT=(calls.KFDB_OUT, hvo.KfdbResult), KFDB_VIEWS=(calls.KFDB_VIEWS, hvo.KfdbResult), BOW_OUT=(calls.BOW_OUT, hvo.Bow),
                KFS_OUT=(calls.KFS_OUT, hvo.KfSearchResult), FUSE_OUT=(calls.FUSE_OUT, hvo.FuseResult), LF_OUT=(calls.LF_OUT, hvo.LfResult),
                NP_OUT=(calls.NP_OUT, hvo.NpResult), NP_SUMMARY=(calls.NP_SUMMARY, hvo.NpSummary), NL_MATCH=(calls.NL_MATCH, hvo.NlMatch),
                NL_OUT=(calls.NL_OUT, hvo.NlResult), NL_SUMMARY=(calls.NL_SUMMARY, hvo.NlSummary),
                MR_POINT_OUT=(calls.MR_OUT[0], hvo.MrPointOut), MR_LINE_OUT=(calls.MR_OUT[1], hvo.MrLineOut))


def test_every_output_table_is_covered(hvo, calls, marshal):
    found = [v for v in vars(calls).values() if isinstance(v, marshal.Outputs)] + [t for v in vars(calls).values() if isinstance(v, tuple)
                                                                                 for t in v if isinstance(t, marshal.Outputs)]
    covered = [t for t, _ in _output_tables(hvo, calls).values()]
    assert found and all(any(t is c for c in covered) for t in found)


def test_sentinels(hvo, calls):
    assert hvo.FUSE_UNTOUCHED == hvo.KF_UNTOUCHED == hvo.NP_UNTOUCHED == hvo.NL_UNTOUCHED == -7 and hvo.MR_UNTOUCHED == hvo.KFI_UNTOUCHED == 119
    assert hvo.PNP_SENTINEL == 0xA5
    for t, s in ((calls.FUSE_OUT, -7), (calls.LF_OUT, -7), (calls.KFS_OUT, -7), (calls.NP_OUT, -7), (calls.NP_SUMMARY, -7), (calls.NL_MATCH, -7), (calls.NL_OUT, -7),
                 (calls.NL_SUMMARY, -7), (calls.MR_OUT[0], 119), (calls.MR_OUT[1], 119), (calls.KFI_OUT, 119), (calls.LL_OUT, 0), (calls.LP_OUT, 0), (calls.BOW_OUT, 0)):
        assert t.sentinel == s
    assert calls.LL_OUT.fill == calls.LP_OUT.fill == dict(held=-1, match_idx=-1, match_dist=256)            # the local-map searches' 0 / -1 / 256
    assert calls.BOW_OUT.fill == dict(word_id=-1, node_id=-1)                                               # BoW's -1 / 0
    assert calls.KFI_OUT.fill == dict(held_points=-1, held_lines=-1)                                        # held_* start at -1, not 119


@pytest.mark.parametrize("n", (0, 1, 5))
@pytest.mark.parametrize("n2", (0, 7))
def test_output_tables(hvo, calls, n, n2):
    for name, (t, Rec) in _output_tables(hvo, calls).items():
        keys = list(dict.fromkeys(r[3] for r in t.rows))
        lens = {k: (n if i == 0 else n2) for i, k in enumerate(keys)}
        rec = Rec()
        a = t.alloc(rec, **lens)
        assert list(a) == [r[0] for r in t.rows], name
        for f, dt, cols, length, cut in t.rows:
            m = max(lens[length], 1)
            assert a[f].dtype == np.dtype(dt) and a[f].shape == ((m, cols) if cols > 1 else (m,)), (name, f)
            assert np.array_equal(a[f], np.full(a[f].shape, t.fill.get(f, t.sentinel), dt)), (name, f)
            assert getattr(rec, f) == a[f].ctypes.data, (name, f)
        for f in t.counts:
            assert getattr(rec, f) == t.sentinel, (name, f)
        whole = t.cut(rec, a, ok=False, **lens)
        for f in a:
            assert whole[f].shape == a[f].shape and (t.copy or whole[f] is a[f]), (name, f)
        for count, want in ((3, lambda L, more: min(3 + more, L)), (n + 7, lambda L, more: min(n + 7 + more, L)), (-2, lambda L, more: max(0, min(-2 + more, L)))):
            for f, _, _, length, cut in t.rows:
                if cut is not None: setattr(rec, cut[0] if isinstance(cut, tuple) else cut, count)
            got = t.cut(rec, a, ok=True, **lens)
            for f, _, _, length, cut in t.rows:
                L = lens[length]
                exp = L if cut is None else want(L, cut[1] if isinstance(cut, tuple) else 0)
                assert len(got[f]) == exp and got[f].shape[1:] == a[f].shape[1:], (name, f, count)
                assert t.copy == (got[f].base is None), (name, f)            # a view of the call's array, or a copy where the family copies
    if n == 5:                                                               # the figures of the fuse family, spelled out
        t, rec = calls.FUSE_OUT, hvo.FuseResult(); a = t.alloc(rec, n=5)
        for count, length in ((3, 3), (12, 5), (-2, 0)):
            rec.n_fused = count
            d = t.finish(rec, a, True, n=5)
            assert len(d["fused_entry"]) == len(d["fused_idx"]) == length and len(d["best_idx"]) == 5 and d["n_fused"] == count and d["kernel_ms"] == (0.0, 0.0, 0.0)


def test_alloc_want_passes_null_but_keeps_the_array(hvo, calls):
    """the map refresh: an output not asked for goes to the call as NULL, and its untouched array is still returned"""
    P, I, O, o, n, keep = hvo._mr_args(False, [0, 2, 3], np.zeros((3, 32)), np.zeros((3, 3)), np.zeros((2, 3)), [0, 1], None, None, 8, 1.2, 3, ("desc", "status"))
    assert n == 2 and I.n == 2 and O.desc == o["desc"].ctypes.data and O.status == o["status"].ctypes.data
    assert O.normal is None and O.best_obs is None and (o["normal"] == hvo.MR_UNTOUCHED).all() and o["normal"].shape == (2, 3)
    assert I.kf_bad is None and I.skip is None and I.obs_desc == keep["obs_desc"].ctypes.data and keep["obs_desc"].dtype == np.uint8
    assert calls.MR_OUT[1].alloc(hvo.MrLineOut(), n=2)["normal"].dtype == np.float64 and "wvec" not in o


def test_inputs_null_flags_and_lengths(hvo, calls):
    kp = np.zeros(3, hvo.KEYPOINT_DT); T = np.arange(12, dtype=np.float64).reshape(3, 4)
    K, keep = calls._fuse_keyframes([dict(kp_un=kp, desc=np.zeros((3, 32)), uright=None, Tcw=T, skip=[2, 0, 5, 0]),
                                     dict(kp_un=kp[:0], desc=np.zeros((0, 32)), uright=np.zeros(0), Tcw=T)], [4, 0])
    assert K[0].n == 3 and K[0].uright is None and K[0].kp_un == keep[0]["kp_un"].ctypes.data                # a None optional array is NULL
    assert keep[0]["skip"].dtype == np.uint8 and keep[0]["skip"].tolist() == [1, 0, 1, 0] and K[0].skip == keep[0]["skip"].ctypes.data    # flags go as 0 / 1 bytes
    assert K[1].n == 0 and K[1].kp_un is None and K[1].desc is None and K[1].uright is None and K[1].skip is None     # an empty array is NULL
    assert list(K[0].Tcw) == list(range(12))
    with pytest.raises(ValueError):                                          # skip has the map side's length
        calls._fuse_keyframes([dict(kp_un=kp, desc=np.zeros((3, 32)), Tcw=T, skip=[1, 0])], [4])
    side = dict(pos=np.zeros((3, 3)), normal=np.zeros((3, 3)), max_dist=np.ones(3), min_dist=np.ones(3), desc=np.zeros((3, 32)))
    with pytest.raises(ValueError, match="^fuse_points: a map side's arrays differ in length$"):
        calls._FUSE.build([dict()], [dict(side, min_dist=np.ones(2))])
    line = dict(pos=np.zeros((3, 6)), normal=np.zeros((3, 3)), max_distance=np.ones(3), min_distance=np.ones(3), desc=np.zeros((4, 32)))
    with pytest.raises(ValueError, match="^fuse_lines: a map side's arrays differ in length$"):
        hvo._lf_maps([line])
    with pytest.raises(ValueError, match="^fuse_points: one map side per key frame, or one dict for all$"):
        calls._FUSE.build([dict(), dict()], [side])
    with pytest.raises(ValueError, match="^search_by_projection_keyframe: a candidate's arrays differ in length$"):
        calls._kfs_args(5, [dict(pos=np.zeros((2, 3)), skip=[0, 0], max_dist=[1, 1], min_dist=[1], desc=np.zeros((2, 32)), Tcw=T)], None, 10.0, 100, True, 0.18, 8)
    with pytest.raises(ValueError, match="^pnp_ransac: a problem's arrays differ in length$"):
        calls.PNP_PROBLEM.fill(hvo.PnpProblem(), dict(p3d=np.zeros((4, 3)), p2d=np.zeros((4, 2)), sigma2=np.ones(3), feature_index=np.arange(4)))
    with pytest.raises(ValueError, match="^pnp_ransac: pos and bad differ in length$"):
        calls.PNP_KF_SIDE.fill(hvo.PnpKeyframeSide(), dict(match_kf=np.arange(9), pos=np.zeros((4, 3)), bad=[0, 1, 0]))
    M, mk, ns = hvo._lf_maps([dict(line, desc=np.zeros((3, 32)))])
    assert ns == [3] and M[0].n == 3 and mk[0]["pos"].dtype == np.float64 and M[0].pos == mk[0]["pos"].ctypes.data and mk[0]["desc"].dtype == np.uint8


def test_small_vectors_and_bounds(hvo, marshal):
    assert list(hvo._ll_params(None, 0.25, 1.0, 0.95).bounds) == [0.0, 1.0, 0.0, 1.0]                     # bounds4=None: the resident frame's own grid
    assert list(hvo._lp_params((1, 639, 2, 479), 0.25, 8, 40.0, 1.0, 100, 0.8, 0.5).bounds) == [1.0, 639.0, 2.0, 479.0]
    P, K, R, keep = hvo._kfs_args(0, [], None, 10.0, 100, True, 0.18, 8)
    assert list(P.bounds) == [0.0, 1.0, 0.0, 1.0]
    k = hvo.NlKeyframe(); marshal.vec(k.cam, (1, 2, 3, 4, 5, 6, 7), 4); marshal.vec(k.Tcw, np.arange(12).reshape(3, 4))
    assert list(k.cam) == [1, 2, 3, 4, 0, 0] and list(k.Tcw) == list(range(12))
    with pytest.raises(ValueError):
        marshal.vec(k.Tcw, np.arange(11))


def test_return_path(marshal):
    seen = []
    def chk(rc, what):
        if rc: raise RuntimeError("%s %d" % (what, rc))
    finish = lambda ok: seen.append(ok) or ("res", ok)
    assert marshal.returned(0, lambda: b"", "call", chk, finish) == ("res", True)
    with pytest.raises(RuntimeError, match="call -4"):
        marshal.returned(-4, lambda: b"why", "call", chk, finish)
    assert marshal.returned(-4, lambda: b"why", "call", chk, finish, check=False) == (-4, "why", "res", False)          # a tuple result is spliced in
    assert marshal.returned(0, lambda: b"", "call", chk, lambda ok: [ok], check=False) == (0, "", [True]) and seen == [True, False]


# ---------------------------------------------------------------------------------------------------------------- the quirks
def test_kf_search_cuts_after_a_refusal_and_fuse_does_not(hvo, calls):
    T = np.eye(4)[:3]
    cand = dict(pos=np.zeros((3, 3)), skip=np.zeros(3), max_dist=np.ones(3), min_dist=np.ones(3), desc=np.zeros((3, 32)), angle=None, Tcw=T, occupied=np.zeros(5))
    empty = dict(pos=np.zeros((0, 3)), skip=[], max_dist=[], min_dist=[], desc=np.zeros((0, 32)), Tcw=T)
    P, K, R, keep = calls._kfs_args(5, [cand, empty], None, 10.0, 100, True, 0.18, 8)
    assert (K[0].n, K[1].n) == (3, 0) and K[0].angle is None and K[0].occupied == keep[0][0]["occupied"].ctypes.data
    assert all(getattr(K[1], k) is None for k in ("pos", "skip", "max_dist", "min_dist", "desc"))            # n == 0: NULL for all five required arrays
    assert R[0].status == R[0].n_matches == hvo.KF_UNTOUCHED
    r = calls._kfs_finish(R, keep)                                           # (the call was never made: this is what a refusal leaves)
    assert len(r[0]["match_idx"]) == 3 and len(r[0]["feature_kf"]) == 5 and len(r[1]["match_idx"]) == 0 and (r[0]["proj"] == hvo.KF_UNTOUCHED).all()
    K, M, sl, per_kf, R, finish, _ = calls._FUSE.build([dict(kp_un=np.zeros(2, hvo.KEYPOINT_DT), desc=np.zeros((2, 32)), Tcw=T)],
                                                       dict(pos=np.zeros((0, 3)), normal=np.zeros((0, 3)), max_dist=[], min_dist=[], desc=np.zeros((0, 32))))
    assert not per_kf and sl is None and M[0].n == 0 and M[0].pos is None
    assert len(finish(False)[0]["best_idx"]) == 1 and len(finish(False)[0]["fused_entry"]) == 1 and len(finish(True)[0]["best_idx"]) == 0
    K, R, S, P, fin, _ = calls._np_args(4, [dict(Tcw=T)], 50, 8, 1.2, 40.0)
    res, summary = fin(2)(False)
    assert len(res[0]["x3d"]) == 4 and len(summary["owner"]) == 4 and len(fin(2)(True)[0][0]["x3d"]) == 2 and summary["n_new"] == hvo.NP_UNTOUCHED


def test_missing_arrays_with_a_count_reach_the_library(hvo, calls):
    T = np.eye(4)[:3]
    K, keep = hvo._lf_keyframes([dict(kl=None, n=16, desc_rows=None, n_desc_rows=16, Tcw=T, cam=(500, 500, 320, 240), bounds=(0, 640, 0, 480), skip=None)], [0])
    assert K[0].n == 16 and K[0].kl is None and K[0].n_desc_rows == 16 and K[0].desc_rows is None and K[0].skip is None
    assert list(K[0].bounds) == [0, 640, 0, 480] and (K[0].fx, K[0].cy) == (500, 240)
    K, keep = hvo._lf_keyframes([dict(kl=np.zeros(3, hvo.KEYLINE_DT), desc_rows=np.zeros((5, 32)), Tcw=T, cam=(1, 1, 1, 1), bounds=(0, 1, 0, 1))], [0])
    assert K[0].n == 3 and K[0].n_desc_rows == 5
    K, keep = hvo._lf_keyframes([dict(Tcw=T, skip=[1, 1])], [2], resident=True)
    assert K[0].n == 0 and K[0].skip == keep[0]["skip"].ctypes.data
    k = hvo.NpKeyframe(); calls._np_keyframe(k, dict(n=7, Tcw=T, mb=0.08, skip=True))
    assert k.n == 7 and k.kp_un is None and k.desc is None and k.skip == 1 and abs(k.mb - 0.08) < 1e-7
    k = hvo.NpKeyframe(); a = calls._np_keyframe(k, dict(kp_un=np.zeros(4, hvo.KEYPOINT_DT), has_map_point=[3, 0, 0, 1], Tcw=T))
    assert k.n == 4 and a["has_map_point"].tolist() == [1, 0, 0, 1] and k.uright is None
    k = hvo.NlKeyframe(); calls._nl_keyframe(k, dict(n=9, Tcw=T, cam=(1, 2, 3, 4)))
    assert k.n == 9 and k.kl is None and list(k.cam)[:4] == [1, 2, 3, 4] and k.median_depth == 1.0


def test_local_map_io(hvo):
    io, a = hvo._lp_io(4, 10, [7, 8, 9, 3], [5, 6])
    assert a["held"].tolist() == [7, 8, 9, 3] and io.n_kp == 4 and io.n_seen_extra == 2 and io.seen_extra == a["seen_extra"].ctypes.data
    assert a["proj"].shape == (10, 3) and (a["match_dist"] == 256).all() and (a["match_idx"] == -1).all() and not a["in_view_slot"].any()
    io, a = hvo._ll_io(0, 0, None, None, True)
    assert a["held"].tolist() == [-1] and io.seen_extra is None and a["proj"].shape == (1, 4) and a["rel_map"].shape == (1,) and io.rel_map == a["rel_map"].ctypes.data
    assert hvo._ll_io(3, 1 << 20, None, None, False)[1]["in_view_slot"].shape == (hvo.LINE_MAP_MAX_QUERIES,) and hvo._ll_io(3, 5, None, None, False)[0].rel_map is None
    with pytest.raises(ValueError, match=r"^held must have one entry per key line \(4\)$"):
        hvo._ll_io(4, 10, [1, 2], None, False)
    with pytest.raises(ValueError, match=r"^held must have one entry per key point \(4\)$"):
        hvo._lp_io(4, 10, [1, 2, 3, 4, 5], None)


def test_new_keyframe_io_starts_held_at_minus_one(hvo):
    p, io, a = hvo._kfi_args(3, 2, hvo.KFI_KEYFRAME, 3.0, 8, 1, 1.2, 1, None, 0.5, -1, -1, [4, 5, 6], None)
    assert a["held_points"].tolist() == [4, 5, 6] and a["held_lines"].tolist() == [-1, -1] and (a["pt_pos"] == hvo.KFI_UNTOUCHED).all()
    assert a["ln_rel"].shape == (2, 2) and (a["ln_rel"] == hvo.KFI_UNTOUCHED).all() and io.ln_rel == a["ln_rel"].ctypes.data and (io.n_kp, io.n_kl) == (3, 2)
    assert p.cos_perp == 0.5 and p.line_geometry == 1 and p.mode == hvo.KFI_KEYFRAME


def test_pnp_results(hvo, calls):
    P = hvo.pnp_params(max_events=3)
    R, keep = calls._pnp_results(2, [5, 0], P, True, spare_events=1)
    sent32 = np.frombuffer(bytes([hvo.PNP_SENTINEL] * 4), np.int32)[0]
    a = keep[0]
    assert R[0].cap_events == 4 and a["ev_inliers"].shape == (4, 5) and keep[1]["best_inliers"].shape == (1,) and (a["best_inliers"] == hvo.PNP_SENTINEL).all()
    assert (a["hyp_inliers"] == sent32).all() and a["hyp_sample"].shape[1] == P.min_set and R[0].hyp_sample == a["hyp_sample"].ctypes.data
    for e in range(4):                                                       # every event starts at -99 and is wired to its two inlier rows
        assert a["events"][e].iteration == -99 and a["events"][e].inliers == a["ev_inliers"][e].ctypes.data
        assert a["events"][e].hyp_inliers == a["ev_hyp_inliers"][e].ctypes.data
    assert calls._pnp_results(1, [5], P, False)[0][0].hyp_sample is None
    R[0].n_features = 5; R[0].best_iteration = 0
    out = calls._pnp_finish(R, keep, P.min_set)
    assert out[0]["raw"] is a and out[0]["best_inliers"].tolist() == [0] * 5 and out[0]["hyp_sample"].shape == (0, P.min_set) and out[0]["events"] == []
    R[0].best_iteration = 2
    assert calls._pnp_finish(R, keep, P.min_set)[0]["best_inliers"].tolist() == [hvo.PNP_SENTINEL] * 5


def test_bow_and_keyframe_db(hvo, calls):
    b, a = calls._bow_out(0)
    assert b.cap == 1 and a["fv_start"].shape == (2,) and a["word_id"].tolist() == [-1] and a["bow_value"].dtype == np.float64
    b, a = calls._bow_out(6); b.n_features = 4; b.n_words = 2; b.n_nodes = 3; b.n_valid = 4; b.computed = 1
    d = calls._bow_finish(b, a)
    assert [len(d[k]) for k in ("word_id", "node_id", "bow_word", "bow_value", "fv_node", "fv_start", "fv_index")] == [4, 4, 2, 2, 3, 4, 4]
    assert d["computed"] is True and d["n_short"] == 0 and d["word_id"].base is None
    k, keep = calls._bow_side(np.zeros((3, 32)), [1, 2, 3])
    assert k.n == 3 and keep["has_map_point"].tolist() == [1, 1, 1] and keep["angle"].tolist() == [0, 0, 0] and k.angle == keep["angle"].ctypes.data
    assert calls._bow_side(np.zeros((0, 32)), [])[0].desc is None
    P, R, a = calls._kfdb_args(4, hvo.KFDB_LOOP, 0.5, [1, 2], True)
    assert R.cap == 4 and R.slot_cap == 4 and P.n_connected == 2 and P.connected == a["connected"].ctypes.data and R.words == a["words"].ctypes.data
    R.n_candidates = 2; R.n_sharing = 9
    r = calls._kfdb_finish(R, a, 4, True)
    assert len(r["candidates"]) == 2 and r["n_sharing"] == 9 and len(r["score"]) == 4 and "candidate" not in r and r["candidates"].base is None
    P, R, a = calls._kfdb_args(0, hvo.KFDB_RELOC, 0.0, None, False)
    assert R.cap == 1 and R.slot_cap == 0 and P.connected is None and R.words is None and "words" not in a


# ---------------------------------------------------------------------------------------------------------------- signatures
# exports the binding never calls, so they have no signature of their own (none today: the table also keeps the signatures that tests and
# tools use through lib(), such as hvo_extract_batch)
NEVER_CALLED = {}


def test_signature_coverage(hvo):
    assert set(hvo.SIGNATURES) <= set(hvo.EXPORTS)
    need = [e for e in hvo.EXPORTS if e != "hvo_abi_version" and not e.startswith("hvo_debug_") and e not in NEVER_CALLED]
    assert [e for e in need if e not in hvo.SIGNATURES] == []
    assert not set(NEVER_CALLED) & set(hvo.SIGNATURES)
    assert all(k.startswith("hvo_debug_") and k not in hvo.EXPORTS for k in hvo.DEBUG_SIGNATURES)
    L = hvo.lib()
    for name, (restype, argtypes) in list(hvo.SIGNATURES.items()) + list(hvo.DEBUG_SIGNATURES.items()):
        f = getattr(L, name)
        assert f.restype is restype and list(f.argtypes) == list(argtypes), name


def test_no_call_sets_a_signature_and_no_size_is_asserted_by_hand(hvo):
    import os
    from conftest import PKG_DIR
    for f in ("__init__.py", "_marshal.py"):
        txt = open(os.path.join(PKG_DIR, f)).read()
        assert "assert C.sizeof" not in txt and ".itemsize ==" not in txt, f
        assert txt.count(".argtypes =") == txt.count(".restype =") == (1 if f == "__init__.py" else 0), f          # once, in lib()
