"""LSDmatcher::Fuse on the CPU: the exports and the Python methods exist, and tests/line_fuse_ref.py (the restatement the device is compared
with in tests/test_line_fuse_gpu.py) gives the known answers on every hand-built case.  The random scene of the device test is shown here
not to be vacuous, on the restatement alone, so the device comparison cannot pass on an empty result."""
import ctypes
import os

import numpy as np
import pytest

import line_fuse_ref as ref
from conftest import PKG_DIR


def test_exports_and_methods_exist(hvo):
    lib = ctypes.CDLL(os.path.join(PKG_DIR, "csrc", "libhvo.so"))
    for name in ("hvo_fuse_lines", "hvo_fuse_lines_slots", "hvo_stream_fuse_lines"):
        assert hasattr(lib, name), name
    assert lib.hvo_abi_version() == 3
    for cls, name in ((hvo.Context, "fuse_lines"), (hvo.Context, "fuse_lines_slots"), (hvo.Stream, "fuse_lines")):
        assert callable(getattr(cls, name, None)), (cls.__name__, name)
    assert hvo.LF_GATES == ref.GATES and hvo.LF_LEVEL_RULES == (ref.CLAMPED, ref.AS_WRITTEN)
    assert (hvo.LF_MAX_LINES, hvo.LF_MAX_ENTRIES) == (ref.MAX_LINES, ref.MAX_ENTRIES)


def test_crafted_gates_say_what_they_are_meant_to(hvo):
    kf, mp, want, names = ref.crafted_gates(hvo.KEYLINE_DT)
    w = ref.fuse(kf, mp)
    for name, a, b in zip(names, want, w["gate"]):
        assert a == b, (name, ref.GATES[a], ref.GATES[b])
    assert set(want) == set(range(7))                                  # every code but LEVEL (test_crafted_levels)
    p = dict(zip(names, w["proj"]))
    assert (p["skipped"] == 0).all() and (p["start behind only"] == 0).all() and (p["end behind only"] == 0).all()
    assert p["u1 on max, u2 in"].tolist() == [640.0, 200.0, 0.0, 0.0]   # IsInImage(u1, v1) fails before u2, v2 exist
    assert p["u1 in, u2 on max"].tolist() == [600.0, 200.0, 640.0, 200.0]
    assert p["u1 just below max, u2 in"][0] == np.nextafter(np.float32(640), np.float32(0))
    assert np.isnan(p["start at z = 0: NaN or inf fails IsInImage"][0])
    assert w["behind_entry"].tolist() == [names.index(n) for n in ("start behind only", "end behind only", "both behind")] and w["n_behind"] == 3
    assert w["n_searched"] == want.count(0) and (w["level"][np.array(want) != 0] == -1).all()


@pytest.mark.parametrize("n_levels", [1, 3])
def test_crafted_levels(hvo, n_levels):
    kf, mp, lv = ref.crafted_levels(hvo.KEYLINE_DT, n_levels)
    c = ref.fuse(kf, mp, log_scale_factor=ref.LOG_11, n_levels=n_levels, level_rule=ref.CLAMPED)
    a = ref.fuse(kf, mp, log_scale_factor=ref.LOG_11, n_levels=n_levels, level_rule=ref.AS_WRITTEN)
    assert (c["gate"] == 0).all() and c["level"].tolist() == [min(max(l, 0), n_levels - 1) for l in lv]
    assert a["level"].tolist() == lv and a["gate"].tolist() == [0 if 0 <= l < n_levels else ref.LEVEL for l in lv]
    assert (c["best_idx"] >= 0).all() and (a["best_idx"][a["gate"] == ref.LEVEL] == -1).all()
    assert a["n_searched"] == sum(0 <= l < n_levels for l in lv)


@pytest.mark.parametrize("n_levels", [1, 3])
def test_crafted_searches(hvo, n_levels):
    kf, mp, bi, bd, names = ref.crafted_search(hvo.KEYLINE_DT, n_levels)
    assert len(kf["kl"]) == 300
    w = ref.fuse(kf, mp, n_levels=n_levels)
    assert (w["gate"] == 0).all()
    for k, name in enumerate(names):
        assert (w["best_idx"][k], w["best_dist"][k]) == (bi[k], bd[k]), (name, w["best_idx"][k], w["best_dist"][k], bi[k], bd[k])
    assert w["fused_entry"].tolist() == [k for k in range(len(names)) if bd[k] <= 50]
    assert w["n_ties"][names.index("equal distances: the lower index")] == 2 and w["n_ties"][names.index("equal distances across the chunk boundary")] == 2
    dy_in, dy_out = ref.cos_pair()
    assert np.nextafter(dy_in, np.float32(np.inf)) == dy_out


def test_short_rows(hvo):
    kf, mp, bi, bd = ref.short_rows(hvo.KEYLINE_DT)
    w = ref.fuse(kf, mp)
    assert w["best_idx"].tolist() == bi.tolist() and w["best_dist"].tolist() == bd.tolist()
    full = ref.fuse(dict(kf, desc_rows=np.concatenate([kf["desc_rows"], np.stack([ref.flip(5), ref.flip(1), ref.flip(9)])])), mp)
    assert full["best_idx"].tolist() == [5, 6] and full["best_dist"].tolist() == [1, 9]          # with every row present the lines past row 4 win


@pytest.mark.parametrize("level_rule", [ref.CLAMPED, ref.AS_WRITTEN])
def test_the_random_scene_is_not_vacuous(hvo, level_rule):
    kfs, mp = ref.random_scene(hvo.KEYLINE_DT)
    assert (len(kfs), len(kfs[0]["kl"]), len(mp["pos"])) == (3, 120, 150)
    ws = [ref.fuse(kf, mp, level_rule=level_rule) for kf in kfs]
    ref.scene_vacuity(ws, 150, level_rule)
    assert all(w["n_behind"] > 0 and w["n_fused"] > 0 for w in ws)


def test_the_walk(hvo):
    """stop_on_behind ends a key frame's walk at the first behind entry that is still not skipped; `false` continues"""
    res = dict(fused_entry=np.array([1, 4, 9]), fused_idx=np.array([7, 8, 9]), behind_entry=np.array([3, 6]))
    seen = []
    out = ref.walk(res, lambda e: False, lambda e, i: seen.append((e, i)) or False)
    assert seen == [(1, 7)] and out == dict(n_fused=1, stopped_at=3, replaced=False)
    seen = []
    out = ref.walk(res, lambda e: e == 3, lambda e, i: seen.append((e, i)) or e == 4)            # entry 3 was replaced away: the stop moves to 6
    assert seen == [(1, 7), (4, 8)] and out == dict(n_fused=2, stopped_at=6, replaced=True)
    seen = []
    out = ref.walk(res, lambda e: False, lambda e, i: seen.append((e, i)) or False, stop_on_behind=False)
    assert seen == [(1, 7), (4, 8), (9, 9)] and out == dict(n_fused=3, stopped_at=-1, replaced=False)
