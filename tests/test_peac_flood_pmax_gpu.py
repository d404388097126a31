"""The one-wave plane flood runs in two forms side by side: frames with at most 16 coarse planes take the slim plane table
(k_peac_flood<64, 1, 16>), frames with more take the MAX_PLANES form.  One batch that mixes both, around the boundary, must match
the CPU oracle frame by frame and be byte-equal with HVO_FLOOD_SLIM=0 (every frame through the MAX_PLANES form)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def grid_depth(nplanes, seed, rows=7, cols=7, w=640, h=480):
    """the first `nplanes` cells of a rows x cols grid (~91 x 68 px each) are tilted planar patches at depths that step from cell
    to cell; the other cells have no depth.  Every patch holds well over MIN_SUPPORT pixels of whole 10x10 blocks."""
    rng = np.random.default_rng(seed)
    j = (np.arange(w)[None, :] - 320.1) / 535.4; i = (np.arange(h)[:, None] - 247.6) / 539.2
    d = np.zeros((h, w), np.int64)
    ys = np.linspace(0, h, rows + 1).astype(int); xs = np.linspace(0, w, cols + 1).astype(int)
    for k in range(nplanes):
        r, c = divmod(k, cols)
        a, b = rng.uniform(-0.6, 0.6, 2); z0 = 1.5 + 0.8 * ((r + c) % 3) + rng.uniform(0, 0.2)
        z = z0 / (a * j + b * i + 1.0)
        d[ys[r]:ys[r + 1], xs[c]:xs[c + 1]] = np.rint(z * 5000)[ys[r]:ys[r + 1], xs[c]:xs[c + 1]]
    return d.clip(0, 65535).astype(np.uint16)


def run_batch(hvo, depth):
    ctx = hvo.Context(max_batch=len(depth))
    try:
        ctx.batch_upload(np.zeros(depth.shape, np.uint8), depth)
        ctx.batch_run(hvo.STAGE_PLANES)
        res = ctx.batch_download(hvo.STAGE_PLANES)
        stats = [ctx.peac_stats(f) for f in range(len(depth))]
        rep = ctx.launch_report()["peac"]
    finally:
        ctx.close()
    return res, stats, rep


def test_flood_slim_and_full_forms_in_one_batch(hvo, orc, synth, monkeypatch):
    monkeypatch.setenv("HVO_FLOOD_T", "64")
    kinds = [("synth", 0x5EED0002), ("grid", 5), ("grid", 16), ("synth", 0x5EED1000), ("grid", 17), ("grid", 49), ("grid", 16), ("synth", 77)]
    depth = np.stack([synth.make_depth(s) if k == "synth" else grid_depth(s, 7 + f) for f, (k, s) in enumerate(kinds)])
    monkeypatch.delenv("HVO_FLOOD_SLIM", raising=False)
    res, stats, rep = run_batch(hvo, depth)
    monkeypatch.setenv("HVO_FLOOD_SLIM", "0")
    res_full, stats_full, rep_full = run_batch(hvo, depth)
    # the slim first launch ran in the first batch and not in the second; both took the one-wave flood
    assert (rep["flood_t"], rep["flood_epl"], rep["flood_slim"]) == (64, 1, 1) and (rep_full["flood_t"], rep_full["flood_epl"], rep_full["flood_slim"]) == (64, 1, 0), (rep, rep_full)
    for f, (k, s) in enumerate(kinds):
        lo, po = orc.peac(depth[f])
        r = res[f]
        assert r["status"] == 0, (f, r["status"])
        assert len(r["planes"]) == len(po), (f, len(r["planes"]), len(po))
        assert np.array_equal(r["planes"]["n_points"], po["n_points"]) and np.array_equal(r["planes"]["rid"], po["rid"]), f
        for fld in ("normal", "center", "mse"):
            assert np.allclose(r["planes"][fld], po[fld], rtol=1e-9, atol=1e-12), (f, fld)
        assert np.array_equal(r["labels"], lo), (f, int((r["labels"] != lo).sum()))
        # the two forms: the same bytes and the same flood (rounds, ranked and serial replays)
        assert r["labels"].tobytes() == res_full[f]["labels"].tobytes(), f
        assert r["planes"].tobytes() == res_full[f]["planes"].tobytes(), f
        assert stats[f] == stats_full[f], (f, stats[f], stats_full[f])
        assert stats[f]["flags"] == 0, (f, stats[f])
        if k == "grid":
            assert len(po) == s, (f, len(po), s)
    cp = [st["coarse_planes"] for st in stats]
    assert cp[2] == 16 and cp[6] == 16 and cp[4] == 17, cp      # both sides of the boundary
    assert cp[5] > 40, cp                                       # the MAX_PLANES form took this frame
    assert cp[1] <= 16, cp
