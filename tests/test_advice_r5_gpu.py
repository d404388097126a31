"""Regression tests for the round-5 code-review findings: the LDS order between the flood's hash clear and a ranked round's
publish, the label range of the slot AHC, the async line growing's fall-back under the split preamble with chunks, the async report
after a launch that was not async, and the messages of refused calls."""
import numpy as np
import pytest

from test_lsd_gpu import check as check_lines
from test_peac_gpu import check as check_planes, corner_depth, polyhedron_depth

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("delay", [None, "16"])
@pytest.mark.parametrize("flood_t", [128, 256, 512])
def test_flood_ranked_round_publishes_after_every_wave_cleared(hvo, orc, monkeypatch, flood_t, delay):
    """k_peac_flood with several waves: every wave clears its own hash slots, then a ranked round publishes the events' distances into
    the same table by compact event index.  A wave that clears late overwrote a distance another wave had already published.
    HVO_FLOOD_DELAY (a test hook) makes wave 0 sleep before its clear in the ranked rounds, which widens that window; labels and planes
    must still be the sequential loop's, and the scenes must have had ranked rounds at all."""
    monkeypatch.setenv("HVO_FLOOD_T", str(flood_t))
    if delay: monkeypatch.setenv("HVO_FLOOD_DELAY", delay)
    scenes = [corner_depth(3, 25, cu=323.0, cv=236.0), corner_depth(4, 60, cu=317.5, cv=243.5), polyhedron_depth(101), polyhedron_depth(107)]
    ctx = hvo.Context()
    try:
        ranked = 0
        for d in scenes:
            lo, po = orc.peac(d)
            lg, pg = ctx.compute_planes(d)
            check_planes(lg, pg, lo, po)
            st = ctx.peac_stats(0)
            assert st["flags"] == 0
            ranked += st["flood_ranked_rounds"]
        assert ranked > 0
    finally:
        ctx.close()


@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("w,h", [(1920, 1080), (1600, 1020)])
def test_slot_ahc_only_while_labels_fit_16_bits(hvo, orc, synth, monkeypatch, w, h, compact):
    """k_peac_cluster_slots packs a label into a signed 16-bit half; labels run up to segcap - 1 = 2 * nblk + 127.  1920x1080 (20 736
    blocks) creates more than 32 767 labels: it must take the four-frames-per-wave kernel without slots.  1600x1020 (16 320 blocks,
    segcap exactly 32 768) is the largest frame the slot form keeps.  Both also with a list pool small enough to be compacted (the
    second launch site)."""
    monkeypatch.setenv("HVO_PEAC_GL", "16")
    nblk = (w // 10) * (h // 10)
    if compact: monkeypatch.setenv("HVO_PEAC_POOLCAP", str(int(7.2 * nblk)))
    d = synth.make_depth(0x5EED5300, w, h)
    K = synth.intrinsics(w, h)
    lo, po = orc.peac(d, fx=np.float32(K["fx"]), fy=np.float32(K["fy"]), cx=np.float32(K["cx"]), cy=np.float32(K["cy"]))
    ctx = hvo.Context(fx=K["fx"], fy=K["fy"], cx=K["cx"], cy=K["cy"])
    try:
        lg, pg = ctx.compute_planes(d)
        st = ctx.peac_stats(0)
    finally:
        ctx.close()
    assert len(po) >= 3
    check_planes(lg, pg, lo, po)
    assert st["flags"] == 0, st
    if w == 1920: assert st["segments"] > 32768, st           # the old guard (nblk < 32768) let these labels go negative
    else: assert 2 * nblk + 128 == 32768


def test_split_preamble_chunked_batch_declines_async_growing(hvo, orc, synth, monkeypatch):
    """HVO_LSD_PRE_SPLIT=1 keeps the fp64 blurred images of one chunk only.  The async growing's fall-back forms its frames again from
    them, so with more frames than a chunk it would read past them: such a batch is grown by the one-wave kernel.  With no more frames
    than a chunk the fall-back is valid and runs (HVO_LSD_ASYNC_SPIN_MAX=0 makes every wait expire)."""
    for k, v in (("HVO_LSD_PRE_SPLIT", "1"), ("HVO_LSD_CHUNK", "2"), ("HVO_LSD_ASYNC", "8"), ("HVO_LSD_ASYNC_SPIN_MAX", "0")):
        monkeypatch.setenv(k, v)
    g = np.stack([synth.make_gray("std" if k != 1 else "lowtex", 0x5EED5400 + k) for k in range(5)])
    ref = [orc.line_extract(g[b]) for b in range(5)]
    ctx = hvo.Context(max_batch=5)
    try:
        ctx.batch_upload(g, np.zeros((5, 480, 640), np.uint16))
        ctx.batch_run(hvo.STAGE_LSD)
        res = ctx.batch_download(hvo.STAGE_LSD)
        assert ctx.lsd_async_report() == (0, 0, 0)                # async declined: 5 frames, chunks of 2
        for b in range(5):
            assert res[b]["status"] == 0
            check_lines(res[b]["kl"], res[b]["ldesc"], res[b]["linefn"], *ref[b])
        ctx.batch_upload(g[:2], np.zeros((2, 480, 640), np.uint16))
        regrown_total = 0
        for _ in range(2):
            ctx.batch_run(hvo.STAGE_LSD)
            res = ctx.batch_download(hvo.STAGE_LSD)
            regrown, foreign, wpf = ctx.lsd_async_report()
            assert wpf == 8 and 0 <= regrown <= 2
            regrown_total += regrown
            for b in range(2):
                assert res[b]["status"] == 0
                check_lines(res[b]["kl"], res[b]["ldesc"], res[b]["linefn"], *ref[b])
        assert regrown_total > 0                                   # the redo under the split preamble did run
    finally:
        ctx.close()


def test_async_report_describes_the_last_launch(hvo, synth, monkeypatch):
    """hvo_lsd_async_report after a launch that was not async: workers_per_frame = 0 and nothing else (include/hvo.h), and
    hvo_profile_last has no lsd_async rows -- not the figures of an earlier async batch of the same plan."""
    monkeypatch.delenv("HVO_LSD_ASYNC", raising=False)
    g = np.stack([synth.make_gray("std", 0x5EED5500 + k) for k in range(24)])
    ctx = hvo.Context(max_batch=24)
    try:
        ctx.profile_enable(1)
        ctx.batch_upload(g[:4], np.zeros((4, 480, 640), np.uint16))
        ctx.batch_run(hvo.STAGE_LSD)
        assert ctx.lsd_async_report()[2] == 32                     # four frames: grown async, 32 workers each
        assert any(k.startswith("lsd_async") for k in ctx.profile_last())
        ctx.batch_upload(g, np.zeros((24, 480, 640), np.uint16))  # same geometry, same plan; 24 frames are not grown async
        ctx.batch_run(hvo.STAGE_LSD)
        assert ctx.lsd_async_report() == (0, 0, 0)
        prof = ctx.profile_last()
        assert "lsd_grow" in prof and not any(k.startswith("lsd_async") for k in prof), prof
    finally:
        ctx.close()


def test_staging_depth_under_a_gray_only_batch_is_refused_with_a_message(hvo, orc, synth):
    """A resident batch without depth has no plane plan; staging a batch WITH depth would build one.  The call is refused
    (HVO_ERR_INVALID_ARG) with a message that names the way out, and the resident batch still gives its own results."""
    g, d = synth.make_batch("std", 0x5EED5600, 2)
    ctx = hvo.Context(max_batch=2)
    try:
        ctx.batch_upload(g)
        with pytest.raises(hvo.HvoError) as e:
            ctx.batch_stage_upload(g, d)
        assert e.value.status == -1 and "hvo_batch_upload" in str(e.value), str(e.value)
        ctx.batch_run(hvo.STAGE_ORB)
        res = ctx.batch_download(hvo.STAGE_ORB)
        o = orc.Orb()
        for k in range(2):
            assert res[k]["status"] == 0
            assert np.array_equal(res[k]["desc"], o.extract(g[k])[1]), k
    finally:
        ctx.close()
