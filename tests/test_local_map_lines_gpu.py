"""The local-map line search on the GPU, LSDmatcher::SearchByProjection(F, vpMapLines, eval_orient, th) (reference src/LSDmatcher.cpp:709-801;
k_lsbp_map_keys + k_lsbp_map_epilogue), host-array form and the form on a resident frame of a stream, bit-exact (match_idx, match_dist,
n_matches) against the CPU restatement tests/local_map_lines_ref.py."""
import numpy as np
import pytest

import local_map_lines_ref as ref

pytestmark = pytest.mark.gpu


def shifted_queries(kl, shift, jitter_seed=0):
    """a frame's lines projected into the next one: the sequence's known image-plane drift plus a sub-pixel jitter"""
    rng = np.random.RandomState(jitter_seed)
    j = (rng.rand(len(kl), 4).astype(np.float32) - np.float32(0.5)) * np.float32(1.5)
    q = np.stack([kl["sx"] - np.float32(shift[0]), kl["sy"] - np.float32(shift[1]), kl["ex"] - np.float32(shift[0]), kl["ey"] - np.float32(shift[1])], axis=1).astype(np.float32)
    return (q + j).astype(np.float32)


def rotate(v, deg, axis):
    """v rotated by deg about a unit axis (Rodrigues), rows of v"""
    a = np.radians(deg); k = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    return v * np.cos(a) + np.cross(k, v) * np.sin(a) + np.outer(v @ k, k) * (1 - np.cos(a))


VC_BELOW = np.nextafter(np.float32(0.998), np.float32(0.0))


def map_queries(kl_a, l3d_a, d_a, shift, seed):
    """queries for frame a's lines seen from frame b: world vectors true, rotated by 10 and 20 degrees, and zero; viewing cosines on both sides
    of 0.998; a few repeated queries at the end"""
    n = len(kl_a)
    q = shifted_queries(kl_a, shift, jitter_seed=seed)
    w = (l3d_a["A"] - l3d_a["B"]).astype(np.float64)
    kind = np.arange(n) % 4
    w[kind == 1] = rotate(w[kind == 1], 10.0, (0.3, -0.5, 0.8))
    w[kind == 2] = rotate(w[kind == 2], 20.0, (0.3, -0.5, 0.8))
    w[kind == 3] = 0.0
    vc = np.choose(np.arange(n) % 4, [np.float32(0.998), VC_BELOW, np.float32(0.5), np.float32(1.0)]).astype(np.float32)
    rep = np.arange(0, n, 5)
    return (np.concatenate([q, q[rep]]), np.concatenate([vc, vc[rep]]), np.concatenate([w, w[rep]]), np.concatenate([d_a, d_a[rep]]))


def check(ctx, q, vc, w, qd, blocks, kl, fn, l3d, dt, occ, cs, ci, b4, th, nn_ratio=0.95):
    n, mi, md = ctx.search_lines_by_projection_map(q, vc, w, qd, blocks, kl, fn, l3d, dt, occ, cs, ci, b4, th=th, nn_ratio=nn_ratio)
    no, mio, mdo = ref.search_lines_by_projection_map(q, vc, w, qd, blocks, kl, fn, l3d, dt, occ, cs, ci, b4, th, nn_ratio)
    assert n == no and np.array_equal(mi, mio) and np.array_equal(md, mdo), (th, n, no, np.nonzero(mi != mio)[0][:8])
    return no, mio


def frames(hvo, synth, seed, n, w, h, nfeat):
    g, d, off = synth.make_sequence("std", seed, n, w=w, h=h)
    kw = dict(fx=535.4 * w / 640, fy=539.2 * h / 480, cx=320.1 * w / 640, cy=247.6 * h / 480) if w != 640 else {}
    ctx = hvo.Context(lsd_nfeatures=nfeat, **kw)
    b4 = np.array([0.0, w, 0.0, h], np.float32)
    fr = []
    for k in range(n):
        kl, ld, fn = ctx.extract_lsd(g[k])
        fr.append((kl, ld, fn, ctx.lines_3d(kl, d[k], seed=3 + k)))
    return ctx, g, d, off, fr, b4


@pytest.mark.parametrize("w,h,nfeat", [(640, 480, 200), (1280, 960, 2000)])
def test_host_arrays_on_a_sequence(hvo, synth, w, h, nfeat):
    ctx, g, d, off, fr, b4 = frames(hvo, synth, 0x5EED6500 + w, 3, w, h, nfeat)
    try:
        for a, b in ((0, 1), (1, 2)):
            kla, lda, _, l3a = fr[a]; klt, dt, fnt, l3t = fr[b]
            assert len(klt) <= 2048 and (l3t["good"] == 1).sum() > 10
            cs, ci = ctx.assign_lines_to_grid(klt, b4)
            q, vc, wv, qd = map_queries(kla, l3a, lda, (off[b] - off[a]).astype(np.float32), a * 7 + b)
            nq = len(q)
            blocks = (np.arange(nq) % 3 != 0).astype(np.uint8); occ = (np.arange(len(klt)) % 11 == 0).astype(np.uint8)
            for th in (1.0, 5.0):
                no, _ = check(ctx, q, vc, wv, qd, blocks, klt, fnt, l3t, dt, occ, cs, ci, b4, th)
                assert no > 10, (a, b, th)
            check(ctx, q, vc, wv, qd, None, klt, fnt, l3t, dt, None, cs, ci, b4, 5.0)
            check(ctx, q, vc, wv, qd, np.ones(nq, np.uint8), klt, fnt, l3t, dt, occ, cs, ci, b4, 5.0)
    finally:
        ctx.close()


def test_tie_heavy_pool_and_the_ratio_rule(hvo, synth):
    """descriptors from a pool of four (two at distance 1), current-line octaves set by hand: equal distances everywhere, so the visit order,
    the ratio rule's same-octave rejection and its different-octave pass all decide"""
    ctx, g, d, off, fr, b4 = frames(hvo, synth, 0x5EED6600, 2, 640, 480, 200)
    try:
        kla, _, _, l3a = fr[0]; klt, _, fnt, l3t = fr[1]
        klt = klt.copy(); klt["octave"] = (np.arange(len(klt)) // 2) % 2
        pool = np.random.RandomState(9).randint(0, 256, (4, 32)).astype(np.uint8)
        pool[1] = pool[0]; pool[1, 0] ^= 1
        qd0 = pool[np.arange(len(kla)) % 4]; dt = pool[(np.arange(len(klt)) * 3) % 4].copy()
        cs, ci = ctx.assign_lines_to_grid(klt, b4)
        q, vc, wv, qd = map_queries(kla, l3a, qd0, (off[1] - off[0]).astype(np.float32), 4)
        wv[:] = 0.0                                                           # every 3-D gate passes (NaN): the window alone decides
        nq = len(q)
        for blocks in (np.ones(nq, np.uint8), np.zeros(nq, np.uint8), (np.arange(nq) % 2).astype(np.uint8)):
            for nn in (0.95, 1.0):
                check(ctx, q, vc, wv, qd, blocks, klt, fnt, l3t, dt, None, cs, ci, b4, 5.0, nn_ratio=nn)
        n95 = ref.search_lines_by_projection_map(q, vc, wv, qd, None, klt, fnt, l3t, dt, None, cs, ci, b4, 5.0, 0.95)[0]
        n100 = ref.search_lines_by_projection_map(q, vc, wv, qd, None, klt, fnt, l3t, dt, None, cs, ci, b4, 5.0, 1.0)[0]
        assert 10 < n95 < n100                                                 # both branches of the rule fire
    finally:
        ctx.close()


def test_edges_and_limits(hvo, synth):
    ctx, g, d, off, fr, b4 = frames(hvo, synth, 0x5EED6700, 2, 640, 480, 200)
    try:
        kla, lda, _, l3a = fr[0]; klt, dt, fnt, l3t = fr[1]
        cs, ci = ctx.assign_lines_to_grid(klt, b4)
        q, vc, wv, qd = map_queries(kla, l3a, lda, (off[1] - off[0]).astype(np.float32), 1)
        nq = len(q)
        # nq = 0, nt = 0, nt = 1, every line occupied
        n, mi, md = ctx.search_lines_by_projection_map(q[:0], vc[:0], wv[:0], qd[:0], None, klt, fnt, l3t, dt, None, cs, ci, b4)
        assert n == 0 and len(mi) == 0
        cs0, ci0 = np.zeros(64 * 48 + 1, np.int32), np.zeros(0, np.int32)
        n, mi, md = ctx.search_lines_by_projection_map(q, vc, wv, qd, None, klt[:0], fnt[:0], l3t[:0], dt[:0], None, cs0, ci0, b4, th=5.0)
        assert n == 0 and np.all(mi == -1) and np.all(md == 256)
        for j in (0, 7):
            k1 = klt[j:j + 1]; cs1, ci1 = ctx.assign_lines_to_grid(k1, b4)
            check(ctx, q, vc, wv, qd, None, k1, fnt[j:j + 1], l3t[j:j + 1], dt[j:j + 1], None, cs1, ci1, b4, 5.0)
        n, mi, _ = ctx.search_lines_by_projection_map(q, vc, wv, qd, None, klt, fnt, l3t, dt, np.ones(len(klt), np.uint8), cs, ci, b4, th=5.0)
        assert n == 0 and np.all(mi == -1)
        # 8192 queries in one call (the sequence's queries over and over, mixed claims)
        rep = -(-8192 // nq); idx = np.tile(np.arange(nq), rep)[:8192]
        blocks = (np.arange(8192) % 5 == 0).astype(np.uint8)
        check(ctx, q[idx], vc[idx], wv[idx], qd[idx], blocks, klt, fnt, l3t, dt, None, cs, ci, b4, 1.0)
        # more than 2048 current lines: refused, with the reason
        big = np.tile(np.arange(len(klt)), -(-2049 // len(klt)))[:2049]
        csb, cib = ctx.assign_lines_to_grid(klt[big], b4)
        with pytest.raises(hvo.HvoError, match="2048"):
            ctx.search_lines_by_projection_map(q, vc, wv, qd, None, klt[big], fnt[big], l3t[big], dt[big], None, csb, cib, b4)
        with pytest.raises(hvo.HvoError, match="16384"):
            z = np.zeros(16385, np.int64)
            ctx.search_lines_by_projection_map(q[z], vc[z], wv[z], qd[z], None, klt, fnt, l3t, dt, None, cs, ci, b4)
    finally:
        ctx.close()


@pytest.mark.parametrize("w,h", [(640, 480), (1280, 960)])
def test_stream_form_on_resident_frames(hvo, synth, w, h):
    n = 3
    g, d, off = synth.make_sequence("std", 0x5EED6800, n, w=w, h=h)
    kw = dict(fx=535.4 * w / 640, fy=539.2 * h / 480, cx=320.1 * w / 640, cy=247.6 * h / 480) if w != 640 else {}
    st = hvo.Stream(depth=4, stages=hvo.STAGE_LSD | hvo.STAGE_LSD_CULL | hvo.STAGE_ORB | hvo.STAGE_GRIDS | hvo.STAGE_LINES3D, bf=0.0, width=w, height=h, **kw)
    ctx = hvo.Context()
    try:
        b4 = np.array(st.bounds, np.float32)
        t = [st.submit(g[k], d[k]) for k in range(n)]
        r = [st.collect(x) for x in t]
        for a, b in ((0, 1), (1, 2)):
            kla, lda, l3a = r[a]["kl"], r[a]["ldesc"], r[a]["lines3d"]
            klt, dt, fnt, l3t = r[b]["kl"], r[b]["ldesc"], r[b]["linefn"], r[b]["lines3d"]
            cs, ci = r[b]["ln_grid"]
            q, vc, wv, qd = map_queries(kla, l3a, lda, (off[b] - off[a]).astype(np.float32), 3 * a + b)
            nq = len(q)
            blocks = (np.arange(nq) % 3 != 1).astype(np.uint8); occ = (np.arange(len(klt)) % 9 == 0).astype(np.uint8)
            for th in (1.0, 5.0):
                ns, mi, md = st.search_lines_by_projection_map(t[b], q, vc, wv, qd, q_blocks=blocks, t_occupied=occ, th=th)
                nh, mih, mdh = ctx.search_lines_by_projection_map(q, vc, wv, qd, blocks, klt, fnt, l3t, dt, occ, cs, ci, b4, th=th)
                no, mio, mdo = ref.search_lines_by_projection_map(q, vc, wv, qd, blocks, klt, fnt, l3t, dt, occ, cs, ci, b4, th, 0.95)
                assert ns == nh == no and np.array_equal(mi, mih) and np.array_equal(mi, mio) and np.array_equal(md, mdh) and np.array_equal(md, mdo), (a, b, th)
            assert no > 10
            ns, mi, md = st.search_lines_by_projection_map(t[b], q[:0], vc[:0], wv[:0], qd[:0])
            assert ns == 0 and len(mi) == 0
    finally:
        ctx.close(); st.close()


def test_stream_form_needs_lines3d(hvo, synth):
    g, d, off = synth.make_sequence("std", 0x5EED6900, 1)
    st = hvo.Stream(depth=2, stages=hvo.STAGE_LSD | hvo.STAGE_ORB | hvo.STAGE_GRIDS, bf=0.0)
    try:
        t = st.submit(g[0], d[0]); st.collect(t)
        q = np.array([[100, 100, 200, 100]], np.float32)
        with pytest.raises(hvo.HvoError, match="LINES3D"):
            st.search_lines_by_projection_map(t, q, np.ones(1, np.float32), np.ones((1, 3)), np.zeros((1, 32), np.uint8))
    finally:
        st.close()
