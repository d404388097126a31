// peac_slots.inc -- k_peac_cluster_slots: ahCluster (include/peac/AHCPlaneFitter.hpp:983-1189) for four frames per wave, where a merge
// costs the SHORTER of the two neighbour lists.  (included by peac.hip, after peac_lend.inc whose helpers it uses)
//
// ah_cluster_lend gives the merged node a new record: every neighbour of p AND of its partner has its list edited (p -> new id, the partner
// dropped).  While a large plane grows that is 40-60 scattered list edits per iteration for a partner that has four neighbours -- pass A and
// its tail were a quarter of the kernel.  Here the node records are SLOTS: the merged node takes over the slot of whichever of the two has
// the longer list (K, "kept"), so the lists of K's neighbours still name it and are not touched; only the neighbours of the other one (D,
// "dropped") are visited: a common neighbour drops D from its list, the others get D -> K and join K's list, which is copied (contiguous:
// one round trip, no dependent chain) to the pool's top with the new members behind it.  Small-to-large: the edits of a merge are
// deg(D) <= min(deg p, deg partner).
//
// Ids.  The reference orders by creation id in three places -- the candidate rule's ties, the queue's ties, and the ids k_peac_final sees --
// so a slot carries the LABEL (creation id, nseg++) of the node that lives in it: in the upper half of HotNode::rid, and as (label << 16 | slot)
// in the queue's id words, which therefore order by label exactly as before while naming the slot.  Both halves are read back as SIGNED
// 16-bit numbers (rid >> 16): a label must stay below 2^15, or it turns negative, breaks the id order, collides with the -1 "no candidate"
// sentinel and reaches ext[] as a segment id.  Labels run up to segcap - 1 = 2 * nblk + 127, so peac_run launches this form only while
// segcap <= 32768 (nblk <= 16320; 1280x960 has 12 288 blocks) and gives larger frames to ah_cluster_lend.  Extracted planes
// are written to segD / segI under their labels, as k_peac_final expects.  The queue loses an update per merge (D leaves, K gets the new
// key and label: two slots instead of three ids) and half of its entries (slots < nblk).
//
// Evaluation, lending of idle lanes and the LDS exchange are ah_cluster_lend's; the tie rule is folded per pass into a running
// (min, smallest good label, largest label) so that the winner's state is always held by a lane of the pass that made it the winner.

struct SlDec { int p, K, D, code, moff, mB, r0, r1; };            // code: 1 merge, 2 no merge, 4 the kept slot is p's
struct __attribute__((aligned(16))) SlLds { double ps[4][16]; LendRed red[4]; LendWin win[4]; SlDec dec[4]; int ncnt[4]; };
#define SL_SLOT(x) ((x) & 0xFFFF)
#define SL_PACK(label, slot) (((label) << 16) | (slot))

static __device__ __forceinline__ void row_min16x2(double (&k)[2], int (&i)[2])
{
    double g[2] = { k[0], k[1] };
#pragma unroll
    for (int s_ = 0; s_ < 4; s_++) {
        double t[2];
#pragma unroll
        for (int n = 0; n < 2; n++) t[n] = dpp_f64(g[n], g[n], s_);
#pragma unroll
        for (int n = 0; n < 2; n++) g[n] = key_min(t[n], g[n]);
    }
    int c[2];
#pragma unroll
    for (int n = 0; n < 2; n++) c[n] = (k[n] == g[n]) ? i[n] : 0x7FFFFFFF;
#pragma unroll
    for (int s_ = 0; s_ < 4; s_++) {
#pragma unroll
        for (int n = 0; n < 2; n++) { const int t = dpp_i32(c[n], c[n], s_); c[n] = min(c[n], t); }
    }
#pragma unroll
    for (int n = 0; n < 2; n++) { k[n] = g[n]; i[n] = c[n]; }
}

// TQUpdate over slots: up to two slots change (x[0]: its key becomes +inf; x[1]: new key and new packed id); lq = packed id of every slot
struct TQUpdateS {
    double kk[2], mk[2], kn[2]; int li[2], mi[2], x[2], ln[2], nx;
    __device__ __forceinline__ void issue(const TQueue &Q, const int *lq, int rl, int nx_, int x0, double k0, int l0, int x1, double k1, int l1)
    {
        nx = nx_; x[0] = x0; x[1] = x1; kn[0] = k0; kn[1] = k1; ln[0] = l0; ln[1] = l1;
#pragma unroll
        for (int t = 0; t < 2; t++) {
            kk[t] = TQ_INF; mk[t] = TQ_INF; mi[t] = 0x7FFFFFFF; li[t] = 0x7FFFFFFF;
            if (t < nx) { const int s = (x[t] & ~15) + rl; kk[t] = Q.K[s]; li[t] = lq[s]; const int j = ((x[t] >> 8) << 4) + rl; mk[t] = Q.M1k[j]; mi[t] = Q.M1i[j]; }
        }
    }
    __device__ __forceinline__ int take(const TQueue &Q, int *lq, int rl, bool writer)
    {
#pragma unroll
        for (int t = 0; t < 2; t++) if (writer && t < nx) { Q.K[x[t]] = kn[t]; lq[x[t]] = ln[t]; }
        double bk[2]; int bi[2];
#pragma unroll
        for (int t = 0; t < 2; t++) {
            double k = kk[t]; int i = li[t];
#pragma unroll
            for (int u = 0; u < 2; u++) if (u < nx && ((x[u] ^ x[t]) >> 4) == 0 && (x[u] & 15) == rl) { k = kn[u]; i = ln[u]; }
            if (t >= nx) { k = TQ_INF; i = 0x7FFFFFFF; }
            bk[t] = k; bi[t] = i;
        }
        row_min16x2(bk, bi);
#pragma unroll
        for (int t = 0; t < 2; t++) if (writer && t < nx) { Q.M1k[x[t] >> 4] = bk[t]; Q.M1i[x[t] >> 4] = bi[t]; }
        double sk[2]; int si[2];
#pragma unroll
        for (int t = 0; t < 2; t++) {
            double k = mk[t]; int i = mi[t];
#pragma unroll
            for (int u = 0; u < 2; u++) if (u < nx && ((x[u] ^ x[t]) >> 8) == 0 && ((x[u] >> 4) & 15) == rl) { k = bk[u]; i = bi[u]; }
            if (t >= nx) { k = TQ_INF; i = 0x7FFFFFFF; }
            sk[t] = k; si[t] = i;
        }
        row_min16x2(sk, si);
        double k = TQ_INF; int i = 0x7FFFFFFF;
        for (int j = rl; j < Q.n0; j += 16) {
            double a = Q.M0k[j]; int b = Q.M0i[j];
#pragma unroll
            for (int u = 0; u < 2; u++) if (u < nx && (x[u] >> 8) == j) { a = sk[u]; b = si[u]; }
            if (hless(a, b, k, i)) { k = a; i = b; }
        }
#pragma unroll
        for (int t = 0; t < 2; t++) if (writer && t < nx) { Q.M0k[x[t] >> 8] = sk[t]; Q.M0i[x[t] >> 8] = si[t]; }
        row_min16(k, i);
        return k < TQ_INF ? i : -1;
    }
};

// how many lanes of the wave below me have their bit set in m (v_mbcnt: no (1 << lane) - 1 mask is kept in registers for it)
static __device__ __forceinline__ int sl_below(unsigned long long m)
{
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// eight entries of a list in registers: where D and K are among the first n
static __device__ __forceinline__ void sl_find8(const int (&u)[8], int n, int x0, int D, int K, int &iD, int &iK)
{
    unsigned mD = 0, mK = 0;
#pragma unroll
    for (int j = 7; j >= 0; j--) { mD = (mD << 1) | (unsigned)(u[j] == D); mK = (mK << 1) | (unsigned)(u[j] == K); }
    const unsigned valid = n >= 8 ? 0xFFu : ((1u << (n < 0 ? 0 : n)) - 1u);
    mD &= valid; mK &= valid;
    if (mD && iD < 0) iD = x0 + __ffs((int)mD) - 1;
    if (mK && iK < 0) iK = x0 + __ffs((int)mK) - 1;
}
// the whole list (the tails: entries beyond what travels with the stages)
static __device__ __forceinline__ void sl_find(const int *pool, int off, int cnt, int D, int K, bool wantK, int &iD, int &iK)
{
    iD = -1; iK = -1;
    for (int x0 = 0; x0 < cnt; x0 += 8) {
        int u[8];
#pragma unroll
        for (int j = 0; j < 8; j++) u[j] = x0 + j < cnt ? pool[off + x0 + j] : -1;
        sl_find8(u, cnt - x0, x0, D, K, iD, iK);
        if (iD >= 0 && (!wantK || iK >= 0)) break;
    }
}

// Three waves per SIMD = 168 registers: two of these waves then leave 176, an LSD-preamble wave (96) and an ORB-level wave (80), where
// 184 left room for one of them (DESIGN 4, "The register file as a budget"; tests/test_kernel_budget.py holds the sum).  The hint only
// makes the allocator hold the band: the kernel fits it without scratch.
__attribute__((amdgpu_waves_per_eu(3, 3)))
__global__ __launch_bounds__(64) void k_peac_cluster_slots(ClArgs a, int nframes)
{
    constexpr int GL = 16, NG = 4;
    extern __shared__ __attribute__((aligned(16))) unsigned char tq_lds[];          // NG groups x n0 x (double + int)
    __shared__ SlLds S;
    const int lane = threadIdx.x, gl = lane & 15, gi = lane >> 4;
    int frame = (a.perm ? a.perm[blockIdx.x] : (int)blockIdx.x) * NG + gi;
    const bool galive = frame < nframes;
    if (!galive) frame = nframes - 1;                          // idle group: aliases a frame read-only, writes nothing
    const int nblk = a.nblk, Nw = a.Nw, Nh = a.Nh;
    TQueue Q; Q.n0 = a.tq_n0;
    Q.K = a.tqK + (size_t)frame * Q.n0 * 256; Q.M1k = a.tqM1k + (size_t)frame * Q.n0 * 16; Q.M1i = a.tqM1i + (size_t)frame * Q.n0 * 16;
    Q.M0k = reinterpret_cast<double *>(tq_lds) + (size_t)gi * Q.n0;
    Q.M0i = reinterpret_cast<int *>(tq_lds + (size_t)NG * Q.n0 * sizeof(double)) + (size_t)gi * Q.n0;
    int *lq = a.tqLq + (size_t)frame * Q.n0 * 256;             // (label << 16 | slot) of every slot
    Q.n0 = (nblk + 255) >> 8;                                  // slots only: half of the entries the id-indexed queue needs
    double *segD = a.segD + (size_t)frame * a.segcap * SEG_D;
    int *segI = a.segI + (size_t)frame * a.segcap * SEG_I;
    int *pool = a.pool + (size_t)frame * a.poolcap, *pool2 = a.pool2 + (size_t)frame * a.poolcap;
    int *parent = a.parent + (size_t)frame * nblk, *dsize = a.dsize + (size_t)frame * nblk;
    int *eflag = a.eflag + (size_t)frame * nblk;
    HotNode *hot = a.hot + (size_t)frame * a.segcap;
    PT_DECL
#ifdef HVO_PEAC_TIMING
    const unsigned long long t_in0 = clock64();
#endif
    if (galive) for (int b = gl; b < nblk; b += GL) { parent[b] = b; dsize[b] = 1; if (!a.edges_done) eflag[b] = 0; }
    __syncthreads();
    // initGraph's edges (AHCPlaneFitter.hpp:896-954) where k_peac_edges has not written them (1280x960: its blocks do not fit LDS) -- the two
    // passes of k_peac_cluster, a row / a column per lane.  bits: 1=left 2=right 4=up 8=down
#define GOK(c) (segI[(size_t)(c) * SEG_I + 6] != 0)
#define SD(c) (segD + (size_t)(c) * SEG_D)
    if (galive && !a.edges_done) for (int i = gl; i < Nh; i += GL) {
        for (int j = 1; j < Nw; j += 2) {
            const int c = i * Nw + j;
            if (!GOK(c - 1)) { --j; continue; }
            if (!GOK(c)) continue;
            if (j < Nw - 1 && !GOK(c + 1)) { ++j; continue; }
            const double th = t_ang_init(a, SD(c)[11]);
            if ((j < Nw - 1 && nsim(SD(c - 1), SD(c + 1)) >= th) || (j == Nw - 1 && nsim(SD(c), SD(c - 1)) >= th)) {
                eflag[c] |= 1; eflag[c - 1] |= 2;
                if (j < Nw - 1) { eflag[c] |= 2; eflag[c + 1] |= 1; }
            } else --j;
        }
    }
    __syncthreads();
    if (galive && !a.edges_done) for (int j = gl; j < Nw; j += GL) {
        for (int i = 1; i < Nh; i += 2) {
            const int c = i * Nw + j;
            if (!GOK(c - Nw)) { --i; continue; }
            if (!GOK(c)) continue;
            if (i < Nh - 1 && !GOK(c + Nw)) { ++i; continue; }
            const double th = t_ang_init(a, SD(c)[11]);
            if ((i < Nh - 1 && nsim(SD(c - Nw), SD(c + Nw)) >= th) || (i == Nh - 1 && nsim(SD(c), SD(c - Nw)) >= th)) {
                eflag[c] |= 4; eflag[c - Nw] |= 8;
                if (i < Nh - 1) { eflag[c] |= 8; eflag[c + Nw] |= 4; }
            } else --i;
        }
    }
#undef GOK
#undef SD
    __syncthreads();
    // adjacency lists (up, left, right, down); keys; packed ids; labels
    int hn = 0;
    for (int base = 0; base < Q.n0 * 256; base += GL) {
        const int b = base + gl;
        bool ok = false; double mse_b = 0;
        if (galive && b < nblk) {
            const int *si = segI + (size_t)b * SEG_I;
            const int e = eflag[b];
            int n = 0;
            if (e & 4) pool[b * 4 + n++] = b - Nw;
            if (e & 1) pool[b * 4 + n++] = b - 1;
            if (e & 2) pool[b * 4 + n++] = b + 1;
            if (e & 8) pool[b * 4 + n++] = b + Nw;
            ok = si[6] != 0;
            hot[b].cnt = n;                                      // (the rest of the record: k_peac_blocks)
            hot[b].rid = SL_PACK(b, b);                          // rid of a block is the block; its label too
            mse_b = hot[b].mse;
        }
        if (galive) { Q.K[b] = ok ? mse_b : TQ_INF; lq[b] = SL_PACK(b, b); }
        hn += __popcll(Grp<GL>::ballot(ok));
    }
    __syncthreads();
#ifdef HVO_PEAC_TIMING
    const unsigned long long t_in1 = clock64();
#endif
    if (galive) for (int j = gl; j < Q.n0 * 16; j += GL) {
        double k = TQ_INF; int i = 0x7FFFFFFF;
        for (int q = 0; q < 16; q++) { const double kq = Q.K[j * 16 + q]; const int iq = SL_PACK(j * 16 + q, j * 16 + q); if (hless(kq, iq, k, i)) { k = kq; i = iq; } }
        Q.M1k[j] = k; Q.M1i[j] = i;
    }
    __syncthreads();
    for (int j = gl; j < Q.n0; j += GL) {
        double k = TQ_INF; int i = 0x7FFFFFFF;
        if (galive) for (int q = 0; q < 16; q++) { const double kq = Q.M1k[j * 16 + q]; const int iq = Q.M1i[j * 16 + q]; if (hless(kq, iq, k, i)) { k = kq; i = iq; } }
        Q.M0k[j] = k; Q.M0i[j] = i;
    }
#ifdef HVO_PEAC_TIMING
    if (lane == 0) { const unsigned long long t_in2 = clock64(); atomicAdd(&g_peac_t[12], t_in1 - t_in0); atomicAdd(&g_peac_t[13], t_in2 - t_in1); atomicAdd(&g_peac_t[14], 1ull); }
#endif
    int nseg = nblk, pooltop = nblk * 4, next = 0, flags = 0;   // nseg counts LABELS
    int *ext = a.extracted + (size_t)frame * 2 * MAX_PLANES;
    const unsigned long long lt_mask = (1ull << gl) - 1;       // lanes of my group below me
    __syncthreads();
    int ptop = hn > 0 ? tq_top(Q, gl) : -1;                    // packed
    double nps[9], npn[3]; int n_cnt = 0, n_off = 0, n_N = 0, n_rid = 0, n_dsr = 0, n_dss = 0;
    auto fetch_next = [&](int r) {
        const HotNode *h = hot + (r < 0 ? 0 : SL_SLOT(r));
        n_cnt = h->cnt; n_off = h->off; n_N = h->N; n_rid = h->rid; n_dsr = h->dsr; n_dss = h->dss;
#pragma unroll
        for (int q2 = 0; q2 < 9; q2++) nps[q2] = h->st[q2];
        npn[0] = h->nrm[0]; npn[1] = h->nrm[1]; npn[2] = h->nrm[2];
    };
    int a0n = -1, f_id = -1, fg = gi, nbase = 16; bool lend = false;
    auto assign_and_prefetch = [&]() {
        const int c = hn > 0 ? n_cnt : 0;
        const int c0 = __builtin_amdgcn_readlane(c, 0), c1 = __builtin_amdgcn_readlane(c, 16), c2 = __builtin_amdgcn_readlane(c, 32), c3 = __builtin_amdgcn_readlane(c, 48);
        const int x0 = max(c0 - 16, 0), x1 = max(c1 - 16, 0), x2 = max(c2 - 16, 0), x3 = max(c3 - 16, 0), X = x0 + x1 + x2 + x3;
        a0n = gl < c ? pool[n_off + gl] : -1;
        lend = false; fg = gi; f_id = -1; nbase = 16;
        if (X > 0) {                                            // uniform
            const bool idle = gl >= c;
            const unsigned long long im = __ballot(idle);
            const int r = sl_below(im), I = __popcll(im);
            const int b1 = x0, b2 = x0 + x1, b3 = b2 + x2;
            const int g2 = r < b1 ? 0 : r < b2 ? 1 : r < b3 ? 2 : 3;
            const int xb = g2 == 0 ? 0 : g2 == 1 ? b1 : g2 == 2 ? b2 : b3;
            const int myxb = gi == 0 ? 0 : gi == 1 ? b1 : gi == 2 ? b2 : b3, myx = gi == 0 ? x0 : gi == 1 ? x1 : gi == 2 ? x2 : x3;
            nbase = 16 + min(myx, max(I - myxb, 0));
            const unsigned long long fp = __shfl((unsigned long long)(uintptr_t)pool, g2 << 4);
            const int foff = __shfl(n_off, g2 << 4);
            lend = idle && r < X;
            if (lend) { fg = g2; f_id = reinterpret_cast<const int *>((uintptr_t)fp)[foff + 16 + r - xb]; }
        }
    };
    fetch_next(ptop);
    assign_and_prefetch();
    while (__any(hn > 0)) {
        const bool act = hn > 0;
        PT_CNT(8, 1)
        const bool need_gc = act && pooltop > a.poolcap - 2 * a.nblk;
        if (__any(need_gc)) {
            gpool_gc<GL>(hot, nblk, pool, pool2, pooltop, need_gc);        // every live node is a slot < nblk
            n_off = hot[ptop < 0 ? 0 : SL_SLOT(ptop)].off;
            assign_and_prefetch();
        }
        PT(0)
        const int p = act ? SL_SLOT(ptop) : -1;
        const bool live = act;
        const int pcnt = live ? n_cnt : 0, poff = n_off, pN = n_N, prid = n_rid & 0xFFFF, pdsr = n_dsr, pdss = n_dss;
        if (gl == 0) {
#pragma unroll
            for (int q = 0; q < 9; q++) S.ps[gi][q] = nps[q];
            S.ps[gi][9] = npn[0]; S.ps[gi][10] = npn[1]; S.ps[gi][11] = npn[2];
            reinterpret_cast<int *>(&S.ps[gi][12])[0] = pN;
            S.ncnt[gi] = -1;
        }
        lend_lds_order();
        const bool anyl = __any(lend);
        // ---- first pass: one candidate per lane, of my group (home) or of group fg (lent) ----
        const bool home = gl < pcnt;
        const bool c1v = home || lend;
        const int cg = lend ? fg : gi;
        const int nb1 = home ? a0n : f_id;                     // slot
        const int cframe = __shfl(frame, cg << 4);
        HotNode *hotc = a.hot + (size_t)cframe * a.segcap;
        int *poolc = reinterpret_cast<int *>((uintptr_t)__shfl((unsigned long long)(uintptr_t)pool, cg << 4));
        int id_cur = (nbase + gl < pcnt) ? pool[poff + nbase + gl] : -1;
        double ps_r[9], pn_r[3]; int pNc;
        PT(2)
        int noff1 = 0, ncnt1 = 0, c1N = 0, c1lab = 0; bool c1has = false; double c1m = 0, c1c2 = 0, c1l0 = 0;
        {
            double lst[9]; int lN = 4; bool has = false;
#pragma unroll
            for (int q = 0; q < 9; q++) lst[q] = 0;
            double nst[9], nnr[3]; int nN = 0;
#pragma unroll
            for (int q = 0; q < 9; q++) nst[q] = 0;
            nnr[0] = nnr[1] = nnr[2] = 0;
            if (c1v) {
                const HotNode *nd = hotc + nb1;
                nN = nd->N; noff1 = nd->off; ncnt1 = nd->cnt; c1lab = nd->rid >> 16;
                nnr[0] = nd->nrm[0]; nnr[1] = nd->nrm[1]; nnr[2] = nd->nrm[2];
#pragma unroll
                for (int q = 0; q < 9; q++) nst[q] = nd->st[q];
            }
            {
                const double *pc = S.ps[cg];
#pragma unroll
                for (int q = 0; q < 9; q++) ps_r[q] = pc[q];
                pn_r[0] = pc[9]; pn_r[1] = pc[10]; pn_r[2] = pc[11];
                pNc = reinterpret_cast<const int *>(pc + 12)[0];
            }
            if (c1v && !(fabs(pn_r[0] * nnr[0] + pn_r[1] * nnr[1] + pn_r[2] * nnr[2]) < a.c60)) {      // T_ang(P_MERGING)
#pragma unroll
                for (int q = 0; q < 9; q++) lst[q] = ps_r[q] + nst[q];
                lN = pNc + nN;
                has = true;
            }
            if (__any(has)) {
                double tc2, tl0, tm;
                PT(2)
                stats_lambda_dev(lst, lN, tc2, tl0, tm);
                PT(4)
                if (has) { c1has = true; c1m = tm; c1c2 = tc2; c1l0 = tl0; c1N = lN; }
            }
        }
        // ---- the tie rule over the first pass: my group's own lanes by DPP, lent lanes through LDS ----
        double gmin; int rg, rx, wlab;                          // running: min mse, smallest good label, largest label, the winner's label
        {
            const bool c1own = c1has && !lend;
            gmin = c1own ? c1m : TQ_INF;
#define GM_STEP(o) { const double t = row_partner<o>(gmin); gmin = key_min(t, gmin); }
            GM_STEP(1) GM_STEP(2) GM_STEP(4) GM_STEP(8)
#undef GM_STEP
            double gminc = gmin;
            if (anyl) {
                if (gl == 0) S.red[gi].minbits = (unsigned long long)__double_as_longlong(gmin);
                lend_lds_order();
                if (lend && c1has) atomicMin(&S.red[fg].minbits, (unsigned long long)__double_as_longlong(c1m));
                lend_lds_order();
                gmin = __longlong_as_double((long long)S.red[gi].minbits);
                gminc = __longlong_as_double((long long)S.red[cg].minbits);
            }
            const bool c1good = (double)c1N >= c1m;
            rg = 0x7FFFFFFF; rx = -1;
            if (c1own && c1m == gmin) { if (c1good) rg = c1lab; rx = c1lab; }
#define GM_STEP(o) { const int t0 = row_partner<o>(rg), t1 = row_partner<o>(rx); rg = min(rg, t0); rx = max(rx, t1); }
            GM_STEP(1) GM_STEP(2) GM_STEP(4) GM_STEP(8)
#undef GM_STEP
            if (anyl) {
                if (gl == 0) { S.red[gi].gid = rg; S.red[gi].xid = rx; }
                lend_lds_order();
                if (lend && c1has && c1m == gminc) { if (c1good) atomicMin(&S.red[fg].gid, c1lab); atomicMax(&S.red[fg].xid, c1lab); }
                lend_lds_order();
                rg = S.red[gi].gid; rx = S.red[gi].xid;
            }
            wlab = rg != 0x7FFFFFFF ? rg : rx;                  // -1: no candidate yet
            int wlabc = wlab;
            if (anyl) {
                if (gl == 0) S.red[gi].gid = wlab;
                lend_lds_order();
                wlabc = S.red[cg].gid;
            }
            if (c1has && c1m == gminc && c1lab == wlabc) {      // the winner's state (its label is unique in the list)
                LendWin &w = S.win[cg];
                w.c2 = c1c2; w.l0 = c1l0; w.noff = noff1; w.ncnt = ncnt1; w.lN = c1N; w.flag = nb1;
            }
        }
        // ---- later passes: my group's entries from nbase on; each pass is folded into the running (min, labels) at once ----
        int t_id = -1, t_off = 0, t_cnt = 0;                   // my entry of the first chunk no lane took, and its list header
        if (__any(nbase < pcnt)) {
            if (anyl) {                                        // a lent lane holds another group's sums
                const double *pc = S.ps[gi];
#pragma unroll
                for (int q = 0; q < 9; q++) ps_r[q] = pc[q];
                pn_r[0] = pc[9]; pn_r[1] = pc[10]; pn_r[2] = pc[11];
            }
            for (int base = nbase; __any(base < pcnt); base += GL) {
                PT_CNT(9, 1)
                const int k = base + gl;
                const int id_nxt = k + GL < pcnt ? pool[poff + k + GL] : -1;
                double lst[9]; int lN = 4, nb = 0, noff_ = 0, ncnt_ = 0, lab = 0; bool has = false;
#pragma unroll
                for (int q = 0; q < 9; q++) lst[q] = 0;
                if (k < pcnt) {
                    nb = id_cur;
                    const HotNode *nd = hot + nb;
                    const int nN = nd->N; noff_ = nd->off; ncnt_ = nd->cnt; lab = nd->rid >> 16;
                    if (base == nbase) { t_id = nb; t_off = noff_; t_cnt = ncnt_; }
                    if (!(fabs(pn_r[0] * nd->nrm[0] + pn_r[1] * nd->nrm[1] + pn_r[2] * nd->nrm[2]) < a.c60)) {
#pragma unroll
                        for (int q = 0; q < 9; q++) lst[q] = ps_r[q] + nd->st[q];
                        lN = pN + nN;
                        has = true;
                    }
                }
                if (__any(has)) {
                    double tc2, tl0, tm;
                    PT(2)
                    stats_lambda_dev(lst, lN, tc2, tl0, tm);
                    PT(4)
                    double pm = has ? tm : TQ_INF;
#define GM_STEP(o) { const double t = row_partner<o>(pm); pm = key_min(t, pm); }
                    GM_STEP(1) GM_STEP(2) GM_STEP(4) GM_STEP(8)
#undef GM_STEP
                    const bool tied = has && tm == pm, good = (double)lN >= tm;
                    int prg = tied && good ? lab : 0x7FFFFFFF, prx = tied ? lab : -1;
#define GM_STEP(o) { const int t0 = row_partner<o>(prg), t1 = row_partner<o>(prx); prg = min(prg, t0); prx = max(prx, t1); }
                    GM_STEP(1) GM_STEP(2) GM_STEP(4) GM_STEP(8)
#undef GM_STEP
                    if (pm < gmin) { gmin = pm; rg = prg; rx = prx; }
                    else if (pm == gmin) { rg = min(rg, prg); rx = max(rx, prx); }
                    const int nw = rg != 0x7FFFFFFF ? rg : rx;
                    if (nw != wlab && tied && tm == gmin && lab == nw) {      // the winner has changed: it is a candidate of this pass
                        LendWin &w = S.win[gi];
                        w.c2 = tc2; w.l0 = tl0; w.noff = noff_; w.ncnt = ncnt_; w.lN = lN; w.flag = nb;
                    }
                    wlab = nw;
                }
                id_cur = id_nxt;
            }
        }
        PT(2)
        lend_lds_order();
        const bool any_cand = gmin < TQ_INF;
        const double m = gmin, c2 = S.win[gi].c2, l0 = S.win[gi].l0; int noff = S.win[gi].noff, ncnt = S.win[gi].ncnt; const int wN = S.win[gi].lN, nb = S.win[gi].flag;   // nb: the partner's SLOT
        PT(3)
        // ---- merge decision ----
        bool do_merge = false;
        if (live && any_cand) {
            const double t = 1.6e-6 * c2 * c2 + 8.0;            // T_mse(P_MERGING)
            if (m < t * t) {
                if (nseg >= a.segcap || pooltop + pcnt + ncnt > a.poolcap) flags |= 8;     // capacity: keep the node unmerged
                else do_merge = true;
            }
        }
        if (!do_merge) ncnt = 0;
        const int id = nseg;                                    // the merged node's LABEL
        const bool no_merge = live && !do_merge;
        if (do_merge) { PT_CNT(10, 1) nseg++; }
        if (no_merge) { PT_CNT(11, 1) }
        PT(4)
        // the slot that stays: the one with the longer list (p on a tie); D's neighbours are the ones visited
        const bool kp = pcnt >= ncnt;
        const int K = do_merge ? (kp ? p : nb) : -1, D = do_merge ? (kp ? nb : p) : p;
        const int moff = pooltop;
        if (act) hn -= 1;                                       // merge: -2 + 1
        int p_c = p, K_c = K, D_c = D, moff_c = moff; bool dm_c = do_merge, nm_c = no_merge, kp_c = kp;
        if (anyl) {
            if (gl == 0) { SlDec &d = S.dec[gi]; d.p = p; d.K = K; d.D = D; d.code = (do_merge ? 1 : 0) | (no_merge ? 2 : 0) | (kp ? 4 : 0); d.moff = moff; }
            lend_lds_order();
            if (lend) { const SlDec &d = S.dec[fg]; p_c = d.p; K_c = d.K; D_c = d.D; moff_c = d.moff; dm_c = (d.code & 1) != 0; nm_c = (d.code & 2) != 0; kp_c = (d.code & 4) != 0; }
        }
        // What the lanes that hold p's members (aid: first-pass candidates, lent lanes included) do:
        //   no merge          p leaves the member's list                                           (disconnectAllNbs)
        //   merge, D == p     the member's list: K there already -> p leaves it; else p -> K and the member joins K's list
        //   merge, K == p     nothing to edit: the member stays in K's list (copied)
        // and the lanes that hold the partner's members (vB), the other way round.
        TQUpdateS qu;
        const int aid = c1v ? nb1 : -1, aoff = noff1, acnt = ncnt1;
        const bool editA = aid >= 0 && (nm_c || (dm_c && !kp_c && aid != K_c));
        // (most merges keep p's slot: then no lane of the wave has a member's list to edit, and the eight guarded loads and the search are skipped)
        const bool anyA = __any(editA);
        ListFind fa; fa.off = 0; fa.cnt = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) fa.u[j] = -1;
        if (anyA) fa.issue(poolc, aoff, editA ? acnt : 0);
        const int vB = gl < ncnt ? pool[noff + gl] : -1;        // ncnt == 0 unless this group merges
        qu.issue(Q, lq, gl, act ? (do_merge ? 2 : 1) : 0, D, TQ_INF, 0x7FFFFFFF, K < 0 ? 0 : K, m, SL_PACK(id, K < 0 ? 0 : K));
        // stage 1: the headers of the partner's members (only when they are the ones edited), the next top
        const bool inB = vB >= 0 && vB != p;
        const bool editB = inB && kp;                           // D == partner: its members' lists are edited
        int qb_off = 0, qb_cnt = 0;
        if (editB) { qb_off = hot[vB].off; qb_cnt = hot[vB].cnt; }
        ptop = qu.take(Q, lq, gl, gl == 0);
        if (hn <= 0) ptop = -1;
        const int ptslot = ptop < 0 ? -1 : SL_SLOT(ptop);
        const int ptslot_c = anyl ? __shfl(ptslot, cg << 4) : ptslot;
        PT(1)
        fetch_next(ptop);
        // stage 2: the lists of the partner's members
        const bool anyB = __any(editB);
        ListFind fb; fb.off = 0; fb.cnt = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) fb.u[j] = -1;
        if (anyB) fb.issue(pool, qb_off, editB ? qb_cnt : 0);
        // A: where D (= p) and K are in my member's list
        int a_iD = -1, a_iK = -1;
        if (anyA) {
            const int wantK = dm_c;
            sl_find8(fa.u, fa.cnt, 0, p_c, wantK ? K_c : p_c, a_iD, a_iK);
            bool more = fa.cnt > 8 && !(a_iD >= 0 && (!wantK || a_iK >= 0));
            for (int x0 = 8; __any(more); x0 += 8) {
                int w[8];
#pragma unroll
                for (int j = 0; j < 8; j++) w[j] = (more && x0 + j < fa.cnt) ? poolc[fa.off + x0 + j] : -1;
                if (more) sl_find8(w, fa.cnt - x0, x0, p_c, wantK ? K_c : p_c, a_iD, a_iK);
                more = more && x0 + 8 < fa.cnt && !(a_iD >= 0 && (!wantK || a_iK >= 0));
            }
        }
        // stage 3: the edits, and K's new list at the pool's top.  B's members first ...
        int mcnt = 0;
        {
            int b_iD = -1, b_iK = -1;
            if (editB) {
                sl_find8(fb.u, fb.cnt, 0, nb, p, b_iD, b_iK);
                if (fb.cnt > 8 && !(b_iD >= 0 && b_iK >= 0)) {
                    for (int x0 = 8; x0 < fb.cnt; x0 += 8) {
                        int w[8];
#pragma unroll
                        for (int j = 0; j < 8; j++) w[j] = x0 + j < fb.cnt ? pool[fb.off + x0 + j] : -1;
                        sl_find8(w, fb.cnt - x0, x0, nb, p, b_iD, b_iK);
                        if (b_iD >= 0 && b_iK >= 0) break;
                    }
                }
            }
            bool keep = inB && !kp;                             // K == partner: all of its members (but p) stay in its list
            if (editB) {
                if (b_iK >= 0) {                                // a common neighbour: the partner leaves its list
                    if (b_iD >= 0) { if (b_iD != qb_cnt - 1) pool[qb_off + b_iD] = pool[qb_off + qb_cnt - 1]; hot[vB].cnt = qb_cnt - 1; if (vB == ptslot) S.ncnt[gi] = qb_cnt - 1; }
                } else { if (b_iD >= 0) pool[qb_off + b_iD] = p; keep = true; }        // the partner -> p; it joins p's list
            }
            const unsigned long long km = Grp<GL>::ballot(keep);
            if (keep) pool[moff + mcnt + __popcll(km & lt_mask)] = vB;
            mcnt += __popcll(km);
        }
        PT(5)
        for (int base = GL; __any(base < ncnt); base += GL) {    // partner lists longer than a chunk
            const int k = base + gl;
            int v = -1; bool keep = false;
            if (k < ncnt) {
                v = pool[noff + k];
                if (v != p) {
                    if (!kp) keep = true;
                    else {
                        const int off = hot[v].off, cnt = hot[v].cnt;
                        int iD, iK;
                        sl_find(pool, off, cnt, nb, p, true, iD, iK);
                        if (iK >= 0) { if (iD >= 0) { if (iD != cnt - 1) pool[off + iD] = pool[off + cnt - 1]; hot[v].cnt = cnt - 1; if (v == ptslot) S.ncnt[gi] = cnt - 1; } }
                        else { if (iD >= 0) pool[off + iD] = p; keep = true; }
                    }
                }
            }
            const unsigned long long km = Grp<GL>::ballot(keep);
            if (keep) pool[moff + mcnt + __popcll(km & lt_mask)] = v;
            mcnt += __popcll(km);
        }
        PT(6)
        // ... then p's members
        if (__any(aid >= 0)) {
            bool keep = aid >= 0 && dm_c && kp_c && aid != D_c;  // K == p: its members (but the partner) stay
            if (editA) {
                HotNode *hv = hotc + aid;
                const int off = aoff, cnt = acnt;
                if (dm_c && a_iK < 0) { if (a_iD >= 0) poolc[off + a_iD] = K_c; keep = true; }      // p -> K; the member joins K's list
                else if (a_iD >= 0) {                           // p leaves the list (no merge, or K is there already)
                    if (a_iD != cnt - 1) poolc[off + a_iD] = poolc[off + cnt - 1];
                    hv->cnt = cnt - 1;
                    if (aid == ptslot_c) S.ncnt[cg] = cnt - 1;
                }
            }
            if (!anyl) {
                const unsigned long long km = Grp<GL>::ballot(keep);
                if (keep) pool[moff + mcnt + __popcll(km & lt_mask)] = aid;
                mcnt += __popcll(km);
            } else {
                if (gl == 0) S.dec[gi].mB = mcnt;
                lend_lds_order();
                const int mB_c = lend ? S.dec[fg].mB : mcnt;
                const unsigned long long km = __ballot(keep);
                const unsigned long long s0 = __ballot(c1v && cg == 0), s1 = __ballot(c1v && cg == 1), s2 = __ballot(c1v && cg == 2), s3 = __ballot(c1v && cg == 3);
                const unsigned long long sc_ = cg == 0 ? s0 : cg == 1 ? s1 : cg == 2 ? s2 : s3, so_ = gi == 0 ? s0 : gi == 1 ? s1 : gi == 2 ? s2 : s3;
                if (keep) poolc[moff_c + mB_c + sl_below(km & sc_)] = aid;
                mcnt += __popcll(km & so_);
            }
        }
        PT(5)
        for (int base = nbase; __any(live && base < pcnt); base += GL) {   // p's entries that no lane took in the first pass
            const int k = base + gl;
            int v = -1; bool keep = false;
            if (live && k < pcnt) {
                const bool first = base == nbase;                 // this chunk's ids and headers came with the evaluation
                v = first ? t_id : pool[poff + k];
                if (do_merge && kp) keep = v != nb;             // K == p: nothing to edit
                else if (!do_merge || v != nb) {
                    HotNode *hv = hot + v;
                    int off = t_off, cnt = t_cnt;
                    if (!first) { off = hv->off; cnt = hv->cnt; }
                    int iD, iK;
                    sl_find(pool, off, cnt, p, do_merge ? nb : p, do_merge, iD, iK);
                    if (do_merge && iK < 0) { if (iD >= 0) pool[off + iD] = nb; keep = true; }
                    else if (iD >= 0) { if (iD != cnt - 1) pool[off + iD] = pool[off + cnt - 1]; hv->cnt = cnt - 1; if (v == ptslot) S.ncnt[gi] = cnt - 1; }
                }
            }
            const unsigned long long km = Grp<GL>::ballot(keep);
            if (keep) pool[moff + mcnt + __popcll(km & lt_mask)] = v;
            mcnt += __popcll(km);
        }
        PT(6)
        // ---- the merged node's record, in slot K ----
        if (__any(do_merge)) {
            const HotNode *W = hot + (do_merge ? nb : 0);
            const double *pc = S.ps[gi];
            double mst[9], mn[3];
#pragma unroll
            for (int q = 0; q < 9; q++) mst[q] = pc[q] + W->st[q];
            const int WN = W->N, Wrid = W->rid & 0xFFFF, bdss = W->dss, bdsr = W->dsr;
            const int bN = do_merge ? wN : 4;
            stats_vector_dev(mst, bN, l0, mn);
            if (do_merge && gl == 0) {
                HotNode *M = hot + K;
#pragma unroll
                for (int q = 0; q < 9; q++) M->st[q] = mst[q];
                M->nrm[0] = mn[0]; M->nrm[1] = mn[1]; M->nrm[2] = mn[2]; M->mse = m;
                // ds.Union(pa.rid, pb.rid) (DisjointSet.hpp:63-83): the two nodes carry their sets' roots and sizes -- two stores, no Find
                int root = pdsr, size = pdss + bdss;
                if (pdsr == bdsr) size = pdss;
                else if (pdss < bdss) { parent[pdsr] = bdsr; dsize[bdsr] = size; root = bdsr; }
                else { parent[bdsr] = pdsr; dsize[pdsr] = size; }
                M->N = bN; M->rid = SL_PACK(id, pN >= WN ? prid : Wrid); M->off = moff; M->cnt = mcnt; M->dss = size; M->dsr = root;
                hot[D].cnt = 0;
            }
        }
        if (do_merge) pooltop += pcnt + ncnt;
        if (no_merge) {
            if (pN >= MIN_SUPPORT) { if (next < MAX_PLANES) { if (gl == 0) ext[next] = p; next++; } else flags |= 16; }
            if (gl == 0) hot[p].cnt = 0;
        }
        PT(7)
        __syncthreads();                                       // this iteration's records, lists and queue stores
        {
            const bool fresh = do_merge && ptslot == K;
            if (__any(fresh)) { if (fresh) fetch_next(ptop); }
            lend_lds_order();
            { const int e = S.ncnt[gi]; if (e >= 0) n_cnt = e; }
            if (fresh) { n_cnt = mcnt; n_off = moff; }
            assign_and_prefetch();
        }
        PT(0)
    }
    // std::sort by N descending, ties -> extraction order (stable insertion sort); ext holds slots until the records are written
    __syncthreads();
    if (gl == 0) {
        for (int i = 1; i < next; i++) {
            int v = ext[i], j = i - 1;
            int vN = hot[v].N;
            while (j >= 0 && hot[ext[j]].N < vN) { ext[j + 1] = ext[j]; j--; }
            ext[j + 1] = v;
        }
    }
    __syncthreads();
    // what the refinement kernels read, under the nodes' LABELS: every label this kernel created says "dead, no list", the extracted
    // planes get their records (sums, centre, normal, mse; N, rid)
    for (int v = a.nblk + gl; v < nseg; v += GL) { int *si = segI + (size_t)v * SEG_I; si[2] = 1; si[3] = 0; si[4] = 0; }
    __syncthreads();
    {
        int lab[(MAX_PLANES + GL - 1) / GL];
        for (int e = gl, q = 0; e < next; e += GL, q++) {
            const int s = ext[e]; const HotNode *nv = hot + s;
            const int v = nv->rid >> 16;
            lab[q] = v;
            double *sd = segD + (size_t)v * SEG_D; int *si = segI + (size_t)v * SEG_I;
            const double sc = 1.0 / nv->N;
#pragma unroll
            for (int q2 = 0; q2 < 9; q2++) sd[q2] = nv->st[q2];
            sd[9] = nv->st[0] * sc; sd[10] = nv->st[1] * sc; sd[11] = nv->st[2] * sc;
            sd[12] = nv->nrm[0]; sd[13] = nv->nrm[1]; sd[14] = nv->nrm[2]; sd[15] = nv->mse;
            si[0] = nv->N; si[1] = nv->rid & 0xFFFF; si[2] = 0; si[3] = 0; si[4] = 0; si[5] = 0; si[6] = 1; si[7] = 0;
        }
        __syncthreads();
        for (int e = gl, q = 0; e < next; e += GL, q++) ext[e] = lab[q];
    }
    __syncthreads();
    PT(0)
    PT_FLUSH
    if (galive && gl == 0) {
        int *meta = a.meta + (size_t)frame * 16;
        meta[0] = nseg; meta[1] = 0; meta[2] = next; meta[3] = flags; meta[6] = 0;      // the lists are dead: k_peac_final starts an empty pool
    }
}
