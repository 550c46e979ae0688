// cnnq_half_entropy.hip.h - the uniform per-channel Q/DQ that counts its codes (-me, iq.py:586-587: the codes exist in the
// reference only as the argument of shannon_entropy) on CONTIGUOUS bf16 / fp16 activations x[N][C][HW]: the pass over (channel,
// batch split) workgroups, its resident form - config 2 in one launch that reads x once - and which classes of layer run where.
// Part of the single translation unit cnnq_kernels.hip (see its header for the design).
//
// Everything around the two kernels is the family's: the extrema partials come from k_h_minmax (config 2), the table from
// k_params on cnnq_pc_stats_dt's statistics (config 3) or from the caller; the counts go to the XHIST_REPLICAS replica tables of
// the single-launch kernels, which k_entropy_replicas and k_hist_replicas_fold consume and leave zero.
//
// The contract: y is k_h_qdq's / k_h_whole's, bit for bit, and the replica tables summed are, word for
// word, the histogram k_qdq<HIST> fills on x.float().
//
// The counting is k_qdq<HIST>'s own definitions (xhist_zero, xhist_add, xhist_add_zp, xhist_fold, xhist_replica in
// cnnq_qdq.hip.h) and nothing else: the table is nbins x HREP words of dynamic LDS, replica = lane & (HREP - 1).  A workgroup
// lies in ONE channel, so the zero point's code (about half of a post-ReLU layer) is ONE register counter per lane, added to
// the table once at the end; after the barrier one thread per bin folds the replicas and issues at most one 64-bit global atomic,
// into replica table (workgroup id & (XHIST_REPLICAS - 1)).  A code indexes the table as code & (nbins - 1): the host passes
// nbins > qmax of every channel (2^num_bits where it derives the table from num_bits itself, 256 otherwise), so the mask only
// keeps a caller's mistaken nbins inside the table.  The code is the fp32 one, taken before the down-conversion.  NaN and the
// infinities take k_qdq<HIST>'s path, as k_cl_qdq_hist's comment states it: a NaN's code is NaN, differs from the zero point, and
// (int)NaN == 0 counts it in bin 0; +inf clamps to qmax and -inf to 0 before the count (a channel that holds one is outside
// qdq_fast_domain: the IEEE divide).
#pragma once
#include "cnnq_half.hip.h"
#include "cnnq_half_midtread.hip.h"

namespace {

// h_qdq_piece with the count: the same two quotients, the same bits of y
template <class T, int W>
__device__ __forceinline__ void h_qdq_hist_piece(uint16_t (&e)[W], bool fast, float sc, float rs, float zp, float qm,
                                                 unsigned* sh_hist, unsigned& nzp, unsigned mask) {
    if (fast) {
        if constexpr (W == 1) {
            float cd;
            e[0] = h_down(T{}, qdq1_fast(h_up(T{}, e[0]), sc, rs, zp, qm, cd));
            xhist_add(sh_hist, cd, zp, nzp, mask);
        } else {
            const f2v s2 = {sc, sc}, r2 = {rs, rs}, z2 = {zp, zp};
#pragma unroll
            for (int i = 0; i < W; i += 2) {
                f2v cd;
                const f2v o = qdq2_fast(f2v{h_up(T{}, e[i]), h_up(T{}, e[i + 1])}, s2, r2, z2, qm, cd);
                e[i] = h_down(T{}, o.x);
                e[i + 1] = h_down(T{}, o.y);
                xhist_add(sh_hist, cd.x, zp, nzp, mask);
                xhist_add(sh_hist, cd.y, zp, nzp, mask);
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < W; ++i) {
            float cd;
            e[i] = h_down(T{}, qdq1(h_up(T{}, e[i]), sc, zp, qm, cd));
            xhist_add(sh_hist, cd, zp, nzp, mask);
        }
    }
}

// the end of a counting workgroup that lies in one channel: the lane's count of the zero point's code, the barrier, the fold
__device__ __forceinline__ void h_hist_flush(unsigned* sh_hist, unsigned long long* __restrict__ hist, int nbins, float zp,
                                             unsigned nzp, unsigned mask) {
    const float z[1] = {zp};
    const unsigned n[1] = {nzp};
    xhist_add_zp<1>(sh_hist, z, n, mask);
    __syncthreads();
    if ((int)threadIdx.x < nbins) xhist_fold(sh_hist, hist, xhist_replica());
}

// k_h_qdq with the count: the same two sources of parameters (the table qp, or k_h_minmax's partials merged in the prologue with
// h_params and published by the first split), the same tiling, descending dispatch, non-temporal load and store, and the same
// choice of quotient - so the same y.  hist: the XHIST_REPLICAS replica tables; the launch ADDS to them.
// A workgroup's flush is up to nbins global atomics, so the launch takes longer parts than k_h_qdq's (h_geo_hist).
// The divide-free branch is kept: with the IEEE divide everywhere config 2 measured slower where the pass is short of issue slots -
// [512,64,112,112] 507.6 (506.5-509.1) against 480.7 (477.7-482.3) us, [512,128,56,56] 240.0 (238.8-241.4) against 224.0
// (223.2-224.6), the resident form on [512,256,14,14] 50.3 (49.6-50.7) against 46.5 (46.1-47.1) - and level elsewhere.
template <class T, int W>
__global__ void __launch_bounds__(TPB) k_h_qdq_hist(const uint16_t* __restrict__ x, uint16_t* __restrict__ y, const HGeo g,
                                                    const float* __restrict__ qp, const float* __restrict__ pmm, const HArgs ha,
                                                    const int nbins, unsigned long long* __restrict__ hist) {
    extern __shared__ unsigned cnnq_dyn_lds[];       // nbins x HREP words, sized by the launch
    unsigned* sh_hist = cnnq_dyn_lds;
    const unsigned mask = (unsigned)nbins - 1u;
    xhist_zero(sh_hist, nbins);
    const HPart t = h_part<W, false>(g, (int)gridDim.x - 1 - (int)blockIdx.x);
    const int c = t.c;
    float sc, zp, qm;
    bool fast = false;
    if (pmm) {
        float mn = INFINITY, mx = -INFINITY;
        for (int i = 0; i < ha.npairs; ++i) {
            mn = pmin(mn, pmm[(size_t)(2 * i) * g.C + c]);
            mx = pmax(mx, pmm[(size_t)(2 * i + 1) * g.C + c]);
        }
        h_params(mn, mx, ha.num_bits, ha.positive, sc, zp, qm);
        fast = qdq_fast_domain(mn, mx, sc);
        if (t.s == 0 && threadIdx.x == 0) h_publish(ha, g.C, c, mn, mx, sc, zp, qm);
    } else {
        h_qp(qp, g.C, c, sc, zp, qm);
    }
    const bool ufast = __builtin_amdgcn_readfirstlane((int)fast) != 0;
    const float rs = ufast ? uniform_f(1.0f / sc) : 0.f;
    __syncthreads();                                 // the table is zero
    unsigned nzp = 0u;
    const size_t P = (size_t)g.C * (size_t)g.HW;
    HWalk w = h_walk(g.ppr);
    for (; w.r < t.rows; h_step(w, g.ppr)) {
        const size_t off = t.off + (size_t)w.r * P + (size_t)w.p * W;
        uint16_t e[W];
        h_ld<W, true>(x + off, e);
        h_qdq_hist_piece<T, W>(e, ufast, sc, rs, zp, qm, sh_hist, nzp, mask);
        h_st_nt<W>(y + off, e);
    }
    h_hist_flush(sh_hist, hist, nbins, zp, nzp, mask);
}

// k_h_whole with the count: config 2 in ONE launch and one read of x (4 B/elem) on the resident tile - extrema, h_params, then
// Q/DQ and count out of the registers.  k_h_whole's domain (N * HW <= h_whole_cap, W >= 2).  HTPB lanes and nbins <= 256: the fold
// is the first nbins threads'.  The table is zeroed before the load; the extrema's fold has the barrier behind it.
template <class T, int W, int K>
__global__ void __launch_bounds__(HTPB) k_h_whole_hist(const uint16_t* __restrict__ x, uint16_t* __restrict__ y, const HGeo g,
                                                       const HArgs ha, const int nbins, unsigned long long* __restrict__ hist) {
    __shared__ float l_mn[HTPB / 64], l_mx[HTPB / 64];
    extern __shared__ unsigned cnnq_dyn_lds[];       // nbins x HREP words, sized by the launch
    unsigned* sh_hist = cnnq_dyn_lds;
    const unsigned mask = (unsigned)nbins - 1u;
    const int c = (int)blockIdx.x;
    xhist_zero(sh_hist, nbins);
    HTile<W, K> tile(g);
    float mn = INFINITY, mx = -INFINITY;
    bool nan = false;
    tile.load(x + (size_t)c * g.HW, [&](const uint16_t (&e)[W]) { h_mm_piece<T, W>(e, mn, mx, nan); });
    if (nan) { mn = NAN; mx = NAN; }
    h_fold_mm(l_mn, l_mx, mn, mx);
    float sc, zp, qm;
    h_params(mn, mx, ha.num_bits, ha.positive, sc, zp, qm);
    if (threadIdx.x == 0) h_publish(ha, g.C, c, mn, mx, sc, zp, qm);
    const bool ufast = __builtin_amdgcn_readfirstlane((int)qdq_fast_domain(mn, mx, sc)) != 0;
    const float rs = ufast ? uniform_f(1.0f / sc) : 0.f;
    unsigned nzp = 0u;
    tile.template store<false>(y + (size_t)c * g.HW, [&](uint16_t (&e)[W]) {
        h_qdq_hist_piece<T, W>(e, ufast, sc, rs, zp, qm, sh_hist, nzp, mask);
    });
    h_hist_flush(sh_hist, hist, nbins, zp, nzp, mask);
}

// ---- host side: the tile of the counting pass and which classes of layer run where (cnnq_pc_route_qdq_hist_dt's route word),
// functions of N, C, HW, the dtype and the bins alone
inline size_t h_hist_lds(int nbins) { return (size_t)nbins * HREP * sizeof(unsigned); }

//
// The yardsticks are the legs of one run (tools/bench_half_entropy.py: MI355X, the twelve classes of ResNet-50 conv outputs at
// batch 512, int4, configs 2 and 3 with -me, us per call, mean (min-max) over three rounds of five steps, the legs alternating
// step by step); a class changes route only where it wins beyond that spread.  profiles/half_entropy.md has every figure.
//
// Elements per workgroup of k_h_qdq_hist: a workgroup zeroes nbins x HREP words of LDS and hands over up to nbins global atomics,
// so it walks four of k_h_qdq's tiles where that leaves enough workgroups - k_h_mt_qdq<HIST>'s rule (h_mt_hist_elems), measured
// here against both fixed lengths (config 2, bf16, the statistics launch and this pass): k_h_qdq's 8192 everywhere lost on every
// long row - [512,64,112,112] 541.8 (540.9-543.6) against 480.7 (477.7-482.3), [512,128,56,56] 261.5 (260.1-264.0) against 224.0
// (223.2-224.6), [512,64,56,56] 175.1 (174.5-175.4) against 144.0 (143.6-144.3), [512,512,28,28] 257.6 (257.4-258.0) against 242.7
// (242.0-243.7); 32768 everywhere lost on the short rows - [512,512,7,7] 108.8 (108.6-109.2) against 73.9 (72.9-75.2),
// [512,2048,7,7] 208.7 (208.5-208.9) against 202.0 (201.5-202.4), [512,1024,14,14] 175.8 (175.4-176.0) against 170.6 (170.1-170.9)
// - and won only [512,128,28,28], 82.4 (81.7-83.3) against 86.4 (85.8-87.4), which the rule leaves at the short tile.
inline HGeo h_geo_hist(int64_t N, int64_t C, int64_t HW, int w) {
    return h_geo(N, C, HW, w, h_splits(N, C, HW, h_mt_hist_elems(N, C, HW), N), 1);
}

inline bool h_ent_whole_fits(int64_t N, int64_t HW, int w) { return N * HW <= h_whole_cap(w); }
// The resident form against the two launches (allow_single_launch = 1).  It won beyond the spread on [512,256,14,14] in all four
// runs (bf16 46.5 (46.1-47.1) against 57.3 (56.6-58.0); fp16 46.8 (46.0-47.9) against 56.7 (56.1-57.7)).  On [512,512,14,14] it won
// in three of four (bf16 92.8 (92.4-93.4) against 96.4 (96.1-97.0)) and overlapped in one (fp16 98.6 (97.6-99.9) against 99.5
// (98.8-100.1)); on [512,1024,14,14] it lost in all four (180.4 (180.0-181.1) against 170.6 (170.1-170.9)): C workgroups of 1024
// lanes run in rounds of 256, and each hands its histogram over at its end.  So: 256 channels at that population, h_mt_whole_wins'
// rule; other populations and fewer channels were not measured and stay on the two launches.
inline int h_ent_whole_wins(int64_t N, int64_t C, int64_t HW, int dtype, int nbins) {
    (void)dtype; (void)nbins;
    return C == 256 && N * HW >= 100352;
}
// The classes that run native against the upcast route: native won beyond the spread on every class with an even HW, in both
// dtypes and both configurations - from 0.29 x ([512,256,56,56] fp16 config 2: 428.0 (425.8-430.8) against 1478.2 (1476.8-1479.8))
// to 0.63 x ([512,256,14,14] config 3: 82.5 (81.0-83.7) against 131.1 (130.9-131.4)).  An odd HW loads single 2-byte elements
// whatever the alignment (h_stats_native's finding), and the two 7x7 classes did not win: [512,512,7,7] lost in all eight runs
// (config 2 bf16 73.9 (72.9-75.2) against 71.1 (70.1-72.3); config 3 105.2 (104.3-106.8) against 96.7 (95.2-97.6)); [512,2048,7,7]
// lost in all four of config 3 (248.8 (246.7-252.1) against 243.0 (242.2-244.5)), and in config 2 the pass won by 3 to 5 % (202.0
// (201.5-202.4) against 207.9 (207.8-208.1)) but the call the quantizer makes was inside the spread in two runs of four (208.9
// (207.4-210.4) against 207.9 (207.8-208.1)).  So h_aciq_native's rule holds here too: odd rows stay on the upcast route from a
// population of 6272 on (the smallest that did not win there); smaller ones were not measured and stay native.
inline int h_ent_native(int64_t N, int64_t C, int64_t HW, int dtype, int nbins) {
    (void)C; (void)dtype; (void)nbins;
    return !(HW % 2 == 1 && N * HW >= 6272);
}

}  // namespace
