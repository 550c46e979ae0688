// cnnq_half_aciq.hip.h - dynamic ACIQ clipping (config 3: -c laplace / gaus, optionally -baa; int_quantizer.py:327-352, 409-451,
// 557-603) on CONTIGUOUS bf16 / fp16 activations x[N][C][HW]: the resident form - statistics, clipping, parameters and Q/DQ of a
// channel whose whole batch population fits one workgroup's registers, in one launch that reads x once - and which classes of
// layer run where.  Part of the single translation unit cnnq_kernels.hip (see its header for the design).
//
// The chain form has no kernel of its own: k_h_moments -> k_combine (-> k_h_absdev<KURT = false> -> k_combine_dev) -> k_params ->
// k_h_qdq, the launches of cnnq_pc_stats_dt, cnnq_pc_params and cnnq_pc_qdq_dt driven from one host call (cnnq_pc_aciq_qdq_dt).
//
// The contract: rows MIN / MAX of the table exact (every element is upconverted exactly; torch's NaN rule),
// MEAN / STD / B within the statistics tier of fp64, and given the published table every output bit for bit - qp and diag are
// channel_params' arithmetic (the single definition k_params runs per table row), y is k_h_qdq's on the published qp.  The tile
// (HTile), the piece arithmetic of both statistics passes (h_mom_piece, k_h_absdev's), the folds (h_fold_mm, h_fold_sums) and the
// rounding of the merged sums (mean_of, std_of, b_of: what k_combine / k_combine_dev call) are the family's shared ones.  The
// order of every addition follows from HGeo alone: no atomics, no exchange between workgroups, run after run the same bits - but
// not the chain's order, so the two routes' MEAN / STD / B agree within the tier, not bit for bit.
#pragma once
#include "cnnq_half_stats.hip.h"
#include "cnnq_params.hip.h"
#include "cnnq_aciq.hip.h"

namespace {

struct HAciqArgs {
    cnnq_params_cfg cfg;
    const float* bits;   // TABLE: [C] allocated widths (k_bitalloc), or null: cfg.num_bits everywhere
    float* stats;        // [CNNQ_NSTAT][C]: written completely (TABLE: rows MIN, MAX, MEAN, STD are read, row B is written)
    float* qp;           // [CNNQ_NQP][C] out
    float* diag;         // [CNNQ_NDIAG][C] out, may be null
};

// sum |x - mean| of one piece into the two running sums of its lane: k_h_absdev<KURT = false>'s arithmetic - the fp32 subtract
// (packed, two elements per instruction), |d| into fp64, the two elements of a pair a running sum each
template <class T, int W>
__device__ __forceinline__ void h_absdev_piece(const uint16_t (&e)[W], const float mean, double& sa0, double& sa1) {
    typedef float f2 __attribute__((ext_vector_type(2)));
    const f2 m2 = {mean, mean};
#pragma unroll
    for (int i = 0; i < W; i += 2) {
        const f2 d = f2{h_up(T{}, e[i]), h_up(T{}, e[i + 1])} - m2;
        sa0 += (double)fabsf(d.x);
        sa1 += (double)fabsf(d.y);
    }
}

// f(e) on each held piece, as HTile::each, for a kernel that walks its tile in more than two phases: the walk starts from an
// opaque copy of the first pair and every piece is unpacked from an opaque copy, HTile::store<true>'s two measures - or the
// compiler keeps the K predicates of the walk (K = 64: more scalar registers than there are) and the fp32 values an earlier
// phase upconverted alive across the folds in between, and the tile no longer fits the registers
template <int W, int K, class F>
__device__ __forceinline__ void h_each_again(HTile<W, K>& tile, F&& f) {
    HWalk w = tile.w0;
    asm volatile("" : "+v"(w.r), "+v"(w.p));
    tile.walk(w, [&](int k, const HWalk&) {
        typename HTile<W, K>::S tk = tile.t[k];
        asm volatile("" : "+v"(tk));
        uint16_t e[W];
        HTile<W, K>::unpack(tk, e);
        f(e);
    });
}

// Config 3 for channels whose whole batch population fits one workgroup's registers, on k_h_whole's resident tile (HTile): one
// HTPB-lane workgroup per channel, x read once.
//   1. load and moments (h_mom_piece<RELU = false>, k_h_moments' NaN rule and folds), mean and std as k_combine forms them
//      (mean_of / std_of on the workgroup's sums; the count is N * HW, what the chain's counts add up to).  TABLE: the phase
//      is skipped - rows MIN / MAX / MEAN / STD of the merged table of a pass A in front (the bit allocation between the two
//      needs every channel's std) and bits[c] are read instead;
//   2. Laplace clipping only: sum |x - mean| out of the registers, folded; b as k_combine_dev forms it (b_of);
//   3. channel_params - uniform per workgroup; lane 0 publishes the channel's column of stats, qp and diag;
//   4. Q/DQ out of the registers (h_qdq_piece: the divide-free quotient inside aciq_fast_domain - there the bits of the IEEE
//      divide k_h_qdq runs on a table - else the divide), store.
// No exchange, no workspace, no atomics.
template <class T, int W, int K, bool TABLE>
__global__ void __launch_bounds__(HTPB) k_h_aciq_whole(const uint16_t* __restrict__ x, uint16_t* __restrict__ y, const HGeo g,
                                                       const HAciqArgs a) {
    __shared__ float l_mn[HTPB / 64], l_mx[HTPB / 64];
    __shared__ double l_s[1][HTPB / 64], l_q[1][HTPB / 64];
    __shared__ double l_b[1][HTPB / 64];
    const int c = (int)blockIdx.x;
    const int C = g.C;
    const double cnt = (double)g.N * (double)g.HW;
    HTile<W, K> tile(g);
    float vmin, vmax, vmean, vstd, vb = 0.f;
    if constexpr (TABLE) {
        tile.load(x + (size_t)c * g.HW);
        vmin = a.stats[(size_t)CNNQ_STAT_MIN * C + c];
        vmax = a.stats[(size_t)CNNQ_STAT_MAX * C + c];
        vmean = a.stats[(size_t)CNNQ_STAT_MEAN * C + c];
        vstd = a.stats[(size_t)CNNQ_STAT_STD * C + c];
    } else {
        Mom m;
        m.init();
        tile.load(x + (size_t)c * g.HW);
        h_each_again(tile, [&](const uint16_t (&e)[W]) { h_mom_piece<T, W, false>(m, e); });
        if (m.ss != m.ss) { m.mn = NAN; m.mx = NAN; }
        // the three folds one after the other, each finished before the next reads its 16 partials: read together (one
        // h_fold_sums of both sums behind h_fold_mm) they take 96 registers on top of the tile's 64 and the tile spills.  Each
        // sum's order of additions is h_fold_sums' either way.
        h_fold_mm(l_mn, l_mx, m.mn, m.mx);
        asm volatile("" : "+v"(m.mn), "+v"(m.mx));
        double vs[1] = {m.s}, vq[1] = {m.ss};
        h_fold_sums(l_s, vs);
        asm volatile("" : "+v"(vs[0]));
        h_fold_sums(l_q, vq);
        const MomSum r{(double)m.mn, (double)m.mx, vs[0], vq[0], cnt, 0., 0.};
        vmin = m.mn;
        vmax = m.mx;
        vmean = mean_of(r);
        vstd = std_of(r);
        // both finished here: left to the scheduler, the second sum's 16 partials wait in registers for the std until phase 3
        asm volatile("" : "+v"(vmean), "+v"(vstd));
    }
    if (a.cfg.clip == 1) {
        const float mean = uniform_f(vmean);
        double sa0 = 0., sa1 = 0.;
        h_each_again(tile, [&](const uint16_t (&e)[W]) { h_absdev_piece<T, W>(e, mean, sa0, sa1); });
        double v[1] = {sa0 + sa1};
        h_fold_sums(l_b, v);
        vb = b_of(v[0], cnt);
    }
    const bool ba = a.cfg.bit_alloc && a.cfg.num_bits <= 4;
    const float bits = (TABLE && a.bits) ? a.bits[c] : (float)a.cfg.num_bits;
    const ChanParams cp = channel_params(a.cfg, ba, bits, vmin, vmax, vmean, vstd, vb);
    if (threadIdx.x == 0) {
        if constexpr (!TABLE) {
            a.stats[(size_t)CNNQ_STAT_MIN * C + c] = vmin;
            a.stats[(size_t)CNNQ_STAT_MAX * C + c] = vmax;
            a.stats[(size_t)CNNQ_STAT_MEAN * C + c] = vmean;
            a.stats[(size_t)CNNQ_STAT_STD * C + c] = vstd;
            a.stats[(size_t)CNNQ_STAT_STD_POS * C + c] = 0.f;
            a.stats[(size_t)CNNQ_STAT_KURT * C + c] = 0.f;
        }
        // the table is written completely: B is zero unless phase 2 ran (TABLE: k_combine left the zero)
        if (!TABLE || a.cfg.clip == 1) a.stats[(size_t)CNNQ_STAT_B * C + c] = vb;
        a.qp[(size_t)CNNQ_QP_SCALE * C + c] = cp.scale;
        a.qp[(size_t)CNNQ_QP_ZP * C + c] = cp.zp;
        a.qp[(size_t)CNNQ_QP_QMAX * C + c] = cp.qmax;
        if (a.diag) {
            a.diag[(size_t)CNNQ_DIAG_BITS * C + c] = bits;
            a.diag[(size_t)CNNQ_DIAG_ALPHA * C + c] = cp.alpha;
            a.diag[(size_t)CNNQ_DIAG_DELTA * C + c] = cp.delta;
            a.diag[(size_t)CNNQ_DIAG_OFFSET * C + c] = cp.offset;
        }
    }
    const bool ufast = __builtin_amdgcn_readfirstlane((int)aciq_fast_domain(vmin, vmax, cp)) != 0;
    const float sc = uniform_f(cp.scale), zp = uniform_f(cp.zp), qm = uniform_f(cp.qmax);
    const float rs = ufast ? uniform_f(1.0f / sc) : 0.f;
    // the upconversions again, from an opaque copy of each piece (k_h_bcorr_whole says why)
    tile.template store<true>(y + (size_t)c * g.HW, [&](uint16_t (&e)[W]) { h_qdq_piece<T, W>(e, ufast, sc, rs, zp, qm); });
}

// ---- host side: which classes of layer run where (cnnq_pc_route_aciq_dt's route word), functions of N, C, HW, the dtype and the
// configuration alone
inline bool h_aciq_whole_fits(int64_t N, int64_t HW, int w) { return N * HW <= h_whole_cap(w); }
// The yardsticks are the routes of the same run (tools/bench_half_aciq.py: MI355X, -c laplace at int4, us per call, mean (min-max),
// 20 steps after 3, the routes alternating step by step); a class changes route only where it wins beyond that spread.
// profiles/half_aciq.md has every figure.
//
// The resident form puts one 1024-lane workgroup on a CU, which loads, reduces and stores in turn: C workgroups run in rounds of
// 256.  Against the chain it won in every measurement from a population of 65536 per channel and 128 channels on - with bit
// allocation (route 3: pass A and k_bitalloc stay in front) up to 512 channels: bf16 [512,512,14,14] 118.8 (116.1-121.3) against
// 129.4 (127.0-132.6), [512,256,14,14] 66.8 (64.5-70.5) against 79.6 (76.0-82.2), [128,512,28,28] 92.3 (85.8-96.8) against 105.9
// (104.3-109.3), [128,128,28,28] 42.4 (39.7-44.0) against 48.4 (46.9-51.0), [32,256,56,56] 49.2 (45.0-51.4) against 65.4
// (60.8-69.9), fp16 alike, but not at 1024 channels ([512,1024,14,14] 217.9 (210.4-225.0) against 230.0 (223.6-267.0), fp16 216.7
// (210.5-225.8) against 228.6 (224.9-233.7): inside the spread); without it (route 1: one launch, one read) up to 1024 channels:
// [512,1024,14,14] 183.6 (178.1-191.4) against 215.4 (211.8-220.8), [512,256,14,14] 49.6 (44.8-52.4) against 74.4 (73.2-76.4).
// At a population of 25088 it won at 256 channels ([128,256,14,14] 41.6 (39.7-43.8) against 48.5 (44.5-50.9), [32,256,28,28] 34.9
// (30.2-36.5) against 41.9 (40.5-44.3); without bit allocation also at 512: [128,512,14,14] 46.1 (43.8-49.2) against 51.7
// (49.9-54.5)), was inside the spread at 128 and, with bit allocation, at 512 channels, and lost at 1024 (84.7 against 83.6; 79.3
// against 74.1 without).  Below that, and at 64 channels, it lost or stayed inside the spread ([32,1024,14,14] 65.1 against 48.6).
inline int h_aciq_whole_wins(int64_t N, int64_t C, int64_t HW, int dtype, bool ba) {
    (void)dtype;
    const int64_t pop = N * HW;
    if (C < 128) return 0;
    if (pop >= 65536) return C <= (ba ? 512 : 1024);
    return pop >= 25088 && C >= 256 && C <= (ba ? 256 : 512);
}
// Against the upcast route the chain won beyond the spread on the 10 classes of ResNet-50 b512 conv outputs with an even HW in
// both dtypes, from 0.33 x ([512,256,56,56] bf16 574.1 (561.8-586.0) against 1752.2 (1733.3-1765.1)) to 0.63 x ([512,256,14,14]
// 79.6 (76.0-82.2) against 126.6 (124.7-129.8)).  An odd HW loads single 2-byte elements whatever the alignment (h_stats_native's
// finding), and four passes of that walk lose where a channel's population is large: [512,2048,7,7] bf16 259.5 (256.0-264.2)
// against 236.1 (232.2-240.4), [512,512,7,7] 103.3 (101.0-107.6) against 88.7 (86.0-98.7), fp16 alike; at batch 128 (a
// population of 6272) the two are inside each other's spread (92.1 (89.6-101.2) against 92.3 (89.0-98.4); 52.9 (51.6-57.7) against
// 57.7 (54.1-61.6)), at batch 32 (1568) the chain wins (52.6 (51.0-55.2) against 60.2 (56.9-65.6); 34.1 (32.2-35.8) against 45.9
// (42.9-54.6)).  So odd rows stay on the upcast route from the smallest population that did not win; smaller ones were not
// measured in between and stay native.
inline int h_aciq_native(int64_t N, int64_t C, int64_t HW, int dtype) {
    (void)C; (void)dtype;
    return !(HW % 2 == 1 && N * HW >= 6272);
}

}  // namespace
