// cnnq_half_midtread.hip.h - config 5 (mid-tread quantization with per-channel bin allocation, and the entropy of its codes:
// -c laplace -baa -mtq [-me]; int_quantizer.py:170-225) on CONTIGUOUS bf16 / fp16 activations x[N][C][HW]: the table-driven Q/DQ
// pass with the code histogram, its resident form - b, step size, clamp bounds and Q/DQ of a channel whose whole batch population
// fits one workgroup's registers, in one launch that reads x once - and which classes of layer run where.  Part of the single
// translation unit cnnq_kernels.hip (see its header for the design).
//
// Everything around the two kernels is the family's: the statistics table comes from k_h_moments / k_h_absdev through k_combine /
// k_combine_dev (cnnq_pc_stats_dt), omega, the clipping multiplier and the histogram window from k_mt_params, the entropy from
// k_mt_entropy / k_mt_entropy_batch on the histogram written here.
//
// The contract: given the published table mt[CNNQ_NMT][C], y and every word of the histogram but the split
// of the window counts over the replica tables are, bit for bit, k_mt_qdq's with CLIP = true on x.float(), y rounded once into
// the element type; rows DELTA / CMIN / CMAX of mt are mt_channel's arithmetic (the single definition k_mt_params runs per table
// row) on the published statistics, on both routes.
#pragma once
#include "cnnq_half_aciq.hip.h"
#include "cnnq_midtread.hip.h"

namespace {

// a channel's step size and clamp bounds, uniform per workgroup; histogram: whether a bound is a value of its own (not an
// integer code) and the first code of the window
struct HMtChan {
    float d, lo, hi;
    bool hi_ni, lo_ni;
    int wstart;
};
template <bool HIST>
__device__ __forceinline__ HMtChan h_mt_chan(float d, float lo, float hi, const float* __restrict__ mt, int C) {
    HMtChan ch{uniform_f(d), uniform_f(lo), uniform_f(hi), false, false, 0};
    if constexpr (HIST) {
        ch.hi_ni = ch.hi != rintf(ch.hi);
        ch.lo_ni = ch.lo != rintf(ch.lo);
        ch.wstart = __builtin_amdgcn_readfirstlane((int)mt[(size_t)CNNQ_MT_WSTART * C]);
    }
    return ch;
}

// what a lane counts in registers: code 0 (the mode of the distribution) and the clamps to a non-integer bound (nlo: or a NaN)
struct HMtCount {
    unsigned nzero = 0, nhi = 0, nlo = 0;
};

// the workgroup's LDS table of the window bins (mt_hist_zero) and its two clamp counters, zeroed (one barrier)
template <int NT>
__device__ __forceinline__ void h_mt_hist_init(unsigned (&sh_hist)[MT_WORDS], unsigned (&sh_c)[2]) {
    mt_hist_zero<NT>(sh_hist);
    if (threadIdx.x < 2) sh_c[threadIdx.x] = 0u;
    __syncthreads();
}

// one piece through y = clamp(rint(x / delta), c_min, c_max) * delta (iq.py:202-224) on the upconverted value, rounded once into
// the element type.  The code and, with HIST, its count are k_mt_qdq<CLIP = true>'s own definitions (mt_code, mt_hist_count in
// cnnq_midtread.hip.h); a NaN goes to the channel's c_min counter, here the lane's own.
template <class T, int W, bool HIST>
__device__ __forceinline__ void h_mt_piece(uint16_t (&e)[W], const HMtChan& ch, HMtCount& n, unsigned* __restrict__ sh_hist,
                                           unsigned long long* __restrict__ hist, int C) {
#pragma unroll
    for (int i = 0; i < W; ++i) {
        const float t = mt_code<true>(h_up(T{}, e[i]) / ch.d, ch.lo, ch.hi);
        e[i] = h_down(T{}, t * ch.d);                            // iq.py:224
        if constexpr (HIST)
            mt_hist_count<true>(t, ch.lo, ch.hi, ch.lo_ni, ch.hi_ni, ch.wstart, sh_hist, hist, C, n.nzero, n.nhi, n.nlo, [&] { n.nlo += 1u; });
    }
}

// What a workgroup of NT lanes hands over at its end: its count of code 0 and the live window bins into replica table `rep`
// (mt_hist_zero_code, mt_hist_fold), and - the workgroup lies in one channel, so the lanes' two clamp counters are folded: the xor
// tree inside the wave, the waves through LDS - one atomic per bound that was hit.
template <int NT>
__device__ __forceinline__ void h_mt_flush(unsigned (&sh_hist)[MT_WORDS], unsigned (&sh_c)[2], HMtCount n, const HMtChan& ch, int c, int C,
                                           unsigned long long* __restrict__ hist, int rep_id) {
    const int tid = (int)threadIdx.x;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        n.nhi += (unsigned)__shfl_xor((int)n.nhi, m, 64);
        n.nlo += (unsigned)__shfl_xor((int)n.nlo, m, 64);
    }
    if ((tid & 63) == 0) {
        if (n.nlo) atomicAdd(&sh_c[0], n.nlo);
        if (n.nhi) atomicAdd(&sh_c[1], n.nhi);
    }
    mt_hist_zero_code(sh_hist, hist, C, ch.wstart, n.nzero);
    __syncthreads();
    if (tid == 0) {
        if (sh_c[0]) atomicAdd(&hist[MT_NB + 2 + c], (unsigned long long)sh_c[0]);
        if (sh_c[1]) atomicAdd(&hist[MT_NB + 2 + C + c], (unsigned long long)sh_c[1]);
    }
    mt_hist_fold<NT>(sh_hist, hist, C, ch.wstart, rep_id);
}

// The table-driven pass: k_h_qdq's tiling - a workgroup is one (channel, batch split) of whole rows, W = 8 / 4 / 2 / 1, x read and
// y written non-temporally, workgroups in descending address order - with delta, c_min, c_max of mt[CNNQ_NMT][C] uniform per
// workgroup.  HIST: the fp32 codes are counted into k_mt_qdq's histogram (layout and rules: the note above k_mt_qdq), the flush
// into replica table (workgroup id & (MT_GR - 1)); hist is zeroed by the caller.
template <class T, int W, bool HIST>
__global__ void __launch_bounds__(TPB) k_h_mt_qdq(const uint16_t* __restrict__ x, uint16_t* __restrict__ y, const HGeo g,
                                                  const float* __restrict__ mt, unsigned long long* __restrict__ hist) {
    __shared__ unsigned sh_hist[HIST ? MT_WORDS : 1];
    __shared__ unsigned sh_c[2];
    if constexpr (HIST) h_mt_hist_init<TPB>(sh_hist, sh_c);
    const HPart t = h_part<W, false>(g, (int)gridDim.x - 1 - (int)blockIdx.x);
    const int c = t.c;
    const HMtChan ch = h_mt_chan<HIST>(mt[(size_t)CNNQ_MT_DELTA * g.C + c], mt[(size_t)CNNQ_MT_CMIN * g.C + c],
                                       mt[(size_t)CNNQ_MT_CMAX * g.C + c], mt, g.C);
    HMtCount n;
    const size_t P = (size_t)g.C * (size_t)g.HW;
    HWalk w = h_walk(g.ppr);
    for (; w.r < t.rows; h_step(w, g.ppr)) {
        const size_t off = t.off + (size_t)w.r * P + (size_t)w.p * W;
        uint16_t e[W];
        h_ld<W, true>(x + off, e);
        h_mt_piece<T, W, HIST>(e, ch, n, sh_hist, hist, g.C);
        h_st_nt<W>(y + off, e);
    }
    if constexpr (HIST) h_mt_flush<TPB>(sh_hist, sh_c, n, ch, c, g.C, hist, (int)blockIdx.x);
}

// The histogram zeroed by a launch, not by hipMemsetAsync: captured in a graph, the memset node of a buffer this size (1.3 MB) wrote
// a stale 16-byte pattern from its second replay on (seen on ROCm 7 / MI355X: every word of hist held two addresses of an
// unrelated copy enqueued between the replays), and the entropy of a replayed call was garbage.  A kernel node replays as launched.
__global__ void __launch_bounds__(TPB) k_h_mt_zero(unsigned long long* __restrict__ hist, const size_t n) {
    for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < n; i += (size_t)gridDim.x * TPB) hist[i] = 0ull;
}

struct HMtArgs {
    MtCfg cfg;
    float* stats;               // [CNNQ_NSTAT][C]: rows MIN, MAX, MEAN, STD of pass A's merge are read, row B is written
    float* mt;                  // [CNNQ_NMT][C]: rows OMEGA, ALPHA, WSTART from k_mt_params<GUESS>; DELTA, CMIN, CMAX written here
    unsigned long long* hist;   // CNNQ_MT_HIST_WORDS(C), zeroed by the caller; null without HIST
};

// Config 5 for channels whose whole batch population fits one workgroup's registers, on the resident tile (HTile): one HTPB-lane
// workgroup per channel behind pass A and k_mt_params<GUESS> (the bin allocation couples all channels through their std: there
// is no route without pass A), x read once by this launch.
//   1. load; rows MIN / MAX / MEAN / STD of the merged table and OMEGA / ALPHA of mt are read;
//   2. sum |x - mean| out of the registers (h_absdev_piece), folded; b as k_combine_dev forms it (b_of);
//   3. mt_channel - uniform per workgroup; lane 0 publishes row B of stats and rows DELTA / CMIN / CMAX of mt;
//   4. Q/DQ out of the registers (h_mt_piece), store; HIST: the codes counted, the flush.
// No exchange between workgroups, no workspace.  WSTART is k_mt_params<GUESS>'s: the bound a Laplace channel would have, so only
// the speed of the histogram depends on it (the note above k_mt_params).
template <class T, int W, int K, bool HIST>
__global__ void __launch_bounds__(HTPB) k_h_mt_whole(const uint16_t* __restrict__ x, uint16_t* __restrict__ y, const HGeo g,
                                                     const HMtArgs a) {
    __shared__ double l_b[1][HTPB / 64];
    __shared__ unsigned sh_hist[HIST ? MT_WORDS : 1];
    __shared__ unsigned sh_c[2];
    const int c = (int)blockIdx.x;
    const int C = g.C;
    const double cnt = (double)g.N * (double)g.HW;
    HTile<W, K> tile(g);
    tile.load(x + (size_t)c * g.HW);
    if constexpr (HIST) h_mt_hist_init<HTPB>(sh_hist, sh_c);
    const float vmin = a.stats[(size_t)CNNQ_STAT_MIN * C + c];
    const float vmax = a.stats[(size_t)CNNQ_STAT_MAX * C + c];
    const float vmean = a.stats[(size_t)CNNQ_STAT_MEAN * C + c];
    const float omega = a.mt[(size_t)CNNQ_MT_OMEGA * C + c];
    const float am = a.mt[(size_t)CNNQ_MT_ALPHA * C + c];
    const float mean = uniform_f(vmean);
    double sa0 = 0., sa1 = 0.;
    h_each_again(tile, [&](const uint16_t (&e)[W]) { h_absdev_piece<T, W>(e, mean, sa0, sa1); });
    double v[1] = {sa0 + sa1};
    h_fold_sums(l_b, v);
    const float vb = b_of(v[0], cnt);
    const MtChan mc = mt_channel(a.cfg, omega, am, vmin, vmax, vmean, vb);
    if (threadIdx.x == 0) {
        a.stats[(size_t)CNNQ_STAT_B * C + c] = vb;
        a.mt[(size_t)CNNQ_MT_DELTA * C + c] = mc.delta;
        a.mt[(size_t)CNNQ_MT_CMIN * C + c] = mc.cmin;
        a.mt[(size_t)CNNQ_MT_CMAX * C + c] = mc.cmax;
    }
    const HMtChan ch = h_mt_chan<HIST>(mc.delta, mc.cmin, mc.cmax, a.mt, C);
    HMtCount n;
    // the upconversions again, from an opaque copy of each piece (k_h_bcorr_whole says why)
    tile.template store<true>(y + (size_t)c * g.HW, [&](uint16_t (&e)[W]) { h_mt_piece<T, W, HIST>(e, ch, n, sh_hist, a.hist, C); });
    if constexpr (HIST) h_mt_flush<HTPB>(sh_hist, sh_c, n, ch, c, C, a.hist, c);
}

// ---- host side: the tile of the table-driven pass and which classes of layer run where (cnnq_pc_route_midtread_dt's route
// word), functions of N, C, HW, the dtype and whether the codes are counted alone
//
// The yardsticks are the routes of the same run (tools/bench_half_midtread.py and the tile sweep next to it: MI355X, the conv
// outputs of VGG-16 and ResNet-50 at batch 512, -bata 5.3 and 4, with and without -me, us per call, mean (min-max), 20 steps after
// 3, the routes alternating step by step); a class changes route only where it wins beyond that spread.
// profiles/half_midtread.md has every figure.
//
// Elements per workgroup of k_h_mt_qdq<HIST>: a workgroup zeroes a 4 KB LDS table and hands over up to MT_W + 2 global atomics, so
// it walks four of k_h_qdq's tiles (the ratio cnnq_pc_midtread_qdq keeps between its tiles) - where that leaves enough workgroups.
// The pass alone, bf16, at 8192 / 32768 / 65536 elements: [512,256,56,56] 447.2 (442.6-458.6) / 382.4 (376.2-394.7) / 382.1
// (378.6-388.0), [512,512,28,28] 226.0 (222.6-232.6) / 202.9 (200.0-207.8) / 209.0 (205.3-213.1), [512,64,56,56] 121.1 (119.0-123.6)
// / 114.5 (112.8-117.1) / 127.4 (125.5-130.0); [512,64,224,224] is one sample per workgroup at every length (1461.5 / 1464.3 /
// 1498.9).  The short rows, and the classes that fill less than one round of the 256 CUs' 8 workgroup slots at the long tile, ran
// faster at k_h_qdq's own: [512,1024,14,14] 127.0 (125.8-129.5) / 139.2 (132.8-151.7) / 145.5 (140.4-158.3), [512,256,14,14] 41.5
// (40.8-43.4) / 47.9 (46.8-51.3) / 70.2 (68.8-74.4), [512,2048,7,7] 131.5 (130.3-134.4) / 138.7 (135.8-146.7) / 139.3
// (136.2-145.7), [32,256,56,56] 37.4 (36.8-38.8) / 39.9 (39.3-41.4) / 53.8 (53.1-59.4).
inline int64_t h_mt_hist_elems(int64_t N, int64_t C, int64_t HW) {
    if (HW <= 196) return H_QDQ_ELEMS;
    return C * h_splits(N, C, HW, 4 * H_QDQ_ELEMS, N) <= 2048 ? H_QDQ_ELEMS : 4 * H_QDQ_ELEMS;
}
inline HGeo h_geo_mt(int64_t N, int64_t C, int64_t HW, int w, bool hist) {
    return h_geo(N, C, HW, w, h_splits(N, C, HW, hist ? h_mt_hist_elems(N, C, HW) : H_QDQ_ELEMS, N), 1);
}

inline bool h_mt_whole_fits(int64_t N, int64_t HW, int w) { return N * HW <= h_whole_cap(w); }
// The resident form against the chain (allow_single_launch = 1).  It won beyond the spread on [512,256,14,14] in seven of the eight
// runs (bf16 -bata 5.3: 63.9 (58.8-68.1) against 76.1 (72.8-84.1), with -me 134.3 (133.0-137.0) against 147.1 (144.5-152.5); fp16
// 63.0 (61.9-65.8) against 73.8 (72.8-76.3) and 131.5 (130.2-134.2) against 143.1 (141.1-148.0); the eighth, bf16 -bata 4 -me,
// 137.7 (132.2-148.1) against 150.7 (143.6-177.0), overlaps).  At 512 channels it won in three of eight runs without -me ([512,512,
// 14,14] bf16 118.1 (115.3-122.2) against 125.9 (123.4-134.8)) and was level with -me (237.7 (235.3-243.2) against 238.3
// (236.4-241.7)); at 1024 channels it won in one of four without -me and lost in three of four with it (568.2 (565.0-573.0) against 549.7
// (546.4-556.0)): C workgroups of 1024 lanes run in rounds of 256, and each hands its histogram over at its end.  So: 256
// channels at that population; other populations and fewer channels were not measured and stay on the chain.
inline int h_mt_whole_wins(int64_t N, int64_t C, int64_t HW, int dtype, bool hist) {
    (void)dtype; (void)hist;
    return C == 256 && N * HW >= 100352;
}
// The classes that run native against the upcast route: the chain won beyond the spread on every class of both networks with an
// even HW, in both dtypes, at both targets, with and without -me - from 0.32 x ([512,64,224,224] bf16 -bata 4 2316.5
// (2302.1-2332.3) against 7305.5 (7271.1-7340.4)) to 0.81 x ([512,256,14,14] -bata 4 -me 150.7 (143.6-177.0) against 185.3
// (180.2-188.2)).  An odd HW loads single 2-byte elements whatever the alignment (h_stats_native's finding), and the two 7x7
// classes did not win: [512,2048,7,7] was inside
// the spread or lost in all eight runs (bf16 254.7 (252.2-266.4) against 250.1 (247.6-254.0); fp16 -bata 4 252.6 (251.4-254.6)
// against 247.2 (244.8-249.2)), [512,512,7,7] won in one of the four runs without -me (95.9 (94.2-99.2) against 105.6
// (102.5-118.0)), was inside in three, and lost in all four with -me (229.9 (226.3-237.2) against 205.2 (201.4-214.5)).  So
// h_aciq_native's rule holds here too: odd rows stay on the upcast route from a population of 6272 on (the smallest that did not
// win there); smaller ones were not measured and stay native.
inline int h_mt_native(int64_t N, int64_t C, int64_t HW, int dtype, bool hist) {
    (void)C; (void)dtype; (void)hist;
    return !(HW % 2 == 1 && N * HW >= 6272);
}

}  // namespace
