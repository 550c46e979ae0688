// cnnq_nhwc_midtread.hip.h - config 5 (mid-tread quantization with per-channel bin allocation, and the entropy of its codes) on
// dense channels_last (NHWC) activations: the Q/DQ pass with the code histogram over [R = N*H*W][C] storage, for fp32, bf16 and
// fp16 elements.
// Part of the single translation unit cnnq_kernels.hip (see its header for the design).
//
// Everything around the pass is layout-free and the NCHW chain's own: the statistics table comes from k_cl_moments / k_cl_absdev
// (cnnq_nhwc_aciq.hip.h) through k_combine / k_combine_dev, the step sizes and clamp bounds from k_mt_params<false>, the entropy
// from k_mt_entropy / k_mt_entropy_batch on the histogram written here.  The contract: given the table
// mt[CNNQ_NMT][C], y and every word of the histogram but the split of the window counts over the replica tables are, bit for
// bit, k_mt_qdq's with CLIP = true on the same values in NCHW order.
//
// Tiling: cnnq_nhwc.hip.h.  A lane keeps one piece of W consecutive channels for its whole slab, so its channels' delta, c_min,
// c_max - and, with the histogram, its counts of "clamped to a non-integer bound" - live in registers from the first row to
// the last.  Activations always clip and nobody asks for the codes here: there is no CLIP = false and no CODES instance.
#pragma once
#include "cnnq_nhwc.hip.h"
#include "cnnq_midtread.hip.h"

namespace {

// y = clamp(rint(x / delta[c]), c_min[c], c_max[c]) * delta[c] (iq.py:202-224) on the upconverted value, rounded once into the
// element type; x read and y written non-temporally, workgroups in descending address order, as k_cl_qdq.
// HIST: the fp32 codes are counted into k_mt_qdq's histogram (layout and rules: the note above k_mt_qdq) - an integer code
// inside the window [wstart, wstart + MT_W) is one LDS atomic, code 0 and the clamps to a non-integer bound are carry adds in
// registers, everything else (rare) goes to global memory at once.  What a workgroup hands over at its end: one atomic per live
// window bin into replica table (workgroup id % MT_GR), and - the RS lanes that share a piece folded through LDS first - one
// atomic per channel and bound that was hit.  Every workgroup of a tensor of up to TPB * W channels hits the same 2 * C clamp
// counters, so the histogram variant runs on the long slabs of cl_geo_hist (cnnq_nhwc.hip.h).
// The code, its count and the LDS table's zeroing and fold are k_mt_qdq's own definitions (mt_code, mt_hist_count, mt_hist_zero,
// mt_hist_zero_code, mt_hist_fold in cnnq_midtread.hip.h); tests/test_channels_last_midtread_gpu.py compares the two histograms.
template <class T, int W, bool HIST>
__global__ void __launch_bounds__(TPB) k_cl_mt_qdq(const typename ClRaw<T>::type* __restrict__ x, typename ClRaw<T>::type* __restrict__ y,
                                                   const ClGeo g, const float* __restrict__ mt, unsigned long long* __restrict__ hist) {
    typedef typename ClRaw<T>::type E;
    __shared__ unsigned sh_hist[HIST ? MT_WORDS : 1];
    __shared__ unsigned sh_clo[HIST ? TPB * W : 1], sh_chi[HIST ? TPB * W : 1];
    const int tid = (int)threadIdx.x;
    const int bid = (int)gridDim.x - 1 - (int)blockIdx.x;
    const int cols = g.CP * W;                       // the workgroup's channels
    if constexpr (HIST) {
        mt_hist_zero<TPB>(sh_hist);
        for (int i = tid; i < cols; i += TPB) { sh_clo[i] = 0u; sh_chi[i] = 0u; }
        __syncthreads();
    }
    const ClLane l = cl_lane(g, bid);
    if constexpr (!HIST) {
        if (l.piece < 0) return;
    }
    const int wstart = HIST ? (int)mt[(size_t)CNNQ_MT_WSTART * g.C] : 0;
    unsigned nzero = 0;                              // code 0 (the mode of the distribution) is counted in a register
    if (l.piece >= 0) {
        const int c0 = l.piece * W;
        float d[W], lo[W], hi[W];
        unsigned nhi[W], nlo[W];                     // histogram: how often this lane clamped to a non-integer bound (nlo: or met a NaN)
        unsigned hi_ni = 0, lo_ni = 0;               // ... bit i: the bound of channel c0 + i is not an integer code
#pragma unroll
        for (int i = 0; i < W; ++i) {
            d[i] = mt[(size_t)CNNQ_MT_DELTA * g.C + c0 + i];
            lo[i] = mt[(size_t)CNNQ_MT_CMIN * g.C + c0 + i];
            hi[i] = mt[(size_t)CNNQ_MT_CMAX * g.C + c0 + i];
            nhi[i] = 0u;
            nlo[i] = 0u;
            if constexpr (HIST) {
                hi_ni |= (unsigned)(hi[i] != rintf(hi[i])) << i;     // a non-integer bound is a value of its own
                lo_ni |= (unsigned)(lo[i] != rintf(lo[i])) << i;
            }
        }
        const int64_t step = (int64_t)g.RS * g.C;
        int64_t off = l.r * g.C + c0;
        for (int64_t r = l.r; r < l.r1; r += g.RS, off += step) {
            E e[W];
            cl_ld<E, W, true>(x + off, e);
#pragma unroll
            for (int i = 0; i < W; ++i) {
                const float t = mt_code<true>(cl_up(T{}, e[i]) / d[i], lo[i], hi[i]);
                e[i] = cl_down(T{}, t * d[i]);                       // iq.py:224
                if constexpr (HIST) {
                    // (a NaN goes to the channel's c_min counter, here the lane's own)
                    mt_hist_count<true>(t, lo[i], hi[i], (lo_ni >> i) & 1u, (hi_ni >> i) & 1u, wstart, sh_hist, hist, g.C, nzero, nhi[i],
                                        nlo[i], [&] { nlo[i] += 1u; });
                }
            }
            cl_st_nt<E, W>(y + off, e);
        }
        if constexpr (HIST) {
            // the lanes that share this piece meet in LDS
            const int lp = l.piece - (bid % g.nb) * g.CP;
#pragma unroll
            for (int i = 0; i < W; ++i) {
                if (nhi[i]) atomicAdd(&sh_chi[lp * W + i], nhi[i]);
                if (nlo[i]) atomicAdd(&sh_clo[lp * W + i], nlo[i]);
            }
        }
    }
    if constexpr (HIST) {
        mt_hist_zero_code(sh_hist, hist, g.C, wstart, nzero);
        __syncthreads();
        const int cbase = (bid % g.nb) * cols;
        for (int j = tid; j < cols; j += TPB) {
            const int c = cbase + j;
            if (c >= g.C) break;
            if (sh_clo[j]) atomicAdd(&hist[MT_NB + 2 + c], (unsigned long long)sh_clo[j]);
            if (sh_chi[j]) atomicAdd(&hist[MT_NB + 2 + g.C + c], (unsigned long long)sh_chi[j]);
        }
        mt_hist_fold<TPB>(sh_hist, hist, g.C, wstart, bid);
    }
}

}  // namespace
