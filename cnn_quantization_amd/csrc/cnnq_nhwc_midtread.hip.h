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
// The update and the flush are k_mt_qdq's, copied: the contract needs both to stay the same for good, and shared __device__
// helpers would make that structural.  They are not shared yet because k_mt_qdq's speed is measured (the note above it: the
// branch-free update was worth 2.2x the VALU instructions) and moving its body behind a call was not re-measured; who changes
// one copy changes the other, and tests/test_channels_last_midtread_gpu.py compares the two histograms word for word.
template <class T, int W, bool HIST>
__global__ void __launch_bounds__(TPB) k_cl_mt_qdq(const typename ClRaw<T>::type* __restrict__ x, typename ClRaw<T>::type* __restrict__ y,
                                                   const ClGeo g, const float* __restrict__ mt, unsigned long long* __restrict__ hist) {
    typedef typename ClRaw<T>::type E;
    constexpr int MT_WORDS = MT_W * MT_REP;
    auto hidx = [](unsigned kk, int tid) -> unsigned { return kk * MT_REP + (unsigned)(tid & (MT_REP - 1)); };
    __shared__ unsigned sh_hist[HIST ? MT_WORDS : 1];
    __shared__ unsigned sh_clo[HIST ? TPB * W : 1], sh_chi[HIST ? TPB * W : 1];
    const int tid = (int)threadIdx.x;
    const int bid = (int)gridDim.x - 1 - (int)blockIdx.x;
    const int cols = g.CP * W;                       // the workgroup's channels
    if constexpr (HIST) {
        for (int i = tid; i < MT_WORDS; i += TPB) sh_hist[i] = 0u;
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
                float t = rintf(cl_up(T{}, e[i]) / d[i]);            // iq.py:202-203
                // torch.min(t, hi) = t < hi ? t : hi and torch.max(t, lo) = t > lo ? t : lo, NaN kept (the bound wins ties:
                // max(-0, +0) is +0, iq.py:213-214)
                t = (t < hi[i] || t != t) ? t : hi[i];
                t = (t > lo[i] || t != t) ? t : lo[i];
                e[i] = cl_down(T{}, t * d[i]);                       // iq.py:224
                if constexpr (HIST) {
                    // k_mt_qdq's update, statement for statement
                    const bool z = (t == 0.f);
                    const bool at_hi = ((hi_ni >> i) & 1u) && t == hi[i];
                    const bool at_lo = ((lo_ni >> i) & 1u) && t == lo[i] && !at_hi;   // (c_min == c_max: ONE value, counted once)
                    nzero += z ? 1u : 0u;
                    nhi[i] += at_hi ? 1u : 0u;
                    nlo[i] += at_lo ? 1u : 0u;
                    const int k = (int)t;                            // saturating; NaN -> 0
                    const unsigned kk = (unsigned)(k - wstart);
                    const bool fast = ((float)k == t) && kk < (unsigned)MT_W;
                    if (fast && !z) {
                        atomicAdd(&sh_hist[hidx(kk, tid)], 1u);
                    } else if (!(z || at_hi || at_lo)) {             // rare
                        if (t == rintf(t)) {                         // integer code outside the window (or inf)
                            if (t >= (float)(-MT_NB / 2) && t < (float)(MT_NB / 2)) atomicAdd(&hist[(int)t + MT_NB / 2], 1ull);
                            else atomicAdd(&hist[t < 0.f ? MT_NB : MT_NB + 1], 1ull);
                            atomicAdd(&hist[mt_flag_word(g.C)], 1ull);   // the global bins are in use
                        } else {
                            nlo[i] += 1u;                            // NaN: the channel's c_min counter
                        }
                    }
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
        if (nzero) {
            const int kk = -wstart;
            if (kk >= 0 && kk < MT_W) {
                atomicAdd(&sh_hist[hidx((unsigned)kk, tid)], nzero);
            } else {
                // code 0 lies outside the window: its count goes to the global bins, and the flag word must say so
                atomicAdd(&hist[MT_NB / 2], (unsigned long long)nzero);
                atomicAdd(&hist[mt_flag_word(g.C)], 1ull);
            }
        }
        __syncthreads();
        const int cbase = (bid % g.nb) * cols;
        for (int j = tid; j < cols; j += TPB) {
            const int c = cbase + j;
            if (c >= g.C) break;
            if (sh_clo[j]) atomicAdd(&hist[MT_NB + 2 + c], (unsigned long long)sh_clo[j]);
            if (sh_chi[j]) atomicAdd(&hist[MT_NB + 2 + g.C + c], (unsigned long long)sh_chi[j]);
        }
        unsigned long long* rep = hist + MT_NB + 2 + 2 * (size_t)g.C + (size_t)(bid & (MT_GR - 1)) * MT_W;
        for (int i = tid; i < MT_W; i += TPB) {
            unsigned tot = 0;
#pragma unroll
            for (int r = 0; r < MT_REP; ++r) tot += sh_hist[hidx((unsigned)i, r + tid)];
            if (tot) {
                if (wstart + i < MT_NB / 2) {
                    atomicAdd(&rep[i], (unsigned long long)tot);
                } else {
                    atomicAdd(&hist[MT_NB + 1], (unsigned long long)tot);
                    atomicAdd(&hist[mt_flag_word(g.C)], 1ull);
                }
            }
        }
    }
}

}  // namespace
