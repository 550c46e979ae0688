// cnnq_sample_extrema.hip.h - the per-sample channel extrema of `-sm collect -sba` (smpc.py:72-78: a channel's max / min is the mean
// over the batch of the samples' own max / min) on contiguous bf16 / fp16 activations x[N][C][HW] and on dense channels_last
// (NHWC) activations x[N][HW][C] of fp32 / bf16 / fp16, read where they lie: ONE read of x, no layout copy, no upcast.
// Part of the single translation unit cnnq_kernels.hip (see its header for the design).
//
// The contract: ext[2][N * C] float32, sample-major (n * C + c), row CNNQ_STAT_MIN the minima and row
// CNNQ_STAT_MAX the maxima - the [2, rows] table of ops.tensor_row_stats, which statistic_manager.batch_extrema_sums reads.
// ext equals, as values, x.float().view(N, C, HW).amin(-1) / .amax(-1) of the exactly upconverted tensor (h_up / cl_up).  An
// (n, c) row that holds a NaN gives NaN in BOTH entries (torch.max's behaviour, and what the records of the former route do):
// v_min / v_max drop a NaN and a min/max-only kernel has no sum of squares to notice one by, so every element is tested v != v
// and a lane that saw one poisons its pair before any fold; pmin / pmax carry it on.  The sign of a zero extremum is not pinned.
// No atomics: every entry of ext (and of the partials) is stored once by one lane with a plain vector store, and extrema do not
// depend on the order of the elements: run after run the same bits.  No scratch.
//
// Contiguous bf16 / fp16 (k_h_sample_extrema): the N * C rows of HW elements lie back to back, and ext is indexed by the row, so
// the workgroups partition the ROWS as they lie - not the channels, as the rest of the half family does: there a workgroup's
// result is per channel, here it is per row, and neighbouring segments read neighbouring memory.  A SEGMENT of seg lanes (a
// power of two, 64 at most, h_se_seg: from HW alone) owns one row at a time, the workgroup's TPB / seg segments take TPB / seg
// rows per step; a segment folds its pair with the fixed xor tree seg / 2 ... 1 and its lane 0 stores it: no LDS, no barrier,
// one launch, no workspace (k_h_qerr's segments).  Loads: because the order does not matter a row is read in 16-byte loads from
// its first 16-byte boundary on, whatever its own alignment - the elements in front of the boundary (7 at most) and behind the
// last whole load (7 at most) one by one (k_h_kld_hist's walk, per row) - so the 98-byte rows of the 7x7 classes, 2-byte
// aligned, and a view at an odd element still move 16 bytes per lane.  Nothing outside the row is read.  Non-temporal: a
// collect step reads x for the last time.
//
// channels_last (k_cl_sample_extrema): cnnq_nhwc.hip.h's tiling planned per SAMPLE, as k_cl_qerr plans it - ClGeo over R = HW
// rows with S slabs and the grid N * S * nb: workgroup (n * S + s) * nb + b owns column block b of slab s of sample n, so a slab
// never crosses a sample boundary.  A lane keeps one piece of W consecutive channels and walks its slab's rows (cl_ld,
// non-temporal); the row-lanes of a workgroup meet once through LDS at the slab's end (k_cl_minmax's meeting).  With S == 1 the
// workgroup stores its C-block of ext directly: one launch, no workspace.  With S > 1 it stores the partial pair into
// ws[n * S + s][2][C] and k_sample_extrema_fold, one thread per (n, c), writes ext.
#pragma once
#include "cnnq_half.hip.h"
#include "cnnq_nhwc.hip.h"

namespace {

constexpr int SE_HW = 8;     // elements of one 16-byte load of a bf16 / fp16 row

// rows: N * C rows of HW elements back to back; workgroup b owns rows [b * steps * (TPB / seg), ...) - steps steps of TPB / seg
// rows - and gridDim.x * steps * (TPB / seg) >= rows
template <class T>
__global__ void __launch_bounds__(TPB) k_h_sample_extrema(const uint16_t* __restrict__ x, const int64_t rows, const int HW, const int seg,
                                                          const int steps, float* __restrict__ ext) {
    const int lane = (int)threadIdx.x & (seg - 1), sg = (int)threadIdx.x >> (31 - __builtin_clz(seg)), nseg = TPB / seg;
    const int64_t r0 = (int64_t)blockIdx.x * steps * nseg;
    for (int k = 0; k < steps; ++k) {                      // uniform: whole waves take part in the shuffles
        const int64_t r = r0 + (int64_t)k * nseg + sg;
        float mn = INFINITY, mx = -INFINITY;
        bool nan = false;
        if (r < rows) {
            const uint16_t* __restrict__ p = x + r * HW;
            // [0, head): up to the 16-byte boundary (p is 2-byte aligned: 0 .. 7 elements); [head, tail): whole loads; the rest
            const int head = min((int)(((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) >> 1), HW);
            const int nv = (HW - head) / SE_HW;
            const int tail = head + nv * SE_HW;
            for (int i = lane; i < head; i += seg) {
                uint16_t e[1];
                h_ld<1, true>(p + i, e);
                h_mm_piece<T, 1>(e, mn, mx, nan);
            }
#pragma unroll 4
            for (int v = lane; v < nv; v += seg) {
                uint16_t e[SE_HW];
                h_ld<SE_HW, true>(p + head + v * SE_HW, e);
                h_mm_piece<T, SE_HW>(e, mn, mx, nan);
            }
            for (int i = tail + lane; i < HW; i += seg) {
                uint16_t e[1];
                h_ld<1, true>(p + i, e);
                h_mm_piece<T, 1>(e, mn, mx, nan);
            }
        }
        if (nan) { mn = NAN; mx = NAN; }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            if (m < seg) { mn = pmin(mn, shfl_xor_f(mn, m)); mx = pmax(mx, shfl_xor_f(mx, m)); }
        }
        if (r < rows && lane == 0) {
            ext[(size_t)CNNQ_STAT_MIN * rows + r] = mn;
            ext[(size_t)CNNQ_STAT_MAX * rows + r] = mx;
        }
    }
}

// g: the geometry of ONE sample (g.R = HW); gridDim.x = N * g.S * g.nb.  g.S == 1: the pair goes to ext[2][N * C]; else to
// ws[n * S + s][2][C] for k_sample_extrema_fold (a trailing slab left without rows stores {inf, -inf}, which the fold passes over)
template <class T, int W>
__global__ void __launch_bounds__(TPB) k_cl_sample_extrema(const typename ClRaw<T>::type* __restrict__ x, const ClGeo g, const int N,
                                                           float* __restrict__ ws, float* __restrict__ ext) {
    typedef typename ClRaw<T>::type E;
    __shared__ float l_mn[TPB * W], l_mx[TPB * W];
    const int per = g.S * g.nb;
    const int n = (int)blockIdx.x / per, wg = (int)blockIdx.x - n * per;
    const ClLane l = cl_lane(g, wg);
    float mn[W], mx[W];
#pragma unroll
    for (int i = 0; i < W; ++i) { mn[i] = INFINITY; mx[i] = -INFINITY; }
    unsigned nanm = 0;
    if (l.piece >= 0) {
        const E* p = x + (int64_t)n * g.R * g.C + l.r * g.C + (int64_t)l.piece * W;
        const int64_t step = (int64_t)g.RS * g.C;
#pragma unroll 4
        for (int64_t r = l.r; r < l.r1; r += g.RS, p += step) {
            E e[W];
            cl_ld<E, W, true>(p, e);
#pragma unroll
            for (int i = 0; i < W; ++i) {
                const float v = cl_up(T{}, e[i]);
                mn[i] = fminf(mn[i], v);
                mx[i] = fmaxf(mx[i], v);
                nanm |= (unsigned)(v != v) << i;
            }
        }
    }
    const int t = (int)threadIdx.x;
    if (t < g.RS * g.CP) {
#pragma unroll
        for (int i = 0; i < W; ++i) {
            const bool isn = (nanm >> i) & 1u;
            l_mn[t * W + i] = isn ? NAN : mn[i];
            l_mx[t * W + i] = isn ? NAN : mx[i];
        }
    }
    __syncthreads();
    // the lanes that share a piece: column j of the [RS][CP * W] table, one thread per column
    const int s = wg / g.nb, b = wg - s * g.nb;
    const int cols = g.CP * W;
    const size_t NC = (size_t)N * g.C;
    float* o_mn = g.S == 1 ? ext + (size_t)CNNQ_STAT_MIN * NC + (size_t)n * g.C : ws + ((size_t)n * g.S + s) * 2 * g.C;
    float* o_mx = g.S == 1 ? ext + (size_t)CNNQ_STAT_MAX * NC + (size_t)n * g.C : o_mn + g.C;
    for (int j = t; j < cols; j += TPB) {
        const int c = b * cols + j;
        if (c >= g.C) break;
        float a = l_mn[j], z = l_mx[j];
        for (int k = 1; k < g.RS; ++k) { a = pmin(a, l_mn[k * cols + j]); z = pmax(z, l_mx[k * cols + j]); }
        o_mn[c] = a;
        o_mx[c] = z;
    }
}

// ws[n * S + s][2][C] -> ext[2][N * C]: one thread per (n, c), the slabs in ascending order
__global__ void __launch_bounds__(TPB) k_sample_extrema_fold(const float* __restrict__ ws, const int64_t NC, const int C, const int S,
                                                             float* __restrict__ ext) {
    const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (i >= NC) return;
    const int64_t n = i / C;
    const int c = (int)(i - n * C);
    const float* p = ws + (size_t)n * S * 2 * C + c;
    float a = p[0], z = p[C];
    for (int s = 1; s < S; ++s) {
        p += 2 * (size_t)C;
        a = pmin(a, p[0]);
        z = pmax(z, p[C]);
    }
    ext[(size_t)CNNQ_STAT_MIN * NC + i] = a;
    ext[(size_t)CNNQ_STAT_MAX * NC + i] = z;
}

// ---- host side: the plans
// Lanes per row, from HW alone: with nv = ceil(HW / 8) sixteen-byte loads in a row, the power of two that gives every load a
// lane up to eight lanes - short rows (2x2, 7x7, 14x14) do not idle a wave: 1x2 and 2x2 take one lane, 7x7 and 14x14 eight -
// then the one that leaves a lane about H_SE_PPL loads, one wave at most: long rows (112x112, 224x224) take several steps of one
// segment.  A read-only pass wants its loads in flight, so fewer per lane than k_h_qerr's segments keep (h_qe_seg).
constexpr int64_t H_SE_PPL = 4;
inline int h_se_seg(int64_t HW) {
    const int64_t nv = (HW + SE_HW - 1) / SE_HW;
    int seg = 1;
    while (seg < 8 && seg < nv) seg <<= 1;
    while (seg < 64 && (int64_t)seg * H_SE_PPL < nv) seg <<= 1;
    return seg;
}
// steps of TPB / seg rows per workgroup: about H_MM_ELEMS elements (the statistics workgroups of the family), no more than the
// tensor has
inline int h_se_steps(int64_t rows, int64_t HW, int seg) {
    const int64_t nseg = TPB / seg, all = (rows + nseg - 1) / nseg;
    int64_t steps = H_MM_ELEMS / (nseg * HW);
    if (steps > all) steps = all;
    return (int)(steps < 1 ? 1 : steps);
}

// The slabs a sample's HW rows are cut into - a function of (N, HW, C) and the element size, not of the alignment, so that the
// workspace is known before the alignment is: about CL_SE_ELEMS elements per workgroup (a column block counted as min(C, TPB
// pieces of 16 bytes) channels), and no more slabs than keep N * S at CL_SE_MAX_WGS workgroups - a batch that fills the device by
// its samples is not cut, a small batch of large images is (cl_qe_slabs' rule; the pass is lighter than k_cl_qerr, so its
// workgroups are shorter and more).
constexpr int64_t CL_SE_ELEMS = 16384;
constexpr int64_t CL_SE_MAX_WGS = 1024;
inline int cl_se_slabs(int64_t N, int64_t HW, int64_t C, int esize) {
    const int64_t wide = (int64_t)TPB * (16 / esize);
    const int64_t colw = C < wide ? C : wide;
    const int64_t rows = (CL_SE_ELEMS + colw - 1) / colw;
    int64_t S = (HW + rows - 1) / rows;
    const int64_t cap = CL_SE_MAX_WGS / N;
    if (S > cap) S = cap;
    return (int)(S < 1 ? 1 : S);
}
// geometry of one sample for piece width w: S = cl_se_slabs slabs of rpw rows, rpw a multiple of RS with S * rpw >= HW
inline ClGeo cl_geo_se(int64_t N, int64_t HW, int64_t C, int w, int esize) {
    ClGeo g;
    g.R = HW;
    g.C = (int)C;
    g.P = (int)(C / w);
    g.CP = g.P < TPB ? g.P : TPB;
    g.RS = TPB / g.CP;
    g.nb = (g.P + g.CP - 1) / g.CP;
    g.S = cl_se_slabs(N, HW, C, esize);
    const int64_t rows = (HW + g.S - 1) / g.S;
    g.rpw = (rows + g.RS - 1) / g.RS * g.RS;
    return g;
}

// The classes of layer that stay on the former route (the "native" word of the two route functions).  Rule: a class counts as won
// when the native step's maximum is under the former route's minimum in one run (tools/bench_sba_collect.py); one that does not
// win gets 0 here.  Figures: profiles/sba_collect.md.
// Contiguous bf16, ResNet-50 b512, us per whole -sba collect step, mean (min-max), native against former: every class won but
// [512,256,14,14] 144.6 (138.7-201.1) / 174.4 (171.5-178.2) and [512,512,7,7] 167.6 (159.0-202.2) / 188.2 (184.2-195.5) - faster
// on average, one step each above the former route's fastest.  The classes next to them won: [512,512,14,14] 188.6 (182.7-201.3)
// / 254.3 (249.0-266.1), [512,2048,7,7] 297.1 (287.6-322.8) / 382.3 (375.4-393.6).  So, as h_qerr_native: rows that are no
// multiple of 8 elements, in tensors below 2^25 elements whose channels fill a workgroup; smaller populations were not measured
// and stay native.
inline int h_sample_extrema_native(int64_t N, int64_t C, int64_t HW, int dtype) {
    (void)dtype;
    return !(HW % 8 != 0 && N * HW >= H_MM_ELEMS && N * C * HW < ((int64_t)1 << 25));
}
// channels_last, fp32 and bf16: all 12 classes won (bf16 14.1 against 50.2 ms for the 53 layers, fp32 18.3 against 44.6)
inline int cl_sample_extrema_native(int64_t, int64_t, int64_t, int) { return 1; }

}  // namespace
