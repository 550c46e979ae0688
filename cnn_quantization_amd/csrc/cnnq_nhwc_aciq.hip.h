// cnnq_nhwc_aciq.hip.h - config 3 (ACIQ clipping, bit allocation) on dense channels_last (NHWC) activations: the two per-channel
// SUM reductions over [R = N*H*W][C] storage that the statistics table needs - pass A {min, max, sum x, sum x^2, count} and pass B
// sum |x - mean| - for fp32, bf16 and fp16 elements.
// Part of the single translation unit cnnq_kernels.hip (see its header for the design).
//
// Everything behind the sums is the NCHW chain's own: the records are the fp64 records k_combine / k_combine_dev merge, the
// parameters come from k_params, the Q/DQ is k_cl_qdq with the table (qdq1, the IEEE divide).  The contract (DESIGN.md section
// 14): the table against fp64 within the statistics tier (extrema exact), and given the table every output bit for bit.  The sums
// are added in an order fixed by the geometry (ClGeo) alone - it is not the NCHW chain's order, so equality with that chain is
// not promised - and run after run the same: no atomics, every record entry stored once by one lane.
//
// Tiling, the two summation regimes (CL_FOLD, CL_EXACT_ROWS and why) and the LDS meeting of the sums: cnnq_nhwc.hip.h.  A lane
// keeps one piece of W consecutive channels and walks the rows of its slab, so it owns W running sums per quantity.
#pragma once
#include "cnnq_nhwc.hip.h"
#include "cnnq_stats.hip.h"

namespace {

// pass A: slab s -> part[s][CNNQ_NMOM][C] (rows SUM_RELU / SUMSQ_RELU zero).  v_min / v_max drop a NaN; the sum of squares is
// NaN iff an element was (inf * inf = inf, nothing cancels), and then the channel's extrema become NaN - k_cl_minmax's rule with
// k_moments' test.  rev: workgroups take the slabs in descending address order (the launch in front of an ascending pass B).
template <class T, int W, bool NTL>
__global__ void __launch_bounds__(TPB) k_cl_moments(const typename ClRaw<T>::type* __restrict__ x, const ClGeo g, const int rev,
                                                    double* __restrict__ part) {
    typedef typename ClRaw<T>::type E;
    __shared__ double l_d[TPB * W];
    const int bid = rev ? (int)gridDim.x - 1 - (int)blockIdx.x : (int)blockIdx.x;
    const ClLane l = cl_lane(g, bid);
    float mn[W], mx[W];
    double s[W], ss[W];
#pragma unroll
    for (int i = 0; i < W; ++i) { mn[i] = INFINITY; mx[i] = -INFINITY; s[i] = 0.; ss[i] = 0.; }
    if (l.piece >= 0) {
        const E* p = x + l.r * g.C + (int64_t)l.piece * W;
        const int64_t step = (int64_t)g.RS * g.C;
        int64_t r = l.r;
        if (g.R > CL_EXACT_ROWS) {
#pragma unroll 2
            for (; r + (CL_FOLD - 1) * (int64_t)g.RS < l.r1; r += (int64_t)CL_FOLD * g.RS, p += CL_FOLD * step) {
                E e[CL_FOLD][W];
#pragma unroll
                for (int k = 0; k < CL_FOLD; ++k) cl_ld<E, W, NTL>(p + k * step, e[k]);
#pragma unroll
                for (int i = 0; i < W; ++i) {
                    const float v0 = cl_up(T{}, e[0][i]), v1 = cl_up(T{}, e[1][i]), v2 = cl_up(T{}, e[2][i]), v3 = cl_up(T{}, e[3][i]);
                    mn[i] = fminf(fminf(mn[i], fminf(v0, v1)), fminf(v2, v3));
                    mx[i] = fmaxf(fmaxf(mx[i], fmaxf(v0, v1)), fmaxf(v2, v3));
                    s[i] += (double)((v0 + v1) + (v2 + v3));
                    ss[i] += (double)((v0 * v0 + v1 * v1) + (v2 * v2 + v3 * v3));
                }
            }
        }
        for (; r < l.r1; r += g.RS, p += step) {
            E e[W];
            cl_ld<E, W, NTL>(p, e);
#pragma unroll
            for (int i = 0; i < W; ++i) {
                const float v = cl_up(T{}, e[i]);
                mn[i] = fminf(mn[i], v);
                mx[i] = fmaxf(mx[i], v);
                const double d = (double)v;
                s[i] += d;
                ss[i] = fma(d, d, ss[i]);
            }
        }
    }
    const int sl = bid / g.nb, b = bid - sl * g.nb;
    double* rec = part + (size_t)sl * CNNQ_NMOM * g.C;
    cl_fold_sums<W>(l_d, g, b, s, rec + (size_t)CNNQ_MOM_SUM * g.C);
    cl_fold_sums<W>(l_d, g, b, ss, rec + (size_t)CNNQ_MOM_SUMSQ * g.C);
    // the extrema: the same LDS as two fp32 tables
    float* l_mn = reinterpret_cast<float*>(l_d);
    float* l_mx = l_mn + TPB * W;
    const int t = (int)threadIdx.x;
    if (t < g.RS * g.CP) {
#pragma unroll
        for (int i = 0; i < W; ++i) {
            const bool n = ss[i] != ss[i];
            l_mn[t * W + i] = n ? NAN : mn[i];
            l_mx[t * W + i] = n ? NAN : mx[i];
        }
    }
    __syncthreads();
    int64_t r1 = (int64_t)(sl + 1) * g.rpw;
    if (r1 > g.R) r1 = g.R;
    const double count = (double)(r1 - (int64_t)sl * g.rpw);
    const int cols = g.CP * W;
    for (int j = t; j < cols; j += TPB) {
        const int c = b * cols + j;
        if (c >= g.C) break;
        float a = l_mn[j], z = l_mx[j];
        for (int k = 1; k < g.RS; ++k) { a = pmin(a, l_mn[k * cols + j]); z = pmax(z, l_mx[k * cols + j]); }
        rec[(size_t)CNNQ_MOM_MIN * g.C + c] = (double)a;
        rec[(size_t)CNNQ_MOM_MAX * g.C + c] = (double)z;
        rec[(size_t)CNNQ_MOM_COUNT * g.C + c] = count;
        rec[(size_t)CNNQ_MOM_SUM_RELU * g.C + c] = 0.;
        rec[(size_t)CNNQ_MOM_SUMSQ_RELU * g.C + c] = 0.;
    }
}

// pass B: slab s -> part2[s][CNNQ_NDEV][C] (row DEV_Z4 zero), sum |x - mean| with the mean of row CNNQ_STAT_MEAN of the table pass
// A's merge wrote: the fp32 subtract and fabsf of k_absdev per element, summed as pass A sums
template <class T, int W, bool NTL>
__global__ void __launch_bounds__(TPB) k_cl_absdev(const typename ClRaw<T>::type* __restrict__ x, const ClGeo g,
                                                   const float* __restrict__ stats, double* __restrict__ part2) {
    typedef typename ClRaw<T>::type E;
    __shared__ double l_d[TPB * W];
    const int bid = (int)blockIdx.x;
    const ClLane l = cl_lane(g, bid);
    double sa[W];
#pragma unroll
    for (int i = 0; i < W; ++i) sa[i] = 0.;
    if (l.piece >= 0) {
        float mean[W];
#pragma unroll
        for (int i = 0; i < W; ++i) mean[i] = stats[(size_t)CNNQ_STAT_MEAN * g.C + l.piece * W + i];
        const E* p = x + l.r * g.C + (int64_t)l.piece * W;
        const int64_t step = (int64_t)g.RS * g.C;
        int64_t r = l.r;
        if (g.R > CL_EXACT_ROWS) {
#pragma unroll 2
            for (; r + (CL_FOLD - 1) * (int64_t)g.RS < l.r1; r += (int64_t)CL_FOLD * g.RS, p += CL_FOLD * step) {
                E e[CL_FOLD][W];
#pragma unroll
                for (int k = 0; k < CL_FOLD; ++k) cl_ld<E, W, NTL>(p + k * step, e[k]);
#pragma unroll
                for (int i = 0; i < W; ++i) {
                    const float a0 = fabsf(cl_up(T{}, e[0][i]) - mean[i]), a1 = fabsf(cl_up(T{}, e[1][i]) - mean[i]);
                    const float a2 = fabsf(cl_up(T{}, e[2][i]) - mean[i]), a3 = fabsf(cl_up(T{}, e[3][i]) - mean[i]);
                    sa[i] += (double)((a0 + a1) + (a2 + a3));
                }
            }
        }
        for (; r < l.r1; r += g.RS, p += step) {
            E e[W];
            cl_ld<E, W, NTL>(p, e);
#pragma unroll
            for (int i = 0; i < W; ++i) sa[i] += (double)fabsf(cl_up(T{}, e[i]) - mean[i]);
        }
    }
    const int sl = bid / g.nb, b = bid - sl * g.nb;
    double* rec = part2 + (size_t)sl * CNNQ_NDEV * g.C;
    cl_fold_sums<W>(l_d, g, b, sa, rec + (size_t)CNNQ_DEV_ABS * g.C);
    const int cols = g.CP * W;
    for (int j = (int)threadIdx.x; j < cols; j += TPB) {
        const int c = b * cols + j;
        if (c >= g.C) break;
        rec[(size_t)CNNQ_DEV_Z4 * g.C + c] = 0.;
    }
}

}  // namespace
