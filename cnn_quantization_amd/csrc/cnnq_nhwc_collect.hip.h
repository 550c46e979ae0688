// cnnq_nhwc_collect.hip.h - `-sm collect` on dense channels_last (NHWC) activations: the two per-channel SUM reductions over
// [R = N*H*W][C] storage that fill the rows config 3's reductions (cnnq_nhwc_aciq.hip.h) leave zero - pass A with the rectified
// sums {sum max(x,0), sum max(x,0)^2} (-> STD_POS) and pass B with the fourth moment sum z^4 (-> KURT) - for fp32, bf16 and fp16.
// Part of the single translation unit cnnq_kernels.hip (see its header for the design).
//
// They are config 3's kernels with more running sums, written as kernels of their own so that every instance of k_cl_moments /
// k_cl_absdev keeps its code: the records are the fp64 records k_combine(has_relu) / k_combine_dev(want_kurt) merge, the sums
// every kernel shares (sum x, sum x^2, sum |x - mean|) are the same expressions added in the same order - so the rows MIN, MAX,
// MEAN, STD and B of the table do not depend on which of the kernels ran - and the order is fixed by the geometry (ClGeo) alone:
// no atomics, every record entry stored once by one lane, run after run the same bits.  The contract: the
// table against fp64 within the statistics tier of the NCHW single launch (extrema exact).
//
// Tiling, the two summation regimes (CL_FOLD, CL_EXACT_ROWS and why) and the LDS meeting of the sums: cnnq_nhwc.hip.h.
#pragma once
#include "cnnq_nhwc.hip.h"
#include "cnnq_stats.hip.h"

namespace {

// pass A: slab s -> part[s][CNNQ_NMOM][C], all seven rows.  Per element the arithmetic of k_moments<RELU> (Mom::add4 for the four
// rows of a fold, Mom::add for a single row: the rectified value is fmaxf(v, 0), which drops a NaN as the NCHW chain does); the
// NaN rule, the count and `rev` are k_cl_moments'.
template <class T, int W, bool NTL>
__global__ void __launch_bounds__(TPB) k_cl_moments_relu(const typename ClRaw<T>::type* __restrict__ x, const ClGeo g, const int rev,
                                                         double* __restrict__ part) {
    typedef typename ClRaw<T>::type E;
    __shared__ double l_d[TPB * W];
    const int bid = rev ? (int)gridDim.x - 1 - (int)blockIdx.x : (int)blockIdx.x;
    const ClLane l = cl_lane(g, bid);
    float mn[W], mx[W];
    double s[W], ss[W], rs[W], rss[W];
#pragma unroll
    for (int i = 0; i < W; ++i) { mn[i] = INFINITY; mx[i] = -INFINITY; s[i] = 0.; ss[i] = 0.; rs[i] = 0.; rss[i] = 0.; }
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
                    const float r0 = fmaxf(v0, 0.f), r1 = fmaxf(v1, 0.f), r2 = fmaxf(v2, 0.f), r3 = fmaxf(v3, 0.f);
                    rs[i] += (double)((r0 + r1) + (r2 + r3));
                    rss[i] += (double)((r0 * r0 + r1 * r1) + (r2 * r2 + r3 * r3));
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
                const double q = (double)fmaxf(v, 0.f);
                rs[i] += q;
                rss[i] = fma(q, q, rss[i]);
            }
        }
    }
    const int sl = bid / g.nb, b = bid - sl * g.nb;
    double* rec = part + (size_t)sl * CNNQ_NMOM * g.C;
    cl_fold_sums<W>(l_d, g, b, s, rec + (size_t)CNNQ_MOM_SUM * g.C);
    cl_fold_sums<W>(l_d, g, b, ss, rec + (size_t)CNNQ_MOM_SUMSQ * g.C);
    cl_fold_sums<W>(l_d, g, b, rs, rec + (size_t)CNNQ_MOM_SUM_RELU * g.C);
    cl_fold_sums<W>(l_d, g, b, rss, rec + (size_t)CNNQ_MOM_SUMSQ_RELU * g.C);
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
    }
}

// pass B: slab s -> part2[s][CNNQ_NDEV][C], both rows, with the mean and the standard deviation of rows CNNQ_STAT_MEAN / _STD of
// the table pass A's merge wrote (k_combine's std_of on the merged record, as the NCHW chain's k_absdev<KURT> reads it): the fp32
// subtract of k_absdev per element, z = (x - mean) * (1 / std) with the fp32 reciprocal formed once per channel, z^4 = (z * z)^2;
// both sums as pass A sums.  A constant channel (std == 0) gives 0 * inf: its kurtosis is NaN, as in the NCHW chain.
template <class T, int W, bool NTL>
__global__ void __launch_bounds__(TPB) k_cl_absdev_kurt(const typename ClRaw<T>::type* __restrict__ x, const ClGeo g,
                                                        const float* __restrict__ stats, double* __restrict__ part2) {
    typedef typename ClRaw<T>::type E;
    __shared__ double l_d[TPB * W];
    const int bid = (int)blockIdx.x;
    const ClLane l = cl_lane(g, bid);
    double sa[W], sk[W];
#pragma unroll
    for (int i = 0; i < W; ++i) { sa[i] = 0.; sk[i] = 0.; }
    if (l.piece >= 0) {
        float mean[W], sd[W];
#pragma unroll
        for (int i = 0; i < W; ++i) {
            mean[i] = stats[(size_t)CNNQ_STAT_MEAN * g.C + l.piece * W + i];
            sd[i] = 1.f / stats[(size_t)CNNQ_STAT_STD * g.C + l.piece * W + i];
        }
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
                    const float d0 = cl_up(T{}, e[0][i]) - mean[i], d1 = cl_up(T{}, e[1][i]) - mean[i];
                    const float d2 = cl_up(T{}, e[2][i]) - mean[i], d3 = cl_up(T{}, e[3][i]) - mean[i];
                    const float a0 = fabsf(d0), a1 = fabsf(d1), a2 = fabsf(d2), a3 = fabsf(d3);
                    sa[i] += (double)((a0 + a1) + (a2 + a3));
                    const float z0 = d0 * sd[i], z1 = d1 * sd[i], z2 = d2 * sd[i], z3 = d3 * sd[i];
                    const float q0 = z0 * z0, q1 = z1 * z1, q2 = z2 * z2, q3 = z3 * z3;
                    sk[i] += (double)((q0 * q0 + q1 * q1) + (q2 * q2 + q3 * q3));
                }
            }
        }
        for (; r < l.r1; r += g.RS, p += step) {
            E e[W];
            cl_ld<E, W, NTL>(p, e);
#pragma unroll
            for (int i = 0; i < W; ++i) {
                const float d = cl_up(T{}, e[i]) - mean[i];
                sa[i] += (double)fabsf(d);
                const float z = d * sd[i];
                const float q = z * z;
                sk[i] += (double)(q * q);
            }
        }
    }
    const int sl = bid / g.nb, b = bid - sl * g.nb;
    double* rec = part2 + (size_t)sl * CNNQ_NDEV * g.C;
    cl_fold_sums<W>(l_d, g, b, sa, rec + (size_t)CNNQ_DEV_ABS * g.C);
    cl_fold_sums<W>(l_d, g, b, sk, rec + (size_t)CNNQ_DEV_Z4 * g.C);
}

}  // namespace
