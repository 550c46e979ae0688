// cnnq_rows.hip.h - the statistics of FEW, VERY LONG rows over flat storage, for fp32, bf16 and fp16 elements: x viewed as
// [rows][len], every row contiguous and the rows back to back.  rows = 1 is the whole tensor (the per-tensor `-sm collect` of
// statistic_manager.py:55-96), rows = N the samples (the per-sample sums of squares of `-ms`).  Whole-tensor and per-sample sums
// and extrema do not depend on the order of the elements, and a sample of a dense channels_last tensor is one contiguous block,
// so the same kernels serve both layouts on the storage as it lies: no layout copy and no upcast.
// Part of the single translation unit cnnq_kernels.hip (see its header for the design).
//
// Tiling (RowsGeo): a row is cut into P = len / W pieces of W elements (W the widest of 16 / 8 / 4 / 2 bytes,
// or one element, that divides len * sizeof(T) and x's alignment - cl_piece - so every row starts on a piece), the pieces into S
// chunks of ppc consecutive pieces (the last chunk takes what is left).  A workgroup owns one (row, chunk): lane t loads pieces
// t, t + TPB, ... of it, ROWS_U of them per step.  The per-channel geometry (make_geo, cl_geo) cuts a tensor into column blocks
// made for thousands of short channels; with C = 1 it launches a workgroup per 4096 elements and merges 100 000 records in one
// wave.  Here a workgroup reads at least CL_MM_ELEMS elements and there are at most CL_MM_MAX_WGS workgroups.
//
// Sums: the two regimes of cnnq_nhwc.hip.h (CL_EXACT_ROWS and its derivation, unchanged: a row here is what a channel is there).
// Above the border four values of a lane are added in fp32 - (v0 + v1) + (v2 + v3), Mom::add4 - and folded into fp64; a row of at
// most CL_EXACT_ROWS elements, and the pieces a lane has left over, are added in fp64 element by element (Mom::add).  The records
// are k_moments' / k_absdev's, merged by k_combine(has_relu) / k_combine_dev(want_kurt) with G = S, C = rows.  Every addition's
// order follows from RowsGeo alone: no atomics, no meeting inside the launch, every record entry stored once by one lane - run
// after run the same bits.  All offsets are 64 bits: len has no 2^31 limit.
//
// Loads are plain (not non-temporal) at every size: following CNNQ_NT_BYTES would take a second set of instances; not A/B-measured.
#pragma once
#include "cnnq_nhwc.hip.h"
#include "cnnq_stats.hip.h"

namespace {

constexpr int ROWS_U = 4;            // pieces of a lane per step of the fp32 regime: 4 * W values, W add4 groups
// steps the compiler overlaps: eight loads of a lane in flight - four of the 16-byte half pieces, whose 32 upconverted values per
// step would otherwise take pass A past 256 VGPRs (one wave per SIMD)
constexpr int rows_unroll(int w) { return w == 8 ? 1 : 2; }

struct RowsGeo {
    int64_t rows, len;   // the view [rows][len]
    int64_t P;           // pieces per row, len / W
    int64_t ppc;         // pieces per chunk
    int S;               // chunks per row
    int exact;           // len <= CL_EXACT_ROWS: fp64 element by element throughout
};

// the workgroup's item `it` of rows * S: (row, first piece, end piece); items are numbered in memory order
struct RowsItem {
    int64_t r, p0, p1;
    int c;
};
__device__ __forceinline__ RowsItem rows_item(const RowsGeo& g, int64_t item) {
    RowsItem w;
    w.r = item / g.S;
    w.c = (int)(item - w.r * g.S);
    w.p0 = (int64_t)w.c * g.ppc;
    w.p1 = w.p0 + g.ppc;
    if (w.p1 > g.P) w.p1 = g.P;
    return w;
}

// ROWS_U pieces of this lane, TPB pieces apart, upconverted: v[k * W + i] = element i of piece k.  The groups of four consecutive
// entries are the add4 groups: the four pieces (W = 1), two pieces each (W = 2), one piece (W = 4), half a piece (W = 8).
template <class T, int W>
__device__ __forceinline__ void rows_ld(const typename ClRaw<T>::type* __restrict__ p, float (&v)[ROWS_U * W]) {
    typedef typename ClRaw<T>::type E;
    E e[ROWS_U][W];
#pragma unroll
    for (int k = 0; k < ROWS_U; ++k) cl_ld<E, W, false>(p + (int64_t)k * TPB * W, e[k]);
#pragma unroll
    for (int k = 0; k < ROWS_U; ++k)
#pragma unroll
        for (int i = 0; i < W; ++i) v[k * W + i] = cl_up(T{}, e[k][i]);
}

// pass A: (row r, chunk c) -> part[c][CNNQ_NMOM][rows], all seven rows; the count is the chunk's exact element count.  The NaN
// rule is k_moments': a sum of squares that came out NaN poisons mn / mx, fmaxf(v, 0) drops a NaN in the rectified sums.
// Workgroups take the items in descending memory order (pass B ascends and re-reads first what this pass read last).
template <class T, int W>
__global__ void __launch_bounds__(TPB) k_rows_moments(const typename ClRaw<T>::type* __restrict__ x, const RowsGeo g,
                                                      double* __restrict__ part) {
    typedef typename ClRaw<T>::type E;
    __shared__ float l_mn[TPB / 64], l_mx[TPB / 64];
    __shared__ double l_s[TPB / 64], l_ss[TPB / 64], l_rs[TPB / 64], l_rss[TPB / 64];
    constexpr int UNR = rows_unroll(W);
    const int t = (int)threadIdx.x;
    const int64_t items = g.rows * g.S;
    for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
        const RowsItem w = rows_item(g, items - 1 - it);
        const E* row = x + w.r * g.len;
        Mom m;
        m.init();
        int64_t p = w.p0 + t;
        if (!g.exact) {
#pragma unroll UNR
            for (; p + (ROWS_U - 1) * TPB < w.p1; p += ROWS_U * TPB) {
                float v[ROWS_U * W];
                rows_ld<T, W>(row + p * W, v);
#pragma unroll
                for (int j = 0; j < W; ++j) {
                    const float q[4] = {v[4 * j], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3]};
                    m.template add4<true>(q);
                }
            }
        }
        for (; p < w.p1; p += TPB) {
            E e[W];
            cl_ld<E, W, false>(row + p * W, e);
#pragma unroll
            for (int i = 0; i < W; ++i) m.template add<true>(cl_up(T{}, e[i]));
        }
        if (m.ss != m.ss) { m.mn = NAN; m.mx = NAN; }
        m.template wave_reduce<true>();
        const int wv = t >> 6;
        if ((t & 63) == 0) { l_mn[wv] = m.mn; l_mx[wv] = m.mx; l_s[wv] = m.s; l_ss[wv] = m.ss; l_rs[wv] = m.rs; l_rss[wv] = m.rss; }
        __syncthreads();
        if (t == 0) {
            Mom a;
            a.init();
            for (int i = 0; i < TPB / 64; ++i) {     // the four wave records in wave order
                Mom o;
                o.mn = l_mn[i]; o.mx = l_mx[i]; o.s = l_s[i]; o.ss = l_ss[i]; o.rs = l_rs[i]; o.rss = l_rss[i];
                a.template merge<true>(o);
            }
            double* rec = part + (size_t)w.c * CNNQ_NMOM * (size_t)g.rows + (size_t)w.r;
            rec[(size_t)CNNQ_MOM_MIN * g.rows] = (double)a.mn;
            rec[(size_t)CNNQ_MOM_MAX * g.rows] = (double)a.mx;
            rec[(size_t)CNNQ_MOM_SUM * g.rows] = a.s;
            rec[(size_t)CNNQ_MOM_SUMSQ * g.rows] = a.ss;
            rec[(size_t)CNNQ_MOM_COUNT * g.rows] = (double)((w.p1 - w.p0) * W);
            rec[(size_t)CNNQ_MOM_SUM_RELU * g.rows] = a.rs;
            rec[(size_t)CNNQ_MOM_SUMSQ_RELU * g.rows] = a.rss;
        }
        __syncthreads();     // the LDS records are free for the next item
    }
}

// pass B: (row r, chunk c) -> part2[c][CNNQ_NDEV][rows], both rows, as k_cl_absdev_kurt forms them: the fp32 subtract of the mean
// of row CNNQ_STAT_MEAN of the merged table, z = (x - mean) * (1 / std) with the fp32 reciprocal formed once per row,
// z^4 = (z * z)^2; the two regimes of pass A.  A constant row (std == 0) gives 0 * inf: its kurtosis is NaN, as in the NCHW chain.
template <class T, int W>
__global__ void __launch_bounds__(TPB) k_rows_absdev(const typename ClRaw<T>::type* __restrict__ x, const RowsGeo g,
                                                     const float* __restrict__ stats, double* __restrict__ part2) {
    typedef typename ClRaw<T>::type E;
    __shared__ double l_a[TPB / 64], l_k[TPB / 64];
    constexpr int UNR = rows_unroll(W);
    const int t = (int)threadIdx.x;
    const int64_t items = g.rows * g.S;
    for (int64_t it = blockIdx.x; it < items; it += gridDim.x) {
        const RowsItem w = rows_item(g, it);
        const E* row = x + w.r * g.len;
        const float mean = stats[(size_t)CNNQ_STAT_MEAN * g.rows + w.r];
        const float sd = 1.f / stats[(size_t)CNNQ_STAT_STD * g.rows + w.r];
        double sa = 0., sk = 0.;
        int64_t p = w.p0 + t;
        if (!g.exact) {
#pragma unroll UNR
            for (; p + (ROWS_U - 1) * TPB < w.p1; p += ROWS_U * TPB) {
                float v[ROWS_U * W];
                rows_ld<T, W>(row + p * W, v);
#pragma unroll
                for (int j = 0; j < W; ++j) {
                    const float d0 = v[4 * j] - mean, d1 = v[4 * j + 1] - mean, d2 = v[4 * j + 2] - mean, d3 = v[4 * j + 3] - mean;
                    const float a0 = fabsf(d0), a1 = fabsf(d1), a2 = fabsf(d2), a3 = fabsf(d3);
                    sa += (double)((a0 + a1) + (a2 + a3));
                    const float z0 = d0 * sd, z1 = d1 * sd, z2 = d2 * sd, z3 = d3 * sd;
                    const float q0 = z0 * z0, q1 = z1 * z1, q2 = z2 * z2, q3 = z3 * z3;
                    sk += (double)((q0 * q0 + q1 * q1) + (q2 * q2 + q3 * q3));
                }
            }
        }
        for (; p < w.p1; p += TPB) {
            E e[W];
            cl_ld<E, W, false>(row + p * W, e);
#pragma unroll
            for (int i = 0; i < W; ++i) {
                const float d = cl_up(T{}, e[i]) - mean;
                sa += (double)fabsf(d);
                const float z = d * sd;
                const float q = z * z;
                sk += (double)(q * q);
            }
        }
#pragma unroll
        for (int msk = 32; msk >= 1; msk >>= 1) { sa += shfl_xor_d(sa, msk); sk += shfl_xor_d(sk, msk); }
        const int wv = t >> 6;
        if ((t & 63) == 0) { l_a[wv] = sa; l_k[wv] = sk; }
        __syncthreads();
        if (t == 0) {
            double ra = 0., rk = 0.;
            for (int i = 0; i < TPB / 64; ++i) { ra += l_a[i]; rk += l_k[i]; }
            double* rec = part2 + (size_t)w.c * CNNQ_NDEV * (size_t)g.rows + (size_t)w.r;
            rec[(size_t)CNNQ_DEV_ABS * g.rows] = ra;
            rec[(size_t)CNNQ_DEV_Z4 * g.rows] = rk;
        }
        __syncthreads();
    }
}

// ---- host side: the geometry for piece width w
// S = the chunks per row: as many as leave every full chunk at least CL_MM_ELEMS elements, at most CL_MM_MAX_WGS workgroups over
// all rows (so S * rows <= CL_MM_MAX_WGS, far below CL_PMM_MAX, whenever a row is cut at all); beyond CL_MM_MAX_WGS rows a row is
// one chunk and the workgroups stride over the rows.
inline RowsGeo rows_geo(int64_t rows, int64_t len, int w) {
    RowsGeo g;
    g.rows = rows;
    g.len = len;
    g.P = len / w;
    const int64_t minp = (CL_MM_ELEMS + w - 1) / w;
    int64_t s = g.P / minp;
    const int64_t cap = CL_MM_MAX_WGS / rows;
    if (s > cap) s = cap;
    if (s < 1) s = 1;
    g.ppc = (g.P + s - 1) / s;
    g.S = (int)((g.P + g.ppc - 1) / g.ppc);
    g.exact = len <= CL_EXACT_ROWS ? 1 : 0;
    return g;
}
inline dim3 rows_grid(const RowsGeo& g) {
    const int64_t items = g.rows * g.S;
    return dim3((unsigned)(items < CL_MM_MAX_WGS ? items : CL_MM_MAX_WGS));
}

}  // namespace
