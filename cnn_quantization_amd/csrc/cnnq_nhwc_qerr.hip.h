// cnnq_nhwc_qerr.hip.h - the per-channel clipping-error columns of `-c mix` (mse_* / cos_* of smpc.py:80-100; cnnq_qerr.hip.h is
// the NCHW form) on dense channels_last (NHWC) activations, for fp32, bf16 and fp16 elements: K candidate quantizations from ONE
// read of x on the storage as it lies - no layout copy, no upcast, no quantized tensor written.
// Part of the single translation unit cnnq_kernels.hip (see its header for the design).
//
// The contract: the columns are those of the exactly upconverted x (cl_up), each term one fp32 operation,
// q_k the fp32 value k_cl_qdq computes with table k before it converts to x's dtype; against fp64 sums of those terms within the
// project's tier (ii).  The records are k_qerr's row records rec[n * nb + p][QE_NV(K)][C] (fp64), p the slab of the sample's HW
// rows, and k_qerr_fold<K> folds them unchanged - rows, not channels, because the cosine takes a root per (n, c) row.
//
// Tiling: cnnq_nhwc.hip.h's, planned per SAMPLE - ClGeo over R = HW rows with S slabs, and the grid N * S * nb: workgroup
// (n * S + s) * nb + b owns column block b of slab s of sample n, so a slab never crosses a sample boundary (the slabs of the
// other channels_last reductions run over N * HW and do).  A lane keeps one piece of W consecutive channels for its whole life:
// its QE_NV(K) * W running sums and its 3 * K * W parameters stay in registers, and a sample's row costs no barrier until the
// slab's end (k_qerr pays one barrier and one LDS fold per sample and load slot).  Pieces are at most CL_QE_WMAX = 2 elements
// wide here whatever the element type: at K = 3 a piece of 4 keeps 40 fp64 sums and 48 parameters per lane - about 260 VGPRs,
// one wave per SIMD - and measured 18 % slower than a piece of 2 (about 160 VGPRs, three waves); the pass is bound by
// instruction issue, not by the width of its loads (profiles/channels_last_qerr.md).
//
// Sums: CL_FOLD rows are added in fp32 - (t0 + t1) + (t2 + t3) - and folded into an fp64 accumulator, a lane's leftover rows in
// fp64 term by term.  Unlike the variance of k_cl_moments nothing here cancels (every term but x q is a square, and q is x's
// own rounding), so the three fp32 roundings per partial, each 6e-8 relative to a four-term sum, stay far inside the 2e-6 tier at
// every size and both regimes apply at every size.  The order of the additions is fixed by the geometry alone; no atomics; every
// record entry is stored once by one lane (cl_fold_sums): run after run the same bits.
#pragma once
#include "cnnq_nhwc.hip.h"
#include "cnnq_qerr.hip.h"

namespace {

constexpr int CL_QE_WMAX = 2;        // the widest piece of k_cl_qerr, elements (4 was measured: profiles/channels_last_qerr.md)

// the QE_NV(K) terms of one element: x^2, then per candidate (x - q)^2, x q, q^2 - one fp32 operation each
template <int K, bool FAST>
__device__ __forceinline__ void cl_qe_terms(float v, const float (&sc)[K], const float (&rs)[K], const float (&zp)[K],
                                            const float (&qm)[K], float (&t)[QE_NV(K)]) {
    t[0] = v * v;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        float cd;
        const float q = FAST ? qdq1_fast(v, sc[k], rs[k], zp[k], qm[k], cd) : qdq1(v, sc[k], zp[k], qm[k], cd);
        const float d = v - q;
        t[1 + 3 * k] = d * d;
        t[2 + 3 * k] = v * q;
        t[3 + 3 * k] = q * q;
    }
}

// g: the geometry of ONE sample (g.R = HW); gridDim.x = N * g.S * g.nb.  x is read for the last time by a collect step:
// non-temporal loads.  mm != NULL: the channel extrema [2][C]; a workgroup whose channels all satisfy qdq_fast_domain and have no
// NaN zero point / qmax for every candidate takes the divide-free quotient (the same function there), any other the IEEE divide
// - a workgroup-uniform choice, k_qerr's rule.
template <class T, int W, int K>
__global__ void __launch_bounds__(TPB) k_cl_qerr(const typename ClRaw<T>::type* __restrict__ x, const ClGeo g,
                                                 const float* __restrict__ qp, const float* __restrict__ mm,
                                                 double* __restrict__ rec) {
    typedef typename ClRaw<T>::type E;
    constexpr int NV = QE_NV(K);
    __shared__ double l_d[TPB * W];
    const int per = g.S * g.nb;
    const int n = (int)blockIdx.x / per, wg = (int)blockIdx.x - n * per;
    const ClLane l = cl_lane(g, wg);
    double acc[NV][W];
#pragma unroll
    for (int vi = 0; vi < NV; ++vi)
#pragma unroll
        for (int i = 0; i < W; ++i) acc[vi][i] = 0.;
    float sc[W][K], rs[W][K], zp[W][K], qm[W][K];
    int fast_ok = mm != nullptr;
    if (l.piece >= 0) {
        const int c0 = l.piece * W;
#pragma unroll
        for (int i = 0; i < W; ++i)
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const float* t = qp + (size_t)k * CNNQ_NQP * g.C + c0 + i;
                sc[i][k] = t[(size_t)CNNQ_QP_SCALE * g.C];
                zp[i][k] = t[(size_t)CNNQ_QP_ZP * g.C];
                qm[i][k] = t[(size_t)CNNQ_QP_QMAX * g.C];
                // a NaN zero point or qmax must keep qdq1's compare+select clamp (k_qerr, cnnq_qerr.hip.h)
                if (mm != nullptr)
                    fast_ok &= (qdq_fast_domain(mm[c0 + i], mm[g.C + c0 + i], sc[i][k]) && zp[i][k] == zp[i][k] && qm[i][k] == qm[i][k])
                                   ? 1 : 0;
            }
    }
    const bool fast = __syncthreads_and(fast_ok) != 0;
    if (l.piece >= 0) {
#pragma unroll
        for (int i = 0; i < W; ++i)
#pragma unroll
            for (int k = 0; k < K; ++k) rs[i][k] = fast ? 1.0f / sc[i][k] : 0.f;
        const E* xs = x + (int64_t)n * g.R * g.C + (int64_t)l.piece * W;
        const int64_t step = (int64_t)g.RS * g.C;
        auto walk = [&](auto FASTC) {
            constexpr bool FAST = decltype(FASTC)::value != 0;
            const E* p = xs + l.r * g.C;
            int64_t r = l.r;
            for (; r + (CL_FOLD - 1) * (int64_t)g.RS < l.r1; r += (int64_t)CL_FOLD * g.RS, p += CL_FOLD * step) {
                E e[CL_FOLD][W];
#pragma unroll
                for (int j = 0; j < CL_FOLD; ++j) cl_ld<E, W, true>(p + j * step, e[j]);
#pragma unroll
                for (int i = 0; i < W; ++i) {
                    float t[CL_FOLD][NV];
#pragma unroll
                    for (int j = 0; j < CL_FOLD; ++j) cl_qe_terms<K, FAST>(cl_up(T{}, e[j][i]), sc[i], rs[i], zp[i], qm[i], t[j]);
#pragma unroll
                    for (int vi = 0; vi < NV; ++vi) acc[vi][i] += (double)((t[0][vi] + t[1][vi]) + (t[2][vi] + t[3][vi]));
                }
            }
            for (; r < l.r1; r += g.RS, p += step) {
                E e[W];
                cl_ld<E, W, true>(p, e);
#pragma unroll
                for (int i = 0; i < W; ++i) {
                    float t[NV];
                    cl_qe_terms<K, FAST>(cl_up(T{}, e[i]), sc[i], rs[i], zp[i], qm[i], t);
#pragma unroll
                    for (int vi = 0; vi < NV; ++vi) acc[vi][i] += (double)t[vi];
                }
            }
        };
        if (fast) walk(IntC<1>{});
        else walk(IntC<0>{});
    }
    const int s = wg / g.nb, b = wg - s * g.nb;
    double* out = rec + ((size_t)n * g.S + s) * NV * g.C;
#pragma unroll
    for (int vi = 0; vi < NV; ++vi) cl_fold_sums<W>(l_d, g, b, acc[vi], out + (size_t)vi * g.C);
}

// ---- host side: the plan of one sample
// The slabs a sample's HW rows are cut into - a function of (N, HW, C) alone, not of the piece width, so that the record count
// is known before the alignment is: about CL_QE_ELEMS elements per workgroup (a column block counted as min(C, TPB * CL_QE_WMAX)
// channels), and no more slabs than keep N * S at CL_QE_MAX_WGS workgroups - a batch that fills the device by its samples is not
// cut.  Every slab costs QE_NV(K) * C fp64 record entries and, more to the point, one more step of k_qerr_fold's walk over a
// channel's N * S records, which C / QF_CH workgroups make one after the other: 512 measured fastest of 512 .. 8192 on every
// ResNet-50 class at batch 512 and 64 (profiles/channels_last_qerr.md).
constexpr int64_t CL_QE_ELEMS = 65536;
constexpr int64_t CL_QE_MAX_WGS = 512;
inline int cl_qe_slabs(int64_t N, int64_t HW, int64_t C) {
    const int64_t colw = C < (int64_t)TPB * CL_QE_WMAX ? C : (int64_t)TPB * CL_QE_WMAX;
    const int64_t rows = (CL_QE_ELEMS + colw - 1) / colw;
    int64_t S = (HW + rows - 1) / rows;
    const int64_t cap = CL_QE_MAX_WGS / N;
    if (S > cap) S = cap;
    return (int)(S < 1 ? 1 : S);
}
inline int cl_qe_piece(int64_t C, int esize, int64_t align_bytes) {
    const int w = cl_piece(C, esize, align_bytes);
    return w > CL_QE_WMAX ? CL_QE_WMAX : w;
}
// geometry of one sample for piece width w: S = cl_qe_slabs slabs of rpw rows, rpw a multiple of RS with S * rpw >= HW (a
// trailing slab left without rows stores zero records)
inline ClGeo cl_geo_qe(int64_t N, int64_t HW, int64_t C, int w) {
    ClGeo g;
    g.R = HW;
    g.C = (int)C;
    g.P = (int)(C / w);
    g.CP = g.P < TPB ? g.P : TPB;
    g.RS = TPB / g.CP;
    g.nb = (g.P + g.CP - 1) / g.CP;
    g.S = cl_qe_slabs(N, HW, C);
    const int64_t rows = (HW + g.S - 1) / g.S;
    g.rpw = (rows + g.RS - 1) / g.RS * g.RS;
    return g;
}

}  // namespace
