// cnnq_qerr.hip.h - per-channel clipping-error columns (mse_* / cos_* of smpc.py:80-100) of K candidate quantizations from ONE
// read of x: no quantized tensor is ever written.
// Part of the single translation unit cnnq_kernels.hip (see its header for the design).
#pragma once
#include "cnnq_common.hip.h"
#include "cnnq_qdq.hip.h"
#include "cnnq_stats.hip.h"

namespace {

// Row records rec[N * nb][QE_NV(K)][C] (fp64): per sample n, piece bb of the channel's row (nb > 1 only when a workgroup owns a
// slice of one channel) and channel c: sum x^2, then per candidate k: sum (x - q_k)^2, sum x q_k, sum q_k^2.  Rows, not
// channels: the cosine of utils/misc.py:23-34 with dims = [-1, 0] takes a square root per (n, c) row before it sums over n.
__host__ __device__ constexpr int QE_NV(int K) { return 1 + 3 * K; }

// q of one candidate for a float4 of ONE channel, two elements per instruction where the divide-free quotient applies
template <bool FAST>
__device__ __forceinline__ void qerr_q4(const float (&x)[4], float sc, float rs, float zp, float qm, f2v& q0, f2v& q1) {
    if constexpr (FAST) {
        const f2v s2 = {sc, sc}, r2 = {rs, rs}, z2 = {zp, zp};
        f2v c;
        q0 = qdq2_fast(f2v{x[0], x[1]}, s2, r2, z2, qm, c);
        q1 = qdq2_fast(f2v{x[2], x[3]}, s2, r2, z2, qm, c);
    } else {
        float c;
        q0 = f2v{qdq1(x[0], sc, zp, qm, c), qdq1(x[1], sc, zp, qm, c)};
        q1 = f2v{qdq1(x[2], sc, zp, qm, c), qdq1(x[3], sc, zp, qm, c)};
    }
}

// Every workgroup walks its column block down its samples (the decomposition of k_absdev).  Nothing is carried from one sample
// to the next: per sample a lane forms the fp32 sums of its own J * VEC elements (each term one fp32 operation, as the
// reference's elementwise ops form it), the workgroup folds them per channel in fp64 through LDS (seg_of(entries) lanes per
// (channel, sum) pair, the xor tree of the statistics passes) and stores the row record - plain stores, each written by exactly
// one lane, no atomics.  The LDS tile is double buffered where it fits (one barrier per sample).
// x is read for the last time by a collect step: non-temporal loads throughout.
// mm != NULL: the channel extrema; a workgroup whose channels all satisfy qdq_fast_domain (and have no NaN zero point / qmax)
// for every candidate takes the divide-free quotient (the same function there), any other the IEEE divide - a workgroup-uniform choice.
template <int VEC, int A, int J, int K, bool MM>
__global__ void __launch_bounds__(TPB) k_qerr(const float* __restrict__ x, const Geo g, const float* __restrict__ qp,
                                              const float* __restrict__ mm, double* __restrict__ rec) {
    constexpr int NV = QE_NV(K);
    constexpr int NE = TPB * J * A;
    constexpr int NBUF = (NE > 512) ? 1 : 2;
    __shared__ float l_p[NBUF][NV][NE];
    __shared__ float sh_sc[K][MAXCH], sh_zp[K][MAXCH], sh_qm[K][MAXCH];

    const Blk b = blk_of<VEC>(g);
    const int tid = threadIdx.x;
    const int nch = b.c1 - b.c0;
    int fast_ok = 1;
    for (int i = tid; i < nch; i += TPB) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const float* t = qp + (size_t)k * CNNQ_NQP * g.C + b.c0 + i;
            const float s = t[(size_t)CNNQ_QP_SCALE * g.C];
            const float z = t[(size_t)CNNQ_QP_ZP * g.C], q = t[(size_t)CNNQ_QP_QMAX * g.C];
            sh_sc[k][i] = s;
            sh_zp[k][i] = z;
            sh_qm[k][i] = q;
            // a NaN zero point or qmax (bit allocation poisoned by a NaN / Inf statistic of ANY channel) must keep qdq1's
            // compare+select clamp: v_med3_f32 treats a NaN bound differently (as aciq_fast_domain, cnnq_aciq.hip.h)
            if constexpr (MM) fast_ok &= (qdq_fast_domain(mm[b.c0 + i], mm[g.C + b.c0 + i], s) && z == z && q == q) ? 1 : 0;
        }
    }
    const bool fast = MM ? (__syncthreads_and(fast_ok) != 0) : false;
    if constexpr (!MM) __syncthreads();

    int col[J];
    bool ok[J];
    float sc[J][A][K], rs[J][A][K], zp[J][A][K], qm[J][A][K];
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int c = b.col0 + j * TPB + tid;
        ok[j] = c < b.col1;
        col[j] = ok[j] ? c : b.col0;
#pragma unroll
        for (int a = 0; a < A; ++a) {
            const unsigned e = (unsigned)col[j] * VEC + (A == 1 ? 0 : a);
            const int ch = (int)(e / (unsigned)g.HW) - b.c0;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                sc[j][a][k] = sh_sc[k][ch];
                rs[j][a][k] = 1.0f / sc[j][a][k];
                zp[j][a][k] = sh_zp[k][ch];
                qm[j][a][k] = sh_qm[k][ch];
            }
        }
    }
    // LDS entries per channel; a slice of one channel (mode 1) is one of nb pieces of its row
    const int epc = (g.mode == 1) ? (b.col1 - b.col0) : g.HW * A / VEC;
    const int nb = (g.mode == 1) ? g.nb : 1;
    const int bb = (g.mode == 1) ? b.grp % g.nb : 0;
    const int nrows = b.n1 - b.n0;

    auto walk = [&](auto FASTC) {
        constexpr bool FAST = decltype(FASTC)::value != 0;
        for (int r = 0; r < nrows; ++r) {
            const int n = b.n0 + r;
            const float* row = x + (size_t)n * (size_t)g.P;
            float (*lp)[NE] = l_p[NBUF == 1 ? 0 : (r & 1)];
            float v[J][VEC];
#pragma unroll
            for (int j = 0; j < J; ++j) ldv_nt<VEC>(row + (size_t)col[j] * VEC, v[j]);
#pragma unroll
            for (int j = 0; j < J; ++j) {
                if (!ok[j]) continue;
                const int e0 = (j * TPB + tid) * A;
                if constexpr (VEC == 4 && A == 1) {
                    const f2v x0 = {v[j][0], v[j][1]}, x1 = {v[j][2], v[j][3]};
                    const f2v xx = x0 * x0 + x1 * x1;
                    lp[0][e0] = xx.x + xx.y;
#pragma unroll
                    for (int k = 0; k < K; ++k) {
                        f2v q0, q1;
                        qerr_q4<FAST>(v[j], sc[j][0][k], rs[j][0][k], zp[j][0][k], qm[j][0][k], q0, q1);
                        const f2v d0 = x0 - q0, d1 = x1 - q1;
                        const f2v dd = d0 * d0 + d1 * d1;
                        const f2v xq = x0 * q0 + x1 * q1;
                        const f2v qq = q0 * q0 + q1 * q1;
                        lp[1 + 3 * k][e0] = dd.x + dd.y;
                        lp[2 + 3 * k][e0] = xq.x + xq.y;
                        lp[3 + 3 * k][e0] = qq.x + qq.y;
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < VEC; ++e) {   // VEC == 1, or a float4 that may straddle channels: per element
                        const int a = (A == 1 ? 0 : e);
                        const float xv = v[j][e];
                        lp[0][e0 + a] = xv * xv;
#pragma unroll
                        for (int k = 0; k < K; ++k) {
                            float cd;
                            const float q = FAST ? qdq1_fast(xv, sc[j][a][k], rs[j][a][k], zp[j][a][k], qm[j][a][k], cd)
                                                 : qdq1(xv, sc[j][a][k], zp[j][a][k], qm[j][a][k], cd);
                            const float d = xv - q;
                            lp[1 + 3 * k][e0 + a] = d * d;
                            lp[2 + 3 * k][e0 + a] = xv * q;
                            lp[3 + 3 * k][e0 + a] = q * q;
                        }
                    }
                }
            }
            __syncthreads();
            double* out = rec + ((size_t)n * nb + bb) * NV * g.C;
            auto fold = [&](auto SEGC) {
                constexpr int SEG = decltype(SEGC)::value;
                const int items = nch * NV;
                for (int base = 0; base < items; base += TPB / SEG) {   // uniform: whole waves take part in the shuffles
                    const int it = base + tid / SEG, l = tid & (SEG - 1);
                    const int i = it / NV, vi = it - i * NV;
                    double t = 0.;
                    if (it < items)
                        for (int e = i * epc + l; e < (i + 1) * epc; e += SEG) t += (double)lp[vi][e];
#pragma unroll
                    for (int m = SEG >> 1; m >= 1; m >>= 1) t += shfl_xor_d(t, m);
                    if (it < items && l == 0) out[(size_t)vi * g.C + b.c0 + i] = t;
                }
            };
            CNNQ_SEG_DISPATCH(seg_of(epc), fold);
            if constexpr (NBUF == 1) __syncthreads();
        }
    };
    if (fast) walk(IntC<1>{});
    else walk(IntC<0>{});
}

// rec -> err[2K][C] (fp32): rows mse_0..K-1 (smpc.py:84: the mean over n of the mean over hw), then cos_0..K-1
// (utils/misc.py:23-34 with dims = [-1, 0] as written: dot / (sqrt(sum_n sqrt(sum_hw x^2)) sqrt(sum_n sqrt(sum_hw q^2))) - the
// root is taken inside the loop over the dimensions, hence nested).  fp64 throughout, rounded once.  32 channels x 8 slices of
// the batch per workgroup (coalesced record reads); the slices meet in LDS and are added in slice order.
constexpr int QF_CH = 32, QF_SL = TPB / QF_CH;
template <int K>
__global__ void __launch_bounds__(TPB) k_qerr_fold(const double* __restrict__ rec, int N, int nb, int C, int HW,
                                                   float* __restrict__ err) {
    constexpr int NV = QE_NV(K);
    constexpr int NA = 1 + 3 * K;   // per channel: sum_n sqrt(xx), then per k: sum_n dd / HW, sum_n xq, sum_n sqrt(qq)
    __shared__ double l_a[QF_SL][NA][QF_CH];
    const int cx = threadIdx.x % QF_CH, sl = threadIdx.x / QF_CH;
    const int c = blockIdx.x * QF_CH + cx;
    double acc[NA];
#pragma unroll
    for (int i = 0; i < NA; ++i) acc[i] = 0.;
    if (c < C)
        for (int n = sl; n < N; n += QF_SL) {
            double row[NV];
#pragma unroll
            for (int vi = 0; vi < NV; ++vi) row[vi] = 0.;
            for (int p = 0; p < nb; ++p) {
                const double* r = rec + ((size_t)n * nb + p) * NV * C + c;
#pragma unroll
                for (int vi = 0; vi < NV; ++vi) row[vi] += r[(size_t)vi * C];
            }
            acc[0] += sqrt(row[0]);
#pragma unroll
            for (int k = 0; k < K; ++k) {
                acc[1 + 3 * k] += row[1 + 3 * k] / (double)HW;
                acc[2 + 3 * k] += row[2 + 3 * k];
                acc[3 + 3 * k] += sqrt(row[3 + 3 * k]);
            }
        }
#pragma unroll
    for (int i = 0; i < NA; ++i) l_a[sl][i][cx] = acc[i];
    __syncthreads();
    if (sl != 0 || c >= C) return;
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        double t = 0.;
        for (int s = 0; s < QF_SL; ++s) t += l_a[s][i][cx];
        acc[i] = t;
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
        err[(size_t)k * C + c] = (float)(acc[1 + 3 * k] / (double)N);
        err[(size_t)(K + k) * C + c] = (float)(acc[2 + 3 * k] / (sqrt(acc[0]) * sqrt(acc[3 + 3 * k])));
    }
}

}  // namespace
