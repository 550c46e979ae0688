// cnnq_nhwc_bcorr.hip.h - activation bias correction (iqm.py:180-196) on dense channels_last (NHWC) activations with a parameter
// table (-sm use): the per-channel sums of the correction over [R = N*H*W][C] storage and the fused quantize + correct pass, for
// fp32, bf16 and fp16 elements.
// Part of the single translation unit cnnq_kernels.hip (see its header for the design).
//
// The NCHW pair is k_bcorr_sums<FROMX> / k_qdq_bias (cnnq_corrections.hip.h); k_bcorr_bias between the two passes is that
// chain's own, on the records written here.  The contract: the sums against fp64 within the statistics
// tier (the count exact), and given the sums every output bit for bit - bias is k_bcorr_bias' arithmetic, y is k_qdq_bias'
// expression on the exactly upconverted values with one round-to-nearest-even into the element type at the end.  The sums are
// added in an order fixed by the geometry (ClGeo) alone - not the NCHW chain's - and run after run the same: no atomics, every
// record entry stored once by one lane.
//
// Tiling, the two summation regimes and the LDS meeting of the sums: cnnq_nhwc.hip.h (k_cl_moments' geometry for the sums,
// k_cl_qdq's for the second pass).  The bias is the small difference (sum x' - sum q) / count, which magnifies the roundings of
// either sum as the variance does in pass A of config 3: the same border, CL_EXACT_ROWS, keeps a channel of few elements exact.
#pragma once
#include "cnnq_nhwc.hip.h"

namespace {

// pass 1, read-only: slab s -> part3[s][3][C] = {sum x', sum q, count(x' > 0)} with q = qdq1(x) from the table qp (the fp32
// value, not the one rounded to the element type) and x' = relu(x) when the layer feeds a ReLU.  The IEEE divide: a calibration
// table does not bound the values.  Workgroups ascend; the second pass descends and re-reads first what was read last.
template <class T, int W>
__global__ void __launch_bounds__(TPB) k_cl_bcorr_sums(const typename ClRaw<T>::type* __restrict__ x, const ClGeo g,
                                                       const int relu_first, const float* __restrict__ qp,
                                                       double* __restrict__ part3) {
    typedef typename ClRaw<T>::type E;
    __shared__ double l_d[TPB * W];
    const int bid = (int)blockIdx.x;
    const ClLane l = cl_lane(g, bid);
    double sx[W], sq[W];
    unsigned cn[W];                          // exact: a lane walks fewer than 2^31 rows (the host refuses longer slabs)
#pragma unroll
    for (int i = 0; i < W; ++i) { sx[i] = 0.; sq[i] = 0.; cn[i] = 0u; }
    if (l.piece >= 0) {
        const int c0 = l.piece * W;
        float sc[W], zp[W], qm[W];
#pragma unroll
        for (int i = 0; i < W; ++i) {
            sc[i] = qp[(size_t)CNNQ_QP_SCALE * g.C + c0 + i];
            zp[i] = qp[(size_t)CNNQ_QP_ZP * g.C + c0 + i];
            qm[i] = qp[(size_t)CNNQ_QP_QMAX * g.C + c0 + i];
        }
        const E* p = x + l.r * g.C + c0;
        const int64_t step = (int64_t)g.RS * g.C;
        int64_t r = l.r;
        if (g.R > CL_EXACT_ROWS) {
            for (; r + (CL_FOLD - 1) * (int64_t)g.RS < l.r1; r += (int64_t)CL_FOLD * g.RS, p += CL_FOLD * step) {
                E e[CL_FOLD][W];
#pragma unroll
                for (int k = 0; k < CL_FOLD; ++k) cl_ld<E, W, false>(p + k * step, e[k]);
#pragma unroll
                for (int i = 0; i < W; ++i) {
                    float v[CL_FOLD], q[CL_FOLD];
#pragma unroll
                    for (int k = 0; k < CL_FOLD; ++k) {
                        float cd;
                        v[k] = cl_up(T{}, e[k][i]);
                        q[k] = qdq1(v[k], sc[i], zp[i], qm[i], cd);
                        if (relu_first) v[k] = fmaxf(v[k], 0.f);
                        cn[i] += (v[k] > 0.f) ? 1u : 0u;
                    }
                    sx[i] += (double)((v[0] + v[1]) + (v[2] + v[3]));
                    sq[i] += (double)((q[0] + q[1]) + (q[2] + q[3]));
                }
            }
        }
        for (; r < l.r1; r += g.RS, p += step) {
            E e[W];
            cl_ld<E, W, false>(p, e);
#pragma unroll
            for (int i = 0; i < W; ++i) {
                float cd;
                float v = cl_up(T{}, e[i]);
                const float q = qdq1(v, sc[i], zp[i], qm[i], cd);
                if (relu_first) v = fmaxf(v, 0.f);
                cn[i] += (v > 0.f) ? 1u : 0u;
                sx[i] += (double)v;
                sq[i] += (double)q;
            }
        }
    }
    const int sl = bid / g.nb, b = bid - sl * g.nb;
    double* rec = part3 + (size_t)sl * 3 * g.C;
    cl_fold_sums<W>(l_d, g, b, sx, rec);
    cl_fold_sums<W>(l_d, g, b, sq, rec + (size_t)g.C);
    // the counts: integers below 2^53, exact in fp64 whatever the order
#pragma unroll
    for (int i = 0; i < W; ++i) sx[i] = (double)cn[i];
    cl_fold_sums<W>(l_d, g, b, sx, rec + (size_t)2 * g.C);
}

// pass 2: y = q + (q > 0) * bias[c] with q = qdq1(x) (k_qdq_bias' expression), rounded once into the element type; k_cl_qdq's
// geometry, descending dispatch and non-temporal load and store
template <class T, int W>
__global__ void __launch_bounds__(TPB) k_cl_qdq_bias(const typename ClRaw<T>::type* __restrict__ x,
                                                     typename ClRaw<T>::type* __restrict__ y, const ClGeo g,
                                                     const float* __restrict__ qp, const float* __restrict__ bias) {
    typedef typename ClRaw<T>::type E;
    const ClLane l = cl_lane(g, (int)gridDim.x - 1 - (int)blockIdx.x);
    if (l.piece < 0) return;
    const int c0 = l.piece * W;
    float sc[W], zp[W], qm[W], qb[W];
#pragma unroll
    for (int i = 0; i < W; ++i) {
        sc[i] = qp[(size_t)CNNQ_QP_SCALE * g.C + c0 + i];
        zp[i] = qp[(size_t)CNNQ_QP_ZP * g.C + c0 + i];
        qm[i] = qp[(size_t)CNNQ_QP_QMAX * g.C + c0 + i];
        qb[i] = bias[c0 + i];
    }
    const int64_t step = (int64_t)g.RS * g.C;
    int64_t off = l.r * g.C + c0;
    for (int64_t r = l.r; r < l.r1; r += g.RS, off += step) {
        E e[W];
        cl_ld<E, W, true>(x + off, e);
#pragma unroll
        for (int i = 0; i < W; ++i) {
            float cd;
            const float q = qdq1(cl_up(T{}, e[i]), sc[i], zp[i], qm[i], cd);
            e[i] = cl_down(T{}, q + ((q > 0.f) ? 1.f : 0.f) * qb[i]);
        }
        cl_st_nt<E, W>(y + off, e);
    }
}

}  // namespace
