// cnnq_flat.hip.h - the element-wise Q/DQ of a WHOLE tensor with ONE parameter set, over flat storage, for fp32, bf16 and fp16
// elements: the per-tensor clipping branch (iq.py:353-357: `gemmlowpClippingQuantize` where -pcq_a does not apply) and the
// per-tensor mid-tread branch (iq.py:158-168).  y[i] depends on x[i] and the tensor's scalars alone, so a contiguous tensor and a
// dense channels_last one are the same n elements here: quantized on the storage as it lies, no layout copy and no upcast.
// Part of the single translation unit cnnq_kernels.hip (see its header for the design).
//
// The arithmetic is the per-channel kernels' (DESIGN.md section 22): qdq1 - IEEE divide, separately rounded add, clamp before
// round, half to even - and k_mt_qdq<CLIP>'s round / two clamps / multiply, on column 0 of the tables cnnq_pc_params
// (direct_range = 1) and cnnq_pc_midtread_params (clip = 1) write for C = 1.  Given the table, y is what cnnq_pc_qdq /
// cnnq_pc_midtread_qdq give for N = 1, C = 1, HW = n on the same values, bit for bit; bf16 / fp16 elements are upconverted
// exactly, go through that fp32 arithmetic, and the fp32 result - made opaque first (h_down) - is rounded to nearest-even once.
// There is no divide-free quotient here (qdq1_fast wants the tensor's exact extrema, which a statistics table does not bound):
// not A/B-measured, left out.
//
// Tiling: x is cut into pieces of W elements, W the widest of 16 / 8 / 4 / 2 bytes (or one element) that the alignment x and y
// share allows - the length does not enter: the n % W elements behind the last piece are taken by the first lanes of workgroup 0,
// as k_h_pt_qdq takes them.  A workgroup owns FLAT_U * TPB consecutive pieces (16 KB of x at 16-byte pieces: many short
// workgroups in address order, as k_qdq / k_h_qdq), lane t the pieces t, t + TPB, ...: every load and store of a wave is one
// contiguous run.  x is read and y written non-temporally.  The three scalars are read through a uniform address: one scalar
// load per workgroup, no LDS.
#pragma once
#include "cnnq_nhwc.hip.h"

namespace {

constexpr int FLAT_U = 4;    // pieces per lane

// the pieces [p0, p0 + FLAT_U * TPB) of this workgroup through f (fp32 in, fp32 out), then the tail elements
template <class T, int W, class F>
__device__ __forceinline__ void flat_apply(const typename ClRaw<T>::type* __restrict__ x, typename ClRaw<T>::type* __restrict__ y,
                                           const int64_t n, F&& f) {
    typedef typename ClRaw<T>::type E;
    const int64_t nv = n / W;
    const int64_t p0 = (int64_t)blockIdx.x * (FLAT_U * TPB) + threadIdx.x;
    E e[FLAT_U][W];
#pragma unroll
    for (int k = 0; k < FLAT_U; ++k)
        if (p0 + k * TPB < nv) cl_ld<E, W, true>(x + (p0 + k * TPB) * W, e[k]);
#pragma unroll
    for (int k = 0; k < FLAT_U; ++k)
        if (p0 + k * TPB < nv) {
#pragma unroll
            for (int i = 0; i < W; ++i) e[k][i] = cl_down(T{}, f(cl_up(T{}, e[k][i])));
            cl_st_nt<E, W>(y + (p0 + k * TPB) * W, e[k]);
        }
    if constexpr (W > 1) {
        const int64_t t = nv * W + threadIdx.x;
        if (blockIdx.x == 0 && threadIdx.x < W && t < n) y[t] = cl_down(T{}, f(cl_up(T{}, x[t])));
    }
}

// y = dequant(quant(x)) with scale / zero point / qmax of qp[CNNQ_NQP][1]
template <class T, int W>
__global__ void __launch_bounds__(TPB) k_flat_qdq(const typename ClRaw<T>::type* __restrict__ x, typename ClRaw<T>::type* __restrict__ y,
                                                  const int64_t n, const float* __restrict__ qp) {
    const float sc = qp[CNNQ_QP_SCALE], zp = qp[CNNQ_QP_ZP], qm = qp[CNNQ_QP_QMAX];
    flat_apply<T, W>(x, y, n, [=](float v) {
        float cd;
        return qdq1(v, sc, zp, qm, cd);
    });
}

// y = clamp(round(x / Delta), c_min, c_max) * Delta with the row entries of mt[CNNQ_NMT][1] (iq.py:202-224; k_mt_qdq<CLIP>)
template <class T, int W>
__global__ void __launch_bounds__(TPB) k_flat_midtread(const typename ClRaw<T>::type* __restrict__ x,
                                                       typename ClRaw<T>::type* __restrict__ y, const int64_t n,
                                                       const float* __restrict__ mt) {
    const float d = mt[CNNQ_MT_DELTA], lo = mt[CNNQ_MT_CMIN], hi = mt[CNNQ_MT_CMAX];
    flat_apply<T, W>(x, y, n, [=](float v) {
        float t = rintf(v / d);
        // torch.min(t, hi) / torch.max(t, lo): NaN kept, the bound wins ties (iq.py:213-214)
        t = (t < hi || t != t) ? t : hi;
        t = (t > lo || t != t) ? t : lo;
        return t * d;
    });
}

// ---- host side: the piece width and the grid
inline int flat_piece(int esize, int align_bytes) { return cl_piece(16, esize, align_bytes); }
// workgroups for n elements at piece width w (at least one: a tensor shorter than a piece is all tail)
inline int64_t flat_blocks(int64_t n, int w) {
    const int64_t b = (n / w + (int64_t)FLAT_U * TPB - 1) / ((int64_t)FLAT_U * TPB);
    return b < 1 ? 1 : b;
}

}  // namespace
