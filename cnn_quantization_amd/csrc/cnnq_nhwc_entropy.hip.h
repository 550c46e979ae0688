// cnnq_nhwc_entropy.hip.h - the uniform per-channel Q/DQ that counts its codes (-me, iq.py:586-587: the codes exist in the
// reference only as the argument of shannon_entropy) on dense channels_last (NHWC) activations: one pass over
// [R = N*H*W][C] storage, for fp32, bf16 and fp16 elements.
// Part of the single translation unit cnnq_kernels.hip (see its header for the design).
//
// Everything around the pass is layout-free and the NCHW chain's own: the parameter table comes from k_minmax_params on
// k_cl_minmax's partials (config 2), from k_params on cl_table's statistics (config 3) or from the caller; the counts go to the
// XHIST_REPLICAS replica tables of the single-launch kernels, which k_entropy_replicas and k_hist_replicas_fold consume and
// leave zero.  The contract: given the table qp[CNNQ_NQP][C], y is k_cl_qdq's, and the replica tables
// summed are, word for word, the histogram k_qdq<HIST> fills on the same values in NCHW order.
//
// Tiling: cnnq_nhwc.hip.h.  A lane keeps one piece of W consecutive channels for its whole slab, so its channels' scale, zero
// point and qmax - and its counts of the zero point's code - live in registers from the first row to the last.
#pragma once
#include "cnnq_nhwc.hip.h"

namespace {

// y = dequant(quant(x)) per channel with qdq1 (the IEEE divide) on the upconverted value, rounded once into the element type:
// the bits of k_cl_qdq in both of its branches (inside qdq_fast_domain the divide-free quotient is the divide's).  x read and y
// written non-temporally, workgroups in descending address order, as k_cl_qdq.
// The counting is k_qdq<HIST>'s own definitions (xhist_add, xhist_add_zp, xhist_fold in cnnq_qdq.hip.h): the table is nbins x
// HREP words of dynamic LDS, replica = lane & (HREP - 1); the zero point's code (about half of a post-ReLU layer) is counted in a register
// per channel of the lane's piece - the lane's channels never change, so W counters serve the whole slab - and added to the
// table once at the end; after the barrier one thread per bin folds the replicas and issues at most one global atomic, into
// replica table (workgroup id & (XHIST_REPLICAS - 1)).  A code indexes the table as code & (nbins - 1): the host passes
// nbins > qmax of every channel (2^num_bits where it derived the table from num_bits itself, 256 otherwise), so the mask only
// keeps a caller's mistaken nbins inside the table.  NaN takes k_qdq's path: its code is NaN, differs from the zero point, and
// (int)NaN == 0 counts it in bin 0; +inf clamps to qmax and -inf to 0 before the count.
// tests/test_channels_last_entropy_gpu.py compares the two histograms word for word.
// A workgroup's flush is up to nbins global atomics, so the launch takes the long slabs of cl_geo_hist, not cl_geo_qdq's.
template <class T, int W>
__global__ void __launch_bounds__(TPB) k_cl_qdq_hist(const typename ClRaw<T>::type* __restrict__ x, typename ClRaw<T>::type* __restrict__ y,
                                                     const ClGeo g, const float* __restrict__ qp, const int nbins,
                                                     unsigned long long* __restrict__ hist) {
    typedef typename ClRaw<T>::type E;
    extern __shared__ unsigned cnnq_dyn_lds[];       // nbins x HREP words, sized by the launch
    unsigned* sh_hist = cnnq_dyn_lds;
    const int tid = (int)threadIdx.x;
    const unsigned mask = (unsigned)nbins - 1u;
    for (int i = tid; i < nbins * HREP; i += TPB) sh_hist[i] = 0u;
    __syncthreads();
    const ClLane l = cl_lane(g, (int)gridDim.x - 1 - (int)blockIdx.x);
    if (l.piece >= 0) {                              // (an idle lane still meets the barrier and folds its bin)
        const int c0 = l.piece * W;
        float sc[W], zp[W], qm[W];
        unsigned nzp[W];
#pragma unroll
        for (int i = 0; i < W; ++i) {
            sc[i] = qp[(size_t)CNNQ_QP_SCALE * g.C + c0 + i];
            zp[i] = qp[(size_t)CNNQ_QP_ZP * g.C + c0 + i];
            qm[i] = qp[(size_t)CNNQ_QP_QMAX * g.C + c0 + i];
            nzp[i] = 0u;
        }
        const int64_t step = (int64_t)g.RS * g.C;
        int64_t off = l.r * g.C + c0;
        for (int64_t r = l.r; r < l.r1; r += g.RS, off += step) {
            E e[W];
            cl_ld<E, W, true>(x + off, e);
#pragma unroll
            for (int i = 0; i < W; ++i) {
                float cd;
                e[i] = cl_down(T{}, qdq1(cl_up(T{}, e[i]), sc[i], zp[i], qm[i], cd));
                xhist_add(sh_hist, cd, zp[i], nzp[i], mask);
            }
            cl_st_nt<E, W>(y + off, e);
        }
        xhist_add_zp<W>(sh_hist, zp, nzp, mask);
    }
    __syncthreads();
    if (tid < nbins) xhist_fold(sh_hist, hist, xhist_replica());
}

}  // namespace
