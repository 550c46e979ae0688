// cnnq_half_bcorr.hip.h - activation bias correction (iqm.py:180-196) folded into the table-driven Q/DQ on CONTIGUOUS bf16 / fp16
// activations x[N][C][HW] (-sm use ... -bca): the per-channel sums of the correction, the fused quantize + correct pass, and both
// in one launch for channels whose batch population fits one workgroup's registers - read where the tensor lies, no fp32 copy.
// Part of the single translation unit cnnq_kernels.hip (see its header for the design).
//
// The fp32 pair is k_bcorr_sums<FROMX> / k_qdq_bias (cnnq_corrections.hip.h), the channels_last pair k_cl_bcorr_sums /
// k_cl_qdq_bias (cnnq_nhwc_bcorr.hip.h); k_bcorr_bias between the two passes is that chain's own, on the records written here.
// The contract: the sums against fp64 within the statistics tier (the count exact), and given the sums
// every output bit for bit - bias is k_bcorr_bias' arithmetic (bcorr_bias_of), y is k_qdq_bias' expression on the exactly
// upconverted values with one round-to-nearest-even into the element type at the end (h_down).
//
// The partition (h_part: batch splits S, column splits cs), the piece loop (h_pieces), the table row (h_qp), the fold of the sums
// (h_fold_sums) and the resident tile (HTile) are the family's shared ones in cnnq_half.hip.h; this header holds the arithmetic
// of the correction and its routes.  A workgroup owns ONE channel, so scale / zero point / qmax / bias are uniform.  Sums: the W
// values of one piece are added in fp32 - pairs, then the two halves, h_mom_piece's order - and the piece sums are accumulated in
// fp64; a single element (W = 1) goes into fp64 as it is.  The order of every addition follows from HGeo alone: the xor tree
// inside the wave, the waves in order through LDS, every record entry stored once by one lane - no atomics, run after run the
// same bits.
#pragma once
#include "cnnq_half_stats.hip.h"
#include "cnnq_corrections.hip.h"

namespace {

// one element: q = qdq1(x) from the table (the IEEE divide: a calibration table does not bound the values; the fp32 value, not
// the one rounded to the element type), v = x' = relu(x) when the layer feeds a ReLU, count(x' > 0)
template <class T>
__device__ __forceinline__ void h_bc_elem(const uint16_t e, const bool relu, const float sc, const float zp, const float qm, float& v,
                                          float& q, unsigned& cn) {
    float cd;
    v = h_up(T{}, e);
    q = qdq1(v, sc, zp, qm, cd);
    if (relu) v = fmaxf(v, 0.f);
    cn += (v > 0.f) ? 1u : 0u;
}
// one piece into a lane's running sums.  No inline asm here: the loops around it have a run-time trip count and are unrolled
// (cnnq_common.hip.h, hadd).
template <class T, int W>
__device__ __forceinline__ void h_bc_piece(const uint16_t (&e)[W], const bool relu, const float sc, const float zp, const float qm,
                                           double& sx, double& sq, unsigned& cn) {
    typedef float f2 __attribute__((ext_vector_type(2)));
    if constexpr (W == 1) {
        float v, q;
        h_bc_elem<T>(e[0], relu, sc, zp, qm, v, q, cn);
        sx += (double)v;
        sq += (double)q;
    } else {
        float v0, v1, q0, q1;
        h_bc_elem<T>(e[0], relu, sc, zp, qm, v0, q0, cn);
        h_bc_elem<T>(e[1], relu, sc, zp, qm, v1, q1, cn);
        f2 px = {v0, v1}, pq = {q0, q1};
#pragma unroll
        for (int i = 2; i < W; i += 2) {
            h_bc_elem<T>(e[i], relu, sc, zp, qm, v0, q0, cn);
            h_bc_elem<T>(e[i + 1], relu, sc, zp, qm, v1, q1, cn);
            px = px + f2{v0, v1};
            pq = pq + f2{q0, q1};
        }
        sx += (double)(px.x + px.y);
        sq += (double)(pq.x + pq.y);
    }
}

// pass 1, read-only: record s of channel c -> part3[s][3][C] = {sum x', sum q, count(x' > 0)}, the arithmetic of
// k_bcorr_sums<FROMX> and k_cl_bcorr_sums.  Workgroups ascend; the second pass descends and re-reads first what was read last.
// The count is an integer below 2^53: exact in fp64 whatever the order of the fold.
template <class T, int W>
__global__ void __launch_bounds__(TPB) k_h_bcorr_sums(const uint16_t* __restrict__ x, const HGeo g, const int relu_first,
                                                      const float* __restrict__ qp, double* __restrict__ part3) {
    __shared__ double l_v[3][TPB / 64];
    const HPart t = h_part<W>(g, (int)blockIdx.x);
    float sc, zp, qm;
    h_qp(qp, g.C, t.c, sc, zp, qm);
    const bool relu = relu_first != 0;
    double sx = 0., sq = 0.;
    unsigned cn = 0u;          // exact: a lane reads fewer than 2^32 elements (at most H_ST_MAX_RECORDS-th of a channel)
    h_pieces<W, 2>(x + t.off, g, t, [&](const uint16_t (&e)[W]) { h_bc_piece<T, W>(e, relu, sc, zp, qm, sx, sq, cn); });
    double v[3] = {sx, sq, (double)cn};
    h_fold_sums(l_v, v);
    if (threadIdx.x == 0) {
        double* p = part3 + (size_t)t.s * 3 * g.C + t.c;
        p[0] = v[0];
        p[(size_t)g.C] = v[1];
        p[(size_t)2 * g.C] = v[2];
    }
}

// one piece through quantize + correct: k_qdq_bias' expression, rounded once into the element type
template <class T, int W>
__device__ __forceinline__ void h_qdq_bias_piece(uint16_t (&e)[W], const float sc, const float zp, const float qm, const float qb) {
#pragma unroll
    for (int i = 0; i < W; ++i) {
        float cd;
        const float q = qdq1(h_up(T{}, e[i]), sc, zp, qm, cd);
        e[i] = h_down(T{}, q + ((q > 0.f) ? 1.f : 0.f) * qb);
    }
}

// pass 2: y = q + (q > 0) * bias[c] with q = qdq1(x); k_h_qdq's geometry, descending dispatch, non-temporal load and store
template <class T, int W>
__global__ void __launch_bounds__(TPB) k_h_qdq_bias(const uint16_t* __restrict__ x, uint16_t* __restrict__ y, const HGeo g,
                                                    const float* __restrict__ qp, const float* __restrict__ bias) {
    const HPart t = h_part<W, false>(g, (int)gridDim.x - 1 - (int)blockIdx.x);
    float sc, zp, qm;
    h_qp(qp, g.C, t.c, sc, zp, qm);
    const float qb = bias[t.c];
    const size_t P = (size_t)g.C * (size_t)g.HW;
    HWalk w = h_walk(g.ppr);
    for (; w.r < t.rows; h_step(w, g.ppr)) {
        const size_t off = t.off + (size_t)w.r * P + (size_t)w.p * W;
        uint16_t e[W];
        h_ld<W, true>(x + off, e);
        h_qdq_bias_piece<T, W>(e, sc, zp, qm, qb);
        h_st_nt<W>(y + off, e);
    }
}

// Both passes in ONE launch and ONE read of x (4 B/elem) for channels whose whole batch population fits one workgroup's
// registers, on k_h_whole's resident tile (HTile): the three sums out of the registers (the piece arithmetic above, the same
// fold: the xor tree, then the 16 waves in order), the bias in every lane (bcorr_bias_of), quantize + correct out of the
// registers, store.  One workgroup per channel; no exchange, no workspace.  Lane 0 publishes sums[3][C] (may be null) and bias[c].
template <class T, int W, int K>
__global__ void __launch_bounds__(HTPB) k_h_bcorr_whole(const uint16_t* __restrict__ x, uint16_t* __restrict__ y, const HGeo g,
                                                        const int relu_first, const float* __restrict__ qp,
                                                        double* __restrict__ sums, float* __restrict__ bias) {
    __shared__ double l_v[3][HTPB / 64];
    const int c = (int)blockIdx.x;
    float sc, zp, qm;
    h_qp(qp, g.C, c, sc, zp, qm);
    const bool relu = relu_first != 0;
    HTile<W, K> tile(g);
    tile.load(x + (size_t)c * g.HW);
    double sx = 0., sq = 0.;
    unsigned cn = 0u;
    tile.each([&](const uint16_t (&e)[W]) { h_bc_piece<T, W>(e, relu, sc, zp, qm, sx, sq, cn); });
    double v[3] = {sx, sq, (double)cn};
    h_fold_sums(l_v, v);
    const float qb = bcorr_bias_of(v[0], v[1], v[2]);
    if (threadIdx.x == 0) {
        if (sums) { sums[c] = v[0]; sums[(size_t)g.C + c] = v[1]; sums[(size_t)2 * g.C + c] = v[2]; }
        bias[c] = qb;
    }
    // the upconversions again, from an opaque copy of each piece: or the compiler keeps the 128 fp32 values of the sums phase
    // alive across the fold
    tile.template store<true>(y + (size_t)c * g.HW, [&](uint16_t (&e)[W]) { h_qdq_bias_piece<T, W>(e, sc, zp, qm, qb); });
}

// ---- host side: which classes of layer run where (cnnq_pc_route_qdq_bcorr_dt's route word), functions of N, C, HW and the dtype
// alone.  The yardsticks are the routes of the same run (tools/bench_half_bcorr.py: MI355X, us per call, mean (min-max), 20 steps
// after 3); a class changes route only where it wins beyond that spread.  profiles/half_bcorr.md has every figure.
inline bool h_bcorr_whole_fits(int64_t N, int64_t HW, int w) { return N * HW <= h_whole_cap(w); }
// The single launch puts one 1024-lane workgroup on a CU, which loads, reduces and stores in turn: C workgroups run in rounds of
// 256, and a partly filled round costs a whole one.  Against the two passes it won in every measurement only on exactly one full
// round, C = 256, with a population of at least 32768 per channel: [512,256,14,14] bf16 54.5 (52.0-56.4) against 65.2 (61.1-70.9),
// fp16 55.1 (53.3-59.3) against 68.0 (64.4-88.8); [128,256,28,28], [32,256,56,56], [256,256,14,14], [64,256,28,28] and
// [512,256,8,8] likewise in both dtypes (23-52 us against 29-67).  It did not at C = 512 ([512,512,14,14] bf16 100.8 (97.3-107.0)
// against 108.2 (104.8-115.6)) or C = 1024 (191.7 (185.8-200.5) against 197.3 (192.0-216.4)), won in about half of the
// measurements at C = 192 and 512, lost at C <= 64 and C = 320 with a full population (49 against 26 us at C = 32, 95 against 79 at
// C = 320), and below a population of 32768 the two routes are within each other's spread.
inline int h_bcorr_whole_wins(int64_t N, int64_t C, int64_t HW, int dtype) {
    (void)dtype;
    return C == 256 && N * HW >= 32768;
}
// Against the upcast route the two passes won beyond the spread on all 12 classes of ResNet-50 b512 conv outputs in both dtypes,
// from 0.35 x ([512,256,56,56] bf16 604.5 (590.9-646.0) against 1718.0 (1704.9-1736.1)) to 0.90 x ([512,2048,7,7] bf16 210.8
// (206.6-216.2) against 234.5 (232.0-237.5); [512,512,7,7] 71.9 (70.4-75.8) against 85.9 (83.7-89.1)): no class is sent back.
inline int h_bcorr_native(int64_t N, int64_t C, int64_t HW, int dtype) {
    (void)N; (void)C; (void)HW; (void)dtype;
    return 1;
}

}  // namespace
