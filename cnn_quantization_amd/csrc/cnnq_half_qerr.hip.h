// cnnq_half_qerr.hip.h - the per-channel clipping-error columns of `-c mix` (mse_* / cos_* of smpc.py:80-100; cnnq_qerr.hip.h is
// the fp32 form, cnnq_nhwc_qerr.hip.h the channels_last one) on contiguous bf16 / fp16 activations x[N][C][HW]: K candidate
// quantizations from ONE non-temporal read of x in its own dtype - 2 B/elem, no fp32 copy, no quantized tensor written.
// Part of the single translation unit cnnq_kernels.hip (see its header for the design).
//
// The contract (DESIGN.md section 31, section 30's carried over): the columns are those of the exactly upconverted x (h_up), each
// term one fp32 operation, q_k the fp32 value the table-driven half Q/DQ (k_h_qdq) computes with table k before it converts
// down; against fp64 sums of those terms within the project's tier (ii).  The records are k_qerr's row records
// rec[n * nb + p][QE_NV(K)][C] (fp64), p one of nb column parts of the row x[n][c][:], and k_qerr_fold<K> folds them unchanged.
//
// Tiling: the family's (cnnq_half.hip.h) - a workgroup owns ONE channel and a range of samples, or (short batches of long rows)
// one of nb column parts of their rows, so the 3 K parameters are uniform and the choice of the quotient needs no vote.  A
// record belongs to one sample (the cosine takes a root per (n, c) row), so a row's lanes meet at the row's end instead of
// running on across rows as h_pieces does: a SEGMENT of seg lanes - a power of two, 64 at most (h_qe_seg) -
// owns one row at a time, the workgroup's TPB / seg segments take TPB / seg rows per step.  A segment folds its QE_NV(K) sums
// with the fixed xor tree seg / 2 ... 1 and lane 0 stores the record entries: no LDS and no barrier (k_qerr pays one LDS fold
// and one barrier per sample).
//
// Sums: the W terms of a piece are added in fp32 - packed pairs, then the two halves, h_mom_piece's order - and the piece sums
// are accumulated in fp64, QE_NV(K) doubles per lane; a single element (W = 1) goes into fp64 as it is.  Nothing here cancels
// (every term but x q is a square, and q is x's own rounding), so the fp32 roundings of a piece sum, each 6e-8 relative, stay
// far inside the 2e-6 tier.  The order of every addition follows from (N, C, HW, the piece width) alone; no atomics; every
// record entry is stored once by one lane: run after run the same bits.
#pragma once
#include "cnnq_half.hip.h"
#include "cnnq_qerr.hip.h"

namespace {

// the QE_NV(K) sums of one piece into the lane's running sums
template <class T, int W, int K, bool FAST>
__device__ __forceinline__ void h_qe_piece(const uint16_t (&e)[W], const float (&sc)[K], const float (&rs)[K], const float (&zp)[K],
                                           const float (&qm)[K], double (&acc)[QE_NV(K)]) {
    if constexpr (W == 1) {
        const float v = h_up(T{}, e[0]);
        acc[0] += (double)(v * v);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            float cd;
            const float q = FAST ? qdq1_fast(v, sc[k], rs[k], zp[k], qm[k], cd) : qdq1(v, sc[k], zp[k], qm[k], cd);
            const float d = v - q;
            acc[1 + 3 * k] += (double)(d * d);
            acc[2 + 3 * k] += (double)(v * q);
            acc[3 + 3 * k] += (double)(q * q);
        }
    } else {
        f2v v[W / 2];
#pragma unroll
        for (int i = 0; i < W / 2; ++i) v[i] = f2v{h_up(T{}, e[2 * i]), h_up(T{}, e[2 * i + 1])};
        f2v xx = v[0] * v[0];
#pragma unroll
        for (int i = 1; i < W / 2; ++i) xx = xx + v[i] * v[i];
        acc[0] += (double)(xx.x + xx.y);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const f2v s2 = {sc[k], sc[k]}, r2 = {rs[k], rs[k]}, z2 = {zp[k], zp[k]};
            auto q_of = [&](const f2v a) {
                if constexpr (FAST) {
                    f2v cd;
                    return qdq2_fast(a, s2, r2, z2, qm[k], cd);
                } else {
                    float cd;
                    return f2v{qdq1(a.x, sc[k], zp[k], qm[k], cd), qdq1(a.y, sc[k], zp[k], qm[k], cd)};
                }
            };
            f2v q = q_of(v[0]), d = v[0] - q;
            f2v dd = d * d, xq = v[0] * q, qq = q * q;
#pragma unroll
            for (int i = 1; i < W / 2; ++i) {
                q = q_of(v[i]);
                d = v[i] - q;
                dd = dd + d * d;
                xq = xq + v[i] * q;
                qq = qq + q * q;
            }
            acc[1 + 3 * k] += (double)(dd.x + dd.y);
            acc[2 + 3 * k] += (double)(xq.x + xq.y);
            acc[3 + 3 * k] += (double)(qq.x + qq.y);
        }
    }
}

// g: HGeo with cs = nb column parts (grid C * S * nb, h_part); seg: lanes per row, a power of two <= 64.  x is read for the last
// time by a collect step: non-temporal loads.  MM: mm holds the channel extrema [2][C]; a workgroup whose channel satisfies
// qdq_fast_domain and has no NaN zero point / qmax for every candidate takes the divide-free quotient (the same function there),
// any other the IEEE divide - k_qerr's rule, uniform here without a vote.
template <class T, int W, int K, bool MM>
__global__ void __launch_bounds__(TPB) k_h_qerr(const uint16_t* __restrict__ x, const HGeo g, const int seg,
                                                const float* __restrict__ qp, const float* __restrict__ mm,
                                                double* __restrict__ rec) {
    constexpr int NV = QE_NV(K);
    const HPart t = h_part<W>(g, (int)blockIdx.x);
    const int sn = t.s / g.cs, sp = t.s - sn * g.cs;
    const int n0 = (int)(((int64_t)sn * g.N) / g.S);
    float sc[K], rs[K], zp[K], qm[K];
    bool fast = MM;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        h_qp(qp + (size_t)k * CNNQ_NQP * g.C, g.C, t.c, sc[k], zp[k], qm[k]);
        // a NaN zero point or qmax must keep qdq1's compare+select clamp (k_qerr, cnnq_qerr.hip.h)
        if constexpr (MM) fast = fast && qdq_fast_domain(mm[t.c], mm[g.C + t.c], sc[k]) && zp[k] == zp[k] && qm[k] == qm[k];
    }
    const bool ufast = MM && __builtin_amdgcn_readfirstlane((int)fast) != 0;
#pragma unroll
    for (int k = 0; k < K; ++k) rs[k] = ufast ? uniform_f(1.0f / sc[k]) : 0.f;
    const int lane = (int)threadIdx.x & (seg - 1), sg = (int)threadIdx.x >> (31 - __builtin_clz(seg)), nseg = TPB / seg;
    const size_t P = (size_t)g.C * (size_t)g.HW;
    auto walk = [&](auto FASTC) {
        constexpr bool FAST = decltype(FASTC)::value != 0;
        for (int r0 = 0; r0 < t.rows; r0 += nseg) {      // uniform: whole waves take part in the shuffles
            const int r = r0 + sg;
            double acc[NV];
#pragma unroll
            for (int vi = 0; vi < NV; ++vi) acc[vi] = 0.;
            if (r < t.rows) {
                const uint16_t* row = x + t.off + (size_t)r * P;
                for (int p = lane; p < t.pw; p += seg) {
                    uint16_t e[W];
                    h_ld<W, true>(row + (size_t)p * W, e);
                    h_qe_piece<T, W, K, FAST>(e, sc, rs, zp, qm, acc);
                }
            }
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
                if (m < seg) {
#pragma unroll
                    for (int vi = 0; vi < NV; ++vi) acc[vi] += shfl_xor_d(acc[vi], m);
                }
            }
            if (r < t.rows && lane == 0) {
                double* out = rec + ((size_t)(n0 + r) * g.cs + sp) * NV * g.C + t.c;
#pragma unroll
                for (int vi = 0; vi < NV; ++vi) out[(size_t)vi * g.C] = acc[vi];
            }
        }
    };
    if (ufast) walk(IntC<1>{});
    else walk(IntC<0>{});
}

// ---- host side: the plan
// Column parts of a row - a function of (N, C, HW) alone, not of the piece width, so that the record count is known before the
// alignment is: only where the N * C rows are fewer than H_QE_ROWS (a wave per row on every SIMD several times over) and parts of
// at least H_QE_PART elements (a whole wave of the widest pieces) remain.  Every part holds a piece at every width.
constexpr int64_t H_QE_ROWS = 4096, H_QE_PART = 512;
constexpr int64_t H_QE_ELEMS = 16384;           // elements per workgroup, about (32768 and 65536 measured slower on the small classes)
inline int h_qe_parts(int64_t N, int64_t C, int64_t HW) {
    const int64_t want = (H_QE_ROWS + N * C - 1) / (N * C), most = HW / H_QE_PART;
    const int64_t nb = want < most ? want : most;
    return (int)(nb < 1 ? 1 : nb);
}
// Lanes per row for piece width w: the power of two that leaves a lane about ppl pieces of a row part - 32 of 16 bytes, 8 of
// the narrower ones - at least four lanes where the row has the pieces, one wave at most.  Few lanes with many pieces each beat
// a whole wave per row (the fold of a row costs QE_NV(K) fp64 shuffles per halving, and a lane's pieces are independent loads in
// flight) as long as a load instruction of the segment still covers 64 contiguous bytes: kernel times on ResNet-50 b512, bf16,
// us (profiles/half_qerr.md): 256x56x56 (392 pieces of 8) 64 lanes 503, 32: 435, 16: 401, 8: 399; 512x28x28 (98) 16 lanes 262,
// 8: 234, 4: 222, 2: 300; 1024x14x14 (49 pieces of 4) 16 lanes 193, 8: 165, 4: 216; 2048x7x7 (49 single elements) 32 lanes 567,
// 16: 298, 8: 284-301, 4: 396.
inline int h_qe_seg(int64_t HW, int w, int nb) {
    const int64_t pw = (HW / w + nb - 1) / nb, ppl = env_int("CNNQ_H_QE_PPL", w == 8 ? 32 : 8);      // (development knob)
    int seg = 1;
    while (seg < 4 && seg < pw) seg <<= 1;
    while (seg < 64 && (int64_t)seg * ppl < pw) seg <<= 1;
    return seg;
}
// batch splits: whole steps of TPB / seg rows, about H_QE_ELEMS elements per workgroup; the grid C * S * nb below 2^31
inline int h_qe_splits(int64_t N, int64_t C, int64_t HW, int nb, int seg) {
    const int64_t rows_step = TPB / seg, elems_step = rows_step * ((HW + nb - 1) / nb);
    int64_t steps = env_int("CNNQ_H_QE_ELEMS", H_QE_ELEMS) / elems_step;                      // (development knob)
    if (steps < 1) steps = 1;
    int64_t s = (N + rows_step * steps - 1) / (rows_step * steps);
    const int64_t most = (((int64_t)1 << 31) - 1) / (C * nb);
    return (int)(s < most ? s : most);
}

// The classes of layer that stay on the upcast route (cnnq_pc_route_qerr_dt's "native" word), a function of N, C, HW and the dtype
// alone: rows of pieces narrower than 16 bytes (HW no multiple of 8) whose channels fill a workgroup, in tensors below 2^26
// elements.  There the whole `-ce` collect step did not beat the upcast route beyond the run's spread (its minimum above native's
// maximum): ResNet-50 b512, tools/bench_half_qerr.py, us per step, median (min-max), native against upcast: [512,512,14,14] bf16
// 488.6 (471.3-568.9) / 557.9 (540.6-576.9), fp16 483.8 (473.0-593.7) / 548.8 (540.8-567.9); [512,256,14,14] bf16 438.8
// (426.0-542.0) / 460.8 (453.0-487.1), fp16 425.4 (418.8-475.7) / 449.0 (440.8-471.0); [512,512,7,7], which h_stats_native keeps
// there already, likewise - about 180 us of every step is k_qerr_fold in either route.  [512,1024,14,14] (2^26.6 elements) won,
// 532.3 (528.0-585.9) / 757.9 (749.9-776.2); smaller populations were not measured and stay native.
inline int h_qerr_native(int64_t N, int64_t C, int64_t HW, int dtype) {
    (void)dtype;
    return !(HW % 8 != 0 && N * HW >= H_MM_ELEMS && N * C * HW < ((int64_t)1 << 26));
}

}  // namespace
