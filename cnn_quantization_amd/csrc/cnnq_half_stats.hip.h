// cnnq_half_stats.hip.h - `-sm collect` on contiguous bf16 / fp16 activations: the two per-channel reductions over x[N][C][HW]
// that fill the seven rows of the calibration table (smpc.py:45-79), read where the tensor lies - two reads of x, 4 B/elem, no
// fp32 copy.  Part of the single translation unit cnnq_kernels.hip (see its header for the design).
//
// The partition (h_part), the piece loop (h_pieces) and the workgroup folds (h_fold_mm, h_fold_sums) are the family's shared
// ones in cnnq_half.hip.h; this header holds the arithmetic of the two passes and their plan.
//
// Tiling: a workgroup owns ONE channel and a range of samples, or - short batches - a range of the pieces of its rows
// (k_h_minmax's column splits); workgroup b = s * C + c, s = batch split * cs + column part.  Every element is upconverted
// exactly (h_up), so the extrema are the fp32 path's extrema on x.float().
//
// Sums: the W values of one piece are added in fp32 - packed pairs, then the two halves, the order of
// Mom::add8 / add4p - and the piece sums are accumulated in fp64; a single element (W = 1) goes into fp64 as it is.  Pass B forms
// d = x - mean in fp32 and adds |d| and (d * (1 / std))^4 into fp64 element by element, k_absdev's arithmetic.  The records are
// k_moments' / k_absdev's, merged by k_combine(has_relu) / k_combine_dev(want_kurt) with G = S * cs.  The order of every addition
// follows from HGeo alone: the xor tree inside the wave, the four waves in order through LDS, every record entry stored once by
// one lane - no atomics, run after run the same bits.
#pragma once
#include "cnnq_half.hip.h"
#include "cnnq_stats.hip.h"

namespace {

// one piece into the running record.  fminf / fmaxf drop a NaN; the sum of squares keeps it (squares do not cancel, inf * inf is
// inf), so a lane whose sum of squares came out NaN saw one and poisons its pair afterwards - k_h_minmax's rule, k_moments' test.
// No inline asm here: the loop around it has a run-time trip count and is unrolled (cnnq_common.hip.h, hadd).
template <class T, int W, bool RELU>
__device__ __forceinline__ void h_mom_piece(Mom& m, const uint16_t (&e)[W]) {
    typedef float f2 __attribute__((ext_vector_type(2)));
    float v[W];
#pragma unroll
    for (int i = 0; i < W; ++i) {
        v[i] = h_up(T{}, e[i]);
        m.mn = fminf(m.mn, v[i]);
        m.mx = fmaxf(m.mx, v[i]);
    }
    if constexpr (W == 1) {
        const double d = (double)v[0];
        m.s += d;
        m.ss = fma(d, d, m.ss);
        if constexpr (RELU) {
            const double r = (double)fmaxf(v[0], 0.f);
            m.rs += r;
            m.rss = fma(r, r, m.rss);
        }
    } else {
        f2 ps = {v[0], v[1]};
        f2 pq = ps * ps;
#pragma unroll
        for (int i = 2; i < W; i += 2) {
            const f2 a = {v[i], v[i + 1]};
            ps = ps + a;
            pq = pq + a * a;
        }
        m.s += (double)(ps.x + ps.y);
        m.ss += (double)(pq.x + pq.y);
        if constexpr (RELU) {
            f2 pr = {fmaxf(v[0], 0.f), fmaxf(v[1], 0.f)};
            f2 pp = pr * pr;
#pragma unroll
            for (int i = 2; i < W; i += 2) {
                const f2 a = {fmaxf(v[i], 0.f), fmaxf(v[i + 1], 0.f)};
                pr = pr + a;
                pp = pp + a * a;
            }
            m.rs += (double)(pr.x + pr.y);
            m.rss += (double)(pp.x + pp.y);
        }
    }
}

// pass A: record s of channel c -> part[s][CNNQ_NMOM][C]; the count is the exact number of elements the workgroup read.  The
// lanes' records meet in the shared folds (h_fold_mm, h_fold_sums): Mom::wave_reduce / merge in the same order, addition by addition
template <class T, int W, bool RELU>
__global__ void __launch_bounds__(TPB) k_h_moments(const uint16_t* __restrict__ x, const HGeo g, double* __restrict__ part) {
    constexpr int NV = RELU ? 4 : 2;
    __shared__ float l_mn[TPB / 64], l_mx[TPB / 64];
    __shared__ double l_v[NV][TPB / 64];
    const HPart t = h_part<W>(g, (int)blockIdx.x);
    Mom m;
    m.init();
    h_pieces<W, 4>(x + t.off, g, t, [&](const uint16_t (&e)[W]) { h_mom_piece<T, W, RELU>(m, e); });
    if (m.ss != m.ss) { m.mn = NAN; m.mx = NAN; }
    h_fold_mm(l_mn, l_mx, m.mn, m.mx);
    double v[NV] = {m.s, m.ss};
    if constexpr (RELU) { v[2] = m.rs; v[3] = m.rss; }
    h_fold_sums(l_v, v);
    if (threadIdx.x == 0) {
        m.s = v[0]; m.ss = v[1];
        if constexpr (RELU) { m.rs = v[2]; m.rss = v[3]; }
        write_mom<RELU>(part, t.s, g.C, t.c, m, (double)t.rows * (double)t.pw * W);
    }
}

// pass B: record s of channel c -> part2[s][CNNQ_NDEV][C], with the mean and the standard deviation of rows CNNQ_STAT_MEAN / _STD
// of the table pass A's merge wrote.  Per element k_absdev's arithmetic: the fp32 subtract, |d| into fp64, z = d * (1 / std) with
// the fp32 reciprocal formed once per workgroup, z^4 = (z * z)^2 into fp64; the two elements of a pair keep a running sum each.
// A constant channel (std == 0) gives 0 * inf: its kurtosis is NaN, as in the fp32 chain.  Workgroups take the tensor in
// descending address order: what pass A read last is re-read first.
template <class T, int W, bool KURT>
__global__ void __launch_bounds__(TPB) k_h_absdev(const uint16_t* __restrict__ x, const HGeo g, const float* __restrict__ stats,
                                                  double* __restrict__ part2) {
    typedef float f2 __attribute__((ext_vector_type(2)));
    constexpr int NV = KURT ? 2 : 1;
    __shared__ double l_v[NV][TPB / 64];
    const HPart t = h_part<W>(g, (int)gridDim.x - 1 - (int)blockIdx.x);
    const float mean = stats[(size_t)CNNQ_STAT_MEAN * g.C + t.c];
    const float sd = KURT ? 1.f / stats[(size_t)CNNQ_STAT_STD * g.C + t.c] : 0.f;
    double sa0 = 0., sa1 = 0., sk0 = 0., sk1 = 0.;
    h_pieces<W, 4>(x + t.off, g, t, [&](const uint16_t (&e)[W]) {
        if constexpr (W == 1) {
            const float d = h_up(T{}, e[0]) - mean;
            sa0 += (double)fabsf(d);
            if constexpr (KURT) {
                const float z = d * sd;
                const float z2 = z * z;
                sk0 += (double)(z2 * z2);
            }
        } else {
            const f2 m2 = {mean, mean}, s2 = {sd, sd};
#pragma unroll
            for (int i = 0; i < W; i += 2) {
                const f2 d = f2{h_up(T{}, e[i]), h_up(T{}, e[i + 1])} - m2;
                sa0 += (double)fabsf(d.x);
                sa1 += (double)fabsf(d.y);
                if constexpr (KURT) {
                    const f2 z = d * s2;
                    const f2 z2 = z * z;
                    const f2 z4 = z2 * z2;
                    sk0 += (double)z4.x;
                    sk1 += (double)z4.y;
                }
            }
        }
    });
    double v[NV] = {sa0 + sa1};
    if constexpr (KURT) v[1] = sk0 + sk1;
    h_fold_sums(l_v, v);
    if (threadIdx.x == 0) {
        double* p = part2 + (size_t)t.s * CNNQ_NDEV * g.C + t.c;
        p[(size_t)CNNQ_DEV_ABS * g.C] = v[0];
        p[(size_t)CNNQ_DEV_Z4 * g.C] = KURT ? v[NV - 1] : 0.;
    }
}

// ---- host side: the splits.  k_h_minmax's rule - ~H_MM_ELEMS elements per workgroup, batch splits first, then (short batches)
// column splits of the rows - with two differences: the records per channel are capped by H_ST_MAX_RECORDS (the merge kernels
// read them all; beyond it a workgroup reads more), and a row is cut into at most HW / 8 parts whatever the piece width, so the
// plan - and with it the workspace - is a function of (N, C, HW) alone and every part holds a piece at every width.  (Fewer
// elements per workgroup where the rows load narrow pieces were measured and lost: 4096 and 2048 instead of 16384 on the 7x7 and
// 14x14 layers of ResNet-50 b512 took 17-44 % longer on [512,2048,7,7] and 15 % longer on [512,1024,14,14].)
constexpr int64_t H_ST_MAX_RECORDS = 2048;
inline void h_stats_splits(int64_t N, int64_t C, int64_t HW, int* S, int* cs) {
    const int total = h_splits(N * HW, C, 1, H_MM_ELEMS, H_ST_MAX_RECORDS);
    *S = total < N ? total : (int)N;
    const int64_t cmax = HW / 8 > 1 ? HW / 8 : 1;
    *cs = total / *S < cmax ? total / *S : (int)cmax;
}

// The classes of layer that stay on the upcast route (cnnq_pc_route_stats_dt's "native" word), a function of N, C, HW and the
// dtype alone.  An odd HW loads single 2-byte elements whatever the alignment, and where a channel's population fills a whole
// workgroup that walk only draws level with the upcast: ResNet-50 b512, tools/bench_half_collect.py, us per call, mean
// (min-max), native against former: [512,2048,7,7] bf16 126.3 (124.4-128.0) / 130.9 (129.8-132.5), fp16 126.2 (124.1-130.3) /
// 130.4 (128.6-133.8); [512,512,7,7] bf16 57.9 (56.7-61.0) / 60.0 (59.0-62.6), fp16 58.1 (55.0-63.3) / 60.3 (59.4-62.9) - not won
// beyond the spread.  (Walking such rows in pairs on the aligned 4-byte words, and 4096 or 2048 elements per workgroup, were
// measured too: 134 / 61 us, and 148-182 / 56-66 us.)  Smaller populations of odd rows were not measured and stay native.
inline int h_stats_native(int64_t N, int64_t C, int64_t HW, int dtype) {
    (void)C; (void)dtype;
    return !(HW % 2 == 1 && N * HW >= H_MM_ELEMS);
}

}  // namespace
