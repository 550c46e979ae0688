// cnnq_nhwc.hip.h - dense channels_last (NHWC) activations: the tiling, the two summation regimes and the LDS meeting that
// every channels_last kernel shares (cnnq_nhwc_aciq.hip.h and cnnq_nhwc_bcorr.hip.h hold the sum reductions built on them),
// and config 2 itself: exact per-channel min / max partials over slabs of rows and the
// per-channel Q/DQ, for fp32, bf16 and fp16 elements.
// Part of the single translation unit cnnq_kernels.hip (see its header for the design).
//
// The contract: for a dense channels_last x, y has x's layout and y.contiguous() equals, bit for bit, the
// NCHW path on x.contiguous().  Min / max do not depend on the order of the elements, and the Q/DQ works element by element, so
// this holds when the arithmetic is the NCHW path's own: the parameters come from k_minmax_params on the partials written here,
// the Q/DQ is qdq1 (IEEE divide) or, inside qdq_fast_domain, the divide-free quotient of the single-launch kernels (the same
// bits, cnnq_qdq.hip.h); bf16 / fp16 go through h_up / h_down of cnnq_half.hip.h.
//
// Tiling: the tensor is the matrix [R = N*H*W][C], C innermost.  A row is cut into P = C / W pieces of W consecutive channels
// (W the widest of 16 / 8 / 4 / 2 / 1 bytes that divides C and both pointers' alignment).  A workgroup owns a column block of
// CP = min(P, TPB) pieces and a slab of rows; lane t keeps piece t % CP for its whole life and walks rows t / CP, t / CP + RS,
// ... (RS = TPB / CP rows per step), so its channels never change: running extrema, running sums and Q/DQ parameters stay in
// registers.
//
// Sums: above CL_EXACT_ROWS rows, CL_FOLD rows are added in fp32 and folded into an fp64 accumulator; smaller tensors and a
// lane's leftover rows are added in fp64 element by element (why, and why there: at CL_EXACT_ROWS below).  The lanes that share
// a piece meet through LDS and are combined in ascending row order by one thread per channel (cl_fold_sums for the sums):
// an order fixed by ClGeo alone.
#pragma once
#include "cnnq_common.hip.h"
#include "cnnq_qdq.hip.h"
#include "cnnq_half.hip.h"

namespace {

struct CF32 {};     // fp32 elements (HBf16 / HF16: cnnq_half.hip.h)

template <class T>
struct ClRaw { typedef uint16_t type; };
template <>
struct ClRaw<CF32> { typedef float type; };

__device__ __forceinline__ float cl_up(CF32, float v) { return v; }
__device__ __forceinline__ float cl_up(HBf16 t, uint16_t u) { return h_up(t, u); }
__device__ __forceinline__ float cl_up(HF16 t, uint16_t u) { return h_up(t, u); }
__device__ __forceinline__ float cl_down(CF32, float v) { return v; }
__device__ __forceinline__ uint16_t cl_down(HBf16 t, float v) { return h_down(t, v); }
__device__ __forceinline__ uint16_t cl_down(HF16 t, float v) { return h_down(t, v); }

// W consecutive elements: one global load / store of W * sizeof(E) bytes (at most 16) - the pair of cnnq_half.hip.h
template <class E, int W, bool NT>
__device__ __forceinline__ void cl_ld(const E* __restrict__ p, E (&e)[W]) { piece_ld<E, W, NT>(p, e); }
template <class E, int W>
__device__ __forceinline__ void cl_st_nt(E* __restrict__ p, const E (&e)[W]) { piece_st_nt<E, W>(p, e); }

// the launch geometry: grid = S * nb workgroups, workgroup b' = s * nb + b owns column block b and rows [s * rpw, (s + 1) * rpw)
struct ClGeo {
    int64_t R;      // rows (N * H * W)
    int64_t rpw;    // rows per workgroup, a multiple of RS
    int C;          // channels (the row length)
    int P;          // pieces per row, C / W
    int CP;         // pieces per column block, min(P, TPB)
    int RS;         // rows per step, TPB / CP
    int nb;         // column blocks, ceil(P / CP)
    int S;          // row slabs
};

// this lane's piece (-1: idle) and first row of the workgroup's slab
struct ClLane {
    int piece;
    int64_t r, r1;
};
__device__ __forceinline__ ClLane cl_lane(const ClGeo& g, int bid) {
    const int s = bid / g.nb, b = bid - s * g.nb;
    const int t = (int)threadIdx.x;
    const int lr = t / g.CP, lp = t - lr * g.CP;
    ClLane l;
    l.piece = b * g.CP + lp;
    if (lr >= g.RS || l.piece >= g.P) l.piece = -1;
    l.r = (int64_t)s * g.rpw + lr;
    l.r1 = (int64_t)(s + 1) * g.rpw;
    if (l.r1 > g.R) l.r1 = g.R;
    return l;
}

// The two summation regimes of the sum reductions (k_cl_moments, k_cl_absdev, k_cl_bcorr_sums).  CL_FOLD rows are added in fp32 - (v0 + v1) + (v2 + v3), three roundings, each
// relative to a four-term sum, as Mom::add4 - and folded into an fp64 accumulator.  Those roundings are unbiased and average out
// over the R / 4 partial sums of a channel, but a channel's variance is the small difference sum x^2 - (sum x)^2 / R, which
// magnifies them by k = 1 + mean^2 / var.  So a tensor of at most CL_EXACT_ROWS rows (the elements per channel), and the rows a lane
// has left over, are added in fp64 element by element - exact sums of the fp32 values.  Derivation of the border: a four-term fp32
// partial sum of squares carries a relative rounding error of about e4 = 6e-8 (rms); over the R / 4 partials of a channel the
// relative error of sum x^2 is e4 / sqrt(R / 4), the variance magnifies it by k, and the std takes half of that.  Assumed
// conditioning: k <= 300 (|mean| <= 3.5 at std >= 0.2, the worst channel of the test generator over 2048 channels; real
// post-BN activations are far below).  R = 4096 then gives 300 * 6e-8 / 32 / 2 = 2.8e-7 (1 sigma) against the 2e-6 tier - seven
// sigma; R = 49 gives 2.6e-6, which is what was seen there (3e-6 on the two worst of 2048 channels).  Channels worse conditioned
// than k = 300 are the open item DESIGN.md section 14 names.  The fp64 path costs one v_add_f64 and one v_fma_f64 per element
// instead of half an fp64 operation; only tensors of at most 4096 * C elements take it, and its speed has not been measured.
constexpr int CL_FOLD = 4;           // rows per fp32 partial sum
static_assert(CL_FOLD == 4, "the fold bodies name their four rows");
constexpr int CL_EXACT_ROWS = 4096;

// The meeting of the lanes that share a piece, for fp64 sums: each stores its W values into the [RS][CP * W] LDS table, and one
// thread per column j (channel c of the tensor) adds the column's RS entries in ascending row order -> rec_row[c], a row of this
// slab's record; two barriers (the table is free again on return).  (The extrema meet the same way in k_cl_minmax, k_cl_moments.)
template <int W>
__device__ __forceinline__ void cl_fold_sums(double* __restrict__ l_d, const ClGeo& g, int b, const double (&v)[W],
                                             double* __restrict__ rec_row) {
    const int t = (int)threadIdx.x;
    if (t < g.RS * g.CP) {
#pragma unroll
        for (int i = 0; i < W; ++i) l_d[t * W + i] = v[i];
    }
    __syncthreads();
    const int cols = g.CP * W;
    for (int j = t; j < cols; j += TPB) {
        const int c = b * cols + j;
        if (c >= g.C) break;
        double a = l_d[j];
        for (int k = 1; k < g.RS; ++k) a += l_d[k * cols + j];
        rec_row[c] = a;
    }
    __syncthreads();
}

// exact per-channel {min, max} of slab s -> pmm[s][2][C] (the layout k_minmax_params / k_minmax_reduce merge): plain stores, every
// entry written exactly once, no atomics.  v_min / v_max drop a NaN: a lane that saw one poisons that channel's result (torch.min /
// max propagate it, as k_h_minmax does); pmin / pmax keep it through the reductions.
template <class T, int W>
__global__ void __launch_bounds__(TPB) k_cl_minmax(const typename ClRaw<T>::type* __restrict__ x, const ClGeo g,
                                                   float* __restrict__ pmm) {
    typedef typename ClRaw<T>::type E;
    __shared__ float l_mn[TPB * W], l_mx[TPB * W];
    const int bid = (int)blockIdx.x;
    const ClLane l = cl_lane(g, bid);
    float mn[W], mx[W];
#pragma unroll
    for (int i = 0; i < W; ++i) { mn[i] = INFINITY; mx[i] = -INFINITY; }
    unsigned nanm = 0;
    if (l.piece >= 0) {
        const E* p = x + l.r * g.C + (int64_t)l.piece * W;
        const int64_t step = (int64_t)g.RS * g.C;
#pragma unroll 4
        for (int64_t r = l.r; r < l.r1; r += g.RS, p += step) {
            E e[W];
            cl_ld<E, W, false>(p, e);
#pragma unroll
            for (int i = 0; i < W; ++i) {
                const float v = cl_up(T{}, e[i]);
                mn[i] = fminf(mn[i], v);
                mx[i] = fmaxf(mx[i], v);
                nanm |= (unsigned)(v != v) << i;
            }
        }
    }
    const int t = (int)threadIdx.x;
    if (t < g.RS * g.CP) {
#pragma unroll
        for (int i = 0; i < W; ++i) {
            const bool n = (nanm >> i) & 1u;
            l_mn[t * W + i] = n ? NAN : mn[i];
            l_mx[t * W + i] = n ? NAN : mx[i];
        }
    }
    __syncthreads();
    // the lanes that share a piece: column j of the [RS][CP * W] table, one thread per column
    const int s = bid / g.nb, b = bid - s * g.nb;
    const int cols = g.CP * W;
    for (int j = t; j < cols; j += TPB) {
        const int c = b * cols + j;
        if (c >= g.C) break;
        float a = l_mn[j], z = l_mx[j];
        for (int k = 1; k < g.RS; ++k) { a = pmin(a, l_mn[k * cols + j]); z = pmax(z, l_mx[k * cols + j]); }
        pmm[(size_t)(2 * s) * g.C + c] = a;
        pmm[(size_t)(2 * s + 1) * g.C + c] = z;
    }
}

// y = dequant(quant(x)) per channel, x read and y written non-temporally, as k_qdq does.  Each lane loads its piece's parameters
// once.  mm == NULL: the table qp alone (-sm use: a calibration table does not bound the channel's values), the IEEE divide of
// k_qdq (qdq1).  mm = the channels' exact extrema [2][C] (config 2): inside qdq_fast_domain the divide-free quotient of the
// single-launch kernels (qdq2_fast, two elements per packed instruction; the bits of the IEEE divide there), elsewhere qdq1.
// Workgroups are dispatched in descending address order: what the statistics pass read last is re-read first.
template <class T, int W>
__global__ void __launch_bounds__(TPB) k_cl_qdq(const typename ClRaw<T>::type* __restrict__ x, typename ClRaw<T>::type* __restrict__ y,
                                                const ClGeo g, const float* __restrict__ qp, const float* __restrict__ mm) {
    typedef typename ClRaw<T>::type E;
    const ClLane l = cl_lane(g, (int)gridDim.x - 1 - (int)blockIdx.x);
    if (l.piece < 0) return;
    const int c0 = l.piece * W;
    float sc[W], zp[W], qm[W], rs[W];
#pragma unroll
    for (int i = 0; i < W; ++i) {
        sc[i] = qp[(size_t)CNNQ_QP_SCALE * g.C + c0 + i];
        zp[i] = qp[(size_t)CNNQ_QP_ZP * g.C + c0 + i];
        qm[i] = qp[(size_t)CNNQ_QP_QMAX * g.C + c0 + i];
    }
    bool fast = mm != nullptr;
    if (fast) {
#pragma unroll
        for (int i = 0; i < W; ++i) fast = fast && qdq_fast_domain(mm[c0 + i], mm[g.C + c0 + i], sc[i]) && qm[i] == qm[0];
    }
#pragma unroll
    for (int i = 0; i < W; ++i) rs[i] = fast ? 1.0f / sc[i] : 0.f;
    const int64_t step = (int64_t)g.RS * g.C;
    int64_t off = l.r * g.C + c0;
    if (fast) {
        for (int64_t r = l.r; r < l.r1; r += g.RS, off += step) {
            E e[W];
            cl_ld<E, W, true>(x + off, e);
            if constexpr (W == 1) {
                float cd;
                e[0] = cl_down(T{}, qdq1_fast(cl_up(T{}, e[0]), sc[0], rs[0], zp[0], qm[0], cd));
            } else {
#pragma unroll
                for (int i = 0; i < W; i += 2) {
                    f2v cd;
                    const f2v o = qdq2_fast(f2v{cl_up(T{}, e[i]), cl_up(T{}, e[i + 1])}, f2v{sc[i], sc[i + 1]},
                                            f2v{rs[i], rs[i + 1]}, f2v{zp[i], zp[i + 1]}, qm[0], cd);
                    e[i] = cl_down(T{}, o.x);
                    e[i + 1] = cl_down(T{}, o.y);
                }
            }
            cl_st_nt<E, W>(y + off, e);
        }
    } else {
        for (int64_t r = l.r; r < l.r1; r += g.RS, off += step) {
            E e[W];
            cl_ld<E, W, true>(x + off, e);
#pragma unroll
            for (int i = 0; i < W; ++i) {
                float cd;
                e[i] = cl_down(T{}, qdq1(cl_up(T{}, e[i]), sc[i], zp[i], qm[i], cd));
            }
            cl_st_nt<E, W>(y + off, e);
        }
    }
}

// ---- host side: piece width, geometry, slabs
constexpr int64_t CL_MM_ELEMS = 65536;       // elements per statistics workgroup at least (amortises the LDS reduction)
constexpr int64_t CL_MM_MAX_WGS = 2048;      // statistics workgroups at most (8 per CU)
constexpr int64_t CL_PMM_MAX = (int64_t)1 << 19;   // S * C at most: the partials stay <= 4 MB
constexpr int64_t CL_QDQ_ELEMS = 8192;       // elements per Q/DQ workgroup (many short workgroups, as k_qdq)
constexpr int64_t CL_C_MAX = (int64_t)1 << 26;

inline int cl_esize(int dtype) { return dtype == CNNQ_DTYPE_F32 ? 4 : 2; }

// the widest piece of at most 16 bytes that divides C and the alignment (bytes) both pointers share
inline int cl_piece(int64_t C, int esize, int64_t align_bytes) {
    for (int w = 16 / esize; w > 1; w >>= 1)
        if (C % w == 0 && align_bytes % ((int64_t)w * esize) == 0) return w;
    return 1;
}

// geometry for piece width w with ~per elements per workgroup (at least `per`, a multiple of RS rows), at most smax slabs
inline ClGeo cl_geo(int64_t R, int64_t C, int w, int64_t per, int64_t max_wgs, int64_t smax) {
    ClGeo g;
    g.R = R;
    g.C = (int)C;
    g.P = (int)(C / w);
    g.CP = g.P < TPB ? g.P : TPB;
    g.RS = TPB / g.CP;
    g.nb = (g.P + g.CP - 1) / g.CP;
    const int64_t rstep = (R + g.RS - 1) / g.RS;                          // row steps of the whole tensor
    const int64_t blk = (int64_t)g.CP * w * g.RS;                         // elements per row step of one workgroup
    int64_t steps = (per + blk - 1) / blk;                                // row steps per workgroup
    int64_t s = (rstep + steps - 1) / steps;
    if (s * g.nb > max_wgs) s = (max_wgs + g.nb - 1) / g.nb;
    if (s > smax) s = smax;
    if (s < 1) s = 1;
    steps = (rstep + s - 1) / s;
    g.rpw = steps * g.RS;
    g.S = (int)((R + g.rpw - 1) / g.rpw);
    return g;
}
inline ClGeo cl_geo_mm(int64_t R, int64_t C, int w) {
    int64_t smax = CL_PMM_MAX / C;
    return cl_geo(R, C, w, CL_MM_ELEMS, CL_MM_MAX_WGS, smax < 1 ? 1 : smax);
}
inline ClGeo cl_geo_qdq(int64_t R, int64_t C, int w) {
    return cl_geo(R, C, w, CL_QDQ_ELEMS, ((int64_t)1 << 31) - 1, ((int64_t)1 << 31) - 1);
}
// The element-wise passes that count their codes (k_cl_mt_qdq<HIST>, k_cl_qdq_hist): every workgroup zeroes and folds an LDS table
// and flushes one global atomic per live bin - and k_cl_mt_qdq, for a tensor of up to TPB * W channels, hits the same 2 * C clamp
// counters - so they take 8 times CL_QDQ_ELEMS per workgroup, to keep the flush a small part of the workgroup's life.  The factor
// is a design guess (CL_MM_ELEMS of the statistics launches); tools/bench_channels_last_entropy.py sweeps it through the
// development knob CNNQ_CL_HIST_ELEMS (builds with -DCNNQ_DEV_KNOBS only, read per call; a workgroup's counts stay in 32 bits).
constexpr int CL_HIST_ELEMS = 65536;
inline ClGeo cl_geo_hist(int64_t R, int64_t C, int w) {
    int64_t per = env_int("CNNQ_CL_HIST_ELEMS", CL_HIST_ELEMS);
    per = per < 1 ? 1 : per > ((int64_t)1 << 30) ? ((int64_t)1 << 30) : per;
    return cl_geo(R, C, w, per, ((int64_t)1 << 31) - 1, ((int64_t)1 << 31) - 1);
}

// runtime (element type, piece width) -> template arguments: f(Piece<T, W>) with T = CF32 (W = 4 / 2 / 1), HBf16 or HF16
// (W = 8 / 4 / 2 / 1).  F32 = false: the bf16 / fp16 kernels of cnnq_half.hip.h, which have no fp32 instance.  A width a kernel
// lacks stays an `if constexpr` at its launch site.
template <class T_, int W_>
struct Piece { using T = T_; static constexpr int W = W_; };
template <class T, int WMAX, class F>
inline void with_width(int w, F&& f) {
    if constexpr (WMAX > 1) {
        if (w == WMAX) f(Piece<T, WMAX>{});
        else with_width<T, WMAX / 2>(w, f);
    } else {
        f(Piece<T, 1>{});
    }
}
template <bool F32 = true, class F>
inline void with_piece(int dt, int w, F&& f) {
    if constexpr (F32) {
        if (dt == CNNQ_DTYPE_F32) return with_width<CF32, 4>(w, f);
    }
    if (dt == CNNQ_DTYPE_BF16) with_width<HBf16, 8>(w, f);
    else with_width<HF16, 8>(w, f);
}

}  // namespace
