// cnnq_half.hip.h - bf16 / fp16 activations for configs 1 and 2: the exact per-channel min / max partials, the table-driven
// per-channel Q/DQ and the per-tensor GEMMLOWP Q/DQ on 2-byte elements.
// Part of the single translation unit cnnq_kernels.hip (see its header for the design).
//
// The contract: for x of dtype bf16 / fp16, y == fp32_path(x.float()).to(x.dtype), bit for bit.  Every
// element is upconverted exactly (bf16: the 16 bits shifted into the top of an fp32 word; fp16: v_cvt_f32_f16), so the extrema
// are the fp32 path's extrema; all arithmetic is the fp32 kernels' own (qdq1 / qdq2_fast, ptq1; the parameters are k_minmax_params'
// arithmetic, k_minmax_reduce and k_pt_setup on fp32 tables); the result is rounded to nearest-even into the input dtype by
// a plain conversion (v_cvt_pk_bf16_f32 / v_cvt_f16_f32), which keeps a NaN a NaN and turns an fp16 overflow into inf exactly as
// torch's .to() does.  These kernels are separate instances: no fp32 kernel changes.
//
// Tiling: a workgroup owns ONE channel and a range of samples (the rows x[n][c][0 .. HW) of that channel), so its parameters are
// uniform (scalar registers) and its extrema finish inside the workgroup.  A row is cut into pieces of W elements, W the widest
// of 8 / 4 / 2 / 1 that divides HW and both pointers' alignment: 16-byte pieces (W = 8) for every row length that is a multiple
// of 8 on a 16-byte aligned tensor, 8-byte pieces for 14x14 (HW = 196), 2-byte elements for 7x7 (49), odd lengths and views at an
// odd element offset.  The lanes walk the workgroup's (row, piece) pairs with a carry, no division in the loop.
//
// What the contiguous bf16 / fp16 family shares lives here (cnnq_half_stats.hip.h and cnnq_half_bcorr.hip.h hold their own
// arithmetic only): the piece load / store (piece_ld / piece_st_nt, the channels_last kernels' pair too), the partition of the
// grid (HGeo, HPart, h_part), the walk and the read-only piece loop (HWalk, h_pieces), the table row (h_qp), the workgroup folds
// (h_fold_mm, h_fold_sums) and the resident tile of the single-launch kernels (HTile).
#pragma once
#include "cnnq_common.hip.h"
#include "cnnq_qdq.hip.h"
#include "cnnq_pertensor.hip.h"

namespace {

struct HBf16 {};
struct HF16 {};

__device__ __forceinline__ float h_up(HBf16, uint16_t u) { return __uint_as_float((unsigned)u << 16); }
__device__ __forceinline__ float h_up(HF16, uint16_t u) { return (float)__builtin_bit_cast(_Float16, u); }
// the fp32 result is made opaque first: the conversion must round the fp32 VALUE (what .to(dtype) of the fp32 path rounds),
// never be folded into the arithmetic in front of it (a v_fma_mix / f16 operation would round once, from a wider result)
__device__ __forceinline__ uint16_t h_down(HBf16, float f) {
    asm("" : "+v"(f));
    return __builtin_bit_cast(uint16_t, (__bf16)f);
}
__device__ __forceinline__ uint16_t h_down(HF16, float f) {
    asm("" : "+v"(f));
    return __builtin_bit_cast(uint16_t, (_Float16)f);
}

// W consecutive elements of type E: one global load / store of W * sizeof(E) bytes, 16 at most (dwordx4) - the one pair every
// bf16 / fp16 and channels_last kernel loads and stores through
template <class E, int W, bool NT>
__device__ __forceinline__ void piece_ld(const E* __restrict__ p, E (&e)[W]) {
    if constexpr (W == 1) {
        e[0] = NT ? __builtin_nontemporal_load(p) : *p;
    } else {
        typedef E V __attribute__((ext_vector_type(W)));
        V v;
        if constexpr (NT) v = __builtin_nontemporal_load(reinterpret_cast<const V*>(p));
        else v = *reinterpret_cast<const V*>(p);
#pragma unroll
        for (int i = 0; i < W; ++i) e[i] = v[i];
    }
}
template <class E, int W>
__device__ __forceinline__ void piece_st_nt(E* __restrict__ p, const E (&e)[W]) {
    if constexpr (W == 1) {
        __builtin_nontemporal_store(e[0], p);
    } else {
        typedef E V __attribute__((ext_vector_type(W)));
        V v;
#pragma unroll
        for (int i = 0; i < W; ++i) v[i] = e[i];
        __builtin_nontemporal_store(v, reinterpret_cast<V*>(p));
    }
}
template <int W, bool NT>
__device__ __forceinline__ void h_ld(const uint16_t* __restrict__ p, uint16_t (&e)[W]) { piece_ld<uint16_t, W, NT>(p, e); }
template <int W>
__device__ __forceinline__ void h_st_nt(uint16_t* __restrict__ p, const uint16_t (&e)[W]) { piece_st_nt<uint16_t, W>(p, e); }

// the launch geometry of the row walk: grid = C * S * cs workgroups, workgroup b = s * C + c owns channel c and part s (h_part)
// (adjacent workgroups: adjacent rows in memory)
struct HGeo {
    int N, C, HW, S;
    int ppr;        // pieces per row, HW / W
    int cs;         // column splits per row (part s = batch split s / cs, pieces [p0, p1) of column part s % cs); 1: whole rows
};
inline HGeo h_geo(int64_t N, int64_t C, int64_t HW, int w, int S, int cs) {
    return HGeo{(int)N, (int)C, (int)HW, S, (int)(HW / w), cs};
}

// what the workgroup `bid` of a C * S * cs grid owns: channel c, part s = samples [n0, n1) of batch split s / cs and pw pieces
// from p0 of each of their rows; off: the element offset of its first piece.  COLS = false: the form for cs == 1 (whole rows),
// without the divisions
struct HPart {
    int c, s, rows, pw;
    size_t off;
};
template <int W, bool COLS = true>
__device__ __forceinline__ HPart h_part(const HGeo& g, int bid) {
    HPart t;
    t.c = bid % g.C;
    t.s = bid / g.C;
    int sn = t.s, p0 = 0;
    t.pw = g.ppr;
    if constexpr (COLS) {
        sn = t.s / g.cs;
        const int sp = t.s - sn * g.cs;
        p0 = (int)(((int64_t)sp * g.ppr) / g.cs);
        t.pw = (int)(((int64_t)(sp + 1) * g.ppr) / g.cs) - p0;
    }
    const int n0 = (int)(((int64_t)sn * g.N) / g.S), n1 = (int)(((int64_t)(sn + 1) * g.N) / g.S);
    t.rows = n1 - n0;
    t.off = (size_t)n0 * ((size_t)g.C * (size_t)g.HW) + (size_t)t.c * g.HW + (size_t)p0 * W;
    return t;
}

// (row, piece) of this lane's first pair and the per-step advance of the walk (TPB pairs per step)
struct HWalk {
    int r, p, dr, dp;
};
template <int NT = TPB>
__device__ __forceinline__ HWalk h_walk(int ppr) {
    HWalk w;
    w.r = (int)threadIdx.x / ppr;
    w.p = (int)threadIdx.x - w.r * ppr;
    w.dr = NT / ppr;
    w.dp = NT - w.dr * ppr;
    return w;
}
__device__ __forceinline__ void h_step(HWalk& w, int ppr) {
    w.r += w.dr;
    w.p += w.dp;
    if (w.p >= ppr) { w.p -= ppr; ++w.r; }
}

// The one piece loop of the read-only kernels: the lanes walk the (row, piece) pairs of part t, load each piece and hand it to
// f(e).  x points at the part (tensor + t.off).  U: the unroll count.  The trip count is a run-time one: no inline asm in f
// (cnnq_common.hip.h, hadd).  The two storing kernels (k_h_qdq, k_h_qdq_bias) keep their loop written out: through this
// template k_h_qdq_bias<T, 8> took 57 VGPRs for 37 and the two-pass correction measured 1-2 % slower.
template <int W, int U, class F>
__device__ __forceinline__ void h_pieces(const uint16_t* x, const HGeo& g, const HPart& t, F&& f) {
    const size_t P = (size_t)g.C * (size_t)g.HW;
    HWalk w = h_walk(t.pw);
#pragma unroll U
    for (; w.r < t.rows; h_step(w, t.pw)) {
        uint16_t e[W];
        h_ld<W, false>(x + (size_t)w.r * P + (size_t)w.p * W, e);
        f(e);
    }
}

// the row qp[CNNQ_NQP][C] holds for channel c
__device__ __forceinline__ void h_qp(const float* __restrict__ qp, int C, int c, float& sc, float& zp, float& qm) {
    sc = qp[(size_t)CNNQ_QP_SCALE * C + c];
    zp = qp[(size_t)CNNQ_QP_ZP * C + c];
    qm = qp[(size_t)CNNQ_QP_QMAX * C + c];
}

// The workgroup folds: the lanes' values -> the workgroup's, in every lane.  The fixed xor tree 32 ... 1 inside the wave, then
// the NW waves in wave order through LDS (the sums from 0.0): an order that follows from the launch alone.  One barrier; the LDS
// is the caller's and is not free again on return.
// Extrema: v_min / v_max drop a NaN, so a lane that saw one has poisoned its pair BEFORE the fold; pmin / pmax carry it on.
template <int NW>
__device__ __forceinline__ void h_fold_mm(float (&l_mn)[NW], float (&l_mx)[NW], float& mn, float& mx) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { mn = pmin(mn, shfl_xor_f(mn, m)); mx = pmax(mx, shfl_xor_f(mx, m)); }
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { l_mn[wv] = mn; l_mx[wv] = mx; }
    __syncthreads();
    mn = l_mn[0];
    mx = l_mx[0];
    for (int i = 1; i < NW; ++i) { mn = pmin(mn, l_mn[i]); mx = pmax(mx, l_mx[i]); }
}
// NV fp64 sums at once
template <int NW, int NV>
__device__ __forceinline__ void h_fold_sums(double (&l)[NV][NW], double (&v)[NV]) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
#pragma unroll
        for (int j = 0; j < NV; ++j) v[j] += shfl_xor_d(v[j], m);
    }
    const int wv = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int j = 0; j < NV; ++j) l[j][wv] = v[j];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < NV; ++j) v[j] = 0.;
    for (int i = 0; i < NW; ++i) {
#pragma unroll
        for (int j = 0; j < NV; ++j) v[j] += l[j][i];
    }
}

// scale / zero point / qmax of a channel from its exact extrema: k_minmax_params' arithmetic (iq.py:559-572), the same bits
__device__ __forceinline__ void h_params(float mn, float mx, int num_bits, int positive, float& sc, float& zp, float& qm) {
    const float offset = positive ? 0.f : mn;
    const float delta = mx - offset;
    qm = qmax_of(num_bits);
    sc = delta / qm;
    sc = (sc < 1e-8f) ? 1e-8f : sc;
    zp = zero_point_of(offset, sc);
}

// what the Q/DQ of config 2 derives its parameters from and where it publishes them
struct HArgs {
    int npairs, num_bits, positive;   // npairs: the {min, max} partials per channel in pmm
    float* qp;                        // out [CNNQ_NQP][C]
    float* mm;                        // out [2][C], may be null
};
__device__ __forceinline__ void h_publish(const HArgs& ha, int C, int c, float mn, float mx, float sc, float zp, float qm) {
    ha.qp[(size_t)CNNQ_QP_SCALE * C + c] = sc;
    ha.qp[(size_t)CNNQ_QP_ZP * C + c] = zp;
    ha.qp[(size_t)CNNQ_QP_QMAX * C + c] = qm;
    if (ha.mm) { ha.mm[c] = mn; ha.mm[C + c] = mx; }
}

// one piece through the Q/DQ: the divide-free quotient (fast, inside qdq_fast_domain) or the IEEE divide
template <class T, int W>
__device__ __forceinline__ void h_qdq_piece(uint16_t (&e)[W], bool fast, float sc, float rs, float zp, float qm) {
    if (fast) {
        if constexpr (W == 1) {
            float cd;
            e[0] = h_down(T{}, qdq1_fast(h_up(T{}, e[0]), sc, rs, zp, qm, cd));
        } else {
            const f2v s2 = {sc, sc}, r2 = {rs, rs}, z2 = {zp, zp};
#pragma unroll
            for (int i = 0; i < W; i += 2) {
                f2v cd;
                const f2v o = qdq2_fast(f2v{h_up(T{}, e[i]), h_up(T{}, e[i + 1])}, s2, r2, z2, qm, cd);
                e[i] = h_down(T{}, o.x);
                e[i + 1] = h_down(T{}, o.y);
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < W; ++i) {
            float cd;
            e[i] = h_down(T{}, qdq1(h_up(T{}, e[i]), sc, zp, qm, cd));
        }
    }
}

// exact per-channel {min, max} of one split -> pmm[s][2][C] (the layout k_minmax_params / k_minmax_reduce merge): plain stores,
// every entry written exactly once.  v_min / v_max drop a NaN: a lane that saw one poisons its result (torch.min / max propagate it)
template <class T, int W>
__device__ __forceinline__ void h_mm_piece(const uint16_t (&e)[W], float& mn, float& mx, bool& nan) {
#pragma unroll
    for (int i = 0; i < W; ++i) {
        const float v = h_up(T{}, e[i]);
        mn = fminf(mn, v);
        mx = fmaxf(mx, v);
        nan |= v != v;
    }
}
template <class T, int W>
__global__ void __launch_bounds__(TPB) k_h_minmax(const uint16_t* __restrict__ x, const HGeo g, float* __restrict__ pmm) {
    __shared__ float l_mn[TPB / 64], l_mx[TPB / 64];
    const HPart t = h_part<W>(g, (int)blockIdx.x);
    float mn = INFINITY, mx = -INFINITY;
    bool nan = false;
    h_pieces<W, 4>(x + t.off, g, t, [&](const uint16_t (&e)[W]) { h_mm_piece<T, W>(e, mn, mx, nan); });
    if (nan) { mn = NAN; mx = NAN; }
    h_fold_mm(l_mn, l_mx, mn, mx);
    if (threadIdx.x == 0) {
        pmm[(size_t)(2 * t.s) * g.C + t.c] = mn;
        pmm[(size_t)(2 * t.s + 1) * g.C + t.c] = mx;
    }
}

// y = dequant(quant(x)) per channel; x read and y written non-temporally, as k_qdq does.  Two sources of parameters:
//  * pmm == NULL: the table qp[CNNQ_NQP][C] (-sm use: a calibration table does not bound the channel's values), the IEEE divide
//    of k_qdq (qdq1);
//  * pmm = the statistics partials [npairs][2][C] of k_h_minmax (config 2, the chain): the workgroup merges its channel's pairs
//    in its prologue (npairs <= the fp32 plan's G: at most 65 on the ResNet-50 b512 set) and derives scale / zero point with
//    h_params (no parameter launch in between); the first split publishes them.  Inside qdq_fast_domain it runs the
//    divide-free quotient of the single-launch kernels (qdq2_fast, two elements per packed instruction; the bits of the IEEE
//    divide there, cnnq_qdq.hip.h), elsewhere qdq1.
// Workgroups are dispatched in descending address order: what the statistics pass read last is re-read first.
template <class T, int W>
__global__ void __launch_bounds__(TPB) k_h_qdq(const uint16_t* __restrict__ x, uint16_t* __restrict__ y, const HGeo g,
                                               const float* __restrict__ qp, const float* __restrict__ pmm, const HArgs ha) {
    const HPart t = h_part<W, false>(g, (int)gridDim.x - 1 - (int)blockIdx.x);
    const int c = t.c;
    float sc, zp, qm;
    bool fast = false;
    if (pmm) {
        float mn = INFINITY, mx = -INFINITY;
        for (int i = 0; i < ha.npairs; ++i) {
            mn = pmin(mn, pmm[(size_t)(2 * i) * g.C + c]);
            mx = pmax(mx, pmm[(size_t)(2 * i + 1) * g.C + c]);
        }
        h_params(mn, mx, ha.num_bits, ha.positive, sc, zp, qm);
        fast = qdq_fast_domain(mn, mx, sc);
        if (t.s == 0 && threadIdx.x == 0) h_publish(ha, g.C, c, mn, mx, sc, zp, qm);
    } else {
        h_qp(qp, g.C, c, sc, zp, qm);
    }
    const bool ufast = __builtin_amdgcn_readfirstlane((int)fast) != 0;
    const float rs = ufast ? uniform_f(1.0f / sc) : 0.f;
    const size_t P = (size_t)g.C * (size_t)g.HW;
    HWalk w = h_walk(g.ppr);
    for (; w.r < t.rows; h_step(w, g.ppr)) {
        const size_t off = t.off + (size_t)w.r * P + (size_t)w.p * W;
        uint16_t e[W];
        h_ld<W, true>(x + off, e);
        h_qdq_piece<T, W>(e, ufast, sc, rs, zp, qm);
        h_st_nt<W>(y + off, e);
    }
}

// Config 2 in ONE launch and ONE read of x (4 B/elem) for channels whose whole batch population fits one workgroup's registers:
// HTPB lanes, K pieces of W >= 2 elements each, kept as loaded - packed, two bf16 / fp16 per VGPR - i.e. the
// elements per workgroup of an fp32 tile of the same registers, doubled.  Extrema (workgroup reduction), parameters (h_params),
// Q/DQ out of the registers, store.  One workgroup per channel; no exchange, no workspace.  qp and mm are written.
constexpr int HTPB = 1024;

// The resident tile of the single-launch kernels: one channel's whole batch population in the registers of one HTPB-lane
// workgroup, K pieces of W >= 2 elements per lane, kept as loaded (packed).  Every phase walks the same (row, piece) pairs again
// from the lane's first pair: the K offsets are not kept (K more 64-bit registers).
template <int W, int K>
struct HTile {
    static_assert(W >= 2, "the resident tile keeps packed pieces");
    typedef uint16_t S __attribute__((ext_vector_type(W)));
    S t[K];
    HWalk w0;
    int N, ppr;
    size_t P;
    __device__ __forceinline__ explicit HTile(const HGeo& g)
        : w0(h_walk<HTPB>(g.ppr)), N(g.N), ppr(g.ppr), P((size_t)g.C * (size_t)g.HW) {}
    // f(k, the pair) for the pairs this lane holds; at(channel, pair): where the pair's piece lies
    template <class F>
    __device__ __forceinline__ void walk(HWalk w, F&& f) {
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if (w.r < N) f(k, w);
            h_step(w, ppr);
        }
    }
    template <class Q>
    __device__ __forceinline__ Q* at(Q* c, const HWalk& w) const { return c + (size_t)w.r * P + (size_t)w.p * W; }
    static __device__ __forceinline__ void unpack(const S& s, uint16_t (&e)[W]) {
#pragma unroll
        for (int i = 0; i < W; ++i) e[i] = (uint16_t)s[i];
    }
    // the non-temporal load of the tile from channel xc; f(e) on each piece as it arrives
    template <class F>
    __device__ __forceinline__ void load(const uint16_t* xc, F&& f) {
        walk(w0, [&](int k, const HWalk& w) {
            t[k] = __builtin_nontemporal_load(reinterpret_cast<const S*>(at(xc, w)));
            uint16_t e[W];
            unpack(t[k], e);
            f(e);
        });
    }
    __device__ __forceinline__ void load(const uint16_t* xc) {
        load(xc, [](const uint16_t (&)[W]) {});
    }
    // f(e) on each held piece
    template <class F>
    __device__ __forceinline__ void each(F&& f) {
        walk(w0, [&](int k, const HWalk&) {
            uint16_t e[W];
            unpack(t[k], e);
            f(e);
        });
    }
    // what f leaves of each held piece -> channel yc, non-temporally.  The walk starts from an opaque copy of the first pair, or
    // the compiler keeps the offsets of the phases before alive across the reduction in between.  OPAQUE: the piece too is
    // unpacked from an opaque copy (k_h_bcorr_whole says why).
    template <bool OPAQUE, class F>
    __device__ __forceinline__ void store(uint16_t* yc, F&& f) {
        HWalk w = w0;
        asm volatile("" : "+v"(w.r), "+v"(w.p));
        walk(w, [&](int k, const HWalk& wk) {
            uint16_t e[W];
            if constexpr (OPAQUE) {
                S tk = t[k];
                asm volatile("" : "+v"(tk));
                unpack(tk, e);
            } else {
                // element by element, not through unpack's reference: k_h_whole<HF16, 2, 64> spills 56 VGPRs that way
                // (profiles/half_shared.md lists the resident instances' registers, to compare after a compiler change)
#pragma unroll
                for (int i = 0; i < W; ++i) e[i] = (uint16_t)t[k][i];
            }
            f(e);
            S o;
#pragma unroll
            for (int i = 0; i < W; ++i) o[i] = e[i];
            __builtin_nontemporal_store(o, reinterpret_cast<S*>(at(yc, wk)));
        });
    }
};

template <class T, int W, int K>
__global__ void __launch_bounds__(HTPB) k_h_whole(const uint16_t* __restrict__ x, uint16_t* __restrict__ y, const HGeo g,
                                                  const HArgs ha) {
    __shared__ float l_mn[HTPB / 64], l_mx[HTPB / 64];
    const int c = (int)blockIdx.x;
    HTile<W, K> tile(g);
    float mn = INFINITY, mx = -INFINITY;
    bool nan = false;
    tile.load(x + (size_t)c * g.HW, [&](const uint16_t (&e)[W]) { h_mm_piece<T, W>(e, mn, mx, nan); });
    if (nan) { mn = NAN; mx = NAN; }
    h_fold_mm(l_mn, l_mx, mn, mx);
    float sc, zp, qm;
    h_params(mn, mx, ha.num_bits, ha.positive, sc, zp, qm);
    if (threadIdx.x == 0) h_publish(ha, g.C, c, mn, mx, sc, zp, qm);
    const bool ufast = __builtin_amdgcn_readfirstlane((int)qdq_fast_domain(mn, mx, sc)) != 0;
    const float rs = ufast ? uniform_f(1.0f / sc) : 0.f;
    tile.template store<false>(y + (size_t)c * g.HW, [&](uint16_t (&e)[W]) { h_qdq_piece<T, W>(e, ufast, sc, rs, zp, qm); });
}
// K of the resident tile for a piece width: 64 VGPRs of packed elements
// Not for W = 1 (2-byte elements, one per VGPR): measured slower than the two launches on the 7x7 layers of ResNet-50 b512
// (1.40 against 1.07 ms per step for the 9 layers) - one 1024-lane workgroup per CU that loads, reduces and stores in turn.
template <int W>
constexpr int h_whole_k() { return 128 / W; }
// the elements a k_h_whole workgroup holds at piece width w (0: no single launch)
inline int64_t h_whole_cap(int w) { return w >= 2 ? (int64_t)HTPB * 128 : 0; }
inline int h_whole_k_rt(int w) { return w >= 2 ? 128 / w : 0; }

// config 1's GEMMLOWP Q/DQ (k_pt_qdq) on 2-byte elements; the noise tensor stays fp32.  W = 8 for 16-byte aligned x, y (and
// noise), the n % 8 tail handled by the first lanes of the grid; W = 1 otherwise
template <class T, int W, bool NOISE>
__global__ void __launch_bounds__(TPB) k_h_pt_qdq(const uint16_t* __restrict__ x, uint16_t* __restrict__ y, int64_t n,
                                                  const float* __restrict__ ptp, const float* __restrict__ noise) {
    const float scale = ptp[0], shift = ptp[1], qmax = ptp[2];
    const bool etz = ptp[3] != 0.f, pass = ptp[4] != 0.f;
    const int64_t nv = n / W;
    const int64_t i = (int64_t)blockIdx.x * TPB + threadIdx.x;
    if (i < nv) {
        uint16_t e[W];
        float z[W];
        h_ld<W, true>(x + i * W, e);
        if constexpr (NOISE) {
            if constexpr (W == 8) {
                float a[4], b[4];
                ldv_nt<4>(noise + i * W, a);
                ldv_nt<4>(noise + i * W + 4, b);
#pragma unroll
                for (int k = 0; k < 4; ++k) { z[k] = a[k]; z[4 + k] = b[k]; }
            } else {
#pragma unroll
                for (int k = 0; k < W; ++k) z[k] = noise[i * W + k];
            }
        }
        if (!pass) {
#pragma unroll
            for (int k = 0; k < W; ++k) e[k] = h_down(T{}, ptq1(h_up(T{}, e[k]), scale, shift, qmax, etz, NOISE ? z[k] : 0.f));
        }
        h_st_nt<W>(y + i * W, e);
    }
    if constexpr (W > 1) {
        const int64_t t = nv * W + i;
        if (i < W && t < n) y[t] = pass ? x[t] : h_down(T{}, ptq1(h_up(T{}, x[t]), scale, shift, qmax, etz, NOISE ? noise[t] : 0.f));
    }
}

// ---- host side: the piece width and the splits
inline int h_piece(int64_t HW, uintptr_t a, uintptr_t b) {
    for (int w = 8; w > 1; w >>= 1)
        if (HW % w == 0 && (a % (2 * w)) == 0 && (b % (2 * w)) == 0) return w;
    return 1;
}
constexpr int64_t H_MM_ELEMS = 16384;   // elements per statistics workgroup (long enough to amortise the reduction)
constexpr int64_t H_QDQ_ELEMS = 8192;   // elements per Q/DQ workgroup (16 KB of x: many short workgroups, as k_qdq)
// S splits of the batch: ~`per` elements per workgroup, at most N, at most smax; the grid C * S below 2^31
inline int h_splits(int64_t N, int64_t C, int64_t HW, int64_t per, int64_t smax) {
    int64_t s = (N * HW + per - 1) / per;
    if (s > N) s = N;
    if (s > smax) s = smax;
    if (s < 1) s = 1;
    while (s > 1 && C * s >= ((int64_t)1 << 31)) --s;
    return (int)s;
}

}  // namespace
