// cnnq_half_packed.hip.h - integer codes as the STORED format of a contiguous bf16 / fp16 NCHW activation:
// per-channel widths of 0..8 bits, on the storage as it is - 2 B read + b / 8 B written per element, no fp32 copy.
// Part of the single translation unit cnnq_kernels.hip (see its header for the design).
//
// Format: the NCHW stream of include/cnnq_hip.h (cnnq_pc_packed_layout, k_packed_layout), unchanged - row (n, c) holds H*W codes of
// b = bits[c] bits, a little-endian bit stream padded with zero bits to whole dwords, at byte n * rowoff[C] + rowoff[c].  A buffer
// packed here is byte for byte what cnnq_pc_quantize_packed writes for x.float(); either decoder reads either buffer.
//
// The stored code is qdq1's `code` of the exactly up-converted element (with the channel's exact extrema, inside qdq_fast_domain,
// the divide-free quotient's: the same bits), masked to b bits.  A NaN code is stored as 0: k_packed converts the code with
// v_cvt_u32_f32, which turns a NaN into 0; here that is a test, not what a conversion happens to give.
//
// k_h_pack, the store direction.  In 2-byte elements a 16-byte load is 8 codes = b whole bytes of the stream, so 64 pieces of W
// elements are 2 * W * b whole dwords at every W and every b.  A workgroup owns one channel and a range of samples (h_part, whole
// rows): scale, zero point, qmax, b, rowoff[c] and rowoff[C] are uniform.  A wave's step is 64 pieces, lane L piece L, one
// coalesced non-temporal load:
//   long rows (more than 64 pieces): 64 * W consecutive elements of one row, steps aligned to rows (the last one partly empty), so
//     every step starts on a dword of the row's stream;
//   short rows: floor(64 / pieces per row) whole rows of consecutive samples, each with its own window of ceil(H*W*b / 32) dwords.
// The lane ORs its run of W * b <= 64 bits into the at most three dwords it covers of the wave's own 128-dword LDS strip, then
// takes dwords L and 64 + L back with an exchange against zero - the strip is clean for the next step, the zero padding falls out
// of it - and stores those inside a row with plain stores: one or a few runs of consecutive dwords per wave.  Every dword of the
// N * rowoff[C] bytes is written exactly once, no byte beyond them, no global atomics, no read-modify-write of global memory.
// Waves never talk and there is no barrier: a wave's LDS operations execute in order (as k_pack_flat relies on).  The lane ->
// (row, piece, window) map is computed once per wave lifetime; no integer division in the loop; the next step's loads are issued
// before the current step is encoded.
//
// k_h_unpack, the load direction: k_h_qdq's geometry and walk; the lane that owns a piece reads, through the cache, the at most
// three dwords that hold its W * b bits, extracts W codes, (code - zp) * scale in fp32, one rounding into T, non-temporal store.
//
// The new kernels are compiled without the packed fp32 instructions (two scalar operations round as one packed one does).
#pragma once
#include "cnnq_half.hip.h"
#include "cnnq_nhwc_packed.hip.h"   // cl_pk_width: a width table entry as the format takes it

namespace {

// (a device attribute: the host pass does not know the feature.  Lambdas do not inherit it and would stay calls: none below)
#if defined(__HIP_DEVICE_COMPILE__)
#define H_PK_TARGET __attribute__((target("no-packed-fp32-ops")))
#else
#define H_PK_TARGET
#endif

constexpr int64_t H_PK_ELEMS = 16384;   // elements per pack workgroup (32 KB of x: 16 steps of 8-element pieces per wave)
constexpr int H_PK_STRIP = 128;         // dwords of a wave's strip: 64 pieces of 64 bits

// dwords of a row of HW codes of b bits
__device__ __forceinline__ uint32_t h_pk_rowdw(int HW, uint32_t b) { return (uint32_t)(((uint64_t)HW * b + 31u) >> 5); }

// the W codes of a piece, masked to b bits and concatenated: W * b <= 64 bits (a NaN code: 0)
template <class T, int W>
__device__ __forceinline__ unsigned long long h_pk_run(const uint16_t (&e)[W], bool fast, float sc, float rs, float zp, float qm, uint32_t b,
                                                       uint32_t mask) {
    float cd[W];
    if (fast) {
        if constexpr (W == 1) {
            (void)qdq1_fast(h_up(T{}, e[0]), sc, rs, zp, qm, cd[0]);
        } else {
            const f2v s2 = {sc, sc}, r2 = {rs, rs}, z2 = {zp, zp};
#pragma unroll
            for (int i = 0; i < W; i += 2) {
                f2v c2;
                (void)qdq2_fast(f2v{h_up(T{}, e[i]), h_up(T{}, e[i + 1])}, s2, r2, z2, qm, c2);
                cd[i] = c2.x;
                cd[i + 1] = c2.y;
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < W; ++i) (void)qdq1(h_up(T{}, e[i]), sc, zp, qm, cd[i]);
    }
    unsigned long long v = 0ull;
#pragma unroll
    for (int i = 0; i < W; ++i) {
        const uint32_t cu = cd[i] == cd[i] ? (uint32_t)cd[i] : 0u;
        v |= (unsigned long long)(cu & mask) << ((uint32_t)i * b);
    }
    return v;
}

// the strip's two operations, as builtins: the library's atomicOr / atomicExch are plain inline functions, which a kernel compiled
// for another feature set calls instead of inlining.  ds_or_b32; ds_wrxchg_rtn_b32 against zero
__device__ __forceinline__ void h_pk_or(uint32_t* p, uint32_t v) {
    (void)__hip_atomic_fetch_or(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ uint32_t h_pk_take(uint32_t* p) {
    return __hip_atomic_exchange(p, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// where a lane finds its piece of the wave's step (q, j), fixed for the wave's lifetime: row q * rmul + lr of the part, piece
// j * 64 + lp of that row
template <int W>
struct HPkLane {
    int rmul, lr, lp, rows, ppr;
    bool on;
    size_t P;
    __device__ __forceinline__ bool live(int q, int j) const { return on && q * rmul + lr < rows && j * 64 + lp < ppr; }
    // unconditional loads (a branch around a load serialises the loads): a dead lane re-reads the part's first piece
    __device__ __forceinline__ void load(const uint16_t* __restrict__ xp, int q, int j, uint16_t (&e)[W]) const {
        const size_t off = live(q, j) ? (size_t)(q * rmul + lr) * P + (size_t)(j * 64 + lp) * W : (size_t)0;
        h_ld<W, true>(xp + off, e);
    }
};

// x -> the packed rows.  rps: rows per step of the short form, 0: long rows.  PARTIALS = false: the table qp and the widths
// bits[C] with their layout rowoff[C + 1] (qdq1, the IEEE divide).  PARTIALS = true (config 2): the statistics partials
// pmm[npairs][2][C] of k_h_minmax - the workgroup merges its channel's pairs, derives the parameters with h_params (inside
// qdq_fast_domain the divide-free quotient) and the uniform width ha.num_bits; its layout is rowoff[c] = c * row bytes, which the
// first split publishes next to qp (rowoff is an OUTPUT then).  Dispatched in descending address order then, as k_h_qdq.
template <class T, int W, bool PARTIALS>
H_PK_TARGET __global__ void __launch_bounds__(TPB) k_h_pack(const uint16_t* __restrict__ x, uint32_t* __restrict__ packed, const HGeo g,
                                                            const int rps, const float* __restrict__ qp, const float* __restrict__ bits,
                                                            uint32_t* __restrict__ rowoff, const float* __restrict__ pmm, const HArgs ha) {
    constexpr int NW = TPB / 64;
    __shared__ uint32_t strips[NW][H_PK_STRIP];
    const HPart t = h_part<W, false>(g, PARTIALS ? (int)gridDim.x - 1 - (int)blockIdx.x : (int)blockIdx.x);
    const int c = t.c, lane = (int)threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint32_t (&strip)[H_PK_STRIP] = strips[wv];
    const int ppr = g.ppr;
    // the lane's (row, piece) inside a step
    HPkLane<W> ln{rps ? rps : 1, 0, lane, t.rows, ppr, true, (size_t)g.C * (size_t)g.HW};
    if (rps) {
        ln.lr = lane / ppr;
        ln.lp = lane - ln.lr * ppr;
        ln.on = ln.lr < rps;
    }
    const int lr = ln.lr, lp = ln.lp;
    // the wave's steps: a cursor (q, j) - long rows: step j of row q (spr steps per row); short rows: step q = rows [q * rps, ..)
    const int spr = rps ? 1 : (ppr + 63) >> 6;
    const int dq = NW / spr, dj = NW - dq * spr;
    int q = wv / spr, j = wv - q * spr;
    const uint16_t* const xp = x + t.off;
    uint16_t e[W];
    ln.load(xp, q, j, e);
    strip[lane] = 0u;
    strip[64 + lane] = 0u;
    // the channel's parameters only now: the first step of x is on its way while they arrive
    float sc, zp, qm;
    bool fast = false;
    uint32_t b, off_c, plane;
    if constexpr (PARTIALS) {
        float mn = INFINITY, mx = -INFINITY;
        for (int i = 0; i < ha.npairs; ++i) {
            mn = pmin(mn, pmm[(size_t)(2 * i) * g.C + c]);
            mx = pmax(mx, pmm[(size_t)(2 * i + 1) * g.C + c]);
        }
        h_params(mn, mx, ha.num_bits, ha.positive, sc, zp, qm);
        fast = qdq_fast_domain(mn, mx, sc);
        b = (uint32_t)ha.num_bits;
        const uint32_t rb = 4u * h_pk_rowdw(g.HW, b);
        off_c = (uint32_t)c * rb;
        plane = (uint32_t)g.C * rb;
        if (t.s == 0 && threadIdx.x == 0) {
            h_publish(ha, g.C, c, mn, mx, sc, zp, qm);
            rowoff[c] = off_c;
            if (c == g.C - 1) rowoff[g.C] = plane;
        }
    } else {
        h_qp(qp, g.C, c, sc, zp, qm);
        b = cl_pk_width(bits, 0, c);
        off_c = rowoff[c];
        plane = rowoff[g.C];
    }
    b = (uint32_t)__builtin_amdgcn_readfirstlane((int)b);
    if (b == 0u) return;                                    // a 0-bit channel stores nothing
    off_c = (uint32_t)__builtin_amdgcn_readfirstlane((int)off_c);
    plane = (uint32_t)__builtin_amdgcn_readfirstlane((int)plane);
    const bool ufast = __builtin_amdgcn_readfirstlane((int)fast) != 0;
    const float rs = ufast ? uniform_f(1.0f / sc) : 0.f;
    const uint32_t mask = (1u << b) - 1u;
    const uint32_t rdw = h_pk_rowdw(g.HW, b);               // dwords of a row
    const uint32_t sdw = rps ? (uint32_t)rps * rdw : 2u * W * b;   // dwords of a full step's windows, <= H_PK_STRIP
    // where the lane's run lies in the strip: bit s of dword d0
    const uint32_t bit0 = (rps ? (uint32_t)lr * rdw * 32u : 0u) + (uint32_t)lp * (W * b);
    const uint32_t d0 = bit0 >> 5, s = bit0 & 31u;
    // the two dwords the lane takes back: their row inside the step and their dword inside that row's window
    uint32_t kr[2] = {0u, 0u}, kd[2] = {(uint32_t)lane, 64u + (uint32_t)lane};
    if (rps) {
#pragma unroll
        for (int k = 0; k < 2; ++k) { kr[k] = kd[k] / rdw; kd[k] -= kr[k] * rdw; }
    }
    const int n0 = (int)(((int64_t)t.s * g.N) / g.S);       // the part's first sample (h_part)
    uint32_t* const chan = packed + (off_c >> 2);
    const int64_t plane4 = (int64_t)(plane >> 2);
    while (q * ln.rmul < t.rows) {
        int qn = q + dq, jn = j + dj;
        if (jn >= spr) { jn -= spr; ++qn; }
        uint16_t en[W];
        ln.load(xp, qn, jn, en);                                 // the prefetch behind the last step: one broadcast piece
        const unsigned long long v = ln.live(q, j) ? h_pk_run<T, W>(e, ufast, sc, rs, zp, qm, b, mask) : 0ull;
        const unsigned long long lo = v << s;
        const uint32_t w0 = (uint32_t)lo, w1 = (uint32_t)(lo >> 32), w2 = s ? (uint32_t)(v >> (64u - s)) : 0u;
        if (w0 && d0 < (uint32_t)H_PK_STRIP) h_pk_or(&strip[d0], w0);
        if (w1 && d0 + 1u < (uint32_t)H_PK_STRIP) h_pk_or(&strip[d0 + 1u], w1);
        if (w2 && d0 + 2u < (uint32_t)H_PK_STRIP) h_pk_or(&strip[d0 + 2u], w2);
        __builtin_amdgcn_wave_barrier();
        // long rows: the step's window is dwords [j * sdw, ..) of its row, cut at the row's end
        const uint32_t wbase = rps ? 0u : (uint32_t)j * sdw;
        const uint32_t wdw = rps ? rdw : (sdw < rdw - wbase ? sdw : rdw - wbase);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            if (k == 0 || sdw > 64u) {                      // uniform: one round covers a step of 64 dwords
                const uint32_t dw = h_pk_take(&strip[k * 64 + lane]);
                const int row = q * ln.rmul + (int)kr[k];
                if ((rps ? kr[k] < (uint32_t)rps : true) && kd[k] < wdw && row < t.rows)
                    chan[(int64_t)(n0 + row) * plane4 + (int64_t)(wbase + kd[k])] = dw;
            }
        }
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int i = 0; i < W; ++i) e[i] = en[i];
        q = qn;
        j = jn;
    }
}

// the packed rows -> y = (code - zp) * scale rounded once into T: k_h_qdq's geometry and walk; any geometry the family's plan admits
template <class T, int W>
H_PK_TARGET __global__ void __launch_bounds__(TPB) k_h_unpack(const uint32_t* __restrict__ packed, uint16_t* __restrict__ y, const HGeo g,
                                                              const float* __restrict__ qp, const float* __restrict__ bits,
                                                              const uint32_t* __restrict__ rowoff) {
    const HPart t = h_part<W, false>(g, (int)blockIdx.x);
    const int c = t.c;
    float sc, zp, qm;
    h_qp(qp, g.C, c, sc, zp, qm);
    const uint32_t b = (uint32_t)__builtin_amdgcn_readfirstlane((int)cl_pk_width(bits, 0, c));
    const uint32_t mask = (1u << b) - 1u, rdw = h_pk_rowdw(g.HW, b);
    const int n0 = (int)(((int64_t)t.s * g.N) / g.S);
    const uint32_t* const chan = packed + (rowoff[c] >> 2);
    const int64_t plane4 = (int64_t)(rowoff[g.C] >> 2);
    const size_t P = (size_t)g.C * (size_t)g.HW;
    HWalk w = h_walk(g.ppr);
    for (; w.r < t.rows; h_step(w, g.ppr)) {
        // the piece's W * b bits: bit s of dword d0 of the row, nd = 0 (b == 0) .. 3 dwords, none past the row's end
        const uint64_t bit0 = (uint64_t)w.p * (W * b);
        const uint32_t d0 = (uint32_t)(bit0 >> 5), s = (uint32_t)bit0 & 31u;
        uint32_t nd = (s + W * b + 31u) >> 5;
        const uint32_t room = d0 < rdw ? rdw - d0 : 0u;
        nd = nd < room ? nd : room;
        const uint32_t* __restrict__ p = chan + (int64_t)(n0 + w.r) * plane4 + (int64_t)d0;
        const uint32_t w0 = nd > 0u ? p[0] : 0u, w1 = nd > 1u ? p[1] : 0u, w2 = nd > 2u ? p[2] : 0u;
        unsigned long long v = (((unsigned long long)w1 << 32) | w0) >> s;
        if (s) v |= (unsigned long long)w2 << (64u - s);
        uint16_t e[W];
#pragma unroll
        for (int i = 0; i < W; ++i) {
            const float cd = (float)((uint32_t)(v >> ((uint32_t)i * b)) & mask);
            e[i] = h_down(T{}, (cd - zp) * sc);                                  // iq.py:591-592
        }
        h_st_nt<W>(y + t.off + (size_t)w.r * P + (size_t)w.p * W, e);
    }
}

// (config 2 on fp32 through the fp32 entry points: they take the widths as a device table)
__global__ void __launch_bounds__(PTPB) k_h_fill_width(float* __restrict__ bits, int C, float b) {
    for (int c = (int)threadIdx.x; c < C; c += PTPB) bits[c] = b;
}

// ---- host side
// rows per step of the pack launch at piece width w: 0 - long rows (more than 64 pieces)
inline int h_pk_rps(int64_t HW, int w) {
    const int64_t ppr = HW / w;
    return ppr > 64 ? 0 : (int)(64 / ppr);
}
inline HGeo h_geo_pack(int64_t N, int64_t C, int64_t HW, int w) { return h_geo(N, C, HW, w, h_splits(N, C, HW, H_PK_ELEMS, N), 1); }

}  // namespace
