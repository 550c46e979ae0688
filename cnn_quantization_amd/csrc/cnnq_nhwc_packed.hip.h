// cnnq_nhwc_packed.hip.h - integer codes as the STORED format of a dense channels_last activation:
// per-channel widths of 0..8 bits, fp32 / bf16 / fp16 elements, on the storage as it is.
// Part of the single translation unit cnnq_kernels.hip (see its header for the design).
//
// Format (include/cnnq_hip.h): the tensor is [R = N*H*W][C], C innermost.  Row r stores the codes of channels 0..C-1 as one
// little-endian bit stream: channel c occupies bits [coloff[c], coloff[c] + bits[c]), coloff[C + 1] the exclusive prefix sum of the
// widths (k_cl_packed_layout), a row is padded with zero bits to rowdw = ceil(coloff[C] / 32) dwords and starts at dword r * rowdw.
// Uniform 4 or 8 bits are the same format with a constant width table.
//
// The stored code is qdq1's `code` (inside qdq_fast_domain, with the channel's exact extrema, the divide-free quotient's: the
// same bits); a NaN code is stored as 0.  Decode is (code - zp) * scale, then cl_down: what k_cl_qdq stores.
//
// Tiling: the piece of cnnq_nhwc.hip.h - W consecutive channels, one load - so a lane's bit offsets, widths and masks are constants
// in registers next to scale and zero point.  Neighbouring pieces share dwords, and so would ClGeo's column blocks, so the pack
// launch has its own geometry (PkGeo): a workgroup owns WHOLE rows.  Its lanes OR their runs (at most 8 codes x 8 bits at a
// constant shift: three dwords) into a zeroed LDS image of a tile of RT rows - OR does not depend on the order - and the
// workgroup then writes the image, which is one contiguous dword range of the buffer, with plain coalesced stores: every dword of
// the buffer is written exactly once, padding included, no global atomics, no read-modify-write of global memory.  Two images
// alternate, so a tile costs one barrier.  More than TPB pieces per row (C > 1024 in fp32, > 2048 in bf16): the lanes walk the
// column blocks of the tile's rows one after the other and reload their constants per block.
//
// CL_PK_IMG: the largest tile image, in dwords.  A row at 8 bits per code is ceil(C / 4) dwords, so C <= 4 * CL_PK_IMG = 8192 is
// native at every piece width; a larger C returns CNNQ_ENOTSUP before any launch.
#pragma once
#include "cnnq_nhwc.hip.h"
#include "cnnq_params.hip.h"   // PTPB

namespace {

constexpr int CL_PK_IMG = 2048;            // dwords of one tile image (two of them: 16 KB of LDS)
constexpr int64_t CL_PK_ELEMS = 32768;     // elements per pack workgroup at least (amortises zeroing the images)
constexpr int CL_PK_ROWS_MAX = 8;          // rows per tile at most when a row has several column blocks

// the pack launch: workgroup b owns rows [b * rpw, (b + 1) * rpw), in tiles of RT rows
struct PkGeo {
    int64_t R;      // rows
    int64_t rpw;    // rows per workgroup, a multiple of RT
    int C;          // channels
    int P;          // pieces per row
    int CP;         // pieces per column block, min(P, TPB)
    int RS;         // rows per step, TPB / CP
    int nb;         // column blocks
    int RT;         // rows per tile: 2 * RS (nb == 1: two loads in flight per lane), else up to CL_PK_ROWS_MAX; RT * capdw <= CL_PK_IMG
    uint32_t capdw; // dwords of a row at 8 bits per code, ceil(C / 4): no row is longer, whatever coloff says
};

// a width table entry as the format takes it: an integer in 0..8, NaN and negative values 0
__device__ __forceinline__ uint32_t cl_pk_width(const float* __restrict__ bits, int uniform, int c) {
    if (!bits) return (uint32_t)min(max(uniform, 0), 8);
    const float b = bits[c];
    return b >= 8.f ? 8u : (b >= 0.f ? (uint32_t)b : 0u);
}

// bits[C] (or, bits == NULL, `uniform` for every channel) -> coloff[C + 1], the exclusive prefix sum: one workgroup, the scan of
// k_packed_layout.  Every width is clamped into 0..8, so coloff[C] <= 8 * C and a bad table can never make k_cl_pack write
// outside cnnq_pc_packed_nhwc_capacity.
__global__ void __launch_bounds__(PTPB) k_cl_packed_layout(const float* __restrict__ bits, int uniform, int C, uint32_t* __restrict__ coloff) {
    __shared__ uint32_t wsum[PTPB / 64];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int per = (C + PTPB - 1) / PTPB;
    uint32_t sum = 0;
    for (int c = tid * per; c < min(C, (tid + 1) * per); ++c) sum += cl_pk_width(bits, uniform, c);
    uint32_t incl = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)incl, d, 64);
        if (lane >= d) incl += o;
    }
    if (lane == 63) wsum[wv] = incl;
    __syncthreads();
    uint32_t base = incl - sum;
    for (int w = 0; w < wv; ++w) base += wsum[w];
    for (int c = tid * per; c < min(C, (tid + 1) * per); ++c) {
        coloff[c] = base;
        base += cl_pk_width(bits, uniform, c);
    }
    if (tid == PTPB - 1) coloff[C] = base;
}

// dwords per row of the table, never more than the 8-bit row (a coloff the library did not write may say anything)
__device__ __forceinline__ uint32_t cl_pk_rowdw(const uint32_t* __restrict__ coloff, int C, uint32_t capdw) {
    const uint32_t dw = (coloff[C] >> 5) + ((coloff[C] & 31u) ? 1u : 0u);
    return dw < capdw ? dw : capdw;
}

// a piece's place in the row's stream: its first dword d0 and the bit s inside it, and per channel the shift inside the piece's
// run and the mask of its width.  Widths above 8 and shifts above 56 (a foreign table) are clamped: the run stays inside 64 bits.
template <int W>
struct PkRun {
    uint32_t d0, s;
    uint32_t sh[W], msk[W];
    __device__ __forceinline__ void load(const uint32_t* __restrict__ coloff, int c0) {
        const uint32_t b0 = coloff[c0];
        d0 = b0 >> 5;
        s = b0 & 31u;
#pragma unroll
        for (int i = 0; i < W; ++i) {
            const uint32_t o = coloff[c0 + i], wd = coloff[c0 + i + 1] - o;
            sh[i] = min(o - b0, 56u);
            msk[i] = (1u << min(wd, 8u)) - 1u;
        }
    }
};

// x -> the packed rows.  mm as k_cl_qdq: NULL - qdq1 (the IEEE divide); the channels' exact extrema [2][C] - inside
// qdq_fast_domain the divide-free quotient.  x is read for the last time: non-temporal loads.  DIRECT (the host knows a uniform
// width b with W * b a multiple of 32): every piece's run is one or two whole dwords, stored straight from registers.
template <class T, int W, bool DIRECT>
__global__ void __launch_bounds__(TPB) k_cl_pack(const typename ClRaw<T>::type* __restrict__ x, uint32_t* __restrict__ packed, const PkGeo g,
                                                 const float* __restrict__ qp, const float* __restrict__ mm,
                                                 const uint32_t* __restrict__ coloff) {
    typedef typename ClRaw<T>::type E;
    __shared__ uint32_t img[DIRECT ? 1 : 2 * CL_PK_IMG];
    const int t = (int)threadIdx.x;
    const uint32_t rowdw = cl_pk_rowdw(coloff, g.C, g.capdw);
    if (rowdw == 0u) return;                                  // every width 0: nothing is stored (uniform)
    if constexpr (!DIRECT) {
        for (int i = t; i < 2 * CL_PK_IMG; i += TPB) img[i] = 0u;
        __syncthreads();
    }
    const int lr = t / g.CP, lp = t - lr * g.CP;
    const int64_t r0 = (int64_t)blockIdx.x * g.rpw;
    const int64_t r1 = r0 + g.rpw < g.R ? r0 + g.rpw : g.R;
    float sc[W], zp[W], qm[W], rs[W];
    PkRun<W> run;
    bool fast = false;
    auto load_piece = [&](int piece) {
        const int c0 = piece * W;
#pragma unroll
        for (int i = 0; i < W; ++i) {
            sc[i] = qp[(size_t)CNNQ_QP_SCALE * g.C + c0 + i];
            zp[i] = qp[(size_t)CNNQ_QP_ZP * g.C + c0 + i];
            qm[i] = qp[(size_t)CNNQ_QP_QMAX * g.C + c0 + i];
        }
        fast = mm != nullptr;
        if (fast) {
#pragma unroll
            for (int i = 0; i < W; ++i) fast = fast && qdq_fast_domain(mm[c0 + i], mm[g.C + c0 + i], sc[i]) && qm[i] == qm[0];
        }
#pragma unroll
        for (int i = 0; i < W; ++i) rs[i] = fast ? 1.0f / sc[i] : 0.f;
        run.load(coloff, c0);
    };
    // the W codes of one row's piece -> the piece's run (a NaN code is stored as 0; every code masked to its channel's width)
    auto run_of = [&](const E (&e)[W]) -> unsigned long long {
        float cd[W];
        if (fast) {
            if constexpr (W == 1) {
                (void)qdq1_fast(cl_up(T{}, e[0]), sc[0], rs[0], zp[0], qm[0], cd[0]);
            } else {
#pragma unroll
                for (int i = 0; i < W; i += 2) {
                    f2v c2;
                    (void)qdq2_fast(f2v{cl_up(T{}, e[i]), cl_up(T{}, e[i + 1])}, f2v{sc[i], sc[i + 1]}, f2v{rs[i], rs[i + 1]},
                                    f2v{zp[i], zp[i + 1]}, qm[0], c2);
                    cd[i] = c2.x;
                    cd[i + 1] = c2.y;
                }
            }
        } else {
#pragma unroll
            for (int i = 0; i < W; ++i) (void)qdq1(cl_up(T{}, e[i]), sc[i], zp[i], qm[i], cd[i]);
        }
        unsigned long long v = 0ull;
#pragma unroll
        for (int i = 0; i < W; ++i) {
            const uint32_t cu = cd[i] == cd[i] ? (uint32_t)cd[i] : 0u;
            v |= (unsigned long long)(cu & run.msk[i]) << run.sh[i];
        }
        return v;
    };
    // the run at bit s of dword d0 of a row: three dwords; only bits of the row's own stream are ever set, and a dword past the
    // row's end (a foreign table) is dropped
    auto emit = [&](unsigned long long v, uint32_t* __restrict__ row) {
        const unsigned long long lo = v << run.s;
        const uint32_t w0 = (uint32_t)lo, w1 = (uint32_t)(lo >> 32), w2 = run.s ? (uint32_t)(v >> (64u - run.s)) : 0u;
        if constexpr (DIRECT) {
            if (run.d0 < rowdw) row[run.d0] = w0;
            if (run.msk[W - 1] && run.sh[W - 1] >= 32u && run.d0 + 1u < rowdw) row[run.d0 + 1u] = w1;
        } else {
            if (w0 && run.d0 < rowdw) atomicOr(&row[run.d0], w0);
            if (w1 && run.d0 + 1u < rowdw) atomicOr(&row[run.d0 + 1u], w1);
            if (w2 && run.d0 + 2u < rowdw) atomicOr(&row[run.d0 + 2u], w2);
        }
    };
    const bool one = g.nb == 1;
    if (one && lr < g.RS) load_piece(lp);
    int buf = 0;
    for (int64_t tr = r0; tr < r1; tr += g.RT) {
        uint32_t* im = img + (DIRECT ? 0 : buf * CL_PK_IMG);
        for (int b = 0; b < g.nb; ++b) {
            const int piece = b * g.CP + lp;
            if (lr >= g.RS || piece >= g.P) continue;
            if (!one) load_piece(piece);
            const int c0 = piece * W;
            for (int rr = lr; rr < g.RT; rr += 2 * g.RS) {
                const int64_t ra = tr + rr, rb = ra + g.RS;
                const bool oka = ra < r1, okb = rr + g.RS < g.RT && rb < r1;
                E ea[W], eb[W];
#pragma unroll
                for (int i = 0; i < W; ++i) { ea[i] = E(0); eb[i] = E(0); }
                if (oka) cl_ld<E, W, true>(x + ra * g.C + c0, ea);
                if (okb) cl_ld<E, W, true>(x + rb * g.C + c0, eb);
                if constexpr (DIRECT) {
                    if (oka) emit(run_of(ea), packed + ra * (int64_t)rowdw);
                    if (okb) emit(run_of(eb), packed + rb * (int64_t)rowdw);
                } else {
                    if (oka) emit(run_of(ea), im + (uint32_t)rr * rowdw);
                    if (okb) emit(run_of(eb), im + (uint32_t)(rr + g.RS) * rowdw);
                }
            }
        }
        if constexpr (!DIRECT) {
            __syncthreads();
            // the tile's rows are one contiguous dword range of the buffer; the lane that stores a dword zeroes it for the tile
            // after next (the next tile's barrier lies in between)
            const int64_t left = r1 - tr;
            const uint32_t n = (uint32_t)(left < g.RT ? left : g.RT) * rowdw;
            uint32_t* __restrict__ dst = packed + tr * (int64_t)rowdw;
            for (uint32_t j = (uint32_t)t; j < n; j += TPB) {
                dst[j] = im[j];
                im[j] = 0u;
            }
            buf ^= 1;
        }
    }
}

// the packed rows -> y = (code - zp) * scale in x's element type: k_cl_qdq's geometry (the element-wise pass), a lane reads the at
// most three dwords that cover its piece's run through the cache and writes y non-temporally
template <class T, int W>
__global__ void __launch_bounds__(TPB) k_cl_unpack(const uint32_t* __restrict__ packed, typename ClRaw<T>::type* __restrict__ y, const ClGeo g,
                                                   const float* __restrict__ qp, const uint32_t* __restrict__ coloff, uint32_t capdw) {
    typedef typename ClRaw<T>::type E;
    const ClLane l = cl_lane(g, (int)blockIdx.x);
    if (l.piece < 0) return;
    const int c0 = l.piece * W;
    const uint32_t rowdw = cl_pk_rowdw(coloff, g.C, capdw);
    float sc[W], zp[W];
#pragma unroll
    for (int i = 0; i < W; ++i) {
        sc[i] = qp[(size_t)CNNQ_QP_SCALE * g.C + c0 + i];
        zp[i] = qp[(size_t)CNNQ_QP_ZP * g.C + c0 + i];
    }
    PkRun<W> run;
    run.load(coloff, c0);
    // dwords of the row that hold bits of this piece, from d0 on: 0 (every width 0) .. 3, none past the row's end
    uint32_t top = 0u;
#pragma unroll
    for (int i = 0; i < W; ++i) top = run.msk[i] ? max(top, run.s + run.sh[i] + (uint32_t)__popc(run.msk[i])) : top;
    uint32_t nd = (top + 31u) >> 5;
    const uint32_t room = run.d0 < rowdw ? rowdw - run.d0 : 0u;
    nd = nd < room ? nd : room;
    const int64_t step = (int64_t)g.RS * g.C, pstep = (int64_t)g.RS * rowdw;
    int64_t off = l.r * g.C + c0;
    const uint32_t* __restrict__ p = packed + l.r * (int64_t)rowdw + run.d0;
    for (int64_t r = l.r; r < l.r1; r += g.RS, off += step, p += pstep) {
        const uint32_t w0 = nd > 0u ? p[0] : 0u, w1 = nd > 1u ? p[1] : 0u, w2 = nd > 2u ? p[2] : 0u;
        unsigned long long v = (((unsigned long long)w1 << 32) | w0) >> run.s;
        if (run.s) v |= (unsigned long long)w2 << (64u - run.s);
        E e[W];
#pragma unroll
        for (int i = 0; i < W; ++i) {
            const float cd = (float)((uint32_t)(v >> run.sh[i]) & run.msk[i]);
            e[i] = cl_down(T{}, (cd - zp[i]) * sc[i]);                                  // iq.py:591-592
        }
        cl_st_nt<E, W>(y + off, e);
    }
}

// ---- host side
inline uint32_t cl_pk_capdw(int64_t C) { return (uint32_t)((C + 3) / 4); }
inline bool cl_pk_native(int64_t C) { return (C + 3) / 4 <= CL_PK_IMG; }

// the pack geometry for piece width w (C native)
inline PkGeo cl_pk_geo(int64_t R, int64_t C, int w) {
    PkGeo g;
    g.R = R;
    g.C = (int)C;
    g.P = (int)(C / w);
    g.CP = g.P < TPB ? g.P : TPB;
    g.RS = TPB / g.CP;
    g.nb = (g.P + g.CP - 1) / g.CP;
    g.capdw = cl_pk_capdw(C);
    if (g.nb == 1) {
        g.RT = 2 * g.RS;                      // at most 2 * (256 / P) * (P * W / 4 + 3 / 4) <= 128 * W + 384 <= 1408 dwords
    } else {
        g.RT = CL_PK_IMG / (int)g.capdw;      // RS == 1
        g.RT = g.RT > CL_PK_ROWS_MAX ? CL_PK_ROWS_MAX : g.RT;
    }
    const int64_t tile = (int64_t)g.RT * C;
    int64_t tiles = (CL_PK_ELEMS + tile - 1) / tile;
    const int64_t all = (R + g.RT - 1) / g.RT;
    tiles = tiles > all ? all : tiles;
    g.rpw = tiles * g.RT;
    return g;
}
inline int64_t cl_pk_wgs(const PkGeo& g) { return (g.R + g.rpw - 1) / g.rpw; }

}  // namespace
