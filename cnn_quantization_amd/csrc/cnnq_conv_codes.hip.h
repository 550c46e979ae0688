// cnnq_conv_codes.hip.h - the integer 2-D convolution on the stored codes: y[N][OH][OW][Cout] from NHWC
// activation codes xq[N][H][W][C] (per tensor or per image) and OHWI weight codes wq[Cout][KH][KW][C] (per output channel), as an
// implicit GEMM on v_mfma_i32_16x16x64_i8: M = N OH OW rows, Cout columns, k = (kh, kw, c).  Everything of the linear layer
// (cnnq_linear_codes.hip.h) that does not depend on where a row of A lies is used as it stands: the operand formats, lc_fetch /
// lc_signed / lc_slot, the swizzled double-buffered LDS, the three macro tiles of lc_plan, the split of k and the fp64 finish
// (lc_combine).  Part of the single translation unit cnnq_kernels.hip.
//
// The arithmetic.  A padded tap is the real value 0.0, not a code: the sums of section 35 run over the VALID taps of output pixel m,
// a rectangle kh in [kh0, kh1) x kw in [kw0, kw1) that depends on (oh, ow) alone:
//     y[m][n] = sx sw[n] (S - zw[n] Rx[m] - zx RwV[m][n] + Kv[m] zx zw[n]) + bias[n]
//     S = sum_valid xq wq,  Rx[m] = sum_valid xq,  RwV[m][n] = sum_{valid taps} sum_c wq[n][tap][c],  Kv[m] = C * #valid taps
// The tiles load an invalid tap (as a row beyond M / Cout and a dword beyond K) as the code whose signed form is zero, so they
// accumulate S' = sum_valid (xq - ox)(wq - ow), and cc_finish returns to S = S' + ow Rx + ox RwV - Kv ox ow in 64-bit integers.
//
// Four kernels (and k_lc_rowsums as it stands for the per-pixel channel sums pix[N H W]):
//   k_cc_tapsums   per layer: the summed-area table taps[Cout][KH + 1][KW + 1] of the tap sums sum_c wq[n][kh][kw][c]; RwV of any
//                  rectangle is four lookups.  One workgroup per output channel, a wave per tap (v_sad_u8 on whole dwords).
//   k_cc_winsums   one thread per output pixel: its valid rectangle, packed into a word, and Rx = the valid pixels' sums.
//   k_cc_gemm      the tiles of S'; k_lc_gemm's schedule with a gathered A operand (below); with one split its tail finishes.
//   k_cc_epilogue  splits > 1: adds the splits' int32 partial tiles, then the same cc_finish - the same bits for every split count.
// The Q instances of k_cc_gemm and k_cc_epilogue_q store NHWC codes instead of fp32, as the linear layer's: cnnq_requant_codes.hip.h;
// the R instances add a residual of NHWC codes before ReLU and the quantizer (section 38).
//
// The A path.  The rows a thread fetches are the same for every step of a tile: they are decomposed into (image, oh, ow) and the
// window origin ih0 = oh sh - ph, iw0 = ow sw - pw ONCE, before the k loop (rows beyond M get an origin no tap of which is inside
// the image).  All chunks of a thread have the same chunk index c & 3 = tid & 3, so ONE position (kh, kw, channel) per thread says
// where its chunks lie in k; it is set by two divisions before the loop and then advanced by 64 codes per step with carries
// (channel -> kw -> kh): no division or modulo inside the loop.  V16 (C % 16 == 0, bases aligned to a chunk): a chunk of 16 codes
// lies inside one tap - lc_fetch's one dwordx4 (dwordx2) load on the pixel's channels, or the fill if the tap is outside the image.
// Otherwise a dword at a time: C % 4 (u8) / C % 8 (pack4) keeps every dword inside one tap, the position is carried from dword to
// dword and the validity test is per dword.  Offsets into xq are 64-bit.  With both operands pack4 the permutes are left out as in
// the linear layer: tap boundaries fall on dword boundaries, so both sides present every dword's nibbles as (even, odd).
#pragma once
#include "cnnq_linear_codes.hip.h"

namespace {

constexpr int CC_MAX_TAPS = 64;      // KH * KW: the rectangle's four bounds fit a byte each, the table a workgroup's LDS

struct CcGeo {
    int H, W, C, OW, OHW, KH, KW, sh, sw, ph, pw;
};

// what the tail of every element needs: section 35's (e.rx = Rx[M]; e.rw and e.K are not read) and the valid rectangles
struct CcEpi {
    LcEpi e;
    const unsigned* rect;   // [M] kh0 | kh1 << 8 | kw0 << 16 | kw1 << 24
    const int* taps;        // [Cout][KH + 1][KW + 1]
    int KW1, ntab, C, OHW;  // KW + 1, (KH + 1)(KW + 1)
};

struct CcArgs {
    const unsigned char* xq;
    const unsigned char* wq;
    float* y;
    int* part;              // [splits][M][Cout], splits > 1
    int M, tilesM, tilesN, splits;
    CcGeo g;
    CcEpi e;
    RqOut q;                // Q instances: the codes' destination instead of y (cnnq_requant_codes.hip.h)
    RqRes r;                // R instances: the residual codes added before ReLU and the quantizer (section 38)
};

// the valid taps of the window whose origin is (ih0, iw0): kh0 <= kh1, kw0 <= kw1 (an empty rectangle where no tap is inside)
__device__ __forceinline__ void cc_window(const CcGeo& g, int ih0, int iw0, int& kh0, int& kh1, int& kw0, int& kw1) {
    kh0 = min(max(-ih0, 0), g.KH);
    kh1 = max(min(g.H - ih0, g.KH), kh0);
    kw0 = min(max(-iw0, 0), g.KW);
    kw1 = max(min(g.W - iw0, g.KW), kw0);
}

// ---- per layer: the summed-area table of the tap sums --------------------------------------------------------------------------
__global__ __launch_bounds__(TPB) void k_cc_tapsums(const unsigned char* __restrict__ wq, int fw, int KH, int KW, int C, int* __restrict__ taps) {
    __shared__ int sums[CC_MAX_TAPS];
    const int lane = threadIdx.x & 63, ntaps = KH * KW;
    const int ndw = fw == CNNQ_CODES_U8 ? C / 4 : C / 8;
    const unsigned* w = reinterpret_cast<const unsigned*>(wq) + (size_t)blockIdx.x * ntaps * ndw;
    for (int t = threadIdx.x >> 6; t < ntaps; t += TPB / 64) {
        const unsigned* p = w + (size_t)t * ndw;
        unsigned acc = 0;
        if (fw == CNNQ_CODES_U8) {
            for (int i = lane; i < ndw; i += 64) acc = __builtin_amdgcn_sad_u8(p[i], 0u, acc);
        } else {
            for (int i = lane; i < ndw; i += 64) {
                const unsigned v = p[i];
                acc = __builtin_amdgcn_sad_u8(v & 0x0F0F0F0Fu, 0u, acc);
                acc = __builtin_amdgcn_sad_u8((v >> 4) & 0x0F0F0F0Fu, 0u, acc);
            }
        }
        int s = (int)acc;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (lane == 0) sums[t] = s;
    }
    __syncthreads();
    // entry (a, b) = the taps kh < a, kw < b: at most 64 additions, serially
    const int KW1 = KW + 1, ntab = (KH + 1) * KW1;
    for (int i = threadIdx.x; i < ntab; i += TPB) {
        const int a = i / KW1, b = i % KW1;
        int s = 0;
        for (int kh = 0; kh < a; ++kh)
            for (int kw = 0; kw < b; ++kw) s += sums[kh * KW + kw];
        taps[(size_t)blockIdx.x * ntab + i] = s;
    }
}

// ---- per call: Rx and the valid rectangle of every output pixel, from the pixel sums ------------------------------------------------
__global__ __launch_bounds__(TPB) void k_cc_winsums(const int* __restrict__ pix, const CcGeo g, int M, int* __restrict__ rx, unsigned* __restrict__ rect) {
    const long long idx = (long long)blockIdx.x * TPB + threadIdx.x;
    if (idx >= M) return;
    const int m = (int)idx, img = m / g.OHW, o = m % g.OHW;
    const int ih0 = (o / g.OW) * g.sh - g.ph, iw0 = (o % g.OW) * g.sw - g.pw;
    int kh0, kh1, kw0, kw1;
    cc_window(g, ih0, iw0, kh0, kh1, kw0, kw1);
    int s = 0;
    for (int kh = kh0; kh < kh1; ++kh) {
        const int* p = pix + ((long long)img * g.H + (ih0 + kh)) * g.W + iw0;
        for (int kw = kw0; kw < kw1; ++kw) s += p[kw];
    }
    rx[m] = s;
    rect[m] = (unsigned)kh0 | (unsigned)kh1 << 8 | (unsigned)kw0 << 16 | (unsigned)kw1 << 24;
}

// ---- the finish ------------------------------------------------------------------------------------------------------------------------
// what every element of row m shares: two words read, nothing divided unless the table is per image
struct CcRow {
    long long rx, kv;
    int at[4];              // the rectangle's corners in a channel's table: + (kh1, kw1) - (kh0, kw1) - (kh1, kw0) + (kh0, kw0)
    int mp;
};
__device__ __forceinline__ CcRow cc_row(int m, const CcEpi& e) {
    const unsigned r = e.rect[m];
    const int kh0 = r & 255, kh1 = (r >> 8) & 255, kw0 = (r >> 16) & 255, kw1 = r >> 24;
    CcRow o;
    o.rx = e.e.rx[m];
    o.kv = (long long)e.C * ((kh1 - kh0) * (kw1 - kw0));
    o.at[0] = kh1 * e.KW1 + kw1;
    o.at[1] = kh0 * e.KW1 + kw1;
    o.at[2] = kh1 * e.KW1 + kw0;
    o.at[3] = kh0 * e.KW1 + kw0;
    o.mp = e.e.Cx == 1 ? 0 : m / e.OHW;
    return o;
}
__device__ __forceinline__ float cc_finish(long long sp, const CcRow& r, int n, const CcEpi& e) {
    const int* t = e.taps + (size_t)n * e.ntab;
    const long long rwv = (long long)t[r.at[0]] - t[r.at[1]] - t[r.at[2]] + t[r.at[3]];
    return lc_combine(sp, r.rx, rwv, r.kv, r.mp, n, e.e);
}

// ---- the gathered operand ---------------------------------------------------------------------------------------------------------------
// where a chunk lies in k = (kh, kw, c); advanced by `by` codes with carries, no division
struct CcPos {
    int kh, kw, c;
};
__device__ __forceinline__ void cc_advance(CcPos& p, int by, const CcGeo& g) {
    p.c += by;
    while (p.c >= g.C) {
        p.c -= g.C;
        if (++p.kw == g.KW) {
            p.kw = 0;
            ++p.kh;
        }
    }
}
// a row of A: its image and window origin (rows beyond M: an origin far outside every image)
struct CcARow {
    int img, ih0, iw0;
};
// the address of pixel (ih0 + kh, iw0 + kw)'s channels, or nullptr when that tap is padding or beyond KH
template <int FMT>
__device__ __forceinline__ const unsigned char* cc_pixel(const unsigned char* __restrict__ xq, const CcGeo& g, const CcARow& r, const CcPos& p) {
    const int ih = r.ih0 + p.kh, iw = r.iw0 + p.kw;
    if (p.kh >= g.KH || (unsigned)ih >= (unsigned)g.H || (unsigned)iw >= (unsigned)g.W) return nullptr;
    const long long px = ((long long)r.img * g.H + ih) * g.W + iw;
    return xq + px * g.C / (FMT == CNNQ_CODES_U8 ? 1 : 2);
}
// the chunk of 16 codes at position p of row r
template <int FMT, bool V16>
__device__ __forceinline__ void cc_fetch(const unsigned char* __restrict__ xq, const CcGeo& g, const CcARow& r, const CcPos& p, LcRaw<FMT>& raw) {
    if constexpr (V16) {                 // C % 16 == 0: the chunk is inside one tap
        const unsigned char* px = cc_pixel<FMT>(xq, g, r, p);
        lc_fetch<FMT, true>(px ? px : xq, px ? 1 : 0, g.C, 0, p.c, raw);
    } else {
        constexpr int ND = LcRaw<FMT>::ND, CPD = LcRaw<FMT>::CPD;
        CcPos q = p;
#pragma unroll
        for (int i = 0; i < ND; ++i) {
            const unsigned char* px = cc_pixel<FMT>(xq, g, r, q);
            raw.d[i] = px ? reinterpret_cast<const unsigned*>(px)[q.c / CPD] : LcRaw<FMT>::FILL;
            cc_advance(q, CPD, g);
        }
    }
}

// ---- the tiles ------------------------------------------------------------------------------------------------------------------
// Q: with one split the tail stores codes (a.q) instead of fp32 (a.y): section 37.  R (with Q): it adds the residual codes a.r first:
// section 38
template <int WM, int WN, int TM, int TN, int FX, int FW, bool V16, bool Q = false, bool R = false>
__global__ __launch_bounds__(TPB) void k_cc_gemm(const CcArgs a) {
    static_assert(WM * WN == TPB / 64, "four waves");
    static_assert(Q || !R, "the residual is added on the way to codes");
    constexpr int BM = WM * TM * 16, BN = WN * TN * 16;
    constexpr int CA = BM * 4, CB = BN * 4;                          // chunks per step
    constexpr int NA = (CA + TPB - 1) / TPB, NB = (CB + TPB - 1) / TPB;
    constexpr bool NATURAL = FX != FW;
    __shared__ lc_u4 lds[2][CA + CB];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / WN, wn = wave % WN;
    unsigned id = blockIdx.x;
    const int tn = (int)(id % (unsigned)a.tilesN);
    id /= (unsigned)a.tilesN;
    const int tm = (int)(id % (unsigned)a.tilesM), split = (int)(id / (unsigned)a.tilesM);
    const int m0 = tm * BM, n0 = tn * BN;
    const int M = a.M, N = a.e.e.N, K = a.e.e.K;
    const CcGeo& g = a.g;
    const int steps = (K + LC_BK - 1) / LC_BK;
    const int s0 = (int)((long long)split * steps / a.splits), s1 = (int)((long long)(split + 1) * steps / a.splits);

    // the thread's rows of A, for the whole tile, and its chunks' position in k at the split's first step
    CcARow rows[NA];
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        const int m = m0 + ((tid + i * TPB) >> 2);
        if (m < M) {
            const int o = m % g.OHW;
            rows[i].img = m / g.OHW;
            rows[i].ih0 = (o / g.OW) * g.sh - g.ph;
            rows[i].iw0 = (o % g.OW) * g.sw - g.pw;
        } else {
            rows[i].img = 0;
            rows[i].ih0 = rows[i].iw0 = -(1 << 30);
        }
    }
    CcPos pos;
    {
        const int k = s0 * LC_BK + (tid & 3) * 16, tap = k / g.C;
        pos.c = k % g.C;
        pos.kh = tap / g.KW;
        pos.kw = tap % g.KW;
    }

    LcRaw<FX> ra[NA];
    LcRaw<FW> rb[NB];
    auto fetch = [&](int step) {
        const int k0 = step * LC_BK;
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int c = tid + i * TPB;
            if (CA % TPB == 0 || c < CA) cc_fetch<FX, V16>(a.xq, g, rows[i], pos, ra[i]);
        }
        cc_advance(pos, LC_BK, g);
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int c = tid + i * TPB;
            if (CB % TPB == 0 || c < CB) lc_fetch<FW, V16>(a.wq, N, K, n0 + (c >> 2), k0 + (c & 3) * 16, rb[i]);
        }
    };
    auto stash = [&](int buf) {
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int c = tid + i * TPB;
            if (CA % TPB == 0 || c < CA) lds[buf][lc_slot(c >> 2, c & 3)] = lc_signed<FX, NATURAL>(ra[i]);
        }
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            const int c = tid + i * TPB;
            if (CB % TPB == 0 || c < CB) lds[buf][CA + lc_slot(c >> 2, c & 3)] = lc_signed<FW, NATURAL>(rb[i]);
        }
    };

    lc_v4i acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) acc[i][j] = lc_v4i{0, 0, 0, 0};

    const int fr = lane & 15, fc = lane >> 4;                        // the lane's row of an instruction tile and its chunk of k
    if (s0 < s1) {
        fetch(s0);
        stash(0);
    }
    __syncthreads();
    for (int s = s0; s < s1; ++s) {
        const int buf = (s - s0) & 1;
        if (s + 1 < s1) fetch(s + 1);                                // in flight during the multiplications
        lc_v4i fa[TM], fb[TN];
#pragma unroll
        for (int i = 0; i < TM; ++i) fa[i] = __builtin_bit_cast(lc_v4i, lds[buf][lc_slot((wm * TM + i) * 16 + fr, fc)]);
#pragma unroll
        for (int j = 0; j < TN; ++j) fb[j] = __builtin_bit_cast(lc_v4i, lds[buf][CA + lc_slot((wn * TN + j) * 16 + fr, fc)]);
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j) acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(fa[i], fb[j], acc[i][j], 0, 0, 0);
        if (s + 1 < s1) stash(buf ^ 1);                              // nobody reads that buffer before the barrier
        __syncthreads();
    }

    // the lane's results: rows 4 (lane / 16) + r, column lane % 16 of every instruction tile
    int* part = a.splits > 1 ? a.part + (size_t)split * M * N : nullptr;
    if constexpr (Q) {
        if (!part) {                                                 // uniform: quantize, stage through the free operand buffers, store
            unsigned* tile = reinterpret_cast<unsigned*>(&lds[0][0]);
            static_assert(BM * RqTile<BN>::P * 4 <= (int)sizeof(lds), "the codes of the tile fit the operand buffers");
            if constexpr (R) {
                // the residual's pieces: global -> the registers the operands have left -> LDS; ONE barrier later every lane reads
                // back the dwords it will write below, so the codes overwrite the residual's image
                rq_u4 res[RqPieces<BM, BN>::NPT];
                rq_fetch_tile<BM, BN>(a.r, m0, n0, M, N, res);
                rq_put_tile<BM, BN>(tile, a.r, res);
                __syncthreads();
            }
            unsigned cd[TM][TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                unsigned rd[TN];
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    cd[i][j] = 0u;
                    if constexpr (R) rd[j] = rq_unstage<BN>(tile, (wm * TM + i) * 16, (wn * TN + j) * 16, lane);
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int m = m0 + (wm * TM + i) * 16 + fc * 4 + r;
                    if (m >= M) continue;
                    const CcRow row = cc_row(m, a.e);
                    const RqRow qrow = rq_row(a.q, a.q.Cy == 1 ? 0 : m / a.e.OHW);
                    RqResRow rrow;
                    if constexpr (R) rrow = rq_res_row(a.r, a.r.Cr == 1 ? 0 : m / a.e.OHW);
#pragma unroll
                    for (int j = 0; j < TN; ++j) {
                        const int n = n0 + (wn * TN + j) * 16 + fr;
                        if (n >= N) continue;
                        float y = cc_finish(acc[i][j][r], row, n, a.e);
                        if constexpr (R) y = rq_add_res(y, (rd[j] >> (8 * r)) & 255u, rrow);
                        cd[i][j] |= rq_code(y, a.q, qrow) << (8 * r);
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j) rq_stage<BN>(tile, (wm * TM + i) * 16, (wn * TN + j) * 16, lane, cd[i][j]);
            __syncthreads();
            rq_store_tile<BM, BN>(tile, a.q, m0, n0, M, N);
            return;
        }
    }
#pragma unroll
    for (int i = 0; i < TM; ++i) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int m = m0 + (wm * TM + i) * 16 + fc * 4 + r;
            if (m >= M) continue;
            const CcRow row = part ? CcRow{} : cc_row(m, a.e);
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int n = n0 + (wn * TN + j) * 16 + fr;
                if (n >= N) continue;
                if (part) part[(size_t)m * N + n] = acc[i][j][r];
                else a.y[(size_t)m * N + n] = cc_finish(acc[i][j][r], row, n, a.e);
            }
        }
    }
}

// splits > 1: the sum of the partial tiles, then the tail of the one-split kernel
__global__ __launch_bounds__(TPB) void k_cc_epilogue(const int* __restrict__ part, int splits, long long MN, const CcEpi e, float* __restrict__ y) {
    const long long idx = (long long)blockIdx.x * TPB + threadIdx.x;
    if (idx >= MN) return;
    long long s = 0;
    for (int i = 0; i < splits; ++i) s += part[(size_t)i * MN + idx];
    y[idx] = cc_finish(s, cc_row((int)(idx / e.e.N), e), (int)(idx % e.e.N), e);
}

// ... to codes: thread idx owns dword idx of y, 4 (u8) or 8 (pack4) consecutive channels of one output pixel.  FR >= 0: the residual
// form (section 38) - the matching residual codes (rq_res_codes) and the residual row's table entry are read once per thread
template <int FY, int FR = -1>
__global__ __launch_bounds__(TPB) void k_cc_epilogue_q(const int* __restrict__ part, int splits, long long MN, const CcEpi e, const RqOut o, const RqRes s) {
    constexpr int CPD = FY == CNNQ_CODES_U8 ? 4 : 8;
    const long long idx = (long long)blockIdx.x * TPB + threadIdx.x;
    if (idx >= MN / CPD) return;
    const long long at = idx * CPD;
    const int m = (int)(at / e.e.N), n = (int)(at % e.e.N);
    const CcRow row = cc_row(m, e);
    const RqRow qrow = rq_row(o, o.Cy == 1 ? 0 : m / e.OHW);
    unsigned rc[2] = {0u, 0u};
    RqResRow rrow{};
    if constexpr (FR >= 0) {
        rq_res_codes<FY, FR>(s, idx, rc[0], rc[1]);
        rrow = rq_res_row(s, s.Cr == 1 ? 0 : m / e.OHW);
    }
    unsigned w = 0u;
#pragma unroll
    for (int c = 0; c < CPD; c += 4) {
        long long sum[4];
        rq_add_splits(part, splits, MN, at + c, sum);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float y = cc_finish(sum[k], row, n + c + k, e);
            if constexpr (FR >= 0) y = rq_add_res(y, (rc[c / 4] >> (8 * k)) & 255u, rrow);
            w |= rq_code(y, o, qrow) << ((c + k) * (32 / CPD));
        }
    }
    reinterpret_cast<unsigned*>(o.y)[idx] = w;
}

// ---- the workspace (host) -----------------------------------------------------------------------------------------------------------
// ws: int32 pix[N H W] | Rx[M] | rect[M] | taps[Cout][KH + 1][KW + 1] (not held by the caller) | part[splits][M][Cout] (splits > 1),
// each piece starting on 16 bytes
struct CcWs {
    int* pix;
    int* rx;
    unsigned* rect;
    int* taps;
    int* part;
    CcWs(void* ws, int64_t pixels, int64_t M, int64_t ntaps) {
        char* b = static_cast<char*>(ws);
        pix = reinterpret_cast<int*>(b);
        b += lc_align16(4 * (size_t)pixels);
        rx = reinterpret_cast<int*>(b);
        b += lc_align16(4 * (size_t)M);
        rect = reinterpret_cast<unsigned*>(b);
        b += lc_align16(4 * (size_t)M);
        taps = reinterpret_cast<int*>(b);
        part = reinterpret_cast<int*>(b + lc_align16(4 * (size_t)ntaps));
    }
    // ntaps: the table's entries, 0 when the caller holds it
    static size_t bytes(int64_t pixels, int64_t M, int64_t ntaps, int64_t Cout, int splits) {
        return lc_align16(4 * (size_t)pixels) + 2 * lc_align16(4 * (size_t)M) + lc_align16(4 * (size_t)ntaps) +
               (splits > 1 ? 4 * (size_t)splits * (size_t)M * (size_t)Cout : 0);
    }
};

}  // namespace
