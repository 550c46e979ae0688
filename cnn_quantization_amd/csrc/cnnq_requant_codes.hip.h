// cnnq_requant_codes.hip.h - the requantizing tail of the integer layers: the tiles of k_lc_gemm / k_cc_gemm
// (cnnq_linear_codes.hip.h, cnnq_conv_codes.hip.h) and the split-K epilogues store CODES - u8, or pack4 with the even column in the
// low nibble - instead of fp32, in the row-major / NHWC operand format the same two layers read, so that layers chain with nothing
// in between.  Part of the single translation unit cnnq_kernels.hip.
//
// The arithmetic.  y32 is what the fp32 kernels store (lc_finish / cc_finish, unchanged); relu: y32 > 0 ? y32 : 0; the code is
// qdq1's (cnnq_qdq.hip.h: the IEEE divide, a separately rounded + zp, two compare-selects, rintf) with the output table's (scale,
// zp, qmax) of the row - per tensor, or per sample / image - a NaN stored as 0, and the code limited to the format's largest (255 /
// 15): a foreign qmax never reaches the neighbouring nibble.  The bytes are those of the fp32 kernel, torch.relu_ and the stored
// format's quantizer (section 19) one after the other, for every tile, split count and held table.
//
// The tile's tail.  The 16 x 16 x 64 instruction leaves a lane column lane % 16 and rows 4 (lane / 16) + r, r = 0..3, of each
// instruction tile: the 16 bytes of one output row lie in 16 lanes.  Three steps bring them together:
//   registers: the lane quantizes its four rows of a column into the four bytes of ONE dword (byte r = row r); a row's table entry
//     is read once per row, before the row's columns.  The four lanes of a quad (columns 4q .. 4q + 3) then transpose their 4 x 4
//     bytes: four DPP quad broadcasts and three v_perm_b32, after which lane 4q + t holds row t, columns 4q .. 4q + 3 - four
//     neighbouring bytes of one output row.
//   LDS: after the k loop's last barrier the operand buffers are free; the codes of the BM x BN tile go there as bytes, row-major
//     with a pitch of BN + 16 bytes (128 x 128: 18 KB of the 32 KB), ONE ds_write_b32 per lane and instruction tile.  Banks: a
//     wave's write is rows R = 0..15 (4 (lane / 16) + t) x dword columns q = 0..3 at dword R P + q, P = BN / 4 + 4 = 36 or 20.
//     P / 4 is odd, so R P mod 64 runs through the sixteen multiples of 4 once, and with q all 64 banks are hit exactly once: no
//     conflict (an unpadded pitch of 32 dwords would put the sixteen rows on two bank groups, eight deep).  No sub-dword LDS
//     write is made.
//   global: one barrier, then thread p takes piece p of the tile - 16 output bytes of one row: 16 u8 codes (one ds_read_b128) or 32
//     pack4 codes (two) - and stores it with one 16-byte store where the output rows are whole 16-byte pieces on a 16-byte base
//     (`wide`), else dword by dword; N % 4 (u8) / N % 8 (pack4) makes every dword wholly inside or outside the row.  Neighbouring
//     threads store neighbouring pieces of one row (128 x 128 u8: eight threads a row's 128 bytes).  The padded pitch costs the
//     ds_read_b128 a two-deep conflict on four banks per sixteen lanes (a row's 32 dwords and the next row's, 36 on, overlap in
//     banks 0..3); the reads are a sixteenth of the tail's LDS instructions.  Rows beyond M and pieces beyond N are not stored.
//   pack4 is combined ON THE WAY OUT of LDS, not before it: the LDS image and its conflict-free dword writes are the same for both
//     formats (the format is a uniform run-time branch around the store loop only: no further instances of the tiles), and a
//     dword of four codes becomes two bytes by one shift-or, two dwords one by a v_perm_b32 - a quarter of an instruction per
//     code.  Combining in registers first would halve the LDS image but turn its writes into 16-bit ones, two lanes to a dword.
//     No byte of global memory is read back or written twice; no atomics.
//
// Split k: the int32 partial tiles are as they were; k_lc_epilogue_q / k_cc_epilogue_q (beside the fp32 epilogues) give a thread
// ONE dword of y - 4 u8 or 8 pack4 codes, consecutive n of one row: 16-byte loads of the partial tiles, the row's table entry once.
//
// The residual (the R instances of k_cc_gemm, k_cc_epilogue_q<FY, FR>): a second code operand of the output's
// shape, u8 or pack4 independently of the output, s32 = y32 + (float(code) - zr) * sr in three separately rounded fp32 operations
// before ReLU and the quantizer.  The store path run backwards: thread p loads piece p of the residual's tile (rq_fetch_pieces, one
// 16-byte load where the residual's own `wide` holds), pack4 is expanded to one code per byte on the way IN (rq_unpack8), the pieces
// go to the same LDS image (rq_put_pieces), and after one barrier a lane reads the dword it will later write (rq_unstage: rq_stage's
// address and the same quad transpose, which is its own inverse).  The output codes overwrite the residual's image in place.
#pragma once
#include "cnnq_common.hip.h"
#include "cnnq_qdq.hip.h"

namespace {

typedef unsigned rq_u4 __attribute__((ext_vector_type(4)));
typedef int rq_v4i __attribute__((ext_vector_type(4)));

// where the codes go; y == NULL: the fp32 kernels' launch
struct RqOut {
    unsigned char* y;     // [M][N] (u8) or [M][N / 2] (pack4), rows back to back, 4-byte aligned
    const float* qpy;     // [CNNQ_NQP][Cy]
    int Cy, fy, relu;     // fy: cnnq_code_format
    int wide;             // output rows of whole 16-byte pieces on a 16-byte base
};

// what the codes of one row share
struct RqRow {
    float scale, zp, qmax, top;
};
// idx: the row's entry of the table (its sample / image; anything when Cy == 1)
__device__ __forceinline__ RqRow rq_row(const RqOut& o, int idx) {
    const int c = o.Cy == 1 ? 0 : idx;
    return RqRow{o.qpy[CNNQ_QP_SCALE * (size_t)o.Cy + c], o.qpy[CNNQ_QP_ZP * (size_t)o.Cy + c], o.qpy[CNNQ_QP_QMAX * (size_t)o.Cy + c],
                 o.fy == CNNQ_CODES_U8 ? 255.f : 15.f};
}
__device__ __forceinline__ unsigned rq_code(float y, const RqOut& o, const RqRow& q) {
    if (o.relu) y = y > 0.f ? y : 0.f;
    float code;
    (void)qdq1(y, q.scale, q.zp, q.qmax, code);
    return code == code ? (unsigned)(code > q.top ? q.top : code) : 0u;
}

// the pitch of the tile's LDS image, in dwords
template <int BN>
struct RqTile {
    static constexpr int P = BN / 4 + 4;
};

// the 4 x 4 byte transpose of a quad: lane 4q + t gives byte j of its dword to lane 4q + j and holds byte t of each of the four
// afterwards, lane j's in byte j.  Its own inverse: "my column, rows 0..3" <-> "my row, columns 4q .. 4q + 3"
__device__ __forceinline__ unsigned rq_quad_transpose(unsigned cd, int lane) {
    const int t = lane & 3;
    // quad_perm broadcasts of the quad's lanes 0..3
    const unsigned d0 = (unsigned)__builtin_amdgcn_update_dpp(0, (int)cd, 0x00, 0xF, 0xF, false);
    const unsigned d1 = (unsigned)__builtin_amdgcn_update_dpp(0, (int)cd, 0x55, 0xF, 0xF, false);
    const unsigned d2 = (unsigned)__builtin_amdgcn_update_dpp(0, (int)cd, 0xAA, 0xF, 0xF, false);
    const unsigned d3 = (unsigned)__builtin_amdgcn_update_dpp(0, (int)cd, 0xFF, 0xF, 0xF, false);
    // v_perm_b32: selector bytes 0..3 take the second source's bytes, 4..7 the first's.  Byte t of each of the four
    const unsigned sel = 0x0C0C0400u + (unsigned)t * 0x0101u;
    const unsigned p01 = __builtin_amdgcn_perm(d1, d0, sel), p23 = __builtin_amdgcn_perm(d3, d2, sel);
    return __builtin_amdgcn_perm(p23, p01, 0x05040100u);
}
// the lane's dword of the instruction tile at (row0, col0) of the macro tile: the four bytes (row0 + 4 (lane / 16) + lane % 4,
// col0 + 4 (lane % 16 / 4) ..) of the LDS image - written by rq_stage, read by rq_unstage
template <int BN>
__device__ __forceinline__ int rq_lane_dword(int row0, int col0, int lane) {
    return (row0 + (lane >> 4) * 4 + (lane & 3)) * RqTile<BN>::P + (col0 >> 2) + ((lane >> 2) & 3);
}
// cd: the lane's codes of rows 4 (lane / 16) + r (byte r) of column lane % 16 of the instruction tile -> transposed within the
// quad and written as the lane's dword
template <int BN>
__device__ __forceinline__ void rq_stage(unsigned* __restrict__ tile, int row0, int col0, int lane, unsigned cd) {
    tile[rq_lane_dword<BN>(row0, col0, lane)] = rq_quad_transpose(cd, lane);
}
// the other direction (section 38): the lane's dword of the image -> the codes of rows 4 (lane / 16) + r (byte r) of column lane % 16
template <int BN>
__device__ __forceinline__ unsigned rq_unstage(const unsigned* __restrict__ tile, int row0, int col0, int lane) {
    return rq_quad_transpose(tile[rq_lane_dword<BN>(row0, col0, lane)], lane);
}

// eight codes of 0..15, one per byte of a, b -> the dword of pack4, the first code in the lowest nibble
__device__ __forceinline__ unsigned rq_pack8(unsigned a, unsigned b) {
    return __builtin_amdgcn_perm(b | (b >> 4), a | (a >> 4), 0x06040200u);
}

// the tile's LDS image -> y: pieces of 16 output bytes, piece p to thread p % TPB
template <int BM, int BN, int FY>
__device__ __forceinline__ void rq_store_pieces(const unsigned* __restrict__ tile, const RqOut& o, int m0, int n0, int M, int N) {
    constexpr int CPD = FY == CNNQ_CODES_U8 ? 4 : 8;      // codes per output dword
    constexpr int CPP = 4 * CPD;                          // codes per piece
    constexpr int PPR = BN / CPP, NP = BM * PPR;
    const size_t rowdw = (size_t)(N / CPD);
    for (int p = threadIdx.x; p < NP; p += TPB) {
        const int r = p / PPR, pc = p % PPR, m = m0 + r, n = n0 + pc * CPP;
        if (m >= M || n >= N) continue;
        const rq_u4* src = reinterpret_cast<const rq_u4*>(tile + r * RqTile<BN>::P) + pc * (CPP / 16);
        rq_u4 v = src[0];
        if constexpr (FY == CNNQ_CODES_PACK4) {
            const rq_u4 w = src[1];
            v = rq_u4{rq_pack8(v.x, v.y), rq_pack8(v.z, v.w), rq_pack8(w.x, w.y), rq_pack8(w.z, w.w)};
        }
        unsigned* dst = reinterpret_cast<unsigned*>(o.y) + (size_t)m * rowdw + n / CPD;
        if (o.wide && n + CPP <= N) {
            *reinterpret_cast<rq_u4*>(dst) = v;
        } else {
#pragma unroll
            for (int d = 0; d < 4; ++d)
                if (n + d * CPD < N) dst[d] = v[d];
        }
    }
}
// behind the barrier that follows the last rq_stage
template <int BM, int BN>
__device__ __forceinline__ void rq_store_tile(const unsigned* __restrict__ tile, const RqOut& o, int m0, int n0, int M, int N) {
    if (o.fy == CNNQ_CODES_U8) rq_store_pieces<BM, BN, CNNQ_CODES_U8>(tile, o, m0, n0, M, N);
    else rq_store_pieces<BM, BN, CNNQ_CODES_PACK4>(tile, o, m0, n0, M, N);
}

// ---- the residual operand (section 38): codes of the output's shape, decoded and added before ReLU and the quantizer ----------------
// rq == NULL: none
struct RqRes {
    const unsigned char* rq;   // [M][N] (u8) or [M][N / 2] (pack4), rows back to back, 4-byte aligned; may be the output itself (same format)
    const float* qpr;          // [CNNQ_NQP][Cr]
    int Cr, fr;                // fr: cnnq_code_format
    int wide;                  // residual rows of whole 16-byte pieces on a 16-byte base
};
struct RqResRow {
    float scale, zp;
};
__device__ __forceinline__ RqResRow rq_res_row(const RqRes& s, int idx) {
    const int c = s.Cr == 1 ? 0 : idx;
    return RqResRow{s.qpr[CNNQ_QP_SCALE * (size_t)s.Cr + c], s.qpr[CNNQ_QP_ZP * (size_t)s.Cr + c]};
}
// y32 + the decoded code: the subtraction, the product and the sum each rounded to fp32 (-ffp-contract=off; the product is an
// operand of the sum, never fused into it)
__device__ __forceinline__ float rq_add_res(float y, unsigned code, const RqResRow& q) {
    const float r = ((float)code - q.zp) * q.scale;
    return y + r;
}

// the dword of pack4 -> eight codes, one per byte, the first in the lowest byte of a: rq_pack8's inverse
__device__ __forceinline__ void rq_unpack8(unsigned v, unsigned& a, unsigned& b) {
    const unsigned lo = v & 0x0F0F0F0Fu, hi = (v >> 4) & 0x0F0F0F0Fu;
    a = __builtin_amdgcn_perm(hi, lo, 0x05010400u);
    b = __builtin_amdgcn_perm(hi, lo, 0x07030602u);
}

// pieces per thread of a BM x BN tile: the u8 count (pack4 has half as many)
template <int BM, int BN>
struct RqPieces {
    static constexpr int NPT = (BM * BN / 16 + TPB - 1) / TPB;
};

// global -> registers: piece p of the tile - 16 residual bytes of one output row, rq_store_pieces' map with the residual's format -
// to thread p % TPB; one 16-byte load where `wide`, else dword by dword.  Rows beyond M and pieces beyond N are not loaded
template <int BM, int BN, int FR>
__device__ __forceinline__ void rq_fetch_pieces(const RqRes& s, int m0, int n0, int M, int N, rq_u4 (&v)[RqPieces<BM, BN>::NPT]) {
    constexpr int CPD = FR == CNNQ_CODES_U8 ? 4 : 8, CPP = 4 * CPD;
    constexpr int PPR = BN / CPP, NP = BM * PPR;
    const size_t rowdw = (size_t)(N / CPD);
#pragma unroll
    for (int i = 0; i < (NP + TPB - 1) / TPB; ++i) {
        const int p = threadIdx.x + i * TPB;
        const int r = p / PPR, pc = p % PPR, m = m0 + r, n = n0 + pc * CPP;
        v[i] = rq_u4{0u, 0u, 0u, 0u};
        if ((NP % TPB && p >= NP) || m >= M || n >= N) continue;
        const unsigned* src = reinterpret_cast<const unsigned*>(s.rq) + (size_t)m * rowdw + n / CPD;
        if (s.wide && n + CPP <= N) {
            v[i] = *reinterpret_cast<const rq_u4*>(src);
        } else {
#pragma unroll
            for (int d = 0; d < 4; ++d)
                if (n + d * CPD < N) v[i][d] = src[d];
        }
    }
}
// registers -> the tile's LDS image, one code per byte in both formats (pack4 expanded on the way in)
template <int BM, int BN, int FR>
__device__ __forceinline__ void rq_put_pieces(unsigned* __restrict__ tile, const rq_u4 (&v)[RqPieces<BM, BN>::NPT]) {
    constexpr int CPP = FR == CNNQ_CODES_U8 ? 16 : 32;
    constexpr int PPR = BN / CPP, NP = BM * PPR;
#pragma unroll
    for (int i = 0; i < (NP + TPB - 1) / TPB; ++i) {
        const int p = threadIdx.x + i * TPB;
        if (NP % TPB && p >= NP) continue;
        rq_u4* dst = reinterpret_cast<rq_u4*>(tile + (p / PPR) * RqTile<BN>::P) + (p % PPR) * (CPP / 16);
        if constexpr (FR == CNNQ_CODES_U8) {
            dst[0] = v[i];
        } else {
            unsigned c[8];
#pragma unroll
            for (int d = 0; d < 4; ++d) rq_unpack8(v[i][d], c[2 * d], c[2 * d + 1]);
            dst[0] = rq_u4{c[0], c[1], c[2], c[3]};
            dst[1] = rq_u4{c[4], c[5], c[6], c[7]};
        }
    }
}
template <int BM, int BN>
__device__ __forceinline__ void rq_fetch_tile(const RqRes& s, int m0, int n0, int M, int N, rq_u4 (&v)[RqPieces<BM, BN>::NPT]) {
    if (s.fr == CNNQ_CODES_U8) rq_fetch_pieces<BM, BN, CNNQ_CODES_U8>(s, m0, n0, M, N, v);
    else rq_fetch_pieces<BM, BN, CNNQ_CODES_PACK4>(s, m0, n0, M, N, v);
}
template <int BM, int BN>
__device__ __forceinline__ void rq_put_tile(unsigned* __restrict__ tile, const RqRes& s, const rq_u4 (&v)[RqPieces<BM, BN>::NPT]) {
    if (s.fr == CNNQ_CODES_U8) rq_put_pieces<BM, BN, CNNQ_CODES_U8>(tile, v);
    else rq_put_pieces<BM, BN, CNNQ_CODES_PACK4>(tile, v);
}

// split k: the residual codes that match thread idx's dword of y - CPD codes from element `at` of row-major [M][N], one per byte of
// a (and b: the second four of a pack4 output).  u8 -> u8 and pack4 -> pack4: the dword idx; u8 -> pack4: dwords 2 idx, 2 idx + 1;
// pack4 -> u8: the thread's OWN half of dword idx / 2 as one 16-bit load - no byte is loaded by two threads
template <int FY, int FR>
__device__ __forceinline__ void rq_res_codes(const RqRes& s, long long idx, unsigned& a, unsigned& b) {
    const unsigned* src = reinterpret_cast<const unsigned*>(s.rq);
    b = 0u;
    if constexpr (FY == FR) {
        const unsigned v = src[idx];
        if constexpr (FR == CNNQ_CODES_U8) a = v;
        else rq_unpack8(v, a, b);
    } else if constexpr (FR == CNNQ_CODES_U8) {
        a = src[2 * idx];
        b = src[2 * idx + 1];
    } else {
        unsigned bb;
        rq_unpack8(reinterpret_cast<const unsigned short*>(s.rq)[idx], a, bb);
    }
}

// split k: the sums of four consecutive elements' partial tiles (at % 4 == 0, MN % 4 == 0: 16-byte loads)
__device__ __forceinline__ void rq_add_splits(const int* __restrict__ part, int splits, long long MN, long long at, long long (&s)[4]) {
    s[0] = s[1] = s[2] = s[3] = 0;
    for (int i = 0; i < splits; ++i) {
        const rq_v4i v = *reinterpret_cast<const rq_v4i*>(part + (size_t)i * MN + at);
        s[0] += v.x; s[1] += v.y; s[2] += v.z; s[3] += v.w;
    }
}

}  // namespace
