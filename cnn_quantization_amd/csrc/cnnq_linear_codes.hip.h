// cnnq_linear_codes.hip.h - the integer linear layer on the stored codes: y[M][N] from activation codes
// xq[M][K] and weight codes wq[N][K], each one byte per code (u8) or two codes per byte (pack4), without ever expanding them to
// floats.  The only contraction of the library, hence its only matrix instructions: v_mfma_i32_16x16x64_i8.
// Part of the single translation unit cnnq_kernels.hip.
//
// The arithmetic.  Neither operand's scale nor zero point varies along k (activations per tensor or per sample, weights per output
// channel), so
//     sum_k ((xq - zx) sx) ((wq - zw) sw) = sx sw (S - zw Rx - zx Rw + K zx zw),   S = sum_k xq wq, Rx = sum_k xq, Rw = sum_k wq
// with S, Rx, Rw exact integers.  The matrix instruction multiplies SIGNED bytes: a u8 code c enters as c ^ 0x80 = c - 128, a pack4
// code (0..15) as it is; the kernel accumulates S' = sum_k (xq - ox)(wq - ow) with ox, ow = 128 or 0 and lc_finish returns to
// S = S' + ow Rx + ox Rw - K ox ow in 64-bit integers before the one fp64 combination, so the re-centring costs no rounding.
//
// Three kernels:
//   k_lc_rowsums   Rx and Rw: one wave per row, one read of the codes, v_sad_u8 on whole dwords (four codes, or twice four nibbles,
//                  per instruction).  A kernel of its own, not a by-product of the GEMM tiles: a row of xq passes through the LDS of
//                  every column tile and every split, so sums taken there are taken ceil(N / BN) x splits times over and need a
//                  slot per split in the workspace; and Rw depends on the weights alone - a caller holds it once per layer
//                  (cnnq_linear_codes_rowsums) and the launch then walks the M activation rows only.
//   k_lc_gemm      the tiles of S' (below); with one split its tail is the epilogue.
//   k_lc_epilogue  splits > 1: adds the splits' int32 partial tiles (integer addition: the same bits for every split count), then
//                  the same lc_finish.
// The Q instances of k_lc_gemm and k_lc_epilogue_q store codes instead of fp32 - ReLU and the output table's quantizer behind the same
// lc_finish: cnnq_requant_codes.hip.h.
//
// k_lc_gemm.  A workgroup of four waves (WM x WN) owns a BM x BN macro tile of y and one split of the k range; a wave owns TM x TN
// instruction tiles of 16 x 16 whose int32 accumulators (four per lane and tile) stay in registers over all its k steps.  A step is
// 64 codes of k - one instruction deep: a lane's operand of v_mfma_i32_16x16x64_i8 is 16 consecutive k bytes of one row (row =
// lane % 16, bytes 16 (lane / 16) ..), i.e. ONE 16-byte LDS read, and the lane's four results are rows 4 (lane / 16) + r of column
// lane % 16.
//   global -> registers: the step's BM + BN rows of 64 codes are cut into chunks of 16 codes (16 B of u8, 8 B of pack4), chunk c of
//     an operand to thread c % 256: four neighbouring threads read one row's 64 (32) contiguous bytes.  Rows of whole 16-byte
//     pieces (K % 16 == 0 and bases aligned: V16) take one dwordx4 (dwordx2) load per chunk, everything else a dword at a time -
//     K % 4 (u8) / K % 8 (pack4) makes every dword wholly inside or outside the row.  Rows beyond M / N and dwords beyond K are
//     not loaded: they become the code whose signed form is zero (0x80 / 0) and add nothing to S'.
//   registers -> LDS: the raw dwords stay in registers while the step before is multiplied (pack4: half the registers of the
//     expanded form) and are turned into signed bytes on the way into LDS - u8: one XOR per dword; pack4: two masks and, when the
//     other operand is u8, two v_perm_b32 that interleave the even and odd nibbles back into k order.  When BOTH operands are pack4
//     the permutes are left out: both sides then present k in the order even codes, odd codes of each dword, and a sum over k does
//     not care.
//   LDS: per buffer (BM + BN) rows x 64 B, no padding; the 16-byte chunk kc of row r lives at chunk kc ^ ((r >> 2) & 3).  The
//     instruction's read - 16 lanes of one chunk index over rows r .. r + 15 - then touches bank group 16 (r & 3) + 4 (kc ^ (r >> 2)):
//     sixteen different groups of four banks, all 64 banks once; the writes of 16 neighbouring threads are 4 whole rows, 256
//     contiguous bytes.  Two buffers: the loads of step i + 1 are issued before the multiplications of step i and land in the other
//     buffer after them, one barrier per step.
//   tail: splits == 1 - lc_finish per element and a plain store; else the int32 tile to part[split][M][N], plain stores, every
//     element of every split written (a split without steps writes zeros): no initialisation, no atomics.
#pragma once
#include "cnnq_common.hip.h"
#include "cnnq_requant_codes.hip.h"

namespace {

constexpr int LC_BK = 64;            // codes of k per step: one v_mfma_i32_16x16x64_i8 deep
constexpr int LC_MAX_SPLITS = 64;
constexpr int LC_MAX_K = 131071;     // K * 128 * 128 < 2^31

typedef int lc_v4i __attribute__((ext_vector_type(4)));

// what the tail of every element needs
struct LcEpi {
    const float* qpx;     // [CNNQ_NQP][Cx]
    const float* qpw;     // [CNNQ_NQP][N]
    const float* bias;    // [N] or NULL
    const int* rx;        // [M] raw code sums
    const int* rw;        // [N]
    int Cx, N, K, ox, ow; // ox, ow: what the signed form of a code subtracted (128: u8, 0: pack4)
};

struct LcArgs {
    const unsigned char* xq;
    const unsigned char* wq;
    float* y;
    int* part;            // [splits][M][N], splits > 1
    int M, tilesM, tilesN, splits;
    LcEpi e;
    RqOut q;              // Q instances: the codes' destination instead of y (cnnq_requant_codes.hip.h)
};

// S' (signed-domain sum of products) of element (m, n) -> y: exact integers, one fp64 combination, one rounding to fp32
// (lc_combine: the same with the element's code sums rx, rw, its count of codes K and its row mp of qpx given - the convolution of
// cnnq_conv_codes.hip.h, whose sums run over an output pixel's valid taps, finishes through it too)
__device__ __forceinline__ float lc_combine(long long sp, long long rx, long long rw, long long K, int mp, int n, const LcEpi& e) {
    const long long s = sp + e.ow * rx + e.ox * rw - K * e.ox * e.ow;
    const double sx = e.qpx[CNNQ_QP_SCALE * (size_t)e.Cx + mp], zx = e.qpx[CNNQ_QP_ZP * (size_t)e.Cx + mp];
    const double sw = e.qpw[CNNQ_QP_SCALE * (size_t)e.N + n], zw = e.qpw[CNNQ_QP_ZP * (size_t)e.N + n];
    const double t = (double)s - zw * (double)rx - zx * (double)rw + (double)K * (zx * zw);
    double v = (sx * sw) * t;
    if (e.bias) v += (double)e.bias[n];
    return (float)v;
}
__device__ __forceinline__ float lc_finish(long long sp, int m, int n, const LcEpi& e) {
    return lc_combine(sp, e.rx[m], e.rw[n], e.K, e.Cx == 1 ? 0 : m, n, e);
}

// ---- row sums ---------------------------------------------------------------------------------------------------------------
// rows [0, M) are xq's, rows [M, M + Nw) are wq's (Nw == 0: the caller holds Rw); one wave per row, lanes stride over its dwords
__global__ __launch_bounds__(TPB) void k_lc_rowsums(const unsigned char* __restrict__ xq, int fx, int M, const unsigned char* __restrict__ wq, int fw,
                                                    int Nw, int K, int* __restrict__ rx, int* __restrict__ rw) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * (TPB / 64) + (threadIdx.x >> 6);
    if (r >= (long long)M + Nw) return;
    const bool isx = r < M;
    const long long row = isx ? r : r - M;
    const int fmt = isx ? fx : fw;
    const int ndw = fmt == CNNQ_CODES_U8 ? K / 4 : K / 8;
    const unsigned* p = reinterpret_cast<const unsigned*>(isx ? xq : wq) + row * ndw;
    unsigned acc = 0;
    if (fmt == CNNQ_CODES_U8) {
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
    if (lane == 0) (isx ? rx : rw)[row] = s;
}

// ---- the operand path: global -> registers -> LDS ---------------------------------------------------------------------------------
// the raw dwords of one chunk of 16 codes
template <int FMT>
struct LcRaw {
    static constexpr int ND = FMT == CNNQ_CODES_U8 ? 4 : 2;   // dwords per chunk
    static constexpr int CPD = 16 / ND;                       // codes per dword
    static constexpr unsigned FILL = FMT == CNNQ_CODES_U8 ? 0x80808080u : 0u;   // the codes whose signed form is zero
    unsigned d[ND];
};

typedef unsigned lc_u4 __attribute__((ext_vector_type(4)));
typedef unsigned lc_u2 __attribute__((ext_vector_type(2)));

// chunk of codes [k, k + 16) of row `row` of codes[rows][K]; k % 16 == 0.  Nothing outside the matrix is read.
template <int FMT, bool V16>
__device__ __forceinline__ void lc_fetch(const unsigned char* __restrict__ codes, int rows, int K, int row, int k, LcRaw<FMT>& r) {
    constexpr int ND = LcRaw<FMT>::ND, CPD = LcRaw<FMT>::CPD;
    const bool rowok = row < rows;
    const unsigned* q = reinterpret_cast<const unsigned*>(codes) + ((long long)row * K + k) / CPD;
    if constexpr (V16) {                 // K % 16 == 0: the chunk is wholly inside or outside
        if (rowok && k < K) {
            if constexpr (ND == 4) {
                const lc_u4 v = *reinterpret_cast<const lc_u4*>(q);
                r.d[0] = v.x; r.d[1] = v.y; r.d[2] = v.z; r.d[3] = v.w;
            } else {
                const lc_u2 v = *reinterpret_cast<const lc_u2*>(q);
                r.d[0] = v.x; r.d[1] = v.y;
            }
        } else {
#pragma unroll
            for (int i = 0; i < ND; ++i) r.d[i] = LcRaw<FMT>::FILL;
        }
    } else {
#pragma unroll
        for (int i = 0; i < ND; ++i) r.d[i] = (rowok && k + i * CPD < K) ? q[i] : LcRaw<FMT>::FILL;
    }
}

// raw dwords -> the 16 signed bytes the instruction reads.  NATURAL: pack4 nibbles back in k order (the other operand is u8)
template <int FMT, bool NATURAL>
__device__ __forceinline__ lc_u4 lc_signed(const LcRaw<FMT>& r) {
    lc_u4 o;
    if constexpr (FMT == CNNQ_CODES_U8) {
        o.x = r.d[0] ^ 0x80808080u; o.y = r.d[1] ^ 0x80808080u; o.z = r.d[2] ^ 0x80808080u; o.w = r.d[3] ^ 0x80808080u;
    } else {
        const unsigned l0 = r.d[0] & 0x0F0F0F0Fu, h0 = (r.d[0] >> 4) & 0x0F0F0F0Fu;   // codes 0 2 4 6 / 1 3 5 7 of the dword
        const unsigned l1 = r.d[1] & 0x0F0F0F0Fu, h1 = (r.d[1] >> 4) & 0x0F0F0F0Fu;
        if constexpr (NATURAL) {         // v_perm_b32: selector bytes 0..3 take the second source's bytes, 4..7 the first's
            o.x = __builtin_amdgcn_perm(h0, l0, 0x05010400u); o.y = __builtin_amdgcn_perm(h0, l0, 0x07030602u);
            o.z = __builtin_amdgcn_perm(h1, l1, 0x05010400u); o.w = __builtin_amdgcn_perm(h1, l1, 0x07030602u);
        } else {
            o.x = l0; o.y = h0; o.z = l1; o.w = h1;
        }
    }
    return o;
}

// the LDS slot (in 16-byte units) of chunk kc of row r of an operand's tile
__device__ __forceinline__ int lc_slot(int r, int kc) { return r * 4 + (kc ^ ((r >> 2) & 3)); }

// ---- the tiles ------------------------------------------------------------------------------------------------------------------
// Q: with one split the tail stores codes (a.q) instead of fp32 (a.y): section 37
template <int WM, int WN, int TM, int TN, int FX, int FW, bool V16, bool Q = false>
__global__ __launch_bounds__(TPB) void k_lc_gemm(const LcArgs a) {
    static_assert(WM * WN == TPB / 64, "four waves");
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
    const int M = a.M, N = a.e.N, K = a.e.K;
    const int steps = (K + LC_BK - 1) / LC_BK;
    const int s0 = (int)((long long)split * steps / a.splits), s1 = (int)((long long)(split + 1) * steps / a.splits);

    LcRaw<FX> ra[NA];
    LcRaw<FW> rb[NB];
    auto fetch = [&](int step) {
        const int k0 = step * LC_BK;
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            const int c = tid + i * TPB;
            if (CA % TPB == 0 || c < CA) lc_fetch<FX, V16>(a.xq, M, K, m0 + (c >> 2), k0 + (c & 3) * 16, ra[i]);
        }
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
            unsigned cd[TM][TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) {
#pragma unroll
                for (int j = 0; j < TN; ++j) cd[i][j] = 0u;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int m = m0 + (wm * TM + i) * 16 + fc * 4 + r;
                    if (m >= M) continue;
                    const RqRow row = rq_row(a.q, m);
#pragma unroll
                    for (int j = 0; j < TN; ++j) {
                        const int n = n0 + (wn * TN + j) * 16 + fr;
                        if (n < N) cd[i][j] |= rq_code(lc_finish(acc[i][j][r], m, n, a.e), a.q, row) << (8 * r);
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
    for (int j = 0; j < TN; ++j) {
        const int n = n0 + (wn * TN + j) * 16 + fr;
        if (n >= N) continue;
#pragma unroll
        for (int i = 0; i < TM; ++i) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + (wm * TM + i) * 16 + fc * 4 + r;
                if (m >= M) continue;
                if (part) part[(size_t)m * N + n] = acc[i][j][r];
                else a.y[(size_t)m * N + n] = lc_finish(acc[i][j][r], m, n, a.e);
            }
        }
    }
}

// splits > 1: the sum of the partial tiles, then the tail of the one-split kernel
__global__ __launch_bounds__(TPB) void k_lc_epilogue(const int* __restrict__ part, int splits, long long MN, const LcEpi e, float* __restrict__ y) {
    const long long idx = (long long)blockIdx.x * TPB + threadIdx.x;
    if (idx >= MN) return;
    long long s = 0;
    for (int i = 0; i < splits; ++i) s += part[(size_t)i * MN + idx];
    y[idx] = lc_finish(s, (int)(idx / e.N), (int)(idx % e.N), e);
}

// ... to codes: thread idx owns dword idx of y, 4 (u8) or 8 (pack4) consecutive n of one row
template <int FY>
__global__ __launch_bounds__(TPB) void k_lc_epilogue_q(const int* __restrict__ part, int splits, long long MN, const LcEpi e, const RqOut o) {
    constexpr int CPD = FY == CNNQ_CODES_U8 ? 4 : 8;
    const long long idx = (long long)blockIdx.x * TPB + threadIdx.x;
    if (idx >= MN / CPD) return;
    const long long at = idx * CPD;
    const int m = (int)(at / e.N), n = (int)(at % e.N);
    const RqRow row = rq_row(o, m);
    unsigned w = 0u;
#pragma unroll
    for (int c = 0; c < CPD; c += 4) {
        long long s[4];
        rq_add_splits(part, splits, MN, at + c, s);
#pragma unroll
        for (int k = 0; k < 4; ++k) w |= rq_code(lc_finish(s[k], m, n + c + k, e), o, row) << ((c + k) * (32 / CPD));
    }
    reinterpret_cast<unsigned*>(o.y)[idx] = w;
}

// ---- the plan (host) ----------------------------------------------------------------------------------------------------------------
// Macro tiles: 16 x 128 (waves 1 x 4, tiles 1 x 2 each) for batches of up to 16 rows - they pay for 16, not 128; 64 x 64 (2 x 2
// waves of 2 x 2); 128 x 128 (2 x 2 waves of 4 x 4: 8 LDS reads per 16 instructions).  The 64 x 64 tile takes M <= 64 and the
// outputs of which the 128 x 128 tile makes fewer tiles than half the chip has CUs while 64 x 64 makes at least that many (512 x
// 1000: 32 against 128) - splitting k eight ways instead would write and re-read eight int32 copies of y.
// Splits: as many as bring the launch to LC_WG_TARGET workgroups (the 16-row tile, whose workgroups keep 9 KB in flight each
// against 16 KB and whose launches are bound by the weight read, to four times that), at least LC_MIN_STEPS steps per split.
constexpr int LC_CUS = 256;
constexpr int LC_MIN_STEPS = 4;

struct LcPlan {
    int tile;       // 0: 16 x 128, 1: 64 x 64, 2: 128 x 128
    int BM, BN, tilesM, tilesN, steps, splits;
};

inline LcPlan lc_plan(int64_t M, int64_t N, int64_t K, int splits) {
    LcPlan p;
    const int64_t t128 = ((M + 127) / 128) * ((N + 127) / 128), t64 = ((M + 63) / 64) * ((N + 63) / 64);
    p.tile = M <= 16 ? 0 : (M <= 64 || (t128 < LC_CUS / 2 && t64 >= LC_CUS / 2)) ? 1 : 2;
    p.BM = p.tile == 0 ? 16 : p.tile == 1 ? 64 : 128;
    p.BN = p.tile == 1 ? 64 : 128;
    p.tilesM = (int)((M + p.BM - 1) / p.BM);
    p.tilesN = (int)((N + p.BN - 1) / p.BN);
    p.steps = (int)((K + LC_BK - 1) / LC_BK);
    if (splits <= 0) {
        const int64_t tiles = (int64_t)p.tilesM * p.tilesN, target = p.tile == 0 ? 4 * LC_CUS : LC_CUS;
        int64_t s = target / tiles;
        if (s > p.steps / LC_MIN_STEPS) s = p.steps / LC_MIN_STEPS;
        splits = (int)(s < 1 ? 1 : s > LC_MAX_SPLITS ? LC_MAX_SPLITS : s);
    }
    p.splits = splits;
    return p;
}

inline size_t lc_align16(size_t b) { return (b + 15) & ~(size_t)15; }

// ws: int32 rx[M] | int32 rw[N] | int32 part[splits][M][N] (splits > 1), each piece starting on 16 bytes
struct LcWs {
    int* rx;
    int* rw;
    int* part;
    LcWs(void* ws, int64_t M, int64_t N) {
        char* b = static_cast<char*>(ws);
        rx = reinterpret_cast<int*>(b);
        rw = reinterpret_cast<int*>(b + lc_align16(4 * (size_t)M));
        part = reinterpret_cast<int*>(b + lc_align16(4 * (size_t)M) + lc_align16(4 * (size_t)N));
    }
    static size_t bytes(int64_t M, int64_t N, int splits) {
        return lc_align16(4 * (size_t)M) + lc_align16(4 * (size_t)N) + (splits > 1 ? 4 * (size_t)splits * (size_t)M * (size_t)N : 0);
    }
};

}  // namespace
