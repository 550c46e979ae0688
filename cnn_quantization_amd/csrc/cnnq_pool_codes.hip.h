// cnnq_pool_codes.hip.h - pooling on the stored NHWC codes: the window maximum (k_mp_codes) and the global
// average (k_ap_codes) of u8 / pack4 codes as cnnq_conv_codes reads and cnnq_conv_codes_q writes them, so that a network stays on
// codes from the stem's output to the classifier.  Both are exact on integers.  Part of the single translation unit cnnq_kernels.hip.
//
// Packed lanes.  gfx950 has no packed byte maximum or sum that runs DOWN a column of bytes (v_sad_u8 sums ALONG a dword); it has
// v_pk_max_u16 and v_pk_add_u16.  A dword of codes is split into NS dwords of two 16-bit lanes, one code per lane (PcSplit):
//   u8:    (x >> 8 k) & 0x00ff00ff, k = 0, 1     lane 0: byte k,   lane 1: byte k + 2
//   pack4: (x >> 4 k) & 0x000f000f, k = 0..3     lane 0: nibble k, lane 1: nibble k + 4
// - in both formats half an instruction per code and tap.  The running maximum / sum stays in split form over all taps / pixels
// and is joined (shift-or) once on the way out.
//
// The maximum (k_mp_codes).  The decode (code - zp) * scale with scale > 0 does not decrease in the code, so the maximum of the codes
// IS the code of the maximum: no table is read, the output keeps the input's table.  A padded position is -inf to max_pool2d; code 0
// is the identity of an unsigned maximum, so padding is loaded as code 0 - exact, and with padding <= kernel / 2 every window holds a
// real element anyway.  A workgroup owns TOH x TOW output pixels of one image times a slab of SD channel dwords and runs three phases:
//   1. the input patch ((TOH - 1) sh + KH) x ((TOW - 1) sw + KW) pixels x SD dwords: global -> LDS, every input byte of the patch read
//      once (16-byte loads where a pixel's channel bytes are whole 16-byte pieces on a 16-byte base - VD = 4 - else dword by dword);
//   2. across the row: item (ow, patch row, dword) = the maximum over kw, written to a second LDS image rm[ow][patch row][dword];
//   3. down the column: item (oh, ow, dword) = the maximum over kh of rm, stored (16-byte stores with VD = 4, else dwords).
// Banks (64 banks of 4 bytes; SD = 16 dwords, the stem's u8 slab): the patch is [row][pixel][dword] with the row pitch PWp SD, PWp
// = the patch width made ODD.  Phase 1 writes consecutive items to consecutive addresses inside a row: conflict-free.  Phase 2's
// items run dword-fastest, then patch row: a wave of dword items is 16 dwords x 4 rows at (row PWp 16 + dword) - PWp odd puts the
// four rows on the four distinct multiples of 16 mod 64: all 64 banks once (ordering by output column instead would stride sw SD = 32
// dwords at stride 2, two deep).  It writes rm at the item's own index: consecutive.  rm's pitch per output column is PHp SD, PHp =
// the patch height made odd, and phase 3 runs dword-fastest, then output column: again four odd multiples of 16.  With VD = 4 the same
// holds per 16 lanes of a ds_read_b128 (4 pieces x 4 rows = 64 consecutive-or-odd-pitched dwords).  Slabs of 8 / 4 dwords put 8 / 16
// rows of odd pitch in a wave the same way; a slab that is no power of two can be two deep.
//
// The global average (k_ap_codes).  S[n][c] = the exact integer sum of the H W codes; y32 = (float)(((double)S / HW - (double)zx) *
// (double)sx), fp64 operations in that order (-ffp-contract=off), one rounding to fp32; the Q instances then call rq_code
// (cnnq_requant_codes.hip.h) with the output row's table.  A workgroup owns one image and a slab of AP_SD = 16 channel dwords; thread
// (g, col) sums pixels g, g + G, .. of column col (VD dwords) on packed 16-bit lanes and widens to int32 before a lane can overflow:
// 257 * 255 < 65536, so every AP_WIDEN = 257 pixels of its own.  The partial sums meet in LDS as int32 part[g][channel of the slab]
// with a pitch of (channels + 4) ints: a thread's ds_write_b128 of four channels lands at g (16 cols + 4) + 16 col + .., and per 16
// lanes (4 cols x 4 groups with 16-byte loads) the 4 g + 16 col are sixteen distinct multiples of 4: conflict-free (an unpadded
// pitch of 64 would put the four groups on the same banks).  After ONE barrier a thread per output dword - 4 u8 or 8 pack4 codes,
// or four floats - adds the G partial sums of its channels (ds_read_b128 of consecutive threads: consecutive), finishes and stores
// a dword / 16 bytes.  One launch, no workspace, no atomics.
#pragma once
#include "cnnq_common.hip.h"
#include "cnnq_requant_codes.hip.h"

namespace {

typedef unsigned short pc_us2 __attribute__((ext_vector_type(2)));

constexpr int MP_LDS_DW = 10240;     // k_mp_codes' patch and row maxima: 40 KB, four workgroups per CU
constexpr int MP_TILE = 8;           // output pixels per tile and axis before the patch is fitted to the LDS
constexpr int MP_SD = 16;            // channel dwords per slab: 64 u8 / 128 pack4 channels
constexpr int AP_SD = 16;
constexpr int AP_WIDEN = 257;        // pixels a 16-bit lane holds: 257 * 255 = 65535

// VD dwords at p: one 16-byte access (p 16-byte aligned) or one dword
template <int VD>
__device__ __forceinline__ void pc_ld(const unsigned* p, unsigned (&v)[VD]) {
    if constexpr (VD == 4) {
        const rq_u4 t = *reinterpret_cast<const rq_u4*>(p);
        v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
    } else {
        v[0] = *p;
    }
}
template <int VD>
__device__ __forceinline__ void pc_st(unsigned* p, const unsigned (&v)[VD]) {
    if constexpr (VD == 4) *reinterpret_cast<rq_u4*>(p) = rq_u4{v[0], v[1], v[2], v[3]};
    else *p = v[0];
}

// a dword of codes on 16-bit lanes: s[k] lane l holds code k + NS l of the dword
template <int FMT>
struct PcSplit {
    static constexpr int NS = FMT == CNNQ_CODES_U8 ? 2 : 4, SH = FMT == CNNQ_CODES_U8 ? 8 : 4;
    static constexpr unsigned MASK = FMT == CNNQ_CODES_U8 ? 0x00FF00FFu : 0x000F000Fu;
    pc_us2 s[NS];
    __device__ __forceinline__ void zero() {
#pragma unroll
        for (int k = 0; k < NS; ++k) s[k] = pc_us2{0, 0};
    }
    __device__ __forceinline__ void max(unsigned x) {       // v_pk_max_u16
#pragma unroll
        for (int k = 0; k < NS; ++k) s[k] = __builtin_elementwise_max(s[k], __builtin_bit_cast(pc_us2, (x >> (k * SH)) & MASK));
    }
    __device__ __forceinline__ void add(unsigned x) {       // v_pk_add_u16
#pragma unroll
        for (int k = 0; k < NS; ++k) s[k] += __builtin_bit_cast(pc_us2, (x >> (k * SH)) & MASK);
    }
    __device__ __forceinline__ unsigned join() const {
        unsigned w = 0u;
#pragma unroll
        for (int k = 0; k < NS; ++k) w |= __builtin_bit_cast(unsigned, s[k]) << (k * SH);
        return w;
    }
};

// ---- the window maximum -------------------------------------------------------------------------------------------------------------
struct MpArgs {
    const unsigned* xq;     // [N][H][W][Cdw]
    unsigned* y;            // [N][OH][OW][Cdw]
    int H, W, OH, OW, Cdw;  // Cdw: dwords of a pixel's channels
    int KH, KW, sh, sw, ph, pw;
    int TOH, TOW, SD;       // the tile of output pixels, the slab's dwords
    int PWp, PHp;           // the patch's width and height made odd: the pitches of the two LDS images
    int tilesH, tilesW, slabs;
};

// the maximum over `taps` items of VD dwords, `pitch` dwords apart
template <int FMT, int VD>
__device__ __forceinline__ void mp_taps(const unsigned* src, int taps, int pitch, unsigned (&out)[VD]) {
    PcSplit<FMT> m[VD];
#pragma unroll
    for (int e = 0; e < VD; ++e) m[e].zero();
    for (int k = 0; k < taps; ++k) {
        unsigned x[VD];
        pc_ld<VD>(src + k * pitch, x);
#pragma unroll
        for (int e = 0; e < VD; ++e) m[e].max(x[e]);
    }
#pragma unroll
    for (int e = 0; e < VD; ++e) out[e] = m[e].join();
}

template <int FMT, int VD>
__global__ __launch_bounds__(TPB) void k_mp_codes(const MpArgs a) {
    __shared__ rq_u4 lds4[MP_LDS_DW / 4];
    unsigned* patch = reinterpret_cast<unsigned*>(lds4);
    const int tid = threadIdx.x;
    unsigned id = blockIdx.x;
    const int slab = (int)(id % (unsigned)a.slabs);
    id /= (unsigned)a.slabs;
    const int tw = (int)(id % (unsigned)a.tilesW);
    id /= (unsigned)a.tilesW;
    const int th = (int)(id % (unsigned)a.tilesH), n = (int)(id / (unsigned)a.tilesH);
    const int d0 = slab * a.SD, nv = min(a.SD, a.Cdw - d0) / VD;            // the slab's items per pixel
    const int oh0 = th * a.TOH, ow0 = tw * a.TOW, toh = min(a.TOH, a.OH - oh0), tow = min(a.TOW, a.OW - ow0);
    const int ih0 = oh0 * a.sh - a.ph, iw0 = ow0 * a.sw - a.pw;
    const int prows = (toh - 1) * a.sh + a.KH, pcols = (tow - 1) * a.sw + a.KW;        // the patch this tile needs
    const int RP = a.PWp * a.SD;
    unsigned* rm = patch + ((a.TOH - 1) * a.sh + a.KH) * RP;

    // 1. the patch; padding and what lies beyond the image: code 0, the identity of the unsigned maximum
    for (int i = tid; i < prows * pcols * nv; i += TPB) {
        const int v = i % nv, p = i / nv, pc = p % pcols, pr = p / pcols;
        const int ih = ih0 + pr, iw = iw0 + pc;
        unsigned x[VD];
#pragma unroll
        for (int e = 0; e < VD; ++e) x[e] = 0u;
        if ((unsigned)ih < (unsigned)a.H && (unsigned)iw < (unsigned)a.W)
            pc_ld<VD>(a.xq + (((long long)n * a.H + ih) * a.W + iw) * a.Cdw + d0 + v * VD, x);
        pc_st<VD>(patch + pr * RP + pc * a.SD + v * VD, x);
    }
    __syncthreads();
    // 2. across the row: item i = (ow, patch row, v), written at its own index of rm[ow][PHp][SD] when the slab is whole
    for (int i = tid; i < tow * prows * nv; i += TPB) {
        const int v = i % nv, q = i / nv, pr = q % prows, ow = q / prows;
        unsigned m[VD];
        mp_taps<FMT, VD>(patch + pr * RP + ow * a.sw * a.SD + v * VD, a.KW, a.SD, m);
        pc_st<VD>(rm + (ow * a.PHp + pr) * a.SD + v * VD, m);
    }
    __syncthreads();
    // 3. down the column, and out: item (oh, ow, v)
    for (int i = tid; i < toh * tow * nv; i += TPB) {
        const int v = i % nv, q = i / nv, ow = q % tow, oh = q / tow;
        unsigned m[VD];
        mp_taps<FMT, VD>(rm + (ow * a.PHp + oh * a.sh) * a.SD + v * VD, a.KH, a.SD, m);
        pc_st<VD>(a.y + (((long long)n * a.OH + oh0 + oh) * a.OW + ow0 + ow) * a.Cdw + d0 + v * VD, m);
    }
}

// the tile and the slab (host): MP_TILE x MP_TILE output pixels x MP_SD dwords, shrunk until both LDS images fit
struct MpPlan {
    int TOH, TOW, SD, PWp, PHp, wide;
    int64_t tilesH, tilesW, slabs;
    bool ok;                // false: even one output pixel of one dword does not fit (a window of ~10^4 taps)
};
inline MpPlan mp_plan(int64_t OH, int64_t OW, int64_t Cdw, int64_t KH, int64_t KW, int64_t sh, int64_t sw, bool wide) {
    int64_t TOH = OH < MP_TILE ? OH : MP_TILE, TOW = OW < MP_TILE ? OW : MP_TILE, SD = Cdw < MP_SD ? Cdw : MP_SD;
    MpPlan p{};
    for (;;) {
        const int64_t PH = (TOH - 1) * sh + KH, PW = (TOW - 1) * sw + KW, PWp = PW | 1, PHp = PH | 1;
        if (PH * PWp * SD + TOW * PHp * SD <= MP_LDS_DW) {
            p = MpPlan{(int)TOH, (int)TOW, (int)SD, (int)PWp, (int)PHp, wide && SD % 4 == 0, (OH + TOH - 1) / TOH, (OW + TOW - 1) / TOW,
                       (Cdw + SD - 1) / SD, true};
            return p;
        }
        if (TOH > 1 && (TOH - 1) * sh >= (TOW - 1) * sw) TOH = (TOH + 1) / 2;
        else if (TOW > 1) TOW = (TOW + 1) / 2;
        else if (TOH > 1) TOH = (TOH + 1) / 2;
        else if (SD > 1) SD = SD > 4 ? (SD / 2 + 3) / 4 * 4 : SD / 2;       // whole 16-byte pieces while it can
        else return p;
    }
}

// ---- the global average -------------------------------------------------------------------------------------------------------------
struct ApArgs {
    const unsigned* xq;     // [N][HW][Cdw]
    float* y;               // [N][C]; the Q instances: q.y
    RqOut q;
    const float* qpx;       // [CNNQ_NQP][Cx]
    int Cx, HW, Cdw, C;
    int cols, G, slabs;     // items per pixel of a whole slab, pixel groups (G cols <= TPB, G <= HW), slabs per image
};

template <int FX, int VD, bool Q>
__global__ __launch_bounds__(TPB) void k_ap_codes(const ApArgs a) {
    constexpr int CPD = FX == CNNQ_CODES_U8 ? 4 : 8, NS = PcSplit<FX>::NS;
    static_assert(2 * NS == CPD, "two lanes per split");
    __shared__ rq_v4i part4[(TPB * VD * CPD + 4 * TPB) / 4];                // G (cols VD CPD + 4) ints at the most
    int* part = reinterpret_cast<int*>(part4);
    const int tid = threadIdx.x;
    const int slab = (int)(blockIdx.x % (unsigned)a.slabs), n = (int)(blockIdx.x / (unsigned)a.slabs);
    const int d0 = slab * AP_SD, sd = min(AP_SD, a.Cdw - d0), nv = sd / VD;
    const int col = tid % a.cols, g = tid / a.cols;
    const int KP = a.cols * VD * CPD + 4;

    if (g < a.G) {
        int acc[VD][CPD];                                                   // acc[e][j]: code j of the column's dword e
#pragma unroll
        for (int e = 0; e < VD; ++e)
#pragma unroll
            for (int j = 0; j < CPD; ++j) acc[e][j] = 0;
        if (col < nv) {
            PcSplit<FX> s[VD];
            auto widen = [&]() {
#pragma unroll
                for (int e = 0; e < VD; ++e) {
#pragma unroll
                    for (int k = 0; k < NS; ++k) {
                        acc[e][k] += s[e].s[k].x;
                        acc[e][k + NS] += s[e].s[k].y;
                    }
                    s[e].zero();
                }
            };
#pragma unroll
            for (int e = 0; e < VD; ++e) s[e].zero();
            const unsigned* src = a.xq + (long long)n * a.HW * a.Cdw + d0 + col * VD;
            int run = 0;
            for (int p = g; p < a.HW; p += a.G) {
                unsigned x[VD];
                pc_ld<VD>(src + (long long)p * a.Cdw, x);
#pragma unroll
                for (int e = 0; e < VD; ++e) s[e].add(x[e]);
                if (++run == AP_WIDEN) {                                    // before a lane can overflow
                    widen();
                    run = 0;
                }
            }
            widen();
        }
        rq_v4i* dst = reinterpret_cast<rq_v4i*>(part + g * KP + col * VD * CPD);
#pragma unroll
        for (int e = 0; e < VD; ++e)
#pragma unroll
            for (int j = 0; j < CPD; j += 4) dst[(e * CPD + j) / 4] = rq_v4i{acc[e][j], acc[e][j + 1], acc[e][j + 2], acc[e][j + 3]};
    }
    __syncthreads();

    // a thread per output dword (four floats): cpt consecutive channels
    const int cpt = Q && a.q.fy == CNNQ_CODES_PACK4 ? 8 : 4;
    const int t = tid;
    if (t * cpt >= sd * CPD) return;
    const int ci = a.Cx == 1 ? 0 : n;
    const double sx = (double)a.qpx[CNNQ_QP_SCALE * (size_t)a.Cx + ci], zx = (double)a.qpx[CNNQ_QP_ZP * (size_t)a.Cx + ci];
    const double hw = (double)a.HW;
    const size_t at = (size_t)n * a.C + (size_t)d0 * CPD + (size_t)t * cpt;  // the thread's first channel in [N][C]
    RqRow qrow{};
    if constexpr (Q) qrow = rq_row(a.q, n);
    unsigned w = 0u;
    for (int h = 0; h * 4 < cpt; ++h) {
        rq_v4i s = rq_v4i{0, 0, 0, 0};
        for (int i = 0; i < a.G; ++i) s += *reinterpret_cast<const rq_v4i*>(part + i * KP + t * cpt + 4 * h);
        float yv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double mean = (double)s[j] / hw;                          // fp64, each operation rounded on its own
            const double diff = mean - zx;
            yv[j] = (float)(diff * sx);
        }
        if constexpr (Q) {
#pragma unroll
            for (int j = 0; j < 4; ++j) w |= rq_code(yv[j], a.q, qrow) << ((4 * h + j) * (32 / cpt));
        } else {
            *reinterpret_cast<float4*>(a.y + at) = float4{yv[0], yv[1], yv[2], yv[3]};
        }
    }
    if constexpr (Q) reinterpret_cast<unsigned*>(a.q.y)[at / cpt] = w;
}

}  // namespace
