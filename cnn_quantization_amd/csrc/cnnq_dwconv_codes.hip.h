// cnnq_dwconv_codes.hip.h - the depthwise 2-D convolution on the stored codes: y[N][OH][OW][C] from NHWC
// activation codes xq[N][H][W][C] (per tensor or per image) and TAP-MAJOR weight codes wq[KH][KW][C] (per channel), channel
// multiplier 1.  There is no reduction over channels (K = KH KW), so the matrix instruction of cnnq_conv_codes.hip.h would do 1 / C
// of its work usefully: this is a kernel of its own on v_dot4_u32_u8.  Part of the single translation unit cnnq_kernels.hip.
//
// The arithmetic is section 36's with the sums taken per channel over the output pixel's VALID taps (cc_window):
//     y[m][c] = sx sw[c] (S - zw[c] Rx - zx RwV + Kv zx zw[c]) + bias[c]
//     S = sum_valid xq wq,  Rx = sum_valid xq,  RwV = sum_valid wq[t][c],  Kv = #valid taps
// - four exact integers below 2^23 (64 * 255 * 255), combined by lc_combine as it stands (ox = ow = 0): one fp64 combination, one
// rounding to fp32.  The Q instances then call rq_code (cnnq_requant_codes.hip.h) as it stands.
//
// The tile.  A workgroup owns TOH x TOW output pixels of one image times a slab of SD dwords of FOUR channels (dw_plan: 8 x 16 x 16,
// shrunk until the patch fits) and runs ONE launch, no workspace, no atomics:
//   1. the input patch ((TOH - 1) sh + KH) x ((TOW - 1) sw + KW) pixels x the slab: global -> LDS, every byte read once, 16-byte
//      loads where a pixel's channel bytes are whole 16-byte pieces on a 16-byte base, else dwords.  What lies outside the image
//      enters as code 0, so S and Rx need no validity test.  pack4 is expanded to ONE CODE PER BYTE on the way in (rq_unpack8): the
//      LDS image has one layout, patch[row][pixel][dword of 4 channels], for both formats, and the expansion is paid once per input
//      byte, not once per tap.  The slab's KH KW weight dwords go to LDS the same way, expanded if pack4.
//   2. wsum[channel] = the full-window sum of the weights, once per workgroup and channel (the RwV of every interior pixel).
//   3. item (unit u, output row oh, run r) - u fastest, then oh: a thread owns one unit - one LDS dword, 4 channels (two, 8 channels,
//      when the output is pack4: a whole dword of output codes) - and a run of DW_RUN = 4 neighbouring outputs along W.  For every
//      tap it reads the unit's weight dword ONCE and masks it to its four bytes (4 v_and, shared by the 4 outputs), then per output
//      reads the patch dword and does per channel c
//          S[c]  = v_dot4_u32_u8(x, w & (0xff << 8 c), S[c])       one product is the channel's, three are with 0
//          Rx[c] = v_dot4_u32_u8(x, 1 << 8 c, Rx[c])
//      - 2 instructions per multiply-add (S and Rx together), + 1/16 of a weight read, 1/4 of a mask and 1/4 of a patch read: 41
//      instructions per 16 multiply-adds, exact for every format pair and tap count (32-bit accumulators).  A border pixel takes
//      RwV by a direct sum over its at most 64 valid taps, an interior one from wsum.
//   4. the finish in registers: lc_combine per channel, then a float4 (fp32), or rq_code and ONE dword of 4 u8 codes / 8 pack4 codes
//      (rq_pack8) per thread and output pixel; neighbouring lanes store neighbouring dwords of the pixel.  No LDS transpose.
// Routes not taken (DESIGN.md section 40 counts them): 16-bit packed lanes (v_pk_mad_u16: exact only below 65536, never for u8 x
// u8 at 3 x 3) and the byte-transposed dot (four taps of one channel per dword through v_perm_b32: 1 instruction per multiply-add,
// but tied to compile-time tap groups).
//
// Banks (64 banks of 4 bytes; SD = 16).  Phase 1 writes consecutive items to consecutive addresses inside a row.  In phase 3 a wave
// is 16 units x 4 output rows at (oh sh RP + u): the row pitch RP (dw_pitch) is the smallest multiple of 4 dwords >= PW SD with
// sh RP an ODD multiple of 16 - the four rows lie on the four distinct multiples of 16 mod 64, all 64 banks once (at stride 1 that
// is section 39's odd patch width; at stride 2 a pitch of 8 mod 16).  The weight read is the same 16 dwords for the four rows: a
// broadcast.  A slab of 8 dwords puts 8 rows at distinct multiples of 8 the same way.
#pragma once
#include "cnnq_conv_codes.hip.h"
#include "cnnq_pool_codes.hip.h"

namespace {

constexpr int DW_PATCH_DW = 8192;    // the patch: 32 KB
constexpr int DW_SD = 16;            // LDS dwords (4 channels each) per slab: 64 channels
constexpr int DW_W_DW = CC_MAX_TAPS * DW_SD;    // the slab's weights, one code per byte: 4 KB
constexpr int DW_TOH = 8, DW_TOW = 16;          // output pixels per tile before the patch is fitted to the LDS
constexpr int DW_RUN = 4;            // outputs along W per thread

struct DwArgs {
    const unsigned* xq;     // [N][H][W][C / 4] (u8) or [C / 8] (pack4)
    const unsigned* wq;     // [KH KW][C / 4] or [C / 8]
    float* y;               // [N][OH][OW][C]; the Q instances: q.y
    RqOut q;
    LcEpi e;                // qpx, qpw, bias, Cx; N = C, ox = ow = 0
    CcGeo g;
    int OH, Cdw;            // Cdw = C / 4: the LDS dwords of a pixel
    int TOH, TOW, SD, RP;   // the tile, the slab, the patch's row pitch in dwords
    int tilesH, tilesW, slabs, wide;
};

// the patch: VD global dwords per item; FX pack4: every global dword becomes two LDS dwords
template <int FX, int VD>
__device__ __forceinline__ void dw_load_patch(const DwArgs& a, unsigned* patch, int n, int d0, int sd, int ih0, int iw0, int prows, int pcols) {
    constexpr int XG = FX == CNNQ_CODES_U8 ? 1 : 2;                         // LDS dwords per global dword
    const int xdw = a.Cdw / XG, g0 = d0 / XG, nv = sd / XG / VD;
    for (int i = threadIdx.x; i < prows * pcols * nv; i += TPB) {
        const int v = i % nv, p = i / nv, pc = p % pcols, pr = p / pcols;
        const int ih = ih0 + pr, iw = iw0 + pc;
        unsigned x[VD];
#pragma unroll
        for (int k = 0; k < VD; ++k) x[k] = 0u;
        if ((unsigned)ih < (unsigned)a.g.H && (unsigned)iw < (unsigned)a.g.W)
            pc_ld<VD>(a.xq + (((long long)n * a.g.H + ih) * a.g.W + iw) * xdw + g0 + v * VD, x);
        unsigned* dst = patch + pr * a.RP + pc * a.SD + v * VD * XG;
        if constexpr (FX == CNNQ_CODES_U8) {
            pc_st<VD>(dst, x);
        } else {
#pragma unroll
            for (int k = 0; k < VD; ++k) rq_unpack8(x[k], dst[2 * k], dst[2 * k + 1]);
        }
    }
}

// OUT: 0 - fp32, 1 - u8 codes, 2 - pack4 codes
template <int FX, int FW, int OUT>
__global__ __launch_bounds__(TPB) void k_dw_codes(const DwArgs a) {
    constexpr int UD = OUT == 2 ? 2 : 1;                                    // LDS dwords of a thread's unit
    __shared__ rq_u4 lds4[(DW_PATCH_DW + DW_W_DW) / 4];
    __shared__ int wsum[DW_SD * 4];
    unsigned* patch = reinterpret_cast<unsigned*>(lds4);
    unsigned* wl = patch + DW_PATCH_DW;                                     // [tap][SD]
    const int tid = threadIdx.x;
    unsigned id = blockIdx.x;
    const int slab = (int)(id % (unsigned)a.slabs);
    id /= (unsigned)a.slabs;
    const int tw = (int)(id % (unsigned)a.tilesW);
    id /= (unsigned)a.tilesW;
    const int th = (int)(id % (unsigned)a.tilesH), n = (int)(id / (unsigned)a.tilesH);
    const CcGeo& g = a.g;
    const int d0 = slab * a.SD, sd = min(a.SD, a.Cdw - d0);
    const int oh0 = th * a.TOH, ow0 = tw * a.TOW, toh = min(a.TOH, a.OH - oh0), tow = min(a.TOW, g.OW - ow0);
    const int prows = (toh - 1) * g.sh + g.KH, pcols = (tow - 1) * g.sw + g.KW;
    const int ntaps = g.KH * g.KW;

    // 1. the patch and the slab's weights, one code per byte
    if (a.wide) dw_load_patch<FX, 4>(a, patch, n, d0, sd, oh0 * g.sh - g.ph, ow0 * g.sw - g.pw, prows, pcols);
    else dw_load_patch<FX, 1>(a, patch, n, d0, sd, oh0 * g.sh - g.ph, ow0 * g.sw - g.pw, prows, pcols);
    if constexpr (FW == CNNQ_CODES_U8) {
        for (int i = tid; i < ntaps * sd; i += TPB) {
            const int t = i / sd, d = i % sd;
            wl[t * a.SD + d] = a.wq[(size_t)t * a.Cdw + d0 + d];
        }
    } else {
        const int hd = sd / 2;
        for (int i = tid; i < ntaps * hd; i += TPB) {
            const int t = i / hd, d = i % hd;
            rq_unpack8(a.wq[(size_t)t * (a.Cdw / 2) + d0 / 2 + d], wl[t * a.SD + 2 * d], wl[t * a.SD + 2 * d + 1]);
        }
    }
    __syncthreads();
    // 2. the full window's weight sums
    if (tid < sd) {
        unsigned s[4] = {0u, 0u, 0u, 0u};
        for (int t = 0; t < ntaps; ++t) {
            const unsigned w = wl[t * a.SD + tid];
#pragma unroll
            for (int c = 0; c < 4; ++c) s[c] = __builtin_amdgcn_udot4(w, 1u << (8 * c), s[c], false);
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) wsum[tid * 4 + c] = (int)s[c];
    }
    __syncthreads();

    // 3. item (u, oh, run), u fastest
    const int nu = sd / UD, runs = (tow + DW_RUN - 1) / DW_RUN;
    const int mp = a.e.Cx == 1 ? 0 : n;
    RqRow qrow{};
    if constexpr (OUT != 0) qrow = rq_row(a.q, n);
    for (int item = tid; item < nu * toh * runs; item += TPB) {
        const int u = item % nu, q = item / nu, oh = q % toh, ow1 = (q / toh) * DW_RUN, nr = min(DW_RUN, tow - ow1);
        unsigned S[DW_RUN][UD][4], R[DW_RUN][UD][4];
        const unsigned* px[DW_RUN];                                          // an output beyond the tile repeats the run's last one
#pragma unroll
        for (int r = 0; r < DW_RUN; ++r) {
            px[r] = patch + oh * g.sh * a.RP + (ow1 + min(r, nr - 1)) * g.sw * a.SD + u * UD;
#pragma unroll
            for (int k = 0; k < UD; ++k)
#pragma unroll
                for (int c = 0; c < 4; ++c) S[r][k][c] = R[r][k][c] = 0u;
        }
        const unsigned* wp = wl + u * UD;
        for (int kh = 0; kh < g.KH; ++kh) {
            for (int kw = 0; kw < g.KW; ++kw) {
                unsigned wm[UD][4];
#pragma unroll
                for (int k = 0; k < UD; ++k) {
                    const unsigned w = wp[(kh * g.KW + kw) * a.SD + k];
#pragma unroll
                    for (int c = 0; c < 4; ++c) wm[k][c] = w & (0xFFu << (8 * c));
                }
#pragma unroll
                for (int r = 0; r < DW_RUN; ++r) {
#pragma unroll
                    for (int k = 0; k < UD; ++k) {
                        const unsigned x = px[r][kh * a.RP + kw * a.SD + k];
#pragma unroll
                        for (int c = 0; c < 4; ++c) {
                            S[r][k][c] = __builtin_amdgcn_udot4(x, wm[k][c], S[r][k][c], false);
                            R[r][k][c] = __builtin_amdgcn_udot4(x, 1u << (8 * c), R[r][k][c], false);
                        }
                    }
                }
            }
        }
        // 4. the finish: the valid rectangle, RwV, lc_combine, the store
        const int ch0 = (d0 + u * UD) * 4;
#pragma unroll
        for (int r = 0; r < DW_RUN; ++r) {
            if (r >= nr) break;
            const int ohg = oh0 + oh, owg = ow0 + ow1 + r;
            int kh0, kh1, kw0, kw1;
            cc_window(g, ohg * g.sh - g.ph, owg * g.sw - g.pw, kh0, kh1, kw0, kw1);
            const int kv = (kh1 - kh0) * (kw1 - kw0);
            unsigned rw[UD][4];
            if (kv == ntaps) {
#pragma unroll
                for (int k = 0; k < UD; ++k)
#pragma unroll
                    for (int c = 0; c < 4; ++c) rw[k][c] = (unsigned)wsum[(u * UD + k) * 4 + c];
            } else {
#pragma unroll
                for (int k = 0; k < UD; ++k)
#pragma unroll
                    for (int c = 0; c < 4; ++c) rw[k][c] = 0u;
                for (int kh = kh0; kh < kh1; ++kh)
                    for (int kw = kw0; kw < kw1; ++kw)
#pragma unroll
                        for (int k = 0; k < UD; ++k) {
                            const unsigned w = wp[(kh * g.KW + kw) * a.SD + k];
#pragma unroll
                            for (int c = 0; c < 4; ++c) rw[k][c] = __builtin_amdgcn_udot4(w, 1u << (8 * c), rw[k][c], false);
                        }
            }
            float yv[UD][4];
#pragma unroll
            for (int k = 0; k < UD; ++k)
#pragma unroll
                for (int c = 0; c < 4; ++c)
                    yv[k][c] = lc_combine((long long)S[r][k][c], (long long)R[r][k][c], (long long)rw[k][c], (long long)kv, mp, ch0 + 4 * k + c, a.e);
            const long long pix = ((long long)n * a.OH + ohg) * g.OW + owg;
            if constexpr (OUT == 0) {
                *reinterpret_cast<float4*>(a.y + pix * g.C + ch0) = float4{yv[0][0], yv[0][1], yv[0][2], yv[0][3]};
            } else {
                unsigned cd[UD];
#pragma unroll
                for (int k = 0; k < UD; ++k) {
                    cd[k] = 0u;
#pragma unroll
                    for (int c = 0; c < 4; ++c) cd[k] |= rq_code(yv[k][c], a.q, qrow) << (8 * c);
                }
                unsigned* dst = reinterpret_cast<unsigned*>(a.q.y);
                if constexpr (OUT == 1) dst[pix * a.Cdw + d0 + u] = cd[0];
                else dst[(pix * a.Cdw + d0) / 2 + u] = rq_pack8(cd[0], cd[1]);
            }
        }
    }
}

// ---- the tile and the slab (host) ----------------------------------------------------------------------------------------------------
// the patch's row pitch: the smallest multiple of 4 dwords >= need with sh * pitch an odd multiple of the slab (a power of two)
inline int64_t dw_pitch(int64_t need, int64_t SD, int64_t sh) {
    const int64_t lo = (need + 3) / 4 * 4;
    if (SD >= 4 && !(SD & (SD - 1)))
        for (int64_t rp = lo; rp < lo + 8 * SD; rp += 4)
            if ((sh * rp) % (2 * SD) == SD) return rp;
    return lo;
}

struct DwPlan {
    int TOH, TOW, SD, RP;
    int64_t tilesH, tilesW, slabs;
    bool ok;                // false: even one output pixel of one unit does not fit
};
// Cdw: the LDS dwords of a pixel (C / 4); even whenever C % 8 == 0, and then every slab is even: whole pack4 dwords
inline DwPlan dw_plan(int64_t N, int64_t OH, int64_t OW, int64_t Cdw, int64_t KH, int64_t KW, int64_t sh, int64_t sw) {
    int64_t TOH = OH < DW_TOH ? OH : DW_TOH, TOW = OW < DW_TOW ? OW : DW_TOW, SD = Cdw < DW_SD ? Cdw : DW_SD;
    const int64_t gran = Cdw % 2 ? 1 : 2;
    // a launch that cannot fill the chip: narrower slabs, twice the workgroups
    if (SD == DW_SD && N * ((OH + TOH - 1) / TOH) * ((OW + TOW - 1) / TOW) * ((Cdw + SD - 1) / SD) < 512) SD = DW_SD / 2;
    DwPlan p{};
    for (;;) {
        const int64_t PH = (TOH - 1) * sh + KH, PW = (TOW - 1) * sw + KW;
        // PW SD first: a stride of 2^30 must not overflow the pitch search
        if (PW * SD <= DW_PATCH_DW) {
            const int64_t RP = dw_pitch(PW * SD, SD, sh);
            if (PH * RP <= DW_PATCH_DW) {
                p = DwPlan{(int)TOH, (int)TOW, (int)SD, (int)RP, (OH + TOH - 1) / TOH, (OW + TOW - 1) / TOW, (Cdw + SD - 1) / SD, true};
                return p;
            }
        }
        if (TOH > 1 && (TOH - 1) * sh >= (TOW - 1) * sw) TOH = (TOH + 1) / 2;
        else if (TOW > 1) TOW = (TOW + 1) / 2;
        else if (TOH > 1) TOH = (TOH + 1) / 2;
        else if (SD > gran) SD = SD > 8 ? (SD / 2 + 7) / 8 * 8 : SD > 4 ? 4 : SD > 2 ? 2 : gran;
        else return p;
    }
}

}  // namespace
