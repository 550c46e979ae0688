// cnnq_kernels.hip - gfx950 (MI355X / CDNA4) kernels behind include/cnnq_hip.h.
//
// Design: the whole path is HBM-bound elementwise + reduction work, so
// nothing here is shaped for MFMA.  All streaming kernels share ONE decomposition of the
// NCHW tensor x[N][C][HW]:
//
//   * the C*HW "plane" of one sample is cut into column blocks; a workgroup owns one column
//     block and walks it down the batch (n = n0 .. n1), so every lane keeps the SAME channel(s)
//     for its whole life: per-channel scale/zero-point are fetched once (staged through LDS)
//     and live in registers, the hot loop is load(16 B) -> ALU -> store(16 B), fully coalesced,
//     with no index division and no transposed copy;
//   * column blocks are aligned to channel boundaries: either a slice of ONE channel (mode 1,
//     large H*W) or k WHOLE channels (mode 2, small H*W), so reductions finish inside the
//     workgroup (wave64 shuffles + LDS) and each (group, channel) partial is written by
//     exactly one workgroup - no atomics, deterministic results;
//   * three load shapes: VEC4 (H*W % 4 == 0), VEC4-straddle (H*W % 4 != 0 but C*H*W % 4 == 0,
//     e.g. 7x7: a float4 may span two channels, per-element bookkeeping) and VEC1 (anything,
//     incl. unaligned base pointers);
//   * two launch geometries over that decomposition (make_geo): the REDUCTION passes (statistics)
//     use <= 64 batch splits, i.e. ~4096 long-lived workgroups that amortise their in-workgroup
//     reduction; the table-driven ELEMENTWISE passes (Q/DQ and friends) use ~14 KB of x per
//     workgroup, dispatched in address order - on MI355X read+write streaming reaches 6.1-6.7 TB/s
//     that way against 5.4 TB/s with long-lived workgroups; statistics passes over tensors too big
//     for the Infinity Cache use non-temporal loads (read-only 7.1 vs 6.3 TB/s).
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (division must stay an IEEE
// divide followed by a separately rounded add: bit-exactness with the reference's aten ops).
//
// Layout: the kernels live in the cnnq_*.hip.h files next to this one (one file per stage of the path),
// all in one anonymous namespace of this single translation unit; below them is the C ABI.  The host glue the entry points
// share is written once: the runtime -> template dispatchers (with_shape / with_int / with_bool), the exchange workspace view
// (gws_view) and the fused-launch rule (fused_ok / plan_fused) in cnnq_plan.hip.h next to the launch_* functions, with_piece
// (element type x piece width) in cnnq_nhwc.hip.h, and - right below the includes here - the argument checks, the small
// argument builders and the channels_last plan and dispatcher (ClPlan, cl_launch); a caller workspace's layout (StatsWs, MmWs,
// AciqWs) stands next to the function that sizes it.

#include <string.h>

#include <vector>
#include "cnnq_common.hip.h"
#include "cnnq_stats.hip.h"
#include "cnnq_params.hip.h"
#include "cnnq_qdq.hip.h"
#include "cnnq_pack4.hip.h"
#include "cnnq_midtread.hip.h"
#include "cnnq_corrections.hip.h"
#include "cnnq_pertensor.hip.h"
#include "cnnq_resident.hip.h"
#include "cnnq_group.hip.h"
#include "cnnq_plan.hip.h"
#include "cnnq_kld.hip.h"
#include "cnnq_half.hip.h"
#include "cnnq_half_stats.hip.h"
#include "cnnq_half_bcorr.hip.h"
#include "cnnq_half_aciq.hip.h"
#include "cnnq_half_midtread.hip.h"
#include "cnnq_half_entropy.hip.h"
#include "cnnq_half_kld.hip.h"
#include "cnnq_nhwc.hip.h"
#include "cnnq_nhwc_aciq.hip.h"
#include "cnnq_nhwc_collect.hip.h"
#include "cnnq_nhwc_bcorr.hip.h"
#include "cnnq_nhwc_midtread.hip.h"
#include "cnnq_nhwc_entropy.hip.h"
#include "cnnq_nhwc_packed.hip.h"
#include "cnnq_qerr.hip.h"
#include "cnnq_nhwc_qerr.hip.h"
#include "cnnq_half_qerr.hip.h"
#include "cnnq_sample_extrema.hip.h"
#include "cnnq_rows.hip.h"
#include "cnnq_flat.hip.h"

namespace {

// ---- shared host helpers of the C ABI below ---------------------------------------------------------------------------------
inline bool nt_loads(int64_t bytes) { return bytes > NT_BYTES; }      // beyond the Infinity Cache: non-temporal loads
inline bool misaligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) != 0; }   // a: a power of two (NULL is aligned)
inline bool pow2(int v) { return v > 0 && !(v & (v - 1)); }
inline bool hist_bins_ok(int nbins) { return nbins >= 2 && nbins <= 256 && pow2(nbins); }   // the bins of a counting pass
inline int g_error(int G) { return G ? G : CNNQ_EINVAL; }             // what a group count G <= 0 says: the plan's error
inline hipStream_t hs(void* stream) { return (hipStream_t)stream; }
inline unsigned long long* u64p(uint64_t* p) { return reinterpret_cast<unsigned long long*>(p); }

// one wave (at least) per 64 channels, PTPB at most: the single-workgroup parameter kernels
inline int param_threads(int64_t C) { return (int)(C >= PTPB ? PTPB : ((C + 63) / 64) * 64); }
// the merge kernels: merge_cpw channels per workgroup
inline dim3 merge_grid(int G, int64_t C) { return dim3((unsigned)((C + merge_cpw(G, (int)C) - 1) / merge_cpw(G, (int)C))); }

// cnnq_params_cfg as every entry point that takes one checks it before its first launch
inline int check_cfg(const cnnq_params_cfg* cfg) {
    if (cfg->num_bits < 1 || cfg->num_bits > 32 || cfg->clip < 0 || cfg->clip > 3) return CNNQ_EINVAL;
    // the ACIQ factor tables have entries for 0..8 bits only (iq.py:14-41: the reference's alpha_laplace / alpha_gaus
    // dictionaries raise KeyError beyond 8); wider codes are accepted for min/max and the '<p>std' clip alone
    return ((cfg->clip == 1 || cfg->clip == 2) && cfg->num_bits > 8) ? CNNQ_EINVAL : 0;
}
inline bool cfg_bit_alloc(const cnnq_params_cfg* cfg) { return cfg->bit_alloc && cfg->num_bits <= 4; }   // (its table lives in diag)

inline XOut xout(uint8_t* codes, uint64_t* hist_rep, uint8_t* packed = nullptr) {
    XOut xo;
    xo.codes = codes;
    xo.hist = u64p(hist_rep);
    xo.packed = packed;
    return xo;
}
// the cross-rank stage's arguments.  seq != 0: host numbering (seq_dev, if `mirror`, follows it); seq == 0: device numbering in
// seq_dev; either way the launches keep the slot counts themselves behind seq_dev (round 6)
inline XRank xrank_args(void* const* windows, int rank, int world, int cmax, uint32_t seq, uint32_t* seq_dev, bool mirror, int zero_c, int nslots,
                        int slot0, uint32_t* status, int64_t timeout) {
    XRank xr;
    xr.windows = windows;
    xr.rank = rank;
    xr.world = world;
    xr.seq = seq;
    xr.seq_dev = seq ? nullptr : seq_dev;
    xr.seq_mirror = (seq && mirror) ? seq_dev : nullptr;
    xr.zero_c = zero_c;
    xr.cdev = seq_dev ? seq_dev + 4 : nullptr;
    xr.nslots = nslots;
    xr.slot0 = slot0;
    xr.no_prologue = 0;
    xr.cmax = cmax;
    xr.status = status;
    xr.timeout = timeout;
    return xr;
}
inline St1Args st1_args(float* stats, double* mom, int64_t N, int64_t HW, int need_b, int need_kurt, int need_relu) {
    St1Args sa;
    sa.stats = stats;
    sa.mom = mom;
    sa.count = (double)N * (double)HW;
    sa.need_relu = need_relu ? 1 : 0;
    sa.need_dev = (need_b || need_kurt) ? 1 : 0;
    sa.need_kurt = need_kurt ? 1 : 0;
    return sa;
}

// pass B (k_absdev, descending: it follows the ascending pass A) from the merged table `stats`, or - raw != NULL - straight
// from the UNMERGED pass-A records (each workgroup merges its own channels' records in its prologue)
int launch_absdev(const float* x, int64_t N, int64_t C, int64_t HW, const float* stats, const double* raw, int want_kurt, double* part2,
                  void* stream) {
    Variant v;
    Geo g;
    const int rc = plan(N, C, HW, al16(x), /*rev=*/1, &v, &g);
    if (rc) return rc;
    const int G = raw ? g.S * g.nb : 0;
    with_shape(v, [&](auto s) {
        with_bool(want_kurt != 0, nt_loads(N * C * HW * 4), raw != nullptr, [&](auto k, auto nt, auto r) {
            using S = decltype(s);
            hipLaunchKernelGGL((k_absdev<S::VEC, S::A, S::J, decltype(k)::value, decltype(nt)::value, decltype(r)::value>), geo_grid(g), dim3(TPB), 0,
                               hs(stream), x, g, stats, part2, raw, G);
        });
    });
    return launch_status();
}

// ---- dense channels_last activations: the plan and the dispatcher of the *_nhwc entry points at the end of this file ----------
// What every channels_last entry point and route function derives - after its argument checks (R, C >= 1, C <= CL_C_MAX), before
// its first launch - from the shape, the element type and the alignment x and y share: the piece width w, the geometry m of the
// statistics launches (cl_geo_mm), the geometry q of the element-wise pass (cl_geo_qdq), and whether 32 bits index them.
struct ClPlan {
    int w;
    ClGeo m, q;
    ClPlan(int64_t R, int64_t C, int dtype, int align_bytes)
        : w(cl_piece(C, cl_esize(dtype), align_bytes)), m(cl_geo_mm(R, C, w)), q(cl_geo_qdq(R, C, w)) {}
    dim3 mgrid() const { return dim3((unsigned)(m.S * m.nb)); }
    dim3 qgrid() const { return dim3((unsigned)(q.S * q.nb)); }
    // CNNQ_ERANGE unless the largest grid, the element-wise pass' q.S * q.nb workgroups, stays below 2^31 (m has q's nb - both
    // come from P and CP - and fewer than CL_MM_MAX_WGS + nb workgroups).  rows32: and a slab has fewer than 2^31 rows.  Asked
    // only by who keeps that count in 32 bits: k_cl_bcorr_sums' per-lane counter and out[2] of cnnq_pc_route_aciq_nhwc.
    // k_cl_minmax counts nothing and k_cl_moments takes its count in fp64 from the 64-bit row bounds, so configs 2 and 3 and
    // cnnq_pc_route_nhwc accept such a slab.
    int range(bool rows32) const {
        if ((int64_t)q.S * q.nb >= ((int64_t)1 << 31)) return CNNQ_ERANGE;
        return (rows32 && m.rpw >= ((int64_t)1 << 31)) ? CNNQ_ERANGE : 0;
    }
};

// with_piece plus the tensors as the kernels' element pointers: f(Piece<T, W>, const Raw* x, Raw* y), or f(Piece<T, W>, const Raw* x)
// for a launch that only reads; the launch's status
template <class F>
inline int cl_launch(int dtype, int w, const void* x, void* y, F&& f) {
    with_piece(dtype, w, [&](auto pc) {
        using Raw = typename ClRaw<typename decltype(pc)::T>::type;
        f(pc, static_cast<const Raw*>(x), static_cast<Raw*>(y));
    });
    return launch_status();
}
template <class F>
inline int cl_launch(int dtype, int w, const void* x, F&& f) {
    return cl_launch(dtype, w, x, nullptr, [&](auto pc, auto* xr, auto*) { f(pc, xr); });
}

// The same for the contiguous bf16 / fp16 kernels (cnnq_half*.hip.h), whose elements are 2-byte words whatever the type:
// f(Piece<T, W>, const uint16_t* x, uint16_t* y), or f(Piece<T, W>, const uint16_t* x); the launch's status
template <class F>
inline int h_launch(int dtype, int w, const void* x, void* y, F&& f) {
    with_piece<false>(dtype, w, [&](auto pc) { f(pc, static_cast<const uint16_t*>(x), static_cast<uint16_t*>(y)); });
    return launch_status();
}
template <class F>
inline int h_launch(int dtype, int w, const void* x, F&& f) {
    return h_launch(dtype, w, x, nullptr, [&](auto pc, const uint16_t* xh, uint16_t*) { f(pc, xh); });
}

inline bool dtype_ok(int dtype) { return dtype >= 0 && dtype < CNNQ_NDTYPE; }

inline int cl_check(int64_t R, int64_t C, int dtype) {
    return (!dtype_ok(dtype) || R < 1 || C < 1 || C > CL_C_MAX) ? CNNQ_EINVAL : 0;
}

// What every channels_last route function opens with: its argument checks (ok: the function's own, refused with them), the plan,
// the plan's range; then report(plan) fills out
template <class F>
inline int cl_route(int64_t R, int64_t C, int dtype, int align_bytes, const int32_t* out, bool rows32, bool ok, F&& report) {
    if (cl_check(R, C, dtype) || !out || !pow2(align_bytes) || !ok) return CNNQ_EINVAL;
    const ClPlan p(R, C, dtype, align_bytes);
    if (const int rc = p.range(rows32)) return rc;
    return report(p);
}

}  // namespace

extern "C" {

const char* cnnq_version(void) { return "cnnq-hip 0.4 gfx950"; }

int cnnq_pc_groups(int64_t N, int64_t C, int64_t HW, int aligned16) {
    Variant v;
    Geo g;
    const int rc = plan(N, C, HW, aligned16 != 0, 0, &v, &g);
    if (rc) return rc;
    return g.S * g.nb;
}

int cnnq_plan_describe(int64_t N, int64_t C, int64_t HW, int aligned16, int fine, int32_t out[12]) {
    if (!out) return CNNQ_EINVAL;
    Variant v;
    Geo g;
    const int rc = plan(N, C, HW, aligned16 != 0, 0, &v, &g, fine);
    if (rc) return rc;
    const int32_t vals[12] = {v.vec, v.A, v.J, g.mode, g.nb, g.w, g.k, g.ncb, g.S, TPB, g.S * g.nb, 0};
    for (int i = 0; i < 12; ++i) out[i] = vals[i];
    return 0;
}

int cnnq_pc_moments(const float* x, int64_t N, int64_t C, int64_t HW, int want_relu, double* part, void* stream) {
    if (!x || !part) return CNNQ_EINVAL;
    Variant v;
    Geo g;
    const int rc = plan(N, C, HW, al16(x), 0, &v, &g);
    if (rc) return rc;
    with_shape(v, [&](auto s) {
        with_bool(want_relu != 0, nt_loads(N * C * HW * 4), [&](auto r, auto nt) {
            using S = decltype(s);
            hipLaunchKernelGGL((k_moments<S::VEC, S::A, S::J, decltype(r)::value, decltype(nt)::value>), geo_grid(g), dim3(TPB), 0, hs(stream), x, g, part);
        });
    });
    return launch_status();
}

int cnnq_pc_combine(const double* part, int G, int64_t C, int has_relu, double* mom, float* stats, void* stream) {
    if (!part || G <= 0 || C <= 0 || C >= ((int64_t)1 << 31) || (!mom && !stats)) return CNNQ_EINVAL;
    hipLaunchKernelGGL(k_combine, merge_grid(G, C), dim3(TPB), 0, (hipStream_t)stream, part, G, (int)C, has_relu, mom, stats);
    return launch_status();
}

int cnnq_pc_absdev(const float* x, int64_t N, int64_t C, int64_t HW, const float* stats, int want_kurt,
                   double* part2, void* stream) {
    if (!x || !stats || !part2) return CNNQ_EINVAL;
    return launch_absdev(x, N, C, HW, stats, nullptr, want_kurt, part2, stream);
}

// All per-channel statistics of one tensor behind ONE call and one caller workspace: pass A -> (pass B with the
// pass-A merge fused into its prologue -> one final merge of both passes) - three launches for the full set of
// smpc.py:45-79 instead of four, two for {min, max, mean, std}.  ws: doubles part[G][NMOM][C], part2[G][NDEV][C].
struct StatsWs {
    double *part, *part2;
    StatsWs(void* ws, int G, int64_t C) : part(reinterpret_cast<double*>(ws)), part2(part + (size_t)G * CNNQ_NMOM * C) {}
    static size_t bytes(int G, int64_t C) { return ((size_t)G * (CNNQ_NMOM + CNNQ_NDEV)) * (size_t)C * sizeof(double); }
};

size_t cnnq_pc_stats_workspace(int64_t N, int64_t C, int64_t HW, int aligned16) {
    const int G = cnnq_pc_groups(N, C, HW, aligned16);
    return G <= 0 ? 0 : StatsWs::bytes(G, C);
}

// the final merge of both passes: every row of the table, and the merged moment record
static int combine_all(const double* part, const double* part2, int G, int64_t C, int need_relu, int need_kurt, double* mom, float* stats,
                       void* stream) {
    hipLaunchKernelGGL(k_combine_all, merge_grid(G, C), dim3(TPB), 0, hs(stream), part, part2, G, (int)C, need_relu, need_kurt, mom, stats);
    return launch_status();
}

int cnnq_pc_stats(const float* x, int64_t N, int64_t C, int64_t HW, int need_b, int need_kurt, int need_relu, void* ws,
                  double* mom, float* stats, void* stream) {
    if (!x || !ws || !stats || misaligned(ws, 8)) return CNNQ_EINVAL;
    const int G = cnnq_pc_groups(N, C, HW, al16(x) ? 1 : 0);
    if (G <= 0) return g_error(G);
    const StatsWs w(ws, G, C);
    // the merge kernels write every row of the table (zero where nothing was requested): no memset
    int rc = cnnq_pc_moments(x, N, C, HW, need_relu, w.part, stream);
    if (rc) return rc;
    if (!(need_b || need_kurt)) return cnnq_pc_combine(w.part, G, C, need_relu, mom, stats, stream);
    rc = launch_absdev(x, N, C, HW, nullptr, w.part, need_kurt, w.part2, stream);
    if (rc) return rc;
    return combine_all(w.part, w.part2, G, C, need_relu, need_kurt, mom, stats, stream);
}

// The same table from ONE launch that reads x once (cnnq_stats1.hip.h: the tile stays in registers across pass A and pass B,
// the partial sums meet through the slot region of the group workspace): 4 instead of 8 bytes per element, one launch instead
// of three.  Flat-tile plans only; CNNQ_ENOTSUP - nothing enqueued - otherwise (and for a gws that is NULL or too small): the
// caller takes cnnq_pc_stats.  flags: bit 0 - skip the waits and recompute (tests); bit 3 - also channels of more than 256 tiles and
// the row-piece routing that the default (0: what cnnq_pc_stats_auto passes) leaves to the chain because it loses there.
static int stats_single_impl(const float* x, int64_t N, int64_t C, int64_t HW, int need_b, int need_kurt, int need_relu, void* gws,
                             size_t gws_bytes, double* mom, float* stats, unsigned flags, void* stream, bool aligned, bool dry) {
    GPlan gp;
    if (plan_sums(N, C, HW, aligned, &gp, 0) != 0 || gp.ws_bytes > gws_bytes) return CNNQ_ENOTSUP;
    // two meetings with nothing to write behind them: with many members per channel they cost more than the second read.  Measured
    // up to 196 members ([512,64,112,112]: 431 us against the chain's 495-560 since the arithmetic of the tile went two elements
    // per instruction, round 6; 529 before, when the rule was 128); nothing measured beyond 256 - tests force those with flag 8
    if (gp.Gs > ST_MAX_MEMBERS && !(flags & 8u)) return CNNQ_ENOTSUP;
    const St1Args sa = st1_args(stats, mom, N, HW, need_b, need_kurt, need_relu);
    if (!gp.flat) {
        // short rows: row-piece tiles (k_stats_group), where they beat the chain (stats_group_pays: every one-channel-per-lane
        // shape, straddling rows only while the tensor is small)
        if (!(flags & 8u) && !stats_group_pays(gp, N, C, HW)) return CNNQ_ENOTSUP;
        const int rc = launch_stats_group(x, gp, sa, gws, gws_bytes, flags & 1u, (hipStream_t)stream, nullptr, dry);
        return (dry && rc == 0) ? 2 : rc;
    }
    const int rc = launch_stats_flat(x, gp, sa, gws, flags & 1u, nt_loads(N * C * HW * 4), hs(stream), nullptr, dry);
    return (dry && rc == 0) ? 1 : rc;
}

int cnnq_pc_stats_single(const float* x, int64_t N, int64_t C, int64_t HW, int need_b, int need_kurt, int need_relu, void* gws,
                         size_t gws_bytes, double* mom, float* stats, unsigned flags, void* stream) {
    if (!x || !stats || misaligned(gws, 128) || misaligned(mom, 8)) return CNNQ_EINVAL;
    if (!gws) return CNNQ_ENOTSUP;
    return stats_single_impl(x, N, C, HW, need_b, need_kurt, need_relu, gws, gws_bytes, mom, stats, flags, stream, al16(x), false);
}

// Which route cnnq_pc_stats_single / _auto take for this geometry (nothing is launched): 1 - the flat-tile single launch, 2 - the
// row-piece single launch, 0 - CNNQ_ENOTSUP there, i.e. the three-launch chain.  For accounting (bench.py prices config 4 at
// the bytes its launches move) and for callers that want to size their expectations; negative: an error of the plan.
int cnnq_pc_stats_route(int64_t N, int64_t C, int64_t HW, int aligned16, size_t gws_bytes, unsigned flags) {
    const int rc = stats_single_impl(nullptr, N, C, HW, 1, 1, 1, nullptr, gws_bytes, nullptr, nullptr, flags, nullptr, aligned16 != 0, true);
    return rc == CNNQ_ENOTSUP ? 0 : rc;
}

// cnnq_pc_stats_single when it applies, else cnnq_pc_stats: one call, the same ws
int cnnq_pc_stats_auto(const float* x, int64_t N, int64_t C, int64_t HW, int need_b, int need_kurt, int need_relu, void* ws, void* gws,
                       size_t gws_bytes, double* mom, float* stats, void* stream) {
    const int rc = cnnq_pc_stats_single(x, N, C, HW, need_b, need_kurt, need_relu, gws, gws_bytes, mom, stats, 0u, stream);
    if (rc != CNNQ_ENOTSUP) return rc;
    return cnnq_pc_stats(x, N, C, HW, need_b, need_kurt, need_relu, ws, mom, stats, stream);
}

int cnnq_pc_combine_dev(const double* part2, int G, int64_t C, const double* mom, int want_kurt, double* dev_out,
                        float* stats, void* stream) {
    if (!part2 || G <= 0 || C <= 0 || C >= ((int64_t)1 << 31) || (!dev_out && !stats) || (stats && !mom))
        return CNNQ_EINVAL;
    hipLaunchKernelGGL(k_combine_dev, merge_grid(G, C), dim3(TPB), 0, (hipStream_t)stream, part2, G, (int)C, mom, want_kurt, dev_out,
                       stats);
    return launch_status();
}

int cnnq_pc_params(const float* stats, int64_t C, const cnnq_params_cfg* cfg, float* qp, float* diag,
                   void* stream) {
    if (!stats || !cfg || !qp || C <= 0 || C >= ((int64_t)1 << 31)) return CNNQ_EINVAL;
    if (check_cfg(cfg)) return CNNQ_EINVAL;
    if (cfg_bit_alloc(cfg) && !diag) return CNNQ_EINVAL;  // bit table lives in diag
    float* bits_ws = diag ? diag + (size_t)CNNQ_DIAG_BITS * C : nullptr;
    hipLaunchKernelGGL(k_params, dim3(1), dim3(param_threads(C)), 0, (hipStream_t)stream, stats, (int)C, *cfg, qp, diag,
                       bits_ws);
    return launch_status();
}

// Per-channel error columns of K candidate parameter tables (cnnq_qerr.hip.h): k_qerr -> k_qerr_fold.  The load shape is the
// plan's with at most two loads per lane and sample: the pass is bound by instruction issue, and its LDS tile (one fp32 entry
// per load slot and sum) has to leave room for several workgroups per CU.
static int qerr_plan(int64_t N, int64_t C, int64_t HW, bool aligned16, Variant* v, Geo* g) {
    if (N < 1 || C < 1 || HW < 1) return CNNQ_EINVAL;
    choose_variant(N, C, HW, aligned16, v);
    if (v->J > 2) v->J = 2;
    return make_geo(N, C, HW, *v, 0, C, /*max_groups=*/0, 0, 0, g);
}
static size_t qerr_records(int64_t N, int64_t C, int64_t HW, bool aligned16, int K) {
    Variant v;
    Geo g;
    if (qerr_plan(N, C, HW, aligned16, &v, &g) != 0) return 0;
    return (size_t)N * (size_t)(g.mode == 1 ? g.nb : 1) * (size_t)QE_NV(K) * (size_t)C;
}

size_t cnnq_pc_qerr_workspace(int64_t N, int64_t C, int64_t HW, int K) {
    if (K < 1 || K > 3) return 0;
    const size_t a = qerr_records(N, C, HW, true, K), u = qerr_records(N, C, HW, false, K);
    if (a == 0 || u == 0) return 0;
    return (a > u ? a : u) * sizeof(double);
}

int cnnq_pc_qerr(const float* x, int64_t N, int64_t C, int64_t HW, const float* qp, int K, const float* mm, void* ws, float* err,
                 void* stream) {
    if (!x || !qp || !ws || !err || K < 1 || K > 3 || N < 1 || C < 1 || HW < 1 || misaligned(ws, 8)) return CNNQ_EINVAL;
    Variant v;
    Geo g;
    const int rc = qerr_plan(N, C, HW, al16(x), &v, &g);
    if (rc) return rc;
    hipStream_t st = hs(stream);
    double* rec = reinterpret_cast<double*>(ws);
    with_shape(v, [&](auto s) {
        with_int<1, 2, 3>(K, [&](auto k) {
            with_bool(mm != nullptr, [&](auto m) {
                using S = decltype(s);
                constexpr int J = S::J > 2 ? 2 : S::J;          // qerr_plan's bound
                hipLaunchKernelGGL((k_qerr<S::VEC, S::A, J, decltype(k)::value, decltype(m)::value>), geo_grid(g), dim3(TPB), 0, st, x, g, qp, mm, rec);
            });
        });
    });
    const int rc2 = launch_status();
    if (rc2) return rc2;
    const int nb = g.mode == 1 ? g.nb : 1;
    with_int<1, 2, 3>(K, [&](auto k) {
        hipLaunchKernelGGL((k_qerr_fold<decltype(k)::value>), dim3((unsigned)((C + QF_CH - 1) / QF_CH)), dim3(TPB), 0, st, rec, (int)N, nb, (int)C,
                           (int)HW, err);
    });
    return launch_status();
}

// channel-slice views: `sample_stride` floats between consecutive samples (>= C*HW; 0 = contiguous).  The
// kernels only ever use the plane size as that stride, so a slice x[:, c0:c1] of a wider NCHW tensor is just
// (x + c0*HW, C = c1 - c0, sample_stride = C_total*HW).
static int strided_ok(int64_t C, int64_t HW, int64_t sample_stride) {
    return sample_stride == 0 || (sample_stride >= C * HW && sample_stride < ((int64_t)1 << 31));
}

int cnnq_pc_qdq_strided(const float* x, float* y, int64_t N, int64_t C, int64_t HW, int64_t sample_stride,
                        const float* qp, uint8_t* codes, uint64_t* hist, int reverse, void* stream) {
    if (!x || !y || !qp || !strided_ok(C, HW, sample_stride)) return CNNQ_EINVAL;
    Variant v;
    Geo g;
    const bool al = al16(x) && al16(y) && !misaligned(codes, 4) && sample_stride % 4 == 0;
    // the histogram variant zeroes and flushes an LDS table per workgroup: keep its workgroups long
    const int rc = plan(N, C, HW, al, reverse ? 1 : 0, &v, &g, /*fine=*/hist ? 0 : 1);
    if (rc) return rc;
    if (sample_stride) g.P = (int)sample_stride;
    return launch_qdq(x, y, g, v, qp, codes, reinterpret_cast<unsigned long long*>(hist), (hipStream_t)stream);
}

int cnnq_pc_qdq(const float* x, float* y, int64_t N, int64_t C, int64_t HW, const float* qp, uint8_t* codes,
                uint64_t* hist, int reverse, void* stream) {
    return cnnq_pc_qdq_strided(x, y, N, C, HW, 0, qp, codes, hist, reverse, stream);
}

// stored-format codes: bits = 4 (two per byte) or 8 (one per byte); x != NULL: x -> packed, else packed -> y
static int codes_launch(const float* x, float* y, uint8_t* packed, int64_t N, int64_t C, int64_t HW, const float* qp, int bits, void* stream) {
    const float* t = x ? x : y;
    if (!t || !packed || !qp) return CNNQ_EINVAL;
    if (HW % 4 != 0 || !al16(t) || misaligned(packed, bits == 4 ? 2 : 4)) return CNNQ_EINVAL;   // whole float4s
    Variant v;
    Geo g;
    const int rc = plan(N, C, HW, true, 0, &v, &g, /*fine=*/1);
    if (rc) return rc;
    with_int<4, 2, 1>(v.J, [&](auto j) {
        with_bool(bits == 4, [&](auto b4) {
            constexpr int J = decltype(j)::value, BITS = decltype(b4)::value ? 4 : 8;
            if (x) hipLaunchKernelGGL((k_q_pack4<J, BITS>), geo_grid(g), dim3(TPB), 0, hs(stream), x, packed, g, qp);
            else hipLaunchKernelGGL((k_unpack4_dq<J, BITS>), geo_grid(g), dim3(TPB), 0, hs(stream), packed, y, g, qp);
        });
    });
    return launch_status();
}

int cnnq_pc_quantize_pack4(const float* x, uint8_t* packed, int64_t N, int64_t C, int64_t HW, const float* qp,
                           void* stream) {
    return codes_launch(x, nullptr, packed, N, C, HW, qp, 4, stream);
}
int cnnq_pc_dequantize_pack4(const uint8_t* packed, float* y, int64_t N, int64_t C, int64_t HW, const float* qp,
                             void* stream) {
    return codes_launch(nullptr, y, const_cast<uint8_t*>(packed), N, C, HW, qp, 4, stream);
}
int cnnq_pc_quantize_u8(const float* x, uint8_t* codes, int64_t N, int64_t C, int64_t HW, const float* qp,
                        void* stream) {
    return codes_launch(x, nullptr, codes, N, C, HW, qp, 8, stream);
}
int cnnq_pc_dequantize_u8(const uint8_t* codes, float* y, int64_t N, int64_t C, int64_t HW, const float* qp,
                          void* stream) {
    return codes_launch(nullptr, y, const_cast<uint8_t*>(codes), N, C, HW, qp, 8, stream);
}

// variable-width packed codes (bit allocation as the stored format)
constexpr bool PACK_FLAT_DEFAULT = false;      // form 0 of the store direction stays k_pack_lean: k_pack_flat measured equal (cnnq_pack4.hip.h)
static int packed_launch(bool quant, const float* x, float* y, uint8_t* packed, int64_t N, int64_t C, int64_t HW,
                         const float* qp, const float* bits, const uint32_t* rowoff, void* stream, int form = 0) {
    if (!packed || !qp || !bits || !rowoff || N <= 0 || C <= 0 || HW <= 0) return CNNQ_EINVAL;
    if (C * HW >= (int64_t)1 << 31 || N >= (int64_t)1 << 31 || C > 65535) return CNNQ_ERANGE;
    // k adjacent channels per workgroup: >= 512 eight-element groups per sample (16 KB contiguous) when the layer has
    // the channels for it
    const int64_t ngroups = (HW + 7) / 8;
    int64_t k = (512 + ngroups - 1) / ngroups;
    if (k > MAXCH) k = MAXCH;
    if (k > C) k = C;
    const int64_t ncb = (C + k - 1) / k;
    // short workgroups in address order, like the other elementwise passes: ~14-28 KB of x each
    int64_t rows = (14336 + k * HW * 2) / (k * HW * 4);
    if (rows < 1) rows = 1;
    int64_t S = (N + rows - 1) / rows;
    if (S * ncb >= (int64_t)1 << 31) return CNNQ_ERANGE;
    if (k * ngroups >= (int64_t)1 << 24) return CNNQ_ERANGE;   // the in-loop index arithmetic is exact in fp32 below that
    // round 3: the lean form (one channel per wave, scalar parameters) for whole-float4 rows; form 1 forces the general
    // kernel, 2 the lean one (CNNQ_ENOTSUP when the geometry does not allow it)
    if (quant && (form == 0 || form == 3)) {
        // round 5: one-shot workgroups in address order of x (k_pack_flat); form 3 forces it (CNNQ_ENOTSUP for rows that are
        // not whole float4s, an unaligned x or stream, or 2^32 groups of 32 codes and more)
        const int64_t fgroups = (HW / 4 + 7) / 8, ftotal = N * C * fgroups;
        constexpr int FU = 4;
        const bool flat_ok = HW % 4 == 0 && al16(x) && ((uintptr_t)packed & 3) == 0 && ftotal < ((int64_t)1 << 32) - 32 * FU &&
                             fgroups < ((int64_t)1 << 24) - 32 * FU && N * C < ((int64_t)1 << 31);
        if (flat_ok && (PACK_FLAT_DEFAULT || form == 3)) {
            hipLaunchKernelGGL((k_pack_flat<FU>), dim3((unsigned)((ftotal + 32 * FU - 1) / (32 * FU))), dim3(TPB), 0, (hipStream_t)stream, x, packed,
                               (unsigned)(N * C), (int)C, (int)HW, (unsigned)fgroups, (unsigned)ftotal, qp, bits, rowoff);
            return launch_status();
        }
        if (form == 3) return CNNQ_ENOTSUP;
    }
    // the lean form of either direction (k_pack_lean / k_unpack_lean: one channel per wave) on the tensor t: whole-float4 rows of
    // an aligned t, or (RAG) any row of at least 8 elements: its slots are 4-byte aligned; the load direction reads the packed
    // stream as dwords.  1: launched; 0: the geometry does not allow it; CNNQ_ERANGE
    auto lean = [&](const float* t) -> int {
        const int64_t nsl = 2 * ngroups;
        const int64_t rpc = nsl <= 128 ? 128 / nsl : 1;
        const bool rag = HW % 4 != 0;
        if (!((rag ? HW >= 8 && !misaligned(t, 4) : al16(t)) && (quant || !misaligned(packed, 4)) && rpc * C * HW * 4 < ((int64_t)1 << 32))) return 0;
        // ~8 KB of x per wave (32 KB per workgroup of four adjacent channels), whole chunks of rows
        int64_t wave_bytes;                                                          // development knobs
        if (quant) { static const int64_t v = env_int("CNNQ_PACK_WAVE_BYTES", 8192); wave_bytes = v; }
        else { static const int64_t v = env_int("CNNQ_UNPACK_WAVE_BYTES", 8192); wave_bytes = v; }
        int64_t rpw = (wave_bytes + HW * 2) / (HW * 4);
        if (rpw < 1) rpw = 1;
        rpw = ((rpw + rpc - 1) / rpc) * rpc;
        const int64_t Sl = (N + rpw - 1) / rpw, ncb4 = (C + 3) / 4;
        if (Sl * ncb4 >= (int64_t)1 << 31) return CNNQ_ERANGE;
        const dim3 lgrid((unsigned)(Sl * ncb4)), lblock(TPB);
        with_bool(nsl <= 128, rag, [&](auto sh, auto r) {
            constexpr bool S = decltype(sh)::value, R = decltype(r)::value;
            if (quant) hipLaunchKernelGGL((k_pack_lean<S, R>), lgrid, lblock, 0, hs(stream), x, packed, (int)N, (int)C, (int)HW, (int)rpw, qp, bits, rowoff);
            else hipLaunchKernelGGL((k_unpack_lean<S, R>), lgrid, lblock, 0, hs(stream), packed, y, (int)N, (int)C, (int)HW, (int)rpw, qp, bits, rowoff);
        });
        return 1;
    };
    if (quant && form != 1) {
        const int rc = lean(x);
        if (rc) return rc < 0 ? rc : launch_status();
        if (form == 2) return CNNQ_ENOTSUP;
    }
    if (!quant && (form == 0 || form == 3)) {
        // round 4: one-shot workgroups in address order of y (k_unpack_flat); form 3 forces it (CNNQ_ENOTSUP when y is not
        // 16-byte aligned, the stream not 4-byte aligned, or the tensor has 2^32 elements or more)
        static const int allow_flat = env_int("CNNQ_UNPACK_FLAT", 1);               // development knob
        const int64_t total = N * C * HW;
        const bool flat_ok = al16(y) && ((uintptr_t)packed & 3) == 0 && total < ((int64_t)1 << 32) - 1024 && N * C < ((int64_t)1 << 31);
        if (flat_ok && (allow_flat || form == 3)) {
            const unsigned total4 = (unsigned)((total + 3) / 4), tail = (unsigned)(total - (int64_t)(total4 - 1) * 4);
            hipStream_t fst = (hipStream_t)stream;
            static const int U = env_int("CNNQ_UNPACK_U", 4);                     // development knob: float4 per lane
            // R = 1: whole-float4 rows, 2: rows of at least 4 elements, 4: shorter ones; U = 8 exists for R = 1 alone, R = 4 takes U = 1
            with_int<1, 2, 4>(HW % 4 == 0 ? 1 : HW >= 4 ? 2 : 4, [&](auto r) {
                with_int<1, 2, 8, 4>(U, [&](auto u) {
                    constexpr int R = decltype(r)::value, UU = R == 4 ? 1 : (R == 2 && decltype(u)::value == 8) ? 4 : decltype(u)::value;
                    hipLaunchKernelGGL((k_unpack_flat<R, UU>), dim3((total4 + TPB * UU - 1) / (TPB * UU)), dim3(TPB), 0, fst, packed, y, (int)N, (int)C,
                                       (int)HW, qp, bits, rowoff, total4, tail);
                });
            });
            return launch_status();
        }
        if (form == 3) return CNNQ_ENOTSUP;
    }
    if (!quant && form != 1 && form != 3) {
        const int rc = lean(y);
        if (rc) return rc < 0 ? rc : launch_status();
        if (form == 2) return CNNQ_ENOTSUP;
    }
    const dim3 grid((unsigned)(ncb * S)), block(TPB);
    static const int64_t rows_min = env_int("CNNQ_PACK_ROWS_MIN", 256);   // development knob (slots per row)
    const bool rows_form = 2 * ngroups >= rows_min;
    hipStream_t st = (hipStream_t)stream;
    with_bool(quant, rows_form, [&](auto q, auto r) {
        hipLaunchKernelGGL((k_packed<decltype(q)::value, decltype(r)::value>), grid, block, 0, st, x, y, packed, (int)N, (int)C, (int)HW, (int)S, (int)k,
                           qp, bits, rowoff);
    });
    return launch_status();
}

int cnnq_pc_packed_layout(const float* bits, int64_t C, int64_t HW, uint32_t* rowoff, void* stream) {
    if (!bits || !rowoff || C <= 0 || HW <= 0 || C * HW >= (int64_t)1 << 31) return CNNQ_EINVAL;
    hipLaunchKernelGGL(k_packed_layout, dim3(1), dim3(PTPB), 0, (hipStream_t)stream, bits, (int)C, (int)HW, rowoff);
    return launch_status();
}

int cnnq_pc_quantize_packed(const float* x, uint8_t* packed, int64_t N, int64_t C, int64_t HW, const float* qp,
                            const float* bits, const uint32_t* rowoff, void* stream) {
    if (!x) return CNNQ_EINVAL;
    return packed_launch(true, x, nullptr, packed, N, C, HW, qp, bits, rowoff, stream);
}

// the same with the kernel form spelled out: 0 = the library's choice, 1 = the general kernel (any geometry), 2 = the
// lean kernel (one channel per wave; CNNQ_ENOTSUP for rows of fewer than 8 elements, or whole-float4 rows of an x that is not 16-byte aligned).  Same bytes.
int cnnq_pc_quantize_packed_form(const float* x, uint8_t* packed, int64_t N, int64_t C, int64_t HW, const float* qp,
                                 const float* bits, const uint32_t* rowoff, int form, void* stream) {
    if (!x || form < 0 || form > 3) return CNNQ_EINVAL;
    return packed_launch(true, x, nullptr, packed, N, C, HW, qp, bits, rowoff, stream, form);
}

int cnnq_pc_dequantize_packed(const uint8_t* packed, float* y, int64_t N, int64_t C, int64_t HW, const float* qp,
                              const float* bits, const uint32_t* rowoff, void* stream) {
    if (!y) return CNNQ_EINVAL;
    return packed_launch(false, nullptr, y, const_cast<uint8_t*>(packed), N, C, HW, qp, bits, rowoff, stream);
}

// the same with the kernel form spelled out (0 / 1 / 2 as in cnnq_pc_quantize_packed_form; the lean form needs a 4-byte
// aligned packed buffer on top of the conditions on y).  Same floats.
int cnnq_pc_dequantize_packed_form(const uint8_t* packed, float* y, int64_t N, int64_t C, int64_t HW, const float* qp,
                                   const float* bits, const uint32_t* rowoff, int form, void* stream) {
    if (!y || form < 0 || form > 3) return CNNQ_EINVAL;
    return packed_launch(false, nullptr, y, const_cast<uint8_t*>(packed), N, C, HW, qp, bits, rowoff, stream, form);
}

int cnnq_pc_minmax_strided(const float* x, int64_t N, int64_t C, int64_t HW, int64_t sample_stride, float* pmm,
                           void* stream) {
    if (!x || !pmm || !strided_ok(C, HW, sample_stride)) return CNNQ_EINVAL;
    Variant v;
    Geo g;
    const int rc = plan(N, C, HW, al16(x) && sample_stride % 4 == 0, 0, &v, &g);
    if (rc) return rc;
    if (sample_stride) g.P = (int)sample_stride;
    with_shape(v, [&](auto s) {
        with_bool(nt_loads(N * C * HW * 4), [&](auto nt) {
            using S = decltype(s);
            hipLaunchKernelGGL((k_minmax<S::VEC, S::A, S::J, decltype(nt)::value>), geo_grid(g), dim3(TPB), 0, hs(stream), x, g, pmm);
        });
    });
    return launch_status();
}

int cnnq_pc_minmax(const float* x, int64_t N, int64_t C, int64_t HW, float* pmm, void* stream) {
    return cnnq_pc_minmax_strided(x, N, C, HW, 0, pmm, stream);
}

int cnnq_pc_minmax_reduce(const float* pmm, int G, int64_t C, float* out, void* stream) {
    if (!pmm || !out || G <= 0 || C <= 0 || C >= ((int64_t)1 << 31)) return CNNQ_EINVAL;
    hipLaunchKernelGGL(k_minmax_reduce, dim3((unsigned)((C + TPB / 64 - 1) / (TPB / 64))), dim3(TPB), 0,
                       (hipStream_t)stream, pmm, G, (int)C, out);
    return launch_status();
}

int cnnq_pc_minmax_params(const float* pmm, int G, int64_t C, int num_bits, int positive, float* qp, void* stream) {
    if (!pmm || !qp || G <= 0 || C <= 0 || C >= ((int64_t)1 << 31) || num_bits < 1 || num_bits > 32)
        return CNNQ_EINVAL;
    hipLaunchKernelGGL(k_minmax_params, dim3((unsigned)((C + TPB / 64 - 1) / (TPB / 64))), dim3(TPB), 0,
                       (hipStream_t)stream, pmm, G, (int)C, num_bits, positive ? 1 : 0, qp);
    return launch_status();
}

int cnnq_pc_minmax_qdq(const float* x, float* y, int64_t N, int64_t C, int64_t HW, int num_bits, int positive,
                       float* pmm, float* qp, uint8_t* codes, uint64_t* hist, void* stream) {
    if (!x || !y || !pmm || !qp || num_bits < 1 || num_bits > 32) return CNNQ_EINVAL;
    if ((codes || hist) && num_bits > 8) return CNNQ_EINVAL;   // one byte per code, 256 histogram bins
    const int G = cnnq_pc_groups(N, C, HW, al16(x) ? 1 : 0);
    if (G <= 0) return g_error(G);
    int rc = cnnq_pc_minmax(x, N, C, HW, pmm, stream);
    if (rc) return rc;
    rc = cnnq_pc_minmax_params(pmm, G, C, num_bits, positive, qp, stream);
    if (rc) return rc;
    // descending address order: what the statistics pass read last is re-read first
    return cnnq_pc_qdq(x, y, N, C, HW, qp, codes, hist, /*reverse=*/1, stream);
}

// Config 2 in one launch and one read of x (cnnq_resident.hip.h)
int cnnq_pc_resident_describe(int64_t N, int64_t C, int64_t HW, int32_t out[8]) {
    if (!out) return CNNQ_EINVAL;
    WPlan p;
    const int rc = plan_whole(N, C, HW, true, &p);
    if (rc) return rc;
    const int32_t vals[8] = {p.A, p.T, p.K, p.g.k, p.g.CL, p.g.RL, p.wgs, 0};
    for (int i = 0; i < 8; ++i) out[i] = vals[i];
    return 0;
}

int cnnq_pc_minmax_qdq_resident(const float* x, float* y, int64_t N, int64_t C, int64_t HW, int num_bits, int positive,
                                float* qp, float* mm, void* stream) {
    if (!x || !y || !qp || num_bits < 1 || num_bits > 32) return CNNQ_EINVAL;
    WPlan p;
    const int rc = plan_whole(N, C, HW, al16(x) && al16(y), &p);
    if (rc) return rc;
    return launch_whole(x, y, p, num_bits, positive ? 1 : 0, qp, mm, (hipStream_t)stream);
}

// Config 2 in one launch and one read of x for tensors whose channels span several workgroups (cnnq_group.hip.h)
size_t cnnq_pc_group_workspace(int64_t N, int64_t C, int64_t HW) {
    // the larger of the two tilings a caller may end up with (flat tiles for the single launch, row pieces for
    // k_minmax_group's half of the multi-GPU path)
    GPlan p, q, r;
    const size_t a = plan_group(N, C, HW, true, &p, true, 1) ? 0 : p.ws_bytes;
    const size_t b = plan_group(N, C, HW, true, &q, /*allow_flat=*/false) ? 0 : q.ws_bytes;
    const size_t c = plan_sums(N, C, HW, true, &r, 1) ? 0 : r.ws_bytes;      // (straddling rows: shorter tiles, more members)
    return a > b ? (a > c ? a : c) : (b > c ? b : c);
}

// The exchange workspace lives in fine-grained (uncached) device memory: the pairs one XCD writes must be what
// another XCD reads in the same launch AND in the next one, whatever a per-XCD L2 (not coherent with the others;
// agent-scope acquires drop L1, not L2) may still hold of the same slots.  These are the only entry points of the
// path that allocate; they synchronise the device.
int cnnq_group_ws_alloc(size_t bytes, void** ws) {
    if (!ws || bytes < GRP_WS_PAIRS) return CNNQ_EINVAL;
    hipError_t e = hipExtMallocWithFlags(ws, bytes, hipDeviceMallocUncached);
    if (e != hipSuccess) return (int)e;
    e = hipMemset(*ws, 0, bytes);
    if (e != hipSuccess) return (int)e;
    return (int)hipDeviceSynchronize();
}

int cnnq_group_ws_free(void* ws) { return ws ? (int)hipFree(ws) : CNNQ_EINVAL; }

int cnnq_group_ws_status(const void* ws, uint32_t* status_host) {
    if (!ws || !status_host) return CNNQ_EINVAL;
    return (int)hipMemcpy(status_host, ws, sizeof(uint32_t), hipMemcpyDeviceToHost);
}

int cnnq_group_ws_status_clear(void* ws) {
    if (!ws) return CNNQ_EINVAL;
    const uint32_t zero = 0;
    return (int)hipMemcpy(ws, &zero, sizeof(uint32_t), hipMemcpyHostToDevice);   // synchronises, like the read
}

// tests: the regions every launch must leave zero - the header after the status word, the counter lines, the slots -
// copied to the host (synchronising) and counted: *nonzero_words_host = the 32-bit words that are not zero
int cnnq_group_ws_at_rest(const void* ws, uint64_t* nonzero_words_host) {
    if (!ws || !nonzero_words_host) return CNNQ_EINVAL;
    std::vector<uint32_t> h(GRP_WS_PAIRS / 4);
    const hipError_t e = hipMemcpy(h.data(), ws, GRP_WS_PAIRS, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return (int)e;
    // the fused per-tensor kernel's corner of the header works by epoch (k_pt_fused: the epoch word and the row records
    // are written before they are read in every launch, nothing there needs to be zero): not part of the invariant
    constexpr size_t ptf0 = PTF_OFF / 4, ptf1 = (PTF_OFF + 256 + (size_t)PTF_MAX_ROWS * 16) / 4;
    uint64_t n = 0;
    for (size_t i = 1; i < h.size(); ++i) n += (i < ptf0 || i >= ptf1) && h[i] != 0u;
    *nonzero_words_host = n;
    return 0;
}

#ifdef GRP_TRACE
// development build only (tools/trace_group.py; not declared in include/cnnq_hip.h, absent from the product library)
int cnnq_debug_group_trace(void* buf) {
    unsigned long long* p = reinterpret_cast<unsigned long long*>(buf);
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_grp_trace), &p, sizeof(p));
}
#endif

int cnnq_pc_group_describe(int64_t N, int64_t C, int64_t HW, int32_t out[8]) {
    if (!out) return CNNQ_EINVAL;
    GPlan p;
    const int rc = plan_group(N, C, HW, true, &p, true, 1);
    if (rc) return rc;
    const int32_t vals[8] = {p.v.A, p.K + p.KL, p.g.mode, p.g.S, p.g.ncb, p.Gs, p.ngroups, p.g.S * p.g.ncb};
    for (int i = 0; i < 8; ++i) out[i] = vals[i];
    return 0;
}

int cnnq_pc_minmax_qdq_group(const float* x, float* y, int64_t N, int64_t C, int64_t HW, int num_bits, int positive,
                             void* ws, float* qp, float* mm, unsigned flags, void* stream) {
    if (!x || !y || !ws || !qp || num_bits < 1 || num_bits > 32 || misaligned(ws, 128)) return CNNQ_EINVAL;
    GPlan p;
    const int rc = plan_group(N, C, HW, al16(x) && al16(y), &p, true, flat_lds_rows(0, false));
    if (rc) return rc;
    return launch_group(x, y, p, num_bits, positive ? 1 : 0, ws, qp, mm, flags, (hipStream_t)stream);
}

// The two halves of config 2 around the cross-rank exchange, one call each: local extrema [2][C] of this rank's
// shard (k_minmax + k_minmax_reduce), and - after the all_gather - parameters from the W gathered records plus the
// fused Q/DQ.  pmm: workspace [G][2][C] floats; qp: workspace / output [CNNQ_NQP][C].
int cnnq_pc_minmax_local(const float* x, int64_t N, int64_t C, int64_t HW, float* pmm, float* local, void* stream) {
    if (!x || !pmm || !local) return CNNQ_EINVAL;
    const int G = cnnq_pc_groups(N, C, HW, al16(x) ? 1 : 0);
    if (G <= 0) return g_error(G);
    const int rc = cnnq_pc_minmax(x, N, C, HW, pmm, stream);
    if (rc) return rc;
    return cnnq_pc_minmax_reduce(pmm, G, C, local, stream);
}

// ... in ONE launch when the geometry has a group plan and the caller brought the exchange workspace (k_minmax_group:
// the last workgroup of a channel group to arrive folds the group's pairs), else the two launches above
int cnnq_pc_minmax_local_auto(const float* x, int64_t N, int64_t C, int64_t HW, float* pmm, void* gws, size_t gws_bytes,
                              float* local, void* stream) {
    if (!x || !local) return CNNQ_EINVAL;
    // tensors beyond the Infinity Cache keep the streaming k_minmax (6.5-6.9 TB/s against ~5.5 for 128 KB register
    // tiles; one launch boundary is nothing next to their 60+ us)
    static const int64_t max_bytes = env_int("CNNQ_LOCAL_GROUP_MAX_MB", 384) * ((int64_t)1 << 20);   // development knob
    if (gws && !misaligned(gws, 128) && N * C * HW * 4 <= max_bytes) {
        GPlan p;
        if (plan_group(N, C, HW, al16(x), &p, /*allow_flat=*/false) == 0 && p.ws_bytes <= gws_bytes)
            return launch_minmax_group(x, p, gws, local, (hipStream_t)stream);
    }
    return cnnq_pc_minmax_local(x, N, C, HW, pmm, local, stream);
}

// one launch: every workgroup of the fused Q/DQ derives the parameters of its channels from the W gathered records
int cnnq_pc_gathered_qdq(const float* x, float* y, int64_t N, int64_t C, int64_t HW, const float* gathered, int W,
                         int num_bits, int positive, float* qp, void* stream) {
    if (!x || !y || !gathered || W <= 0 || num_bits < 1 || num_bits > 32) return CNNQ_EINVAL;
    Variant v;
    Geo g;
    // the local statistics pass walked x ascending: descend, so that what it touched last is re-read first
    const int rc = plan(N, C, HW, al16(x) && al16(y), /*rev=*/1, &v, &g, /*fine=*/1);
    if (rc) return rc;
    const GathArgs ga{W, num_bits, positive ? 1 : 0, qp};
    return launch_qdq_gathered(x, y, g, v, gathered, ga, (hipStream_t)stream);
}

// Config 2 behind ONE call: the resident single launch when the shape has one, else the group-exchange single
// launch (needs gws), else the three-launch chain.  ws layout (floats): qp[CNNQ_NQP][C], mm[2][C], pmm[G][2][C].
struct MmWs {
    float *qp, *mm, *pmm;
    MmWs(float* ws, int64_t C) : qp(ws), mm(ws + (size_t)CNNQ_NQP * C), pmm(mm + 2 * (size_t)C) {}
    static size_t bytes(int G, int64_t C) { return ((size_t)CNNQ_NQP + 2 + 2 * (size_t)G) * (size_t)C * sizeof(float); }
};

size_t cnnq_pc_minmax_qdq_workspace(int64_t N, int64_t C, int64_t HW) {
    const int g1 = cnnq_pc_groups(N, C, HW, 1), g0 = cnnq_pc_groups(N, C, HW, 0);
    const int G = g1 > g0 ? g1 : g0;
    return G <= 0 ? 0 : MmWs::bytes(G, C);
}

// Config 2's single-launch route: the whole-channel form when the shape has one and it is not starved, else the group form,
// else whole.  group_ok: the caller's own group plan fits (each caller plans the group form with its own arguments, on purpose).
enum { ROUTE_NONE = 0, ROUTE_WHOLE, ROUTE_GROUP };
static int mm_route(int64_t N, int64_t C, int64_t HW, bool aligned16, bool group_ok, WPlan* wp) {
    // whole channels per workgroup needs no exchange, but with fewer channel blocks than ~3/4 of the CUs it leaves
    // the chip idle: [64,128,28,28] = 128 workgroups takes 17.8 us, the group form (1024 tiles) 13.4
    const bool whole_ok = plan_whole(N, C, HW, aligned16, wp) == 0;
    if (whole_ok && !(group_ok && wp->wgs < RES_MIN_WGS)) return ROUTE_WHOLE;
    return group_ok ? ROUTE_GROUP : whole_ok ? ROUTE_WHOLE : ROUTE_NONE;
}

int cnnq_pc_minmax_qdq_auto(const float* x, float* y, int64_t N, int64_t C, int64_t HW, int num_bits, int positive,
                            float* ws, void* gws, size_t gws_bytes, int allow_single_launch, void* stream) {
    if (!x || !y || !ws || num_bits < 1 || num_bits > 32 || C <= 0) return CNNQ_EINVAL;
    const MmWs w(ws, C);
    if (allow_single_launch) {
        const size_t gneed = gws ? cnnq_pc_group_workspace(N, C, HW) : 0;
        WPlan wp;
        int route = mm_route(N, C, HW, al16(x) && al16(y), gneed > 0 && gneed <= gws_bytes, &wp);
        if (route == ROUTE_GROUP) {
            const int rc = cnnq_pc_minmax_qdq_group(x, y, N, C, HW, num_bits, positive, gws, w.qp, w.mm, 0u, stream);
            if (rc != CNNQ_ENOTSUP) return rc;
            route = mm_route(N, C, HW, al16(x) && al16(y), false, &wp);      // no group plan for these pointers after all
        }
        if (route == ROUTE_WHOLE) return launch_whole(x, y, wp, num_bits, positive ? 1 : 0, w.qp, w.mm, hs(stream));
    }
    return cnnq_pc_minmax_qdq(x, y, N, C, HW, num_bits, positive, w.pmm, w.qp, nullptr, nullptr, stream);
}

// Config 2 in ONE launch with the outputs the chain form used to be needed for: the uint8 codes, the code histogram
// (-me: iq.py:586-587) and / or the packed 4-bit codes INSTEAD of y (4.5 bytes per element straight from
// x).  Routing as cnnq_pc_minmax_qdq_auto, without the chain: CNNQ_ENOTSUP when the shape has no single-launch kernel.
size_t cnnq_hist_replica_bytes(void) { return (size_t)XHIST_REPLICAS * 256 * sizeof(unsigned long long); }

int cnnq_pc_minmax_qdq_single(const float* x, float* y, int64_t N, int64_t C, int64_t HW, int num_bits, int positive,
                              void* gws, size_t gws_bytes, float* qp, float* mm, uint8_t* codes, uint64_t* hist_rep,
                              uint8_t* packed, void* stream) {
    if (!x || !qp || num_bits < 1 || num_bits > 32 || C <= 0) return CNNQ_EINVAL;
    if (packed ? (y || codes || hist_rep || num_bits > 4 || misaligned(packed, 2)) : !y) return CNNQ_EINVAL;
    if ((codes || hist_rep) && num_bits > 8) return CNNQ_EINVAL;
    if (misaligned(codes, 4) || misaligned(hist_rep, 8) || misaligned(gws, 128)) return CNNQ_EINVAL;
    const int out = packed ? 2 : (codes || hist_rep) ? 1 : 0;
    const XOut xo = xout(codes, hist_rep, packed);
    const bool al = al16(x) && (packed ? true : al16(y));
    GPlan gp;
    const bool group_ok = gws && plan_group(N, C, HW, al, &gp, true, flat_lds_rows(out, false)) == 0 && gp.ws_bytes <= gws_bytes;
    WPlan wp;
    switch (mm_route(N, C, HW, al, group_ok, &wp)) {
    case ROUTE_WHOLE: return launch_whole(x, y, wp, num_bits, positive ? 1 : 0, qp, mm, hs(stream), out, xo);
    case ROUTE_GROUP: return launch_group(x, y, gp, num_bits, positive ? 1 : 0, gws, qp, mm, 0u, hs(stream), out, xo);
    }
    return CNNQ_ENOTSUP;
}

// The same single launch when the batch is sharded over `world` GPUs (opt-in; csrc/cnnq_xrank.hip.h): x is this rank's
// shard, the channel extrema are exchanged with the other ranks through `windows` INSIDE the launch, y / qp / mm are
// what a single GPU holding the whole batch would produce.  CNNQ_ENOTSUP when the shape has no single-launch kernel
// (nothing is enqueued and no sequence number is consumed: the caller takes the collective path on every rank - the
// plan depends only on the shape and the alignment of x / y, which must agree between the ranks).
size_t cnnq_xrank_window_bytes(int world, int cmax) {
    return (world > 0 && cmax > 0) ? xr_window_bytes(world, cmax) : 0;
}

int cnnq_xrank_alloc(int world, int cmax, void** window, unsigned char handle[64]) {
    if (!window || !handle || world <= 0 || cmax <= 0) return CNNQ_EINVAL;
    const size_t bytes = xr_window_bytes(world, cmax);
    hipError_t e = hipExtMallocWithFlags(window, bytes, hipDeviceMallocUncached);
    if (e != hipSuccess) return (int)e;
    e = hipMemset(*window, 0, bytes);                  // an empty slot is zero
    hipIpcMemHandle_t h;
    if (e == hipSuccess) e = hipIpcGetMemHandle(&h, *window);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {                             // nothing is handed out on failure: the window is released here
        (void)hipFree(*window);
        *window = nullptr;
        return (int)e;
    }
    memcpy(handle, &h, 64);
    return 0;
}

// seq != 0: host numbering (seq_dev, if given, mirrors it; with `lean` no kernel is enqueued behind the launch: the caller passes
// zero_c, the channel count of the launch two back, and workgroup 0 cleans up); seq == 0: device numbering (k_xr_finish behind it)
static int xrank_launch(const float* x, float* y, int64_t N, int64_t C, int64_t HW, int num_bits, int positive, float* ws, void* gws,
                        size_t gws_bytes, void* const* windows, int rank, int world, int cmax, uint32_t seq, uint32_t* seq_dev,
                        uint32_t* status, int64_t timeout_ticks, uint8_t* codes, uint64_t* hist_rep, void* stream, int zero_c = 0,
                        bool lean = false) {
    if (!x || !y || !ws || num_bits < 1 || num_bits > 32 || C <= 0) return CNNQ_EINVAL;
    if (!windows || !status || world <= 0 || rank < 0 || rank >= world || (!seq && !seq_dev) || C > cmax || timeout_ticks <= 0) return CNNQ_EINVAL;
    if (misaligned(gws, 128)) return CNNQ_EINVAL;
    if ((codes || hist_rep) && num_bits > 8) return CNNQ_EINVAL;
    if (misaligned(codes, 4) || misaligned(hist_rep, 8) || misaligned(seq_dev, 4)) return CNNQ_EINVAL;
    const MmWs w(ws, C);                                  // the layout of cnnq_pc_minmax_qdq_auto's workspace
    float *const qp = w.qp, *const mm = w.mm, *const pmm = w.pmm;
    if (zero_c < 0 || zero_c > cmax || (lean && !seq)) return CNNQ_EINVAL;
    const XRank xr = xrank_args(windows, rank, world, cmax, seq, seq_dev, lean, zero_c, (int)C, 0, status, timeout_ticks);
    const int out = (codes || hist_rep) ? 1 : 0;
    const XOut xo = xout(codes, hist_rep);
    const bool al = al16(x) && al16(y);
    GPlan gp;
    const bool group_ok = gws && plan_group(N, C, HW, al, &gp) == 0 && gp.ws_bytes <= gws_bytes;
    WPlan wp;
    hipStream_t st = hs(stream);
    const int route = mm_route(N, C, HW, al, group_ok, &wp);
    int rc;
    if (route == ROUTE_WHOLE) rc = launch_whole(x, y, wp, num_bits, positive ? 1 : 0, qp, mm, st, out, xo, 0u, &xr);
    else if (route == ROUTE_GROUP) rc = launch_group(x, y, gp, num_bits, positive ? 1 : 0, gws, qp, mm, 0u, st, out, xo, &xr);
    else {
        // no single-launch kernel for this rank's shard (the ranks' shards may differ by a sample, and so may their plans):
        // the same window protocol around two passes - local extrema, one thread per channel pushes / waits / folds, Q/DQ
        // with the folded extrema as the only "gathered" record (codes / histogram: the parameter kernel + the fused Q/DQ,
        // which counts into the first replica table).  Every rank consumes the sequence number either way.
        rc = cnnq_pc_minmax_local_auto(x, N, C, HW, pmm, gws, gws_bytes, mm, stream);
        if (rc) return rc;
        hipLaunchKernelGGL(k_xr_exchange, dim3((unsigned)((C + TPB - 1) / TPB)), dim3(TPB), 0, st, mm, (int)C, xr);
        rc = launch_status();
        if (rc) return rc;
        if (!out) rc = cnnq_pc_gathered_qdq(x, y, N, C, HW, mm, 1, num_bits, positive, qp, stream);
        else {
            rc = cnnq_pc_minmax_params(mm, 1, C, num_bits, positive, qp, stream);
            if (!rc) rc = cnnq_pc_qdq(x, y, N, C, HW, qp, codes, hist_rep, 1, stream);
        }
    }
    if (rc) return rc;
    if (lean) return 0;                                   // host numbering, cleaned up by workgroup 0 of the launch after next
    // behind the launch: the slots of its parity back to zero (every reader of this rank is done), the device-side launch
    // number advanced
    hipLaunchKernelGGL(k_xr_finish, dim3(1), dim3(1024), 0, st, windows, rank, world, cmax, (int)C, seq, seq ? nullptr : seq_dev,
                       seq_dev ? seq_dev + 4 : nullptr);
    return launch_status();
}

// Round 5: ONE launch per tensor on the eager path.  seq: the host's launch number (1, 2, 3, ... the same on every rank);
// zero_c: the channel count C of the launch two back on this stream (0 for the first two launches): workgroup 0 zeroes the slots
// that launch used; seq_dev (may be NULL): device word that follows the host's count, so that a later captured launch
// (cnnq_pc_minmax_qdq_xrank_dev on the same word) continues the numbering.  seq == 0: device numbering as
// cnnq_pc_minmax_qdq_xrank_dev, plus the clean-up of zero_c (the first two launches after the switch).
int cnnq_pc_minmax_qdq_xrank_seq(const float* x, float* y, int64_t N, int64_t C, int64_t HW, int num_bits, int positive,
                                 float* ws, void* gws, size_t gws_bytes, void* const* windows, int rank, int world, int cmax,
                                 uint32_t seq, uint32_t* seq_dev, int zero_c, uint32_t* status, int64_t timeout_ticks, uint8_t* codes,
                                 uint64_t* hist_rep, void* stream) {
    if (!seq && !seq_dev) return CNNQ_EINVAL;
    return xrank_launch(x, y, N, C, HW, num_bits, positive, ws, gws, gws_bytes, windows, rank, world, cmax, seq, seq_dev, status,
                        timeout_ticks, codes, hist_rep, stream, zero_c, seq != 0);
}

int cnnq_pc_minmax_qdq_xrank(const float* x, float* y, int64_t N, int64_t C, int64_t HW, int num_bits, int positive,
                             float* ws, void* gws, size_t gws_bytes, void* const* windows, int rank, int world, int cmax,
                             uint32_t seq, uint32_t* status, int64_t timeout_ticks, void* stream) {
    if (!seq) return CNNQ_EINVAL;
    return xrank_launch(x, y, N, C, HW, num_bits, positive, ws, gws, gws_bytes, windows, rank, world, cmax, seq, nullptr, status,
                        timeout_ticks, nullptr, nullptr, stream);
}

int cnnq_pc_minmax_qdq_xrank_dev(const float* x, float* y, int64_t N, int64_t C, int64_t HW, int num_bits, int positive,
                                 float* ws, void* gws, size_t gws_bytes, void* const* windows, int rank, int world, int cmax,
                                 uint32_t* seq_dev, uint32_t* status, int64_t timeout_ticks, uint8_t* codes, uint64_t* hist_rep,
                                 void* stream) {
    if (!seq_dev) return CNNQ_EINVAL;
    return xrank_launch(x, y, N, C, HW, num_bits, positive, ws, gws, gws_bytes, windows, rank, world, cmax, 0u, seq_dev, status,
                        timeout_ticks, codes, hist_rep, stream);
}

// the replica tables of the single-launch kernels folded into one plain table hist[256] (+=: the caller zeroes it), the
// replicas left zero: a sharded run sums the ranks' tables before the entropy
int cnnq_hist_replicas_fold(uint64_t* hist_rep, uint64_t* hist, void* stream) {
    if (!hist_rep || !hist) return CNNQ_EINVAL;
    hipLaunchKernelGGL(k_hist_replicas_fold, dim3(1), dim3(TPB), 0, (hipStream_t)stream,
                       reinterpret_cast<unsigned long long*>(hist_rep), reinterpret_cast<unsigned long long*>(hist));
    return launch_status();
}

// entropy (bits) of the replica histogram the call above filled; the tables are zero again afterwards
// n sets of replica tables, back to back (cnnq_hist_replica_bytes each), in ONE launch: out[i] = the entropy of set i; all left zero
int cnnq_entropy_replicas_batch(uint64_t* hist_rep, int n, float* out, void* stream) {
    if (!hist_rep || !out || n <= 0) return CNNQ_EINVAL;
    hipLaunchKernelGGL(k_entropy_replicas, dim3((unsigned)n), dim3(TPB), 0, (hipStream_t)stream,
                       reinterpret_cast<unsigned long long*>(hist_rep), out);
    return launch_status();
}

int cnnq_entropy_replicas(uint64_t* hist_rep, float* out, void* stream) {
    if (!hist_rep || !out) return CNNQ_EINVAL;
    hipLaunchKernelGGL(k_entropy_replicas, dim3(1), dim3(TPB), 0, (hipStream_t)stream,
                       reinterpret_cast<unsigned long long*>(hist_rep), out);
    return launch_status();
}

// The whole dynamic ACIQ pipeline (iq.py:327-352 + 409-451) behind ONE call: statistics pass A, merge, pass B
// when b is needed, merge, parameters (ACIQ clipping, bit allocation, scale / zero point), fused Q/DQ - six
// launches (five since round 2: the first merge runs inside pass B), one host call, one caller workspace.  ws layout (doubles first): part[G][NMOM][C], mom[NMOM][C],
// part2[G][NDEV][C], then floats stats[NSTAT][C].
// (the channels_last form, cnnq_pc_aciq_qdq_nhwc, carves the same doubles with its slab count for G and keeps stats outside)
struct AciqWs {
    double *part, *mom, *part2;
    float* stats;
    AciqWs(void* ws, int G, int64_t C)
        : part(reinterpret_cast<double*>(ws)), mom(part + (size_t)G * CNNQ_NMOM * C), part2(mom + (size_t)CNNQ_NMOM * C),
          stats(reinterpret_cast<float*>(part2 + (size_t)G * CNNQ_NDEV * C)) {}
    static size_t bytes(size_t G, int64_t C, bool with_stats) {
        return (G * CNNQ_NMOM + CNNQ_NMOM + G * CNNQ_NDEV) * (size_t)C * sizeof(double) + (with_stats ? (size_t)CNNQ_NSTAT * (size_t)C * sizeof(float) : 0);
    }
};

size_t cnnq_pc_aciq_workspace(int64_t N, int64_t C, int64_t HW, int aligned16) {
    const int G = cnnq_pc_groups(N, C, HW, aligned16);
    return G <= 0 ? 0 : AciqWs::bytes((size_t)G, C, true);
}

int cnnq_pc_aciq_qdq(const float* x, float* y, int64_t N, int64_t C, int64_t HW, const cnnq_params_cfg* cfg, void* ws,
                     float* qp, float* diag, void* stream) {
    if (!x || !y || !cfg || !ws || !qp || misaligned(ws, 8)) return CNNQ_EINVAL;
    if (check_cfg(cfg)) return CNNQ_EINVAL;                                      // as cnnq_pc_params, before any launch
    const int G = cnnq_pc_groups(N, C, HW, al16(x) ? 1 : 0);
    if (G <= 0) return g_error(G);
    const AciqWs w(ws, G, C);
    const bool need_b = cfg->clip == 1 || (cfg_bit_alloc(cfg) && cfg->prior_is_b);
    // the merge kernels write every row of the table (zero for KURT, STD_POS; B without pass B)
    int rc = cnnq_pc_moments(x, N, C, HW, 0, w.part, stream);
    if (rc) return rc;
    if (need_b) {
        // pass B merges the pass-A records of its own channels in its prologue; one final merge writes all rows
        rc = launch_absdev(x, N, C, HW, nullptr, w.part, 0, w.part2, stream);
        if (rc) return rc;
        rc = combine_all(w.part, w.part2, G, C, 0, 0, w.mom, w.stats, stream);
    } else {
        rc = cnnq_pc_combine(w.part, G, C, 0, w.mom, w.stats, stream);
    }
    if (rc) return rc;
    rc = cnnq_pc_params(w.stats, C, cfg, qp, diag, stream);
    if (rc) return rc;
    // pass B walks the tensor descending, so the Q/DQ after it ascends; straight after pass A it descends
    return cnnq_pc_qdq(x, y, N, C, HW, qp, nullptr, nullptr, /*reverse=*/need_b ? 0 : 1, stream);
}

// the bit allocation in front of a fused launch (k_bitalloc on the std row): *bits = the table inside diag
static int launch_bitalloc(const float* stats, int64_t C, const cnnq_params_cfg* cfg, float* diag, float** bits, hipStream_t st) {
    *bits = diag + (size_t)CNNQ_DIAG_BITS * C;
    hipLaunchKernelGGL(k_bitalloc, dim3(1), dim3(param_threads(C)), 0, st, stats + (size_t)CNNQ_STAT_STD * C, (int)C, *cfg, *bits);
    return launch_status();
}
// launch_fused's arguments, mode 0 / mode 1; count_dev (the sharded forms): the global batch's count row, else count
static FusedArgs fused_aciq(float* stats, const float* bits, float* qp, float* diag, const cnnq_params_cfg* cfg, double count, const double* count_dev) {
    FusedArgs fa = {};
    fa.stats = stats;
    fa.bits = bits;
    fa.qp = qp;
    fa.diag = diag;
    fa.cfg = *cfg;
    fa.count = count;
    fa.count_dev = count_dev;
    return fa;
}
static FusedArgs fused_mt(float* stats, float* mt, const MtCfg& mcfg, uint64_t* hist, double count, const double* count_dev) {
    FusedArgs fa = {};
    fa.stats = stats;
    fa.count = count;
    fa.count_dev = count_dev;
    fa.mt = mt;
    fa.mcfg = mcfg;
    fa.hist = u64p(hist);
    return fa;
}
// omega and the clipping multiplier from the std alone (k_mt_params<GUESS>), in front of a fused mode-1 launch
static int launch_mt_guess(const float* stats, int64_t C, const MtCfg& mcfg, const double* tables, int ntab, float* mt, hipStream_t st) {
    hipLaunchKernelGGL(k_mt_params<true>, dim3(1), dim3(PTPB), 0, st, stats, (int)C, mcfg, tables, ntab, mt);
    return launch_status();
}

// Config 3 with pass B, the parameters and the Q/DQ in ONE launch (cnnq_aciq.hip.h): pass A -> merge -> (bit allocation)
// -> k_fused_flat / k_fused_group<MODE 0>: 12 instead of 16 bytes per element, four launches.  Laplace clipping on the per-channel
// route (clip == 1, no direct_range), bit allocation on the 'gaus' prior only (the 'laplace' prior IS b, which only exists
// inside the last launch).  CNNQ_ENOTSUP - nothing enqueued - for every other configuration, for shapes without a
// single-launch plan and for a `gws` too small: the caller takes cnnq_pc_aciq_qdq.  ws: part[G][CNNQ_NMOM][C] doubles
// (cnnq_pc_aciq_workspace covers it); stats [CNNQ_NSTAT][C] is written completely (KURT, STD_POS: zero).
int cnnq_pc_aciq_qdq_single(const float* x, float* y, int64_t N, int64_t C, int64_t HW, const cnnq_params_cfg* cfg, void* ws,
                            void* gws, size_t gws_bytes, float* stats, float* qp, float* diag, uint8_t* codes,
                            uint64_t* hist_rep, unsigned flags, void* stream) {
    if (!x || !y || !cfg || !ws || !stats || !qp || misaligned(ws, 8)) return CNNQ_EINVAL;
    if (check_cfg(cfg)) return CNNQ_EINVAL;
    if (misaligned(codes, 4) || misaligned(hist_rep, 8) || misaligned(gws, 128)) return CNNQ_EINVAL;
    const bool use_ba = cfg_bit_alloc(cfg);
    if (use_ba && !diag) return CNNQ_EINVAL;                     // the bit table lives in diag
    if (cfg->clip != 1 || cfg->direct_range || (use_ba && cfg->prior_is_b) || !gws) return CNNQ_ENOTSUP;
    const int out = (codes || hist_rep) ? 1 : 0;
    GPlan gp;
    if (!plan_fused(0, N, C, HW, al16(x) && al16(y), gws_bytes, out, &gp)) return CNNQ_ENOTSUP;
    const int G = cnnq_pc_groups(N, C, HW, al16(x) ? 1 : 0);
    if (G <= 0) return g_error(G);
    double* part = reinterpret_cast<double*>(ws);
    int rc = cnnq_pc_moments(x, N, C, HW, 0, part, stream);
    if (rc) return rc;
    rc = cnnq_pc_combine(part, G, C, 0, nullptr, stats, stream);
    if (rc) return rc;
    float* bits = nullptr;
    if (use_ba) rc = launch_bitalloc(stats, C, cfg, diag, &bits, hs(stream));
    if (rc) return rc;
    return launch_fused(0, x, y, gp, fused_aciq(stats, bits, qp, diag, cfg, (double)N * (double)HW, nullptr), gws, flags & 3u, hs(stream), out,
                        xout(codes, hist_rep));
}

// ... behind ONE call with the chain as the fallback: ws as cnnq_pc_aciq_qdq (cnnq_pc_aciq_workspace bytes); the
// statistics table is the one inside ws either way
int cnnq_pc_aciq_qdq_auto(const float* x, float* y, int64_t N, int64_t C, int64_t HW, const cnnq_params_cfg* cfg, void* ws,
                          void* gws, size_t gws_bytes, float* qp, float* diag, void* stream) {
    if (!x || !y || !cfg || !ws || !qp || misaligned(ws, 8)) return CNNQ_EINVAL;
    const int G = cnnq_pc_groups(N, C, HW, al16(x) ? 1 : 0);
    if (G <= 0) return g_error(G);
    float* stats = AciqWs(ws, G, C).stats;
    const int rc = cnnq_pc_aciq_qdq_single(x, y, N, C, HW, cfg, ws, gws, gws_bytes, stats, qp, diag, nullptr, nullptr, 0u, stream);
    if (rc != CNNQ_ENOTSUP) return rc;
    return cnnq_pc_aciq_qdq(x, y, N, C, HW, cfg, ws, qp, diag, stream);
}

// ---- round 6: configs 3 / 5 / 4 of a batch shard with the cross-rank exchange INSIDE the launches --------------------------------
// (cnnq_xrank.hip.h; the same windows, numbering and status word as config 2's cnnq_pc_minmax_qdq_xrank_seq / _dev).  One host
// call per tensor, ONE launch number, no collective: every statistic of the global batch travels through the windows.
static int xr_from_ctx(const cnnq_xrank_ctx* xc, int64_t C, XRank* xr) {
    if (!xc || !xc->windows || !xc->status || !xc->seq_dev || misaligned(xc->seq_dev, 4)) return CNNQ_EINVAL;
    if (xc->world <= 0 || xc->rank < 0 || xc->rank >= xc->world || xc->timeout_ticks <= 0 || C <= 0 || C * ST_XW > xc->cmax) return CNNQ_EINVAL;
    // the sums layout: eight words per channel; the fused kernels' sum |x - mean| is word 6
    *xr = xrank_args(xc->windows, xc->rank, xc->world, xc->cmax, xc->seq, xc->seq_dev, true, 0, (int)(C * ST_XW), (int)(C * (ST_XW_COUNT + 1)),
                     xc->status, xc->timeout_ticks);
    return 0;
}
// device numbering: the slots of the launch zeroed and the number advanced behind it (host numbering: the launch after next cleans up)
static int xr_finish_ctx(const cnnq_xrank_ctx* xc, int64_t C, hipStream_t st) {
    if (xc->seq) return 0;
    hipLaunchKernelGGL(k_xr_finish, dim3(1), dim3(1024), 0, st, xc->windows, xc->rank, xc->world, xc->cmax, (int)(C * ST_XW), 0u, xc->seq_dev,
                       xc->seq_dev + 4);
    return launch_status();
}
// pass A of a shard made global: k_moments -> k_xr_moments (the first kernel of the launch number: it runs the prologue)
static int xr_pass_a(const float* x, int64_t N, int64_t C, int64_t HW, int need_relu, double* part, int G, const XRank& xr, double* mom,
                     float* stats, void* stream) {
    int rc = cnnq_pc_moments(x, N, C, HW, need_relu, part, stream);
    if (rc) return rc;
    hipLaunchKernelGGL(k_xr_moments, dim3((unsigned)((C + XS_CPB - 1) / XS_CPB)), dim3(TPB), 0, (hipStream_t)stream, part, G, (int)C, need_relu, xr, mom, stats);
    return launch_status();
}
// pass B of a shard through the chain's kernel, its sums made global: k_absdev -> k_xr_devsums (rows B / KURT of stats)
static int xr_pass_b(const float* x, int64_t N, int64_t C, int64_t HW, int nw, int want_kurt, double* part2, int G, const double* mom,
                     XRank xr, float* stats, void* stream) {
    int rc = cnnq_pc_absdev(x, N, C, HW, stats, want_kurt, part2, stream);
    if (rc) return rc;
    xr.no_prologue = 1;
    hipLaunchKernelGGL(k_xr_devsums, dim3((unsigned)((C + 31) / 32)), dim3(TPB), 0, (hipStream_t)stream, part2, G, (int)C, nw, want_kurt,
                       mom + (size_t)CNNQ_MOM_COUNT * C, xr, stats);
    return launch_status();
}

// Config 3 of a batch shard (Laplace clipping, optional bit allocation on the 'gaus' prior), the whole pipeline: k_moments ->
// k_xr_moments (the six words of the pass-A record through the windows: the table of the GLOBAL batch on every rank) ->
// (k_bitalloc) -> ONE launch for the tile's sum |x - mean|, the local slot meeting, the ranks' sums through the windows, added in
// rank order, the parameters and the Q/DQ out of the registers - the four launches of one GPU, x read twice (12 bytes per
// element), no collective.  stats [CNNQ_NSTAT][C], mom [CNNQ_NMOM][C] (fp64), qp, diag: outputs, the same on every rank.  A
// shard without a single-launch plan runs k_absdev -> k_xr_devsums -> k_params -> k_qdq around the same slots, so the ranks need
// not agree on their plans; either way the call consumes ONE launch number.  ws: cnnq_pc_aciq_workspace bytes.  CNNQ_ENOTSUP
// (nothing enqueued, no number consumed) only for configurations cnnq_pc_aciq_qdq_single refuses too.
int cnnq_pc_aciq_fused_xrank(const float* x, float* y, int64_t N, int64_t C, int64_t HW, const cnnq_params_cfg* cfg, void* ws, void* gws,
                             size_t gws_bytes, float* stats, double* mom, float* qp, float* diag, const cnnq_xrank_ctx* xc, unsigned flags,
                             void* stream) {
    if (!x || !y || !cfg || !ws || !stats || !mom || !qp || misaligned(ws, 8) || misaligned(mom, 8)) return CNNQ_EINVAL;
    if (cfg->num_bits < 1 || cfg->num_bits > 8 || misaligned(gws, 128)) return CNNQ_EINVAL;
    const bool use_ba = cfg_bit_alloc(cfg);
    if (use_ba && !diag) return CNNQ_EINVAL;
    if (cfg->clip != 1 || cfg->direct_range || (use_ba && cfg->prior_is_b)) return CNNQ_ENOTSUP;
    XRank xr;
    int rc = xr_from_ctx(xc, C, &xr);
    if (rc) return rc;
    const int G = cnnq_pc_groups(N, C, HW, al16(x) ? 1 : 0);
    if (G <= 0) return g_error(G);
    hipStream_t st = (hipStream_t)stream;
    double* part = reinterpret_cast<double*>(ws);
    rc = xr_pass_a(x, N, C, HW, 0, part, G, xr, mom, stats, stream);
    if (rc) return rc;
    GPlan gp;
    if (gws && plan_fused(0, N, C, HW, al16(x) && al16(y), gws_bytes, 0, &gp)) {
        float* bits = nullptr;
        if (use_ba) rc = launch_bitalloc(stats, C, cfg, diag, &bits, st);
        if (rc) return rc;
        XRank xb = xr;
        xb.no_prologue = 1;
        rc = launch_fused(0, x, y, gp, fused_aciq(stats, bits, qp, diag, cfg, 0., mom + (size_t)CNNQ_MOM_COUNT * C), gws, flags & 3u, st, 0, XOut{}, &xb);
    } else {
        rc = xr_pass_b(x, N, C, HW, 1, 0, part, G, mom, xr, stats, stream);
        if (!rc) rc = cnnq_pc_params(stats, C, cfg, qp, diag, stream);
        if (!rc) rc = cnnq_pc_qdq(x, y, N, C, HW, qp, nullptr, nullptr, 0, stream);
    }
    if (rc) return rc;
    return xr_finish_ctx(xc, C, st);
}

// Config 5 of a batch shard (mid-tread, clip = 1): as above with the bin allocation (k_mt_params<GUESS> on the global std) in
// place of the bit allocation and MODE 1 of the fused kernels; mt [CNNQ_NMT][C] out; hist (optional, CNNQ_MT_HIST_WORDS(C),
// zeroed here) counts THIS rank's codes - sum it over the ranks, then cnnq_midtread_entropy_count with mom's COUNT row.
int cnnq_pc_midtread_fused_xrank(const float* x, float* y, int64_t N, int64_t C, int64_t HW, double target, int sym, const double* tables,
                                 int ntab, void* ws, void* gws, size_t gws_bytes, float* stats, double* mom, float* mt, uint64_t* hist,
                                 const cnnq_xrank_ctx* xc, unsigned flags, void* stream) {
    if (!x || !y || !tables || ntab < 2 || !ws || !stats || !mom || !mt || misaligned(ws, 8) || misaligned(hist, 8) || misaligned(mom, 8)) return CNNQ_EINVAL;
    if (misaligned(gws, 128)) return CNNQ_EINVAL;
    XRank xr;
    int rc = xr_from_ctx(xc, C, &xr);
    if (rc) return rc;
    const int G = cnnq_pc_groups(N, C, HW, al16(x) ? 1 : 0);
    if (G <= 0) return g_error(G);
    hipStream_t st = (hipStream_t)stream;
    if (hist && hipMemsetAsync(hist, 0, (size_t)CNNQ_MT_HIST_WORDS(C) * sizeof(uint64_t), st) != hipSuccess) return launch_status();
    double* part = reinterpret_cast<double*>(ws);
    rc = xr_pass_a(x, N, C, HW, 0, part, G, xr, mom, stats, stream);
    if (rc) return rc;
    GPlan gp;
    const MtCfg mcfg{target, 1, sym ? 1 : 0};
    if (gws && plan_fused(1, N, C, HW, al16(x) && al16(y), gws_bytes, hist ? 1 : 0, &gp)) {
        rc = launch_mt_guess(stats, C, mcfg, tables, ntab, mt, st);
        if (rc) return rc;
        XRank xb = xr;
        xb.no_prologue = 1;
        rc = launch_fused(1, x, y, gp, fused_mt(stats, mt, mcfg, hist, 0., mom + (size_t)CNNQ_MOM_COUNT * C), gws, flags & 3u, st, hist ? 1 : 0, XOut{}, &xb);
    } else {
        rc = xr_pass_b(x, N, C, HW, 1, 0, part, G, mom, xr, stats, stream);
        if (!rc) rc = cnnq_pc_midtread_params(stats, C, target, 1, sym, tables, ntab, mt, stream);
        if (!rc) rc = cnnq_pc_midtread_qdq(x, y, N, C, HW, mt, 1, nullptr, hist, stream);
    }
    if (rc) return rc;
    return xr_finish_ctx(xc, C, st);
}

// Config 4 of a batch shard: the seven statistics of the GLOBAL batch from ONE read of this rank's shard (k_stats_flat with the
// cross-rank stage: both phases' folds exchanged inside the launch; eight slots per channel, 8 C <= cmax).  stats [CNNQ_NSTAT][C]
// and mom [CNNQ_NMOM][C] are the global batch's on every rank.  A shard without a flat-tile plan (or with more than 256 tiles per
// channel) runs the chain's two passes with their records made global by k_xr_moments / k_xr_devsums around the same slots -
// four launches, no collective (ws: cnnq_pc_stats_workspace bytes).  ONE launch number per call.
int cnnq_pc_stats_xrank(const float* x, int64_t N, int64_t C, int64_t HW, int need_b, int need_kurt, int need_relu, void* ws, void* gws,
                        size_t gws_bytes, double* mom, float* stats, const cnnq_xrank_ctx* xc, unsigned flags, void* stream) {
    if (!x || !stats || !mom || !ws || misaligned(ws, 8) || misaligned(gws, 128) || misaligned(mom, 8)) return CNNQ_EINVAL;
    XRank xr;
    int rc = xr_from_ctx(xc, C, &xr);
    if (rc) return rc;
    const int G = cnnq_pc_groups(N, C, HW, al16(x) ? 1 : 0);
    if (G <= 0) return g_error(G);
    hipStream_t st = (hipStream_t)stream;
    const int need_dev = (need_b || need_kurt) ? 1 : 0;
    GPlan gp;
    const bool planned = gws && plan_sums(N, C, HW, al16(x), &gp, 0) == 0 && gp.ws_bytes <= gws_bytes;
    const bool single = planned && gp.flat && !gp.KL && (gp.Gs <= ST_MAX_MEMBERS || (flags & 8u)) && slots_fit(gp, ST_LINE);
    const St1Args sa = st1_args(stats, mom, N, HW, need_b, need_kurt, need_relu);      // count: this rank's; the launch exchanges it with the sums
    rc = CNNQ_ENOTSUP;
    if (single) {
        rc = launch_stats_flat(x, gp, sa, gws, flags & 1u, false, st, &xr);
    } else if (planned && !gp.flat && ((flags & 8u) || stats_group_pays(gp, N, C, HW))) {
        rc = launch_stats_group(x, gp, sa, gws, gws_bytes, flags & 1u, st, &xr);       // CNNQ_ENOTSUP (nothing enqueued): the slots do not fit
    }
    if (rc == CNNQ_ENOTSUP) {
        const StatsWs w(ws, G, C);
        rc = xr_pass_a(x, N, C, HW, need_relu ? 1 : 0, w.part, G, xr, mom, stats, stream);
        if (!rc && need_dev) rc = xr_pass_b(x, N, C, HW, 2, need_kurt ? 1 : 0, w.part2, G, mom, xr, stats, stream);
    }
    if (rc) return rc;
    return xr_finish_ctx(xc, C, st);
}

int cnnq_pc_weight_correct(float* wq, int64_t C, int64_t HW, const float* stats_w, const float* stats_q, int vcorr,
                           int bcorr, void* stream) {
    if (!wq || !stats_w || !stats_q || C <= 0 || HW <= 0 || C > 65535 * 1024 || HW >= ((int64_t)1 << 31))
        return CNNQ_EINVAL;
    if (C > 65535) return CNNQ_ERANGE;
    int64_t bx = (HW + TPB - 1) / TPB;
    if (bx > 64) bx = 64;
    hipLaunchKernelGGL(k_weight_correct, dim3((unsigned)bx, (unsigned)C), dim3(TPB), 0, (hipStream_t)stream, wq, (int)C,
                       (int)HW, stats_w, stats_q, vcorr, bcorr);
    return launch_status();
}

// the bias-correction sums of x against y, or - qp != NULL - against the Q/DQ of x computed in flight
static int bcorr_sums_launch(const float* x, const float* y, bool aligned16, int64_t N, int64_t C, int64_t HW, const float* qp, int relu_first,
                             double* part3, void* stream) {
    Variant v;
    Geo g;
    const int rc = plan(N, C, HW, aligned16, 0, &v, &g);
    if (rc) return rc;
    with_shape(v, [&](auto s) {
        with_bool(qp != nullptr, qp && nt_loads(N * C * HW * 4), [&](auto q, auto nt) {
            using S = decltype(s);
            constexpr bool Q = decltype(q)::value, NT = decltype(nt)::value;
            if constexpr (Q || !NT)                                 // two tensors to read: plain loads
                hipLaunchKernelGGL((k_bcorr_sums<S::VEC, S::A, S::J, Q, NT>), geo_grid(g), dim3(TPB), 0, hs(stream), x, y, g, relu_first, qp, part3);
        });
    });
    return launch_status();
}

int cnnq_pc_bcorr_sums(const float* x, const float* y, int64_t N, int64_t C, int64_t HW, int relu_first,
                       double* part3, void* stream) {
    if (!x || !y || !part3) return CNNQ_EINVAL;
    return bcorr_sums_launch(x, y, al16(x) && al16(y), N, C, HW, nullptr, relu_first, part3, stream);
}

int cnnq_pc_qdq_bcorr_sums(const float* x, int64_t N, int64_t C, int64_t HW, const float* qp, int relu_first,
                           double* part3, void* stream) {
    if (!x || !qp || !part3) return CNNQ_EINVAL;
    return bcorr_sums_launch(x, nullptr, al16(x), N, C, HW, qp, relu_first, part3, stream);
}

int cnnq_pc_qdq_bcorr(const float* x, float* y, int64_t N, int64_t C, int64_t HW, const float* qp, const float* bias,
                      int reverse, void* stream) {
    if (!x || !y || !qp || !bias) return CNNQ_EINVAL;
    Variant v;
    Geo g;
    const int rc = plan(N, C, HW, al16(x) && al16(y), reverse != 0, &v, &g, /*fine=*/1);
    if (rc) return rc;
    with_shape(v, [&](auto s) {
        using S = decltype(s);
        hipLaunchKernelGGL((k_qdq_bias<S::VEC, S::A, S::J>), geo_grid(g), dim3(TPB), 0, hs(stream), x, y, g, qp, bias);
    });
    return launch_status();
}

int cnnq_pc_bcorr_bias(const double* part3, int G, int64_t C, double* sums, float* bias, void* stream) {
    if (!part3 || G <= 0 || C <= 0 || C >= ((int64_t)1 << 31) || (!sums && !bias)) return CNNQ_EINVAL;
    hipLaunchKernelGGL(k_bcorr_bias, dim3((unsigned)((C + TPB / 64 - 1) / (TPB / 64))), dim3(TPB), 0, (hipStream_t)stream, part3, G,
                       (int)C, sums, bias);
    return launch_status();
}

int cnnq_pc_bcorr_apply(float* y, int64_t N, int64_t C, int64_t HW, const float* bias, void* stream) {
    if (!y || !bias) return CNNQ_EINVAL;
    Variant v;
    Geo g;
    const int rc = plan(N, C, HW, al16(y), 0, &v, &g, /*fine=*/1);
    if (rc) return rc;
    with_shape(v, [&](auto s) {
        using S = decltype(s);
        hipLaunchKernelGGL((k_bcorr_apply<S::VEC, S::A, S::J>), geo_grid(g), dim3(TPB), 0, hs(stream), y, g, bias);
    });
    return launch_status();
}

int cnnq_pc_midtread_params(const float* stats, int64_t C, double target, int clip, int sym, const double* tables,
                            int ntab, float* mt, void* stream) {
    if (!stats || !mt || !tables || ntab < 2 || C <= 0 || C >= ((int64_t)1 << 31)) return CNNQ_EINVAL;
    const MtCfg cfg{target, clip ? 1 : 0, sym ? 1 : 0};
    hipLaunchKernelGGL(k_mt_params<false>, dim3(1), dim3(PTPB), 0, (hipStream_t)stream, stats, (int)C, cfg, tables, ntab, mt);
    return launch_status();
}

int cnnq_pc_midtread_qdq(const float* x, float* y, int64_t N, int64_t C, int64_t HW, const float* mt, int clip,
                         float* codes, uint64_t* hist, void* stream) {
    if (!x || !y || !mt) return CNNQ_EINVAL;
    Variant v;
    Geo g;
    // short tiles in address order (14 KB); 56 KB with the histogram, whose per-workgroup flush - one global atomic per
    // live bin - wants fewer workgroups (swept 14 .. 448 KB on VGG-16 b512: 21.7 / 20.2 / 19.4 / 19.5 / 20.3 / 20.9 ms)
    const int rc = plan(N, C, HW, al16(x) && al16(y) && (!codes || al16(codes)), 0, &v, &g, /*fine=*/hist ? 57344 : 1);
    if (rc) return rc;
    const int total = g.S * g.ncb;
    unsigned long long* h = u64p(hist);
    with_shape(v, [&](auto s) {
        with_bool(clip != 0, h != nullptr, codes != nullptr, [&](auto cl, auto hi, auto co) {
            using S = decltype(s);
            hipLaunchKernelGGL((k_mt_qdq<S::VEC, S::A, S::J, decltype(cl)::value, decltype(hi)::value, decltype(co)::value>), dim3((unsigned)total),
                               dim3(TPB), 0, hs(stream), x, y, g, mt, codes, h, total);
        });
    });
    return launch_status();
}

// Config 5 with pass B, the step sizes / clamp bounds and the quantization in ONE launch (cnnq_aciq.hip.h, MODE 1): pass A ->
// merge -> k_mt_params<GUESS> (omega and the clipping multiplier need nothing but the std) -> k_fused_flat / k_fused_group:
// 12 instead of 16 bytes per element.  clip = 1 only (without clipping nothing needs pass B).  hist (optional,
// CNNQ_MT_HIST_WORDS(C) words) is zeroed here.  CNNQ_ENOTSUP - nothing enqueued - for shapes without a single-launch plan or a
// gws that is NULL / too small: the caller takes pc_stats -> cnnq_pc_midtread_params -> cnnq_pc_midtread_qdq.
int cnnq_pc_midtread_qdq_single(const float* x, float* y, int64_t N, int64_t C, int64_t HW, double target, int sym,
                                const double* tables, int ntab, void* ws, void* gws, size_t gws_bytes, float* stats, float* mt,
                                uint64_t* hist, unsigned flags, void* stream) {
    if (!x || !y || !tables || ntab < 2 || !ws || !stats || !mt || misaligned(ws, 8) || misaligned(hist, 8)) return CNNQ_EINVAL;
    if (misaligned(gws, 128)) return CNNQ_EINVAL;
    if (!gws) return CNNQ_ENOTSUP;
    GPlan gp;
    if (!plan_fused(1, N, C, HW, al16(x) && al16(y), gws_bytes, hist ? 1 : 0, &gp)) return CNNQ_ENOTSUP;
    const int G = cnnq_pc_groups(N, C, HW, al16(x) ? 1 : 0);
    if (G <= 0) return g_error(G);
    double* part = reinterpret_cast<double*>(ws);
    hipStream_t st = hs(stream);
    if (hist && hipMemsetAsync(hist, 0, (size_t)CNNQ_MT_HIST_WORDS(C) * sizeof(uint64_t), st) != hipSuccess) return launch_status();
    int rc = cnnq_pc_moments(x, N, C, HW, 0, part, stream);
    if (rc) return rc;
    rc = cnnq_pc_combine(part, G, C, 0, nullptr, stats, stream);
    if (rc) return rc;
    const MtCfg mcfg{target, 1, sym ? 1 : 0};
    rc = launch_mt_guess(stats, C, mcfg, tables, ntab, mt, st);
    if (rc) return rc;
    return launch_fused(1, x, y, gp, fused_mt(stats, mt, mcfg, hist, (double)N * (double)HW, nullptr), gws, flags & 3u, st, hist ? 1 : 0, XOut{});
}

int cnnq_midtread_entropy(const uint64_t* hist, const float* mt, int64_t C, int64_t total, float* out, void* stream) {
    if (!hist || !mt || !out || C <= 0 || total <= 0) return CNNQ_EINVAL;
    hipLaunchKernelGGL(k_mt_entropy, dim3(1), dim3(PTPB), 0, (hipStream_t)stream,
                       reinterpret_cast<const unsigned long long*>(hist), mt, (int)C, (double)total, out);
    return launch_status();
}

// the same with the element count taken from device memory: count[0] elements per channel (row CNNQ_MOM_COUNT of the merged
// moment record of a batch-sharded run, whose global batch size only the device knows exactly - shards may differ by a sample)
int cnnq_midtread_entropy_count(const uint64_t* hist, const float* mt, int64_t C, const double* count, float* out, void* stream) {
    if (!hist || !mt || !out || !count || misaligned(count, 8) || C <= 0) return CNNQ_EINVAL;
    hipLaunchKernelGGL(k_mt_entropy, dim3(1), dim3(PTPB), 0, (hipStream_t)stream,
                       reinterpret_cast<const unsigned long long*>(hist), mt, (int)C, 0., out, count);
    return launch_status();
}

// the entropies of n histograms of the mid-tread path in ONE launch (n <= 16; the arrays are host arrays of n entries)
int cnnq_midtread_entropy_batch(int n, const uint64_t* const* hist, const float* const* mt, const int64_t* C, const int64_t* total,
                                float* out, void* stream) {
    if (n <= 0 || n > MT_ENT_BATCH || !hist || !mt || !C || !total || !out) return CNNQ_EINVAL;
    MtEntBatch b = {};
    for (int i = 0; i < n; ++i) {
        if (!hist[i] || !mt[i] || C[i] <= 0 || total[i] <= 0) return CNNQ_EINVAL;
        b.hist[i] = reinterpret_cast<const unsigned long long*>(hist[i]);
        b.mt[i] = mt[i];
        b.C[i] = (int)C[i];
        b.total[i] = (double)total[i];
    }
    hipLaunchKernelGGL(k_mt_entropy_batch, dim3((unsigned)n), dim3(PTPB), 0, (hipStream_t)stream, b, out);
    return launch_status();
}

int cnnq_entropy(const uint64_t* hist, int nbins, float* out, void* stream) {
    if (!hist || !out || nbins <= 0) return CNNQ_EINVAL;
    hipLaunchKernelGGL(k_entropy, dim3(1), dim3(TPB), 0, (hipStream_t)stream,
                       reinterpret_cast<const unsigned long long*>(hist), nbins, out);
    return launch_status();
}

int cnnq_pt_setup(const float* range_offset_host, const float* stats, int64_t stats_stride, int rows, int rows_mode,
                  int zero_min, int num_bits, int int_exp, int enforce_true_zero, float* ptp, void* stream) {
    if (!ptp || num_bits < 1 || num_bits > 31) return CNNQ_EINVAL;
    if (!range_offset_host && (!stats || rows <= 0 || stats_stride < rows)) return CNNQ_EINVAL;
    const float hr = range_offset_host ? range_offset_host[0] : 0.f;
    const float ho = range_offset_host ? range_offset_host[1] : 0.f;
    hipLaunchKernelGGL(k_pt_setup, dim3(1), dim3(64), 0, (hipStream_t)stream, range_offset_host ? 1 : 0, hr, ho,
                       stats, stats_stride, rows, rows_mode, zero_min, num_bits, int_exp, enforce_true_zero, ptp);
    return launch_status();
}

// config 1 behind one call AND one launch (k_pt_fused): x viewed as [rows][n / rows]; rows_mode 0: batch mean of the
// per-row extrema (conv activations, iq.py:515-526), 1: the tensor's extrema.  gws: the exchange workspace of
// cnnq_group_ws_alloc (its header region: an epoch word and row records that every launch writes
// before it reads - nothing there has to be zero - and the counter lines, zero between launches).  ptp_out (may be NULL): the eight parameters
// cnnq_pt_setup would have written.  CNNQ_ENOTSUP: shapes the kernel does not take (rows not whole float4s, more than
// 1024 rows, unaligned pointers, more 16 KB tiles than the workspace has records for) - use cnnq_pc_minmax + cnnq_pc_minmax_reduce + cnnq_pt_setup + cnnq_pt_qdq.
int cnnq_pt_minmax_qdq_fused(const float* x, float* y, int64_t n, int rows, int rows_mode, int zero_min, int num_bits,
                             int int_exp, int enforce_true_zero, void* gws, size_t gws_bytes, float* ptp_out, void* stream) {
    if (!x || !y || !gws || gws_bytes < GRP_WS_PAIRS || n <= 0 || rows <= 0 || num_bits < 1 || num_bits > 31 || misaligned(gws, 128)) return CNNQ_EINVAL;
    if (n % rows) return CNNQ_EINVAL;
    const int64_t L = n / rows;
    if (L % 4 || rows > PTF_MAX_ROWS || !al16(x) || !al16(y) || L / 4 >= ((int64_t)1 << 31)) return CNNQ_ENOTSUP;
    const int64_t L4 = L / 4;
    const int64_t tpr = (L4 + PTF_TILE4 - 1) / PTF_TILE4;
    if (tpr * rows >= ((int64_t)1 << 31) - 64) return CNNQ_ENOTSUP;
    if ((size_t)(tpr * rows) * sizeof(uint4) > gws_bytes - GRP_WS_PAIRS) return CNNQ_ENOTSUP;     // one record per tile
    char* base = reinterpret_cast<char*>(gws) + PTF_OFF;
    PtfWs w;
    w.status = reinterpret_cast<unsigned*>(gws);
    w.cnt = reinterpret_cast<unsigned*>(reinterpret_cast<char*>(gws) + GRP_WS_HDR);
    w.epoch = reinterpret_cast<unsigned*>(base);
    w.rows = reinterpret_cast<unsigned*>(base + 256);
    w.recs = reinterpret_cast<uint4*>(reinterpret_cast<char*>(gws) + GRP_WS_PAIRS);   // write-before-read: garbage-tolerant
    static_assert(PTF_OFF + 256 + (size_t)PTF_MAX_ROWS * 16 <= GRP_WS_HDR, "the fused per-tensor region must fit the header");
    const int cus = chip_cus();
    // a co-resident grid: 4 workgroups per CU of the 5 that fit (83 VGPRs, 13 KB of LDS), fewer when the tensor is small
    const int64_t ntiles = tpr * rows;
    int64_t G = (int64_t)cus * 4;
    if (G > GRP_GS_MAX * 2) G = GRP_GS_MAX * 2;
    if (G > ntiles) G = ntiles;
    const int64_t per = (ntiles + G - 1) / G;
    G = (ntiles + per - 1) / per;
    if (grp_lines_per_group_host((int)G) > GRP_MAX_LINES) return CNNQ_ENOTSUP;
    const dim3 grid((unsigned)G), block(TPB);
    hipStream_t st = (hipStream_t)stream;
    // beyond the Infinity Cache the first sweep leaves nothing behind for the second: stream it
    with_bool(n * 4 > ((int64_t)192 << 20), [&](auto nt) {
        hipLaunchKernelGGL(k_pt_fused<decltype(nt)::value>, grid, block, 0, st, x, y, rows, (unsigned)L4, (unsigned)tpr, (unsigned)per, w, rows_mode,
                           zero_min, num_bits, int_exp, enforce_true_zero, ptp_out);
    });
    return launch_status();
}

// fp32: float4 or single elements; bf16 / fp16 (cnnq_half.hip.h): eight elements or one
static int pt_qdq_launch(const void* x, void* y, int dtype, int64_t n, const float* ptp, const float* noise, void* stream);

int cnnq_pt_qdq(const float* x, float* y, int64_t n, const float* ptp, const float* noise, void* stream) {
    return pt_qdq_launch(x, y, CNNQ_DTYPE_F32, n, ptp, noise, stream);
}

int cnnq_kld_hist(const float* x, int64_t rows, int64_t len, const float* rowmm, uint32_t* hist, void* stream) {
    if (!x || !rowmm || !hist || rows <= 0 || len <= 0) return CNNQ_EINVAL;
    if (rows > 65535 || len >= ((int64_t)1 << 31)) return CNNQ_ERANGE;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(hist, 0, (size_t)rows * KB * sizeof(uint32_t), st) != hipSuccess) return launch_status();
    const dim3 grid((unsigned)((len + KCHUNK - 1) / KCHUNK), (unsigned)rows), block(TPB);
    if (al16(x) && len % 4 == 0)
        hipLaunchKernelGGL((k_kld_hist<4>), grid, block, 0, st, x, len, rowmm, (int)rows, hist);
    else
        hipLaunchKernelGGL((k_kld_hist<1>), grid, block, 0, st, x, len, rowmm, (int)rows, hist);
    return launch_status();
}

// bf16 / fp16 rows where they lie (cnnq_half_kld.hip.h): cnnq_kld_hist's checks, zeroing and grid
int cnnq_kld_hist_dt(const void* x, int dtype, int64_t rows, int64_t len, const float* rowmm, uint32_t* hist, void* stream) {
    if (!dtype_ok(dtype)) return CNNQ_EINVAL;
    if (dtype == CNNQ_DTYPE_F32) return cnnq_kld_hist(static_cast<const float*>(x), rows, len, rowmm, hist, stream);
    if (!x || !rowmm || !hist || rows <= 0 || len <= 0) return CNNQ_EINVAL;
    if (rows > 65535 || len >= ((int64_t)1 << 31)) return CNNQ_ERANGE;
    if (misaligned(x, 2)) return CNNQ_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(hist, 0, (size_t)rows * KB * sizeof(uint32_t), st) != hipSuccess) return launch_status();
    const dim3 grid((unsigned)((len + KCHUNK - 1) / KCHUNK), (unsigned)rows), block(TPB);
    const uint16_t* xh = static_cast<const uint16_t*>(x);
    if (dtype == CNNQ_DTYPE_BF16)
        hipLaunchKernelGGL((k_h_kld_hist<HBf16>), grid, block, 0, st, xh, len, rowmm, (int)rows, hist);
    else
        hipLaunchKernelGGL((k_h_kld_hist<HF16>), grid, block, 0, st, xh, len, rowmm, (int)rows, hist);
    return launch_status();
}

int cnnq_kld_search(const uint32_t* hist, int64_t rows, const float* rowmm, double* div, double* out, void* stream) {
    if (!hist || !rowmm || !div || !out || rows <= 0) return CNNQ_EINVAL;
    if (rows > 65535) return CNNQ_ERANGE;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_kld_search, dim3(KC, (unsigned)rows), dim3(TPB), 0, st, hist, div);
    hipLaunchKernelGGL(k_kld_pick, dim3((unsigned)rows), dim3(64), 0, st, div, rowmm, (int)rows, out);
    return launch_status();
}

// ---- the windows of the in-launch cross-rank exchange: a peer's window mapped from its hipIpc handle, unmapped, the own
//      one released (with cnnq_xrank_alloc the only entry points of the multi-GPU path that allocate or synchronise)
int cnnq_xrank_open(const unsigned char handle[64], void** window) {
    if (!handle || !window) return CNNQ_EINVAL;
    hipIpcMemHandle_t h;
    memcpy(&h, handle, 64);
    return (int)hipIpcOpenMemHandle(window, h, hipIpcMemLazyEnablePeerAccess);
}
int cnnq_xrank_close(void* window) { return window ? (int)hipIpcCloseMemHandle(window) : CNNQ_EINVAL; }
int cnnq_xrank_free(void* window) { return window ? (int)hipFree(window) : CNNQ_EINVAL; }

// ---- activations of another element type (cnnq_half.hip.h): bf16 / fp16 x and y, fp32 tables ---------------------------------

// the common alignment of x and y in bytes (16 at most): what h_piece needs to know of the pointers
static int h_align(const void* x, const void* y) {
    const uintptr_t a = (uintptr_t)x | (uintptr_t)y | 16u;
    return (int)(a & (~a + 1));
}

// the fp32 plan's record count at either alignment (what bounds the extrema's partials, and what the fp32 correction chain
// writes); <= 0: cnnq_pc_groups' code
static int h_records_f32(int64_t N, int64_t C, int64_t HW) {
    const int g1 = cnnq_pc_groups(N, C, HW, 1), g0 = cnnq_pc_groups(N, C, HW, 0);
    return g1 > g0 ? g1 : g0;
}

// config 2's route for a bf16 / fp16 tensor: out = {1: the single launch k_h_whole / 2: the chain, piece width W, pieces per lane K
// (0 for the chain), workgroups of the Q/DQ launch}
static int h_route(int64_t N, int64_t C, int64_t HW, int align_bytes, int allow_single_launch, int32_t out[4]) {
    const int rc = cnnq_pc_groups(N, C, HW, 0);       // the fp32 entry points' geometry limits
    if (rc <= 0) return g_error(rc);
    const int w = h_piece(HW, (uintptr_t)align_bytes, 0);
    const bool whole = allow_single_launch && N * HW <= h_whole_cap(w);
    out[0] = whole ? 1 : 2;
    out[1] = w;
    out[2] = whole ? h_whole_k_rt(w) : 0;
    out[3] = whole ? (int32_t)C : (int32_t)(C * h_splits(N, C, HW, H_QDQ_ELEMS, N));
    return 0;
}

// the statistics launch of config 2 at piece width w, G the fp32 plan's record count: ~H_MM_ELEMS per workgroup - batch splits
// first, then (short batches: config 1's rows, N = 1) column splits of the rows
static HGeo h_geo_mm(int64_t N, int64_t C, int64_t HW, int w, int G) {
    const int total = h_splits(N * HW, C, 1, H_MM_ELEMS, G);
    const int bs = total < N ? total : (int)N, ppr = (int)(HW / w);
    return h_geo(N, C, HW, w, bs, total / bs < ppr ? total / bs : ppr);
}

// the statistics half of the chain: per-split extrema into pmm[S][2][C], S <= the fp32 plan's G (the callers' workspace rule)
static int h_minmax(const void* x, int dtype, int64_t N, int64_t C, int64_t HW, float* pmm, int* S, hipStream_t st) {
    const int G = h_records_f32(N, C, HW);
    if (G <= 0) return g_error(G);
    const int w = h_piece(HW, (uintptr_t)x, 0);
    const HGeo g = h_geo_mm(N, C, HW, w, G);
    *S = g.S * g.cs;
    return h_launch(dtype, w, x, [&](auto pc, const uint16_t* xh) {
        using P = decltype(pc);
        hipLaunchKernelGGL((k_h_minmax<typename P::T, P::W>), dim3((unsigned)(C * g.S * g.cs)), dim3(TPB), 0, st, xh, g, pmm);
    });
}

// the element-wise pass of every chain: ~H_QDQ_ELEMS per workgroup, whole rows
static HGeo h_geo_qdq(int64_t N, int64_t C, int64_t HW, int w) { return h_geo(N, C, HW, w, h_splits(N, C, HW, H_QDQ_ELEMS, N), 1); }

// pmm == NULL: the parameters from the table qp; else from the statistics partials pmm (published to ha.qp / ha.mm, k_h_qdq)
static int h_qdq(const void* x, void* y, int dtype, int64_t N, int64_t C, int64_t HW, const float* qp, const float* pmm, const HArgs& ha,
                 hipStream_t st) {
    const int rc = cnnq_pc_groups(N, C, HW, 0);    // the fp32 entry points' geometry limits
    if (rc <= 0) return g_error(rc);
    const int w = h_piece(HW, (uintptr_t)x, (uintptr_t)y);
    const HGeo g = h_geo_qdq(N, C, HW, w);
    return h_launch(dtype, w, x, y, [&](auto pc, const uint16_t* xh, uint16_t* yh) {
        using P = decltype(pc);
        hipLaunchKernelGGL((k_h_qdq<typename P::T, P::W>), dim3((unsigned)(C * g.S)), dim3(TPB), 0, st, xh, yh, g, qp, pmm, ha);
    });
}

int cnnq_pc_route_dt(int64_t N, int64_t C, int64_t HW, int align_bytes, int allow_single_launch, int32_t out[4]) {
    if (!out || !pow2(align_bytes)) return CNNQ_EINVAL;
    return h_route(N, C, HW, align_bytes, allow_single_launch, out);
}

int cnnq_pc_minmax_qdq_auto_dt(const void* x, void* y, int dtype, int64_t N, int64_t C, int64_t HW, int num_bits,
                               int positive, float* ws, void* gws, size_t gws_bytes, int allow_single_launch, void* stream) {
    if (!dtype_ok(dtype)) return CNNQ_EINVAL;
    if (dtype == CNNQ_DTYPE_F32)
        return cnnq_pc_minmax_qdq_auto(static_cast<const float*>(x), static_cast<float*>(y), N, C, HW, num_bits, positive, ws,
                                       gws, gws_bytes, allow_single_launch, stream);
    if (!x || !y || !ws || num_bits < 1 || num_bits > 32 || N <= 0 || C <= 0 || HW <= 0) return CNNQ_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const MmWs w(ws, C);                               // the layout of cnnq_pc_minmax_qdq_auto's workspace
    float *const qp = w.qp, *const mm = w.mm, *const pmm = w.pmm;
    int32_t route[4];
    int rc = h_route(N, C, HW, h_align(x, y), allow_single_launch, route);
    if (rc) return rc;
    if (route[0] == 1) {
        const HGeo g = h_geo(N, C, HW, route[1], 1, 1);
        const HArgs ha{0, num_bits, positive ? 1 : 0, qp, mm};
        const int w = route[1] >= 4 ? route[1] : 2;      // (no whole-tensor instance of single elements)
        return h_launch(dtype, w, x, y, [&](auto pc, const uint16_t* xh, uint16_t* yh) {
            using P = decltype(pc);
            if constexpr (P::W > 1)
                hipLaunchKernelGGL((k_h_whole<typename P::T, P::W, h_whole_k<P::W>()>), dim3((unsigned)C), dim3(HTPB), 0, st, xh, yh, g, ha);
        });
    }
    int S = 0;
    rc = h_minmax(x, dtype, N, C, HW, pmm, &S, st);
    if (rc) return rc;
    return h_qdq(x, y, dtype, N, C, HW, qp, pmm, HArgs{S, num_bits, positive ? 1 : 0, qp, mm}, st);
}

int cnnq_pc_qdq_dt(const void* x, void* y, int dtype, int64_t N, int64_t C, int64_t HW, const float* qp, uint8_t* codes,
                   uint64_t* hist, int reverse, void* stream) {
    if (!dtype_ok(dtype)) return CNNQ_EINVAL;
    if (dtype == CNNQ_DTYPE_F32)
        return cnnq_pc_qdq(static_cast<const float*>(x), static_cast<float*>(y), N, C, HW, qp, codes, hist, reverse, stream);
    if (!x || !y || !qp || N <= 0 || C <= 0 || HW <= 0) return CNNQ_EINVAL;
    if (codes || hist) return CNNQ_ENOTSUP;
    return h_qdq(x, y, dtype, N, C, HW, qp, nullptr, HArgs{}, (hipStream_t)stream);
}

int cnnq_pc_minmax_local_dt(const void* x, int dtype, int64_t N, int64_t C, int64_t HW, float* pmm, float* local,
                            void* stream) {
    if (!dtype_ok(dtype)) return CNNQ_EINVAL;
    if (dtype == CNNQ_DTYPE_F32) return cnnq_pc_minmax_local(static_cast<const float*>(x), N, C, HW, pmm, local, stream);
    if (!x || !pmm || !local || N <= 0 || C <= 0 || HW <= 0) return CNNQ_EINVAL;
    int S = 0;
    const int rc = h_minmax(x, dtype, N, C, HW, pmm, &S, (hipStream_t)stream);
    if (rc) return rc;
    return cnnq_pc_minmax_reduce(pmm, S, C, local, stream);
}

// ---- `-sm collect` on contiguous bf16 / fp16 activations (cnnq_half_stats.hip.h) ------------------------------------------------
// What the entry points, the workspace and the route functions of this section and the next open with: the checks of the shape
// and the dtype (ok: the function's own, refused with them), then - bf16 / fp16, and fp32 where f32_too - the fp32 entry points'
// geometry limits and the plan: the batch splits S and the column splits cs of the read-only launches (G = S * cs records per
// channel; h_stats_splits).  rc: what a refused call returns.
struct HPlan {
    int rc, S = 0, cs = 0;
    HPlan(int64_t N, int64_t C, int64_t HW, int dtype, bool ok, bool f32_too = false)
        : rc((!dtype_ok(dtype) || N < 1 || C < 1 || HW < 1 || !ok) ? CNNQ_EINVAL : 0) {
        if (rc || (dtype == CNNQ_DTYPE_F32 && !f32_too)) return;
        const int G0 = cnnq_pc_groups(N, C, HW, 0);
        if (G0 <= 0) rc = g_error(G0);
        else h_stats_splits(N, C, HW, &S, &cs);
    }
    int G() const { return S * cs; }
};

// ws, doubles: part[G][CNNQ_NMOM][C], mom[CNNQ_NMOM][C], part2[G][CNNQ_NDEV][C] (AciqWs without the table) with G = S * cs; fp32:
// what cnnq_pc_stats takes at either alignment
size_t cnnq_pc_stats_dt_workspace(int64_t N, int64_t C, int64_t HW, int dtype) {
    const HPlan p(N, C, HW, dtype, true);
    if (p.rc) return 0;
    if (dtype == CNNQ_DTYPE_F32) {
        const size_t a = cnnq_pc_stats_workspace(N, C, HW, 1), b = cnnq_pc_stats_workspace(N, C, HW, 0);
        return a > b ? a : b;
    }
    return AciqWs::bytes((size_t)p.G(), C, false);
}

// Which launches cnnq_pc_stats_dt makes for this geometry (host only): out = {piece width W, batch splits S, column splits,
// 1 - the native launches / 0 - a class of layer that did not win against the upcast route and stays there: h_stats_native, with
// the figures next to the rule}.  fp32: {0, the records of cnnq_pc_stats' own plan, 1, 1}.  cnnq_pc_stats_dt itself runs every class.
int cnnq_pc_route_stats_dt(int64_t N, int64_t C, int64_t HW, int dtype, int align_bytes, int32_t out[4]) {
    const HPlan p(N, C, HW, dtype, out && pow2(align_bytes), true);
    if (p.rc) return p.rc;
    const bool f32 = dtype == CNNQ_DTYPE_F32;
    out[0] = f32 ? 0 : h_piece(HW, (uintptr_t)align_bytes, 0);
    out[1] = f32 ? cnnq_pc_groups(N, C, HW, align_bytes >= 16) : p.S;
    out[2] = f32 ? 1 : p.cs;
    out[3] = h_stats_native(N, C, HW, dtype);
    return 0;
}

// smpc.py:45-79 on x[N][C][HW] of bf16 / fp16: k_h_moments -> k_combine(has_relu) (-> k_h_absdev on the merged table ->
// k_combine_dev(want_kurt); need_b or need_kurt), two or four launches
int cnnq_pc_stats_dt(const void* x, int dtype, int64_t N, int64_t C, int64_t HW, int need_b, int need_kurt, int need_relu, void* ws,
                     double* mom, float* stats, void* stream) {
    const bool f32 = dtype == CNNQ_DTYPE_F32;
    const HPlan p(N, C, HW, dtype, x && ws && stats && !misaligned(ws, 8) && !misaligned(mom, 8) && (f32 || !misaligned(x, 2)));
    if (p.rc) return p.rc;
    if (f32) return cnnq_pc_stats(static_cast<const float*>(x), N, C, HW, need_b, need_kurt, need_relu, ws, mom, stats, stream);
    const int w = h_piece(HW, (uintptr_t)x, 0), G = p.G();
    const HGeo g = h_geo(N, C, HW, w, p.S, p.cs);
    const AciqWs a(ws, G, C);
    double* rec = mom ? mom : a.mom;
    const dim3 grid((unsigned)(C * G));
    hipStream_t st = hs(stream);
    int rc = h_launch(dtype, w, x, [&](auto pc, const uint16_t* xh) {
        with_bool(need_relu != 0, [&](auto relu) {
            using P = decltype(pc);
            hipLaunchKernelGGL((k_h_moments<typename P::T, P::W, decltype(relu)::value>), grid, dim3(TPB), 0, st, xh, g, a.part);
        });
    });
    if (!rc) rc = cnnq_pc_combine(a.part, G, C, need_relu ? 1 : 0, rec, stats, stream);
    if (rc || !(need_b || need_kurt)) return rc;
    rc = h_launch(dtype, w, x, [&](auto pc, const uint16_t* xh) {
        with_bool(need_kurt != 0, [&](auto kurt) {
            using P = decltype(pc);
            hipLaunchKernelGGL((k_h_absdev<typename P::T, P::W, decltype(kurt)::value>), grid, dim3(TPB), 0, st, xh, g, stats, a.part2);
        });
    });
    if (!rc) rc = cnnq_pc_combine_dev(a.part2, G, C, rec, need_kurt ? 1 : 0, nullptr, stats, stream);
    return rc;
}

// ---- `-sm collect -ce` on contiguous bf16 / fp16 activations (cnnq_half_qerr.hip.h) -----------------------------------------------
// the argument checks the three functions share, HPlan's with K: 0 - the plan exists (bf16 / fp16: N and C * HW below 2^31, so
// k_qerr_fold takes N, nb, C and HW as int and the grid C * S * nb stays in 32 bits by h_qe_splits)
static int h_qe_check(int64_t N, int64_t C, int64_t HW, int K, int dtype, bool ok) {
    return HPlan(N, C, HW, dtype, ok && K >= 1 && K <= 3).rc;
}

// ws, doubles: rec[N * nb][QE_NV(K)][C] with nb = h_qe_parts, not the alignment's; fp32: what cnnq_pc_qerr takes
size_t cnnq_pc_qerr_dt_workspace(int64_t N, int64_t C, int64_t HW, int K, int dtype) {
    if (h_qe_check(N, C, HW, K, dtype, true)) return 0;
    if (dtype == CNNQ_DTYPE_F32) return cnnq_pc_qerr_workspace(N, C, HW, K);
    return (size_t)N * (size_t)h_qe_parts(N, C, HW) * (size_t)QE_NV(K) * (size_t)C * sizeof(double);
}

// Which launch cnnq_pc_qerr_dt makes for this geometry (host only): out = {piece width W, column parts per row nb, rows a workgroup
// takes per step (TPB / the lanes of a row), 1 - the native launch / 0 - a class of layer that did not win against the upcast
// route and stays there: h_qerr_native, with the figures next to the rule}.  fp32: cnnq_pc_qerr's plan - {elements per load, slices per row, 1, 1}.
int cnnq_pc_route_qerr_dt(int64_t N, int64_t C, int64_t HW, int dtype, int align_bytes, int32_t out[4]) {
    if (const int rc = h_qe_check(N, C, HW, 1, dtype, out && pow2(align_bytes))) return rc;
    if (dtype == CNNQ_DTYPE_F32) {
        Variant v;
        Geo g;
        if (const int rc = qerr_plan(N, C, HW, align_bytes >= 16, &v, &g)) return rc;
        out[0] = v.vec;
        out[1] = g.mode == 1 ? g.nb : 1;
        out[2] = 1;
        out[3] = 1;
        return 0;
    }
    out[0] = h_piece(HW, (uintptr_t)align_bytes, 0);
    out[1] = h_qe_parts(N, C, HW);
    out[2] = TPB / h_qe_seg(HW, out[0], out[1]);
    out[3] = h_qerr_native(N, C, HW, dtype);
    return 0;
}

// smpc.py:80-100 (the cosine: utils/misc.py:23-34) on x[N][C][HW] of bf16 / fp16: k_h_qerr -> k_qerr_fold, the fold of
// cnnq_pc_qerr on the same row records
int cnnq_pc_qerr_dt(const void* x, int dtype, int64_t N, int64_t C, int64_t HW, const float* qp, int K, const float* mm, void* ws,
                    float* err, void* stream) {
    const bool f32 = dtype == CNNQ_DTYPE_F32;
    if (const int rc = h_qe_check(N, C, HW, K, dtype, x && qp && ws && err && !misaligned(ws, 8) && (f32 || !misaligned(x, 2)))) return rc;
    if (f32) return cnnq_pc_qerr(static_cast<const float*>(x), N, C, HW, qp, K, mm, ws, err, stream);
    const int w = h_piece(HW, (uintptr_t)x, 0), nb = h_qe_parts(N, C, HW), seg = h_qe_seg(HW, w, nb);
    const HGeo g = h_geo(N, C, HW, w, h_qe_splits(N, C, HW, nb, seg), nb);
    hipStream_t st = hs(stream);
    double* rec = reinterpret_cast<double*>(ws);
    const dim3 grid((unsigned)(C * g.S * nb));
    const int rc = h_launch(dtype, w, x, [&](auto pc, const uint16_t* xh) {
        with_int<1, 2, 3>(K, [&](auto k) {
            with_bool(mm != nullptr, [&](auto m) {
                using P = decltype(pc);
                hipLaunchKernelGGL((k_h_qerr<typename P::T, P::W, decltype(k)::value, decltype(m)::value>), grid, dim3(TPB), 0, st, xh, g, seg,
                                   qp, mm, rec);
            });
        });
    });
    if (rc) return rc;
    with_int<1, 2, 3>(K, [&](auto k) {
        hipLaunchKernelGGL((k_qerr_fold<decltype(k)::value>), dim3((unsigned)((C + QF_CH - 1) / QF_CH)), dim3(TPB), 0, st, rec, (int)N, nb, (int)C,
                           (int)HW, err);
    });
    return launch_status();
}

// ---- `-sm use ... -bca` on contiguous bf16 / fp16 activations (cnnq_half_bcorr.hip.h) -------------------------------------------
// ws, doubles: part3[G][3][C] with G = S * column splits (h_stats_splits: not the alignment's); fp32: the chain's records
size_t cnnq_pc_qdq_bcorr_dt_workspace(int64_t N, int64_t C, int64_t HW, int dtype) {
    const HPlan p(N, C, HW, dtype, true);
    const int64_t G = p.rc ? 0 : dtype == CNNQ_DTYPE_F32 ? h_records_f32(N, C, HW) : p.G();
    return G <= 0 ? 0 : (size_t)G * 3 * (size_t)C * sizeof(double);
}

// the route word of a bf16 / fp16 tensor at piece width w: 1 - k_h_bcorr_whole / 2 - the two passes and the bias between them /
// 0 - a class of layer that did not win against the upcast route and stays there (h_bcorr_native; the call itself runs every class)
static int h_bcorr_route(int64_t N, int64_t C, int64_t HW, int dtype, int w, int allow_single_launch) {
    const bool wins = allow_single_launch > 1 || h_bcorr_whole_wins(N, C, HW, dtype);
    if (allow_single_launch && h_bcorr_whole_fits(N, HW, w) && wins) return 1;
    return h_bcorr_native(N, C, HW, dtype) ? 2 : 0;
}

// Which launches cnnq_pc_qdq_bcorr_dt makes for this geometry with allow_single_launch 0 / 1 (host only): out = {piece width W,
// batch splits S, column splits of the sums pass, route (h_bcorr_route)}.  fp32: {0, the chain's records, 1, 2}.
int cnnq_pc_route_qdq_bcorr_dt(int64_t N, int64_t C, int64_t HW, int dtype, int align_bytes, int allow_single_launch, int32_t out[4]) {
    const HPlan p(N, C, HW, dtype, out && pow2(align_bytes), true);
    if (p.rc) return p.rc;
    const bool f32 = dtype == CNNQ_DTYPE_F32;
    const int w = f32 ? 0 : h_piece(HW, (uintptr_t)align_bytes, 0);
    out[0] = w;
    out[1] = f32 ? h_records_f32(N, C, HW) : p.S;
    out[2] = f32 ? 1 : p.cs;
    out[3] = f32 ? 2 : h_bcorr_route(N, C, HW, dtype, w, allow_single_launch);
    return 0;
}

// iqm.py:180-196 folded into int_quantizer.py:573-592 on x[N][C][HW] of bf16 / fp16 with a given table (-sm use): k_h_bcorr_whole,
// or k_h_bcorr_sums (ascending) -> k_bcorr_bias on its S * cs records -> k_h_qdq_bias (descending)
int cnnq_pc_qdq_bcorr_dt(const void* x, void* y, int dtype, int64_t N, int64_t C, int64_t HW, const float* qp, int relu_first, void* ws,
                         double* sums, float* bias, int allow_single_launch, void* stream) {
    const bool f32 = dtype == CNNQ_DTYPE_F32;
    const uintptr_t es = f32 ? 4 : 2;
    const bool ok = x && y && x != y && qp && ws && bias && !misaligned(ws, 8) && !misaligned(sums, 8) && !misaligned(qp, 4) &&
                    !misaligned(bias, 4) && !misaligned(x, es) && !misaligned(y, es);
    const HPlan p(N, C, HW, dtype, ok);
    if (p.rc) return p.rc;
    double* part3 = static_cast<double*>(ws);
    if (f32) {
        const int G = cnnq_pc_groups(N, C, HW, al16(x));
        if (G <= 0) return g_error(G);
        const float* xf = static_cast<const float*>(x);
        int rc = cnnq_pc_qdq_bcorr_sums(xf, N, C, HW, qp, relu_first, part3, stream);
        if (!rc) rc = cnnq_pc_bcorr_bias(part3, G, C, sums, bias, stream);
        if (!rc) rc = cnnq_pc_qdq_bcorr(xf, static_cast<float*>(y), N, C, HW, qp, bias, 1, stream);
        return rc;
    }
    const int w = h_piece(HW, (uintptr_t)h_align(x, y), 0);
    hipStream_t st = hs(stream);
    const int relu = relu_first ? 1 : 0;
    if (h_bcorr_route(N, C, HW, dtype, w, allow_single_launch) == 1) {
        const HGeo g = h_geo(N, C, HW, w, 1, 1);
        return h_launch(dtype, w, x, y, [&](auto pc, const uint16_t* xh, uint16_t* yh) {
            using P = decltype(pc);
            if constexpr (P::W > 1)
                hipLaunchKernelGGL((k_h_bcorr_whole<typename P::T, P::W, h_whole_k<P::W>()>), dim3((unsigned)C), dim3(HTPB), 0, st, xh, yh, g, relu, qp,
                                   sums, bias);
        });
    }
    const int G = p.G();
    const HGeo gs = h_geo(N, C, HW, w, p.S, p.cs), gq = h_geo_qdq(N, C, HW, w);
    int rc = h_launch(dtype, w, x, [&](auto pc, const uint16_t* xh) {
        using P = decltype(pc);
        hipLaunchKernelGGL((k_h_bcorr_sums<typename P::T, P::W>), dim3((unsigned)(C * G)), dim3(TPB), 0, st, xh, gs, relu, qp, part3);
    });
    if (!rc) rc = cnnq_pc_bcorr_bias(part3, G, C, sums, bias, stream);
    if (rc) return rc;
    return h_launch(dtype, w, x, y, [&](auto pc, const uint16_t* xh, uint16_t* yh) {
        using P = decltype(pc);
        hipLaunchKernelGGL((k_h_qdq_bias<typename P::T, P::W>), dim3((unsigned)(C * gq.S)), dim3(TPB), 0, st, xh, yh, gq, qp, bias);
    });
}

// ---- dynamic ACIQ clipping (config 3) on contiguous bf16 / fp16 activations (cnnq_half_aciq.hip.h) ------------------------------
// ws, doubles: part[G][CNNQ_NMOM][C], mom[CNNQ_NMOM][C], part2[G][CNNQ_NDEV][C] with G = S * column splits - cnnq_pc_stats_dt's
// (the table stays outside); fp32: what cnnq_pc_aciq_qdq takes at either alignment
size_t cnnq_pc_aciq_dt_workspace(int64_t N, int64_t C, int64_t HW, int dtype) {
    if (dtype == CNNQ_DTYPE_F32) {
        const size_t a = cnnq_pc_aciq_workspace(N, C, HW, 1), b = cnnq_pc_aciq_workspace(N, C, HW, 0);
        return a > b ? a : b;
    }
    return cnnq_pc_stats_dt_workspace(N, C, HW, dtype);
}

// what config 3's entry points on contiguous tensors check of their configuration, before any launch
static bool h_aciq_cfg_ok(const cnnq_params_cfg* cfg) {
    return cfg && !check_cfg(cfg) && !cfg->direct_range && (cfg->clip == 1 || cfg->clip == 2);
}

// the route word of a bf16 / fp16 tensor at piece width w: 1 - k_h_aciq_whole alone (no bit allocation in effect) / 3 - pass A,
// merge and k_bitalloc, then k_h_aciq_whole<TABLE> (bit allocation on the std prior) / 2 - the chain (also: bit allocation on the
// b prior, which needs every channel's b before any channel's parameters) / 0 - a class of layer that did not win against the
// upcast route and stays there (h_aciq_native; the call itself runs every class, on the chain)
static int h_aciq_route(int64_t N, int64_t C, int64_t HW, int dtype, int w, const cnnq_params_cfg* cfg, int allow_single_launch) {
    const bool ba = cfg_bit_alloc(cfg);
    if (allow_single_launch && !(ba && cfg->prior_is_b) && h_aciq_whole_fits(N, HW, w) &&
        (allow_single_launch > 1 || h_aciq_whole_wins(N, C, HW, dtype, ba)))
        return ba ? 3 : 1;
    return h_aciq_native(N, C, HW, dtype) ? 2 : 0;
}

// Which launches cnnq_pc_aciq_qdq_dt makes for this geometry and configuration (host only): out = {piece width W, batch splits S,
// column splits of the statistics launches, route (h_aciq_route)}.  fp32: {0, the chain's records, 1, 2}.
int cnnq_pc_route_aciq_dt(int64_t N, int64_t C, int64_t HW, int dtype, int align_bytes, const cnnq_params_cfg* cfg, int allow_single_launch,
                          int32_t out[4]) {
    const HPlan p(N, C, HW, dtype, out && pow2(align_bytes) && h_aciq_cfg_ok(cfg), true);
    if (p.rc) return p.rc;
    const bool f32 = dtype == CNNQ_DTYPE_F32;
    const int w = f32 ? 0 : h_piece(HW, (uintptr_t)align_bytes, 0);
    out[0] = w;
    out[1] = f32 ? h_records_f32(N, C, HW) : p.S;
    out[2] = f32 ? 1 : p.cs;
    out[3] = f32 ? 2 : h_aciq_route(N, C, HW, dtype, w, cfg, allow_single_launch);
    return 0;
}

// int_quantizer.py:327-352 (statistics, ACIQ clipping, bit allocation) + 409-451, 557-603 (parameters, Q/DQ) on x[N][C][HW] of
// bf16 / fp16 with dynamic statistics: k_h_aciq_whole (route 1), or k_h_moments -> k_combine -> k_bitalloc -> k_h_aciq_whole<TABLE>
// (route 3), or the chain k_h_moments -> k_combine (-> k_h_absdev -> k_combine_dev) -> k_params -> k_h_qdq (route 2)
int cnnq_pc_aciq_qdq_dt(const void* x, void* y, int dtype, int64_t N, int64_t C, int64_t HW, const cnnq_params_cfg* cfg, void* ws,
                        float* stats, float* qp, float* diag, int allow_single_launch, void* stream) {
    const bool f32 = dtype == CNNQ_DTYPE_F32;
    const uintptr_t es = f32 ? 4 : 2;
    const bool ok = x && y && x != y && ws && stats && qp && !misaligned(ws, 8) && !misaligned(stats, 4) && !misaligned(qp, 4) &&
                    !misaligned(diag, 4) && !misaligned(x, es) && !misaligned(y, es) && h_aciq_cfg_ok(cfg) &&
                    !(cfg_bit_alloc(cfg) && !diag);                                   // the bit table lives in diag
    const HPlan p(N, C, HW, dtype, ok);
    if (p.rc) return p.rc;
    hipStream_t st = hs(stream);
    if (f32) {
        const float* xf = static_cast<const float*>(x);
        const int G = cnnq_pc_groups(N, C, HW, al16(xf) ? 1 : 0);
        if (G <= 0) return g_error(G);
        const int rc = cnnq_pc_aciq_qdq(xf, static_cast<float*>(y), N, C, HW, cfg, ws, qp, diag, stream);
        if (rc) return rc;
        // the chain keeps its table behind its records: the caller's copy
        if (hipMemcpyAsync(stats, AciqWs(ws, G, C).stats, (size_t)CNNQ_NSTAT * (size_t)C * sizeof(float), hipMemcpyDeviceToDevice, st) != hipSuccess)
            return launch_status();
        return 0;
    }
    const int w = h_piece(HW, (uintptr_t)h_align(x, y), 0);
    const int route = h_aciq_route(N, C, HW, dtype, w, cfg, allow_single_launch);
    const bool need_b = cfg->clip == 1 || (cfg_bit_alloc(cfg) && cfg->prior_is_b);
    if (route == 1 || route == 3) {
        HAciqArgs a{*cfg, nullptr, stats, qp, diag};
        if (route == 3) {
            int rc = cnnq_pc_stats_dt(x, dtype, N, C, HW, 0, 0, 0, ws, nullptr, stats, stream);
            float* bits = nullptr;
            if (!rc) rc = launch_bitalloc(stats, C, cfg, diag, &bits, st);
            if (rc) return rc;
            a.bits = bits;
        }
        const HGeo g = h_geo(N, C, HW, w, 1, 1);
        return h_launch(dtype, w, x, y, [&](auto pc, const uint16_t* xh, uint16_t* yh) {
            with_bool(route == 3, [&](auto table) {
                using P = decltype(pc);
                if constexpr (P::W > 1)
                    hipLaunchKernelGGL((k_h_aciq_whole<typename P::T, P::W, h_whole_k<P::W>(), decltype(table)::value>), dim3((unsigned)C),
                                       dim3(HTPB), 0, st, xh, yh, g, a);
            });
        });
    }
    int rc = cnnq_pc_stats_dt(x, dtype, N, C, HW, need_b ? 1 : 0, 0, 0, ws, nullptr, stats, stream);
    if (!rc) rc = cnnq_pc_params(stats, C, cfg, qp, diag, stream);
    if (rc) return rc;
    return h_qdq(x, y, dtype, N, C, HW, qp, nullptr, HArgs{}, st);
}

// ---- config 5 (mid-tread, bin allocation, entropy) on contiguous bf16 / fp16 activations (cnnq_half_midtread.hip.h) ------------
// ws, doubles: cnnq_pc_stats_dt's records (the tables stay outside); fp32 has no plan here: 0
size_t cnnq_pc_midtread_dt_workspace(int64_t N, int64_t C, int64_t HW, int dtype) {
    return dtype == CNNQ_DTYPE_F32 ? 0 : cnnq_pc_stats_dt_workspace(N, C, HW, dtype);
}

// the route word of a bf16 / fp16 tensor at piece width w: 3 - pass A, merge and k_mt_params<GUESS>, then k_h_mt_whole / 2 - the
// chain / 0 - a class of layer that did not win against the upcast route and stays there (h_mt_native; the call itself runs
// every class, on the chain)
static int h_mt_route(int64_t N, int64_t C, int64_t HW, int dtype, int w, bool hist, int allow_single_launch) {
    if (allow_single_launch && h_mt_whole_fits(N, HW, w) && (allow_single_launch > 1 || h_mt_whole_wins(N, C, HW, dtype, hist))) return 3;
    return h_mt_native(N, C, HW, dtype, hist) ? 2 : 0;
}

// Which launches cnnq_pc_midtread_dt makes for this geometry (host only): out = {piece width W, batch splits S, column splits of
// the statistics launches, route (h_mt_route)}.  fp32: CNNQ_ENOTSUP, as the call.
int cnnq_pc_route_midtread_dt(int64_t N, int64_t C, int64_t HW, int dtype, int align_bytes, int hist, int allow_single_launch,
                              int32_t out[4]) {
    const HPlan p(N, C, HW, dtype, out && pow2(align_bytes));
    if (p.rc) return p.rc;
    if (dtype == CNNQ_DTYPE_F32) return CNNQ_ENOTSUP;
    const int w = h_piece(HW, (uintptr_t)align_bytes, 0);
    out[0] = w;
    out[1] = p.S;
    out[2] = p.cs;
    out[3] = h_mt_route(N, C, HW, dtype, w, hist != 0, allow_single_launch);
    return 0;
}

static int h_mt_qdq(const void* x, void* y, int dtype, int64_t N, int64_t C, int64_t HW, int w, const float* mt, uint64_t* hist,
                    hipStream_t st) {
    const HGeo g = h_geo_mt(N, C, HW, w, hist != nullptr);
    return h_launch(dtype, w, x, y, [&](auto pc, const uint16_t* xh, uint16_t* yh) {
        with_bool(hist != nullptr, [&](auto h) {
            using P = decltype(pc);
            hipLaunchKernelGGL((k_h_mt_qdq<typename P::T, P::W, decltype(h)::value>), dim3((unsigned)(C * g.S)), dim3(TPB), 0, st, xh, yh, g,
                               mt, u64p(hist));
        });
    });
}

// iq.py:202-224 on x[N][C][HW] of bf16 / fp16 with a given table mt (cnnq_pc_midtread_params, clip = 1), and the codes counted
// into hist (zeroed by the caller): one launch
int cnnq_pc_midtread_qdq_dt(const void* x, void* y, int dtype, int64_t N, int64_t C, int64_t HW, const float* mt, uint64_t* hist,
                            void* stream) {
    const bool f32 = dtype == CNNQ_DTYPE_F32;
    const uintptr_t es = f32 ? 4 : 2;
    const HPlan p(N, C, HW, dtype, x && y && x != y && mt && !misaligned(mt, 4) && !misaligned(hist, 8) && !misaligned(x, es) &&
                                       !misaligned(y, es));
    if (p.rc) return p.rc;
    if (f32) return cnnq_pc_midtread_qdq(static_cast<const float*>(x), static_cast<float*>(y), N, C, HW, mt, 1, nullptr, hist, stream);
    return h_mt_qdq(x, y, dtype, N, C, HW, h_piece(HW, (uintptr_t)h_align(x, y), 0), mt, hist, hs(stream));
}

// iq.py:170-225 (per-channel statistics, bin allocation eq. 10, Laplace clipping, mid-tread Q/DQ) on x[N][C][HW] of bf16 / fp16:
// k_h_moments -> k_combine -> k_h_absdev -> k_combine_dev -> k_mt_params -> k_h_mt_qdq (route 2), or k_h_moments -> k_combine ->
// k_mt_params<GUESS> -> k_h_mt_whole (route 3)
int cnnq_pc_midtread_dt(const void* x, void* y, int dtype, int64_t N, int64_t C, int64_t HW, double target, int sym, const double* tables,
                        int ntab, void* ws, float* stats, float* mt, uint64_t* hist, int allow_single_launch, void* stream) {
    const bool f32 = dtype == CNNQ_DTYPE_F32;
    const uintptr_t es = f32 ? 4 : 2;
    const bool ok = x && y && x != y && tables && ntab >= 2 && ws && stats && mt && !misaligned(ws, 8) && !misaligned(tables, 8) &&
                    !misaligned(stats, 4) && !misaligned(mt, 4) && !misaligned(hist, 8) && !misaligned(x, es) && !misaligned(y, es) &&
                    target - target == 0.;                                            // (not NaN or infinite)
    const HPlan p(N, C, HW, dtype, ok);
    if (p.rc) return p.rc;
    if (f32) return CNNQ_ENOTSUP;                    // fp32 callers have cnnq_pc_midtread_qdq_single and the chain
    hipStream_t st = hs(stream);
    const int w = h_piece(HW, (uintptr_t)h_align(x, y), 0);
    const int route = h_mt_route(N, C, HW, dtype, w, hist != nullptr, allow_single_launch);
    if (hist) {
        const size_t words = (size_t)CNNQ_MT_HIST_WORDS(C);
        hipLaunchKernelGGL(k_h_mt_zero, dim3((unsigned)((words + 4 * TPB - 1) / (4 * TPB))), dim3(TPB), 0, st, u64p(hist), words);
        if (const int rc = launch_status()) return rc;
    }
    const MtCfg mcfg{target, 1, sym ? 1 : 0};
    if (route == 3) {
        int rc = cnnq_pc_stats_dt(x, dtype, N, C, HW, 0, 0, 0, ws, nullptr, stats, stream);
        if (!rc) rc = launch_mt_guess(stats, C, mcfg, tables, ntab, mt, st);
        if (rc) return rc;
        const HGeo g = h_geo(N, C, HW, w, 1, 1);
        const HMtArgs a{mcfg, stats, mt, u64p(hist)};
        return h_launch(dtype, w, x, y, [&](auto pc, const uint16_t* xh, uint16_t* yh) {
            with_bool(hist != nullptr, [&](auto h) {
                using P = decltype(pc);
                if constexpr (P::W > 1)
                    hipLaunchKernelGGL((k_h_mt_whole<typename P::T, P::W, h_whole_k<P::W>(), decltype(h)::value>), dim3((unsigned)C),
                                       dim3(HTPB), 0, st, xh, yh, g, a);
            });
        });
    }
    int rc = cnnq_pc_stats_dt(x, dtype, N, C, HW, 1, 0, 0, ws, nullptr, stats, stream);
    if (!rc) rc = cnnq_pc_midtread_params(stats, C, target, 1, sym, tables, ntab, mt, stream);
    if (rc) return rc;
    return h_mt_qdq(x, y, dtype, N, C, HW, w, mt, hist, st);
}

// ---- the uniform Q/DQ that counts its codes (-me) on contiguous bf16 / fp16 activations (cnnq_half_entropy.hip.h) ----------------
// the route word of a bf16 / fp16 tensor at piece width w: 1 - k_h_whole_hist alone / 2 - k_h_minmax, then k_h_qdq_hist / 0 - a
// class of layer that did not win against the upcast route and stays there (h_ent_native; the calls themselves run every class,
// on route 2)
static int h_ent_route(int64_t N, int64_t C, int64_t HW, int dtype, int w, int nbins, int allow_single_launch) {
    if (allow_single_launch && h_ent_whole_fits(N, HW, w) && (allow_single_launch > 1 || h_ent_whole_wins(N, C, HW, dtype, nbins))) return 1;
    return h_ent_native(N, C, HW, dtype, nbins) ? 2 : 0;
}

// Which launches cnnq_pc_minmax_qdq_hist_dt makes for this geometry (host only): out = {piece width W, batch splits S of the
// counting launch, column splits of the statistics launch, route (h_ent_route)}.  fp32: CNNQ_ENOTSUP, as the calls.
int cnnq_pc_route_qdq_hist_dt(int64_t N, int64_t C, int64_t HW, int dtype, int align_bytes, int nbins, int allow_single_launch,
                              int32_t out[4]) {
    const HPlan p(N, C, HW, dtype, out && pow2(align_bytes) && hist_bins_ok(nbins));
    if (p.rc) return p.rc;
    if (dtype == CNNQ_DTYPE_F32) return CNNQ_ENOTSUP;
    const int w = h_piece(HW, (uintptr_t)align_bytes, 0);
    out[0] = w;
    out[1] = h_geo_hist(N, C, HW, w).S;
    out[2] = h_geo_mm(N, C, HW, w, h_records_f32(N, C, HW)).cs;
    out[3] = h_ent_route(N, C, HW, dtype, w, nbins, allow_single_launch);
    return 0;
}

// pmm == NULL: the parameters from the table qp; else from the statistics partials pmm (published to ha.qp / ha.mm)
static int h_qdq_hist(const void* x, void* y, int dtype, int64_t N, int64_t C, int64_t HW, int w, const float* qp, const float* pmm,
                      const HArgs& ha, int nbins, uint64_t* hist_rep, hipStream_t st) {
    const HGeo g = h_geo_hist(N, C, HW, w);
    return h_launch(dtype, w, x, y, [&](auto pc, const uint16_t* xh, uint16_t* yh) {
        using P = decltype(pc);
        hipLaunchKernelGGL((k_h_qdq_hist<typename P::T, P::W>), dim3((unsigned)(C * g.S)), dim3(TPB), h_hist_lds(nbins), st, xh, yh, g, qp,
                           pmm, ha, nbins, u64p(hist_rep));
    });
}

// int_quantizer.py:573-592 on x[N][C][HW] of bf16 / fp16 with a given table, and the codes of 586-587 counted into hist_rep: one
// launch
int cnnq_pc_qdq_hist_dt(const void* x, void* y, int dtype, int64_t N, int64_t C, int64_t HW, const float* qp, int nbins,
                        uint64_t* hist_rep, void* stream) {
    const HPlan p(N, C, HW, dtype, x && y && x != y && qp && hist_rep && !misaligned(hist_rep, 8) && hist_bins_ok(nbins));
    if (p.rc) return p.rc;
    if (dtype == CNNQ_DTYPE_F32) return CNNQ_ENOTSUP;
    return h_qdq_hist(x, y, dtype, N, C, HW, h_piece(HW, (uintptr_t)h_align(x, y), 0), qp, nullptr, HArgs{}, nbins, hist_rep, hs(stream));
}

// int_quantizer.py:409-451, 557-603 with 586-587 on x[N][C][HW] of bf16 / fp16: k_h_whole_hist (route 1), or k_h_minmax ->
// k_h_qdq_hist (route 2), 2^num_bits bins
int cnnq_pc_minmax_qdq_hist_dt(const void* x, void* y, int dtype, int64_t N, int64_t C, int64_t HW, int num_bits, int positive,
                               float* ws, float* qp, float* mm, uint64_t* hist_rep, int allow_single_launch, void* stream) {
    const bool ok = x && y && x != y && ws && qp && hist_rep && !misaligned(ws, 4) && !misaligned(hist_rep, 8) && num_bits >= 1 &&
                    num_bits <= 8;                                                    // the codes fit a byte, the bins 256
    const HPlan p(N, C, HW, dtype, ok);
    if (p.rc) return p.rc;
    if (dtype == CNNQ_DTYPE_F32) return CNNQ_ENOTSUP;
    hipStream_t st = hs(stream);
    const int nbins = 1 << num_bits;
    const int w = h_piece(HW, (uintptr_t)h_align(x, y), 0);
    if (h_ent_route(N, C, HW, dtype, w, nbins, allow_single_launch) == 1) {
        const HGeo g = h_geo(N, C, HW, w, 1, 1);
        const HArgs ha{0, num_bits, positive ? 1 : 0, qp, mm};
        return h_launch(dtype, w, x, y, [&](auto pc, const uint16_t* xh, uint16_t* yh) {
            using P = decltype(pc);
            if constexpr (P::W > 1)
                hipLaunchKernelGGL((k_h_whole_hist<typename P::T, P::W, h_whole_k<P::W>()>), dim3((unsigned)C), dim3(HTPB), h_hist_lds(nbins),
                                   st, xh, yh, g, ha, nbins, u64p(hist_rep));
        });
    }
    float* const pmm = MmWs(ws, C).pmm;              // where cnnq_pc_minmax_qdq_auto_dt keeps its partials
    int S = 0;
    const int rc = h_minmax(x, dtype, N, C, HW, pmm, &S, st);
    if (rc) return rc;
    return h_qdq_hist(x, y, dtype, N, C, HW, w, qp, pmm, HArgs{S, num_bits, positive ? 1 : 0, qp, mm}, nbins, hist_rep, st);
}

// int_quantizer.py:327-352 + 409-451, 557-603 with 586-587 on x[N][C][HW] of bf16 / fp16: cnnq_pc_aciq_qdq_dt's route 2 with the
// counting pass last - k_h_moments -> k_combine (-> k_h_absdev -> k_combine_dev) -> k_params -> k_h_qdq_hist; 256 bins under bit
// allocation (the channels' qmax is decided on the device), else 2^num_bits
int cnnq_pc_aciq_qdq_hist_dt(const void* x, void* y, int dtype, int64_t N, int64_t C, int64_t HW, const cnnq_params_cfg* cfg, void* ws,
                             float* stats, float* qp, float* diag, uint64_t* hist_rep, void* stream) {
    const bool f32 = dtype == CNNQ_DTYPE_F32;
    const uintptr_t es = f32 ? 4 : 2;
    const bool ok = x && y && x != y && ws && stats && qp && hist_rep && !misaligned(ws, 8) && !misaligned(stats, 4) && !misaligned(qp, 4) &&
                    !misaligned(diag, 4) && !misaligned(hist_rep, 8) && !misaligned(x, es) && !misaligned(y, es) && h_aciq_cfg_ok(cfg) &&
                    cfg->num_bits <= 8 && !(cfg_bit_alloc(cfg) && !diag);             // the bit table lives in diag
    const HPlan p(N, C, HW, dtype, ok);
    if (p.rc) return p.rc;
    if (f32) return CNNQ_ENOTSUP;
    const bool need_b = cfg->clip == 1 || (cfg_bit_alloc(cfg) && cfg->prior_is_b);
    int rc = cnnq_pc_stats_dt(x, dtype, N, C, HW, need_b ? 1 : 0, 0, 0, ws, nullptr, stats, stream);
    if (!rc) rc = cnnq_pc_params(stats, C, cfg, qp, diag, stream);
    if (rc) return rc;
    return h_qdq_hist(x, y, dtype, N, C, HW, h_piece(HW, (uintptr_t)h_align(x, y), 0), qp, nullptr, HArgs{}, cfg_bit_alloc(cfg) ? 256 : 1 << cfg->num_bits,
                      hist_rep, hs(stream));
}

int cnnq_pt_qdq_dt(const void* x, void* y, int dtype, int64_t n, const float* ptp, const float* noise, void* stream) {
    if (!dtype_ok(dtype)) return CNNQ_EINVAL;
    return pt_qdq_launch(x, y, dtype, n, ptp, noise, stream);
}

static int pt_qdq_launch(const void* x, void* y, int dtype, int64_t n, const float* ptp, const float* noise, void* stream) {
    if (!x || !y || !ptp || n <= 0) return CNNQ_EINVAL;
    const bool vec = al16(x) && al16(y) && (!noise || al16(noise));
    const int wide = dtype == CNNQ_DTYPE_F32 ? 4 : 8;
    const int64_t work = vec ? (n + wide - 1) / wide : n;
    const int64_t blocks = (work + TPB - 1) / TPB;
    if (blocks >= ((int64_t)1 << 31)) return CNNQ_ERANGE;
    const dim3 grid((unsigned)blocks), block(TPB);
    if (dtype == CNNQ_DTYPE_F32) {
        with_bool(vec, noise != nullptr, [&](auto vc, auto nz) {
            hipLaunchKernelGGL((k_pt_qdq<decltype(vc)::value ? 4 : 1, decltype(nz)::value>), grid, block, 0, hs(stream), static_cast<const float*>(x),
                               static_cast<float*>(y), n, ptp, noise);
        });
        return launch_status();
    }
    return h_launch(dtype, vec ? 8 : 1, x, y, [&](auto pc, const uint16_t* xh, uint16_t* yh) {
        with_bool(noise != nullptr, [&](auto nz) {
            using P = decltype(pc);
            if constexpr (P::W == 8 || P::W == 1)
                hipLaunchKernelGGL((k_h_pt_qdq<typename P::T, P::W, decltype(nz)::value>), grid, block, 0, hs(stream), xh, yh, n, ptp, noise);
        });
    });
}

// ---- dense channels_last activations (cnnq_nhwc.hip.h): x and y [R = N*H*W][C], C innermost; fp32 tables ----------------------
// the widest slab count of the statistics launches over the piece widths C allows (the alignment is not known yet)
static int64_t cl_slabs_max(int64_t R, int64_t C, int dtype) {
    int64_t S = 1;
    for (int w = 16 / cl_esize(dtype); w >= 1; w >>= 1) {
        if (C % w) continue;
        const int64_t s = cl_geo_mm(R, C, w).S;
        S = s > S ? s : S;
    }
    return S;
}

size_t cnnq_pc_nhwc_workspace(int64_t R, int64_t C, int dtype) {
    if (cl_check(R, C, dtype)) return 0;
    return ((size_t)2 + 2 * (size_t)cl_slabs_max(R, C, dtype)) * (size_t)C * sizeof(float);
}

int cnnq_pc_route_nhwc(int64_t R, int64_t C, int dtype, int align_bytes, int32_t out[4]) {
    return cl_route(R, C, dtype, align_bytes, out, /*rows32=*/false, /*ok=*/true, [&](const ClPlan& p) {
        out[0] = p.w;
        out[1] = p.m.S;
        out[2] = p.q.S * p.q.nb;
        out[3] = (int32_t)(p.m.rpw / p.m.RS);
        return 0;
    });
}

static int cl_qdq(const void* x, void* y, int dtype, const ClPlan& p, const float* qp, const float* mm, hipStream_t st) {
    return cl_launch(dtype, p.w, x, y, [&](auto pc, auto* xr, auto* yr) {
        using P = decltype(pc);
        hipLaunchKernelGGL((k_cl_qdq<typename P::T, P::W>), p.qgrid(), dim3(TPB), 0, st, xr, yr, p.q, qp, mm);
    });
}

// The front of config 2 on [R][C], three launches: k_cl_minmax -> k_minmax_params (qp) -> k_minmax_reduce (the extrema, into mm or -
// mm == NULL - the head of ws); returns them through *ext
static int cl_minmax_front(const void* x, int dtype, int64_t C, const ClPlan& p, int num_bits, int positive, float* ws, float* qp, float* mm,
                           float** ext, void* stream) {
    *ext = mm ? mm : ws;
    float* pmm = ws + 2 * (size_t)C;
    int rc = cl_launch(dtype, p.w, x, [&](auto pc, auto* xr) {
        using P = decltype(pc);
        hipLaunchKernelGGL((k_cl_minmax<typename P::T, P::W>), p.mgrid(), dim3(TPB), 0, hs(stream), xr, p.m, pmm);
    });
    if (!rc) rc = cnnq_pc_minmax_params(pmm, p.m.S, C, num_bits, positive, qp, stream);
    if (!rc) rc = cnnq_pc_minmax_reduce(pmm, p.m.S, C, *ext, stream);
    return rc;
}

// int_quantizer.py:409-451, 557-603 on [R][C]: cl_minmax_front -> k_cl_qdq
int cnnq_pc_minmax_qdq_nhwc(const void* x, void* y, int dtype, int64_t R, int64_t C, int num_bits, int positive, float* ws,
                            float* qp, float* mm, void* stream) {
    if (cl_check(R, C, dtype)) return CNNQ_EINVAL;
    if (!x || !y || !ws || !qp || num_bits < 1 || num_bits > 32) return CNNQ_EINVAL;
    const ClPlan p(R, C, dtype, h_align(x, y));
    if (const int rc = p.range(false)) return rc;
    float* ext;
    int rc = cl_minmax_front(x, dtype, C, p, num_bits, positive, ws, qp, mm, &ext, stream);
    if (!rc) rc = cl_qdq(x, y, dtype, p, qp, ext, hs(stream));
    return rc;
}

// int_quantizer.py:573-592 on [R][C] with a given table (-sm use): the IEEE divide
int cnnq_pc_qdq_nhwc(const void* x, void* y, int dtype, int64_t R, int64_t C, const float* qp, void* stream) {
    if (cl_check(R, C, dtype)) return CNNQ_EINVAL;
    if (!x || !y || !qp) return CNNQ_EINVAL;
    const ClPlan p(R, C, dtype, h_align(x, y));
    if (const int rc = p.range(false)) return rc;
    return cl_qdq(x, y, dtype, p, qp, nullptr, hs(stream));
}

// ---- config 3 on dense channels_last activations (cnnq_nhwc_aciq.hip.h) --------------------------------------------------------
// ws of cnnq_pc_aciq_qdq_nhwc, doubles: part[S][CNNQ_NMOM][C], mom[CNNQ_NMOM][C], part2[S][CNNQ_NDEV][C]
size_t cnnq_pc_aciq_nhwc_workspace(int64_t R, int64_t C, int dtype) {
    if (cl_check(R, C, dtype)) return 0;
    return AciqWs::bytes((size_t)cl_slabs_max(R, C, dtype), C, false);
}

// Which launches cnnq_pc_aciq_qdq_nhwc makes for this geometry (host only).  out[5] is 1 throughout: no class of layer is sent
// back to the copy route; one that measures slower native than through the copy (tools/bench_channels_last_aciq.py) goes back here.
int cnnq_pc_route_aciq_nhwc(int64_t R, int64_t C, int dtype, int align_bytes, int32_t out[6]) {
    return cl_route(R, C, dtype, align_bytes, out, /*rows32=*/true, /*ok=*/true, [&](const ClPlan& p) {
        out[0] = p.w;
        out[1] = p.m.S;
        out[2] = (int32_t)p.m.rpw;
        out[3] = (int32_t)(p.m.rpw / p.m.RS);
        out[4] = p.q.S * p.q.nb;
        out[5] = 1;
        return 0;
    });
}

// The statistics table of a channels_last tensor - the front of configs 3 and 5 and all of `-sm collect` (smpc.py:45-79): pass A
// (k_cl_moments, with the rectified sums k_cl_moments_relu) -> k_combine(has_relu) (-> pass B (k_cl_absdev, with the fourth moment
// k_cl_absdev_kurt) on the merged table -> k_combine_dev(want_kurt); need_b or need_kurt), two or four launches.  The merge writes
// every row of stats (zero for the rows nobody asked for; B comes with pass B); ws: the AciqWs records for the plan's slab count;
// mom: where the caller wants the merged moment record, or NULL (it stays in ws).  The element-wise pass behind it walks the
// tensor descending, so the statistics launch in front of it ascends: with pass B, pass A descends.
static int cl_table(const void* x, int dtype, int64_t R, int64_t C, const ClPlan& p, bool need_b, bool need_kurt, bool need_relu, void* ws,
                    double* mom, float* stats, void* stream) {
    const ClGeo& m = p.m;
    const AciqWs a(ws, m.S, C);
    double* rec = mom ? mom : a.mom;
    hipStream_t st = hs(stream);
    const bool ntl = nt_loads(R * C * cl_esize(dtype));
    const bool pass_b = need_b || need_kurt;
    const int rev = pass_b ? 1 : 0;
    int rc = cl_launch(dtype, p.w, x, [&](auto pc, auto* xr) {
        with_bool(ntl, need_relu, [&](auto nt, auto relu) {
            using P = decltype(pc);
            constexpr bool NT = decltype(nt)::value;
            if constexpr (decltype(relu)::value)
                hipLaunchKernelGGL((k_cl_moments_relu<typename P::T, P::W, NT>), p.mgrid(), dim3(TPB), 0, st, xr, m, rev, a.part);
            else
                hipLaunchKernelGGL((k_cl_moments<typename P::T, P::W, NT>), p.mgrid(), dim3(TPB), 0, st, xr, m, rev, a.part);
        });
    });
    if (!rc) rc = cnnq_pc_combine(a.part, m.S, C, need_relu ? 1 : 0, rec, stats, stream);
    if (rc || !pass_b) return rc;
    rc = cl_launch(dtype, p.w, x, [&](auto pc, auto* xr) {
        with_bool(ntl, need_kurt, [&](auto nt, auto kurt) {
            using P = decltype(pc);
            constexpr bool NT = decltype(nt)::value;
            if constexpr (decltype(kurt)::value)
                hipLaunchKernelGGL((k_cl_absdev_kurt<typename P::T, P::W, NT>), p.mgrid(), dim3(TPB), 0, st, xr, m, stats, a.part2);
            else
                hipLaunchKernelGGL((k_cl_absdev<typename P::T, P::W, NT>), p.mgrid(), dim3(TPB), 0, st, xr, m, stats, a.part2);
        });
    });
    if (!rc) rc = cnnq_pc_combine_dev(a.part2, m.S, C, rec, need_kurt ? 1 : 0, nullptr, stats, stream);
    return rc;
}

// The argument checks of config 3's entry points, before any launch
static int cl_aciq_check(const void* x, void* y, int dtype, int64_t R, int64_t C, const cnnq_params_cfg* cfg, void* ws, float* stats, float* qp,
                         float* diag) {
    if (cl_check(R, C, dtype)) return CNNQ_EINVAL;
    if (!x || !y || !cfg || !ws || !stats || !qp || misaligned(ws, 8)) return CNNQ_EINVAL;
    if (check_cfg(cfg)) return CNNQ_EINVAL;                                              // as cnnq_pc_params, before any launch
    if (cfg->direct_range) return CNNQ_EINVAL;                                           // the per-tensor branch has no channels
    return (cfg_bit_alloc(cfg) && !diag) ? CNNQ_EINVAL : 0;                              // the bit table lives in diag
}

// The front of config 3 on [R][C]: cl_table -> k_params (qp, diag)
static int cl_aciq_front(const void* x, int dtype, int64_t R, int64_t C, const ClPlan& p, const cnnq_params_cfg* cfg, void* ws, float* stats,
                         float* qp, float* diag, void* stream) {
    const bool need_b = cfg->clip == 1 || (cfg_bit_alloc(cfg) && cfg->prior_is_b);
    int rc = cl_table(x, dtype, R, C, p, need_b, false, false, ws, nullptr, stats, stream);
    if (!rc) rc = cnnq_pc_params(stats, C, cfg, qp, diag, stream);
    return rc;
}

// int_quantizer.py:327-352 (statistics, ACIQ clipping, bit allocation) + 409-451, 557-603 (parameters, Q/DQ) on [R][C]:
// cl_aciq_front -> k_cl_qdq with the table
int cnnq_pc_aciq_qdq_nhwc(const void* x, void* y, int dtype, int64_t R, int64_t C, const cnnq_params_cfg* cfg, void* ws,
                          float* stats, float* qp, float* diag, void* stream) {
    if (cl_aciq_check(x, y, dtype, R, C, cfg, ws, stats, qp, diag)) return CNNQ_EINVAL;
    const ClPlan p(R, C, dtype, h_align(x, y));
    if (const int rc = p.range(false)) return rc;
    int rc = cl_aciq_front(x, dtype, R, C, p, cfg, ws, stats, qp, diag, stream);
    if (!rc) rc = cl_qdq(x, y, dtype, p, qp, nullptr, hs(stream));
    return rc;
}

// ---- `-sm collect` on dense channels_last activations (cnnq_nhwc_collect.hip.h) ---------------------------------------------------
// ws of cnnq_pc_stats_nhwc: config 3's records (AciqWs without the table) for the widest slab count over the piece widths
size_t cnnq_pc_stats_nhwc_workspace(int64_t R, int64_t C, int dtype) { return cnnq_pc_aciq_nhwc_workspace(R, C, dtype); }

// Which launches cnnq_pc_stats_nhwc makes for this geometry (host only): out = {elements per load W, row slabs S, rows per slab, 1 -
// the native launches}.  out[3] is 1 throughout: no class of layer is sent back to the copy route; one that measures slower native
// than through the copy (tools/bench_channels_last_collect.py) goes back here, with the figures next to the rule.
int cnnq_pc_route_stats_nhwc(int64_t R, int64_t C, int dtype, int align_bytes, int32_t out[4]) {
    return cl_route(R, C, dtype, align_bytes, out, /*rows32=*/true, /*ok=*/true, [&](const ClPlan& p) {
        out[0] = p.w;
        out[1] = p.m.S;
        out[2] = (int32_t)p.m.rpw;
        out[3] = 1;
        return 0;
    });
}

// smpc.py:45-79 on [R][C]: cl_table with every flag the caller raises
int cnnq_pc_stats_nhwc(const void* x, int dtype, int64_t R, int64_t C, int need_b, int need_kurt, int need_relu, void* ws, double* mom,
                       float* stats, void* stream) {
    if (cl_check(R, C, dtype)) return CNNQ_EINVAL;
    if (!x || !ws || !stats || misaligned(ws, 8) || misaligned(mom, 8)) return CNNQ_EINVAL;
    const ClPlan p(R, C, dtype, h_align(x, x));
    if (const int rc = p.range(true)) return rc;
    return cl_table(x, dtype, R, C, p, need_b != 0, need_kurt != 0, need_relu != 0, ws, mom, stats, stream);
}

// ---- `-sm collect -ce` on dense channels_last activations (cnnq_nhwc_qerr.hip.h): x [N][HW][C], C innermost ------------------------
// the argument checks the three functions share: 0 - the plan exists (the grid N * S * nb and the fold's N stay in 32 bits)
static int cl_qe_check(int64_t N, int64_t HW, int64_t C, int K, int dtype) {
    if (!dtype_ok(dtype) || K < 1 || K > 3 || N < 1 || HW < 1 || C < 1 || C > CL_C_MAX) return CNNQ_EINVAL;
    if (N >= ((int64_t)1 << 31) || HW >= ((int64_t)1 << 31)) return CNNQ_ERANGE;      // k_qerr_fold takes both as int
    const int64_t nbmax = (C + TPB - 1) / TPB;      // column blocks of the narrowest piece
    return N * cl_qe_slabs(N, HW, C) * nbmax >= ((int64_t)1 << 31) ? CNNQ_ERANGE : 0;
}

size_t cnnq_pc_qerr_nhwc_workspace(int64_t N, int64_t HW, int64_t C, int K, int dtype) {
    if (cl_qe_check(N, HW, C, K, dtype)) return 0;
    return (size_t)N * (size_t)cl_qe_slabs(N, HW, C) * (size_t)QE_NV(K) * (size_t)C * sizeof(double);
}

// Which launch cnnq_pc_qerr_nhwc makes for this geometry (host only): out = {elements per load W, slabs per sample nb, rows per
// slab, 1 - the native launch}.  out[3] is 1 throughout: no class of layer is sent back to the copy route; one that measures slower
// native than through the copy (tools/bench_channels_last_qerr.py) goes back here, with the figures next to the rule.
int cnnq_pc_route_qerr_nhwc(int64_t N, int64_t HW, int64_t C, int dtype, int align_bytes, int32_t out[4]) {
    if (!out || !pow2(align_bytes)) return CNNQ_EINVAL;
    if (const int rc = cl_qe_check(N, HW, C, 1, dtype)) return rc;
    const ClGeo g = cl_geo_qe(N, HW, C, cl_qe_piece(C, cl_esize(dtype), align_bytes));
    out[0] = g.P ? (int32_t)(C / g.P) : 0;
    out[1] = g.S;
    out[2] = (int32_t)(g.rpw < INT32_MAX ? g.rpw : INT32_MAX);
    out[3] = 1;
    return 0;
}

// smpc.py:80-100 on [N][HW][C]: k_cl_qerr -> k_qerr_fold, the fold of cnnq_pc_qerr on the same row records
int cnnq_pc_qerr_nhwc(const void* x, int dtype, int64_t N, int64_t HW, int64_t C, const float* qp, int K, const float* mm, void* ws,
                      float* err, void* stream) {
    if (!x || !qp || !ws || !err || misaligned(ws, 8)) return CNNQ_EINVAL;
    if (const int rc = cl_qe_check(N, HW, C, K, dtype)) return rc;
    const ClGeo g = cl_geo_qe(N, HW, C, cl_qe_piece(C, cl_esize(dtype), h_align(x, x)));
    hipStream_t st = hs(stream);
    double* rec = reinterpret_cast<double*>(ws);
    const dim3 grid((unsigned)(N * g.S * g.nb));
    const int rc = cl_launch(dtype, (int)(C / g.P), x, [&](auto pc, auto* xr) {
        using P = decltype(pc);
        if constexpr (P::W <= CL_QE_WMAX)
            with_int<1, 2, 3>(K, [&](auto k) {
                hipLaunchKernelGGL((k_cl_qerr<typename P::T, P::W, decltype(k)::value>), grid, dim3(TPB), 0, st, xr, g, qp, mm, rec);
            });
    });
    if (rc) return rc;
    with_int<1, 2, 3>(K, [&](auto k) {
        hipLaunchKernelGGL((k_qerr_fold<decltype(k)::value>), dim3((unsigned)((C + QF_CH - 1) / QF_CH)), dim3(TPB), 0, st, rec, (int)N, g.S, (int)C,
                           (int)HW, err);
    });
    return launch_status();
}

// ---- `-sm collect -sba`: the per-sample channel extrema (cnnq_sample_extrema.hip.h) -------------------------------------------------
// the argument checks of the contiguous bf16 / fp16 form: 0 - the plan exists (the fp32 entry points' geometry limits, N and
// C * HW below 2^31, and N * C rows below 2^31, which bounds the grid too).  fp32 has no kernel here: CNNQ_ENOTSUP.
static int h_se_check(int64_t N, int64_t C, int64_t HW, int dtype, bool ok) {
    if (!dtype_ok(dtype) || N < 1 || C < 1 || HW < 1 || !ok) return CNNQ_EINVAL;
    if (dtype == CNNQ_DTYPE_F32) return CNNQ_ENOTSUP;
    const int G0 = cnnq_pc_groups(N, C, HW, 0);
    if (G0 <= 0) return g_error(G0);
    return N * C >= ((int64_t)1 << 31) ? CNNQ_ERANGE : 0;
}

// Which launch cnnq_pc_sample_extrema_dt makes for this geometry (host only; smpc.py:72-78): out = {lanes per row seg, rows per
// workgroup (whole steps of TPB / seg rows), workgroups, 1 - the native launch / 0 - a class of layer that did not win against the
// former route and stays there: h_sample_extrema_native}.  The plan does not depend on the alignment: the kernel finds every
// row's 16-byte boundary itself.
int cnnq_pc_route_sample_extrema_dt(int64_t N, int64_t C, int64_t HW, int dtype, int align_bytes, int32_t out[4]) {
    if (const int rc = h_se_check(N, C, HW, dtype, out && pow2(align_bytes))) return rc;
    const int64_t rows = N * C;
    const int seg = h_se_seg(HW), rpw = h_se_steps(rows, HW, seg) * (TPB / seg);
    out[0] = seg;
    out[1] = rpw;
    out[2] = (int32_t)((rows + rpw - 1) / rpw);
    out[3] = h_sample_extrema_native(N, C, HW, dtype);
    return 0;
}

// smpc.py:72-78 (the per-sample extrema behind the batch mean) on x[N][C][HW] of bf16 / fp16: k_h_sample_extrema, one launch
int cnnq_pc_sample_extrema_dt(const void* x, int dtype, int64_t N, int64_t C, int64_t HW, float* ext, void* stream) {
    if (const int rc = h_se_check(N, C, HW, dtype, x && ext && !misaligned(x, 2) && !misaligned(ext, 4))) return rc;
    const int64_t rows = N * C;
    const int seg = h_se_seg(HW), steps = h_se_steps(rows, HW, seg);
    const int64_t rpw = (int64_t)steps * (TPB / seg);
    const dim3 grid((unsigned)((rows + rpw - 1) / rpw));
    const uint16_t* xh = static_cast<const uint16_t*>(x);
    if (dtype == CNNQ_DTYPE_BF16) hipLaunchKernelGGL(k_h_sample_extrema<HBf16>, grid, dim3(TPB), 0, hs(stream), xh, rows, (int)HW, seg, steps, ext);
    else hipLaunchKernelGGL(k_h_sample_extrema<HF16>, grid, dim3(TPB), 0, hs(stream), xh, rows, (int)HW, seg, steps, ext);
    return launch_status();
}

// the argument checks of the channels_last form: 0 - the plan exists (N, HW, N * C and the grid N * S * nb stay in 32 bits)
static int cl_se_check(int64_t N, int64_t HW, int64_t C, int dtype) {
    if (!dtype_ok(dtype) || N < 1 || HW < 1 || C < 1 || C > CL_C_MAX) return CNNQ_EINVAL;
    if (N >= ((int64_t)1 << 31) || HW >= ((int64_t)1 << 31) || N * C >= ((int64_t)1 << 31)) return CNNQ_ERANGE;
    const int64_t nbmax = (C + TPB - 1) / TPB;      // column blocks of the narrowest piece
    return N * cl_se_slabs(N, HW, C, cl_esize(dtype)) * nbmax >= ((int64_t)1 << 31) ? CNNQ_ERANGE : 0;
}

// ws of cnnq_pc_sample_extrema_nhwc, floats: the partial pairs [N * S][2][C] - N * S * 2 * C * 4 bytes; 0 at S == 1 (no workspace:
// the one launch stores ext) and on arguments the call refuses
size_t cnnq_pc_sample_extrema_nhwc_workspace(int64_t N, int64_t HW, int64_t C, int dtype) {
    if (cl_se_check(N, HW, C, dtype)) return 0;
    const int S = cl_se_slabs(N, HW, C, cl_esize(dtype));
    return S == 1 ? 0 : (size_t)N * (size_t)S * 2 * (size_t)C * sizeof(float);
}

// Which launches cnnq_pc_sample_extrema_nhwc makes for this geometry (host only; smpc.py:72-78): out = {elements per load W, slabs
// per sample S (1: one launch, no workspace), column blocks nb - the grid is N * S * nb, 1 - the native launches / 0 - a class of
// layer that did not win against the former route and stays there: cl_sample_extrema_native}
int cnnq_pc_route_sample_extrema_nhwc(int64_t N, int64_t HW, int64_t C, int dtype, int align_bytes, int32_t out[4]) {
    if (!out || !pow2(align_bytes)) return CNNQ_EINVAL;
    if (const int rc = cl_se_check(N, HW, C, dtype)) return rc;
    const int es = cl_esize(dtype), w = cl_piece(C, es, align_bytes);
    const ClGeo g = cl_geo_se(N, HW, C, w, es);
    out[0] = w;
    out[1] = g.S;
    out[2] = g.nb;
    out[3] = cl_sample_extrema_native(N, HW, C, dtype);
    return 0;
}

// smpc.py:72-78 on [N][HW][C]: k_cl_sample_extrema (-> k_sample_extrema_fold on its partial pairs, S > 1)
int cnnq_pc_sample_extrema_nhwc(const void* x, int dtype, int64_t N, int64_t HW, int64_t C, void* ws, float* ext, void* stream) {
    if (!x || !ext || misaligned(ext, 4) || misaligned(ws, 4)) return CNNQ_EINVAL;
    if (const int rc = cl_se_check(N, HW, C, dtype)) return rc;
    const int es = cl_esize(dtype);
    if (misaligned(x, (uintptr_t)es)) return CNNQ_EINVAL;
    const int w = cl_piece(C, es, h_align(x, x));
    const ClGeo g = cl_geo_se(N, HW, C, w, es);
    if (g.S > 1 && !ws) return CNNQ_EINVAL;
    hipStream_t st = hs(stream);
    float* part = static_cast<float*>(ws);
    const dim3 grid((unsigned)(N * g.S * g.nb));
    const int rc = cl_launch(dtype, w, x, [&](auto pc, auto* xr) {
        using P = decltype(pc);
        hipLaunchKernelGGL((k_cl_sample_extrema<typename P::T, P::W>), grid, dim3(TPB), 0, st, xr, g, (int)N, part, ext);
    });
    if (rc || g.S == 1) return rc;
    const int64_t NC = N * C;
    hipLaunchKernelGGL(k_sample_extrema_fold, dim3((unsigned)((NC + TPB - 1) / TPB)), dim3(TPB), 0, st, part, NC, (int)C, g.S, ext);
    return launch_status();
}

// ---- config 5 on dense channels_last activations (cnnq_nhwc_midtread.hip.h) ----------------------------------------------------
// Which launches cnnq_pc_midtread_nhwc makes for this geometry (host only): cnnq_pc_route_aciq_nhwc's report with out[4] the
// workgroups of the Q/DQ launch without (hist = 0) or with the code histogram.  out[5] is 1 throughout: no class of layer is sent
// back to the copy route; one that measures slower native than through the copy (tools/bench_channels_last_midtread.py) goes back here.
int cnnq_pc_route_midtread_nhwc(int64_t R, int64_t C, int dtype, int align_bytes, int hist, int32_t out[6]) {
    const int rc = cnnq_pc_route_aciq_nhwc(R, C, dtype, align_bytes, out);
    if (rc) return rc;
    if (hist) {
        const ClGeo g = cl_geo_hist(R, C, out[0]);
        out[4] = g.S * g.nb;
    }
    return 0;
}

static int cl_mt_qdq(const void* x, void* y, int dtype, const ClPlan& p, int64_t R, int64_t C, const float* mt, uint64_t* hist, hipStream_t st) {
    const ClGeo g = hist ? cl_geo_hist(R, C, p.w) : p.q;
    const dim3 grid((unsigned)(g.S * g.nb));
    return cl_launch(dtype, p.w, x, y, [&](auto pc, auto* xr, auto* yr) {
        with_bool(hist != nullptr, [&](auto h) {
            using P = decltype(pc);
            hipLaunchKernelGGL((k_cl_mt_qdq<typename P::T, P::W, decltype(h)::value>), grid, dim3(TPB), 0, st, xr, yr, g, mt, u64p(hist));
        });
    });
}

// iq.py:202-224 on [R][C] with a given table mt (cnnq_pc_midtread_params, clip = 1): one launch
int cnnq_pc_midtread_qdq_nhwc(const void* x, void* y, int dtype, int64_t R, int64_t C, const float* mt, uint64_t* hist, void* stream) {
    if (cl_check(R, C, dtype)) return CNNQ_EINVAL;
    if (!x || !y || x == y || !mt || misaligned(hist, 8)) return CNNQ_EINVAL;
    const ClPlan p(R, C, dtype, h_align(x, y));
    if (const int rc = p.range(false)) return rc;
    return cl_mt_qdq(x, y, dtype, p, R, C, mt, hist, hs(stream));
}

// iq.py:170-225 (per-channel statistics, bin allocation eq. 10, Laplace clipping, mid-tread Q/DQ) on [R][C]:
// cl_table with pass B -> k_mt_params -> k_cl_mt_qdq
int cnnq_pc_midtread_nhwc(const void* x, void* y, int dtype, int64_t R, int64_t C, double target, int sym, const double* tables, int ntab,
                          void* ws, float* stats, float* mt, uint64_t* hist, void* stream) {
    if (cl_check(R, C, dtype)) return CNNQ_EINVAL;
    if (!x || !y || x == y || !tables || ntab < 2 || !ws || !stats || !mt || misaligned(ws, 8) || misaligned(hist, 8)) return CNNQ_EINVAL;
    if (!(target - target == 0.)) return CNNQ_EINVAL;                                    // NaN or infinite
    const ClPlan p(R, C, dtype, h_align(x, y));
    if (const int rc = p.range(false)) return rc;
    hipStream_t st = hs(stream);
    if (hist && hipMemsetAsync(hist, 0, (size_t)CNNQ_MT_HIST_WORDS(C) * sizeof(uint64_t), st) != hipSuccess) return launch_status();
    int rc = cl_table(x, dtype, R, C, p, /*need_b=*/true, false, false, ws, nullptr, stats, stream);
    if (!rc) rc = cnnq_pc_midtread_params(stats, C, target, 1, sym, tables, ntab, mt, stream);
    if (!rc) rc = cl_mt_qdq(x, y, dtype, p, R, C, mt, hist, st);
    return rc;
}

// ---- the uniform Q/DQ that counts its codes (-me) on dense channels_last activations (cnnq_nhwc_entropy.hip.h) ------------------
static size_t cl_hist_lds(int nbins) { return (size_t)nbins * HREP * sizeof(unsigned); }

// Which launch the counting pass makes for this geometry (host only): out = {elements per load W, workgroups of the counting
// launch, its dynamic LDS bytes, 1 - the native launch}.  out[3] is 1 throughout: no class of layer is sent back to the copy
// route; one that measures slower native than through the copy (tools/bench_channels_last_entropy.py) goes back here, with the
// figure next to the rule.
int cnnq_pc_route_qdq_hist_nhwc(int64_t R, int64_t C, int dtype, int align_bytes, int nbins, int32_t out[4]) {
    return cl_route(R, C, dtype, align_bytes, out, /*rows32=*/false, hist_bins_ok(nbins), [&](const ClPlan& p) {
        const ClGeo g = cl_geo_hist(R, C, p.w);
        out[0] = p.w;
        out[1] = g.S * g.nb;
        out[2] = (int32_t)cl_hist_lds(nbins);
        out[3] = 1;
        return 0;
    });
}

static int cl_qdq_hist(const void* x, void* y, int dtype, const ClPlan& p, int64_t R, int64_t C, const float* qp, int nbins, uint64_t* hist_rep,
                       hipStream_t st) {
    const ClGeo g = cl_geo_hist(R, C, p.w);          // at most p.q's workgroups: inside ClPlan::range
    const dim3 grid((unsigned)(g.S * g.nb));
    return cl_launch(dtype, p.w, x, y, [&](auto pc, auto* xr, auto* yr) {
        using P = decltype(pc);
        hipLaunchKernelGGL((k_cl_qdq_hist<typename P::T, P::W>), grid, dim3(TPB), cl_hist_lds(nbins), st, xr, yr, g, qp, nbins, u64p(hist_rep));
    });
}

// int_quantizer.py:573-592 on [R][C] with a given table, and the codes of 586-587 counted into hist_rep: one launch
int cnnq_pc_qdq_hist_nhwc(const void* x, void* y, int dtype, int64_t R, int64_t C, const float* qp, int nbins, uint64_t* hist_rep, void* stream) {
    if (cl_check(R, C, dtype)) return CNNQ_EINVAL;
    if (!x || !y || x == y || !qp || !hist_rep || misaligned(hist_rep, 8) || !hist_bins_ok(nbins)) return CNNQ_EINVAL;
    const ClPlan p(R, C, dtype, h_align(x, y));
    if (const int rc = p.range(false)) return rc;
    return cl_qdq_hist(x, y, dtype, p, R, C, qp, nbins, hist_rep, hs(stream));
}

// int_quantizer.py:409-451, 557-603 with 586-587 on [R][C]: cl_minmax_front -> k_cl_qdq_hist with 2^num_bits bins
int cnnq_pc_minmax_qdq_hist_nhwc(const void* x, void* y, int dtype, int64_t R, int64_t C, int num_bits, int positive, float* ws, float* qp,
                                 float* mm, uint64_t* hist_rep, void* stream) {
    if (cl_check(R, C, dtype)) return CNNQ_EINVAL;
    if (!x || !y || x == y || !ws || !qp || !hist_rep || misaligned(ws, 4) || misaligned(hist_rep, 8)) return CNNQ_EINVAL;
    if (num_bits < 1 || num_bits > 8) return CNNQ_EINVAL;                                // the codes fit a byte, the bins 256
    const ClPlan p(R, C, dtype, h_align(x, y));
    if (const int rc = p.range(false)) return rc;
    float* ext;
    int rc = cl_minmax_front(x, dtype, C, p, num_bits, positive, ws, qp, mm, &ext, stream);
    if (!rc) rc = cl_qdq_hist(x, y, dtype, p, R, C, qp, 1 << num_bits, hist_rep, hs(stream));
    return rc;
}

// int_quantizer.py:327-352 + 409-451, 557-603 with 586-587 on [R][C]: cl_aciq_front -> k_cl_qdq_hist; 256 bins under bit
// allocation (the channels' qmax is decided on the device), else 2^num_bits
int cnnq_pc_aciq_qdq_hist_nhwc(const void* x, void* y, int dtype, int64_t R, int64_t C, const cnnq_params_cfg* cfg, void* ws, float* stats,
                               float* qp, float* diag, uint64_t* hist_rep, void* stream) {
    if (cl_aciq_check(x, y, dtype, R, C, cfg, ws, stats, qp, diag)) return CNNQ_EINVAL;
    if (x == y || !hist_rep || misaligned(hist_rep, 8) || cfg->num_bits > 8) return CNNQ_EINVAL;
    const ClPlan p(R, C, dtype, h_align(x, y));
    if (const int rc = p.range(false)) return rc;
    int rc = cl_aciq_front(x, dtype, R, C, p, cfg, ws, stats, qp, diag, stream);
    if (!rc) rc = cl_qdq_hist(x, y, dtype, p, R, C, qp, cfg_bit_alloc(cfg) ? 256 : 1 << cfg->num_bits, hist_rep, hs(stream));
    return rc;
}

// ---- activation bias correction on dense channels_last activations (cnnq_nhwc_bcorr.hip.h) --------------------------------------
// ws of cnnq_pc_qdq_bcorr_nhwc, doubles: part3[S][3][C]
size_t cnnq_pc_qdq_bcorr_nhwc_workspace(int64_t R, int64_t C, int dtype) {
    if (cl_check(R, C, dtype)) return 0;
    return (size_t)cl_slabs_max(R, C, dtype) * 3 * (size_t)C * sizeof(double);
}

// iqm.py:180-196 folded into int_quantizer.py:573-592 on [R][C] with a given table (-sm use):
// k_cl_bcorr_sums (ascending) -> k_bcorr_bias on its S records -> k_cl_qdq_bias (descending)
int cnnq_pc_qdq_bcorr_nhwc(const void* x, void* y, int dtype, int64_t R, int64_t C, const float* qp, int relu_first, void* ws,
                           double* sums, float* bias, void* stream) {
    if (cl_check(R, C, dtype)) return CNNQ_EINVAL;
    if (!x || !y || x == y || !qp || !ws || !bias || misaligned(ws, 8) || misaligned(sums, 8)) return CNNQ_EINVAL;
    const ClPlan p(R, C, dtype, h_align(x, y));
    if (const int rc = p.range(true)) return rc;                                         // a lane counts its rows in 32 bits
    double* part3 = static_cast<double*>(ws);
    hipStream_t st = hs(stream);
    int rc = cl_launch(dtype, p.w, x, [&](auto pc, auto* xr) {
        using P = decltype(pc);
        hipLaunchKernelGGL((k_cl_bcorr_sums<typename P::T, P::W>), p.mgrid(), dim3(TPB), 0, st, xr, p.m, relu_first ? 1 : 0, qp, part3);
    });
    if (!rc) rc = cnnq_pc_bcorr_bias(part3, p.m.S, C, sums, bias, stream);
    if (rc) return rc;
    return cl_launch(dtype, p.w, x, y, [&](auto pc, auto* xr, auto* yr) {
        using P = decltype(pc);
        hipLaunchKernelGGL((k_cl_qdq_bias<typename P::T, P::W>), p.qgrid(), dim3(TPB), 0, st, xr, yr, p.q, qp, bias);
    });
}

// ---- integer codes as the stored format of dense channels_last activations (cnnq_nhwc_packed.hip.h) ------------------------------
size_t cnnq_pc_packed_nhwc_capacity(int64_t R, int64_t C) {
    if (R < 1 || C < 1) return 0;
    return (size_t)R * 4 * (size_t)cl_pk_capdw(C);
}

int cnnq_pc_packed_layout_nhwc(const float* bits, int uniform_bits, int64_t C, uint32_t* coloff, void* stream) {
    if (!coloff || C < 1 || C > CL_C_MAX) return CNNQ_EINVAL;
    if (!bits && (uniform_bits < 0 || uniform_bits > 8)) return CNNQ_EINVAL;
    hipLaunchKernelGGL(k_cl_packed_layout, dim3(1), dim3(PTPB), 0, hs(stream), bits, uniform_bits, (int)C, coloff);
    return launch_status();
}

// Which launch cnnq_pc_quantize_packed_nhwc makes for this geometry (host only).  out[3] is 0 only for a row image beyond
// CL_PK_IMG (C > 8192): a class of layer the pack kernel cannot stage.  No class is sent back to the copy route for speed; one
// that measures slower native than through the copy beyond the run's spread (tools/bench_channels_last_packed.py,
// profiles/channels_last_packed.md) goes back here.
int cnnq_pc_route_packed_nhwc(int64_t R, int64_t C, int dtype, int align_bytes, int32_t out[4]) {
    return cl_route(R, C, dtype, align_bytes, out, /*rows32=*/false, /*ok=*/true, [&](const ClPlan& p) {
        out[0] = p.w;
        out[1] = out[2] = out[3] = 0;
        if (!cl_pk_native(C)) return 0;
        const PkGeo g = cl_pk_geo(R, C, p.w);
        if (cl_pk_wgs(g) >= ((int64_t)1 << 31) || g.rpw >= ((int64_t)1 << 31)) return (int)CNNQ_ERANGE;
        out[1] = (int32_t)cl_pk_wgs(g);
        out[2] = (int32_t)g.rpw;
        out[3] = 1;
        return 0;
    });
}

// the pack launch.  uniform: the width every channel has when the host knows it (the one-call fronts), else -1; it selects the
// register-to-memory form where every piece's run is whole dwords
static int cl_pack(const void* x, int dtype, int64_t R, int64_t C, const ClPlan& p, const float* qp, const float* mm, const uint32_t* coloff,
                   uint8_t* packed, int uniform, hipStream_t st) {
    if (!cl_pk_native(C)) return CNNQ_ENOTSUP;
    const PkGeo g = cl_pk_geo(R, C, p.w);
    if (cl_pk_wgs(g) >= ((int64_t)1 << 31)) return CNNQ_ERANGE;
    const bool direct = uniform > 0 && (p.w * uniform) % 32 == 0;
    uint32_t* out = reinterpret_cast<uint32_t*>(packed);
    return cl_launch(dtype, p.w, x, [&](auto pc, auto* xr) {
        using P = decltype(pc);
        if constexpr (P::W >= 4) {
            if (direct) {
                hipLaunchKernelGGL((k_cl_pack<typename P::T, P::W, true>), dim3((unsigned)cl_pk_wgs(g)), dim3(TPB), 0, st, xr, out, g, qp, mm, coloff);
                return;
            }
        }
        hipLaunchKernelGGL((k_cl_pack<typename P::T, P::W, false>), dim3((unsigned)cl_pk_wgs(g)), dim3(TPB), 0, st, xr, out, g, qp, mm, coloff);
    });
}

static int cl_pack_check(const void* x, int dtype, int64_t R, int64_t C, const float* qp, const uint32_t* coloff, const uint8_t* packed) {
    if (cl_check(R, C, dtype)) return CNNQ_EINVAL;
    return (!x || !qp || !coloff || !packed || misaligned(packed, 4)) ? CNNQ_EINVAL : 0;
}

int cnnq_pc_quantize_packed_nhwc(const void* x, int dtype, int64_t R, int64_t C, const float* qp, const float* mm, const uint32_t* coloff,
                                 uint8_t* packed, void* stream) {
    if (cl_pack_check(x, dtype, R, C, qp, coloff, packed)) return CNNQ_EINVAL;
    const ClPlan p(R, C, dtype, h_align(x, x));
    if (const int rc = p.range(false)) return rc;
    return cl_pack(x, dtype, R, C, p, qp, mm, coloff, packed, -1, hs(stream));
}

int cnnq_pc_dequantize_packed_nhwc(const uint8_t* packed, void* y, int dtype, int64_t R, int64_t C, const float* qp, const uint32_t* coloff,
                                   void* stream) {
    if (cl_pack_check(y, dtype, R, C, qp, coloff, packed)) return CNNQ_EINVAL;
    const ClPlan p(R, C, dtype, h_align(y, y));
    if (const int rc = p.range(false)) return rc;
    const uint32_t* in = reinterpret_cast<const uint32_t*>(packed);
    return cl_launch(dtype, p.w, nullptr, y, [&](auto pc, auto*, auto* yr) {
        using P = decltype(pc);
        hipLaunchKernelGGL((k_cl_unpack<typename P::T, P::W>), p.qgrid(), dim3(TPB), 0, hs(stream), in, yr, p.q, qp, coloff, cl_pk_capdw(C));
    });
}

// int_quantizer.py:409-451, 557-587 on [R][C], the codes kept: cl_minmax_front -> k_cl_packed_layout (uniform) -> k_cl_pack with the extrema
int cnnq_pc_minmax_quantize_packed_nhwc(const void* x, int dtype, int64_t R, int64_t C, int num_bits, int positive, float* ws, float* qp,
                                        float* mm, uint32_t* coloff, uint8_t* packed, void* stream) {
    if (cl_pack_check(x, dtype, R, C, qp, coloff, packed)) return CNNQ_EINVAL;
    if (!ws || misaligned(ws, 4) || num_bits < 1 || num_bits > 8) return CNNQ_EINVAL;
    if (!cl_pk_native(C)) return CNNQ_ENOTSUP;
    const ClPlan p(R, C, dtype, h_align(x, x));
    if (const int rc = p.range(false)) return rc;
    float* ext;
    int rc = cl_minmax_front(x, dtype, C, p, num_bits, positive, ws, qp, mm, &ext, stream);
    if (!rc) rc = cnnq_pc_packed_layout_nhwc(nullptr, num_bits, C, coloff, stream);
    if (!rc) rc = cl_pack(x, dtype, R, C, p, qp, ext, coloff, packed, num_bits, hs(stream));
    return rc;
}

// int_quantizer.py:327-352 + 409-451, 557-587 on [R][C], the codes kept: cl_aciq_front -> k_cl_packed_layout (the allocated widths, or
// cfg->num_bits) -> k_cl_pack with the table
int cnnq_pc_aciq_quantize_packed_nhwc(const void* x, int dtype, int64_t R, int64_t C, const cnnq_params_cfg* cfg, void* ws, float* stats,
                                      float* qp, float* diag, uint32_t* coloff, uint8_t* packed, void* stream) {
    if (cl_aciq_check(x, packed, dtype, R, C, cfg, ws, stats, qp, diag)) return CNNQ_EINVAL;
    if (!coloff || misaligned(packed, 4) || cfg->num_bits > 8) return CNNQ_EINVAL;
    if (!cl_pk_native(C)) return CNNQ_ENOTSUP;
    const ClPlan p(R, C, dtype, h_align(x, x));
    if (const int rc = p.range(false)) return rc;
    const bool ba = cfg_bit_alloc(cfg);
    int rc = cl_aciq_front(x, dtype, R, C, p, cfg, ws, stats, qp, diag, stream);
    if (!rc) rc = cnnq_pc_packed_layout_nhwc(ba ? diag + (size_t)CNNQ_DIAG_BITS * C : nullptr, ba ? 0 : cfg->num_bits, C, coloff, stream);
    if (!rc) rc = cl_pack(x, dtype, R, C, p, qp, nullptr, coloff, packed, ba ? -1 : cfg->num_bits, hs(stream));
    return rc;
}


// ---- statistics of few, very long rows over flat storage (cnnq_rows.hip.h): x [rows][len], fp32 / bf16 / fp16 -------------------
// What the three entry points derive from (rows, len, dtype, alignment) after their argument checks: the piece width and the
// geometry.  CNNQ_ERANGE: 2^31 rows (the merge kernels index the records' columns in 32 bits), a chunk of 2^31 pieces (out[2] of
// the route function), or a tensor whose byte offsets leave 63 bits.
static int rows_check(int64_t rows, int64_t len, int dtype) { return (!dtype_ok(dtype) || rows < 1 || len < 1) ? CNNQ_EINVAL : 0; }
static int rows_plan(int64_t rows, int64_t len, int dtype, int align_bytes, int* w, RowsGeo* g) {
    if (rows >= ((int64_t)1 << 31) || len > (INT64_MAX >> 3) / rows) return CNNQ_ERANGE;
    *w = cl_piece(len, cl_esize(dtype), align_bytes);
    *g = rows_geo(rows, len, *w);
    return g->ppc >= ((int64_t)1 << 31) ? CNNQ_ERANGE : 0;
}

// ws, doubles: part[S][CNNQ_NMOM][rows], mom[CNNQ_NMOM][rows], part2[S][CNNQ_NDEV][rows] (AciqWs without the table) for the largest
// S over the piece widths len allows (the alignment is not known yet)
size_t cnnq_rows_stats_workspace(int64_t rows, int64_t len, int dtype) {
    if (rows_check(rows, len, dtype) || rows >= ((int64_t)1 << 31)) return 0;
    int64_t S = 1;
    for (int w = 16 / cl_esize(dtype); w >= 1; w >>= 1) {
        if (len % w) continue;
        const int64_t s = rows_geo(rows, len, w).S;
        S = s > S ? s : S;
    }
    return AciqWs::bytes((size_t)S, rows, false);
}

// Which launches cnnq_rows_stats makes for this geometry (host only): out = {elements per load W, chunks per row S, pieces per
// chunk, 1 - the row is summed in fp64 throughout}.  No class of tensor is sent back to the copy route: none measured slower
// native than through the copy (tools/bench_tensor_collect.py); one that does gets its rule here, with the figures next to it.
int cnnq_rows_stats_route(int64_t rows, int64_t len, int dtype, int align_bytes, int32_t out[4]) {
    if (rows_check(rows, len, dtype) || !out || !pow2(align_bytes) || align_bytes < cl_esize(dtype)) return CNNQ_EINVAL;
    int w;
    RowsGeo g;
    if (const int rc = rows_plan(rows, len, dtype, align_bytes, &w, &g)) return rc;
    out[0] = w;
    out[1] = g.S;
    out[2] = (int32_t)g.ppc;
    out[3] = g.exact;
    return 0;
}

// statistic_manager.py:55-96 (rows = 1) and distance_stats.py:22-33 (rows = N) on the storage as it lies: k_rows_moments ->
// k_combine(has_relu) (-> k_rows_absdev on the merged table -> k_combine_dev(want_kurt); need_dev), two or four launches
int cnnq_rows_stats(const void* x, int dtype, int64_t rows, int64_t len, int need_dev, void* ws, double* mom, float* stats, void* stream) {
    if (rows_check(rows, len, dtype)) return CNNQ_EINVAL;
    if (!x || !ws || !stats || misaligned(ws, 8) || misaligned(mom, 8) || misaligned(x, (uintptr_t)cl_esize(dtype))) return CNNQ_EINVAL;
    int w;
    RowsGeo g;
    if (const int rc = rows_plan(rows, len, dtype, h_align(x, x), &w, &g)) return rc;
    const AciqWs a(ws, g.S, rows);
    double* rec = mom ? mom : a.mom;
    hipStream_t st = hs(stream);
    int rc = cl_launch(dtype, w, x, [&](auto pc, auto* xr) {
        using P = decltype(pc);
        hipLaunchKernelGGL((k_rows_moments<typename P::T, P::W>), rows_grid(g), dim3(TPB), 0, st, xr, g, a.part);
    });
    if (!rc) rc = cnnq_pc_combine(a.part, g.S, rows, 1, rec, stats, stream);
    if (rc || !need_dev) return rc;
    rc = cl_launch(dtype, w, x, [&](auto pc, auto* xr) {
        using P = decltype(pc);
        hipLaunchKernelGGL((k_rows_absdev<typename P::T, P::W>), rows_grid(g), dim3(TPB), 0, st, xr, g, stats, a.part2);
    });
    if (!rc) rc = cnnq_pc_combine_dev(a.part2, g.S, rows, rec, 1, nullptr, stats, stream);
    return rc;
}


// ---- per-tensor clipping and mid-tread over flat storage (cnnq_flat.hip.h): x and y [n], fp32 / bf16 / fp16 ---------------------
// What every entry point of the family refuses before anything touches the device
static int flat_check(const void* x, const void* y, int dtype, int64_t n) {
    if (!dtype_ok(dtype) || n < 1 || !x || !y || x == y) return CNNQ_EINVAL;
    if (misaligned(x, (uintptr_t)cl_esize(dtype)) || misaligned(y, (uintptr_t)cl_esize(dtype))) return CNNQ_EINVAL;
    if (n > (INT64_MAX >> 3)) return CNNQ_ERANGE;
    return flat_blocks(n, flat_piece(cl_esize(dtype), h_align(x, y))) >= ((int64_t)1 << 31) ? CNNQ_ERANGE : 0;
}
// the launch of k_flat_qdq (midtread = false) or k_flat_midtread on a checked tensor
static int flat_launch(bool midtread, const void* x, void* y, int dtype, int64_t n, const float* tab, void* stream) {
    const int w = flat_piece(cl_esize(dtype), h_align(x, y));
    const dim3 grid((unsigned)flat_blocks(n, w));
    return cl_launch(dtype, w, x, y, [&](auto pc, auto* xr, auto* yr) {
        using P = decltype(pc);
        if (midtread) hipLaunchKernelGGL((k_flat_midtread<typename P::T, P::W>), grid, dim3(TPB), 0, hs(stream), xr, yr, n, tab);
        else hipLaunchKernelGGL((k_flat_qdq<typename P::T, P::W>), grid, dim3(TPB), 0, hs(stream), xr, yr, n, tab);
    });
}

int cnnq_flat_qdq(const void* x, void* y, int dtype, int64_t n, const float* qp, void* stream) {
    if (const int rc = flat_check(x, y, dtype, n)) return rc;
    if (!qp) return CNNQ_EINVAL;
    return flat_launch(false, x, y, dtype, n, qp, stream);
}

int cnnq_flat_midtread_qdq(const void* x, void* y, int dtype, int64_t n, const float* mt, void* stream) {
    if (const int rc = flat_check(x, y, dtype, n)) return rc;
    if (!mt) return CNNQ_EINVAL;
    return flat_launch(true, x, y, dtype, n, mt, stream);
}

// ws of cnnq_pt_clip_qdq / cnnq_pt_midtread: the records of cnnq_rows_stats on one row of n elements
size_t cnnq_pt_clip_workspace(int64_t n, int dtype) { return cnnq_rows_stats_workspace(1, n, dtype); }

// iq.py:353-357 in one host call: the whole-tensor table (pass B only where the clipping reads b: Laplace), the parameters of
// one channel with delta = the range itself, the flat Q/DQ
int cnnq_pt_clip_qdq(const void* x, void* y, int dtype, int64_t n, const cnnq_params_cfg* cfg, void* ws, float* stats, float* qp, float* diag,
                     void* stream) {
    if (const int rc = flat_check(x, y, dtype, n)) return rc;
    if (!cfg || !ws || !stats || !qp || misaligned(ws, 8)) return CNNQ_EINVAL;
    if (check_cfg(cfg) || cfg->clip == 0 || cfg->bit_alloc) return CNNQ_EINVAL;
    cnnq_params_cfg c = *cfg;
    c.direct_range = 1;
    int rc = cnnq_rows_stats(x, dtype, 1, n, c.clip == 1, ws, nullptr, stats, stream);
    if (!rc) rc = cnnq_pc_params(stats, 1, &c, qp, diag, stream);
    if (!rc) rc = flat_launch(false, x, y, dtype, n, qp, stream);
    return rc;
}

// iq.py:158-168 without -pcq_a in one host call: the whole-tensor table with b, step size and clamp bounds of one channel, the flat pass
int cnnq_pt_midtread(const void* x, void* y, int dtype, int64_t n, double target, int sym, const double* tables, int ntab, void* ws,
                     float* stats, float* mt, void* stream) {
    if (const int rc = flat_check(x, y, dtype, n)) return rc;
    if (!tables || ntab < 2 || !ws || !stats || !mt || misaligned(ws, 8) || !(target - target == 0.)) return CNNQ_EINVAL;
    int rc = cnnq_rows_stats(x, dtype, 1, n, 1, ws, nullptr, stats, stream);
    if (!rc) rc = cnnq_pc_midtread_params(stats, 1, target, 1, sym, tables, ntab, mt, stream);
    if (!rc) rc = flat_launch(true, x, y, dtype, n, mt, stream);
    return rc;
}

}  // extern "C"
