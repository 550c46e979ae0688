/*
 * cnnq_hip.h - C ABI of libcnnq_hip.so: MI355X (gfx950) kernels for the GEMMLOWP-style
 * per-channel quantize / clip / dequantize hot path of submission2019/cnn-quantization.
 *
 * This is the drop-in boundary.  The reference's only native module is
 *     kernels/int_quantization.cpp:10-12  ->  float2gemmlowp(in, range, offset, num_bits,
 *                                             int_exp, enforce_true_zero, noise)
 *     kernels/gemmlowp.cu:8-45            (kernel + host wrapper)
 * which cnnq_pt_qdq replaces one for one.  Everything else the reference does on this path
 * is a chain of aten ops inside pytorch_quantizer/quantization/qtypes/int_quantizer.py
 * (abbreviated iq.py) and pytorch_quantizer/quantization/inference/
 * statistic_manager_perchannel.py (smpc.py); each entry point below names the lines it fuses.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless it says "host";
 *   - activations are fp32 NCHW, addressed as x[N][C][HW] (HW = H*W contiguous floats);
 *     weights [OFM][IFM*K*K] are the same layout with N = 1, C = OFM;
 *     per-sample statistics of any tensor are the same layout with N = 1, C = samples;
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); kernels are
 *     enqueued, never synchronised; nothing is allocated, every function is re-entrant; the
 *     library keeps no state and reads ONE environment variable, once per process:
 *     CNNQ_NT_BYTES (default 402653184) - tensors above it are streamed with non-temporal loads
 *     by the read-only passes (a property of the part's Infinity Cache; 0: always).  The kernel
 *     sweep knobs of the development builds (-DCNNQ_DEV_KNOBS) do not exist in this library;
 *   - return value: 0 on success, a positive hipError_t from the launch, or a negative
 *     CNNQ_E* for rejected arguments (nothing is enqueued then).
 */
#ifndef CNNQ_HIP_H
#define CNNQ_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CNNQ_EINVAL (-1) /* null pointer, non-positive size, unsupported option */
#define CNNQ_ERANGE (-2) /* C*HW does not fit the 31-bit plane index */
#define CNNQ_ENOTSUP (-3) /* this entry point has no kernel for the shape / alignment: use the general one */

/* Rows of the per-channel fp32 statistics table `stats[CNNQ_NSTAT][C]`
 * (iq.py:530-555 and smpc.py:54-79 name the same quantities). */
enum {
    CNNQ_STAT_MIN = 0,
    CNNQ_STAT_MAX = 1,
    CNNQ_STAT_MEAN = 2,
    CNNQ_STAT_STD = 3,     /* unbiased (n-1) */
    CNNQ_STAT_B = 4,       /* mean |x - mean| */
    CNNQ_STAT_KURT = 5,    /* mean(((x-mean)/std)^4) - 3 */
    CNNQ_STAT_STD_POS = 6, /* unbiased std of relu(x) */
    CNNQ_NSTAT = 7
};

/* Rows of the fp64 moment records `mom[CNNQ_NMOM][C]` that ranks exchange (all_gather) and
 * cnnq_pc_combine merges: partial results are mergeable, statistics are not. */
enum {
    CNNQ_MOM_MIN = 0,
    CNNQ_MOM_MAX = 1,
    CNNQ_MOM_SUM = 2,
    CNNQ_MOM_SUMSQ = 3,
    CNNQ_MOM_COUNT = 4,
    CNNQ_MOM_SUM_RELU = 5,
    CNNQ_MOM_SUMSQ_RELU = 6,
    CNNQ_NMOM = 7
};
/* Rows of the second-pass records `dev[CNNQ_NDEV][C]` (need the global mean / std). */
enum { CNNQ_DEV_ABS = 0, CNNQ_DEV_Z4 = 1, CNNQ_NDEV = 2 };

/* Rows of the quantisation parameter table `qp[CNNQ_NQP][C]` (iq.py:559-572). */
enum { CNNQ_QP_SCALE = 0, CNNQ_QP_ZP = 1, CNNQ_QP_QMAX = 2, CNNQ_NQP = 3 };
/* Rows of the diagnostic table `diag[CNNQ_NDIAG][C]` written by cnnq_pc_params. */
enum { CNNQ_DIAG_BITS = 0, CNNQ_DIAG_ALPHA = 1, CNNQ_DIAG_DELTA = 2, CNNQ_DIAG_OFFSET = 3, CNNQ_NDIAG = 4 };

/* Rows of the mid-tread parameter table `mt[CNNQ_NMT][C]` (row WSTART: the first integer code of the histogram
 * window, the same value in every column) and the size of its code histogram in uint64 words,
 * CNNQ_MT_HIST_WORDS(C): CNNQ_MT_HIST_BINS integer-code bins centred on 0, 2 out-of-range bins, 2*C counters for
 * codes clamped to a non-integer c_min[c] / c_max[c], then CNNQ_MT_HIST_REPLICAS copies of the
 * CNNQ_MT_HIST_WINDOW bins of the codes WSTART .. WSTART + WINDOW - 1 (workgroups spread their updates over the
 * copies; cnnq_midtread_entropy adds them up), and one flag word: non-zero when a count went to the
 * CNNQ_MT_HIST_BINS + 2 global bins, i.e. a code fell outside the window. */
enum {
    CNNQ_MT_DELTA = 0, CNNQ_MT_CMIN = 1, CNNQ_MT_CMAX = 2, CNNQ_MT_OMEGA = 3, CNNQ_MT_ALPHA = 4, CNNQ_MT_WSTART = 5,
    CNNQ_NMT = 6
};
#define CNNQ_MT_HIST_BINS 131072
#define CNNQ_MT_HIST_WINDOW 128
#define CNNQ_MT_HIST_REPLICAS 256
#define CNNQ_MT_HIST_WORDS(C) (CNNQ_MT_HIST_BINS + 2 + 2 * (C) + CNNQ_MT_HIST_REPLICAS * CNNQ_MT_HIST_WINDOW + 1)

/* library / build identification ("cnnq-hip <version> gfx950") */
const char* cnnq_version(void);

/* Number of partial groups G that the streaming statistics kernels emit per channel for a
 * tensor of this geometry; the caller sizes `part` as [G][CNNQ_NMOM][C] doubles (and
 * [G][CNNQ_NDEV][C] for the second pass).  `aligned16` = (x % 16 == 0).  Returns G > 0 or
 * a negative CNNQ_E*. */
int cnnq_pc_groups(int64_t N, int64_t C, int64_t HW, int aligned16);

/* Diagnostics (host only, nothing is enqueued): the launch plan the streaming kernels use for a
 * tensor - out = {vec, A, J, mode, nb, w, k, ncb, S, threads per workgroup, G, 0}: loads of `vec`
 * floats, A parameter sets per load (4 = a float4 may straddle two channels), J loads per lane per
 * sample; mode 1: a workgroup owns `w` loads of ONE channel (`nb` workgroups per channel), mode 2: `k`
 * whole channels; ncb column blocks x S batch splits workgroups; fine != 0: the short-workgroup
 * geometry of the table-driven elementwise passes.  tests/test_plan_cpu.py checks on the CPU that
 * these plans cover every element exactly once. */
int cnnq_plan_describe(int64_t N, int64_t C, int64_t HW, int aligned16, int fine, int32_t out[12]);

/* Pass A over x[N][C][HW]: per channel min, max, sum, sum of squares, count (and, when
 * want_relu, sum and sum of squares of relu(x)) -> part[G][CNNQ_NMOM][C].  One coalesced
 * read of x, no transposed copy.  Fuses the reductions of iq.py:534-550 (max/min/mean/std),
 * smpc.py:54-55,64-66 (mean, std, std_pos) that the reference runs as one full pass each
 * after a transpose+copy. */
int cnnq_pc_moments(const float* x, int64_t N, int64_t C, int64_t HW, int want_relu, double* part,
                    void* stream);

/* Merge G moment records per channel (G = groups of one tensor, or G = world size after an
 * all_gather of per-rank records) into mom[CNNQ_NMOM][C] and, when `stats` is not NULL, write
 * the whole table stats[CNNQ_NSTAT][C]: rows MIN, MAX, MEAN, STD, STD_POS (zero unless the records carry relu
 * sums), and zeros in rows B and KURT (cnnq_pc_combine_dev fills them after pass B).
 * Fixed merge order (a function of G and C) -> deterministic.  `mom` may be NULL. */
int cnnq_pc_combine(const double* part, int G, int64_t C, int has_relu, double* mom, float* stats,
                    void* stream);

/* Pass B: per channel sum |x - mean[c]| and (want_kurt) sum ((x-mean[c])/std[c])^4, reading
 * mean/std from stats rows MEAN/STD -> part2[G][CNNQ_NDEV][C].  iq.py:548 ('b'),
 * smpc.py:58-61 (kurtosis, b). */
int cnnq_pc_absdev(const float* x, int64_t N, int64_t C, int64_t HW, const float* stats, int want_kurt,
                   double* part2, void* stream);

/* All statistics of cnnq_pc_stats from ONE launch that reads x once (round 5; csrc/cnnq_stats1.hip.h): a workgroup keeps its
 * tile of x in registers (and LDS) across pass A and pass B, and the workgroups of a channel exchange their partial sums twice
 * through the slot region of the exchange workspace (cnnq_group_ws_alloc) - 4 instead of 8 bytes per element, one launch
 * instead of three; the same per-element arithmetic and final formulas as the chain, a different (fixed) order of the fp64
 * additions (round 6: nobody waits for the second exchange - the workgroup that arrives LAST folds it, writes the channel's row
 * and re-arms the slots; the others leave after publishing their words).  Flat-tile geometries (H*W % 4 == 0, H*W / 4 >= 128 and not a multiple of 256, 2 .. 512 tiles per channel), and
 * the row-piece tiles of cnnq_pc_minmax_qdq_group for shorter rows (k_stats_group).  CNNQ_ENOTSUP where the chain is faster:
 * more than 256 tiles per channel, row-piece geometries whose channels straddle the 16-byte loads (7x7) above 8 MB (flags
 * bit 3 lifts these two rules: tests), and where there is no 16-byte tiling at all.  (Round 6: every one-channel-per-lane
 * row-piece shape with a plan is taken - at a 64-sample shard the one launch of 20-45 us beats three launches and two merges.)
 * flags: 0 (tests: 1 = skip the waits and recompute).  cnnq_pc_stats_auto: this when it applies,
 * else cnnq_pc_stats (ws as there). */
int cnnq_pc_stats_single(const float* x, int64_t N, int64_t C, int64_t HW, int need_b, int need_kurt, int need_relu, void* gws,
                         size_t gws_bytes, double* mom, float* stats, unsigned flags, void* stream);
int cnnq_pc_stats_auto(const float* x, int64_t N, int64_t C, int64_t HW, int need_b, int need_kurt, int need_relu, void* ws, void* gws,
                       size_t gws_bytes, double* mom, float* stats, void* stream);
/* The route cnnq_pc_stats_single (flags as there) / cnnq_pc_stats_auto (flags 0) take for a geometry, without launching anything:
 * 1 - the flat-tile single launch, 2 - the row-piece single launch, 0 - the three-launch chain (cnnq_pc_stats_single would answer
 * CNNQ_ENOTSUP).  aligned16: x is 16-byte aligned; gws_bytes: the exchange workspace the caller holds (cnnq_pc_group_workspace). */
int cnnq_pc_stats_route(int64_t N, int64_t C, int64_t HW, int aligned16, size_t gws_bytes, unsigned flags);

/* Merge pass-B records; divides by the COUNT row of `mom` and writes stats rows B (and KURT).
 * `dev_out` (merged [CNNQ_NDEV][C] sums, for the cross-rank exchange) may be NULL, and
 * `stats` may be NULL when only the merged sums are wanted. */
int cnnq_pc_combine_dev(const double* part2, int G, int64_t C, const double* mom, int want_kurt,
                        double* dev_out, float* stats, void* stream);

/* All per-channel statistics of one tensor behind one call and one caller workspace `ws` of
 * cnnq_pc_stats_workspace(...) bytes (8-byte aligned): pass A -> pass B with the merge of the pass-A records fused
 * into its prologue -> one final merge of both passes (three launches for the seven statistics of smpc.py:45-79,
 * two when neither b nor kurtosis is wanted).  stats[CNNQ_NSTAT][C] is written completely (rows not requested are
 * zero); mom[CNNQ_NMOM][C] (merged moment record) may be NULL.  Single process: the cross-rank exchange needs the
 * separate calls above. */
size_t cnnq_pc_stats_workspace(int64_t N, int64_t C, int64_t HW, int aligned16);
int cnnq_pc_stats(const float* x, int64_t N, int64_t C, int64_t HW, int need_b, int need_kurt, int need_relu, void* ws,
                  double* mom, float* stats, void* stream);

/* Per-channel statistics -> quantisation parameters, entirely on the device (the reference
 * takes >= 6 host round trips here: iq.py:248,285-288,355,405).  One workgroup.
 *   clip: 0 = min/max range (iq.py:409-424), 1 = ACIQ laplace (iq.py:227-253),
 *         2 = ACIQ gaus (iq.py:255-264), 3 = p*std (iq.py:266-275, p = pstd);
 *   positive = force_positive || half_range (iq.py:289,411);
 *   bit_alloc != 0 (and num_bits <= 4): per-channel bit allocation from the prior statistic
 *         (prior_is_b ? B : STD) by the fixed-target iteration of iq.py:381-407 with
 *         `target` bits and round (1) or ceil (0);
 *   alpha2DeltaOffset (iq.py:284-300), delta = (offset + range) - offset (iq.py:351,443),
 *   scale / zero-point (iq.py:559-572).
 * Reads stats[CNNQ_NSTAT][C] rows as needed, writes qp[CNNQ_NQP][C] and (if not NULL)
 * diag[CNNQ_NDIAG][C]. */
typedef struct cnnq_params_cfg {
    int32_t num_bits;
    int32_t positive;
    int32_t clip;
    float pstd;
    int32_t bit_alloc;
    int32_t prior_is_b;
    double target;
    int32_t round_mode;
    int32_t direct_range; /* per-tensor clipping branch (iq.py:353-357): delta = range itself */
} cnnq_params_cfg;
int cnnq_pc_params(const float* stats, int64_t C, const cnnq_params_cfg* cfg /* host */, float* qp,
                   float* diag, void* stream);

/* Per-channel clipping-error columns for `-c mix` (smpc.py:24-32 declares them, :80-100 are the formulas; iq.py:310-323 is the
 * consumer) of K = 1..3 candidate quantizations, from ONE read of x and without writing a quantized tensor.
 * qp: K parameter tables [K][CNNQ_NQP][C] as cnnq_pc_params writes them; q_k is exactly what cnnq_pc_qdq stores for table k.
 * mm (optional): the channel extrema [2][C] of THIS tensor (rows min, max) - where they put a channel in the domain of the
 * divide-free quotient - and no candidate of the channel has a NaN zero point or qmax - it is used (the same function there:
 * the results do not depend on mm).
 * err [2K][C] fp32: rows mse_0..K-1 - the mean over n of the mean over hw of (x - q_k)^2 (smpc.py:84) - then cos_0..K-1 -
 * sum x q_k / (sqrt(sum_n sqrt(sum_hw x^2)) sqrt(sum_n sqrt(sum_hw q_k^2))), i.e. utils/misc.py:23-34 with dims = [-1, 0]
 * as written (the root is taken inside the loop over the dimensions).  The nan_to_num / 0 -> 1 of smpc.py:113-115 is the
 * caller's.  Sums in fp64, rounded once; no atomics: bit-identical run after run.
 * ws: cnnq_pc_qerr_workspace bytes, 8-byte aligned (fp64 row records).  Two launches, no host synchronisation, no allocation.
 * K outside 1..3, a size < 1 or a null x / qp / ws / err: CNNQ_EINVAL (0 bytes) before anything touches the device. */
size_t cnnq_pc_qerr_workspace(int64_t N, int64_t C, int64_t HW, int K);
int cnnq_pc_qerr(const float* x, int64_t N, int64_t C, int64_t HW, const float* qp, int K, const float* mm /* or NULL */,
                 void* ws, float* err, void* stream);

/* Weights (iq.py:453-476): identical parameter derivation with the range always min/max and
 * the bit allocation prior always STD; provided as cnnq_pc_params with clip = 0. */

/* The core: y = dequant(quant(x)) on native NCHW with per-channel scale / zero point / qmax
 * (iq.py:573-592 - div, add, clamp, round, sub, mul as ONE pass; the four transpose copies of
 * iq.py:427,450,534 disappear).  IEEE division, separate roundings (no FMA), clamp before
 * round, round half to even: integer codes are bit-exact with the reference's.
 * Non-temporal loads and stores (x is read for the last time, y is never re-read by this path);
 * launched as many short workgroups in address order, which is what read+write streaming on
 * MI355X wants; reverse != 0 walks the tensor in descending address order (use it when the
 * previous pass over x went ascending: its tail is still in the 256 MB Infinity Cache).
 * `codes` (optional, may be NULL): the integer codes as one byte per element.
 * `hist` (optional, may be NULL): 256 uint64 bins, ZEROED BY THE CALLER, to which the code
 * histogram of the whole tensor is added (integer atomics -> deterministic); with cnnq_entropy
 * this replaces the full sort of torch.unique in utils/entropy.py:6-17 (iq.py:586-587). */
int cnnq_pc_qdq(const float* x, float* y, int64_t N, int64_t C, int64_t HW, const float* qp,
                uint8_t* codes, uint64_t* hist, int reverse, void* stream);

/* Packed int4 as the STORED activation format (beyond the reference, which only
 * simulates): cnnq_pc_quantize_pack4 writes the integer codes of a <= 4-bit quantization two per
 * byte (even element in the low nibble, N*C*HW/2 bytes) - 4 B read + 0.5 B written per element;
 * cnnq_pc_dequantize_pack4 turns them back into exactly the floats cnnq_pc_qdq would have produced.
 * Requires HW % 4 == 0, 16-byte aligned x / y, qmax <= 15 in every channel of qp. */
int cnnq_pc_quantize_pack4(const float* x, uint8_t* packed, int64_t N, int64_t C, int64_t HW, const float* qp,
                           void* stream);
int cnnq_pc_dequantize_pack4(const uint8_t* packed, float* y, int64_t N, int64_t C, int64_t HW, const float* qp,
                             void* stream);
/* The same with one byte per code (quantizations of up to 8 bits, e.g. the first layer the reference keeps at
 * 8 bit, iqm.py:551-555): 4 + 1 bytes per element; `codes` 4-byte aligned, H*W % 4 == 0. */
int cnnq_pc_quantize_u8(const float* x, uint8_t* codes, int64_t N, int64_t C, int64_t HW, const float* qp,
                        void* stream);
int cnnq_pc_dequantize_u8(const uint8_t* codes, float* y, int64_t N, int64_t C, int64_t HW, const float* qp,
                          void* stream);

/* Bit allocation as the STORED format (the per-channel qmax = 2**bit_alloc - 1 of iq.py:563-564,
 * 582-584 made real): channel c stores bits[c] in 0..8 bits per code (bits = row CNNQ_DIAG_BITS of cnnq_pc_params'
 * diag), i.e. sum(bits)/8 bytes per spatial position.  Row (n, c) = H*W codes as a little-endian bit stream,
 * padded to 4 bytes, at byte n * rowoff[C] + rowoff[c]; cnnq_pc_packed_layout fills rowoff[C + 1] (uint32, device)
 * from bits; the packed buffer needs N * rowoff[C] bytes.  A 0-bit channel stores nothing.  The round trip
 * reproduces the fused Q/DQ (cnnq_pc_qdq with the same qp) bit for bit. */
int cnnq_pc_packed_layout(const float* bits, int64_t C, int64_t HW, uint32_t* rowoff, void* stream);
int cnnq_pc_quantize_packed(const float* x, uint8_t* packed, int64_t N, int64_t C, int64_t HW, const float* qp,
                            const float* bits, const uint32_t* rowoff, void* stream);
/* The same pass with its kernel form spelled out (tests, measurements): form 0 = the library's choice, 1 = the general
 * kernel (any geometry), 2 = the lean kernel of round 3 (one channel per wave, scalar parameters; CNNQ_ENOTSUP for rows
 * of fewer than 8 elements, or whole-float4 rows (H*W % 4 == 0) of an x that is not 16-byte aligned).  Every form writes
 * the same bytes / the same floats; the load direction's lean form also needs a 4-byte aligned packed buffer.  Form 3: one-shot
 * workgroups in address order of the fp32 tensor, per-lane channel parameters - load direction (round 4; the library's choice
 * when it applies): CNNQ_ENOTSUP unless y is 16-byte aligned, the stream 4-byte aligned and the tensor below 2^32 elements;
 * store direction (round 5, k_pack_flat): CNNQ_ENOTSUP unless H*W % 4 == 0, x is 16-byte and the stream 4-byte aligned. */
int cnnq_pc_quantize_packed_form(const float* x, uint8_t* packed, int64_t N, int64_t C, int64_t HW, const float* qp,
                                 const float* bits, const uint32_t* rowoff, int form, void* stream);
int cnnq_pc_dequantize_packed_form(const uint8_t* packed, float* y, int64_t N, int64_t C, int64_t HW, const float* qp,
                                   const float* bits, const uint32_t* rowoff, int form, void* stream);
int cnnq_pc_dequantize_packed(const uint8_t* packed, float* y, int64_t N, int64_t C, int64_t HW, const float* qp,
                              const float* bits, const uint32_t* rowoff, void* stream);

/* Config 2 (dynamic per-channel min/max, no clipping, uniform bit width: iq.py:409-451 with
 * bit allocation off) as three launches, two of them streaming:
 *   cnnq_pc_minmax         exact per-channel {min, max} partials pmm[G][2][C] (G = cnnq_pc_groups;
 *                          every entry written exactly once: no atomics, no initialisation);
 *   cnnq_pc_minmax_params  reduces the G pairs and derives qp[CNNQ_NQP][C] (iq.py:559-572);
 *   cnnq_pc_qdq            the fused Q/DQ (reverse = 1: descending addresses).
 *   cnnq_pc_minmax_qdq     all three in one call; pmm and qp are caller workspaces (qp is also the
 *                          parameter table used, for inspection).
 *   cnnq_pc_minmax_reduce  pmm[G][2][C] -> out[2][C]: a rank's local extrema.  Multi-GPU config 2:
 *                          minmax -> reduce -> all_gather of out over the ranks -> minmax_params with
 *                          the gathered [W][2][C] as pmm and G = W -> qdq (exact, so any world size
 *                          gives the bit-identical result of one GPU holding the whole batch). */
int cnnq_pc_minmax(const float* x, int64_t N, int64_t C, int64_t HW, float* pmm, void* stream);
/* Channel-slice views of a wider NCHW tensor (x[:, c0:c1]: pass x + c0*HW, C = c1 - c0 and the parent's
 * sample stride C_total*HW; 0 = contiguous): the same kernels, the plane size only ever served as that
 * stride.  For a (pointer, stride) pair `aligned16` of cnnq_pc_groups is (x % 16 == 0 && stride % 4 == 0).
 * Used to quantize concatenated outputs in place and to pipeline the multi-GPU exchange (half the
 * channels' statistics travel while the other half is being read). */
int cnnq_pc_minmax_strided(const float* x, int64_t N, int64_t C, int64_t HW, int64_t sample_stride, float* pmm,
                           void* stream);
int cnnq_pc_qdq_strided(const float* x, float* y, int64_t N, int64_t C, int64_t HW, int64_t sample_stride,
                        const float* qp, uint8_t* codes, uint64_t* hist, int reverse, void* stream);
int cnnq_pc_minmax_reduce(const float* pmm, int G, int64_t C, float* out, void* stream);
int cnnq_pc_minmax_params(const float* pmm, int G, int64_t C, int num_bits, int positive, float* qp, void* stream);
int cnnq_pc_minmax_qdq(const float* x, float* y, int64_t N, int64_t C, int64_t HW, int num_bits, int positive,
                       float* pmm, float* qp, uint8_t* codes, uint64_t* hist, void* stream);

/* Config 2 in ONE launch that reads x ONCE (8 instead of 12 bytes per element, one launch boundary instead of
 * three): the same arithmetic as cnnq_pc_minmax_qdq (iq.py:409-451 + 557-603, bit allocation off), the same bits.
 * A workgroup owns whole channels for the whole batch and keeps them in registers between the statistics and the
 * Q/DQ; nothing is exchanged between workgroups and no workspace is needed.
 *   qp   out: qp[CNNQ_NQP][C].   mm: optional out [2][C] = the per-channel min and max.
 * Applies when one channel's batch population fits a workgroup's registers (N*H*W up to ~50 K elements per
 * channel: e.g. 64 x 28x28) with 16-byte aligned x and y and H*W % 4 == 0 (or a straddling layout such as 7x7
 * with C*H*W % 4 == 0); returns CNNQ_ENOTSUP otherwise (nothing enqueued: call cnnq_pc_minmax_qdq).
 * cnnq_pc_resident_describe fills out[8] = {A, threads per workgroup, K loads per lane, channels per workgroup,
 * float4 columns, row lanes, workgroups, 0} or returns CNNQ_ENOTSUP (tests, tools). */
int cnnq_pc_resident_describe(int64_t N, int64_t C, int64_t HW, int32_t out[8]);
int cnnq_pc_minmax_qdq_resident(const float* x, float* y, int64_t N, int64_t C, int64_t HW, int num_bits, int positive,
                                float* qp, float* mm, void* stream);

/* Config 2 in ONE launch and ONE read of x for tensors whose channels span several workgroups (csrc/cnnq_group.hip.h):
 * every workgroup keeps its tile of x in registers; the workgroups that hold pieces of the same channels exchange
 * their {min, max} pairs through `ws` (round 4, the slot meeting: a member's pair is stored once into its zero-at-rest slot
 * and IS its arrival, the members poll the group's slots, the last one to leave zeroes them; flags bit 5: write-through
 * stores and one arrival counter per channel group as in round 2; either way a bounded wait that falls back to recomputing
 * the extrema from x - never a deadlock, never different bits).
 *   x, y must not overlap (both are read / written through __restrict__ pointers, and a workgroup whose bounded wait
 *        expires re-reads x after other workgroups may have stored y); the same holds for every single-launch entry point.
 *   ws   from cnnq_group_ws_alloc(bytes >= cnnq_pc_group_workspace(N, C, HW)): fine-grained (uncached) device
 *        memory, zeroed once (the kernel re-arms it), so that what a workgroup reads never depends on the state of
 *        a per-XCD L2; one workspace must not be used by two launches that can run concurrently.
 *        Word 0 is a status word (cnnq_group_ws_status copies it to the host, synchronising): bit 0 is set when
 *        a wait timed out (results are unaffected; while it is set, later waits give up after 0.5 ms instead of 20 -
 *        cnnq_group_ws_status_clear lowers it).
 *   qp   out: qp[CNNQ_NQP][C].   mm: optional out [2][C] = the per-channel min and max.
 *   flags  bit 0: take the recompute path unconditionally (tests).
 *          bit 1: quantize every channel through the hardware divide (tests).  By default a channel whose extrema are finite, at most 2^70 in
 *          magnitude, with a scale of at most 2^30, takes the correctly rounded quotient from the channel's reciprocal
 *          (two fma corrections, csrc/cnnq_qdq.hip.h qdq1_fast): the same bits, half the arithmetic.
 *          bit 5 (32): the counter meeting of round 2 instead of the slot meeting (tests, A/B).
 *        A slot of the slot meeting must be ZERO AT REST - a stale non-zero word would be folded into a channel's extrema
 *        as if a member had stored it: hand the kernel only workspaces from cnnq_group_ws_alloc (zeroed at their full size),
 *        never one a launch was aborted on (device reset), and never replay a captured graph concurrently with eager
 *        launches on the same workspace; cnnq_group_ws_at_rest checks it.  The slot region sits between the counter lines
 *        and the pair blocks (2 MB, since round 4: re-query cnnq_pc_group_workspace, do not hard-code a size).
 * Same shape / alignment conditions and CNNQ_ENOTSUP convention as cnnq_pc_minmax_qdq_resident.
 * cnnq_pc_group_describe: out[8] = {A, K, mode, S, column blocks, workgroups per group, groups, workgroups}. */
size_t cnnq_pc_group_workspace(int64_t N, int64_t C, int64_t HW);
int cnnq_group_ws_alloc(size_t bytes, void** ws);   /* allocates + zeroes, synchronises the device */
int cnnq_group_ws_free(void* ws);
int cnnq_group_ws_status(const void* ws, uint32_t* status_host);
int cnnq_group_ws_status_clear(void* ws);
/* tests: counts the 32-bit words that are not zero in the regions every launch leaves zero (everything below the pair
 * blocks but the status word and the epoch-versioned corner of the header that cnnq_pt_minmax_qdq_fused writes before it
 * reads: counter lines, the slot meeting's slots); synchronises. */
int cnnq_group_ws_at_rest(const void* ws, uint64_t* nonzero_words_host);
int cnnq_pc_group_describe(int64_t N, int64_t C, int64_t HW, int32_t out[8]);
int cnnq_pc_minmax_qdq_group(const float* x, float* y, int64_t N, int64_t C, int64_t HW, int num_bits, int positive,
                             void* ws, float* qp, float* mm, unsigned flags, void* stream);

/* The two halves of config 2 around the cross-rank exchange (multi-GPU: every rank holds a batch shard), one call
 * each: cnnq_pc_minmax_local = cnnq_pc_minmax + cnnq_pc_minmax_reduce -> local[2][C] (two launches);
 * cnnq_pc_minmax_local_auto does the same in ONE launch when the geometry has a group plan and `gws` (the exchange
 * workspace of cnnq_pc_minmax_qdq_group, gws_bytes >= cnnq_pc_group_workspace(...); may be NULL) is given: the last
 * workgroup of a channel group to arrive folds the group's pairs - nobody waits.  After the all_gather of the W ranks'
 * records, cnnq_pc_gathered_qdq is ONE launch as well: every workgroup of the fused Q/DQ derives scale / zero point
 * of its channels from gathered[W][2][C] (the arithmetic of cnnq_pc_minmax_params: same bits on every rank) and the
 * first batch split writes them to qp[CNNQ_NQP][C] (may be NULL). */
int cnnq_pc_minmax_local(const float* x, int64_t N, int64_t C, int64_t HW, float* pmm, float* local, void* stream);
int cnnq_pc_minmax_local_auto(const float* x, int64_t N, int64_t C, int64_t HW, float* pmm, void* gws, size_t gws_bytes,
                              float* local, void* stream);
int cnnq_pc_gathered_qdq(const float* x, float* y, int64_t N, int64_t C, int64_t HW, const float* gathered, int W,
                         int num_bits, int positive, float* qp, void* stream);

/* Config 2 behind one call.  `ws`: caller workspace of cnnq_pc_minmax_qdq_workspace(N, C, HW) bytes (4-byte aligned;
 * floats qp[CNNQ_NQP][C], mm[2][C], pmm[G][2][C]).  allow_single_launch != 0: the resident single launch when the
 * shape has one, else - when `gws` (a zeroed-once group workspace of gws_bytes >= cnnq_pc_group_workspace(...), see
 * cnnq_pc_minmax_qdq_group) is given - the group-exchange single launch; mm is valid after either.  Otherwise,
 * and for shapes neither supports, the three-launch chain. */
size_t cnnq_pc_minmax_qdq_workspace(int64_t N, int64_t C, int64_t HW);
int cnnq_pc_minmax_qdq_auto(const float* x, float* y, int64_t N, int64_t C, int64_t HW, int num_bits, int positive,
                            float* ws, void* gws, size_t gws_bytes, int allow_single_launch, void* stream);

/* Config 2 in ONE launch with the outputs that otherwise need the three-launch chain (round 3): y, plus optionally
 * `codes` (uint8, one per element, <= 8 bits; 4-byte aligned) and / or the code histogram `hist_rep`
 * (cnnq_hist_replica_bytes() bytes, zeroed ONCE by the caller: cnnq_entropy_replicas folds the replica tables into the
 * Shannon entropy of utils/entropy.py:6-17 - iq.py:586-587 - and leaves them zero) - or, with y == codes == hist_rep ==
 * NULL, `packed`: the 4-bit codes two per byte INSTEAD of y (<= 4 bits; the layout of cnnq_pc_quantize_pack4, decoded by
 * cnnq_pc_dequantize_pack4 with the qp this call writes): 4.5 bytes per element straight from x.
 * gws / gws_bytes: the exchange workspace of cnnq_pc_minmax_qdq_group (may be NULL: whole-channel shapes only).
 * qp[CNNQ_NQP][C] is written; mm[2][C] (may be NULL) receives the extrema.  CNNQ_ENOTSUP: the shape has no
 * single-launch kernel (use cnnq_pc_minmax_qdq and friends). */
size_t cnnq_hist_replica_bytes(void);
int cnnq_pc_minmax_qdq_single(const float* x, float* y, int64_t N, int64_t C, int64_t HW, int num_bits, int positive,
                              void* gws, size_t gws_bytes, float* qp, float* mm, uint8_t* codes, uint64_t* hist_rep,
                              uint8_t* packed, void* stream);
int cnnq_entropy_replicas(uint64_t* hist_rep, float* out, void* stream);
/* Round 6: the entropies of a whole forward's tensors in ONE launch at its end (the reference logs the value, nothing consumes
 * it mid-forward: int_quantizer.py:445,179,217): n sets of replica tables back to back (cnnq_hist_replica_bytes() each, every
 * tensor's launch counting into its own set) -> out[n]; all tables are zero afterwards. */
int cnnq_entropy_replicas_batch(uint64_t* hist_rep, int n, float* out, void* stream);

/* Config 2 in ONE launch and ONE read of x when the batch is sharded over `world` GPUs of one node
 * (csrc/cnnq_xrank.hip.h; opt-in in the Python host - CNNQ_XRANK=1 / auto - and only after it reproduced the collective
 * form's bits at first use; the collective form is cnnq_pc_minmax_local_auto -> all_gather -> cnnq_pc_gathered_qdq, which
 * reads x twice).  The reference has no counterpart (its DataParallel replicas use their own sub-batch's range,
 * inference_sim.py:196-200); this reproduces the single-GPU result of int_quantizer.py:409-451,557-603 on the global batch.
 *   windows  device array [world] of pointers: entry r is rank r's window (cnnq_xrank_alloc on rank r, opened here with
 *            cnnq_xrank_open from its hipIpc handle; the own window at [rank]); every window holds cmax channels: one 8-byte
 *            slot per (parity, source rank, channel), zero when empty - a rank stores the complement of its {min, max}
 *            pair into every window and polls its own (round 4: the pair is the signal; a small kernel behind the launch
 *            zeroes the launch's parity again).
 *   seq      1, 2, 3, ...: the same on every rank for the same launch; the ranks issue the same launches in the same
 *            order, each on ONE stream.  Not capturable into a graph (the number is a kernel argument; see _xrank_dev).
 *   status   device word: bit 2 is raised when a wait for a peer's record expired after timeout_ticks of the 100 MHz
 *            clock (the affected channels' outputs are NaN then) - check it at the next synchronisation point.
 *   ws / gws  as for cnnq_pc_minmax_qdq_auto (ws: cnnq_pc_minmax_qdq_workspace bytes; qp[CNNQ_NQP][C] and mm[2][C] - the
 *            GLOBAL extrema - are left at its start).
 * A rank whose shard has no single-launch kernel (shards may differ by a sample) speaks the same window protocol around
 * two passes over x, so every rank consumes the sequence number whatever its own plan. */
size_t cnnq_xrank_window_bytes(int world, int cmax);
int cnnq_xrank_alloc(int world, int cmax, void** window, unsigned char handle[64]);   /* allocates + zeroes the own window, exports its hipIpc handle; synchronises */
int cnnq_xrank_open(const unsigned char handle[64], void** window);                   /* maps a peer's window */
int cnnq_xrank_close(void* window);                                                   /* unmaps it */
int cnnq_xrank_free(void* window);                                                    /* releases the own window */
int cnnq_pc_minmax_qdq_xrank(const float* x, float* y, int64_t N, int64_t C, int64_t HW, int num_bits, int positive,
                             float* ws, void* gws, size_t gws_bytes, void* const* windows, int rank, int world, int cmax,
                             uint32_t seq, uint32_t* status, int64_t timeout_ticks, void* stream);
/* The same with DEVICE-side sequence numbers and the optional outputs of cnnq_pc_minmax_qdq_single (round 4):
 *   seq_dev   EIGHT device words (zero at start, one block per rank; round 6: words [4..7] hold the slots in use per parity,
 *             kept by the launches themselves): the launch's number is seq_dev[0] + 1 and the small kernel
 *             enqueued behind the launch advances the word - nothing about the call changes from launch to launch, so it
 *             can be captured into a HIP graph and replayed (every rank replays the same graph the same number of times).
 *   codes / hist_rep   as for cnnq_pc_minmax_qdq_single (num_bits <= 8): this rank's codes, and this rank's code counts in
 *             the replica tables - fold them with cnnq_hist_replicas_fold, sum the folded tables over the ranks, then
 *             cnnq_entropy gives the entropy of the global batch's codes (iq.py:586-587).
 * cnnq_hist_replicas_fold adds the replica tables to hist[256] and leaves them zero. */
int cnnq_pc_minmax_qdq_xrank_dev(const float* x, float* y, int64_t N, int64_t C, int64_t HW, int num_bits, int positive,
                                 float* ws, void* gws, size_t gws_bytes, void* const* windows, int rank, int world, int cmax,
                                 uint32_t* seq_dev, uint32_t* status, int64_t timeout_ticks, uint8_t* codes, uint64_t* hist_rep,
                                 void* stream);
/* ONE launch per tensor on the eager path (round 5): host numbering without the kernel behind the launch.
 *   seq       the host's launch number (1, 2, 3, ... the same on every rank, one per launch of the stream); 0: device numbering
 *             exactly as cnnq_pc_minmax_qdq_xrank_dev (seq_dev required), plus the clean-up of zero_c.
 *   zero_c    only without seq_dev: the channel count C of the launch TWO BACK on this stream (0 for the first two launches):
 *             workgroup 0 zeroes the slots that launch used - no reader of this rank is left and no peer can be pushing there yet
 *             (csrc/cnnq_xrank.hip.h).  With seq_dev (eight words) the launches keep these counts on the device and zero_c is
 *             ignored (round 6, ADVICE r5: captured, replayed and eager launches in any order leave the same trail).
 *   seq_dev   (may be NULL with seq != 0) device word that follows the host's count, so that a later captured launch with device
 *             numbering on the same word continues it.  A stream that switches to device numbering (its first captured launch)
 *             stays there, and passes the channel counts of its last two host-numbered launches as zero_c of its first two
 *             device-numbered ones.
 * The windows hold four parities (cnnq_xrank_window_bytes accounts for them). */
int cnnq_pc_minmax_qdq_xrank_seq(const float* x, float* y, int64_t N, int64_t C, int64_t HW, int num_bits, int positive,
                                 float* ws, void* gws, size_t gws_bytes, void* const* windows, int rank, int world, int cmax,
                                 uint32_t seq, uint32_t* seq_dev, int zero_c, uint32_t* status, int64_t timeout_ticks, uint8_t* codes,
                                 uint64_t* hist_rep, void* stream);
int cnnq_hist_replicas_fold(uint64_t* hist_rep, uint64_t* hist, void* stream);

/* The dynamic ACIQ configurations (config 3: iq.py:327-352 + 409-451, statistics of this very tensor) behind
 * one call: pass A -> merge -> pass B when `b` is needed (laplace clipping, or bit allocation with the laplace
 * prior) -> merge -> cnnq_pc_params(cfg) -> fused Q/DQ.  `ws`: caller workspace of cnnq_pc_aciq_workspace(...)
 * bytes, 8-byte aligned (0 = invalid geometry); qp[CNNQ_NQP][C] and diag[CNNQ_NDIAG][C] (diag required with
 * bit allocation) are outputs.  Single process only: the cross-rank exchange sits between the launches. */
size_t cnnq_pc_aciq_workspace(int64_t N, int64_t C, int64_t HW, int aligned16);
int cnnq_pc_aciq_qdq(const float* x, float* y, int64_t N, int64_t C, int64_t HW, const cnnq_params_cfg* cfg, void* ws,
                     float* qp, float* diag, void* stream);

/* The same pipeline with pass B, the parameter derivation and the Q/DQ in ONE launch that reads x once (round 5; 12
 * instead of 16 bytes per element, four launches: pass A, merge, bit allocation, the single launch): the register-resident
 * tiles and the in-launch slot meeting of cnnq_pc_minmax_qdq_group, exchanging per-channel partial sums of |x - mean|
 * (added in member order by every member: the same b, bit for bit, in all of them and run after run).  For Laplace
 * clipping on the per-channel route (cfg->clip == 1, !direct_range), bit allocation on the 'gaus' prior only.  Returns
 * CNNQ_ENOTSUP - nothing enqueued - for other configurations, shapes without a single-launch plan, or a group workspace
 * `gws` (cnnq_group_ws_alloc, >= cnnq_pc_group_workspace bytes) that is NULL or too small.
 * ws: >= cnnq_pc_aciq_workspace bytes; stats[CNNQ_NSTAT][C] out (every row written; KURT / STD_POS zero); qp, diag as
 * cnnq_pc_params (diag required with bit allocation); codes / hist_rep (optional) as cnnq_pc_minmax_qdq_single;
 * flags: 0 (tests: 1 = skip the wait and recompute, 2 = IEEE divide for every channel). */
int cnnq_pc_aciq_qdq_single(const float* x, float* y, int64_t N, int64_t C, int64_t HW, const cnnq_params_cfg* cfg, void* ws,
                            void* gws, size_t gws_bytes, float* stats, float* qp, float* diag, uint8_t* codes,
                            uint64_t* hist_rep, unsigned flags, void* stream);
/* cnnq_pc_aciq_qdq_single when it applies, else cnnq_pc_aciq_qdq: one call, same ws. */
int cnnq_pc_aciq_qdq_auto(const float* x, float* y, int64_t N, int64_t C, int64_t HW, const cnnq_params_cfg* cfg, void* ws,
                          void* gws, size_t gws_bytes, float* qp, float* diag, void* stream);

/* Round 6 - configs 3 / 5 / 4 of a BATCH SHARD with the cross-rank exchange inside the launches (csrc/cnnq_xrank.hip.h,
 * csrc/cnnq_aciq.hip.h, csrc/cnnq_stats1.hip.h): the sharded forms of cnnq_pc_aciq_qdq_single, cnnq_pc_midtread_qdq_single and
 * cnnq_pc_stats_single - one host call per tensor, the launches of one GPU, NO collective.  The reference has no counterpart (its
 * DataParallel replicas quantize with their own sub-batch's statistics, inference_sim.py:196-200); these reproduce
 * int_quantizer.py:327-359 / 185-225 and statistic_manager_perchannel.py:45-79 on the GLOBAL batch from each rank's shard.
 *   cnnq_xrank_ctx   the exchange of config 2 (same windows, same launch numbering, same status word - the launches of all
 *                    four entry points share ONE sequence per stream):
 *       windows / rank / world / cmax   as cnnq_pc_minmax_qdq_xrank; these launches use eight slots per channel: 8 C <= cmax
 *       seq       the host's launch number (1, 2, 3, ...); 0: device numbering (captured launches), see _xrank_dev
 *       seq_dev   EIGHT device words, zeroed once (one block per rank and stream): [0] the launch number, [4..7] the slots in
 *                 use per parity - the launches record and clean them themselves (no host bookkeeping; also used by
 *                 cnnq_pc_minmax_qdq_xrank_seq / _dev since round 6, which therefore need the eight words too)
 *       status / timeout_ticks   as cnnq_pc_minmax_qdq_xrank: bit 2 when a wait for a peer expired (outputs NaN)
 * What travels (slot = word * C + channel): word 0 the {min, max} pair, 1 sum, 2 sum of squares, 3 / 4 the sums of relu(x), 5
 * the rank's element count, 6 sum |x - mean|, 7 sum ((x - mean) / std)^4 - sums as the complement of their fp64 bits, and every
 * reader adds the W ranks' words in RANK order: all ranks derive the same mean / std / b, hence the same parameters, bit for
 * bit.  A shard without a single-launch plan runs the chain's passes around the same slots, so the ranks need not agree on their
 * plans; every call consumes exactly one launch number. */
typedef struct cnnq_xrank_ctx {
    void* const* windows;
    int32_t rank, world, cmax;
    uint32_t seq;
    uint32_t* seq_dev;
    uint32_t* status;
    int64_t timeout_ticks;
} cnnq_xrank_ctx;
/* Config 3: k_moments -> k_xr_moments -> (k_bitalloc) -> k_fused_* <XR>: x read twice (12 bytes per element).  ws:
 * cnnq_pc_aciq_workspace bytes; stats [CNNQ_NSTAT][C], mom [CNNQ_NMOM][C] (fp64), qp, diag (as cnnq_pc_params): outputs, the
 * global batch's, the same on every rank.  Laplace clipping, bit allocation on the 'gaus' prior, num_bits <= 8 (else
 * CNNQ_ENOTSUP: nothing enqueued, no number consumed).  flags as cnnq_pc_aciq_qdq_single. */
int cnnq_pc_aciq_fused_xrank(const float* x, float* y, int64_t N, int64_t C, int64_t HW, const cnnq_params_cfg* cfg, void* ws, void* gws,
                             size_t gws_bytes, float* stats, double* mom, float* qp, float* diag, const cnnq_xrank_ctx* xc, unsigned flags,
                             void* stream);
/* Config 5 (mid-tread with clipping); mt [CNNQ_NMT][C] out; hist (optional, CNNQ_MT_HIST_WORDS(C), zeroed here) counts THIS
 * rank's codes: sum the ranks' tables, then cnnq_midtread_entropy_count with mom's COUNT row. */
int cnnq_pc_midtread_fused_xrank(const float* x, float* y, int64_t N, int64_t C, int64_t HW, double target, int sym, const double* tables,
                                 int ntab, void* ws, void* gws, size_t gws_bytes, float* stats, double* mom, float* mt, uint64_t* hist,
                                 const cnnq_xrank_ctx* xc, unsigned flags, void* stream);
/* Config 4: the seven statistics and the merged moment record of the GLOBAL batch on every rank, from ONE read of the shard
 * where it has a flat-tile plan (k_stats_flat<XR>), else k_moments -> k_xr_moments -> k_absdev -> k_xr_devsums.  ws:
 * cnnq_pc_stats_workspace bytes; flags as cnnq_pc_stats_single (bit 0: recompute path, bit 3: also channels of more than 128
 * tiles). */
int cnnq_pc_stats_xrank(const float* x, int64_t N, int64_t C, int64_t HW, int need_b, int need_kurt, int need_relu, void* ws, void* gws,
                        size_t gws_bytes, double* mom, float* stats, const cnnq_xrank_ctx* xc, unsigned flags, void* stream);

/* Weight bias / variance correction after quantization (iqm.py:374-391), in place on
 * wq[C][HW]: vcorr: wq = (wq - mean_q) * std_w/(std_q + 1e-8) + mean_q; bcorr: wq = wq - mean_q + mean_w
 * (mean_q is the pre-correction mean in both), with the reference's operation order.  stats_w /
 * stats_q are the stats tables (rows MEAN, STD) of the original and the quantized weights. */
int cnnq_pc_weight_correct(float* wq, int64_t C, int64_t HW, const float* stats_w, const float* stats_q, int vcorr,
                           int bcorr, void* stream);

/* Activation bias correction (iqm.py:180-196; -sm use with -bca):
 *   cnnq_pc_bcorr_sums   per channel sum(x'), sum(y), count(x' > 0), x' = relu(x) when relu_first,
 *                        -> part3[G][3][C] fp64 (G = cnnq_pc_groups);
 *   cnnq_pc_bcorr_bias   merges G records (or W ranks' sums) -> sums[3][C] (optional, for the
 *                        cross-rank exchange) and bias[c] = (sum x' - sum y)/(count + 1e-8);
 *   cnnq_pc_bcorr_apply  y += (y > 0) * bias[c], in place.
 * Fused form for per-channel quantizers with a parameter table qp (12 instead of 24 bytes per element,
 * the same floats): the quantized value is recomputed from x instead of stored and re-read -
 *   cnnq_pc_qdq_bcorr_sums  the sums of cnnq_pc_bcorr_sums with y = Q/DQ(x; qp) computed on the fly;
 *   cnnq_pc_qdq_bcorr       y = q + (q > 0) * bias[c], q = Q/DQ(x; qp) (iq.py:573-592 then iqm.py:196). */
int cnnq_pc_bcorr_sums(const float* x, const float* y, int64_t N, int64_t C, int64_t HW, int relu_first,
                       double* part3, void* stream);
int cnnq_pc_qdq_bcorr_sums(const float* x, int64_t N, int64_t C, int64_t HW, const float* qp, int relu_first,
                           double* part3, void* stream);
int cnnq_pc_qdq_bcorr(const float* x, float* y, int64_t N, int64_t C, int64_t HW, const float* qp, const float* bias,
                      int reverse, void* stream);
int cnnq_pc_bcorr_bias(const double* part3, int G, int64_t C, double* sums, float* bias, void* stream);
int cnnq_pc_bcorr_apply(float* y, int64_t N, int64_t C, int64_t HW, const float* bias, void* stream);

/* Mid-tread quantization with per-channel BIN allocation (config 5, -mtq; iq.py:128-225):
 *   cnnq_pc_midtread_params  stats -> mt[CNNQ_NMT][C]: omega = round(C*2^target*std^(2/3)/sum) (eq. 10),
 *       clip != 0: alpha multiplier by linear interpolation in the 101-entry (omega, alpha) tables
 *       (`tables` = device fp64 [2][ntab], omega row then alpha row; iq.py:41-51,137-145),
 *       range = 2*alpha*b (sym) or max(mean,0)+alpha*b, Delta = range/omega, clamp bounds around the
 *       quantized mean; clip == 0 (weights): range = max-min (sym) or max.  One workgroup.
 *       Where the reference raises IndexError the library chooses: omega beyond the last knot
 *       extrapolates along the last segment; a NaN omega - one NaN / negative std, or every channel constant
 *       (sum == 0) - gives a NaN multiplier and NaN bounds with Delta = FLT_MAX in EVERY channel; below the first
 *       knot the segment wraps to the last entry, as numpy's index -1 does.  clip == 0: rows ALPHA 0, CMIN / CMAX
 *       -inf / +inf.  Row WSTART: floor of the smallest c_min (each clamped to +-1e9, NaN as -1e9), not below
 *       -CNNQ_MT_HIST_BINS / 2; -CNNQ_MT_HIST_WINDOW / 2 without clipping.  Refuses ntab < 2, null pointers,
 *       C <= 0 and C >= 2^31 with CNNQ_EINVAL and writes nothing.
 *   cnnq_pc_midtread_qdq     y = clamp(round(x/Delta[c]), c_min[c], c_max[c]) * Delta[c] in one pass;
 *       `codes` (optional) fp32 codes; `hist` (optional, zeroed by the caller,
 *       CNNQ_MT_HIST_WORDS(C) uint64 words) the code histogram.  A NaN code (a NaN in x) is counted in
 *       its channel's c_min counter, where torch.unique would keep every NaN apart: nothing in the
 *       reference depends on either, and no test feeds one.
 *   cnnq_midtread_entropy    Shannon entropy of that histogram (equal clamp values merged). */
int cnnq_pc_midtread_params(const float* stats, int64_t C, double target, int clip, int sym, const double* tables,
                            int ntab, float* mt, void* stream);
int cnnq_pc_midtread_qdq(const float* x, float* y, int64_t N, int64_t C, int64_t HW, const float* mt, int clip,
                         float* codes, uint64_t* hist, void* stream);
/* Config 5 (clip = 1) with pass B, the parameter derivation and the quantization in ONE launch that reads x once (round 5;
 * csrc/cnnq_aciq.hip.h MODE 1): pass A, merge, omega / clipping multiplier from the std alone, the single launch - 12 instead of
 * 16 bytes per element.  Channels too populous for the plain register tiles ([512,64,224,224]: 103 MB per channel) take eight
 * more tile rows in LDS and have the chip to themselves, one channel at a time.  mt: out, every row; row WSTART is the exact
 * first code of the histogram window for the non-negative range and an estimate (b = std / sqrt 2) for the symmetric one - the
 * histogram is correct either way (codes outside the window are counted in the global bins and the flag word says so).
 * stats [CNNQ_NSTAT][C] out; ws >= cnnq_pc_aciq_workspace bytes; gws / flags as cnnq_pc_aciq_qdq_single; hist: optional,
 * CNNQ_MT_HIST_WORDS(C) words, zeroed HERE (cnnq_midtread_entropy consumes it).  CNNQ_ENOTSUP: no single-launch plan. */
int cnnq_pc_midtread_qdq_single(const float* x, float* y, int64_t N, int64_t C, int64_t HW, double target, int sym,
                                const double* tables, int ntab, void* ws, void* gws, size_t gws_bytes, float* stats, float* mt,
                                uint64_t* hist, unsigned flags, void* stream);
int cnnq_midtread_entropy(const uint64_t* hist, const float* mt, int64_t C, int64_t total, float* out, void* stream);
/* ... with the element count in device memory: count[0] = elements per channel of the tensor the codes were counted over (row
 * CNNQ_MOM_COUNT of the merged moment record; total = count[0] * C).  For batch-sharded runs, whose shards may differ by a
 * sample: the global batch's size is known exactly on the device. */
int cnnq_midtread_entropy_count(const uint64_t* hist, const float* mt, int64_t C, const double* count, float* out, void* stream);
/* ... and of n <= 16 tensors in one launch (host arrays of n entries each: the histograms, their mt tables, channel counts and
 * element totals) -> out[n]. */
int cnnq_midtread_entropy_batch(int n, const uint64_t* const* hist, const float* const* mt, const int64_t* C, const int64_t* total,
                                float* out, void* stream);

/* Shannon entropy in bits, -sum p*log2(p) over the non-empty bins -> out[0] (utils/entropy.py:12-15). */
int cnnq_entropy(const uint64_t* hist, int nbins, float* out, void* stream);

/* Per-tensor path, replaces kernels/gemmlowp.cu:8-45 (`float2gemmlowp`).
 * cnnq_pt_setup derives {scale, shift, qmax, ...} on the device into ptp[8]:
 *   - from host scalars (range_offset_host != NULL: {range, offset}), or
 *   - from per-row statistics (rows MIN/MAX of a stats table with row stride `stats_stride`,
 *     `rows` entries each): rows_mode 0 = their mean over rows, the per-sample-then-batch-mean
 *     of iq.py:372,515-526; rows_mode 1 = min of mins / max of maxes, the whole-tensor
 *     min/max of iq.py:515-517; zero_min (iq.py:376-377) is applied afterwards;
 *   preserve_zero follows iq.py:613 when enforce_true_zero != 0.
 * cnnq_pt_qdq then streams x -> y with roundf / fminf / fmaxf semantics (gemmlowp.cu:11-24);
 * range <= 0 copies x to y (the reference returns its input there, gemmlowp.cu:31-32).
 * `noise` may be NULL (stochastic rounding is hard-wired off, iq.py:60). */
int cnnq_pt_setup(const float* range_offset_host, const float* stats, int64_t stats_stride, int rows,
                  int rows_mode, int zero_min, int num_bits, int int_exp, int enforce_true_zero, float* ptp,
                  void* stream);
int cnnq_pt_qdq(const float* x, float* y, int64_t n, const float* ptp, const float* noise, void* stream);
/* Config 1 in ONE launch (round 3): dynamic min / max of x viewed as [rows][n / rows] (rows_mode 0: batch mean of the
 * per-row extrema, iq.py:515-526; 1: the tensor's extrema) -> range / offset -> the GEMMLOWP kernel above, the same
 * bits as cnnq_pc_minmax + cnnq_pc_minmax_reduce + cnnq_pt_setup + cnnq_pt_qdq.  gws: an exchange workspace of
 * cnnq_group_ws_alloc of gws_bytes bytes.  ptp_out[8] (may be NULL) receives the parameters.  CNNQ_ENOTSUP: rows that
 * are not whole float4s, more than 1024 rows, unaligned pointers, a tensor of more 16 KB tiles than the workspace
 * holds 16-byte records for (use the four calls). */
int cnnq_pt_minmax_qdq_fused(const float* x, float* y, int64_t n, int rows, int rows_mode, int zero_min, int num_bits,
                             int int_exp, int enforce_true_zero, void* gws, size_t gws_bytes, float* ptp_out, void* stream);

/* KLD calibration (`-kld` with `-sm collect`): replaces the host loops of
 * inference/kld_threshold.py:6-84 (`get_kld_threshold_15bins`, one call per sample at
 * statistic_manager.py:80-82).  x is [rows][len] contiguous (rows = samples of the batch),
 * rowmm[2][rows] the per-row {min, max} (cnnq_pc_minmax + cnnq_pc_minmax_reduce with N = 1, C = rows).
 *   cnnq_kld_hist    hist[rows][CNNQ_KLD_BINS] (uint32; zeroed here): numpy.histogram(arr, 2001,
 *                    range = (-th, th)), th = max(|min|, |max|), float64 edges (kld_threshold.py:19-23);
 *                    NaN elements are not counted; len < 2^31.
 *   cnnq_kld_search  div[rows][CNNQ_KLD_NCAND] = KL(P || Q) for the 994 symmetric clipping candidates
 *                    (kld_threshold.py:31-77, 15 quantized bins), then per row
 *                    out[rows][3] = {optimal threshold (the upper histogram edge of the kept range),
 *                    its divergence, candidate index}: numpy.argmin semantics (kld_threshold.py:79-81).
 *                    The `kld_th` statistic is the maximum of out[:,0] over the batch.
 * A row whose min or max is NaN or +-inf has no range (numpy.histogram raises): its hist row stays all zero and its
 * out is {NaN, NaN, 0}, whatever hist holds; the other rows are not affected. */
#define CNNQ_KLD_BINS 2001
#define CNNQ_KLD_QBINS 15
#define CNNQ_KLD_NCAND 994
int cnnq_kld_hist(const float* x, int64_t rows, int64_t len, const float* rowmm, uint32_t* hist, void* stream);
int cnnq_kld_search(const uint32_t* hist, int64_t rows, const float* rowmm, double* div, double* out, void* stream);

/* Activations of another element type: x and y are `const void*` / `void*` of the type `dtype` names, every table
 * (qp, mm, pmm, ptp, the row extrema, noise) stays fp32 and codes stay uint8.  For BF16 / F16 the result is, bit for
 * bit, the fp32 entry point's on the exactly upconverted input, rounded to nearest-even into the input type (a NaN
 * stays a NaN; an fp16 value above 65504 becomes inf): y == fp32_path(x.float()).to(x.dtype).  CNNQ_DTYPE_F32 calls
 * the fp32 entry point named with the same arguments.  A `dtype` outside the enum returns CNNQ_EINVAL before anything
 * touches the device; CNNQ_ENOTSUP: nothing was enqueued. */
enum { CNNQ_DTYPE_F32 = 0, CNNQ_DTYPE_BF16 = 1, CNNQ_DTYPE_F16 = 2, CNNQ_NDTYPE = 3 };

/* cnnq_kld_hist on rows of another element type (`-kld` with `-sm collect --dtype bfloat16 / float16`; kld_threshold.py:19-23
 * on the activation as the model produced it): x is [rows][len] of `dtype`, rows back to back, 2-byte aligned; the arguments,
 * the zeroing of hist and the status codes are cnnq_kld_hist's (CNNQ_EINVAL: a NULL pointer, rows <= 0, len <= 0; CNNQ_ERANGE:
 * rows > 65535, len >= 2^31), plus CNNQ_EINVAL for a dtype outside the enum.  BF16 / F16: hist is, count for count,
 * cnnq_kld_hist's on the exactly upconverted rows, so cnnq_kld_search behind it gives that route's bits; the rows are read once,
 * 2 B/elem, in 16-byte loads whatever their alignment (single elements up to the first boundary and behind the last). */
int cnnq_kld_hist_dt(const void* x, int dtype, int64_t rows, int64_t len, const float* rowmm, uint32_t* hist, void* stream);

/* Config 2 behind one call (iq.py:409-451,557-603; counterpart of cnnq_pc_minmax_qdq_auto, same `ws` of
 * cnnq_pc_minmax_qdq_workspace(N, C, HW) bytes; qp[CNNQ_NQP][C] and mm[2][C] are written).  BF16 / F16, two routes:
 *   - allow_single_launch != 0 and a channel's N*HW elements fit one workgroup's registers (131072) and the rows
 *     load at least 4 bytes at a time (H*W even, pointers 4-byte aligned): ONE launch that reads x once, one workgroup per channel (k_h_whole);
 *   - otherwise two launches - exact per-channel min / max partials into ws's pmm, then the Q/DQ, whose workgroups derive
 *     their channel's parameters from the partials (cnnq_pc_minmax_params' arithmetic).
 * gws / gws_bytes are not used: channels that span several workgroups take the two launches.
 * cnnq_pc_route_dt (host only, nothing enqueued) names the route: out = {1 single launch / 2 two launches, elements per
 * load W, loads per lane (0 for two launches), workgroups}; align_bytes: the power of two that divides both x and y (<= 16). */
int cnnq_pc_route_dt(int64_t N, int64_t C, int64_t HW, int align_bytes, int allow_single_launch, int32_t out[4]);
int cnnq_pc_minmax_qdq_auto_dt(const void* x, void* y, int dtype, int64_t N, int64_t C, int64_t HW, int num_bits,
                               int positive, float* ws, void* gws, size_t gws_bytes, int allow_single_launch, void* stream);
/* The table-driven Q/DQ (iq.py:573-592, counterpart of cnnq_pc_qdq).  BF16 / F16: codes and hist must be NULL
 * (CNNQ_ENOTSUP otherwise); `reverse` is ignored. */
int cnnq_pc_qdq_dt(const void* x, void* y, int dtype, int64_t N, int64_t C, int64_t HW, const float* qp, uint8_t* codes,
                   uint64_t* hist, int reverse, void* stream);
/* Per-channel extrema of x[N][C][HW] -> local[2][C] (counterpart of cnnq_pc_minmax_local; with N = 1, C = rows the
 * per-sample statistics of config 1, iq.py:510-517).  pmm: workspace of
 * max(cnnq_pc_groups(N, C, HW, 1), cnnq_pc_groups(N, C, HW, 0)) * 2 * C floats. */
int cnnq_pc_minmax_local_dt(const void* x, int dtype, int64_t N, int64_t C, int64_t HW, float* pmm, float* local,
                            void* stream);
/* Config 1's GEMMLOWP Q/DQ (kernels/gemmlowp.cu:8-45, counterpart of cnnq_pt_qdq); ptp from cnnq_pt_setup; noise fp32. */
int cnnq_pt_qdq_dt(const void* x, void* y, int dtype, int64_t n, const float* ptp, const float* noise, void* stream);

/* Dense channels_last (NHWC) activations: x and y are the matrix [R = N*H*W][C] with C innermost, `const void*` / `void*`
 * of cnnq_dtype; qp, mm and ws stay fp32.  y has x's layout and equals, bit for bit, the NCHW entry point's result on the
 * same values in NCHW order (min / max do not depend on the order; the Q/DQ is element by element, with the NCHW path's
 * arithmetic).  A bad dtype, R < 1 or C < 1 returns CNNQ_EINVAL before anything touches the device.  Rows load the widest
 * of 16 / 8 / 4 / 2 / 1 bytes that divides C and the alignment of both pointers, so every C and every element offset has a
 * route.  x != y (both are read / written in several launches).
 * cnnq_pc_nhwc_workspace: bytes of `ws` for cnnq_pc_minmax_qdq_nhwc (0 on bad arguments).
 * cnnq_pc_route_nhwc (host only, nothing enqueued): out = {elements per load W, row slabs S of the statistics launch,
 * workgroups of the Q/DQ launch, row loads per lane of the statistics launch}; align_bytes: the power of two that
 * divides both x and y (<= 16 is what matters). */
size_t cnnq_pc_nhwc_workspace(int64_t R, int64_t C, int dtype);
int cnnq_pc_route_nhwc(int64_t R, int64_t C, int dtype, int align_bytes, int32_t out[4]);
/* Config 2 (int_quantizer.py:409-451, 557-603; counterpart of cnnq_pc_minmax_qdq_auto): exact per-channel {min, max}
 * partials over slabs of rows into ws, cnnq_pc_minmax_params -> qp[CNNQ_NQP][C], cnnq_pc_minmax_reduce -> mm[2][C] (the
 * channel extrema; NULL: kept in ws), then the Q/DQ (divide-free inside the fast domain, the IEEE divide elsewhere: the
 * same bits).  Four launches, no host synchronisation. */
int cnnq_pc_minmax_qdq_nhwc(const void* x, void* y, int dtype, int64_t R, int64_t C, int num_bits, int positive,
                            float* ws, float* qp, float* mm, void* stream);
/* The table-driven Q/DQ (int_quantizer.py:573-592, -sm use; counterpart of cnnq_pc_qdq): the IEEE divide, one launch. */
int cnnq_pc_qdq_nhwc(const void* x, void* y, int dtype, int64_t R, int64_t C, const float* qp, void* stream);

/* Config 3 - ACIQ clipping with bit allocation - on dense channels_last activations.  The per-channel sums are added in an
 * order fixed by (R, C, dtype, alignment) alone: run after run the same bits, but not the NCHW chain's order, so the result
 * is NOT promised to equal cnnq_pc_aciq_qdq's on the same values.  Promised: the table `stats` is within the statistics tier
 * of fp64 (rows MIN / MAX exact, a NaN element makes them NaN), and given that table qp, diag and y are, bit for bit,
 * cnnq_pc_params' and the table-driven Q/DQ's (cnnq_pc_qdq_nhwc: the IEEE divide) - for bf16 / fp16 on the exactly
 * upconverted values with one round-to-nearest-even at the end.
 * cnnq_pc_aciq_nhwc_workspace: bytes of `ws` for cnnq_pc_aciq_qdq_nhwc - the pass-A and pass-B records of the widest slab
 * count over the piece widths and the merged moment record (0 on bad arguments).
 * cnnq_pc_route_aciq_nhwc (host only, nothing enqueued; cnnq_pc_route_nhwc is unchanged): out = {elements per load W, row
 * slabs S of the statistics launches, rows per slab, row loads per lane and slab, workgroups of the Q/DQ launch, 1 - the native
 * launches (0 would say: this class of layer goes back to the copy route; none does)}. */
size_t cnnq_pc_aciq_nhwc_workspace(int64_t R, int64_t C, int dtype);
int cnnq_pc_route_aciq_nhwc(int64_t R, int64_t C, int dtype, int align_bytes, int32_t out[6]);
/* The dynamic ACIQ pipeline (int_quantizer.py:327-352: per-channel min / max / mean / std / b, alpha from the Laplace or
 * Gaussian tables, bit allocation 227-253, delta / offset 284-300; then 409-451, 557-603: scale, zero point, Q/DQ) behind
 * ONE call on [R][C]; counterpart of cnnq_pc_aciq_qdq: pass A -> merge -> (pass B -> merge, when b is needed: Laplace
 * clipping, or bit allocation on the b prior) -> parameters -> Q/DQ, four or six launches.  stats[CNNQ_NSTAT][C] is an
 * OUTPUT and is written completely (KURT, STD_POS zero; B zero without pass B); qp[CNNQ_NQP][C]; diag[CNNQ_NDIAG][C] may
 * be NULL without bit allocation.  ws: cnnq_pc_aciq_nhwc_workspace bytes, 8-byte aligned.  cfg->direct_range (the
 * per-tensor branch) is CNNQ_EINVAL, as are the cases cnnq_pc_aciq_qdq refuses - before anything touches the device.
 * Re-entrant, allocates nothing, no host synchronisation; x != y. */
int cnnq_pc_aciq_qdq_nhwc(const void* x, void* y, int dtype, int64_t R, int64_t C, const cnnq_params_cfg* cfg, void* ws,
                          float* stats, float* qp, float* diag, void* stream);

/* `-sm collect` - the per-channel calibration table of statistic_manager_perchannel.py:45-125 (the permuted copy of 49-50 and
 * the nine full-tensor reductions of 51-79) - on dense channels_last activations, on the storage as it lies: no layout copy and
 * no upcast, x is read once per pass (8 B/elem in fp32, 4 in bf16 / fp16 for the full table).  As for config 3 the per-channel
 * sums are added in an order fixed by (R, C, dtype, alignment) alone: run after run the same bits, no atomics, but not the NCHW
 * chain's order.  Promised: rows MIN / MAX exact (a NaN element makes them NaN), every other row within the statistics tier of
 * fp64 that cnnq_pc_stats_single keeps; rows MIN, MAX, MEAN, STD (and B) do not depend on which of the other rows were asked for
 * and equal, bit for bit, the table cnnq_pc_aciq_qdq_nhwc writes for the same tensor.
 * cnnq_pc_stats_nhwc_workspace: bytes of `ws` - cnnq_pc_aciq_nhwc_workspace's: the pass-A and pass-B records of the widest slab
 * count over the piece widths and the merged moment record (0 on bad arguments).
 * cnnq_pc_route_stats_nhwc (host only, nothing enqueued): out = {elements per load W, row slabs S of the statistics launches,
 * rows per slab, 1 - the native launches (0 would say: this class of layer goes back to the copy route; none does)};
 * align_bytes: the power of two that divides x (<= 16 is what matters). */
size_t cnnq_pc_stats_nhwc_workspace(int64_t R, int64_t C, int dtype);
int cnnq_pc_route_stats_nhwc(int64_t R, int64_t C, int dtype, int align_bytes, int32_t out[4]);
/* The table behind ONE call on [R][C]; counterpart of cnnq_pc_stats: pass A -> cnnq_pc_combine(has_relu = need_relu) (-> pass B
 * -> cnnq_pc_combine_dev(want_kurt = need_kurt), when need_b or need_kurt), two or four launches.  stats[CNNQ_NSTAT][C] is
 * written completely: STD_POS is zero without need_relu, KURT without need_kurt, B unless pass B ran (need_b or need_kurt, as
 * cnnq_pc_stats).  mom[CNNQ_NMOM][C]: the merged moment record, may be NULL (kept in ws).  ws: cnnq_pc_stats_nhwc_workspace
 * bytes, 8-byte aligned.  A bad dtype, R < 1, C < 1, a NULL x / ws / stats or a misaligned ws / mom returns CNNQ_EINVAL, a
 * slab of 2^31 rows or a grid of 2^31 workgroups CNNQ_ERANGE, before anything touches the device.  Re-entrant, allocates
 * nothing, no host synchronisation, graph-capturable. */
int cnnq_pc_stats_nhwc(const void* x, int dtype, int64_t R, int64_t C, int need_b, int need_kurt, int need_relu, void* ws,
                       double* mom, float* stats, void* stream);

/* `-sm collect -ce` - the per-channel clipping-error columns of smpc.py:80-100 (declared at smpc.py:24-32, consumed by
 * iq.py:310-323), counterpart of cnnq_pc_qerr - on dense channels_last activations x[N][HW][C] of fp32 / bf16 / fp16, on the
 * storage as it lies: ONE read of x, no layout copy, no upcast, no quantized tensor written.  qp, K, mm and err are
 * cnnq_pc_qerr's: K = 1..3 tables [K][CNNQ_NQP][C]; mm (optional) the channel extrema [2][C], on which the result does not
 * depend; err [2K][C] fp32, rows mse_0..K-1 then cos_0..K-1.  The columns are those of the exactly upconverted x: q_k is the
 * fp32 value cnnq_pc_qdq_nhwc computes with table k BEFORE it converts to x's dtype, every term is one fp32 operation, the
 * sums are fp64 row records (per sample and slab of its HW rows, folded by cnnq_pc_qerr's own fold), rounded once; against fp64
 * sums of the same terms within 2e-6.  The order of the additions is fixed by (N, HW, C, dtype, alignment) alone: no atomics,
 * bit-identical run after run - not the NCHW kernel's order.
 * cnnq_pc_qerr_nhwc_workspace: bytes of `ws` = N * nb * (1 + 3K) * C * 8 with nb the slabs per sample of the route's report
 * (they do not depend on the alignment); 0 on sizes it has no plan for.
 * cnnq_pc_route_qerr_nhwc (host only, nothing enqueued): out = {elements per load W (at most 2), slabs per sample nb, rows
 * per slab, 1 - the native launch (0 would say: this class of layer goes back to the copy route; none does)}.
 * ws: 8-byte aligned.  A bad dtype, K outside 1..3, N / HW / C < 1, a NULL x / qp / ws / err or a misaligned ws returns
 * CNNQ_EINVAL, N or HW of 2^31 or a grid of 2^31 workgroups CNNQ_ERANGE, before anything touches the device.  Two launches,
 * no host synchronisation, no allocation, graph-capturable. */
size_t cnnq_pc_qerr_nhwc_workspace(int64_t N, int64_t HW, int64_t C, int K, int dtype);
int cnnq_pc_route_qerr_nhwc(int64_t N, int64_t HW, int64_t C, int dtype, int align_bytes, int32_t out[4]);
int cnnq_pc_qerr_nhwc(const void* x, int dtype, int64_t N, int64_t HW, int64_t C, const float* qp, int K,
                      const float* mm /* or NULL */, void* ws, float* err, void* stream);

/* `-sm collect` - the same table - on CONTIGUOUS bf16 / fp16 activations x[N][C][HW], on the storage as it lies: no fp32 copy, x is
 * read once per pass (4 B/elem for the full table).  A row x[n][c][0 .. HW) is cut into pieces of W elements (the widest of 8 / 4 /
 * 2 / 1 that divides HW and x's alignment: every (HW, alignment) has a route); a 256-lane workgroup owns one channel and one of S
 * ranges of samples, or - short batches - one of `column splits` ranges of the pieces of its rows.  Every element is upconverted
 * exactly; the values of a piece are added in fp32 (pairs, then halves), the pieces in fp64, in an order fixed by (N, C, HW,
 * alignment) alone: run after run the same bits, no atomics, but not the fp32 chain's order.  Promised: rows MIN / MAX exact - the
 * extrema of cnnq_pc_stats on x.float(), a NaN element makes them NaN - every other row within the statistics tier of fp64 that
 * cnnq_pc_stats_single keeps; rows MIN, MAX, MEAN, STD (and B) do not depend on which of the other rows were asked for.
 * CNNQ_DTYPE_F32 forwards to cnnq_pc_stats (its workspace: what that call takes at either alignment).
 * cnnq_pc_stats_dt_workspace: bytes of `ws` - doubles part[G][CNNQ_NMOM][C], mom[CNNQ_NMOM][C], part2[G][CNNQ_NDEV][C] with
 * G = S * column splits, which do not depend on the alignment (0 on bad arguments or a geometry beyond cnnq_pc_groups' limits).
 * cnnq_pc_route_stats_dt (host only, nothing enqueued): out = {piece width W, batch splits S, column splits, 1 - the native
 * launches / 0 - a class of layer that did not measure faster than the upcast route and is left there by callers that have the
 * choice: an odd HW with N * HW >= 16384 (cnnq_pc_stats_dt itself runs every class)}; a function of N, C, HW and the dtype alone;
 * fp32: {0, cnnq_pc_groups' records, 1, 1}; align_bytes: the power of two that divides x (<= 16 is what matters). */
size_t cnnq_pc_stats_dt_workspace(int64_t N, int64_t C, int64_t HW, int dtype);
int cnnq_pc_route_stats_dt(int64_t N, int64_t C, int64_t HW, int dtype, int align_bytes, int32_t out[4]);
/* The table behind ONE call; counterpart of cnnq_pc_stats: pass A -> cnnq_pc_combine(has_relu = need_relu) (-> pass B on the merged
 * table -> cnnq_pc_combine_dev(want_kurt = need_kurt), when need_b or need_kurt), two or four launches.  stats[CNNQ_NSTAT][C] is
 * written completely: STD_POS is zero without need_relu, KURT without need_kurt, B unless pass B ran (need_b or need_kurt, as
 * cnnq_pc_stats).  mom[CNNQ_NMOM][C]: the merged moment record - row COUNT is exactly N * HW - may be NULL (kept in ws).  ws:
 * cnnq_pc_stats_dt_workspace bytes, 8-byte aligned.  A bad dtype, N, C or HW < 1, a NULL x / ws / stats, a misaligned ws / mom or
 * an x not aligned to its element size returns CNNQ_EINVAL, a geometry beyond cnnq_pc_groups' limits that function's code - before
 * anything touches the device.  Re-entrant, allocates nothing, no host synchronisation, graph-capturable. */
int cnnq_pc_stats_dt(const void* x, int dtype, int64_t N, int64_t C, int64_t HW, int need_b, int need_kurt, int need_relu, void* ws,
                     double* mom, float* stats, void* stream);

/* `-sm collect -ce` - the per-channel clipping-error columns of smpc.py:80-100 with the cosine of utils/misc.py:23-34 (declared at
 * smpc.py:24-32, consumed by iq.py:310-323), counterpart of cnnq_pc_qerr - on CONTIGUOUS bf16 / fp16 activations x[N][C][HW], on
 * the storage as it lies: ONE read of x in its own dtype (2 B/elem), no fp32 copy, no quantized tensor written.  qp, K, mm and
 * err are cnnq_pc_qerr's: K = 1..3 tables [K][CNNQ_NQP][C]; mm (optional) the channel extrema [2][C], on which the result does
 * not depend; err [2K][C] fp32, rows mse_0..K-1 then cos_0..K-1.  The columns are those of the exactly upconverted x: q_k is the
 * fp32 value cnnq_pc_qdq_dt computes with table k BEFORE it converts to x's dtype, every term is one fp32 operation, the terms of
 * a piece of W elements (cnnq_pc_stats_dt's pieces) are added in fp32 (pairs, then halves), the pieces in fp64 row records (per
 * sample and column part of its row, folded by cnnq_pc_qerr's own fold), rounded once; against fp64 sums of the same terms
 * within 2e-6.  The order of the additions is fixed by (N, C, HW, alignment) alone: no atomics, bit-identical run after run -
 * not the fp32 kernel's order.  CNNQ_DTYPE_F32 forwards to cnnq_pc_qerr.
 * cnnq_pc_qerr_dt_workspace: bytes of `ws` = N * nb * (1 + 3K) * C * 8 with nb the column parts per row of the route's report
 * (a function of N, C, HW and the dtype, never of the alignment; fp32: cnnq_pc_qerr_workspace); 0 on bad arguments or sizes it
 * has no plan for.
 * cnnq_pc_route_qerr_dt (host only, nothing enqueued): out = {piece width W, column parts per row nb, rows a workgroup takes per
 * step, 1 - the native launch / 0 - a class of layer that did not measure faster than the upcast route beyond the run's spread and
 * is left there by callers that have the choice: HW no multiple of 8 with N * HW >= 16384 and N * C * HW < 2^26 (cnnq_pc_qerr_dt
 * itself runs every class)}; fp32: cnnq_pc_qerr's plan as {elements per load, slices per row, 1, 1}; align_bytes: the power of two
 * that divides x (<= 16 is what matters).
 * ws: 8-byte aligned.  A bad dtype, K outside 1..3, N / C / HW < 1, a NULL x / qp / ws / err, a misaligned ws or an x not aligned
 * to its element size returns CNNQ_EINVAL, a geometry beyond cnnq_pc_groups' limits (N or C * HW of 2^31) CNNQ_ERANGE, before
 * anything touches the device.  Two launches, no host synchronisation, no allocation, graph-capturable. */
size_t cnnq_pc_qerr_dt_workspace(int64_t N, int64_t C, int64_t HW, int K, int dtype);
int cnnq_pc_route_qerr_dt(int64_t N, int64_t C, int64_t HW, int dtype, int align_bytes, int32_t out[4]);
int cnnq_pc_qerr_dt(const void* x, int dtype, int64_t N, int64_t C, int64_t HW, const float* qp, int K,
                    const float* mm /* or NULL */, void* ws, float* err, void* stream);

/* `-sm collect -sba` - the per-sample channel extrema behind smpc.py:72-78, where a channel's max / min is the MEAN over the batch
 * of the samples' own max / min - on activations read where they lie: ONE read of x, no layout copy, no upcast.  Both forms write
 * ext[2][N * C] fp32, sample-major (n * C + c): row CNNQ_STAT_MIN the minima, row CNNQ_STAT_MAX the maxima.  Promised: ext
 * equals, as values, the min / max over HW of the exactly upconverted x; an (n, c) row that holds a NaN gives NaN in BOTH entries;
 * the sign of a zero extremum is not pinned.  No atomics - every entry is stored once by one lane - and extrema do not depend on
 * the order of the elements: bit-identical run after run.  No host synchronisation, no allocation, graph-capturable.
 *
 * CONTIGUOUS bf16 / fp16 x[N][C][HW] (smpc.py:72-78): the N * C rows lie back to back; `seg` lanes (a power of two <= 64, from HW
 * alone) own one row at a time and a 256-lane workgroup takes 256 / seg rows per step: one launch, no workspace, no LDS.  A row is
 * read in 16-byte loads from its first 16-byte boundary on and element by element in front of it and behind the last whole load,
 * so every alignment of x (2 bytes at least) and every HW takes the same route.  CNNQ_DTYPE_F32 is REFUSED with CNNQ_ENOTSUP by
 * both functions (contiguous fp32 keeps cnnq_pc_minmax + cnnq_pc_minmax_reduce with N = 1, C = the rows, which need a workspace
 * this call does not take).
 * cnnq_pc_route_sample_extrema_dt (host only, nothing enqueued): out = {seg, rows per workgroup (whole steps of 256 / seg rows),
 * workgroups, 1 - the native launch / 0 - a class of layer that did not measure faster than the former route (upcast +
 * cnnq_pc_stats on the (n, c) rows) beyond the run's spread and is left there by callers that have the choice: HW no multiple of
 * 8 with N * HW >= 16384 and N * C * HW < 2^25 (cnnq_pc_sample_extrema_dt itself runs every class)}; align_bytes: a power of two,
 * on which the plan does not depend.
 * A bad dtype, N / C / HW < 1, a NULL x / ext, an x not aligned to 2 bytes or an ext not aligned to 4 returns CNNQ_EINVAL, a
 * geometry beyond cnnq_pc_groups' limits (N or C * HW of 2^31) or N * C of 2^31 CNNQ_ERANGE, before anything touches the device. */
int cnnq_pc_route_sample_extrema_dt(int64_t N, int64_t C, int64_t HW, int dtype, int align_bytes, int32_t out[4]);
int cnnq_pc_sample_extrema_dt(const void* x, int dtype, int64_t N, int64_t C, int64_t HW, float* ext, void* stream);
/* Dense CHANNELS_LAST fp32 / bf16 / fp16, storage x[N][HW][C] (smpc.py:72-78): cnnq_pc_qerr_nhwc's tiling - a sample's HW rows are
 * cut into S slabs, the grid is N * S * nb workgroups, a lane keeps one piece of W consecutive channels (the widest of 16 / 8 / 4 /
 * 2 / 1 bytes that divides C and x's alignment) and the lanes of a workgroup meet once through LDS.  S == 1: one launch stores
 * ext, ws is not touched and may be NULL.  S > 1 (small batches of large images): the partial pairs go to ws[N * S][2][C] and a
 * second launch, one thread per (n, c), writes ext.
 * cnnq_pc_sample_extrema_nhwc_workspace (smpc.py:72-78): bytes of `ws` = N * S * 2 * C * 4 with S of the route's report, which
 * does not depend on the alignment; 0 at S == 1 and on arguments the call refuses.
 * cnnq_pc_route_sample_extrema_nhwc (host only, nothing enqueued; smpc.py:72-78): out = {elements per load W, slabs per sample S,
 * column blocks nb, 1 - the native launches / 0 - a class of layer that did not measure faster than the former route (upcast,
 * layout copy, cnnq_pc_stats on the (n, c) rows) beyond the run's spread and is left there by callers that have the choice; none
 * so far}; align_bytes: the power of two that divides x (<= 16 is what matters).
 * A bad dtype, N / HW / C < 1, C > 2^26, a NULL x / ext, a NULL ws at S > 1, a misaligned ws / ext or an x not aligned to its
 * element size returns CNNQ_EINVAL; N, HW or N * C of 2^31 or a grid of 2^31 workgroups CNNQ_ERANGE, before anything touches the
 * device. */
size_t cnnq_pc_sample_extrema_nhwc_workspace(int64_t N, int64_t HW, int64_t C, int dtype);
int cnnq_pc_route_sample_extrema_nhwc(int64_t N, int64_t HW, int64_t C, int dtype, int align_bytes, int32_t out[4]);
int cnnq_pc_sample_extrema_nhwc(const void* x, int dtype, int64_t N, int64_t HW, int64_t C, void* ws /* or NULL at S == 1 */,
                                float* ext, void* stream);

/* Activation bias correction (iqm.py:180-196) fused into the table-driven Q/DQ - `-sm use ... -bca` - on CONTIGUOUS bf16 / fp16
 * activations x[N][C][HW], on the storage as it lies: no fp32 copy, 6 B/elem (x read twice, y written once), or 4 B/elem in one
 * launch where a channel's whole batch population fits one workgroup's registers.  Counterpart of cnnq_pc_qdq_bcorr_sums +
 * cnnq_pc_bcorr_bias + cnnq_pc_qdq_bcorr behind ONE call.  The rows are cut into pieces as for cnnq_pc_stats_dt (W = 8 / 4 / 2 / 1
 * from HW and the alignment x and y share: every (HW, alignment) has a route); a workgroup owns one channel.  Two routes:
 *   2. three launches: per channel sum x', sum q, count(x' > 0) over S batch splits x `column splits` (cnnq_pc_stats_dt's
 *      partition) with q = the fp32 Q/DQ of x from qp[CNNQ_NQP][C] (the IEEE divide) and x' = relu(x) when relu_first != 0, into
 *      ws (read-only pass over x); cnnq_pc_bcorr_bias on those records: bias[c] = ((float)sum x' - (float)sum q) /
 *      ((float)count + 1e-8f) and - sums != NULL - the merged sums[3][C] (doubles); y = q + (q > 0) * bias[c], rounded once into
 *      the element type;
 *   1. one launch, one 1024-lane workgroup per channel that keeps the channel in registers: the same sums, bias and y.  Only
 *      where N * HW <= 131072 and W >= 2.
 * The values of a piece are added in fp32 (pairs, then halves), the pieces in fp64, in an order fixed by (N, C, HW, alignment,
 * route) alone: run after run the same bits, no atomics, but not the fp32 chain's order.  Promised: the sums within the statistics
 * tier of fp64 (the count exact), and given them bias and y bit for bit.  CNNQ_DTYPE_F32 forwards to the three fp32 calls named
 * above (its workspace: their records at either alignment).
 * cnnq_pc_qdq_bcorr_dt_workspace: bytes of `ws` - doubles part3[G][3][C] with G = S * column splits, which do not depend on the
 * alignment or the route (0 on bad arguments or a geometry beyond cnnq_pc_groups' limits).
 * cnnq_pc_route_qdq_bcorr_dt (host only, nothing enqueued): out = {piece width W, batch splits S, column splits, route}; route 1
 * / 2 as above, 0 - a class of layer that did not measure faster than the upcast route and is left there by callers that have
 * the choice (cnnq_pc_qdq_bcorr_dt itself runs every class, on route 2).  allow_single_launch: 0 - never route 1; 1 - route 1
 * for the classes where it measured faster than route 2 (C == 256 with N * HW >= 32768: one full round of workgroups on the
 * device); 2 - route 1 wherever the channel fits (tests, A/B).  A function of its
 * arguments alone; fp32: {0, cnnq_pc_groups' records, 1, 2}; align_bytes: the power of two that divides x and y (<= 16 is what
 * matters). */
size_t cnnq_pc_qdq_bcorr_dt_workspace(int64_t N, int64_t C, int64_t HW, int dtype);
int cnnq_pc_route_qdq_bcorr_dt(int64_t N, int64_t C, int64_t HW, int dtype, int align_bytes, int allow_single_launch, int32_t out[4]);
/* bias[C] is an OUTPUT; sums[3][C] may be NULL.  ws: cnnq_pc_qdq_bcorr_dt_workspace bytes, 8-byte aligned, as sums (route 1 does
 * not touch ws).  A bad dtype, N, C or HW < 1, a NULL x / y / qp / ws / bias, a misaligned ws / sums / qp / bias, an x or y not
 * aligned to its element size, or x == y returns CNNQ_EINVAL, a geometry beyond cnnq_pc_groups' limits that function's code -
 * before anything touches the device.  Re-entrant, allocates nothing, no host synchronisation, graph-capturable. */
int cnnq_pc_qdq_bcorr_dt(const void* x, void* y, int dtype, int64_t N, int64_t C, int64_t HW, const float* qp, int relu_first, void* ws,
                         double* sums, float* bias, int allow_single_launch, void* stream);

/* Dynamic ACIQ clipping (config 3: -c laplace / gaus, optionally -baa; int_quantizer.py:327-352 statistics, clipping and bit
 * allocation, 409-451 and 557-603 parameters and Q/DQ) on CONTIGUOUS bf16 / fp16 activations x[N][C][HW], on the storage as it
 * lies: no fp32 copy.  Counterpart of cnnq_pc_aciq_qdq behind ONE call; the rows are cut into pieces as for cnnq_pc_stats_dt
 * (W = 8 / 4 / 2 / 1 from HW and the alignment x and y share: every (HW, alignment) has a route); a workgroup owns one channel.
 * Routes:
 *   2. the chain: cnnq_pc_stats_dt's launches (pass A, merge; pass B and its merge when b is needed: Laplace clipping, or bit
 *      allocation on the b prior), cnnq_pc_params, cnnq_pc_qdq_dt's launch - 8 B/elem with b, 6 without;
 *   1. one launch, one 1024-lane workgroup per channel that keeps the channel in registers: moments, (b,) parameters, Q/DQ -
 *      4 B/elem.  Only where N * HW <= 131072 and W >= 2, and only without bit allocation in effect (which couples all
 *      channels through their std);
 *   3. pass A, merge and the bit allocation on the std prior, then route 1's launch reading its table - 6 B/elem;
 * The values of a piece are added in fp32 (pairs, then halves), the pieces in fp64, in an order fixed by (N, C, HW, alignment,
 * route) alone: run after run the same bits, no atomics, but not the fp32 chain's order.  Promised: stats[CNNQ_NSTAT][C] is
 * written completely (KURT and STD_POS zero, B zero unless b was needed), rows MIN / MAX exact (a NaN element makes them NaN),
 * MEAN / STD / B within the statistics tier of fp64; given that table, qp[CNNQ_NQP][C] and diag[CNNQ_NDIAG][C] are cnnq_pc_params'
 * and y is cnnq_pc_qdq_dt's on qp, bit for bit, on every route.  CNNQ_DTYPE_F32 forwards to cnnq_pc_aciq_qdq (stats: a copy of
 * its table).
 * cnnq_pc_aciq_dt_workspace: bytes of `ws` - cnnq_pc_stats_dt's records, which do not depend on the alignment or the route (fp32:
 * cnnq_pc_aciq_workspace at either alignment; 0 on bad arguments or a geometry beyond cnnq_pc_groups' limits).
 * cnnq_pc_route_aciq_dt (host only, nothing enqueued): out = {piece width W, batch splits S, column splits, route}; route 1 / 2 /
 * 3 as above, 0 - a class of layer that did not measure faster than the upcast route and is left there by callers that have the
 * choice (cnnq_pc_aciq_qdq_dt itself runs every class, on route 2): rows of an odd HW with N * HW >= 6272.  allow_single_launch:
 * 0 - never route 1 / 3; 1 - where they measured faster than route 2 (at least 128 channels and, from N * HW >= 65536 on, at
 * most 512 with bit allocation, 1024 without; from 25088 on, 256 channels, without bit allocation up to 512); 2 - wherever the
 * channel fits (tests, A/B).  A function of its arguments alone; fp32: {0,
 * cnnq_pc_groups' records, 1, 2}; align_bytes: the power of two that divides x and y (<= 16 is what matters). */
size_t cnnq_pc_aciq_dt_workspace(int64_t N, int64_t C, int64_t HW, int dtype);
int cnnq_pc_route_aciq_dt(int64_t N, int64_t C, int64_t HW, int dtype, int align_bytes, const cnnq_params_cfg* cfg, int allow_single_launch,
                          int32_t out[4]);
/* stats, qp and diag are OUTPUTS; diag may be NULL without bit allocation in effect.  ws: cnnq_pc_aciq_dt_workspace bytes, 8-byte
 * aligned (route 1 does not touch it).  A bad dtype, N, C or HW < 1, a NULL x / y / cfg / ws / stats / qp, a misaligned ws / stats /
 * qp / diag, an x or y not aligned to its element size, x == y, a cfg cnnq_pc_params refuses, direct_range, a clip other than
 * Laplace / Gaussian (1 / 2) or bit allocation without diag returns CNNQ_EINVAL, a geometry beyond cnnq_pc_groups' limits that
 * function's code - before anything touches the device.  Re-entrant, allocates nothing, no host synchronisation,
 * graph-capturable. */
int cnnq_pc_aciq_qdq_dt(const void* x, void* y, int dtype, int64_t N, int64_t C, int64_t HW, const cnnq_params_cfg* cfg, void* ws,
                        float* stats, float* qp, float* diag, int allow_single_launch, void* stream);

/* Config 5 (mid-tread quantization with per-channel bin allocation and Laplace clipping, optionally the histogram of its codes:
 * -c laplace -baa -mtq [-me]; int_quantizer.py:170-183 statistics and dispatch, 128-145 and 185-214 bin allocation, step sizes
 * and clamp bounds, 202-224 Q/DQ) on CONTIGUOUS bf16 / fp16 activations x[N][C][HW], on the storage as it lies: no fp32 copy.
 * Counterpart of cnnq_pc_midtread_nhwc; the rows are cut into pieces as for cnnq_pc_stats_dt (W = 8 / 4 / 2 / 1 from HW and the
 * alignment x and y share: every (HW, alignment) has a route); a workgroup owns one channel.
 * cnnq_pc_midtread_qdq_dt (iq.py:202-224): the table-driven pass with mt from cnnq_pc_midtread_params (clip = 1), one launch.
 * hist: NULL, or CNNQ_MT_HIST_WORDS(C) words ZEROED BY THE CALLER, read by cnnq_midtread_entropy[_batch].  Given mt, y and every
 * word of hist but the split of the window counts over the replica tables are, bit for bit, cnnq_pc_midtread_qdq's (clip = 1) on
 * x.float(), y rounded once into the element type.  CNNQ_DTYPE_F32 forwards to cnnq_pc_midtread_qdq(..., clip = 1, codes = NULL, ...).
 * cnnq_pc_midtread_dt (iq.py:170-225): ONE host call; stats[CNNQ_NSTAT][C] and mt[CNNQ_NMT][C] are OUTPUTS, hist is NULL or is
 * zeroed here.  Routes:
 *   2. the chain: cnnq_pc_stats_dt with b (four launches), cnnq_pc_midtread_params, the table-driven pass - 8 B/elem;
 *   3. pass A and its merge, omega and the clipping multiplier from the std alone, then one launch of one 1024-lane workgroup
 *      per channel that keeps the channel in registers: b, step size, clamp bounds, Q/DQ (and the histogram) - 6 B/elem.  Only
 *      where N * HW <= 131072 and W >= 2.  There is no route without pass A: the bin allocation couples all channels.
 * Promised on both routes: stats is written completely (KURT and STD_POS zero), rows MIN / MAX exact (a NaN element makes them
 * NaN), MEAN / STD / B within the statistics tier of fp64; given that table, rows OMEGA / ALPHA / DELTA / CMIN / CMAX of mt are
 * cnnq_pc_midtread_params', and y and hist are cnnq_pc_midtread_qdq_dt's on mt, bit for bit.  Row WSTART: route 2
 * cnnq_pc_midtread_params'; route 3 the bound a Laplace channel (b = std / sqrt 2) would have - an integer, >= -CNNQ_MT_HIST_BINS / 2,
 * the same in every channel; only the speed of the histogram depends on it.  CNNQ_DTYPE_F32: CNNQ_ENOTSUP, nothing enqueued
 * (fp32 has cnnq_pc_midtread_qdq_single and the chain).
 * cnnq_pc_midtread_dt_workspace: bytes of `ws` - cnnq_pc_stats_dt's records, which do not depend on the alignment or the route (0
 * on bad arguments, fp32, or a geometry beyond cnnq_pc_groups' limits).
 * cnnq_pc_route_midtread_dt (host only, nothing enqueued, a function of its arguments alone): out = {piece width W, batch splits S,
 * column splits of the statistics launches, route}; route 2 / 3 as above, 0 - a class of layer that did not measure faster than
 * the upcast route and is left there by callers that have the choice (cnnq_pc_midtread_dt itself runs every class, on route 2).
 * hist: whether the codes are counted.  allow_single_launch: 0 - never route 3; 1 - where it measured faster than route 2; 2 -
 * wherever the channel fits (tests, A/B).  align_bytes: the power of two that divides x and y (<= 16 is what matters).  fp32:
 * CNNQ_ENOTSUP.
 * A bad dtype, N, C or HW < 1, a NULL x / y / mt (/ tables / ws / stats), ntab < 2, a target that is not finite, a misaligned ws /
 * tables / stats / mt / hist, an x or y not aligned to its element size, x == y, a NULL out or an align_bytes that is not a power
 * of two return CNNQ_EINVAL, a geometry beyond cnnq_pc_groups' limits that function's code - before anything touches the device.
 * Re-entrant, allocate nothing, no host synchronisation, graph-capturable. */
size_t cnnq_pc_midtread_dt_workspace(int64_t N, int64_t C, int64_t HW, int dtype);
int cnnq_pc_route_midtread_dt(int64_t N, int64_t C, int64_t HW, int dtype, int align_bytes, int hist, int allow_single_launch,
                              int32_t out[4]);
int cnnq_pc_midtread_qdq_dt(const void* x, void* y, int dtype, int64_t N, int64_t C, int64_t HW, const float* mt, uint64_t* hist,
                            void* stream);
int cnnq_pc_midtread_dt(const void* x, void* y, int dtype, int64_t N, int64_t C, int64_t HW, double target, int sym, const double* tables,
                        int ntab, void* ws, float* stats, float* mt, uint64_t* hist, int allow_single_launch, void* stream);

/* The uniform per-channel Q/DQ with the histogram of its codes (-me: int_quantizer.py:586-587, the codes exist in the reference
 * only as the argument of shannon_entropy, 445) on CONTIGUOUS bf16 / fp16 activations x[N][C][HW], on the storage as it lies: no
 * fp32 copy.  Counterpart of the cnnq_pc_*_hist_nhwc entries; the rows are cut into pieces as for cnnq_pc_qdq_dt (W = 8 / 4 / 2 / 1
 * from HW and the alignment x and y share: every (HW, alignment) has a route); a workgroup owns one channel.
 * Given the table qp[CNNQ_NQP][C], y is cnnq_pc_qdq_dt's bit for bit, and the counts are, word for word once the replica tables
 * are summed, the histogram cnnq_pc_qdq fills on x.float().
 * hist_rep: cnnq_hist_replica_bytes() bytes, 8-byte aligned, zero at rest - the contract of the single-launch kernels: the calls
 * ADD to it, cnnq_entropy_replicas[_batch] and cnnq_hist_replicas_fold consume it and leave it zero.
 * nbins: the bins the counting workgroups keep, a power of two in [2, 256] above every channel's qmax (a code is counted in bin
 * code & (nbins - 1)); the dynamic forms choose it: 2^num_bits, 256 under bit allocation.
 * cnnq_pc_qdq_hist_dt (int_quantizer.py:573-592 with 586-587; counterpart of cnnq_pc_qdq with hist): the table-driven pass, one
 * launch.
 * cnnq_pc_minmax_qdq_hist_dt (int_quantizer.py:409-451, 557-603 with 586-587; config 2, dynamic; counterpart of
 * cnnq_pc_minmax_qdq_single with hist_rep), 2^num_bits bins.  Routes:
 *   1. one launch of one 1024-lane workgroup per channel that keeps the channel in registers: extrema, parameters, Q/DQ and the
 *      count - 4 B/elem.  Only where N * HW <= 131072 and W >= 2;
 *   2. cnnq_pc_minmax_qdq_auto_dt's statistics launch, then the counting pass, which merges the partials in its prologue - 6 B/elem.
 *   Both routes give the same bits.  ws: cnnq_pc_minmax_qdq_workspace bytes, 4-byte aligned (the partials live behind the tables'
 *   place in it); qp[CNNQ_NQP][C] and mm[2][C] (may be NULL) are OUTPUTS, written as cnnq_pc_minmax_qdq_auto_dt writes its own.
 * cnnq_pc_aciq_qdq_hist_dt (int_quantizer.py:327-352 + 409-451, 557-603 with 586-587; config 3, dynamic; counterpart of
 * cnnq_pc_aciq_qdq_single with hist_rep): cnnq_pc_aciq_qdq_dt's route 2 - cnnq_pc_stats_dt, cnnq_pc_params - with the counting
 * pass last; 256 bins under bit allocation, else 2^num_bits.  ws: cnnq_pc_aciq_dt_workspace bytes, 8-byte aligned; cfg, stats,
 * qp, diag as cnnq_pc_aciq_qdq_dt, whose refusals and promises apply; on top of them: num_bits > 8.
 * cnnq_pc_route_qdq_hist_dt (host only, nothing enqueued, a function of its arguments alone): out = {piece width W, batch splits
 * S of the counting launch (C * S workgroups), column splits of config 2's statistics launch, route}; route 1 / 2 as above, 0 - a
 * class of layer that did not measure faster than the upcast route and is left there by callers that have the choice (the calls
 * themselves run every class, on route 2).  allow_single_launch: 0 - never route 1; 1 - where it measured faster than route 2;
 * 2 - wherever the channel fits (tests, A/B).  align_bytes: the power of two that divides x and y (<= 16 is what matters).
 * A bad dtype, N, C or HW < 1, a NULL required pointer (hist_rep included), a misaligned ws / hist_rep, x == y, an nbins that is
 * not a power of two in [2, 256], num_bits outside [1, 8], a NULL out or an align_bytes that is not a power of two return
 * CNNQ_EINVAL, a geometry beyond cnnq_pc_groups' limits that function's code - before anything touches the device.
 * CNNQ_DTYPE_F32: CNNQ_ENOTSUP, nothing enqueued (fp32 has cnnq_pc_qdq with hist and the single-launch kernels).
 * Re-entrant, allocate nothing, no host synchronisation, graph-capturable.  cnnq_pc_qdq_dt keeps its contract: hist must be NULL. */
int cnnq_pc_route_qdq_hist_dt(int64_t N, int64_t C, int64_t HW, int dtype, int align_bytes, int nbins, int allow_single_launch,
                              int32_t out[4]);
int cnnq_pc_qdq_hist_dt(const void* x, void* y, int dtype, int64_t N, int64_t C, int64_t HW, const float* qp, int nbins,
                        uint64_t* hist_rep, void* stream);
int cnnq_pc_minmax_qdq_hist_dt(const void* x, void* y, int dtype, int64_t N, int64_t C, int64_t HW, int num_bits, int positive,
                               float* ws, float* qp, float* mm, uint64_t* hist_rep, int allow_single_launch, void* stream);
int cnnq_pc_aciq_qdq_hist_dt(const void* x, void* y, int dtype, int64_t N, int64_t C, int64_t HW, const cnnq_params_cfg* cfg, void* ws,
                             float* stats, float* qp, float* diag, uint64_t* hist_rep, void* stream);

/* The statistics of FEW, VERY LONG rows over flat storage - the per-tensor calibration table of statistic_manager.py:55-96
 * (rows = 1: the whole tensor) and the per-sample sums of squares of distance_stats.py:22-33 (rows = N: the samples) - for fp32 /
 * bf16 / fp16 elements, on the storage as it lies: x is viewed as [rows][len], every row contiguous and the rows back to back.
 * Whole-tensor and per-sample sums and extrema do not depend on the order of the elements and a sample of a dense channels_last
 * tensor is one contiguous block, so one reduction serves both layouts: no layout copy, no upcast, x read once per pass (8 B/elem
 * in fp32, 4 in bf16 / fp16 for the full table).  A row is cut into pieces of W elements (the widest of 16 / 8 / 4 / 2 bytes, or
 * one element, that divides len * sizeof(element) and x's alignment: every (rows, len, alignment) has a route) and into S chunks
 * of consecutive pieces, one 256-lane workgroup per (row, chunk); the sums are added in an order fixed by (rows, len, dtype,
 * alignment) alone: run after run the same bits, no atomics.  Promised: rows MIN / MAX exact (a NaN element makes them NaN),
 * every other row within the statistics tier of fp64 that cnnq_pc_stats_single keeps.  All offsets are 64 bits.
 * cnnq_rows_stats_workspace: bytes of `ws` - doubles part[S][CNNQ_NMOM][rows], mom[CNNQ_NMOM][rows], part2[S][CNNQ_NDEV][rows] for
 * the largest S over the piece widths (0 on bad arguments).
 * cnnq_rows_stats_route (host only, nothing enqueued): out = {elements per load W, chunks per row S, pieces per chunk, 1 - the row
 * has at most 4096 elements and is summed in fp64 element by element}; align_bytes: the power of two that divides x (at least the
 * element size; <= 16 is what matters). */
size_t cnnq_rows_stats_workspace(int64_t rows, int64_t len, int dtype);
int cnnq_rows_stats_route(int64_t rows, int64_t len, int dtype, int align_bytes, int32_t out[4]);
/* The table behind ONE call: pass A (all seven moment rows, the rectified sums included) -> cnnq_pc_combine(G = S, C = rows,
 * has_relu = 1) (-> pass B -> cnnq_pc_combine_dev(want_kurt = 1), when need_dev), two or four launches.  stats[CNNQ_NSTAT][rows]
 * is written completely: rows B and KURT are zero without need_dev.  mom[CNNQ_NMOM][rows]: the merged moment record, may be NULL
 * (kept in ws).  ws: cnnq_rows_stats_workspace bytes, 8-byte aligned.  A dtype outside cnnq_dtype, rows < 1, len < 1, a NULL x / ws /
 * stats, a misaligned ws / mom or an x not aligned to its element size returns CNNQ_EINVAL; 2^31 rows, a chunk of 2^31 pieces or
 * byte offsets beyond 63 bits CNNQ_ERANGE - before anything touches the device.  Re-entrant, allocates nothing, no host
 * synchronisation, graph-capturable. */
int cnnq_rows_stats(const void* x, int dtype, int64_t rows, int64_t len, int need_dev, void* ws, double* mom, float* stats,
                    void* stream);

/* Per-tensor clipping (iq.py:353-357: gemmlowpClippingQuantize where -pcq_a does not apply - "ACIQ layer-wise") and per-tensor
 * mid-tread quantization (iq.py:158-168) of fp32 / bf16 / fp16 elements over flat storage: x and y are n elements back to back.
 * One parameter set serves the whole tensor and y[i] depends on x[i] alone, so a contiguous tensor and a dense channels_last one
 * are the same call: no layout copy, no upcast, x read and y written once (8 B/elem in fp32, 4 in bf16 / fp16).  The arithmetic is
 * the per-channel kernels': given the table, y is, bit for bit, what cnnq_pc_qdq (cnnq_pc_midtread_qdq with clip = 1) gives for
 * N = 1, C = 1, HW = n on the same values - the IEEE divide, separate roundings, clamp before round, half to even; bf16 / fp16
 * elements are upconverted exactly and the fp32 result is rounded to nearest-even once (a NaN stays a NaN, an fp16 overflow
 * becomes inf): y == fp32_path(x.float()).to(x.dtype).  Elements go in pieces of 16 / 8 / 4 / 2 bytes (or one element), the widest
 * the alignment x and y share allows; the length does not matter (the first lanes take the n % W tail).
 * All of them return - before anything touches the device - CNNQ_EINVAL for a dtype outside cnnq_dtype, n < 1, a NULL required
 * pointer, an x or y not aligned to its element size, x == y; CNNQ_ERANGE for byte offsets beyond 63 bits or a grid of 2^31
 * workgroups.  Re-entrant, allocate nothing, no host synchronisation, graph-capturable.
 * cnnq_flat_qdq: the table-driven pass, one launch; qp[CNNQ_NQP][1] as cnnq_pc_params writes it for C = 1 (direct_range = 1 for
 *   the per-tensor branch: the kernel reads the three scalars and does not care).
 * cnnq_flat_midtread_qdq: the same for mt[CNNQ_NMT][1] of cnnq_pc_midtread_params (C = 1, clip = 1): t = round(x / delta), the two
 *   clamps, t * delta.  No histogram: the per-tensor branch discards the entropy. */
int cnnq_flat_qdq(const void* x, void* y, int dtype, int64_t n, const float* qp, void* stream);
int cnnq_flat_midtread_qdq(const void* x, void* y, int dtype, int64_t n, const float* mt, void* stream);
/* The dynamic forms behind ONE call.  ws: cnnq_pt_clip_workspace(n, dtype) bytes (= cnnq_rows_stats_workspace(1, n, dtype); 0 on
 * bad arguments), 8-byte aligned; stats[CNNQ_NSTAT][1] is an OUTPUT and is cnnq_rows_stats' table of the tensor, bit for bit.
 * cnnq_pt_clip_qdq: cnnq_rows_stats(rows = 1, need_dev = the clipping reads b: cfg->clip == 1) -> cnnq_pc_params(C = 1, with
 *   direct_range forced to 1: delta is the range itself, iq.py:357) -> the flat pass; three or five launches.  cfg->clip is 1, 2 or
 *   3 (laplace / gaus / pstd * std); bit allocation does not apply per tensor (iq.py:236): clip == 0 or bit_alloc != 0 is
 *   CNNQ_EINVAL, as is a cfg cnnq_pc_params refuses.  qp[CNNQ_NQP][1] out; diag[CNNQ_NDIAG][1] out, may be NULL.
 * cnnq_pt_midtread: cnnq_rows_stats(rows = 1, need_dev = 1) -> cnnq_pc_midtread_params(C = 1, clip = 1) -> the flat pass, five
 *   launches.  mt[CNNQ_NMT][1] out; tables: the (omega, alpha) tables [2][ntab] in device memory.  On top of the refusals above: a
 *   NULL cfg / ws / stats / qp / mt / tables, ntab < 2, a misaligned ws or a target that is not finite - CNNQ_EINVAL. */
size_t cnnq_pt_clip_workspace(int64_t n, int dtype);
int cnnq_pt_clip_qdq(const void* x, void* y, int dtype, int64_t n, const cnnq_params_cfg* cfg, void* ws, float* stats, float* qp,
                     float* diag, void* stream);
int cnnq_pt_midtread(const void* x, void* y, int dtype, int64_t n, double target, int sym, const double* tables, int ntab, void* ws,
                     float* stats, float* mt, void* stream);

/* Config 5 - mid-tread quantization with per-channel bin allocation, and the histogram of its codes for the entropy - on dense
 * channels_last activations.  As for config 3 the per-channel sums are added in an order fixed by (R, C, dtype, alignment)
 * alone, so `stats` is promised within the statistics tier of fp64 (MIN / MAX exact), not equal to the NCHW chain's.  Given
 * the table mt[CNNQ_NMT][C] (cnnq_pc_midtread_params with clip = 1 on stats), y is, bit for bit, cnnq_pc_midtread_qdq's with
 * clip = 1 on the same values in NCHW order - for bf16 / fp16 on the exactly upconverted values with one round-to-nearest-even
 * at the end - and so is the histogram: its first CNNQ_MT_HIST_BINS + 2 + 2 * C words and its flag word (zero or not), and the
 * window bins summed over the replica tables; cnnq_midtread_entropy / _batch consume it unchanged.  Activations always clip:
 * there is no clip = 0 form, and no codes output.
 * cnnq_pc_route_midtread_nhwc (host only, nothing enqueued): out as cnnq_pc_route_aciq_nhwc - {elements per load W, row slabs S
 * of the statistics launches, rows per slab, row loads per lane and slab, workgroups of the Q/DQ launch without (hist = 0) or
 * with (hist != 0) the histogram, 1 - the native launches (0 would say: this class of layer goes back to the copy route; none
 * does)}. */
int cnnq_pc_route_midtread_nhwc(int64_t R, int64_t C, int dtype, int align_bytes, int hist, int32_t out[6]);
/* The table-driven pass (int_quantizer.py:202-224: t = round(x / delta[c]), the two clamps, t * delta[c]; counterpart of
 * cnnq_pc_midtread_qdq with clip = 1): one launch.  hist: NULL, or CNNQ_MT_HIST_WORDS(C) words zeroed by the caller, 8-byte
 * aligned.  A bad dtype, R < 1, C < 1, a NULL x / y / mt, a misaligned hist or x == y returns CNNQ_EINVAL before anything
 * touches the device.  Re-entrant, allocates nothing, no host synchronisation. */
int cnnq_pc_midtread_qdq_nhwc(const void* x, void* y, int dtype, int64_t R, int64_t C, const float* mt, uint64_t* hist, void* stream);
/* The dynamic pipeline (int_quantizer.py:170-225: per-channel min / max / mean / std / b, omega by eq. 10 128-135, the clipping
 * multiplier 137-145, delta and the clamp bounds 193-214, the Q/DQ 202-224, the codes' histogram for 179, 217) behind ONE call
 * on [R][C]; counterpart of cnnq_pc_stats + cnnq_pc_midtread_params + cnnq_pc_midtread_qdq: pass A -> merge -> pass B -> merge
 * -> cnnq_pc_midtread_params (clip = 1) -> Q/DQ, six launches.  stats[CNNQ_NSTAT][C] and mt[CNNQ_NMT][C] are OUTPUTS.  hist:
 * NULL, or CNNQ_MT_HIST_WORDS(C) words, 8-byte aligned, zeroed HERE on the stream.  tables: the (omega, alpha) tables
 * [2][ntab] in device memory.  ws: cnnq_pc_aciq_nhwc_workspace bytes (the same records), 8-byte aligned.  On top of the
 * refusals above: a NULL tables / ws / stats / mt, ntab < 2, a misaligned ws or a target that is not finite - CNNQ_EINVAL
 * before anything touches the device.  Re-entrant, allocates nothing, no host synchronisation. */
int cnnq_pc_midtread_nhwc(const void* x, void* y, int dtype, int64_t R, int64_t C, double target, int sym, const double* tables,
                          int ntab, void* ws, float* stats, float* mt, uint64_t* hist, void* stream);

/* The uniform per-channel Q/DQ with the histogram of its codes (-me: int_quantizer.py:586-587, the codes exist in the
 * reference only as the argument of shannon_entropy, 445) on dense channels_last activations.  Given the table
 * qp[CNNQ_NQP][C], y is cnnq_pc_qdq_nhwc's bit for bit, and the counts are, word for word once the replica tables are summed,
 * the histogram cnnq_pc_qdq fills on the same values in NCHW order (for bf16 / fp16 on the exactly upconverted values).
 * hist_rep: cnnq_hist_replica_bytes() bytes, 8-byte aligned, zero at rest - the contract of the single-launch kernels: the
 * calls ADD to it, cnnq_entropy_replicas[_batch] and cnnq_hist_replicas_fold consume it and leave it zero.
 * nbins: the bins the counting workgroups keep, a power of two in [2, 256] above every channel's qmax (a code is counted in
 * bin code & (nbins - 1)); the dynamic forms choose it: 2^num_bits, 256 under bit allocation.
 * All three refuse - CNNQ_EINVAL before anything touches the device - a bad dtype, R < 1, C < 1, a NULL required pointer
 * (hist_rep included), a misaligned ws or hist_rep, and x == y; CNNQ_ERANGE as their counterparts without the histogram.
 * Re-entrant, no allocation, no host synchronisation, graph-capturable.
 * cnnq_pc_route_qdq_hist_nhwc (host only, nothing enqueued): out = {elements per load W (cnnq_pc_route_nhwc's out[0]),
 * workgroups of the counting launch, its dynamic LDS bytes (nbins * 32 replicas * 4), 1 - the native launch (0 would say:
 * this class of layer goes back to the copy route; none does)}. */
int cnnq_pc_route_qdq_hist_nhwc(int64_t R, int64_t C, int dtype, int align_bytes, int nbins, int32_t out[4]);
/* The table-driven pass (int_quantizer.py:573-592 with 586-587; counterpart of cnnq_pc_qdq with hist): one launch.  On top
 * of the refusals above: an nbins that is not a power of two in [2, 256]. */
int cnnq_pc_qdq_hist_nhwc(const void* x, void* y, int dtype, int64_t R, int64_t C, const float* qp, int nbins, uint64_t* hist_rep,
                          void* stream);
/* Config 2, dynamic (int_quantizer.py:409-451, 557-603 with 586-587; counterpart of cnnq_pc_minmax_qdq_single with hist_rep):
 * the three launches in front of cnnq_pc_minmax_qdq_nhwc's Q/DQ unchanged, then the counting pass with 2^num_bits bins.  ws:
 * cnnq_pc_nhwc_workspace bytes, 4-byte aligned; qp and mm (may be NULL) as cnnq_pc_minmax_qdq_nhwc.  On top of the refusals
 * above: num_bits outside [1, 8]. */
int cnnq_pc_minmax_qdq_hist_nhwc(const void* x, void* y, int dtype, int64_t R, int64_t C, int num_bits, int positive, float* ws,
                                 float* qp, float* mm, uint64_t* hist_rep, void* stream);
/* Config 3, dynamic (int_quantizer.py:327-352 + 409-451, 557-603 with 586-587; counterpart of cnnq_pc_aciq_qdq_single with
 * hist_rep): cnnq_pc_aciq_qdq_nhwc's statistics and parameter launches unchanged, then the counting pass - 256 bins under bit
 * allocation, else 2^num_bits.  ws: cnnq_pc_aciq_nhwc_workspace bytes, 8-byte aligned; cfg, stats, qp, diag as
 * cnnq_pc_aciq_qdq_nhwc, whose refusals apply; on top of them: num_bits > 8. */
int cnnq_pc_aciq_qdq_hist_nhwc(const void* x, void* y, int dtype, int64_t R, int64_t C, const cnnq_params_cfg* cfg, void* ws,
                               float* stats, float* qp, float* diag, uint64_t* hist_rep, void* stream);

/* Activation bias correction (iqm.py:180-196) fused into the table-driven Q/DQ on dense channels_last activations; counterpart
 * of cnnq_pc_qdq_bcorr_sums + cnnq_pc_bcorr_bias + cnnq_pc_qdq_bcorr behind ONE call on [R][C], three launches:
 *   1. per channel sum x', sum q, count(x' > 0) over slabs of rows, with q = the fp32 Q/DQ of x from qp[CNNQ_NQP][C] (the IEEE
 *      divide) and x' = relu(x) when relu_first != 0, into ws (read-only pass over x);
 *   2. cnnq_pc_bcorr_bias on those records: bias[c] = ((float)sum x' - (float)sum q) / ((float)count + 1e-8f), and - sums !=
 *      NULL - the merged sums[3][C] (doubles);
 *   3. y = q + (q > 0) * bias[c], rounded once into the element type.
 * The sums are added in an order fixed by (R, C, dtype, alignment) alone: run after run the same bits, not the NCHW chain's
 * order.  Promised: the sums within the statistics tier of fp64 (the count exact), and given them bias and y bit for bit.
 * bias[C] is an OUTPUT.  ws: cnnq_pc_qdq_bcorr_nhwc_workspace bytes (the records of the widest slab count over the piece
 * widths; 0 on bad arguments), 8-byte aligned, as sums.  A bad dtype, R < 1, C < 1, a NULL x / y / qp / ws / bias, a
 * misaligned ws / sums or x == y returns CNNQ_EINVAL before anything touches the device.  Re-entrant, allocates nothing, no host
 * synchronisation. */
size_t cnnq_pc_qdq_bcorr_nhwc_workspace(int64_t R, int64_t C, int dtype);
int cnnq_pc_qdq_bcorr_nhwc(const void* x, void* y, int dtype, int64_t R, int64_t C, const float* qp, int relu_first, void* ws,
                           double* sums, float* bias, void* stream);

/* Integer codes as the STORED format of a dense channels_last activation: per-channel widths of 0..8
 * bits on [R = N*H*W][C], C innermost, fp32 / bf16 / fp16 elements, on the storage as it is (no upcast, no transpose).
 *
 * Format.  Row r stores the codes of channels 0..C-1 as one little-endian bit stream: channel c occupies bits
 * [coloff[c], coloff[c] + bits[c]) of the row.  coloff holds C + 1 uint32 entries (device memory), the exclusive prefix sum of
 * the widths; coloff[C] is the number of bits per row.  A row is padded with zero bits to whole dwords, rowbytes =
 * 4 * ceil(coloff[C] / 32), and row r starts at byte r * rowbytes; the buffer holds R * rowbytes bytes and no byte beyond them
 * is ever written.  Every width is an integer in 0..8; a 0-bit channel stores nothing and decodes to (0 - zp) * scale.  Uniform
 * 4 bits (coloff[c] = 4 c) and uniform 8 bits are this format with a constant width table: there is no second format.
 * Examples: bits = {3, 0, 5} with the codes {5, 0, 17} is the row 8D 00 00 00; bits = {8, 8, 8, 7, 3} gives coloff =
 * {0, 8, 16, 24, 31, 34} - the last channel straddles dwords 0 and 1 - and rowbytes = 8.
 *
 * The stored code is the code of cnnq_pc_qdq_nhwc for that element with the same qp[CNNQ_NQP][C] (with the channels' exact
 * extrema mm[2][C] the divide-free quotient's inside its domain: the same bits; mm may be NULL), masked to the channel's width:
 * a qp whose qmax[c] exceeds 2^bits[c] - 1 is the caller's error and may truncate that channel's codes, never touch a
 * neighbour's bits.  Decode is (code - zp) * scale rounded once into the element type, so the round trip reproduces
 * cnnq_pc_qdq_nhwc bit for bit - with one exception: a NaN code cannot be stored and is stored as 0, so a NaN element of a
 * channel with finite parameters comes back as (0 - zp) * scale; a channel whose zp is NaN still decodes to NaN.
 *
 * cnnq_pc_packed_nhwc_capacity (host only): R * 4 * ceil(8 * C / 32), the bytes of the buffer at 8 bits per code - enough for
 *   every width table; 0 on R < 1 or C < 1.
 * cnnq_pc_packed_layout_nhwc: coloff from the device table bits[C] (floats, e.g. row CNNQ_DIAG_BITS of diag), or - bits == NULL -
 *   from the width uniform_bits for every channel.  Every width is clamped into 0..8, NaN to 0.
 * cnnq_pc_route_packed_nhwc (host only, nothing enqueued): out = {elements per load W (cnnq_pc_route_nhwc's out[0]), workgroups
 *   of the pack launch, rows per pack workgroup, 1 - native}.  out[3] == 0: the library has no pack kernel for this class of
 *   layer (a row image beyond 8 KB, C > 8192: cnnq_pc_quantize_packed_nhwc returns CNNQ_ENOTSUP) and out[1], out[2] are 0.
 * cnnq_pc_quantize_packed_nhwc: x -> packed, one launch.  Every dword of the R * rowbytes bytes is written exactly once by a
 *   plain store, padding bits included: no atomics on global memory, the same bytes run after run.
 * cnnq_pc_dequantize_packed_nhwc: packed -> y, one launch (any C).
 * cnnq_pc_minmax_quantize_packed_nhwc: config 2 in one call - the three statistics launches of cnnq_pc_minmax_qdq_nhwc, the
 *   layout for the uniform width num_bits (1..8), the pack launch with the extrema.  ws: cnnq_pc_nhwc_workspace bytes; qp and
 *   mm (may be NULL) as cnnq_pc_minmax_qdq_nhwc; coloff[C + 1] is an OUTPUT.
 * cnnq_pc_aciq_quantize_packed_nhwc: config 3 in one call - cnnq_pc_aciq_qdq_nhwc's statistics and parameter launches, the
 *   layout from diag[CNNQ_DIAG_BITS] under bit allocation, else from cfg->num_bits (which must then be <= 8), the pack launch.
 *   ws: cnnq_pc_aciq_nhwc_workspace bytes, 8-byte aligned; cfg, stats, qp, diag as cnnq_pc_aciq_qdq_nhwc; coloff is an OUTPUT.
 * The piece width comes from x's (the decoder: y's) alignment alone, so a Q/DQ entry point whose plan has the same W writes the
 * same tables bit for bit.  All of them return CNNQ_EINVAL before anything touches the device for a NULL required pointer,
 * R < 1, C < 1, a bad dtype, a `packed` that is not 4-byte aligned, a misaligned ws, num_bits outside 1..8; CNNQ_ERANGE as
 * cnnq_pc_qdq_nhwc; CNNQ_ENOTSUP (the encoders, C > 8192) before any launch.  Re-entrant, allocate nothing, no host
 * synchronisation. */
size_t cnnq_pc_packed_nhwc_capacity(int64_t R, int64_t C);
int cnnq_pc_packed_layout_nhwc(const float* bits, int uniform_bits, int64_t C, uint32_t* coloff, void* stream);
int cnnq_pc_route_packed_nhwc(int64_t R, int64_t C, int dtype, int align_bytes, int32_t out[4]);
int cnnq_pc_quantize_packed_nhwc(const void* x, int dtype, int64_t R, int64_t C, const float* qp, const float* mm,
                                 const uint32_t* coloff, uint8_t* packed, void* stream);
int cnnq_pc_dequantize_packed_nhwc(const uint8_t* packed, void* y, int dtype, int64_t R, int64_t C, const float* qp,
                                   const uint32_t* coloff, void* stream);
int cnnq_pc_minmax_quantize_packed_nhwc(const void* x, int dtype, int64_t R, int64_t C, int num_bits, int positive, float* ws,
                                        float* qp, float* mm, uint32_t* coloff, uint8_t* packed, void* stream);
int cnnq_pc_aciq_quantize_packed_nhwc(const void* x, int dtype, int64_t R, int64_t C, const cnnq_params_cfg* cfg, void* ws,
                                      float* stats, float* qp, float* diag, uint32_t* coloff, uint8_t* packed, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CNNQ_HIP_H */
