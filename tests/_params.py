"""Reference restatements for the parameter kernels (k_params / bit_alloc_block / channel_params, k_pt_setup / ptf_params) on
statistics TABLES - helper, no tests.  Everything is built from oracle/quant_oracle.py's own pieces; test_params_table_cpu.py
pins it to the oracle's end-to-end functions and to the bit-allocation golden, so the GPU tests compare against something
anchored.  The only line that is not the oracle's is marked LIBRARY CHOICE: an input on which the reference raises."""
import math

import numpy as np
import torch

from oracle import quant_oracle as O

STAT_MIN, STAT_MAX, STAT_MEAN, STAT_STD, STAT_B, NSTAT = 0, 1, 2, 3, 4, 7


def f32(v):
    return np.ascontiguousarray(np.asarray(v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else v, dtype=np.float32))


def same_bits(a, b):
    """fp32 arrays equal bit for bit where neither is NaN, and NaN in the same places (a NaN's payload is not pinned)."""
    a, b = f32(a), f32(b)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def first_diff(a, b):
    """Index, got and expected of the first element on which same_bits fails (for messages)."""
    a, b = f32(a).ravel(), f32(b).ravel()
    na, nb = np.isnan(a), np.isnan(b)
    bad = (na != nb) | (~na & ~nb & (a.view(np.uint32) != b.view(np.uint32)))
    i = int(np.flatnonzero(bad)[0])
    return i, float(a[i]), float(b[i])


def make_table(C, mn, mx, mean, std, b):
    t = torch.zeros(NSTAT, C, dtype=torch.float32)
    for row, v in ((STAT_MIN, mn), (STAT_MAX, mx), (STAT_MEAN, mean), (STAT_STD, std), (STAT_B, b)):
        t[row] = torch.as_tensor(v, dtype=torch.float32)
    return t


def _target(num_bits, target):
    """What act_per_channel_qdq hands to bits_alloc_fixed_target: the target, an int where it is one (as the CLI gives it)."""
    t = num_bits if target is None else target
    return int(t) if float(t) == int(t) else float(t)


def params_ref(table, num_bits, positive, clip, bit_alloc, prior_is_b, target, round_mode, direct_range):
    """[>= 5, C] statistics table -> (scale, zp, qmax, bits, alpha, delta, offset), fp32 numpy [C] each: iq.py:227-300 (alpha),
    :284-300 (range / offset), :351 / :443 (delta), :381-407 (bit allocation), :559-572 (scale, floor, zero point)."""
    table = torch.from_numpy(f32(table))
    C = table.shape[1]
    mn, mx, mean, std, b = (table[r] for r in (STAT_MIN, STAT_MAX, STAT_MEAN, STAT_STD, STAT_B))
    ba = bool(bit_alloc) and num_bits <= 4                                              # iq.py:432
    bits = O.bits_alloc_fixed_target(b if prior_is_b else std, _target(num_bits, target), bool(round_mode)) if ba else None
    with np.errstate(all='ignore'):
        if clip == 'no':
            alpha = np.zeros(C, dtype=np.float32)
            offset = torch.zeros(C) if positive else mn                                 # iq.py:411-416
            delta = mx - offset                                                         # iq.py:443
        else:
            if clip == 'laplace':
                if ba:
                    # LIBRARY CHOICE: the reference raises on NaN bits (int(nan)); here they take the 0-bit factor
                    fac = [O.aciq_factor(int(v) if v == v else 0, 'laplace', positive) for v in bits.tolist()]
                    alpha = b * torch.tensor(np.array(fac), dtype=torch.float32)        # as O.alpha_laplace
                else:
                    alpha = O.alpha_laplace(b, num_bits, positive)
            elif clip == 'gaus':
                alpha = std * O.aciq_factor(num_bits, 'gaus', positive)                 # num_bits, not the channel's bits: iq.py:264
            else:
                alpha = float(clip.replace('std', '')) * std
            rng, off = O.alpha_to_delta_offset(alpha, mx, mn, mean, positive)
            rng = torch.from_numpy(f32(rng))
            offset = torch.from_numpy(np.broadcast_to(f32(off), (C,)).copy())
            if direct_range:
                delta = rng                                                             # iq.py:357
            else:
                delta = (offset + rng) - offset                                         # iq.py:351, :443
            alpha = f32(alpha)
        _, _, scale, zp, qmax = O.qdq_core(torch.zeros(C, 1), delta, offset, num_bits=num_bits, bit_alloc=bits, return_parts=True)
    qmax = np.broadcast_to(f32(qmax), (C,)).copy()
    scale, zp = f32(scale).copy(), f32(zp).copy()
    bits = f32(bits) if ba else np.full(C, float(num_bits), dtype=np.float32)
    return scale, zp, qmax, bits, alpha, f32(delta), f32(offset)


def bit_alloc_f64(prior, target, round_mode):
    """iq.py:381-407 restated in fp64 -> (bits [C] fp64, margin).  margin: the smallest distance of any live channel's
    log2(bins) from a rounding boundary (k + 0.5 for round, integers for ceil) over all iterations; live: -0.6 < log2(bins) <
    8.6 (beyond that the clamps decide).  inf when no channel is ever live."""
    p = np.asarray(f32(prior), dtype=np.float64) ** (2. / 3)
    C = p.size
    psum = p.sum()
    goal = float(target)
    tgt, delta, it, margin, bits = goal, 1., 0, math.inf, None
    while abs(2 * delta) > 0.01 and it < 10:
        it += 1
        with np.errstate(all='ignore'):
            lg = np.log2((C * 2. ** tgt) * p / psum)
        bits = np.clip(np.rint(lg) if round_mode else np.ceil(lg), 0., 8.)
        live = lg[(lg > -0.6) & (lg < 8.6)]
        if live.size:
            d = np.abs(live - (np.floor(live) + 0.5)) if round_mode else np.abs(live - np.rint(live))
            margin = min(margin, float(d.min()))
        delta = (goal - bits.mean()) / 2
        tgt += delta
    return bits, margin


def bit_alloc_margin(prior, target, round_mode):
    return bit_alloc_f64(prior, target, round_mode)[1]


MARGIN = 2e-5


def guarded_prior(C, seed):
    """The prior of the guarded list: log-normal, about three octaves wide."""
    gen = torch.Generator().manual_seed(seed)
    return torch.exp(1.2 * torch.randn(C, generator=gen)) * 0.3


# (C, target, round_mode, seed): every cell the GPU test runs.  test_params_table_cpu.py asserts for each that bit_alloc_margin >
# MARGIN and that the fp32 oracle equals the fp64 restatement - a condition on the inputs, computed from the reference alone.
# C = 1 makes bins == 2^target exactly (a boundary for ceil and for 5.3): round and integer targets only.
BA_COMBOS = [(4, True), (4, False), (5.3, True), (2, False), (3, True)]
BA_SEEDS = {
    (1, 4, True): 0, (1, 3, True): 0,
    (2, 4, True): 0, (2, 4, False): 0, (2, 5.3, True): 0, (2, 2, False): 0, (2, 3, True): 0,
    (63, 4, True): 0, (63, 4, False): 0, (63, 5.3, True): 0, (63, 2, False): 0, (63, 3, True): 0,
    (64, 4, True): 0, (64, 4, False): 0, (64, 5.3, True): 0, (64, 2, False): 0, (64, 3, True): 0,
    (65, 4, True): 0, (65, 4, False): 0, (65, 5.3, True): 0, (65, 2, False): 0, (65, 3, True): 0,
    (1000, 4, True): 2, (1000, 4, False): 0, (1000, 5.3, True): 0, (1000, 2, False): 0, (1000, 3, True): 1,
    (1024, 4, True): 1, (1024, 4, False): 0, (1024, 5.3, True): 0, (1024, 2, False): 0, (1024, 3, True): 0,
    (1025, 4, True): 3, (1025, 4, False): 0, (1025, 5.3, True): 0, (1025, 2, False): 0, (1025, 3, True): 0,
    (4096, 4, True): 3, (4096, 4, False): 1, (4096, 5.3, True): 0, (4096, 2, False): 0, (4096, 3, True): 3,
    (4097, 4, True): 0, (4097, 4, False): 0, (4097, 5.3, True): 2, (4097, 2, False): 1, (4097, 3, True): 0,
    (6000, 4, True): 7, (6000, 4, False): 0, (6000, 5.3, True): 4, (6000, 2, False): 3, (6000, 3, True): 4,
}


def ba_cases():
    return [(C, t, r, s) for (C, t, r), s in BA_SEEDS.items()]


def hi_prior(seed):
    """C = 6000 with every varied channel at an index >= 4096 (the recompute loop of bit_alloc_block); the rest share one value."""
    p = guarded_prior(6000, seed)
    p[:4096] = 0.3
    return p


HI_SEED = 2


# ------------------------------------------------------------------------------------------------ per tensor (config 1)
def _exact_sum(v):
    v = [float(e) for e in v]
    if all(math.isfinite(e) for e in v):
        return math.fsum(v)
    return float(np.sum(np.asarray(v, dtype=np.float64)))        # NaN / inf: the outcome does not depend on the order


def exact_ceil_log2(s):
    """ceil(log2(s)) of a positive finite float, exactly (from the binary exponent)."""
    m, e = math.frexp(float(s))
    return e - 1 if m == 0.5 else e


def log2_frac(s):
    """The fractional part of log2 of a positive finite float, in [0, 1): 0 exactly for the powers of two."""
    m, _ = math.frexp(float(s))
    return math.log2(2 * m)


def ptp_words(rng, offset, ptz, num_bits, int_exp):
    """kernels/gemmlowp.cu:30-41 on fp32 range / offset -> the eight ptp words: scale, shift, qmax, true-zero flag, pass flag
    (range <= 0), range, offset, 0."""
    rng, offset = np.float32(rng), np.float32(offset)
    qmax = np.float32((1 << num_bits) - 1)
    with np.errstate(all='ignore'):
        scale = np.float32(rng / qmax)
        if int_exp:
            scale = np.float32(2.0 ** exact_ceil_log2(scale))
        zp = O.roundf_np(np.asarray([np.float32(-offset / scale)], dtype=np.float32))[0]
        shift = zp if ptz else np.float32(-offset)
    return np.array([scale, shift, qmax, 1. if ptz else 0., 1. if rng <= 0 else 0., rng, offset, 0.], dtype=np.float32)


def pt_extrema(mins, maxs, rows_mode, zero_min):
    """The fp32 (min, max) of iq.py:361-379 from per-row extrema: rows_mode 0 - the batch mean, an fp64 sum, one division, one
    rounding to fp32; rows_mode 1 - the NaN-propagating extrema.  zero_min: half range."""
    mins, maxs = f32(mins), f32(maxs)
    rows = mins.size
    with np.errstate(all='ignore'):
        if rows_mode == 0:
            mn, mx = np.float32(_exact_sum(mins) / rows), np.float32(_exact_sum(maxs) / rows)
        else:
            mn, mx = np.float32(np.min(mins)), np.float32(np.max(maxs))       # np.min / np.max propagate NaN, as torch.min / max
    if zero_min:
        mn = np.float32(0.)
    return mn, mx


def pt_params_ref(mins, maxs, rows_mode, zero_min, num_bits, int_exp, etz):
    mn, mx = pt_extrema(mins, maxs, rows_mode, zero_min)
    with np.errstate(all='ignore'):
        rng = np.float32(mx - mn)                                            # iq.py:379, fp32
        ptz = bool(etz) and bool(np.float32(mn + rng) > 0) and bool(mn < 0)  # iq.py:613
    return ptp_words(rng, mn, ptz, num_bits, int_exp)


def pt_params_host_ref(rng, offset, num_bits, int_exp, etz):
    """Host scalars (`range_offset=`): the caller has decided the true-zero flag (iq.py:613 ran on the host)."""
    return ptp_words(rng, offset, bool(etz), num_bits, int_exp)


# ------------------------------------------------------------------------------------------------ clip modes on edge statistics
# name, min, max, mean, std, b: one channel per branch of channel_params, so a failure names the branch
EDGE_ROWS = [
    ('plain',              -1.0,   2.0,  0.3,  0.8,  0.6),
    ('mean_neg',           -3.0,   1.0, -0.4,  0.7,  0.5),     # positive: max(mean, 0) = 0
    ('all_neg',            -5.0,  -1.0, -3.0,  0.9,  0.7),
    ('vmin_above',         -0.1,   4.0,  0.3,  0.8,  0.6),     # vmin > mean - alpha: the offset is vmin
    ('vmin_below',        -50.0,   4.0,  0.3,  0.8,  0.6),     # vmin < mean - alpha: the offset is mean - alpha
    ('std0',               -1.0,   2.0,  0.3,  0.0,  0.6),
    ('b0',                 -1.0,   2.0,  0.3,  0.8,  0.0),
    ('std0_b0',            -1.0,   2.0,  0.3,  0.0,  0.0),
    ('max_eq_min',          0.7,   0.7,  0.7,  0.0,  0.0),
    ('zero_bits',          -1.0,   2.0,  0.3, 1e-7, 1e-7),     # bit allocation drives it to 0 bits: scale at the 1e-8 floor
    ('wide',             -300.0, 500.0, 20.0, 120., 90.0),
    ('narrow',            -0.02,  0.03, 0.001, 0.01, 0.007),
]
EDGE_NAMES = [r[0] for r in EDGE_ROWS]
# the bit-allocated runs on the edge table: (num_bits = target, round_mode), both priors - guarded like BA_SEEDS
EDGE_BA = [(2, True), (3, True), (4, True), (4, False)]


def edge_table():
    cols = list(zip(*[r[1:] for r in EDGE_ROWS]))
    return make_table(len(EDGE_ROWS), *cols)
