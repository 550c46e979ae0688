"""Reference restatement for the mid-tread parameter kernel (k_mt_params: mt_omega_alpha + mt_channel) on statistics TABLES -
helper, no tests.  mt_ref is built from oracle/quant_oracle.py's own pieces (omega_alloc, alpha_mult_from_tables, the lines of
mid_tread_core behind the statistics); test_midtread_params_cpu.py pins it to the oracle's end-to-end function, to the mid-tread
golden and to tests/golden/midtread_params.npz (the reference's own get_omega / get_alpha_mult), so the GPU test compares against
something anchored.  Every line that is not the oracle's is marked LIBRARY CHOICE: an input on which the reference raises, or a
row the reference does not have.

Guarded inputs: the device's powf and its fp64 sum of the priors may differ from the CPU's in the last place, so every std vector
the GPU test uses keeps the fp64 quotient C * 2^target * p / sum p of every channel more than MARGIN * max(1, quotient) away from a
half-integer (omega_margin) - a condition on the inputs, computed from the arithmetic alone.  The one exception is TIE, which needs
no powf."""
import math

import numpy as np
import torch

from _params import MARGIN, STAT_B, STAT_MAX, STAT_MEAN, STAT_MIN, STAT_STD, f32, first_diff, guarded_prior, make_table, same_bits  # noqa: F401
from oracle import quant_oracle as O

MT_DELTA, MT_CMIN, MT_CMAX, MT_OMEGA, MT_ALPHA, MT_WSTART, NMT = 0, 1, 2, 3, 4, 5, 6   # include/cnnq_hip.h (pinned in the CPU test)
HIST_BINS, HIST_WINDOW = 131072, 128
ROWS = ('omega', 'alpha', 'delta', 'cmin', 'cmax', 'wstart')
ROW_INDEX = (MT_OMEGA, MT_ALPHA, MT_DELTA, MT_CMIN, MT_CMAX, MT_WSTART)
F32_MAX = np.finfo(np.float32).max
SQRT_HALF = np.float32(0.70710678)               # the <GUESS> form's b: std * 0.70710678f


def real_tables():
    from _direct import midtread_tables
    return midtread_tables()


# hand-built dyadic interpolation tables.  A: the first knot is 0 (as in the real table) - omega 0 sits ON it and the wrapped
# segment has zero distance; B: the first knot is above zero, so omega 0 and 1 take the wrapped segment (last entry -> first) with
# a non-zero distance, and the first segment (2, 4] has an integer strictly inside
HAND_A = (np.array([0., 1., 2., 4., 8., 16.]), np.array([0., .5, 1.25, 2., 3.5, 4.]))
HAND_B = (np.array([2., 4., 8., 16., 18.]), np.array([1., 1.5, 2.5, 3., 5.]))
# C: a cliff behind the knot at 4.  Linear interpolation is continuous at a knot, so taking the segment behind it (side='right')
# gives the same value wherever the fp64 arithmetic is exact - not here: (1e17 - 1) / 3 * 3 is not 1e17 - 1, while the segment
# in front of the knot gives alpha_table[i] - inc * 0 == 1 exactly
HAND_C = (np.array([0., 4., 7., 8.]), np.array([0., 1., 1e17, 1e17]))
# omega -> multiplier, worked out by hand from iq.py:142-144 (symmetric range)
HAND_A_VALUES = {0: 0., 1: .5, 3: 1.625, 16: 4., 2: 1.25, 6: 2.75, 12: 3.75, 20: 4.25}
HAND_C_VALUES = {0: 0., 2: .5, 4: 1., 7: 1e17, 8: 1e17, 10: 1e17}
HAND_B_VALUES = {0: .5, 1: .75, 2: 1., 3: 1.25, 4: 1.5, 12: 2.75, 17: 4., 18: 5., 20: 7., 43: 30.}


def alpha_ref(omega, sym, otab, atab):
    """The clipping multiplier of fp32 `omega` [C] -> fp64 numpy [C]: the oracle's alpha_mult_from_tables wherever the reference
    computes one (numpy's i - 1 == -1 wrap at i == 0 included - that one is the reference's own behaviour), else the library's."""
    otab, atab = np.asarray(otab, dtype=np.float64), np.asarray(atab, dtype=np.float64)
    om = omega.detach().numpy().copy()
    if not sym:
        om *= 2                                                                 # fp32, as the oracle
    inside = om <= otab[-1]                                                     # (False for NaN)
    am = np.empty(om.shape, dtype=np.float64)
    if inside.any():
        am[inside] = O.alpha_mult_from_tables(omega[torch.from_numpy(inside)], sym, otab, atab)
    with np.errstate(all='ignore'):
        # LIBRARY CHOICE: beyond the last knot the reference raises IndexError (searchsorted == ntab); the kernel clamps the
        # index to the last entry, i.e. extrapolates along the last segment
        i, im = otab.size - 1, otab.size - 2
        inc = (atab[i] - atab[im]) / (otab[i] - otab[im])
        beyond = ~inside & ~np.isnan(om)
        am[beyond] = atab[i] - inc * (otab[i] - om[beyond].astype(np.float64))
    # LIBRARY CHOICE: a NaN omega (the reference raises IndexError: NaN sorts behind the table) gives a NaN multiplier - the
    # kernel's search ends at i == 0, wraps to the last entry and the NaN distance poisons the result
    am[np.isnan(om)] = np.nan
    return am


def mt_ref(table, target, clip, sym, otab, atab):
    """[>= 5, C] statistics table -> (omega, alpha, delta, cmin, cmax, wstart), fp32 numpy [C] each: iq.py:128-135 and :187
    (omega), :137-145 (the multiplier), :194-199 (range, Delta), :208-210 (clamp bounds), in the fp32 operation order of
    iq.py:185-214; WSTART is the library's own row."""
    table = torch.from_numpy(f32(table))
    C = table.shape[1]
    mn, mx, mu, std, b = (table[r] for r in (STAT_MIN, STAT_MAX, STAT_MEAN, STAT_STD, STAT_B))
    zero = mu.new_tensor([0.])
    with np.errstate(all='ignore'):
        omega = O.omega_alloc(std, target_bins=(2 ** target)).round()                                   # iq.py:187
        if clip:
            am = mu.new_tensor(alpha_ref(omega, sym, otab, atab))                                       # iq.py:190
            rng = (2 * am * b) if sym else (torch.max(mu, zero) + am * b)                               # iq.py:194
        else:
            am = torch.zeros(C)                                    # LIBRARY CHOICE: row ALPHA without clipping holds 0
            rng = (mx - mn) if sym else mx                                                              # iq.py:196
        delta = torch.where(omega > 0, rng / omega, mu.new_tensor([F32_MAX]))                           # iq.py:198
        if clip:
            mu_q = mu / delta if sym else torch.max(mu, zero) / delta                                   # iq.py:208
            c_max = mu_q + (omega / 2 if sym else omega)                                                # iq.py:209
            c_min = (mu_q - omega / 2) if sym else torch.zeros(C)                                       # iq.py:210
            # LIBRARY CHOICE (row WSTART, the first code of the histogram window): the floor of the tensor's smallest clamp
            # bound, each bound clamped to +-1e9 with NaN counting as -1e9, not below -CNNQ_MT_HIST_BINS / 2
            cm = f32(c_min)
            cm = np.clip(np.where(np.isnan(cm), np.float32(-1e9), cm), np.float32(-1e9), np.float32(1e9))
            wstart = max(np.floor(cm.min()), np.float32(-HIST_BINS // 2))
        else:
            # LIBRARY CHOICE: no clamp without clipping (rows CMIN / CMAX hold -inf / +inf), the window is centred on zero
            c_min, c_max = torch.full((C,), -math.inf), torch.full((C,), math.inf)
            wstart = np.float32(-HIST_WINDOW // 2)
    return f32(omega), f32(am), f32(delta), f32(c_min), f32(c_max), np.full(C, wstart, dtype=np.float32)


def with_guess_b(table):
    """The table the <GUESS> launches compute their window start from: row B replaced by std * 0.70710678f."""
    t = torch.from_numpy(f32(table).copy())
    t[STAT_B] = torch.from_numpy(f32(t[STAT_STD]) * SQRT_HALF)
    return t


# ------------------------------------------------------------------------------------------------ the guard
def quotients(std, target):
    """C * 2^target * p / sum p in fp64 (the real-valued omega), or None when the sum is zero or not finite (every omega is then
    0 or NaN whatever the last place of powf is)."""
    with np.errstate(all='ignore'):
        p = np.asarray(f32(std), dtype=np.float64) ** (2. / 3)
        s = p.sum()
        if not (np.isfinite(s) and s > 0):
            return None
        return (p.size * 2. ** float(target)) * p / s


def omega_margin(std, target):
    """The smallest over the channels of |quotient - nearest half-integer| / max(1, quotient); inf when there is nothing to guard.
    A std vector is guarded when this exceeds MARGIN."""
    q = quotients(std, target)
    if q is None:
        return math.inf
    d = np.abs(q - (np.floor(q) + 0.5)) / np.maximum(1., q)
    return float(d.min())


def _ulps(v, k):
    """Positive finite fp32 values moved by k units in the last place (zeros stay)."""
    v = f32(v).copy()
    i = v.view(np.int32)
    i[v > 0] += k
    return v


def omega_moved(std, target, kp, ks):
    """iq.py:128-135 and :187 in fp32 with every p moved by kp ulps and their sum by ks ulps."""
    std = torch.from_numpy(f32(std))
    B = len(std) * (2 ** target)
    p = std ** (2. / 3)
    psum = torch.from_numpy(_ulps(p.sum().reshape(1), ks))
    return f32(((B * torch.from_numpy(_ulps(p, kp))) / psum).round())


# ------------------------------------------------------------------------------------------------ guarded cells
# (C, target) -> seed of guarded_prior: every cell the channel-count test runs.  test_midtread_params_cpu.py asserts for each that
# omega_margin > MARGIN and that omega survives +-4 ulps.  (65, 8) and (65, 9.5) reach omega > 955 by themselves.
CELLS = {
    (1, 4): 0, (1, 5.3): 0, (2, 4): 0, (2, 5.3): 0, (63, 4): 0, (63, 5.3): 1, (64, 4): 0, (64, 5.3): 0,
    (65, 4): 0, (65, 5.3): 0, (65, 8): 5, (65, 9.5): 14,
    (1000, 4): 0, (1000, 5.3): 0, (1024, 4): 0, (1024, 5.3): 2, (1025, 4): 2, (1025, 5.3): 2,
    (4096, 4): 8, (4096, 2): 1, (4097, 4): 8, (4097, 2): 0, (6000, 3): 2, (6000, 2.5): 4,
}
# the cells recorded in tests/golden/midtread_params.npz: C <= 1025, omegas inside the real table
GOLDEN_CELLS = [(1, 4), (2, 5.3), (63, 4), (64, 5.3), (65, 4), (1000, 4), (1025, 4), (1025, 5.3)]


def cells():
    return [(C, t, s) for (C, t), s in CELLS.items()]


def cell_table(C, seed):
    """The guarded prior as STD under ordinary extrema, means of both signs and a Laplace-like b."""
    gen = torch.Generator().manual_seed(1000 + C)
    std = guarded_prior(C, seed)
    mean = torch.randn(C, generator=gen) * 0.2
    b = std * (0.6 + 0.3 * torch.rand(C, generator=gen))
    return make_table(C, mean - 1 - torch.rand(C, generator=gen), mean + 1 + torch.rand(C, generator=gen), mean, std, b)


# the exact tie: both priors are powf(1, y) == 1, B == 5.0f exactly, the quotient is 2.5 -> omega 2 (half to even), not 3
TIE_TARGET = math.log2(2.5)


def tie_table():
    return make_table(2, [-1., -2.], [2., 1.], [.25, -.5], [1., 1.], [.75, .5])


# ------------------------------------------------------------------------------------------------ chosen omegas
def stds_for(omegas):
    """(std [C], target) on which channel c gets omega == omegas[c] (non-negative integers): std = omega^1.5 makes
    the quotient omegas[c] up to the rounding of powf, target = log2(mean omega).  The guard still applies (the CPU test runs it)."""
    w = np.asarray(omegas, dtype=np.float64)
    assert (w >= 0).all() and (w == np.rint(w)).all()
    return torch.from_numpy((w ** 1.5).astype(np.float32)), math.log2(w.sum() / w.size) if w.sum() > 0 else 0.


def segment_of(omega, sym, otab):
    """(i, kind) of iq.py:142 for an integer omega: the index searchsorted gives (ntab: beyond the table) and which case it is."""
    om = float(omega) * (1 if sym else 2)
    i = int(np.searchsorted(otab, om))
    if i >= len(otab):
        return i, 'beyond_last'
    if otab[i] == om:
        return i, 'at_knot'
    return i, 'below_first' if i == 0 else 'between'


def reachable_segments(sym, otab):
    """The indices i of iq.py:142 some integer omega reaches: omega is rounded, so under `sym` a segment (otab[i-1], otab[i]] is
    reachable only if it holds an integer, under the doubled form an even one.  (40 of the real table's 100 segments lie inside
    (0, 0.955] and 11 more hold no integer.)"""
    step = 1 if sym else 2
    return sorted({int(np.searchsorted(otab, float(k))) for k in range(0, int(otab[-1]) + 1, step)})


def omegas_covering(sym, otab):
    """One omega per reachable segment (the smallest), every integer knot, and two beyond the table."""
    step = 1 if sym else 2
    seen, out = set(), []
    for k in range(0, int(otab[-1]) + 1, step):
        i = int(np.searchsorted(otab, float(k)))
        if i not in seen or otab[i] == k:
            seen.add(i)
            out.append(k // step)
    last = int(otab[-1]) // step
    return out + [last + 1, 2 * last + 3]


def interp_table(omegas, seed):
    """Statistics around chosen omegas: means of both signs, b a dyadic fraction of 1."""
    std, target = stds_for(omegas)
    C = std.numel()
    gen = torch.Generator().manual_seed(seed)
    mean = (torch.randint(-8, 9, (C,), generator=gen).float()) / 16
    b = (torch.randint(1, 17, (C,), generator=gen).float()) / 8
    return make_table(C, mean - 2, mean + 3, mean, std, b), target


HAND_A_OMEGAS = [0, 1, 2, 3, 4, 6, 8, 12, 16, 17, 20, 40]           # knots, between, beyond (sym); doubled: 9+ leave the table
HAND_C_OMEGAS = [0, 2, 4, 5, 7, 8, 10]                              # 4: the knot in front of the cliff
HAND_B_OMEGAS = [0, 1, 2, 3, 4, 6, 8, 12, 16, 17, 18, 19, 20, 43]       # below the first knot, first / middle / last segment, beyond


HAND = {'hand_a': (HAND_A, HAND_A_OMEGAS, HAND_A_VALUES), 'hand_b': (HAND_B, HAND_B_OMEGAS, HAND_B_VALUES),
        'hand_c': (HAND_C, HAND_C_OMEGAS, HAND_C_VALUES)}


# ------------------------------------------------------------------------------------------------ edge statistics
# name, omega wanted (None: see std), min, max, mean, std (None: from omega), b: one channel per branch of mt_channel, so a failure
# names the branch.  ORD rows are the ordinary company.
NAN, INF = math.nan, math.inf
ORD_ROWS = [
    ('ord5',          5,  -1.0,    2.0,   0.3,  None, 0.6),
    ('ord9',          9,  -3.0,    1.0,  -0.4,  None, 0.5),
    ('ord2',          2,  -0.5,    4.0,   1.0,  None, 1.25),
]
EDGE_ROWS = [
    ('std0',          0,  -1.0,    2.0,   0.3,  0.0,  0.6),          # omega == 0: Delta = FLT_MAX, both bounds mu / FLT_MAX
    ('b0',            4,  -1.0,    2.0,   0.3,  None, 0.0),          # range 0 -> Delta 0 -> mu / 0
    ('b0_mean0',      4,  -1.0,    2.0,   0.0,  None, 0.0),          # 0 / 0: NaN bounds
    ('mean_neg',      6,  -3.0,    1.0,  -0.7,  None, 0.5),          # non-negative range: mu0 = max(mean, 0) = 0
    ('far_mean',      8, -3001., -2999., -3000., None, 1e-4),        # floor(c_min) far below -65536: the WSTART clamp
    ('huge',          3, -3e38,   3e38,  -3e38, None, 3e38),         # 2 * am * b and max - min overflow
    ('denormal',      2, -1e-40,  2e-40,  1e-40, None, 1e-41),
    ('std_denormal',  0,  -1.0,    2.0,   0.3,  1e-42, 0.6),         # p ~ 1e-28 of the sum: omega 0 through the quotient
    ('nan_mean',      4,  -1.0,    2.0,   NAN,  None, 0.6),          # torch.max(mu, 0) propagates NaN (iq.py:194, :208)
    ('ninf_mean',     4,  -INF,    2.0,  -INF,  None, 0.6),          # a -inf bound
    ('inf_mean',      4,  -1.0,    INF,   INF,  None, 0.6),
    ('nan_b',         4,  -1.0,    2.0,   0.3,  None, NAN),
    ('inf_b',         4,  -1.0,    2.0,   0.3,  None, INF),
    ('nan_min',       4,   NAN,    2.0,   0.3,  None, 0.6),          # clip = 0 reads min / max
    ('inf_max',       4,  -1.0,    INF,   0.3,  None, 0.6),
    ('max_eq_min',    4,   0.7,    0.7,   0.7,  None, 0.2),
]
# std values that change every channel's omega: given to one channel of an ordinary table, and alone at C = 1
POISON_STD = [('std_nan', NAN), ('std_inf', INF), ('std_neg', -0.5), ('std_huge', 3e38)]
EDGE_NAMES = [r[0] for r in ORD_ROWS + EDGE_ROWS]


def rows_table(rows):
    """The table of a list of rows above -> (table, target)."""
    om = [r[1] for r in rows]
    std, target = stds_for(om)
    for c, r in enumerate(rows):
        if r[5] is not None:
            std[c] = r[5]
    cols = list(zip(*[(r[2], r[3], r[4], 0., r[6]) for r in rows]))
    t = make_table(len(rows), *cols)
    t[STAT_STD] = std
    return t, target


def edge_table():
    return rows_table(ORD_ROWS + EDGE_ROWS)


def single_table(row):
    """One row alone at C = 1 (the per-tensor form): omega == 2^target == the row's omega where its std is live."""
    t, _ = rows_table([row])
    if row[5] is None:
        t[STAT_STD] = 1.
    return t, math.log2(max(row[1], 1))


def poison_table(value, where=1):
    """The ordinary rows three times over with one channel's std replaced."""
    t, target = rows_table(ORD_ROWS * 3)
    t[STAT_STD, where] = value
    return t, target


def constant_table(C):
    """Every channel constant: std == 0 everywhere, psum == 0."""
    v = torch.linspace(-1., 2., C) if C > 1 else torch.tensor([0.7])
    return make_table(C, v, v, v, torch.zeros(C), torch.zeros(C))


# ------------------------------------------------------------------------------------------------ WSTART
WSTART_SLOTS = {63: [0, 62], 1025: [0, 63, 64, 1023, 1024], 4097: [0, 63, 64, 1023, 1024, 4096]}


def wstart_table(C, slot, kind='low'):
    """An ordinary guarded table (symmetric bounds around -20 .. 0) in which channel `slot` alone holds the smallest clamp bound:
    'low' - a mean of -1000 b, some hundreds of codes below zero; 'clamp' - floor(c_min) < -65536; 'nan' - a NaN bound; 'ninf' - a -inf bound."""
    seed = CELLS[(C, 4)] if (C, 4) in CELLS else 0
    t = cell_table(C, seed)
    if kind == 'low':
        t[STAT_MEAN, slot] = -1000. * t[STAT_B, slot]
    elif kind == 'clamp':
        t[STAT_MEAN, slot] = -1e6 * t[STAT_B, slot]
    elif kind == 'nan':
        t[STAT_MEAN, slot] = NAN
    elif kind == 'ninf':
        t[STAT_MEAN, slot] = -INF
    return t


# ------------------------------------------------------------------------------------------------ what the GPU test runs
def gpu_tables():
    """name -> (table, target): every statistics table test_midtread_params_gpu.py hands to the kernel; it takes them from here by
    name, and test_midtread_params_cpu.py runs the guard over all of them."""
    out = []
    for C, target, seed in cells():
        out.append((('cell', C, target), cell_table(C, seed), target))
    for nm, tabs, omegas in (('hand_a', HAND_A, HAND_A_OMEGAS), ('hand_b', HAND_B, HAND_B_OMEGAS), ('hand_c', HAND_C, HAND_C_OMEGAS)):
        out.append((nm,) + interp_table(omegas, 3))
    for sym in (True, False):
        out.append((('real', sym),) + interp_table(omegas_covering(sym, real_tables()[0]), 4))
    out.append(('edge',) + edge_table())
    for row in ORD_ROWS + EDGE_ROWS:
        out.append((('single', row[0]),) + single_table(row))
    for nm, v in POISON_STD:
        out.append((('poison', nm),) + poison_table(v))
        out.append((('poison1', nm), make_table(1, -1., 2., .3, v, .6), 4))
    for C in (1, 2, 65, 1025):
        out.append((('constant', C), constant_table(C), 4))
    for C, slots in WSTART_SLOTS.items():
        for slot in slots:
            out.append((('wstart', C, slot), wstart_table(C, slot), 4))
    for kind in ('clamp', 'nan', 'ninf'):
        out.append((('wstart', kind), wstart_table(1025, 700, kind), 4))
    return {o[0]: (o[1], o[2]) for o in out}
