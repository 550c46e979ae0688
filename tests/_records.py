"""The record-merge kernels of csrc/cnnq_stats.hip.h (k_combine, k_combine_dev, k_combine_all; merge_moments / merge_sums /
merge_dev, mean_of, std_of, b_of) restated on the CPU, and the hand-built records that make their tests exact - helper, no tests.

The library is built with -ffp-contract=off, fp64 add / mul / div / sqrt are correctly rounded on both sides, and the order of
the additions is fixed by mseg_of(G, C): merge_col / combine_ref / combine_dev_ref are therefore the kernels' results bit for
bit, and nothing here takes a tolerance.  What the formulas are the reference's (smpc.py:45-79: mean, unbiased std, std of the
rectified values, mean |x - mean|, kurtosis) is pinned in test_records_cpu.py; every line that is this library's own choice and
not the reference's is marked LIBRARY CHOICE."""
import numpy as np

from _params import first_diff as first_diff32, same_bits as same_bits32  # noqa: F401

F64, F32 = np.float64, np.float32
MOM_MIN, MOM_MAX, MOM_SUM, MOM_SUMSQ, MOM_COUNT, MOM_SUM_RELU, MOM_SUMSQ_RELU, NMOM = 0, 1, 2, 3, 4, 5, 6, 7   # pinned to _lib
STAT_MIN, STAT_MAX, STAT_MEAN, STAT_STD, STAT_B, STAT_KURT, STAT_STD_POS, NSTAT = 0, 1, 2, 3, 4, 5, 6, 7      # in the CPU test
DEV_ABS, DEV_Z4, NDEV = 0, 1, 2
SEGS = (1, 8, 64)
TPB = 256
INF, NAN = float('inf'), float('nan')
EMPTY = np.array([INF, -INF, 0., 0., 0., 0., 0.])            # the record of a shard that holds no sample


def mseg_of(G, C):
    """lanes per channel of the merge kernels - the constexpr rule of cnnq_stats.hip.h, copied"""
    return (1 if G <= 16 else 8) if (G <= 64 and C >= 512) else 64


# ------------------------------------------------------------------------------------------ comparisons
def same_bits64(a, b):
    """fp64 arrays equal bit for bit where neither is NaN, and NaN in the same places (a NaN's sign and payload are not pinned)"""
    a, b = np.ascontiguousarray(a, dtype=F64), np.ascontiguousarray(b, dtype=F64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb]))


def first_diff(a, b):
    """(index, got, expected) of the first element on which same_bits64 / same_bits32 fails, for messages"""
    a, b = np.asarray(a), np.asarray(b)
    bits = np.uint32 if a.dtype == np.float32 else np.uint64
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b, dtype=a.dtype)
    na, nb = np.isnan(a), np.isnan(b)
    bad = (na != nb) | (~na & ~nb & (a.view(bits) != b.view(bits)))
    idx = np.argwhere(bad)
    if not len(idx):
        return None
    i = tuple(int(v) for v in idx[0])
    return i, float(a[i]), float(b[i])


# ------------------------------------------------------------------------------------------ the merge
def pmind(a, b):
    """as written in cnnq_common.hip.h: (a < b || a != a) ? a : b - a NaN on either side comes out, a tie takes b"""
    return np.where((a < b) | (a != a), a, b)


def pmaxd(a, b):
    return np.where((a > b) | (a != a), a, b)


def tree_masks(seg, ascending=False):
    m = [seg >> k for k in range(1, seg.bit_length())]
    return m[::-1] if ascending else m


def merge_col(part, seg, rows_min=(MOM_MIN,), rows_max=(MOM_MAX,), skip=(), ascending=False):
    """merge_moments_seg (and, with no extremum rows, merge_dev_seg / merge_sums_seg) for all channels at once.
    part [G, K, C] float64 -> [K, C]: lane j of `seg` starts from (+inf, -inf, 0...) and takes records j, j + seg, ... in
    ascending order; then the xor tree runs with masks seg/2 ... 1 (`ascending`: 1 ... seg/2, the order the kernels do NOT
    use); lane 0 holds the result.  Rows in `skip` are not read and stay 0.
    LIBRARY CHOICE: the lane order - the reference sums a channel's elements in one torch reduction."""
    part = np.asarray(part, dtype=F64)
    G, K, C = part.shape
    acc = np.zeros((K, seg, C), dtype=F64)
    for r in rows_min:
        acc[r] = INF
    for r in rows_max:
        acc[r] = -INF
    live = [r for r in range(K) if r not in skip]
    with np.errstate(all='ignore'):
        for g0 in range(0, G, seg):
            n = min(seg, G - g0)
            rec = part[g0:g0 + n]                                   # lanes 0 .. n-1 take one record each
            for r in live:
                if r in rows_min:
                    acc[r, :n] = pmind(acc[r, :n], rec[:, r])
                elif r in rows_max:
                    acc[r, :n] = pmaxd(acc[r, :n], rec[:, r])
                else:
                    acc[r, :n] = acc[r, :n] + rec[:, r]
        lanes = np.arange(seg)
        for m in tree_masks(seg, ascending):
            for r in range(K):                                      # every row takes part in the shuffles, the skipped ones as 0 + 0
                other = acc[r][lanes ^ m]
                if r in rows_min:
                    acc[r] = pmind(acc[r], other)
                elif r in rows_max:
                    acc[r] = pmaxd(acc[r], other)
                else:
                    acc[r] = acc[r] + other
    return acc[:, 0].copy()


def _std(ss, s, cnt):
    """std_of: the unbiased standard deviation from the merged sums, float64 throughout, one rounding to float32"""
    with np.errstate(all='ignore'):
        mean = s / cnt
        var = (ss - s * mean) / (cnt - 1.)
        var = np.where(var < 0., 0., var)           # LIBRARY CHOICE: the clamp, written as `if (var < 0) var = 0` - a NaN passes
        return np.sqrt(var).astype(F32)


def combine_ref(part, has_relu, seg=None, ascending=False):
    """k_combine: part [G, NMOM, C] -> (mom [NMOM, C] float64, stats [NSTAT, C] float32)"""
    part = np.asarray(part, dtype=F64)
    G, K, C = part.shape
    assert K == NMOM
    seg = mseg_of(G, C) if seg is None else seg
    # LIBRARY CHOICE: without has_relu the rectified rows are not read; mom's are 0 and so is STD_POS
    mom = merge_col(part, seg, skip=() if has_relu else (MOM_SUM_RELU, MOM_SUMSQ_RELU), ascending=ascending)
    stats = np.zeros((NSTAT, C), dtype=F32)         # LIBRARY CHOICE: B and KURT are written as +0 (k_combine_dev fills them in)
    with np.errstate(all='ignore'):
        stats[STAT_MIN], stats[STAT_MAX] = mom[MOM_MIN].astype(F32), mom[MOM_MAX].astype(F32)
        stats[STAT_MEAN] = (mom[MOM_SUM] / mom[MOM_COUNT]).astype(F32)
        stats[STAT_STD] = _std(mom[MOM_SUMSQ], mom[MOM_SUM], mom[MOM_COUNT])
        if has_relu:
            stats[STAT_STD_POS] = _std(mom[MOM_SUMSQ_RELU], mom[MOM_SUM_RELU], mom[MOM_COUNT])
    return mom, stats


def combine_dev_ref(part2, mom, want_kurt, stats_in, seg=None):
    """k_combine_dev: part2 [G, NDEV, C], the COUNT row of mom -> (dev [NDEV, C] float64, stats: stats_in with B - and, want_kurt,
    KURT - replaced; every other row as it was)"""
    part2 = np.asarray(part2, dtype=F64)
    G, K, C = part2.shape
    assert K == NDEV
    seg = mseg_of(G, C) if seg is None else seg
    dev = merge_col(part2, seg, rows_min=(), rows_max=())
    stats = np.array(stats_in, dtype=F32, copy=True)
    cnt = np.asarray(mom, dtype=F64)[MOM_COUNT]
    with np.errstate(all='ignore'):
        stats[STAT_B] = (dev[DEV_ABS] / cnt).astype(F32)
        if want_kurt:
            stats[STAT_KURT] = (dev[DEV_Z4] / cnt - 3.).astype(F32)
    return dev, stats


def two_level_ref(part, W, has_relu):
    """the sharded route: the G records in W consecutive groups, each merged on its own; the W merged records [W, NMOM, C] - what
    all_gather_records lays out - merged again"""
    groups = np.array_split(np.arange(part.shape[0]), W)
    moms = np.stack([combine_ref(part[g], has_relu)[0] for g in groups])
    return moms, combine_ref(moms, has_relu)


# ------------------------------------------------------------------------------------------ hand-built pass-A records
def integer_records(G, C):
    """part [G, NMOM, C] of integers below 2^21 that tell (g, row, c) apart from their neighbours in every direction: any order
    of addition is exact, so a wrong row, channel or record, a skipped record and a double count all show, whatever the order.
    MIN is negative, MAX positive, COUNT a positive integer."""
    g, r, c = np.meshgrid(np.arange(G), np.arange(NMOM), np.arange(C), indexing='ij')
    part = ((g * 257 + c * 19 + r * 7) % 1999 + r + 1).astype(F64)
    part[:, MOM_MIN] = -part[:, MOM_MIN]
    return part


def integer_channel(G, ch):
    """[G, NMOM]: channel ch of integer_records(G, C), any C > ch"""
    g, r = np.meshgrid(np.arange(G), np.arange(NMOM), indexing='ij')
    col = ((g * 257 + ch * 19 + r * 7) % 1999 + r + 1).astype(F64)
    col[:, MOM_MIN] = -col[:, MOM_MIN]
    return col


def extremum_record(G, C, seg=None):
    """[C]: the record that holds channel c's extrema in ordered_records - record 0, the last record, a lane's second record
    (g >= seg, where there is one) and one that walks through all of them, in turn"""
    seg = mseg_of(G, C) if seg is None else seg
    c = np.arange(C)
    second = seg if seg < G else G // 2
    return np.choose(c % 4, [np.zeros(C, dtype=np.int64), np.full(C, G - 1), np.full(C, second), (c * 7 + 3) % G])


def _scaled(rng, G, C):
    """draws [G, C] words |randn| * 2^k or randn * 2^k with the exponents of ordered_records"""
    kind = np.arange(C) % 4
    base = np.where(kind == 0, rng.integers(-20, 37, size=C), rng.integers(-20, 25, size=C))
    heavy = 12 * ((np.arange(G) % 8 == 0)[:, None] & ((kind == 1) | (kind == 2))[None, :])

    def scaled(absolute):
        v = rng.standard_normal((G, C))
        k = np.where(kind == 3, rng.integers(-20, 40, size=(G, C)), base + heavy + rng.integers(0, 4, size=(G, C)))
        return (np.abs(v) if absolute else v) * 2. ** k
    return scaled


def ordered_records(G, C, seed):
    """part [G, NMOM, C] whose sums depend on the order of addition in their last bits: the SUM rows hold |randn| or randn times
    2^k, k in [-20, 40).  By channel modulo 4: 3 - k uniform per word; 0 - k within four octaves of a base the channel draws,
    so every record reaches the last bits of the sum; 1, 2 - the same with the records g = 0, 8, 16, ... twelve octaves above
    the others: those are the records the lane layouts arrange differently (with G = 17, 8 and 64 lanes differ in the place of
    ONE addition, r0 + r8 + r16), and the lighter records behind them do not round the difference away.
    The squares rows lie above s^2 / cnt record by record, so the merged variance is positive (Cauchy-Schwarz) and the STD rows
    carry information.  Counts are ordinary integers; the extrema are float32 values, and channel c's lie in record
    extremum_record(G, C)[c]."""
    rng = np.random.default_rng(seed)
    scaled = _scaled(rng, G, C)
    part = np.empty((G, NMOM, C), dtype=F64)
    cnt = rng.integers(1, 5000, size=(G, C)).astype(F64)
    s, rs = scaled(False), scaled(True)
    part[:, MOM_COUNT] = cnt
    part[:, MOM_SUM], part[:, MOM_SUM_RELU] = s, rs
    part[:, MOM_SUMSQ] = s * s / cnt * (1. + np.abs(rng.standard_normal((G, C)))) + scaled(True)
    part[:, MOM_SUMSQ_RELU] = rs * rs / cnt * (1. + np.abs(rng.standard_normal((G, C)))) + scaled(True)
    part[:, MOM_MIN] = (-np.abs(rng.standard_normal((G, C))) * 3 - 0.5).astype(F32)
    part[:, MOM_MAX] = (np.abs(rng.standard_normal((G, C))) * 3 + 0.5).astype(F32)
    ext = extremum_record(G, C)
    c = np.arange(C)
    part[ext, MOM_MIN, c] = F32(-100.) - (c % 13).astype(F32) / F32(8)
    part[ext, MOM_MAX, c] = F32(100.) + (c % 17).astype(F32) / F32(8)
    return part


# Named channels.  (total s, total ss, total count, quantum of s, quantum of ss): records 1 .. G-1 hold small integer multiples of
# the quantum (every partial sum stays a multiple of it below 2^53 quanta: any order of addition is exact), record 0 what is left
# of the total - so every record still differs from its neighbours, and the merged sums are the totals EXACTLY.  The rectified
# rows repeat the raw ones, so STD_POS meets the same edges.
def _constant_sums(n=196):
    """the sums of n samples of f32(0.1) accumulated as Mom::add does: s += d; ss = fma(d, d, ss) - d * d is exact in float64 (48
    bits), so the fused form is plain ss + d * d here"""
    d = F64(F32(0.1))
    s = ss = F64(0.)
    for _ in range(n):
        s = s + d
        ss = ss + d * d
    return float(s), float(ss), float(n)


CONSTANT = _constant_sums()
TOTALS = {
    'count_one': (2.5, 6.25, 1., .25, .25),                                     # STD NaN (0 / 0, what torch.std gives), MEAN 2.5
    'count_two': (3., 5., 2., 1., 1.),                                          # STD f32(sqrt(0.5))
    'negative_variance': (3., float(np.nextafter(3., 0.)), 3., 1., 2. ** -51),  # var -2.2e-16: STD +0.0, not NaN
    'constant': CONSTANT + (2. ** -27, 2. ** -52),                              # var -4e-17: STD +0.0
    'mean_tie': (4. * (1. + 2. ** -24), 5., 4., 2. ** -22, 1.),                 # MEAN 1.0: the tie goes to even, down
    'mean_tie_up': (4. * (1. + 3 * 2. ** -24), 5., 4., 2. ** -22, 1.),          # MEAN 1 + 2^-22: the tie goes to even, up
    'count_2p24_plus_1': (2. ** 24, 2. ** 24, 2. ** 24 + 1, 1., 1.),            # MEAN f32(2^24 / (2^24 + 1)): divided in float64
    'huge': (0., 1e300, 10., 1., float(np.spacing(1e300))),                     # STD +inf in float32, finite in float64
}
# channels built record by record (with_named): the other nine rows of the issue's table
SPECIAL = ('empty_among_full', 'all_empty', 'nan_record', 'inf_extrema', 'signed_zero')
NAMES = tuple(TOTALS) + SPECIAL


def _spread(total, quantum, G, ch, row):
    """[G]: small integer multiples of `quantum` in records 1 .. G-1 (a pattern of g, the channel and the row, -5 .. 5), record 0
    what is left of `total`"""
    g = np.arange(G)
    v = (((g * 7 + ch * 3 + row * 5) % 11) - 5).astype(F64) * quantum
    v[0] = total - v[1:].sum()
    return v


def named_record_index(G, ch, rot):
    """the record a named channel's single special record sits in: it rotates with the channel and with rot"""
    return (ch * 5 + rot * 3 + 1) % G


def empty_positions(G, ch, rot):
    """the records of `empty_among_full` that are empty: every third one, from an offset that rotates, never all of them"""
    idx = np.arange(G)
    empty = (idx + ch + rot) % 3 == 0
    if empty.all():
        empty[:] = False
    return empty


def with_named(part, rot=0):
    """a copy of part [G, NMOM, C] with the named channels written over channels 0 .. and - C > 2 * len(NAMES) - over the last
    channels too, the names rotated by rot; {channel: name}.  `empty_among_full` needs a second record: with G == 1 the channel
    stays ordinary."""
    part = np.array(part, dtype=F64, copy=True)
    G, _, C = part.shape
    n = len(NAMES)
    chans = list(range(min(C, n))) + (list(range(C - n, C)) if C > 2 * n else [])
    named = {}
    for i, ch in enumerate(chans):
        name = NAMES[(i + rot) % n]
        k = named_record_index(G, ch, rot)
        if name in TOTALS:
            s, ss, cnt, qs, qss = TOTALS[name]
            part[:, MOM_SUM, ch] = part[:, MOM_SUM_RELU, ch] = _spread(s, qs, G, ch, MOM_SUM)
            part[:, MOM_SUMSQ, ch] = part[:, MOM_SUMSQ_RELU, ch] = _spread(ss, qss, G, ch, MOM_SUMSQ)
            part[:, MOM_COUNT, ch] = _spread(cnt, 1., G, ch, MOM_COUNT)
        elif name == 'empty_among_full':
            if G == 1:
                continue
            part[:, :, ch] = integer_channel(G, ch)           # integers: removing records changes no rounding
            part[empty_positions(G, ch, rot), :, ch] = EMPTY
        elif name == 'all_empty':
            part[:, :, ch] = EMPTY
        elif name == 'nan_record':
            part[:, :, ch] = integer_channel(G, ch)
            part[k, [MOM_MIN, MOM_MAX, MOM_SUM, MOM_SUMSQ], ch] = NAN
        elif name == 'inf_extrema':
            part[:, :, ch] = integer_channel(G, ch)
            part[k, [MOM_MAX, MOM_SUM, MOM_SUMSQ], ch] = INF
        elif name == 'signed_zero':
            part[:, :, ch] = integer_channel(G, ch)
            part[:, MOM_MIN, ch] = np.abs(part[:, MOM_MIN, ch])             # every other minimum is positive ...
            part[:, MOM_MAX, ch] = -np.abs(part[:, MOM_MAX, ch])            # ... and every other maximum negative
            part[k, MOM_MIN, ch], part[k, MOM_MAX, ch] = 0., -0.
            part[(k + 1) % G, MOM_MIN, ch], part[(k + 1) % G, MOM_MAX, ch] = -0., 0.    # (G == 1: the second pair alone)
        named[ch] = name
    return part, named


def empty_twin(part, ch):
    """the channel `ch` of part as a table of its own, [G', NMOM, 1], with the empty records REMOVED (G' < G: the twin cannot be
    a channel of the same table)"""
    col = part[:, :, ch:ch + 1]
    full = ~((col[:, MOM_COUNT, 0] == 0) & (col[:, MOM_MIN, 0] == INF) & (col[:, MOM_MAX, 0] == -INF))
    return np.ascontiguousarray(col[full])


# ------------------------------------------------------------------------------------------ hand-built pass-B records
DEV_NAMES = ('count_zero', 'z4_nan_without_kurt', 'kurt_minus_3', 'count_zero_sum_zero')


def dev_records(G, C, seed, rot=0):
    """(part2 [G, NDEV, C], mom [NMOM, C], {channel: name}): order-sensitive sums (|randn| * 2^k, the exponents of
    ordered_records) in three channels of four, integers in the fourth; of mom only the COUNT row is read - the others hold NaN.  Named channels over 0 .. and the last ones:
    count_zero - count 0, the sums positive: B = sa / 0 = +inf; count_zero_sum_zero - 0 / 0;
    z4_nan_without_kurt - a NaN in one record's Z4 word: B stays finite and exact whatever want_kurt;
    kurt_minus_3 - the Z4 words all zero: KURT = -3."""
    rng = np.random.default_rng(seed)
    scaled = _scaled(rng, G, C)
    part2 = np.stack([scaled(True), scaled(True)], axis=1)
    g, r, c = np.meshgrid(np.arange(G), np.arange(NDEV), np.arange(C), indexing='ij')
    ints = ((g * 257 + c * 19 + r * 7) % 1999 + r + 1).astype(F64)
    part2[:, :, 3::4] = ints[:, :, 3::4]
    mom = np.full((NMOM, C), NAN, dtype=F64)
    mom[MOM_COUNT] = rng.integers(2, 1 << 20, size=C).astype(F64)
    n = len(DEV_NAMES)
    chans = list(range(min(C, n))) + (list(range(C - n, C)) if C > 2 * n else [])
    named = {}
    for i, ch in enumerate(chans):
        name = DEV_NAMES[(i + rot) % n]
        named[ch] = name
        part2[:, :, ch] = ints[:, :, ch]
        if name == 'count_zero':
            mom[MOM_COUNT, ch] = 0.
        elif name == 'count_zero_sum_zero':
            mom[MOM_COUNT, ch] = 0.
            part2[:, :, ch] = 0.
        elif name == 'z4_nan_without_kurt':
            part2[named_record_index(G, ch, rot), DEV_Z4, ch] = NAN
        elif name == 'kurt_minus_3':
            part2[:, DEV_Z4, ch] = 0.
    return part2, mom, named


# ------------------------------------------------------------------------------------------ the cases of the GPU test
GRID_G = (1, 2, 3, 15, 16, 17, 63, 64, 65, 130, 256)
GRID_C = (1, 3, 4, 5, 63, 64, 65, 511, 512, 513, 767, 1031)   # 767: the one size short by one at 256 channels per workgroup
ROTATIONS = (0, 7)                              # with 13 names: every name lands on a first and on a last channel of C = 1031
TWO_LEVEL_W = (2, 3, 8)
ORDER_MIN_CHANNELS = 8


def ordered_seed(G, C):
    return 1000 * G + C


def alternatives(G, C):
    """[(seg, ascending)]: the orders of addition a slip in the kernels could take instead of (mseg_of(G, C), descending tree) -
    the other two lane counts, and the tree run with ascending masks.  Left out are the two that are the SAME order, term for
    term: one lane has no tree to reverse; and with G <= 16 eight lanes hold records j and j + 8 and finish with masks 4, 2, 1,
    which is what the last four steps of the 64-lane tree do with one record per lane (the steps 32 and 16 add zeros)."""
    own = mseg_of(G, C)
    alts = [(s, False) for s in SEGS if s != own and not (G <= 16 and {s, own} == {8, 64})]
    if own > 1:
        alts.append((own, True))
    return alts


def order_sensitive_channels(part, G, C, seg, ascending):
    """the number of channels whose merged SUM or SUMSQ changes in its bits when (seg, ascending) replaces the kernels' order"""
    rows = [MOM_SUM, MOM_SUMSQ]
    own = merge_col(part[:, rows], mseg_of(G, C), rows_min=(), rows_max=())
    alt = merge_col(part[:, rows], seg, rows_min=(), rows_max=(), ascending=ascending)
    return int(((own.view(np.uint64) != alt.view(np.uint64)).any(0)).sum())
