"""The hand-built histograms the entropy kernels are tested on (test_entropy_table_gpu.py imports the case lists from here), and
the conditions on them that need no GPU:

  * the float32 arithmetic of the kernels, restated in numpy (E.entropy32), is within the tier 2e-5 * max(1, H) of the fp64
    entropy of every case - so a device result outside the tier is the device's doing, not the number format's;
  * every mistake E.mutations() knows (a region dropped or counted twice, the window laid one code off, equal clamp values not
    merged, unequal ones merged, 32-bit words) moves the fp64 entropy of every case it applies to by >= 1e-3 * max(1, H), fifty
    tiers - a case in which a region is too small to matter fails here instead of passing on the device;
  * the builder refuses what no producer writes.

Mid-tread cases: C in {1, 31, 33, 512, 2048, 2049, 3000} (2C: below one wave, not a multiple of 64, the cap of k_mt_entropy's LDS
list, one past it, well past it) with clamp hits on the first and the last entry of every wave's segment of that list; equal
clamp values of every kind; the flag clear and raised; the window at -MT_NB/2, -64, 0 and ending at MT_NB/2 - 1 with live bins on
both sides of both its ends; counts beyond 2^32; three placements over the replicas."""
import numpy as np
import pytest

import _entropy as E
from cnn_quantization_amd import _lib

NB, W = E.NB, E.W


# ------------------------------------------------------------------------------------------ mid-tread descriptions
def hit_entries(C):
    """Entries (i < C: cmin[i], else cmax[i - C]) of the 2C clamp counters that get hits: the first and the last entry of every
    wave's segment of k_mt_entropy's compaction (ceil(2C / 1024) * 64 entries per wave), and every 37th in between."""
    n2 = 2 * C
    seg = (n2 + E.ENT_THREADS - 1) // E.ENT_THREADS * 64
    s = set(range(5, n2, 37))
    for w in range(E.ENT_THREADS // 64):
        if w * seg < n2:
            s |= {w * seg, min((w + 1) * seg, n2) - 1}
    return sorted(s)


def bounds(C, scheme, hits):
    """(cmin, cmax, {entry: count}) - all finite, cmin <= cmax.  'different': 2C distinct non-integer values; 'three_cmax': one
    c_max in three channels; 'cross': a c_min of one channel is the c_max of another; 'one': a single value everywhere;
    'integer': integer bounds (no clamp counter can be used)."""
    c = np.arange(C, dtype=np.float32)
    cmin, cmax = -(c + 10.5), c + 10.25
    cnt = {e: 20 + e % 5 for e in hits}
    cnt[hits[0]], cnt[hits[-1]] = 5000, 4500               # (entry 0 and entry 2C - 1: one c_min, one c_max)
    lo = [e for e in hits if e < C]
    hi = [e - C for e in hits if e >= C]
    if scheme == 'three_cmax':
        for ch in (hi[0], hi[len(hi) // 2], hi[-1]):
            cmax[ch] = 7.75
            cnt[C + ch] = max(cnt[C + ch], 900)
    elif scheme == 'cross':
        a, b = lo[0], next(ch for ch in hi if ch != lo[0])
        cmin[a] = cmax[b] = -2.5
        cnt[C + b] = 1700
    elif scheme == 'one':
        cmin[:] = cmax[:] = 2.5
    elif scheme == 'integer':
        cmin, cmax, cnt = -(c + 10), c + 10, {}
    else:
        assert scheme == 'different'
    return cmin, cmax, cnt


def describe(C, wstart, scheme='different', flag=True, zero_global=False):
    hits = hit_entries(C)
    cmin, cmax, cnt = bounds(C, scheme, hits)
    window = {wstart: 4000, wstart + 1: 2500, wstart + 64: 6000, wstart + 100: 1500, wstart + W - 1: 3000}
    glob, below, above = {}, 0, 0
    if flag:
        below, above = 1100, 900
        glob = {k: n for k, n in ((wstart - 1, 3500), (wstart + W, 2500), (-NB // 2, 1200), (NB // 2 - 1, 1300))
                if -NB // 2 <= k < NB // 2 and not wstart <= k < wstart + W}
        if zero_global:
            assert not wstart <= 0 < wstart + W
            glob[0] = 5000
    d = E.MtDesc(C, wstart, cmin, cmax, window, glob, below, above,
                 clo={e: n for e, n in cnt.items() if e < C}, chi={e - C: n for e, n in cnt.items() if e >= C})
    return whole_channels(d)


def whole_channels(d):
    """total a multiple of C (cnnq_midtread_entropy_count takes the elements per channel): the remainder joins a window bin"""
    k = max(d.window, key=d.window.get)
    d.window[k] += -d.total % d.C
    assert d.total % d.C == 0
    return d


def big(C, counts_window, clamp=None):
    cmin, cmax = np.full(C, -3.5, np.float32), np.full(C, 9.5, np.float32) + np.arange(C, dtype=np.float32)
    return E.MtDesc(C, -64, cmin, cmax, counts_window, chi=clamp or {})


MT_CASES = {}               # name -> (description, spread)
for _C in (1, 31, 33, 512, 2048, 2049, 3000):
    MT_CASES['C%d' % _C] = (describe(_C, -64), 'even')
for _C in (33, 2048, 2049):
    for _s in ('three_cmax', 'cross', 'one'):
        MT_CASES['C%d_%s' % (_C, _s)] = (describe(_C, -64, _s), ('random', 11))
MT_CASES['C1_one'] = (describe(1, -64, 'one'), 'even')
MT_CASES['C31_integer_bounds'] = (describe(31, -64, 'integer'), 'even')
MT_CASES['clear_C31'] = (describe(31, -64, flag=False), 'even')
MT_CASES['clear_C2049_cross'] = (describe(2049, -9, 'cross', flag=False), ('random', 5))
MT_CASES['clear_single_bin'] = (E.MtDesc(33, -64, np.full(33, -0.5), np.full(33, 9.5), {5: 33 * 1000}), 'even')
MT_CASES['clear_single_clamp'] = (E.MtDesc(3, 0, np.full(3, 0.), np.full(3, 6.5), chi={0: 100, 1: 100, 2: 100}), 'even')
MT_CASES['window_lowest'] = (describe(33, -NB // 2), 'even')
MT_CASES['window_at_0'] = (describe(33, 0, 'cross'), 'even')
MT_CASES['window_highest'] = (describe(33, NB // 2 - W), 'even')
MT_CASES['window_past_the_table'] = (whole_channels(E.MtDesc(
    4, NB // 2 - 3, np.full(4, -1.5), np.full(4, 1.5), {NB // 2 - 3: 700, NB // 2 - 1: 900}, {NB // 2 - 4: 800, 0: 600}, 300, 500,
    {2: 400}, {3: 450})), 'one')
MT_CASES['zero_in_global_bins'] = (describe(31, 200, zero_global=True), 'even')
MT_CASES['two_symbols_2p33'] = (big(1, {-3: 1 << 33, 40: 1 << 33}), 'one')
MT_CASES['window_and_clamp_2p33'] = (big(2, {0: 1 << 33}, {1: 1 << 33}), 'one')
MT_CASES['mixed_wide_counts'] = (whole_channels(big(
    31, {-64: (1 << 33) + 1234567, 0: (1 << 32) + 3, 1: (1 << 31) + 7, 63: 3 * (1 << 30) + 1, 17: (1 << 28) + 5},
    {0: (1 << 34) + 99, 30: (1 << 29) + 1})), 'one')
MT_CASES['wide_counts_2p40'] = (whole_channels(big(33, {2: 1 << 39, 3: 1 << 38, 4: (1 << 37) + 1}, {7: 1 << 37, 8: 1 << 36})),
                                ('random', 3))
# one description, its window counts in one replica each, spread evenly, spread at random: the same bits on the device
PLACEMENTS = ['placed_one', 'placed_even', 'placed_random']
for _n, _how in zip(PLACEMENTS, ('one', 'even', ('random', 7))):
    MT_CASES[_n] = (describe(512, -64, 'three_cmax'), _how)
MT_NAMES = sorted(MT_CASES)


def window_and_global_forms():
    """The same counts once in the window and once in the global bins (the window moved away and left empty)."""
    codes = {-64: 4000, -1: 300, 0: 9000, 1: 2500, 5: 700, 63: 3000}
    cm, cx = np.full(2, -70.5), np.full(2, 70.25)
    kw = dict(below=1100, above=900, clo={0: 500}, chi={1: 650})
    return (E.MtDesc(2, -64, cm, cx, codes, {-65: 350, 64: 450}, **kw),
            E.MtDesc(2, 4096, cm, cx, {}, {**codes, -65: 350, 64: 450}, **kw))


# ------------------------------------------------------------------------------------------ the uniform quantizers' tables
def ramp(bins):
    """unequal counts on every bin; the last one holds a ninth of the total, so that losing it shows at any table size"""
    c = {int(k): 100 + (37 * int(k)) % 61 for k in bins}
    if len(c) > 1:
        c[max(c)] = sum(c.values()) // 8
    return c


PLAIN_CASES = {}            # name -> ({bin: count}, nbins): cnnq_entropy
for _nb in (1, 2, 16, 255, 256, 257, 1000, 5000):
    PLAIN_CASES['ramp_%d' % _nb] = (ramp(range(_nb)), _nb)
    PLAIN_CASES['ends_%d' % _nb] = ({0: 300, _nb - 1: 500} if _nb > 1 else {0: 300}, _nb)
    PLAIN_CASES['empty_%d' % _nb] = ({}, _nb)
for _k in range(9):
    PLAIN_CASES['pow2_%d_of_256' % _k] = ({b * (256 >> _k): 1000 for b in range(1 << _k)}, 256)
PLAIN_CASES['pow2_12_of_5000'] = ({b + 450: 77 for b in range(4096)}, 5000)
PLAIN_CASES['two_bins_2p33'] = ({3: 1 << 33, 200: 1 << 33}, 256)
PLAIN_CASES['mixed_wide_counts'] = ({0: (1 << 33) + 1234567, 5: (1 << 32) + 3, 255: (1 << 34) + 99, 256: (1 << 29) + 1,
                                     999: 3 * (1 << 30) + 1}, 1000)
PLAIN_NAMES = sorted(PLAIN_CASES)
POW2_TOL = 1e-6
POW2 = {n: int(n.split('_')[1]) for n in PLAIN_NAMES if n.startswith('pow2_')}

REPLICA_CASES = {}          # name -> ({bin: count}, spread): cnnq_entropy_replicas[_batch], cnnq_hist_replicas_fold
for _live in (16, 256):
    for _how in ('one', 'even', ('random', 21)):
        REPLICA_CASES['ramp_%d_%s' % (_live, _how if isinstance(_how, str) else _how[0])] = (ramp(range(_live)), _how)
for _k in (0, 4, 8):
    REPLICA_CASES['pow2_%d' % _k] = ({b * (256 >> _k): 64 * 1000 for b in range(1 << _k)}, ('random', _k))
REPLICA_CASES['empty'] = ({}, 'even')
REPLICA_CASES['two_bins_2p33_one'] = ({3: 1 << 33, 255: 1 << 33}, 'one')
REPLICA_CASES['two_bins_2p33_even'] = ({3: 1 << 33, 255: 1 << 33}, 'even')
REPLICA_CASES['mixed_wide_counts'] = ({0: (1 << 33) + 1234567, 5: (1 << 32) + 3, 254: (1 << 34) + 99, 255: (1 << 29) + 1}, 'one')
REPLICA_NAMES = sorted(REPLICA_CASES)


def mt_reference(name):
    d, _ = MT_CASES[name]
    return E.entropy64(E.symbols(d), d.total)


def table_reference(counts):
    return E.entropy64(counts.values(), sum(counts.values()))


# ------------------------------------------------------------------------------------------ the tests
def test_the_layout_constants_are_the_library_s():
    assert (NB, W, E.GR, E.NMT) == (_lib.MT_HIST_BINS, _lib.MT_HIST_WINDOW, _lib.MT_HIST_REPLICAS, _lib.NMT)
    assert (E.MT_CMIN, E.MT_CMAX, E.MT_WSTART) == (_lib.MT_CMIN, _lib.MT_CMAX, _lib.MT_WSTART)
    assert all(E.mt_hist_words(C) == _lib.mt_hist_words(C) for C in (1, 33, 3000))


def test_the_case_list_covers_what_it_claims():
    Cs = {d.C for d, _ in MT_CASES.values()}
    assert {1, 31, 33, 512, 2048, 2049, 3000} <= Cs
    assert {d.wstart for d, _ in MT_CASES.values()} >= {-NB // 2, -64, 0, NB // 2 - W}
    for C in (1, 31, 33, 512, 2048, 2049, 3000):
        d, _ = MT_CASES['C%d' % C]
        live = set(d.clo) | {C + c for c in d.chi}
        seg = (2 * C + 1023) // 1024 * 64
        assert all({w * seg, min((w + 1) * seg, 2 * C) - 1} <= live for w in range(16) if w * seg < 2 * C)
        assert len(live) < 2 * C or C == 1                     # scattered, not everywhere
    for n in ('window_lowest', 'window_at_0', 'window_highest', 'C33'):
        d, _ = MT_CASES[n]
        assert d.flag and d.below and d.above and d.wstart in d.window
        assert d.wstart + W - 1 in d.window
        assert (d.wstart - 1 in d.glob or d.wstart == -NB // 2) and (d.wstart + W in d.glob or d.wstart + W == NB // 2)
    d, _ = MT_CASES['zero_in_global_bins']
    assert 0 in d.glob
    assert max(max(d.window.values(), default=0) for d, _ in MT_CASES.values()) >= 1 << 39


@pytest.mark.parametrize('name', MT_NAMES)
def test_every_region_of_a_mid_tread_case_weighs_a_percent(name):
    d, _ = MT_CASES[name]
    for r in d.REGIONS:
        assert d.region_total(r) == 0 or d.region_total(r) * 100 >= d.total, r
    assert d.total % d.C == 0


@pytest.mark.parametrize('name', MT_NAMES)
def test_mid_tread_float32_arithmetic_is_within_the_tier(name):
    d, spread = MT_CASES[name]
    h64, h32 = mt_reference(name), E.entropy32(E.symbols(d), d.total)
    print('%-26s H64 %.9f  |H32 - H64| %.3g  tier %.3g' % (name, h64, abs(h32 - h64), E.tier(h64)))
    assert abs(h32 - h64) <= E.tier(h64)
    words = E.mt_words(d, spread)
    assert E.entropy64(E.symbols_of_words(words, d), d.total) == pytest.approx(h64, abs=1e-12)     # layout and symbols agree


@pytest.mark.parametrize('name', MT_NAMES)
def test_every_mutation_moves_a_mid_tread_case(name):
    d, spread = MT_CASES[name]
    h64 = mt_reference(name)
    muts = E.mutations(d, spread)
    assert muts
    for m, counts in muts.items():
        moved = abs(E.entropy64(counts, d.total) - h64)
        print('%-26s %-14s moves H by %.4g (needs %.3g)' % (name, m, moved, E.MOVE * max(1., h64)))
        assert moved >= E.MOVE * max(1., h64), m


def test_the_applicable_mutations_are_the_expected_ones():
    m = set(E.mutations(*MT_CASES['C33_cross']))
    assert {'shift_-1', 'shift_+1', 'no_merge', 'merge_unequal', 'drop_window', 'twice_chi', 'drop_below'} <= m and 'low32' not in m
    assert 'low32' in E.mutations(*MT_CASES['two_symbols_2p33']) and 'low32' in E.mutations(*MT_CASES['wide_counts_2p40'])
    m = set(E.mutations(*MT_CASES['clear_C31']))
    assert 'shift_+1' not in m and 'drop_glob' not in m and 'no_merge' not in m and 'merge_unequal' in m
    assert 'no_merge' in E.mutations(*MT_CASES['C2049_one']) and 'merge_unequal' not in E.mutations(*MT_CASES['C2049_one'])


def test_known_entropies():
    assert mt_reference('clear_single_bin') == 0. and mt_reference('clear_single_clamp') == 0.
    assert mt_reference('two_symbols_2p33') == 1. and mt_reference('window_and_clamp_2p33') == 1.
    for n, k in POW2.items():
        assert table_reference(PLAIN_CASES[n][0]) == float(k)
    a, b = window_and_global_forms()
    assert sorted(E.symbols(a)) == sorted(E.symbols(b)) and a.total == b.total


def test_the_three_placements_are_one_description():
    words = [E.mt_words(*MT_CASES[n]) for n in PLACEMENTS]
    regs = [E.mt_regions(w, 512) for w in words]
    assert all(np.array_equal(r['win'], regs[0]['win']) for r in regs)
    assert not np.array_equal(regs[0]['rep'], regs[1]['rep']) and not np.array_equal(regs[1]['rep'], regs[2]['rep'])
    assert ((regs[0]['rep'] != 0).sum(0) <= 1).all() and (regs[1]['rep'] != 0).sum() > (regs[2]['rep'] != 0).sum()
    assert all(np.array_equal(w[:NB + 2 + 1024], words[0][:NB + 2 + 1024]) for w in words)


def test_the_builder_refuses_what_no_producer_writes():
    cm, cx = np.full(2, -3.5, np.float32), np.array([4.5, 6.], np.float32)
    ok = E.MtDesc(2, -64, cm, cx, {0: 5}, {100: 2}, chi={0: 1})
    assert E.mt_words(ok)[-1] != 0 and E.mt_words(E.MtDesc(2, -64, cm, cx, {0: 5}))[-1] == 0
    for kw in (dict(window={64: 1}),                               # not in the window
               dict(glob={0: 1}),                                  # in the window: never in the global bins
               dict(glob={NB // 2: 1}),                            # no such bin: that is the above-range word
               dict(chi={1: 1}),                                   # an integer bound has no counter
               dict(clo={2: 1}),                                   # no such channel
               dict(window={0: 0})):
        with pytest.raises(AssertionError):
            E.MtDesc(2, -64, cm, cx, **kw)
    with pytest.raises(AssertionError):
        E.MtDesc(2, NB // 2 - 3, cm, cx, {NB // 2: 1})             # a window bin past the last integer code is not used
    with pytest.raises(AssertionError):
        E.MtDesc(2, -NB // 2 - 1, cm, cx)


@pytest.mark.parametrize('name', PLAIN_NAMES)
def test_plain_tables(name):
    counts, nbins = PLAIN_CASES[name]
    check_table(name, counts, E.plain_table(counts, nbins).reshape(1, -1))


@pytest.mark.parametrize('name', REPLICA_NAMES)
def test_replica_tables(name):
    counts, spread = REPLICA_CASES[name]
    check_table(name, counts, E.replica_tables(counts, spread))


def check_table(name, counts, table):
    total = sum(counts.values())
    assert table.sum() == total and all(int(table[:, k].sum()) == c for k, c in counts.items())
    h64 = table_reference(counts)
    assert abs(E.entropy32(counts.values(), total) - h64) <= E.tier(h64)
    # the uniform tables over 2^k bins are held to |H - k| <= POW2_TOL on the device: fifty times THAT is what a mutation must move
    need = 50 * POW2_TOL if name.startswith('pow2_') else E.MOVE * max(1., h64)
    for m, c in E.table_mutations(counts).items():
        assert abs(E.entropy64(c, total) - h64) >= need, (name, m)


def test_spreading_keeps_the_sum():
    for count in (0, 1, 63, 64, 65, 12345, (1 << 33) + 5, 1 << 40):
        for how in ('one', 'even', ('random', 1), ('random', 2)):
            for n in (E.XREP, E.GR):
                assert int(E.spread_count(count, n, how).sum()) == count
