"""Hand-built code histograms for the entropy kernels (k_entropy, k_entropy_replicas, k_hist_replicas_fold, k_mt_entropy,
k_mt_entropy_batch) and what their entropy is - helper, no tests.

A mid-tread histogram is DESCRIBED by region (MtDesc): window codes, integer codes outside the window, the two out-of-range
words, the per-channel clamp counters, and the three rows of mt[CNNQ_NMT][C] the kernels read.  mt_words() lays a description
out as include/cnnq_hip.h documents CNNQ_MT_HIST_WORDS(C) and refuses what no producer can write; symbols() lists the counts of
its distinct symbols without going through the words, so the reference does not share the layout arithmetic with the kernel.
entropy64 is utils/entropy.py:6-17 in fp64 on those counts, entropy32 the kernels' float32 arithmetic in numpy.  mutations()
restates a description the way a plausible mistake in a consumer would read it; test_entropy_table_cpu.py demands that each moves
the entropy far beyond the tier, so that a case cannot pass on the device by having nothing at stake."""
import copy

import numpy as np

NB, W, GR = 131072, 128, 256                   # CNNQ_MT_HIST_BINS, _WINDOW, _REPLICAS (pinned to _lib in the CPU test)
MT_DELTA, MT_CMIN, MT_CMAX, MT_OMEGA, MT_ALPHA, MT_WSTART, NMT = 0, 1, 2, 3, 4, 5, 6
XREP, XBINS = 64, 256                          # the replica tables of the uniform quantizers: cnnq_hist_replica_bytes() / 8 words
ENT_THREADS, ENT_LIST = 1024, 4096             # k_mt_entropy: threads of its workgroup, entries of its LDS clamp-value list

TIER = 2e-5                                    # |H - H64| <= TIER * max(1, H64): test_entropy_batch_gpu.py's against the golden entropies
MOVE = 1e-3                                    # what every mutation must move H64 by, same scale: 50 tiers


def tier(h):
    return TIER * max(1., h)


def mt_hist_words(C):
    return NB + 2 + 2 * C + GR * W + 1


class MtDesc:
    """One mid-tread code histogram by region.  cmin / cmax: float32 [C]; window / glob: {integer code: count}; below / above: the
    counts of the out-of-range words; clo / chi: {channel: count} of the elements clamped to cmin[c] / cmax[c]."""

    def __init__(self, C, wstart, cmin, cmax, window=None, glob=None, below=0, above=0, clo=None, chi=None):
        self.C, self.wstart = int(C), int(wstart)
        self.cmin = np.asarray(cmin, dtype=np.float32).reshape(self.C).copy()
        self.cmax = np.asarray(cmax, dtype=np.float32).reshape(self.C).copy()
        self.window, self.glob = dict(window or {}), dict(glob or {})
        self.below, self.above = int(below), int(above)
        self.clo, self.chi = dict(clo or {}), dict(chi or {})
        self.validate()

    REGIONS = ('window', 'glob', 'below', 'above', 'clo', 'chi')

    def region_total(self, r):
        v = getattr(self, r)
        return int(v) if isinstance(v, int) else sum(int(c) for c in v.values())

    @property
    def total(self):
        return sum(self.region_total(r) for r in self.REGIONS)

    @property
    def flag(self):
        return bool(self.glob or self.below or self.above)

    def validate(self):
        """what the producers guarantee (k_mt_qdq, the channels_last pass, the single launches): anything else is refused"""
        assert self.C >= 1 and -NB // 2 <= self.wstart
        for d in (self.window, self.glob, self.clo, self.chi):
            assert all(int(k) == k and int(c) == c and c > 0 for k, c in d.items()), 'integer keys, positive counts'
        assert self.below >= 0 and self.above >= 0
        for k in self.window:
            assert self.wstart <= k < self.wstart + W, 'code %d is not in the window' % k
            assert k < NB // 2, 'a window bin whose code is >= MT_NB/2 is not used (the count goes to the above-range word)'
        for k in self.glob:
            assert -NB // 2 <= k < NB // 2, 'code %d has no global bin' % k
            assert not self.wstart <= k < self.wstart + W, 'code %d lies in the window: never counted in the global bins' % k
        for d, bound in ((self.clo, self.cmin), (self.chi, self.cmax)):
            for c in d:
                assert 0 <= c < self.C and np.isfinite(bound[c]), c
                assert bound[c] != np.rint(bound[c]), 'a clamp counter is used only where the bound is not an integer'


def mt_table(d, fill=0.5):
    """mt[CNNQ_NMT][C] (float32): rows CMIN, CMAX and WSTART (one value in every channel) from the description; the consumers
    read nothing else, so the other rows hold `fill`."""
    mt = np.full((NMT, d.C), fill, dtype=np.float32)
    mt[MT_CMIN], mt[MT_CMAX], mt[MT_WSTART] = d.cmin, d.cmax, np.float32(d.wstart)
    assert int(mt[MT_WSTART, 0]) == d.wstart
    return mt


def spread_count(count, n, how):
    """count split over n replicas -> int64 [n] with that sum.  how: 'one' (everything in one replica: the widest words),
    'even', or ('random', seed)."""
    count = int(count)
    out = np.zeros(n, dtype=np.int64)
    if how == 'one':
        out[(count * 7 + 3) % n] = count
    elif how == 'even':
        out[:] = count // n
        out[:count % n] += 1
    else:
        assert how[0] == 'random'
        rng = np.random.default_rng([int(how[1]), count % (1 << 31)])
        w = rng.random(n) * (rng.random(n) < 0.5)          # about half of the replicas stay empty
        if w.sum() == 0:
            w[0] = 1.
        out[:] = np.floor(w / w.sum() * count * (1 - 1e-9)).astype(np.int64)
        assert out.sum() <= count
        out[int(rng.integers(n))] += count - int(out.sum())
    assert out.sum() == count and out.min() >= 0
    return out


def mt_words(d, spread='even'):
    """The int64 words of the description: [0, NB) integer codes -NB/2 .., [NB] below, [NB + 1] above, C + C clamp counters, GR
    replicas of the W window bins (bin i: code wstart + i), the flag word."""
    d.validate()
    h = np.zeros(mt_hist_words(d.C), dtype=np.int64)
    for k, c in d.glob.items():
        h[k + NB // 2] = c
    h[NB], h[NB + 1] = d.below, d.above
    for c, n in d.clo.items():
        h[NB + 2 + c] = n
    for c, n in d.chi.items():
        h[NB + 2 + d.C + c] = n
    rep = h[NB + 2 + 2 * d.C:-1].reshape(GR, W)
    for j, (k, c) in enumerate(sorted(d.window.items())):
        how = (spread[0], spread[1] + j) if isinstance(spread, tuple) else spread
        rep[:, k - d.wstart] = spread_count(c, GR, how)
    # the producers add 1 per count that went to a global word: any non-zero value says "read the global bins"
    h[-1] = int((h[:NB + 2] != 0).sum())
    assert (h[-1] != 0) == d.flag and int(h[:-1].sum()) == d.total
    return h


def mt_regions(words, C):
    """The regions of a histogram's words (as the producers wrote them): dict(glob [NB], below, above, clo [C], chi [C], win [W]
    summed over the replicas, rep [GR, W], flag)."""
    words = np.asarray(words, dtype=np.int64)
    assert words.shape == (mt_hist_words(C),)
    rep = words[NB + 2 + 2 * C:-1].reshape(GR, W)
    return dict(glob=words[:NB], below=int(words[NB]), above=int(words[NB + 1]), clo=words[NB + 2:NB + 2 + C],
                chi=words[NB + 2 + C:NB + 2 + 2 * C], rep=rep, win=rep.sum(0), flag=int(words[-1]))


def _clamp_entries(d):
    """(value, count, entry index) of the clamp counters with hits; entry i < C is cmin[i], else cmax[i - C]"""
    return ([(d.cmin[c], int(n), c) for c, n in sorted(d.clo.items())]
            + [(d.cmax[c], int(n), d.C + c) for c, n in sorted(d.chi.items())])


def symbols(d, merge=True, shift=0):
    """The counts of the distinct symbols of a description: integer codes, the two out-of-range words, the distinct float32 clamp
    values (as np.unique on the float32 values merges them).  merge=False and shift are the mutations' (see mutations())."""
    bins = {}
    for k, c in d.glob.items():
        bins[k + NB // 2] = bins.get(k + NB // 2, 0) + int(c)
    if d.below:
        bins[NB] = d.below
    if d.above:
        bins[NB + 1] = d.above
    for k, c in d.window.items():
        i = k + NB // 2 + shift
        if i >= 0:                                       # (a bin shifted below the table is lost)
            bins[i] = bins.get(i, 0) + int(c)
    out = list(bins.values())
    ent = _clamp_entries(d)
    if ent:
        vals = np.array([v for v, _, _ in ent], dtype=np.float32)
        cnts = np.array([n for _, n, _ in ent], dtype=object)
        if merge:
            u, inv = np.unique(vals, return_inverse=True)
            out += [int(sum(cnts[inv == j])) for j in range(u.size)]
        else:
            out += [int(n) for n in cnts]
    return out


def entropy64(counts, total):
    """-sum p log2 p over the non-empty symbols, p = count / total, fp64 (utils/entropy.py:12-15)"""
    c = np.array([int(v) for v in counts if int(v)], dtype=np.float64)
    if not c.size:
        return 0.
    p = c / float(total)
    return float(-(p * np.log2(p)).sum() + 0.)


def entropy32(counts, total):
    """The kernels' arithmetic: pr = (float)count / (float)total, -pr * log2f(pr) in float32, the terms summed in fp64."""
    c = np.array([int(v) for v in counts if int(v)], dtype=np.uint64).astype(np.float32)
    if not c.size:
        return 0.
    pr = c / np.float32(np.uint64(int(total)))
    assert pr.dtype == np.float32
    return float((-pr * np.log2(pr)).astype(np.float64).sum() + 0.)


def symbols_of_words(words, d):
    """symbols() read back from words (every word counted, whatever the flag says) - for the mutation that damages the words"""
    r = mt_regions(words, d.C)
    bins = r['glob'].astype(object).copy()
    out = [r['below'], r['above']]
    for i in range(W):
        j = d.wstart + i + NB // 2
        if j < NB:
            bins[j] += int(r['win'][i])
    out += [int(v) for v in bins[bins != 0]]
    vals = np.concatenate([d.cmin, d.cmax])
    cnts = np.concatenate([r['clo'], r['chi']]).astype(object)
    live = np.flatnonzero(cnts != 0)
    if live.size:
        u, inv = np.unique(vals[live], return_inverse=True)
        out += [int(sum(cnts[live][inv == j])) for j in range(u.size)]
    return [c for c in out if c]


def mutations(d, spread='even'):
    """{name: symbol counts} of every mistake that applies to the description:
    drop_R / twice_R     region R not counted / counted twice (no drop_R where there is one symbol: its term is 0 anyway);
    shift_-1 / shift_+1  the window laid over the global bins one code off (flag raised only: without it nothing is overlaid);
    no_merge             equal clamp values kept apart;
    merge_unequal        the two most frequent distinct clamp values taken for one;
    low32                every word read as 32 bits."""
    out = {}
    for r in MtDesc.REGIONS:
        if d.region_total(r):
            for name, f in (('drop', 0), ('twice', 2)):
                if name == 'drop' and len(symbols(d)) == 1:
                    continue                             # one symbol, p = 1: its term is 0, present or not (the H = 0 cases)
                m = copy.deepcopy(d)
                v = getattr(m, r)
                setattr(m, r, v * f if isinstance(v, int) else {k: c * f for k, c in v.items() if f})
                out['%s_%s' % (name, r)] = symbols(m)
    if d.flag and d.window:
        out['shift_-1'], out['shift_+1'] = symbols(d, shift=-1), symbols(d, shift=1)
    ent = _clamp_entries(d)
    vals = np.array([v for v, _, _ in ent], dtype=np.float32)
    if vals.size and np.unique(vals).size < vals.size:
        out['no_merge'] = symbols(d, merge=False)
    if np.unique(vals).size >= 2:
        u, inv = np.unique(vals, return_inverse=True)
        tot = [sum(n for (_, n, _), j in zip(ent, inv) if j == q) for q in range(u.size)]
        a, b = sorted(range(u.size), key=lambda q: -tot[q])[:2]
        m = copy.deepcopy(d)
        for bound in (m.cmin, m.cmax):
            bound[bound == u[b]] = u[a]
        out['merge_unequal'] = symbols(m)
    words = mt_words(d, spread)
    if (words >> 32).any():
        out['low32'] = symbols_of_words(words & 0xffffffff, d)
    return out


# ------------------------------------------------------------------------------------------ the uniform quantizers' tables
def plain_table(counts, nbins):
    """{bin: count} -> int64 [nbins] (cnnq_entropy's argument)"""
    h = np.zeros(nbins, dtype=np.int64)
    for k, c in counts.items():
        assert 0 <= k < nbins and c > 0
        h[k] = c
    return h


def replica_tables(counts, spread='even'):
    """{bin: count} -> int64 [XREP, XBINS]: the replica tables cnnq_entropy_replicas and cnnq_hist_replicas_fold consume"""
    t = np.zeros((XREP, XBINS), dtype=np.int64)
    for j, (k, c) in enumerate(sorted(counts.items())):
        assert 0 <= k < XBINS and c > 0
        how = (spread[0], spread[1] + j) if isinstance(spread, tuple) else spread
        t[:, k] = spread_count(c, XREP, how)
    return t


def table_mutations(counts):
    """{name: symbol counts}: the last live bin not counted / counted twice, and every count read as 32 bits"""
    c = [int(v) for _, v in sorted(counts.items())]
    out = {}
    if len(c) > 1:
        out['drop_last'], out['twice_last'] = c[:-1], c + c[-1:]
    if any(v >> 32 for v in c):
        out['low32'] = [v & 0xffffffff for v in c]
    return out
