"""Reference restatements for the KLD calibration kernels (k_kld_hist, k_kld_search, k_kld_pick) on hand-built histograms and
edge-valued rows - helper, no tests.  divergences64 is oracle/kld_oracle.py::divergences with every float32 step of the reference
kept bit for bit and only the normalisation and the sum of p*log(p/q) carried out in np.longdouble; test_kld_table_cpu.py pins it to
the oracle and to the golden rows, so the GPU tests compare against something anchored.  The only line that is not the oracle's is
marked LIBRARY CHOICE: an input on which the reference raises."""
import functools

import numpy as np

from oracle import kld_oracle as K

NB, NQ, NC = K.NUM_BINS, K.NUM_QUANTIZED_BINS, 994
ZERO, HALF_Q = NB // 2, NQ // 2
EPS = 0.0001

# |div - div64| <= TOL * mag, mag = sum |p_k log(p_k / q_k)|: eight times the worst ratio measured on the MI355X over every case of
# test_kld_table_gpu.py (2.63e-13, see its docstring); an fp32 accumulation shows 1.1e-6, the cap the tests accept is TOL_CAP
TOL = 2.1e-12
TOL_CAP = 1e-10


def _smooth32(v):
    """K.smooth's float32 result for an integer or float32 vector, or None where it raises (no non-zero entry): float32(v) +
    float32(+eps) on the zeros, + float32(-eps1) on the others, eps1 formed in Python double."""
    zeros = v == 0
    n_zeros = int(zeros.sum())
    n_nonzeros = v.size - n_zeros
    if not n_nonzeros:
        return None
    eps1 = EPS * float(n_zeros) / float(n_nonzeros)
    return v.astype(np.float32) + np.where(zeros, np.float32(EPS), np.float32(-eps1))


def smoothed(hist):
    """-> (ps, qs, offs, alive): the float32 smoothed P and Q of the candidates `alive`, packed one after the other (candidate
    alive[j] occupies offs[j]:offs[j + 1]).  The others have an all-zero Q (the oracle's entropy() then yields NaN) or the row is
    empty."""
    hist = np.asarray(hist, dtype=np.int64)
    assert hist.shape == (NB,) and hist.min() >= 0 and hist.sum() < 2 ** 31
    csum = np.concatenate([[0], np.cumsum(hist)])
    ps, qs, alive = [], [], []
    for i in range(HALF_Q, NB // 2 + 1):
        start, stop = ZERO - i, ZERO + i + 1
        sl = hist[start:stop]
        m = sl.size
        p = sl.copy()
        p[0] += csum[start]
        p[-1] += csum[NB] - csum[stop]
        w = m // NQ
        first = np.arange(NQ) * w
        seg = np.minimum(np.arange(m) // w, NQ - 1)
        mass = np.add.reduceat(sl, first)                               # < 2^31 (asserted above): the reference's int32 holds it
        live = sl != 0
        live[-1] = False
        norm = np.add.reduceat(live.astype(np.int64), first)
        with np.errstate(divide='ignore', invalid='ignore'):
            level = (mass.astype(np.float64) / norm.astype(np.float64)).astype(np.float32)
        q = np.where(live, level[seg], np.float32(0)).astype(np.float32)
        # LIBRARY CHOICE: the reference raises on an empty row (smooth(p): 'all entries are 0'); the device cannot, and gives NaN
        sp, sq = _smooth32(p), _smooth32(q)
        if sp is not None and sq is not None:
            ps.append(sp)
            qs.append(sq)
            alive.append(i - HALF_Q)
    offs = np.concatenate([[0], np.cumsum([v.size for v in ps])]).astype(np.int64)
    cat = lambda v: np.concatenate(v) if v else np.zeros(0, dtype=np.float32)
    return cat(ps), cat(qs), offs, np.asarray(alive, dtype=np.int64)


def _kl(ps, qs, offs, alive, ftype):
    """KL(P || Q) and sum |p_k log(p_k / q_k)| of the packed candidates, normalised and summed in ftype; NaN for the others."""
    div, mag = np.full(NC, np.nan, dtype=ftype), np.full(NC, np.nan, dtype=ftype)
    if alive.size:
        ps, qs, lens = ps.astype(ftype), qs.astype(ftype), np.diff(offs)
        pk = ps / np.repeat(np.add.reduceat(ps, offs[:-1]), lens)
        qk = qs / np.repeat(np.add.reduceat(qs, offs[:-1]), lens)
        term = pk * np.log(pk / qk)
        div[alive] = np.add.reduceat(term, offs[:-1])
        mag[alive] = np.add.reduceat(np.abs(term), offs[:-1])
    return div, mag


@functools.lru_cache(maxsize=None)
def _divergences64(key):
    hist = np.frombuffer(key, dtype=np.int64)
    div, mag = _kl(*smoothed(hist), np.longdouble)
    div.setflags(write=False)
    mag.setflags(write=False)
    return div, mag


def divergences64(hist):
    """-> (div, mag), np.longdouble [994]: KL(P || Q) of every candidate and the scale sum |p_k log(p_k / q_k)|; NaN exactly where
    the oracle yields NaN.  Computed once per histogram and shared (read-only)."""
    return _divergences64(np.ascontiguousarray(hist, dtype=np.int64).tobytes())


def pick(div):
    """numpy.argmin: the first NaN wins, else the first minimum."""
    return int(np.argmin(np.asarray(div, dtype=np.float64)))


def pick64(hist):
    """The restatement's own choice, on the longdouble curve."""
    div, _ = divergences64(hist)
    nan = np.flatnonzero(np.isnan(div))
    return int(nan[0]) if nan.size else int(np.argmin(div))


def is_clear(hist, tol=None):
    """The minimum is not a near tie: the runner-up lies more than 100 tolerances above it, or the curve starts with NaN."""
    tol = TOL if tol is None else tol
    div, mag = divergences64(hist)
    if np.isnan(div[0]):
        return True
    assert not np.isnan(div).any()                                      # NaN is a prefix of the curve (nested kept ranges)
    order = np.argsort(div, kind='stable')
    return bool(div[order[1]] - div[order[0]] > 100 * tol * mag[order[0]])


def edges64(mn, mx):
    """The 2002 float64 edges numpy.histogram builds for range (-th, th), th = max(|mn|, |mx|) of two float32 values - the +-0.5
    widening of an empty range included."""
    mn, mx = np.float64(np.float32(mn)), np.float64(np.float32(mx))
    th = max(abs(mn), abs(mx))
    first, last = -th, th
    if first == last:
        first, last = first - 0.5, last + 0.5
    return np.linspace(first, last, NB + 1)


def device_index(row):
    """k_kld_hist's index rule restated in numpy on one float32 row: estimate (a - first) * (2001 / den), clamp, one step down, one
    step up, clamp (numpy itself divides by den and multiplies by 2001; both are corrected against the same edges) -> (bin of every
    value inside the range, how many took the step down, how many the step up)."""
    row = np.asarray(row, dtype=np.float32)
    e = edges64(row.min(), row.max())
    a = row.astype(np.float64)
    a = a[(a >= e[0]) & (a <= e[-1])]
    idx = ((a - e[0]) * (NB / (e[-1] - e[0]))).astype(np.int64)
    idx = np.clip(idx, 0, NB - 1)
    down = a < e[idx]
    idx -= down
    up = (idx != NB - 1) & (a >= e[idx + 1])
    idx += up
    return np.clip(idx, 0, NB - 1), int(down.sum()), int(up.sum())


def device_hist(row):
    return np.bincount(device_index(row)[0], minlength=NB).astype(np.int64)


def numpy_hist(row):
    """The reference's histogram of one float32 row (K.histogram: float64 values, range (-th, th))."""
    return K.histogram(np.asarray(row, dtype=np.float32))[2].astype(np.int64)


# ------------------------------------------------------------------------------------------------ hand-built histograms
def _one(b, count):
    h = np.zeros(NB, dtype=np.int64)
    h[b] = count
    return h


def _bounds(cand):
    i = cand + HALF_Q
    start, stop = ZERO - i, ZERO + i + 1
    return start, stop, (stop - start) // NQ


GROUP_CAND = 301            # m = 617 = 15 * 41 + 2: the last group is two bins wider than the others


def _build_cases():
    rng = np.random.default_rng(20240607)
    cases = {}
    # one occupied bin: the centre, both ends, the first / last kept bins of candidate 0 (993 .. 1007) and their neighbours
    for n, b in enumerate((0, 1, 992, 993, 994, 1000, 1006, 1007, 1008, 1999, 2000)):
        cases['one_%d' % b] = _one(b, 3 + n)
    # the centre plus only the LAST kept bin of candidate 500 (the bin the expansion never writes)
    h = _one(ZERO, 100)
    h[_bounds(500)[1] - 1] = 3
    cases['centre_last500'] = h
    cases['ones'] = np.ones(NB, dtype=np.int64)
    cases['random'] = rng.integers(1, 10 ** 6, NB)
    h = np.zeros(NB, dtype=np.int64)
    on = rng.choice(NB, NB // 50, replace=False)
    h[on] = rng.integers(1, 1000, on.size)
    cases['sparse2'] = h
    h = np.zeros(NB, dtype=np.int64)
    h[::7] = 10 ** 6
    cases['every7'] = h
    # occupied bins only at the group boundaries of one candidate, and one bin before them: a boundary that is off by one moves a
    # whole bin's mass into the neighbouring group
    start, stop, w = _bounds(GROUP_CAND)
    at = start + w * np.arange(NQ)
    counts = rng.integers(10, 1000, NQ)
    h = np.zeros(NB, dtype=np.int64)
    h[at] = counts
    cases['group_at'] = h
    h = np.zeros(NB, dtype=np.int64)
    h[at[1:] - 1] = counts[1:]
    h[start] = counts[0]
    cases['group_before'] = h
    # both at once, every count different: each group holds its first and its last bin
    h = np.zeros(NB, dtype=np.int64)
    h[at] = counts
    h[at[1:] - 1] = rng.integers(10, 1000, NQ - 1)
    h[stop - 1] = 77
    h[stop - 2] = 55
    cases['group_both'] = h
    # a count that rounds when cast to float32, among small ones
    h = rng.integers(1, 50, NB)
    h[1100] = 2 ** 24 + 1
    cases['big24'] = h
    # folded outliers dwarf everything: a flat curve and a genuine near tie (float32 oracle: candidate 0, longdouble: another)
    h = np.zeros(NB, dtype=np.int64)
    h[0] = 2 ** 30 - 12345
    h[NB - 1] = 2 ** 30 - 777
    h[ZERO - 3:ZERO + 4] = (2, 5, 11, 40, 9, 6, 1)
    cases['ends_2p30'] = h
    # empty end bins without outliers (p_first = p_last = 0 at the widest candidates) around a dense middle
    h = np.zeros(NB, dtype=np.int64)
    h[40:1950] = rng.integers(0, 30, 1910)
    cases['empty_ends'] = h
    # outliers on one side only, beyond an empty kept end bin
    h = np.zeros(NB, dtype=np.int64)
    h[700:1300] = rng.integers(1, 200, 600)
    h[1990:] = rng.integers(1, 10 ** 5, 11)
    cases['right_tail'] = h
    # candidate 95 (m = 205) with 158 zeros in P: -(0.0001 * 158 / 47) rounded once from double and the same expression
    # evaluated in float32 differ in the last place, and a count of 9 .. 16 plus the one or the other rounds differently
    start, stop, w = _bounds(95)
    h = np.zeros(NB, dtype=np.int64)
    h[start:start + 2 * 47:2] = np.resize((9, 13, 16, 100), 47)
    cases['smooth_ulp'] = h
    cases['laplace'] = numpy_hist(rng.laplace(0.03, 0.8, 200000).astype(np.float32))
    for h in cases.values():
        h.setflags(write=False)
    return cases


CASES = _build_cases()
CASE_NAMES = list(CASES)

F32_MAX = float(np.finfo(np.float32).max)
DENORM = float(np.float32(1e-45))                                       # the smallest float32 denormal, 2^-149
# the hand-given (min, max) of test (a), cycled over the rows: the search must not depend on them, the picked edge must
ROWMM = [(-1., 1.), (-3., 0.5), (0.25, 2.), (0., 0.), (-2001., 2001.), (-F32_MAX, F32_MAX), (-3 * DENORM, DENORM)]


# ------------------------------------------------------------------------------------------------ edge-valued rows
# the last two are there for the corrections of the index estimate: 98049 = 2001 * 49 has integer edges (-98049 + 98 k) and a scale
# 1 / 98 that rounds low, so the estimate of the edges k = 2^n falls just below k (step up); on 20.489496 two values take the step
# down.  No other range here needs either step.
EDGE_TH = [np.float32(v) for v in (1.0, 0.7, 3.0, 2001.0, 0.1, 6.1234567, 1e-30, 1e30, F32_MAX, DENORM, 98049.0, 20.4894962310791)]


def edge_row(th, drop_pos):
    """float32(edge_k) for each of the 2002 edges of (-th, th), both float32 neighbours of each (without what falls outside +-th),
    +-th and +-0.0; drop_pos: without +th, so that |min| > max."""
    th = np.float32(th)
    e32 = edges64(-th, th).astype(np.float32)
    inf = np.float32(np.inf)
    with np.errstate(over='ignore'):                                    # the neighbour beyond float32 max is inf, and dropped
        v = np.concatenate([e32, np.nextafter(e32, -inf), np.nextafter(e32, inf), np.array([-th, th, 0., -0.], dtype=np.float32)])
    v = v[np.abs(v) <= th]
    if drop_pos:
        v = v[v != th]
    return np.ascontiguousarray(v, dtype=np.float32)


def edge_drops(r, drop_parity):
    return r % 2 == drop_parity and float(EDGE_TH[r]) != DENORM


def edge_batch(length_mod4, drop_parity):
    """The edge rows as one [len(EDGE_TH), L] float32 array, padded with 0.0 to the smallest common L with L % 4 == length_mod4;
    the rows whose index has parity drop_parity go without +th (not the denormal's, which holds three distinct values)."""
    rows = [edge_row(th, edge_drops(r, drop_parity)) for r, th in enumerate(EDGE_TH)]
    L = max(r.size for r in rows)
    L += (length_mod4 - L) % 4
    out = np.zeros((len(rows), L), dtype=np.float32)
    for r, v in enumerate(rows):
        out[r, :v.size] = v
    return out
