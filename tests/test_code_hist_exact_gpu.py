"""The kernels that COUNT codes (k_mt_qdq<HIST>, the channels_last mid-tread pass, the contiguous bf16 / fp16 mid-tread pass,
k_qdq<HIST>, k_cl_qdq_hist) on inputs whose histogram is known without the device.

The parameter tables are hand-built with a step of 1 or 0.5 and the inputs are exact multiples of the step, so x / step is an
integer before the clamps: no rounding tie, no divide to trust, and one numpy expression gives every code (the kernels' own
codes output is compared with it where there is one).  From the codes numpy derives every word the producer must write - the
window bins summed over the replicas, every global bin, the two out-of-range words, every clamp counter, whether the flag word is
raised - and the fp64 entropy (tests/_entropy.py) that cnnq_midtread_entropy / cnnq_entropy must then report within the tier
2e-5 * max(1, H).  All counts are compared exactly.  The values used are exact in bf16 and fp16 (asserted), so the channels_last
and the contiguous half kernels see the same numbers in every element type and must write the NCHW kernel's histogram.

NaN inputs are left out: the kernel counts a NaN code into the channel's c_min counter while torch.unique keeps NaNs apart, and
nothing in the reference depends on either.  Needs an MI355X: `pytest -m gpu`."""
import numpy as np
import pytest
import torch

import _entropy as E
from cnn_quantization_amd import _lib, ops

pytestmark = pytest.mark.gpu
NB, W = E.NB, E.W
# H*W % 4 != 0, H*W % 4 == 0, H*W < 4, and a few hundred tiles (several workgroups flush into one replica table)
SHAPES = [(2, 3, 5, 7), (2, 4, 8, 8), (3, 8, 1, 2), (8, 16, 28, 28)]
DTYPES = [torch.float32, torch.bfloat16, torch.float16]


def ids(v):
    return 'x'.join(map(str, v)) if isinstance(v, tuple) else str(v).replace('torch.', '')


def nhwc(a):
    """[N, C, H, W] -> the same values as dense [R = N*H*W][C]"""
    return np.ascontiguousarray(a.transpose(0, 2, 3, 1)).reshape(-1, a.shape[1])


def exact_in(x, dtype):
    t = torch.from_numpy(x)
    return bool((t.to(dtype).float() == t).all())


# ------------------------------------------------------------------------------------------ mid-tread
def mt_table(C, wstart, integer_bounds=False):
    """mt[NMT][C]: steps 1 and 0.5; channel 0 clamps most of its elements to a non-integer c_max, channel 1 is a constant channel
    (c_min == c_max, not an integer), channel 2 has the integer bounds wstart - 1 and wstart + 128 (its clamps are codes next to
    the window's ends and no clamp counter), the others non-integer bounds well outside the window."""
    mt = np.full((E.NMT, C), 0.5, dtype=np.float32)
    c = np.arange(C)
    mt[E.MT_DELTA] = np.where(c % 2, 0.5, 1.)
    mt[E.MT_CMIN], mt[E.MT_CMAX], mt[E.MT_WSTART] = wstart - 36.5, wstart + 164.25, wstart
    if integer_bounds:
        mt[E.MT_CMIN], mt[E.MT_CMAX] = -5., 5.
        return mt
    mt[E.MT_CMAX, 0] = wstart + 20.25
    mt[E.MT_CMIN, 1] = mt[E.MT_CMAX, 1] = wstart + 3.5
    mt[E.MT_CMIN, 2], mt[E.MT_CMAX, 2] = wstart - 1, wstart + W
    return mt


def mt_input(shape, mt, seed, forced=(), lo=-40, hi=170):
    """x = k * step[c] with integer k around the window (k in wstart + [lo, hi)), the codes next to the window's ends and `forced`
    planted from channel 2 upwards and from the last channel downwards; -> x float32 [N, C, H, W]"""
    N, C, H, Wd = shape
    ws = int(mt[E.MT_WSTART, 0])
    rng = np.random.default_rng(seed)
    k = rng.integers(ws + lo, ws + hi, size=shape).astype(np.float64)
    k[rng.random(shape) < 0.2] = 0.                                                   # (zero: the register-counted code)
    edge = [ws - 1, ws, ws + W - 1, ws + W] + list(forced)
    n_c = N * H * Wd
    assert len(edge) <= n_c * (C - 2)
    kc = np.ascontiguousarray(k.transpose(1, 0, 2, 3)).reshape(C, n_c)
    for i, v in enumerate(edge):                                                      # from channel 2 upwards, from the last one downwards
        kc[2 + i // n_c, i % n_c] = v
        kc[C - 1 - i // n_c, i % n_c] = v
    k = np.ascontiguousarray(kc.reshape(C, N, H, Wd).transpose(1, 0, 2, 3))
    x = (k * mt[E.MT_DELTA].astype(np.float64)[None, :, None, None]).astype(np.float32)
    assert np.array_equal(x.astype(np.float64) / mt[E.MT_DELTA][None, :, None, None], k)   # exact multiples
    return x


def mt_codes(x, mt, clip):
    """iq.py:202-214 in numpy float32: t = round(x / delta), then torch.min(t, c_max), torch.max(t, c_min)"""
    b = lambda row: mt[row][None, :, None, None]
    with np.errstate(over='ignore'):
        t = np.rint(x / b(E.MT_DELTA)).astype(np.float32)
    if clip:
        t = np.where(t < b(E.MT_CMAX), t, b(E.MT_CMAX))
        t = np.where(t > b(E.MT_CMIN), t, b(E.MT_CMIN))
    return t.astype(np.float32)


def mt_expected(t, mt, clip):
    """The regions the producers must write for the codes t [N, C, H, W] (the rules: the note above k_mt_qdq)."""
    C = t.shape[1]
    ws = int(mt[E.MT_WSTART, 0])
    lo, hi = mt[E.MT_CMIN][None, :, None, None], mt[E.MT_CMAX][None, :, None, None]
    at_hi = (t == hi) & (hi != np.rint(hi)) & bool(clip)
    at_lo = (t == lo) & (lo != np.rint(lo)) & bool(clip) & ~at_hi                      # c_min == c_max: counted once, as c_max
    r = t[~(at_hi | at_lo)].astype(np.float64)
    assert np.array_equal(r, np.rint(r))                                               # integer codes and infinities
    in_w = (r >= ws) & (r < ws + W)
    used = in_w & (r < NB // 2)                                                        # a window bin past the last integer code is not used
    rest = r[~used]
    in_g = (rest >= -NB // 2) & (rest < NB // 2)
    return dict(win=np.bincount((r[used] - ws).astype(np.int64), minlength=W),
                glob=np.bincount((rest[in_g] + NB // 2).astype(np.int64), minlength=NB),
                below=int((rest < -NB // 2).sum()), above=int((rest >= NB // 2).sum()),
                clo=at_lo.sum(axis=(0, 2, 3)), chi=at_hi.sum(axis=(0, 2, 3)))


def codes_entropy(t):
    """fp64 entropy of the codes as utils/entropy.py:6-17 computes it (torch.unique on the float32 codes).  The histogram has ONE
    word for everything above the integer bins and one for everything below: the inputs keep to one distinct code in each."""
    assert np.unique(t[t >= NB // 2]).size <= 1 and np.unique(t[t < -NB // 2]).size <= 1
    _, counts = np.unique(t, return_counts=True)
    return E.entropy64(counts, t.size)


def check_hist(words, t, mt, clip, what):
    C = t.shape[1]
    want, got = mt_expected(t, mt, clip), E.mt_regions(words, C)
    assert np.array_equal(got['win'], want['win']), what                              # the window totals over the replicas
    assert np.array_equal(got['glob'], want['glob']), what
    assert (got['below'], got['above']) == (want['below'], want['above']), what
    assert np.array_equal(got['clo'], want['clo']) and np.array_equal(got['chi'], want['chi']), what
    uses_global = bool(want['glob'].any() or want['below'] or want['above'])
    assert (got['flag'] != 0) == uses_global, what
    assert int(words[:-1].sum()) == t.size, what
    assert (got['rep'] >= 0).all()
    return got


def hist_entropy(h, mt_d, C, total):
    out = torch.full((1,), -7.25, dtype=torch.float32, device='cuda')
    _lib.check(_lib.load().cnnq_midtread_entropy(ops._ptr(h), ops._ptr(mt_d), C, total, ops._ptr(out), ops._stream(h)),
               'cnnq_midtread_entropy')
    return float(out)


def run_nchw(x, mt, clip):
    """cnnq_pc_midtread_qdq with codes and histogram -> (codes, words, entropy)"""
    N, C, H, Wd = x.shape
    xd, md = torch.from_numpy(x).cuda(), torch.from_numpy(mt).cuda()
    y, codes = torch.empty_like(xd), torch.empty_like(xd)
    h = torch.zeros(E.mt_hist_words(C), dtype=torch.int64, device='cuda')
    _lib.check(_lib.load().cnnq_pc_midtread_qdq(ops._ptr(xd), ops._ptr(y), N, C, H * Wd, ops._ptr(md), int(clip), ops._ptr(codes),
                                                ops._ptr(h), ops._stream(xd)), 'cnnq_pc_midtread_qdq')
    ent = hist_entropy(h, md, C, x.size)
    with np.errstate(invalid='ignore'):
        want_y = (mt_codes(x, mt, clip) * mt[E.MT_DELTA][None, :, None, None]).astype(np.float32)
    assert np.array_equal(y.cpu().numpy(), want_y, equal_nan=True)
    return codes.cpu().numpy(), h.cpu().numpy(), ent


def run_nhwc(x, mt, dtype):
    """cnnq_pc_midtread_qdq_nhwc on the same values as [R][C] of `dtype` -> (words, entropy)"""
    C = x.shape[1]
    assert exact_in(x, dtype)
    xd, md = torch.from_numpy(nhwc(x)).to(dtype).cuda(), torch.from_numpy(mt).cuda()
    y = torch.empty_like(xd)
    h = torch.zeros(E.mt_hist_words(C), dtype=torch.int64, device='cuda')
    _lib.check(_lib.load().cnnq_pc_midtread_qdq_nhwc(ops._ptr(xd), ops._ptr(y), ops._DTYPE_CODES[dtype], xd.shape[0], C, ops._ptr(md),
                                                     ops._ptr(h), ops._stream(xd)), 'cnnq_pc_midtread_qdq_nhwc')
    return h.cpu().numpy(), hist_entropy(h, md, C, x.size)


def run_half(x, mt, dtype):
    """cnnq_pc_midtread_qdq_dt on the same values as contiguous [N, C, H, W] of bf16 / fp16 (the histogram zeroed by the caller, as
    ops.mid_tread_qdq_half does) -> (words, entropy); y is checked against the codes * delta rounded into the dtype"""
    N, C, H, Wd = x.shape
    assert exact_in(x, dtype)
    xd, md = torch.from_numpy(x).to(dtype).cuda(), torch.from_numpy(mt).cuda()
    y = torch.empty_like(xd)
    h = torch.zeros(E.mt_hist_words(C), dtype=torch.int64, device='cuda')
    _lib.check(_lib.load().cnnq_pc_midtread_qdq_dt(ops._ptr(xd), ops._ptr(y), ops._DTYPE_CODES[dtype], N, C, H * Wd, ops._ptr(md), ops._ptr(h),
                                                   ops._stream(xd)), 'cnnq_pc_midtread_qdq_dt')
    want_y = torch.from_numpy((mt_codes(x, mt, 1) * mt[E.MT_DELTA][None, :, None, None]).astype(np.float32)).to(dtype)
    assert torch.equal(y.cpu(), want_y), dtype
    return h.cpu().numpy(), hist_entropy(h, md, C, x.size)


def check_all_layouts(x, mt, what, dtypes=DTYPES):
    """clip = 1: the NCHW kernel, then the channels_last kernel in every element type and the contiguous bf16 / fp16 pass, against
    numpy and region by region against the NCHW kernel"""
    t = mt_codes(x, mt, 1)
    h64 = codes_entropy(t)
    codes, words, ent = run_nchw(x, mt, 1)
    assert np.array_equal(codes, t), what
    ref = check_hist(words, t, mt, 1, what)
    print('%-40s H64 %.9f  H %.9f' % (what, h64, ent))
    assert abs(ent - h64) <= E.tier(h64), what
    for dt in dtypes:
        w2, e2 = run_nhwc(x, mt, dt)
        got = check_hist(w2, t, mt, 1, (what, dt))
        for r in ('win', 'glob', 'below', 'above', 'clo', 'chi'):
            assert np.array_equal(got[r], ref[r]), (what, dt, r)
        assert abs(e2 - h64) <= E.tier(h64), (what, dt)
    for dt in (torch.bfloat16, torch.float16):
        w3, e3 = run_half(x, mt, dt)
        got = check_hist(w3, t, mt, 1, (what, 'contiguous', dt))
        for r in ('win', 'glob', 'below', 'above', 'clo', 'chi'):
            assert np.array_equal(got[r], ref[r]), (what, 'contiguous', dt, r)
        assert abs(e3 - h64) <= E.tier(h64), (what, 'contiguous', dt)
    return ref


@pytest.mark.parametrize('wstart', [-64, 8])
@pytest.mark.parametrize('shape', SHAPES, ids=ids)
def test_midtread_clipped_codes_around_the_window(shape, wstart):
    """codes at wstart - 1, wstart, wstart + 127, wstart + 128; a channel that mostly clamps to a non-integer c_max; a constant
    channel; integer bounds; with wstart = 8 the zeros lie outside the window and go to the global bin of code 0"""
    C = shape[1]
    mt = mt_table(C, wstart)
    x = mt_input(shape, mt, seed=shape[0] * 100 + wstart + 64)
    ref = check_all_layouts(x, mt, 'clip1 %s wstart %d' % (ids(shape), wstart))
    n_c = shape[0] * shape[2] * shape[3]
    assert ref['chi'][1] == n_c and ref['clo'][1] == 0                                # the constant channel: counted once
    assert ref['chi'][0] * 2 > n_c or n_c < 50                                        # most of channel 0 sits on its c_max
    assert ref['clo'][2] == 0 and ref['chi'][2] == 0                                  # integer bounds: no clamp counter
    assert ref['win'][0] and ref['win'][W - 1] and ref['glob'][wstart - 1 + NB // 2] and ref['glob'][wstart + W + NB // 2]
    assert ref['flag'] != 0
    if wstart > 0:
        assert ref['glob'][NB // 2] > 0                                               # code 0, outside the window
    elif x.size >= 1000:
        assert ref['win'][-wstart] > 0


@pytest.mark.parametrize('shape', SHAPES, ids=ids)
def test_midtread_unclipped_codes_at_the_ends_of_the_table(shape):
    """clip = 0, fp32, window at -64: codes -MT_NB/2 - 1 (below), -MT_NB/2 (the first bin), MT_NB/2 - 1 (the last), MT_NB/2 (above)"""
    mt = mt_table(shape[1], -64)
    x = mt_input(shape, mt, seed=7, forced=(-NB // 2 - 1, -NB // 2, NB // 2 - 1, NB // 2), lo=-200, hi=330)
    t = mt_codes(x, mt, 0)
    codes, words, ent = run_nchw(x, mt, 0)
    assert np.array_equal(codes, t)
    got = check_hist(words, t, mt, 0, ids(shape))
    twice = 2 if shape[1] > 3 else 1                                                  # (C = 3: both plantings are channel 2)
    assert got['below'] == twice and got['above'] == twice and got['glob'][0] == twice and got['glob'][NB - 1] == twice
    assert not got['clo'].any() and not got['chi'].any()
    h64 = codes_entropy(t)
    assert abs(ent - h64) <= E.tier(h64)


def test_midtread_unclipped_infinities():
    shape = (2, 4, 8, 8)
    mt = mt_table(shape[1], -64)
    x = mt_input(shape, mt, seed=9)
    x[0, 0, 0, :3], x[1, 3, 7, 5:], x[1, 1, 2, 2] = np.inf, -np.inf, np.inf
    t = mt_codes(x, mt, 0)
    codes, words, ent = run_nchw(x, mt, 0)
    assert np.array_equal(codes, t)
    got = check_hist(words, t, mt, 0, 'inf')
    assert got['above'] == 4 and got['below'] == 3
    h64 = codes_entropy(t)
    assert abs(ent - h64) <= E.tier(h64)


def test_midtread_window_past_the_last_integer_code():
    """the window starts 3 codes before MT_NB/2: its bins 3.. stand for codes that have no integer bin - the above-range word"""
    shape = (2, 3, 5, 7)
    mt = mt_table(shape[1], NB // 2 - 3)
    rng = np.random.default_rng(3)
    k = rng.integers(NB // 2 - 5, NB // 2 + 1, size=shape).astype(np.float64)
    x = (k * mt[E.MT_DELTA].astype(np.float64)[None, :, None, None]).astype(np.float32)
    t = mt_codes(x, mt, 0)
    assert np.array_equal(t, k)
    codes, words, ent = run_nchw(x, mt, 0)
    got = check_hist(words, t, mt, 0, 'past')
    assert got['above'] == (k == NB // 2).sum() > 0 and got['win'][:3].all() and not got['win'][3:].any()
    h64 = codes_entropy(t)
    assert abs(ent - h64) <= E.tier(h64)


@pytest.mark.parametrize('wstart', [-64, 8])
@pytest.mark.parametrize('shape', SHAPES, ids=ids)
def test_midtread_all_zeros(shape, wstart):
    """one symbol, counted in registers: in the window bin of code 0 - or, with a window that does not hold 0, in the global bin
    with the flag raised.  H = 0."""
    mt = mt_table(shape[1], wstart, integer_bounds=True)
    x = np.zeros(shape, dtype=np.float32)
    ref = check_all_layouts(x, mt, 'zeros %s wstart %d' % (ids(shape), wstart))
    if wstart <= 0:
        assert ref['win'][-wstart] == x.size and ref['flag'] == 0
    else:
        assert ref['glob'][NB // 2] == x.size and ref['flag'] != 0
    for clip in (0, 1):
        codes, words, ent = run_nchw(x, mt, clip)
        check_hist(words, np.zeros(shape, np.float32), mt, clip, 'zeros')
        assert ent == 0.


# ------------------------------------------------------------------------------------------ the uniform quantizers
def qp_table(C, bits, zp_kind):
    """qp[NQP][C]: scale 1 or 0.5, an integer zero point (0, qmax, or one per channel), qmax = 2^bits - 1"""
    qmax = (1 << bits) - 1
    c = np.arange(C)
    zp = {'zero': np.zeros(C), 'qmax': np.full(C, qmax), 'mixed': (c * 7 + 3) % (qmax + 1)}[zp_kind]
    qp = np.zeros((_lib.NQP, C), dtype=np.float32)
    qp[_lib.QP_SCALE], qp[_lib.QP_ZP], qp[_lib.QP_QMAX] = np.where(c % 2, 0.5, 1.), zp, qmax
    return qp


def uniform_input(shape, qp, kind, seed):
    """x = (k - zp) * scale for integer k: 'all_codes' every code 0 .. qmax (and -1 and qmax + 1, which clamp), 'one_code'
    every element on code 5, 'zero_point' every element 0 (code zp: the register counter)"""
    qmax = int(qp[_lib.QP_QMAX, 0])
    n = int(np.prod(shape))
    rng = np.random.default_rng(seed)
    if kind == 'all_codes':
        k = rng.integers(-1, qmax + 2, size=n)
        k[:qmax + 1] = np.arange(qmax + 1)[:n]
        k = rng.permutation(k).reshape(shape)
    elif kind == 'one_code':
        k = np.full(shape, 5)
    else:
        k = np.broadcast_to(qp[_lib.QP_ZP].astype(np.int64)[None, :, None, None], shape).copy()
    b = lambda row: qp[row].astype(np.float64)[None, :, None, None]
    x = ((k - b(_lib.QP_ZP)) * b(_lib.QP_SCALE)).astype(np.float32)
    want = np.clip(k, 0, qmax)
    q = x / qp[_lib.QP_SCALE][None, :, None, None] + qp[_lib.QP_ZP][None, :, None, None]       # qdq1 in numpy float32
    assert q.dtype == np.float32 and np.array_equal(np.rint(np.clip(q, 0, qmax)), want)
    return x, want


@pytest.mark.parametrize('zp_kind', ['zero', 'qmax', 'mixed'])
@pytest.mark.parametrize('kind', ['all_codes', 'one_code', 'zero_point'])
@pytest.mark.parametrize('shape', SHAPES, ids=ids)
def test_uniform_code_histograms(shape, kind, zp_kind):
    lib = _lib.load()
    N, C, H, Wd = shape
    for bits in (4, 8):
        qp = qp_table(C, bits, zp_kind)
        x, want = uniform_input(shape, qp, kind, seed=bits + N)
        table = np.bincount(want.reshape(-1), minlength=256).astype(np.int64)
        if kind == 'all_codes' and x.size >= 4 << bits:
            assert table[:1 << bits].all()
        h64 = E.entropy64(table, x.size)
        xd, qd = torch.from_numpy(x).cuda(), torch.from_numpy(qp).cuda()
        # NCHW: the plain 256-word table
        hist = torch.zeros(256, dtype=torch.int64, device='cuda')
        y, codes = ops.pc_qdq(xd, N, C, H * Wd, qd, want_codes=True, hist=hist)
        assert np.array_equal(codes.cpu().numpy(), want)
        got = hist.cpu().numpy()
        assert np.array_equal(got, table) and int(got.sum()) == x.size
        out = torch.full((1,), -7.25, dtype=torch.float32, device='cuda')
        _lib.check(lib.cnnq_entropy(ops._ptr(hist), 256, ops._ptr(out), ops._stream(hist)), 'cnnq_entropy')
        assert abs(float(out) - h64) <= E.tier(h64)
        # channels_last: the replica tables, folded
        for dt in DTYPES:
            assert exact_in(x, dt)
            xn = torch.from_numpy(nhwc(x)).to(dt).cuda()
            yn = torch.empty_like(xn)
            rep = torch.zeros(lib.cnnq_hist_replica_bytes() // 8, dtype=torch.int64, device='cuda')
            _lib.check(lib.cnnq_pc_qdq_hist_nhwc(ops._ptr(xn), ops._ptr(yn), ops._DTYPE_CODES[dt], xn.shape[0], C, ops._ptr(qd), 1 << bits,
                                                 ops._ptr(rep), ops._stream(xn)), 'cnnq_pc_qdq_hist_nhwc')
            assert int(rep.sum()) == x.size and int(rep.min()) >= 0
            folded = torch.zeros(256, dtype=torch.int64, device='cuda')
            _lib.check(lib.cnnq_hist_replicas_fold(ops._ptr(rep), ops._ptr(folded), ops._stream(rep)), 'cnnq_hist_replicas_fold')
            assert np.array_equal(folded.cpu().numpy(), table), (bits, dt)
            assert int(rep.abs().sum()) == 0
            assert np.array_equal(yn.float().cpu().numpy(), nhwc(y.cpu().numpy())), (bits, dt)
