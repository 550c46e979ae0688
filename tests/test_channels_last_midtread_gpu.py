"""Config 5 (mid-tread quantization with per-channel bin allocation, and the entropy of its codes) on dense channels_last
activations, fp32 / bf16 / fp16.

As for config 3 the per-channel sums are added in the NHWC geometry's order, so equality with the NCHW chain's table is not the
contract.  The contract has two halves:
  1. the table: `stats` against fp64 on x.float() by check_table of tests/test_channels_last_aciq_gpu.py (MIN / MAX bit-equal,
     MEAN / STD / B within RTOL_STAT = 2e-6 and its absolute floors);
  2. given the table, bit for bit: mt equals cnnq_pc_midtread_params on it; y equals the NCHW kernel (cnnq_pc_midtread_qdq through
     the C ABI on x.contiguous().float() with that mt) cast to x's dtype; and against that kernel's histogram the first
     MT_HIST_BINS + 2 + 2 * C words are equal word for word, the window bins summed over the replica tables are equal, the flag
     word is zero in both or in neither, the entropy equals cnnq_midtread_entropy on the NCHW histogram bit for bit, and every
     element was counted once."""
import ctypes
import importlib

import pytest
import torch
from hypothesis import HealthCheck, assume, given, settings
from hypothesis import strategies as st

import _quantizer as Q
from test_channels_last_aciq_gpu import WIDTH_CASES, check_table
from test_channels_last_gpu import DTYPES, IDS, cl, is_cl, same, values

pytestmark = pytest.mark.gpu


def mods():
    from cnn_quantization_amd import _lib as L, ops
    return L, ops


def run(x, target, sym, **kw):
    L, ops = mods()
    return ops.mid_tread_qdq_nhwc(x, target, sym, **kw)


def mt_of(stats, target, sym):
    """cnnq_pc_midtread_params (clip = 1) on a table."""
    L, ops = mods()
    C = stats.shape[1]
    tabs = ops._midtread_tables(stats.device)
    mt = torch.empty((L.NMT, C), dtype=torch.float32, device=stats.device)
    L.check(L.load().cnnq_pc_midtread_params(ops._ptr(stats), C, float(target), 1, int(bool(sym)), ops._ptr(tabs), tabs.shape[1],
                                             ops._ptr(mt), ops._stream(stats)), 'cnnq_pc_midtread_params')
    return mt


def nchw_kernel(x, mt, want_hist=False, want_codes=False):
    """The existing NCHW kernel with the table mt on x.contiguous().float(): (y in x's dtype, codes, hist, entropy)."""
    L, ops = mods()
    N, C, H, W = x.shape
    xc = x.contiguous().float()
    y = torch.empty_like(xc)
    codes = torch.empty_like(xc) if want_codes else None
    hist = torch.zeros(L.mt_hist_words(C), dtype=torch.int64, device='cuda') if want_hist else None
    L.check(L.load().cnnq_pc_midtread_qdq(ops._ptr(xc), ops._ptr(y), N, C, H * W, ops._ptr(mt), 1, ops._ptr(codes), ops._ptr(hist),
                                          ops._stream(xc)), 'cnnq_pc_midtread_qdq')
    ent = None
    if want_hist:
        ent = torch.empty(1, dtype=torch.float32, device='cuda')
        L.check(L.load().cnnq_midtread_entropy(ops._ptr(hist), ops._ptr(mt), C, x.numel(), ops._ptr(ent), ops._stream(xc)),
                'cnnq_midtread_entropy')
    return y.to(x.dtype), codes, hist, ent


def same_scalar(a, b):
    a, b = a.reshape(1).float(), b.reshape(1).float()
    return same(a, b)


def check_given_table(x, y, ent, parts, target, sym):
    """Half 2: everything behind the table, bit for bit."""
    L, _ = mods()
    C = x.shape[1]
    mt, hist = parts['mt'], parts['hist']
    assert same(mt, mt_of(parts['stats'], target, sym))
    y_ref, _, h_ref, e_ref = nchw_kernel(x, mt, want_hist=hist is not None)
    assert same(y, y_ref), (tuple(x.shape), x.dtype, target, sym, x.storage_offset())
    if hist is None:
        assert ent is None
        return
    n = L.MT_HIST_BINS + 2 + 2 * C
    assert torch.equal(hist[:n], h_ref[:n])
    reps = hist[n:-1].view(L.MT_HIST_REPLICAS, L.MT_HIST_WINDOW).sum(0)
    assert torch.equal(reps, h_ref[n:-1].view(L.MT_HIST_REPLICAS, L.MT_HIST_WINDOW).sum(0))
    assert (int(hist[-1]) != 0) == (int(h_ref[-1]) != 0)
    assert same_scalar(ent, e_ref), (float(ent), float(e_ref))
    assert int(hist[:-1].sum()) == x.numel()


def check(x, target, sym, want_entropy, half1=True):
    L, ops = mods()
    before = ops.LAYOUT_COPIES
    y, ent, parts = run(x, target, sym, want_entropy=want_entropy, want_parts=True)
    assert ops.LAYOUT_COPIES == before
    assert is_cl(y) and y.dtype == x.dtype and y.shape == x.shape
    if half1:
        check_table(x, parts['stats'], True)
    check_given_table(x, y, ent, parts, target, sym)
    return y, ent, parts


def route(x, hist):
    L, ops = mods()
    out = (ctypes.c_int32 * 6)()
    C = x.shape[1]
    align = (x.data_ptr() | 16) & -(x.data_ptr() | 16)               # y is a fresh allocation: x's alignment decides
    assert L.load().cnnq_pc_route_midtread_nhwc(x.numel() // C, C, ops._DTYPE_CODES[x.dtype], align, int(hist), out) == 0
    return list(out)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('case', WIDTH_CASES, ids=lambda c: 'C%d+%d' % c[:2])
def test_every_piece_width(case, dtype):
    C, offset, w32, w16 = case
    want = w32 if dtype == torch.float32 else w16
    # R = 98 takes the fp64 sums, R = 6272 the four-row fp32 partial sums (4096 rows is the border)
    for shape in ((2, C, 7, 7), (8, C, 28, 28)):
        for sym in (True, False):
            x = cl(values(shape, seed=C + offset + sym, positive=not sym), dtype, offset)
            for hist in (False, True):
                r = route(x, hist)
                assert r[0] == want and r[5] == 1, (shape, dtype, offset, r, want)
                check(x, 4, sym, hist)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('shape', [(3, 5, 7, 9), (1, 2, 4, 4), (1, 3, 1, 2), (2, 2048, 7, 7)], ids=lambda s: 'x'.join(map(str, s)))
def test_ragged_and_tiny(shape, dtype):
    for target, sym, offset in ((3, False, 0), (2, True, 1), (4, True, 3)):
        x = cl(values(shape, seed=int(target) + offset, positive=not sym), dtype, offset)
        check(x, target, sym, True)
        check(x, target, sym, False)


def laplace_like(shape, seed, spread, sym):
    """The generator of tests/test_midtread_hist_gpu.py."""
    g = torch.Generator(device='cuda').manual_seed(seed)
    C = shape[1]
    scale = (1 + spread * torch.arange(C, device='cuda').view(1, C, 1, 1) / max(C - 1, 1))
    x = torch.empty(shape, device='cuda').exponential_(generator=g) * scale
    x = x * torch.where(torch.rand(shape, device='cuda', generator=g) < 0.5, -1.0, 1.0)
    return x if sym else x.clamp(min=0)


def entropy_of(codes):
    """utils/entropy.py:8-15 on the device codes (fp64)."""
    _, counts = torch.unique(codes.flatten(), return_counts=True)
    p = counts.double() / codes.numel()
    return float(-(p * torch.log2(p)).sum())


def check_entropy_against_unique(x, ent, parts):
    _, codes, _, _ = nchw_kernel(x, parts['mt'], want_codes=True)
    ref = entropy_of(codes)
    assert abs(float(ent) - ref) < 2e-4 * max(1.0, ref), (float(ent), ref)
    return ref


# shape, target, sym, scale spread, the flag word is raised
REGIMES = [((16, 32, 28, 28), 4.0, False, 1.0, False),     # every code inside the window
           ((16, 32, 28, 28), 4.0, True, 1.0, False),      # symmetric: negative clamp bounds, the window starts below zero
           ((8, 16, 14, 14), 8.0, False, 1.0, True),       # ~256 bins per channel: codes beyond the 128-code window
           ((8, 16, 14, 14), 9.0, True, 4.0, True)]        # ~512 bins, wide spread of channel scales


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('shape,target,sym,spread,flagged', REGIMES)
def test_histogram_regimes(shape, target, sym, spread, flagged, dtype):
    L, _ = mods()
    x = cl(laplace_like(shape, int(target * 100) + shape[1], spread, sym), dtype, 0)
    y, ent, parts = check(x, target, sym, True)
    assert (int(parts['hist'][-1]) != 0) == flagged
    w0 = int(parts['mt'][L.MT_WSTART][0])
    assert (w0 < 0) == sym
    check_entropy_against_unique(x, ent, parts)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_zero_code_outside_the_window(dtype):
    """A symmetric clip with ~512 bins per channel puts code 0 beyond the window: the register-counted zeros go to the global bins
    and raise the flag word (tests/test_midtread_hist_gpu.py's mostly-zero tensor)."""
    L, _ = mods()
    g = torch.Generator(device='cuda').manual_seed(11)
    x = torch.zeros(8, 16, 14, 14, device='cuda')
    mask = torch.rand(x.shape, device='cuda', generator=g) < 0.02
    x[mask] = torch.randn(int(mask.sum()), device='cuda', generator=g) * 0.01
    x = cl(x, dtype, 0)
    y, ent, parts = check(x, 9.0, True, True)
    assert int(parts['mt'][L.MT_WSTART][0]) + L.MT_HIST_WINDOW <= 0
    assert int(parts['hist'][-1]) != 0 and int(parts['hist'][L.MT_HIST_BINS // 2]) > 0
    assert check_entropy_against_unique(x, ent, parts) > 0.05


def special_cases(dtype):
    """name -> (tensor, the channels a special value touches)"""
    def base():
        return values((4, 16, 7, 7), seed=9)
    cases = {}
    x = base()
    x[1, 0, 2, 3] = float('nan')
    cases['nan'] = (x, [0])
    x = base()
    x[0, 1, 0, 0] = float('inf')
    cases['+inf'] = (x, [1])
    x = base()
    x[2, 2, 1, 1] = float('-inf')
    cases['-inf'] = (x, [2])
    x = base()
    x[3, 3, 4, 4] = float('inf')
    x[3, 3, 5, 5] = float('-inf')
    cases['both'] = (x, [3])
    if dtype == torch.float16:
        x = base()
        x[1, 4] *= 1e5                          # beyond 65504: inf in fp16
        cases['overflow'] = (x, [4])
    x = base()
    x[:, 5] = 1.25
    cases['constant'] = (x, [5])
    return cases


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_special_values(dtype):
    L, ops = mods()
    import numpy as np
    from test_channels_last_aciq_gpu import RTOL_STAT, ref_extrema
    for name, (x, special) in special_cases(dtype).items():
        finite = [c for c in range(16) if c not in special]
        xc = cl(x, dtype, 1)
        xf = xc.contiguous().float()
        for sym in (True, False):
            y, ent, parts = check(xc, 4, sym, True, half1=False)
            s = parts['stats'].cpu()
            mn, mx = ref_extrema(xf.cpu())
            assert same(s[L.STAT_MIN], mn) and same(s[L.STAT_MAX], mx), name
            # the non-finite pattern of the table is the NCHW chain's on the same values
            sn = ops.pc_stats(xf, 4, 16, 49, need_b=True, local_only=True)[0].cpu()
            for row in (L.STAT_MIN, L.STAT_MAX, L.STAT_MEAN, L.STAT_STD, L.STAT_B):
                assert torch.equal(torch.isnan(s[row]), torch.isnan(sn[row])), (name, row)
                assert torch.equal(torch.isinf(s[row]), torch.isinf(sn[row])), (name, row)
            # the channels without a special value keep their statistics
            t64 = xf.cpu().double().transpose(0, 1).reshape(16, -1)[finite]
            np.testing.assert_allclose(s[L.STAT_MEAN][finite].double(), t64.mean(1), rtol=RTOL_STAT, atol=1e-7)
            np.testing.assert_allclose(s[L.STAT_STD][finite].double(), t64.std(1, unbiased=True), rtol=RTOL_STAT, atol=0)
            b64 = (t64 - s[L.STAT_MEAN][finite].double()[:, None]).abs().mean(1)
            np.testing.assert_allclose(s[L.STAT_B][finite].double(), b64, rtol=RTOL_STAT, atol=1e-9)
            if name == 'constant':
                # a constant channel is ONE value, counted once: the other channels quantize as usual
                assert torch.isfinite(y.float()).all()
                assert y[:, 5].float().unique().numel() == 1
                check_entropy_against_unique(xc, ent, parts)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_stats_table_form(dtype):
    L, ops = mods()
    for shape, offset in (((8, 24, 14, 14), 0), ((4, 7, 7, 7), 1), ((2, 64, 28, 28), 3)):
        x = cl(values(shape, seed=11), dtype, offset)
        N, C, H, W = shape
        xf = x.float()
        table = torch.zeros((L.NSTAT, C), dtype=torch.float32, device='cuda')
        table[L.STAT_MIN] = xf.amin(dim=(0, 2, 3)) * 0.8
        table[L.STAT_MAX] = xf.amax(dim=(0, 2, 3)) * 0.9
        table[L.STAT_MEAN] = xf.mean(dim=(0, 2, 3))
        table[L.STAT_STD] = xf.std(dim=(0, 2, 3)) * 1.1
        table[L.STAT_B] = (xf - table[L.STAT_MEAN].view(1, C, 1, 1)).abs().mean(dim=(0, 2, 3)) * 0.9
        for sym, want_entropy in ((True, True), (False, False), (False, True)):
            before = ops.LAYOUT_COPIES
            y, ent, parts = run(x, 4, sym, want_entropy=want_entropy, stats=table, want_parts=True)
            assert ops.LAYOUT_COPIES == before and is_cl(y) and y.dtype == dtype
            assert parts['stats'] is table
            check_given_table(x, y, ent, parts, 4, sym)
            out = torch.empty_like(x)
            y2, ent2 = run(x, 4, sym, want_entropy=want_entropy, stats=table, out=out)
            assert y2 is out and same(out, y) and (ent is None or same_scalar(ent, ent2))
    with pytest.raises(L.CnnqError):
        run(x, 4, True, stats=table[:, :8].contiguous())


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_deterministic_out_placement_and_cached_workspace(dtype):
    for shape, offset in (((16, 64, 14, 14), 0), ((3, 5, 28, 28), 1), ((4, 2048, 7, 7), 0)):
        x = cl(values(shape, seed=21), dtype, offset)
        y1, e1, p1 = run(x, 4, True, want_entropy=True, want_parts=True)
        y2, e2, p2 = run(x, 4, True, want_entropy=True, want_parts=True)
        n = p1['hist'].numel() - 1 - 256 * 128
        assert same(y1, y2) and same_scalar(e1, e2) and same(p1['stats'], p2['stats']) and same(p1['mt'], p2['mt'])
        assert torch.equal(p1['hist'][:n], p2['hist'][:n])
        # the hot forms (tables in the cached workspace; entropy without parts) give the same bits
        y3, e3 = run(x, 4, True)
        assert e3 is None and same(y3, y1)
        y4, e4 = run(x, 4, True, want_entropy=True)
        assert same(y4, y1) and same_scalar(e4, e1)
        # another placement of y, with the alignment x has (the piece width is a function of both pointers' alignment)
        _, c, h, w = shape
        base = torch.zeros(x.numel() + 64 + offset, dtype=dtype, device='cuda')
        out = base.as_strided(x.shape, (h * w * c, 1, w * c, c), offset + 16 // x.element_size() * 3)
        y5, e5, p5 = run(x, 4, True, want_entropy=True, want_parts=True, out=out)
        assert y5 is out and same(y5, y1) and same_scalar(e5, e1) and same(p5['stats'], p1['stats'])


@pytest.mark.parametrize('hist', [False, True], ids=['plain', 'hist'])
@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
def test_out_at_another_alignment_narrows_the_piece(dtype, hist):
    """A 16-byte aligned x with C % 8 == 0 and an `out` one element further into its storage: the piece width follows the
    alignment BOTH pointers share, so it drops (fp32: 4 -> 1, bf16: 8 -> 1) and y is stored at that width.  The sums follow W's
    order: the table is held to half 1, not to the aligned run's bits; everything behind it to half 2."""
    L, ops = mods()
    shape = (8, 64, 28, 28)
    n, c, h, w = shape
    x = cl(values(shape, seed=31), dtype, 0)
    assert x.data_ptr() % 16 == 0
    base = torch.zeros(x.numel() + 64, dtype=dtype, device='cuda')
    assert base.data_ptr() % 16 == 0
    out = base.as_strided(x.shape, (h * w * c, 1, w * c, c), 1)
    es = x.element_size()
    common = es                                                         # the power of two dividing both addresses: one element
    assert (x.data_ptr() | out.data_ptr()) & -(x.data_ptr() | out.data_ptr()) == common
    r = (ctypes.c_int32 * 6)()
    dt = ops._DTYPE_CODES[dtype]
    assert L.load().cnnq_pc_route_midtread_nhwc(n * h * w, c, dt, 16, int(hist), r) == 0
    wide = r[0]
    assert L.load().cnnq_pc_route_midtread_nhwc(n * h * w, c, dt, common, int(hist), r) == 0
    assert wide == 16 // es and r[0] == 1, (wide, r[0])
    for sym in (True, False):
        y, ent, parts = run(x, 4, sym, want_entropy=hist, want_parts=True, out=out)
        assert y is out and is_cl(y) and y.dtype == dtype
        check_table(x, parts['stats'], True)
        check_given_table(x, y, ent, parts, 4, sym)
    assert not base[0].item() and not base[x.numel() + 1:].any()       # nothing stored outside out
    # and an out two elements in (bf16: W = 2, fp32: W = 2)
    out2 = base.as_strided(x.shape, (h * w * c, 1, w * c, c), 2)
    assert L.load().cnnq_pc_route_midtread_nhwc(n * h * w, c, dt, 2 * es, int(hist), r) == 0 and r[0] == 2
    base.zero_()
    y, ent, parts = run(x, 4, True, want_entropy=hist, want_parts=True, out=out2)
    check_table(x, parts['stats'], True)
    check_given_table(x, y, ent, parts, 4, True)
    assert not base[:2].any() and not base[x.numel() + 2:].any()


def test_out_must_match():
    L, ops = mods()
    x = cl(values((2, 8, 7, 7)), torch.float32)
    with pytest.raises(L.CnnqError):
        run(x, 4, True, out=torch.empty(x.shape, device='cuda'))        # NCHW
    with pytest.raises(L.CnnqError):
        run(x, 4, True, out=x)
    with pytest.raises(L.CnnqError):
        run(x, float('nan'), True)                                      # the C side refuses a target that is not finite


def test_inside_an_entropy_batch():
    """Two channels_last tensors and one NCHW mid-tread tensor in one block: one entropy launch at its end, the per-tensor values."""
    L, ops = mods()
    a = cl(values((8, 32, 14, 14), seed=1), torch.bfloat16)
    b = cl(values((4, 20, 7, 7), seed=2, positive=True), torch.float32, 1)
    c = values((4, 16, 14, 14), seed=3).cuda()
    ya, ea = run(a, 4, True, want_entropy=True)
    yb, eb = run(b, 3, False, want_entropy=True)
    yc, ec = ops.mid_tread_qdq(c, 4, clip=True, sym=True, group=False, want_entropy=True)
    with ops.entropy_batch() as eb_block:
        ya2, ea2 = run(a, 4, True, want_entropy=True)
        yb2, eb2 = run(b, 3, False, want_entropy=True)
        yc2, ec2 = ops.mid_tread_qdq(c, 4, clip=True, sym=True, group=False, want_entropy=True)
        assert len(eb_block.mt) >= 2                                    # nothing launched yet: they wait for the block's end
    assert same(ya2, ya) and same(yb2, yb) and same(yc2, yc)
    assert same_scalar(ea2, ea) and same_scalar(eb2, eb) and same_scalar(ec2, ec)
    assert float(ea) > 0 and float(eb) > 0


class Logger:
    def __init__(self):
        self.rows = []

    def log_metric(self, name, value, step=None, meterId=None, weight=None):
        self.rows.append((name, value, meterId, weight))


def quantizer(**kw):
    return Q.quantizer(**dict(dict(clipping='laplace', pcq_act=True, bit_alloc_act=True, bit_alloc_target_act=5.3, mtd_quant=True), **kw))


@pytest.mark.parametrize('me', [False, True], ids=['plain', 'me'])
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32], ids=['bf16', 'f32'])
def test_through_the_quantizer(monkeypatch, dtype, me):
    L, ops = mods()
    iq = importlib.import_module('cnn_quantization_amd.qtypes.int_quantizer')
    x = cl(values((8, 32, 14, 14), seed=6), dtype, 0 if dtype == torch.bfloat16 else 1)
    log = Logger()
    q = quantizer(measure_entropy=me, logger=log)
    fb, copies = iq.HALF_FALLBACKS, ops.LAYOUT_COPIES
    y = q(x, 'act')
    assert is_cl(y) and y.dtype == dtype and y.shape == x.shape
    assert iq.HALF_FALLBACKS == fb and ops.LAYOUT_COPIES == copies
    y_ref, e_ref = run(x, 5.3, True, want_entropy=me)
    assert same(y, y_ref)
    if me:
        assert len(log.rows) == 1 and log.rows[0][0] == 'act.entropy' and log.rows[0][2] == 'avg.entropy.act'
        assert log.rows[0][1] == float(e_ref) and log.rows[0][3] == x.numel()
    else:
        assert not log.rows
    q.force_positive = True
    xp = cl(values((8, 32, 14, 14), seed=6, positive=True), dtype)
    assert same(q(xp, 'act'), run(xp, 5.3, False)[0])
    q.force_positive = False
    assert same(q(x, 'act', override_att=('clipping', 'gaus')), y_ref)          # mid-tread clips by the Laplace prior either way
    assert iq.HALF_FALLBACKS == fb and ops.LAYOUT_COPIES == copies
    # with each of these the old route is taken and counted as before
    half = int(dtype != torch.float32)

    def old_route(qq):
        fb, copies = iq.HALF_FALLBACKS, ops.LAYOUT_COPIES
        yo = qq(x, 'act')
        assert (iq.HALF_FALLBACKS, ops.LAYOUT_COPIES) == (fb + half, copies + 1)
        assert yo.is_contiguous() and yo.dtype == dtype and yo.shape == x.shape
    monkeypatch.setenv('CNNQ_NHWC', '0')
    ops.reload_switches()
    try:
        old_route(q)
    finally:
        monkeypatch.delenv('CNNQ_NHWC')
        ops.reload_switches()
    q.fuse_bcorr = False                                    # a pending request (the relu-first flag)
    old_route(q)
    q.fuse_bcorr = None
    q.group = False
    old_route(q)
    q.group = None
    assert is_cl(q(x, 'act'))
    # an NCHW tensor behaves as before
    fb, copies = iq.HALF_FALLBACKS, ops.LAYOUT_COPIES
    yn = q(x.contiguous(), 'act')
    assert yn.is_contiguous() and (iq.HALF_FALLBACKS, ops.LAYOUT_COPIES) == (fb + half, copies)


def test_op_fallback_is_the_counted_copy(monkeypatch):
    L, ops = mods()
    x = cl(values((4, 16, 14, 14), seed=4), torch.float32)
    monkeypatch.setenv('CNNQ_NHWC', '0')
    ops.reload_switches()
    try:
        before = ops.LAYOUT_COPIES
        y, ent = run(x, 4, True, want_entropy=True)
        assert ops.LAYOUT_COPIES == before + 1 and y.is_contiguous()
        y_ref, e_ref = ops.mid_tread_qdq(x.contiguous(), 4, clip=True, sym=True, group=False, want_entropy=True)
        assert same(y, y_ref) and same_scalar(ent, e_ref)
        xh, before = x.bfloat16(), ops.LAYOUT_COPIES
        with pytest.raises(L.CnnqError):
            run(xh, 4, True)                                # the NCHW chain has no half kernels for config 5: an error ...
        assert ops.LAYOUT_COPIES == before                  # ... raised before anything is copied or counted
    finally:
        monkeypatch.delenv('CNNQ_NHWC')
        ops.reload_switches()
    # an NCHW tensor: mid_tread_qdq, no copy
    before = ops.LAYOUT_COPIES
    y2, _ = run(x.contiguous(), 4, True)
    assert ops.LAYOUT_COPIES == before and same(y2, y_ref)


def test_graph_capture_replays_eager():
    x = cl(values((16, 64, 14, 14), seed=2), torch.bfloat16)
    eager = run(x, 4, True)[0]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run(x, 4, True)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = run(x, 4, True)[0]
    x.copy_(cl(values((16, 64, 14, 14), seed=3), torch.bfloat16))
    graph.replay()
    torch.cuda.synchronize()
    assert is_cl(y) and same(y, run(x, 4, True)[0])
    assert not same(y, eager)


CFG = dict(max_examples=40, deadline=None, derandomize=True, suppress_health_check=list(HealthCheck))


@settings(**CFG)
@given(n=st.integers(1, 9), c=st.integers(2, 70), h=st.integers(1, 9), w=st.integers(1, 9), offset=st.integers(0, 7),
       dt=st.sampled_from([0, 1, 2]), sym=st.booleans(), target=st.sampled_from([2, 3, 4, 5.3]), hist=st.booleans(),
       seed=st.integers(0, 1 << 16))
def test_fuzz(n, c, h, w, offset, dt, sym, target, hist, seed):
    assume(h * w > 1)
    x = cl(values((n, c, h, w), seed=seed, positive=not sym), DTYPES[dt], offset)
    y, ent, parts = run(x, target, sym, want_entropy=hist, want_parts=True)
    assert is_cl(y) and y.dtype == x.dtype
    check_given_table(x, y, ent, parts, target, sym)
