"""Config 3 (ACIQ clipping, bit allocation) on dense channels_last activations, fp32 / bf16 / fp16.

The per-channel sums are added in an order fixed by the NHWC geometry - not the NCHW chain's - so equality with the NCHW path is
not the contract.  The contract has two halves:
  1. the table: `stats` from the device against fp64 on x.float() - MIN / MAX bit-equal, MEAN / STD / B within RTOL_STAT = 2e-6
     (absolute floors 1e-7 for the mean, 1e-9 for b: those of tests/test_aciq_single_gpu.py), B around the device's fp32 mean;
  2. given the table, bit for bit: y equals pc_qdq(x.contiguous().float(), pc_params(table)) cast to x's dtype, qp and diag equal
     pc_params(table)'s; for Laplace clipping with and without bit allocation on the std prior also the oracle on the table."""
import importlib

import numpy as np
import pytest
import torch
from hypothesis import HealthCheck, given, settings
from hypothesis import strategies as st

import _quantizer as Q
from _direct import aciq_on_table
from test_channels_last_gpu import DTYPES, IDS, cl, is_cl, same, values

pytestmark = pytest.mark.gpu
RTOL_STAT = 2e-6


def mods():
    from cnn_quantization_amd import _lib as L, ops
    return L, ops


def run(x, bits, positive=False, clip='laplace', ba=False, prior_b=False, rmode=True, **kw):
    L, ops = mods()
    return ops.aciq_qdq_nhwc(x, bits, positive=positive, clip=clip, bit_alloc=ba, prior_is_b=prior_b, round_mode=rmode, **kw)


def ref_extrema(xf):
    """Per-channel min / max of NCHW xf with torch's NaN rule."""
    nan = torch.isnan(xf).any(dim=(0, 2, 3))
    nanv = torch.full_like(xf[0, :, 0, 0], float('nan'))
    return torch.where(nan, nanv, xf.amin(dim=(0, 2, 3))), torch.where(nan, nanv, xf.amax(dim=(0, 2, 3)))


def check_table(x, stats, need_b):
    """Half 1 on the CPU in fp64."""
    L, _ = mods()
    xf = x.contiguous().float().cpu()
    C = xf.shape[1]
    s = stats.cpu()
    mn, mx = ref_extrema(xf)
    assert same(s[L.STAT_MIN], mn) and same(s[L.STAT_MAX], mx)
    t64 = xf.double().transpose(0, 1).reshape(C, -1)
    np.testing.assert_allclose(s[L.STAT_MEAN].double(), t64.mean(1), rtol=RTOL_STAT, atol=1e-7)
    np.testing.assert_allclose(s[L.STAT_STD].double(), t64.std(1, unbiased=True), rtol=RTOL_STAT, atol=0)
    if need_b:
        b64 = (t64 - s[L.STAT_MEAN].double()[:, None]).abs().mean(1)
        np.testing.assert_allclose(s[L.STAT_B].double(), b64, rtol=RTOL_STAT, atol=1e-9)
    else:
        assert not s[L.STAT_B].any()
    assert not s[L.STAT_KURT].any() and not s[L.STAT_STD_POS].any()


def check_given_table(x, y, parts, bits, positive, clip, ba, prior_b, rmode, oracle=True):
    """Half 2: everything behind the table, bit for bit."""
    L, ops = mods()
    N, C, H, W = x.shape
    stt, qp, diag = parts['stats'], parts['qp'], parts['diag']
    use_ba = ba and bits <= 4
    qp_ref, diag_ref = ops.pc_params(stt, bits, positive, clip, use_ba, prior_b, None, rmode)
    assert same(qp, qp_ref) and same(diag, diag_ref)
    xc = x.contiguous().float()
    y_ref = ops.pc_qdq(xc, N, C, H * W, qp_ref).to(x.dtype)
    assert same(y, y_ref), (tuple(x.shape), x.dtype, bits, positive, clip, ba, prior_b, rmode, x.storage_offset())
    if oracle and clip == 'laplace' and rmode and not (use_ba and prior_b):
        ref = aciq_on_table(xc.cpu(), stt, diag[L.DIAG_BITS], bits, positive, use_ba)
        assert same(diag[L.DIAG_ALPHA].cpu(), ref['alpha'])
        assert same(diag[L.DIAG_DELTA].cpu(), ref['delta']) and same(diag[L.DIAG_OFFSET].cpu(), ref['offset'])
        assert same(qp[L.QP_SCALE].cpu(), ref['scale']) and same(qp[L.QP_ZP].cpu(), ref['zp'])
        assert same(y.cpu(), ref['y'].to(x.dtype))


def check(x, bits, positive=False, clip='laplace', ba=False, prior_b=False, rmode=True, oracle=True):
    L, ops = mods()
    before = ops.LAYOUT_COPIES
    y, parts = run(x, bits, positive, clip, ba, prior_b, rmode, want_parts=True)
    assert ops.LAYOUT_COPIES == before
    assert is_cl(y) and y.dtype == x.dtype and y.shape == x.shape
    need_b = clip == 'laplace' or (ba and bits <= 4 and prior_b)
    check_table(x, parts['stats'], need_b)
    check_given_table(x, y, parts, bits, positive, clip, ba, prior_b, rmode, oracle)
    # the hot form (tables in the cached workspace) gives the same bits
    assert same(run(x, bits, positive, clip, ba, prior_b, rmode), y)
    return y, parts


SHAPES = [(N, C, H, W) for N in (1, 3, 32) for C in (3, 5, 64, 2048) for (H, W) in ((1, 2), (7, 7), (14, 14), (56, 56))
          if N * C * H * W <= (1 << 24)]
# (bits, positive, storage offset, clip, bit allocation, b prior, round)
COMBOS = [(4, False, 0, 'laplace', False, False, True), (4, True, 1, 'laplace', True, False, True),
          (8, False, 3, 'gaus', False, False, True), (2, True, 0, 'laplace', True, True, False),
          (3, False, 1, 'gaus', True, False, False), (4, False, 3, 'gaus', True, True, True)]


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_shapes(shape, dtype):
    for bits, positive, offset, clip, ba, prior_b, rmode in COMBOS:
        check(cl(values(shape, seed=bits + offset, positive=positive), dtype, offset), bits, positive, clip, ba, prior_b, rmode)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_all_bit_widths_and_modes(dtype):
    for offset, shape in ((0, (4, 24, 7, 7)), (1, (4, 24, 7, 7)), (3, (3, 10, 14, 14))):
        for positive in (False, True):
            x = cl(values(shape, seed=5 + offset, positive=positive), dtype, offset)
            for bits in range(2, 9):
                for clip in ('laplace', 'gaus'):
                    for ba, prior_b in ((False, False), (True, False), (True, True)):
                        for rmode in (True, False):
                            if not ba and not rmode:
                                continue
                            check(x, bits, positive, clip, ba, prior_b, rmode)


# Every piece width W of every dtype with the full check (halves 1 and 2), on both summation paths: the channel counts of SHAPES
# at offsets 0 / 1 / 3 only reach W = 1 and the widest W.  (C, storage offset in elements) -> W for fp32, W for bf16 / fp16:
WIDTH_CASES = [(6, 0, 2, 2), (10, 0, 2, 2), (12, 0, 4, 4), (20, 0, 4, 4), (64, 2, 2, 2), (64, 4, 4, 4), (64, 0, 4, 8), (7, 0, 1, 1)]


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('case', WIDTH_CASES, ids=lambda c: 'C%d+%d' % c[:2])
def test_every_piece_width_on_both_summation_paths(case, dtype):
    import ctypes
    L, ops = mods()
    C, offset, w32, w16 = case
    want = w32 if dtype == torch.float32 else w16
    out = (ctypes.c_int32 * 6)()
    # R = 6272 and 9408 take the four-row fp32 partial sums, R = 588 and 98 the fp64 sums (4096 rows is the border)
    for shape in ((8, C, 28, 28), (3, C, 56, 56), (3, C, 14, 14), (2, C, 7, 7)):
        for bits, positive, clip, ba, prior_b in ((4, False, 'laplace', True, False), (4, True, 'gaus', True, True)):
            x = cl(values(shape, seed=C + offset + bits, positive=positive), dtype, offset)
            align = (x.data_ptr() | 16) & -(x.data_ptr() | 16)           # y is a fresh allocation: x's alignment decides
            R = x.numel() // C
            assert L.load().cnnq_pc_route_aciq_nhwc(R, C, ops._DTYPE_CODES[dtype], align, out) == 0
            assert out[0] == want, (shape, dtype, offset, out[0], want)
            check(x, bits, positive, clip, ba, prior_b, True)


def test_other_clippings_raise():
    L, ops = mods()
    x = cl(values((2, 8, 7, 7)), torch.float32)
    for clip in ('no', 'mix', '2std'):
        with pytest.raises(L.CnnqError):
            ops.aciq_qdq_nhwc(x, 4, clip=clip)
    with pytest.raises(L.CnnqError):
        ops.aciq_qdq_nhwc(x, 9)                            # the ACIQ tables end at 8 bits


def quantizer(**kw):
    return Q.quantizer(**dict(dict(clipping='laplace', pcq_act=True, bit_alloc_act=True), **kw))


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_ab_switch_takes_the_copy_route(monkeypatch, dtype):
    """CNNQ_NHWC=0: the quantizer is back on the parent route - one counted copy (and for bf16 / fp16 the upcast), an NCHW result."""
    L, ops = mods()
    iq = importlib.import_module('cnn_quantization_amd.qtypes.int_quantizer')
    x = cl(values((8, 32, 14, 14), seed=4), dtype)
    q = quantizer()
    before, fb = ops.LAYOUT_COPIES, iq.HALF_FALLBACKS
    native = q(x, 'a')
    assert is_cl(native) and native.dtype == dtype and (ops.LAYOUT_COPIES, iq.HALF_FALLBACKS) == (before, fb)
    monkeypatch.setenv('CNNQ_NHWC', '0')
    ops.reload_switches()
    try:
        y = q(x, 'a')
        assert ops.LAYOUT_COPIES == before + 1
        assert iq.HALF_FALLBACKS == fb + (dtype != torch.float32)
        assert y.is_contiguous() and y.dtype == dtype and y.shape == x.shape
        if dtype == torch.float32:
            y2 = run(x, 4, ba=True)                         # the op itself: copied, counted, the NCHW chain's result
            assert ops.LAYOUT_COPIES == before + 2 and y2.is_contiguous() and same(y2, y)
        else:
            with pytest.raises(L.CnnqError):                # the NCHW chain has no half kernels for config 3: an error
                run(x, 4, ba=True)
    finally:
        monkeypatch.delenv('CNNQ_NHWC')
        ops.reload_switches()
    assert is_cl(q(x, 'a'))


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_stats_table(dtype):
    """-sm use: the parameters from a calibration table."""
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
        for clip, ba, prior_b in (('laplace', False, False), ('gaus', True, False), ('laplace', True, True)):
            before = ops.LAYOUT_COPIES
            y, parts = run(x, 4, clip=clip, ba=ba, prior_b=prior_b, stats=table, want_parts=True)
            assert ops.LAYOUT_COPIES == before and is_cl(y) and y.dtype == dtype
            assert parts['stats'] is table
            qp, diag = ops.pc_params(table, 4, False, clip, ba, prior_b)
            assert same(parts['qp'], qp) and same(parts['diag'], diag)
            ref = ops.pc_qdq(x.contiguous().float(), N, C, H * W, qp).to(dtype)
            assert same(y, ref)
            out = torch.empty_like(x)
            assert run(x, 4, clip=clip, ba=ba, prior_b=prior_b, stats=table, out=out) is out and same(out, ref)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_special_values(dtype):
    L, ops = mods()
    x = values((4, 16, 7, 7), seed=9)
    x[1, 0, 2, 3] = float('nan')
    x[0, 1, 0, 0] = float('inf')
    x[2, 2, 1, 1] = float('-inf')
    x[3, 3, 4, 4] = float('inf')
    x[3, 3, 5, 5] = float('-inf')
    special = [0, 1, 2, 3]
    if dtype == torch.float16:
        x[1, 4] *= 1e5                      # beyond 65504: inf in fp16
        special.append(4)
    finite = [c for c in range(16) if c not in special]
    xc = cl(x, dtype, 1)
    xf = xc.contiguous().float()
    for bits, positive, clip, ba in ((4, False, 'laplace', False), (4, True, 'gaus', False), (8, False, 'laplace', False),
                                     (4, False, 'laplace', True), (3, False, 'gaus', True)):
        y, parts = run(xc, bits, positive, clip, ba, want_parts=True)
        assert is_cl(y)
        check_given_table(xc, y, parts, bits, positive, clip, ba, False, True, oracle=False)
        s = parts['stats'].cpu()
        mn, mx = ref_extrema(xf.cpu())
        assert same(s[L.STAT_MIN], mn) and same(s[L.STAT_MAX], mx)
        assert torch.isnan(s[[L.STAT_MIN, L.STAT_MAX, L.STAT_MEAN]][:, 0]).all()
        # the channels without a special value keep their statistics
        t64 = xf.cpu().double().transpose(0, 1).reshape(16, -1)[finite]
        np.testing.assert_allclose(s[L.STAT_MEAN][finite].double(), t64.mean(1), rtol=RTOL_STAT, atol=1e-7)
        np.testing.assert_allclose(s[L.STAT_STD][finite].double(), t64.std(1, unbiased=True), rtol=RTOL_STAT, atol=0)
        if dtype == torch.float32:
            # the NCHW chain on the same values: the same non-finite pattern in the table, and - without bit allocation, which
            # a NaN / Inf statistic poisons for every channel in both - in the result
            _, pn = ops.act_qdq_per_channel(xf, bits, positive=positive, clip=clip, bit_alloc=ba, want_parts=True, group=False)
            sn = pn['stats'].cpu()
            for row in (L.STAT_MIN, L.STAT_MAX, L.STAT_MEAN, L.STAT_STD) + ((L.STAT_B,) if clip == 'laplace' else ()):
                assert torch.equal(torch.isnan(s[row]), torch.isnan(sn[row])), row
                assert torch.equal(torch.isinf(s[row]), torch.isinf(sn[row])), row
            assert torch.equal(s[L.STAT_MIN][finite], sn[L.STAT_MIN][finite])
            assert torch.equal(s[L.STAT_MAX][finite], sn[L.STAT_MAX][finite])
            if not ba:
                yn = ops.act_qdq_per_channel(xf, bits, positive=positive, clip=clip, group=False)
                assert torch.equal(torch.isnan(y.contiguous()), torch.isnan(yn))
                assert torch.isfinite(y.contiguous()[:, finite]).all()


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_deterministic_and_out_placement(dtype):
    for shape, offset in (((16, 64, 14, 14), 0), ((3, 5, 56, 56), 1), ((32, 2048, 7, 7), 0)):
        x = cl(values(shape, seed=21), dtype, offset)
        y1, p1 = run(x, 4, ba=True, want_parts=True)
        y2, p2 = run(x, 4, ba=True, want_parts=True)
        assert same(y1, y2) and all(same(p1[k], p2[k]) for k in ('stats', 'qp', 'diag'))
        # another placement of y, with the alignment x has (the piece width is a function of both pointers' alignment)
        n, c, h, w = shape
        esize = x.element_size()
        base = torch.zeros(x.numel() + 64 + offset, dtype=dtype, device='cuda')
        out = base.as_strided(x.shape, (h * w * c, 1, w * c, c), offset + 16 // esize * 3)
        y3, p3 = run(x, 4, ba=True, want_parts=True, out=out)
        assert y3 is out and same(y3, y1) and all(same(p1[k], p3[k]) for k in ('stats', 'qp', 'diag'))


def test_out_must_match():
    L, ops = mods()
    x = cl(values((2, 8, 7, 7)), torch.float32)
    with pytest.raises(L.CnnqError):
        run(x, 4, out=torch.empty(x.shape, device='cuda'))          # NCHW
    with pytest.raises(L.CnnqError):
        run(x, 4, out=x)


def test_graph_capture_replays_eager():
    x = cl(values((16, 64, 14, 14), seed=2), torch.bfloat16)
    eager = run(x, 4, ba=True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run(x, 4, ba=True)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = run(x, 4, ba=True)
    x.copy_(cl(values((16, 64, 14, 14), seed=3), torch.bfloat16))
    graph.replay()
    torch.cuda.synchronize()
    assert is_cl(y) and same(y, run(x, 4, ba=True))
    assert not same(y, eager)


def test_through_the_quantizer():
    L, ops = mods()
    q = quantizer()
    iq = importlib.import_module('cnn_quantization_amd.qtypes.int_quantizer')
    x = cl(values((8, 32, 14, 14), seed=6), torch.bfloat16)
    fb, copies = iq.HALF_FALLBACKS, ops.LAYOUT_COPIES
    y = q(x, 'act')
    assert is_cl(y) and y.dtype == torch.bfloat16 and y.shape == x.shape
    assert iq.HALF_FALLBACKS == fb and ops.LAYOUT_COPIES == copies
    assert same(y, run(x, 4, ba=True, prior_b=False))
    q.force_positive = True
    assert same(q(x, 'act'), run(x, 4, positive=True, ba=True))
    q.force_positive = False
    assert same(q(x, 'act', override_att=('clipping', 'gaus')), run(x, 4, clip='gaus', ba=True))
    assert iq.HALF_FALLBACKS == fb and ops.LAYOUT_COPIES == copies
    # fp32 channels_last: native too
    xf = cl(values((8, 32, 14, 14), seed=6), torch.float32, 1)
    yf = q(xf, 'act')
    assert is_cl(yf) and ops.LAYOUT_COPIES == copies and same(yf, run(xf, 4, ba=True))
    # the unchanged routes: NCHW bf16 with clipping upcasts ...
    yn = q(x.contiguous(), 'act')
    assert iq.HALF_FALLBACKS == fb + 1 and yn.is_contiguous() and yn.dtype == torch.bfloat16 and ops.LAYOUT_COPIES == copies
    # ... entropy measurement and a pending bias correction keep the copy, counted
    fb, copies = iq.HALF_FALLBACKS, ops.LAYOUT_COPIES
    qe = quantizer(measure_entropy=True)
    ye = qe(xf, 'act')
    assert ops.LAYOUT_COPIES == copies + 1 and ye.is_contiguous()
    ye = qe(x, 'act')
    assert ops.LAYOUT_COPIES == copies + 2 and iq.HALF_FALLBACKS == fb + 1 and ye.is_contiguous()
    q.fuse_bcorr = False                                    # a pending request (the relu-first flag)
    yb = q(xf, 'act')
    assert q.fuse_bcorr is None and q.bcorr_fused and ops.LAYOUT_COPIES == copies + 3 and yb.is_contiguous()
    # -c mix and mid-tread are not this route
    assert not q._nhwc_aciq(xf, 'mix')
    assert not quantizer(mtd_quant=True)._half_native(x)


def test_quantizer_with_a_statistics_table(monkeypatch):
    """-sm use through the quantizer: the table it builds from the statistics manager, on the channels_last storage."""
    L, ops = mods()
    x = cl(values((4, 16, 14, 14), seed=8), torch.bfloat16)
    xf = x.float()
    C = 16
    rows = {'min': xf.amin(dim=(0, 2, 3)), 'max': xf.amax(dim=(0, 2, 3)), 'mean': xf.mean(dim=(0, 2, 3)),
            'std': xf.std(dim=(0, 2, 3)), 'b': (xf - xf.mean(dim=(0, 2, 3)).view(1, C, 1, 1)).abs().mean(dim=(0, 2, 3))}

    class SM:
        def get_tensor_stat(self, stat_id, stat, kind='mean'):
            return rows[stat].cpu().numpy()
    q = quantizer()
    q.sm = SM
    copies = ops.LAYOUT_COPIES
    y = q(x, 'act', stat_id='layer0')
    assert is_cl(y) and y.dtype == torch.bfloat16 and ops.LAYOUT_COPIES == copies
    table = torch.zeros((L.NSTAT, C), dtype=torch.float32, device='cuda')
    for k, r in (('min', L.STAT_MIN), ('max', L.STAT_MAX), ('mean', L.STAT_MEAN), ('std', L.STAT_STD), ('b', L.STAT_B)):
        table[r] = rows[k]
    assert same(y, run(x, 4, ba=True, stats=table))


def device_values(shape, dtype, seed):
    g = torch.Generator(device='cuda').manual_seed(seed)
    C = shape[1]
    scale = 0.2 + 3 * torch.rand(1, C, 1, 1, generator=g, device='cuda')
    shift = torch.randn(1, C, 1, 1, generator=g, device='cuda')
    x = torch.empty(shape, dtype=dtype, device='cuda', memory_format=torch.channels_last)
    n = max(1, shape[0] // 8)
    for i in range(0, shape[0], n):                          # in pieces: no fp32 copy of the whole tensor
        x[i:i + n] = (torch.randn((min(n, shape[0] - i),) + tuple(shape[1:]), generator=g, device='cuda') * scale + shift).to(dtype)
    return x


def full_size_shapes():
    big = (512, 256, 56, 56)
    try:
        free = torch.cuda.mem_get_info()[0] if torch.cuda.is_available() else 0
    except Exception:
        free = 0
    if free < (40 << 30):
        big = (128, 256, 56, 56)
    return [big, (512, 2048, 7, 7)]


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
@pytest.mark.parametrize('which', [0, 1], ids=['256x56', '2048x7'])
def test_full_size_layers(which, dtype):
    L, ops = mods()
    shape = full_size_shapes()[which]
    N, C, H, W = shape
    x = device_values(shape, dtype, 7)
    assert ops._layout(x) == 'nhwc'
    before = ops.LAYOUT_COPIES
    y, parts = run(x, 4, ba=True, want_parts=True)
    assert ops.LAYOUT_COPIES == before and is_cl(y) and y.dtype == dtype
    s = parts['stats']
    # half 1, per channel in chunks, fp64 on the device
    step = max(1, (1 << 25) // (N * H * W))
    for c0 in range(0, C, step):
        t = x[:, c0:c0 + step].double()
        mean = t.mean(dim=(0, 2, 3))
        std = t.std(dim=(0, 2, 3), unbiased=True)
        b = (t - s[L.STAT_MEAN, c0:c0 + step].double().view(1, -1, 1, 1)).abs().mean(dim=(0, 2, 3))
        tf = x[:, c0:c0 + step].float()
        sl = slice(c0, c0 + step)
        assert torch.equal(s[L.STAT_MIN, sl], tf.amin(dim=(0, 2, 3))) and torch.equal(s[L.STAT_MAX, sl], tf.amax(dim=(0, 2, 3)))
        np.testing.assert_allclose(s[L.STAT_MEAN, sl].double().cpu(), mean.cpu(), rtol=RTOL_STAT, atol=1e-7)
        np.testing.assert_allclose(s[L.STAT_STD, sl].double().cpu(), std.cpu(), rtol=RTOL_STAT, atol=0)
        np.testing.assert_allclose(s[L.STAT_B, sl].double().cpu(), b.cpu(), rtol=RTOL_STAT, atol=1e-9)
        del t, tf
    # half 2
    qp, diag = ops.pc_params(s, 4, False, 'laplace', True, False)
    assert same(parts['qp'], qp) and same(parts['diag'], diag)
    y_ref = ops.pc_qdq(x.contiguous().float(), N, C, H * W, qp).to(dtype)
    assert same(y, y_ref)


CFG = dict(max_examples=40, deadline=None, derandomize=True, suppress_health_check=list(HealthCheck))


@settings(**CFG)
@given(n=st.integers(1, 9), c=st.integers(2, 70), h=st.integers(1, 9), w=st.integers(1, 9), offset=st.integers(0, 7),
       dt=st.sampled_from([0, 1, 2]), bits=st.sampled_from([2, 3, 4, 8]), positive=st.booleans(), gaus=st.booleans(),
       ba=st.sampled_from([0, 1, 2]), rmode=st.booleans(), seed=st.integers(0, 1 << 16))
def test_fuzz(n, c, h, w, offset, dt, bits, positive, gaus, ba, rmode, seed):
    if h * w == 1:
        return
    x = cl(values((n, c, h, w), seed=seed, positive=positive), DTYPES[dt], offset)
    clip = 'gaus' if gaus else 'laplace'
    y, parts = run(x, bits, positive, clip, ba > 0, ba == 2, rmode, want_parts=True)
    assert is_cl(y) and y.dtype == x.dtype
    check_given_table(x, y, parts, bits, positive, clip, ba > 0, ba == 2, rmode)
