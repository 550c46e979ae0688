"""Activation bias correction (-bca, iqm.py:180-196) on dense channels_last activations with a calibration table (DESIGN.md
section 15), fp32 / bf16 / fp16: ops.qdq_bias_corrected_nhwc and the quantizer's route to it.

The per-channel sums are added in an order fixed by the NHWC geometry, so the contract has two halves:
  1. the sums: sum x' and sum q against fp64 on the CPU over x.float() and q = pc_qdq(x.contiguous().float(), qp), within
     RTOL_STAT = 2e-6 of sum |term| per channel (three fp32 roundings in a four-term sum are about 1.8e-7 of it); the count exact;
  2. given the sums, bit for bit (NaN == NaN): bias == (float32(sum x') - float32(sum q)) / (float32(count) + 1e-8f), and
     y.contiguous() == (q + (q > 0) * bias).to(x.dtype), y channels_last, no layout copy and no upcast counted."""
import contextlib
import ctypes
import importlib
import io

import numpy as np
import pytest
import torch

import _quantizer as Q
from oracle import quant_oracle as O
from test_channels_last_gpu import DTYPES, IDS, cl, is_cl, same, values

pytestmark = pytest.mark.gpu
RTOL_STAT = 2e-6


def mods():
    from cnn_quantization_amd import _lib as L, ops
    return L, ops


def iq_mod():
    return importlib.import_module('cnn_quantization_amd.qtypes.int_quantizer')


def calib_table(xf):
    """A calibration-like table of the NCHW fp32 device tensor xf: near the tensor's statistics, but not bounding its values."""
    L, _ = mods()
    C = xf.shape[1]
    table = torch.zeros((L.NSTAT, C), dtype=torch.float32, device='cuda')
    table[L.STAT_MIN] = xf.amin(dim=(0, 2, 3)) * 0.8
    table[L.STAT_MAX] = xf.amax(dim=(0, 2, 3)) * 0.9
    table[L.STAT_MEAN] = xf.mean(dim=(0, 2, 3))
    table[L.STAT_STD] = xf.std(dim=(0, 2, 3)) * 1.1
    table[L.STAT_B] = (xf - table[L.STAT_MEAN].view(1, C, 1, 1)).abs().mean(dim=(0, 2, 3)) * 0.9
    return table


# (clip, bit allocation): min/max, Laplace clipping with bit allocation, Gaussian clipping
PARAMS = {'no': ('no', False), 'laplace_ba': ('laplace', True), 'gaus': ('gaus', False)}


def params(table, bits, positive, kind):
    _, ops = mods()
    clip, ba = PARAMS[kind]
    return ops.pc_params(table, bits, positive, clip, ba and bits <= 4, False)[0]


def same64(a, b):
    """`same` for the float64 sums."""
    na, nb = torch.isnan(a), torch.isnan(b)
    return a.shape == b.shape and torch.equal(na, nb) and torch.equal(a.view(torch.int64)[~na], b.view(torch.int64)[~nb])


def rows(t):
    return t.transpose(0, 1).reshape(t.shape[1], -1)


def close(dev, ref, tol):
    """|dev - ref| <= tol per channel; equal infinities and a NaN on both sides count as equal."""
    return bool(((dev == ref) | ((dev - ref).abs() <= tol) | (torch.isnan(dev) & torch.isnan(ref))).all())


def check(x, qp, relu_first, sums_on=None):
    """Both halves of the contract for one call; sums_on: the channels whose sums are compared (None: all).  Returns y."""
    L, ops = mods()
    iq = iq_mod()
    N, C, H, W = x.shape
    before = (ops.LAYOUT_COPIES, iq.HALF_FALLBACKS)
    y, parts = ops.qdq_bias_corrected_nhwc(x, qp, relu_first, want_parts=True)
    assert (ops.LAYOUT_COPIES, iq.HALF_FALLBACKS) == before
    assert is_cl(y) and y.dtype == x.dtype and y.shape == x.shape
    xf = x.contiguous().float()
    q = ops.pc_qdq(xf, N, C, H * W, qp)
    # half 1
    v64, q64 = rows(xf.cpu().double()), rows(q.cpu().double())
    if relu_first:
        v64 = v64.relu()
    sums = parts['sums'].cpu()
    ch = slice(None) if sums_on is None else sums_on
    for name, dev, t in (('sum x', sums[0], v64), ('sum q', sums[1], q64)):
        ref, mag = t.sum(1), t.abs().sum(1)
        worst = ((dev - ref).abs() / mag.clamp_min(1e-300))[ch]
        worst = worst[torch.isfinite(worst)]
        print('%s %s %s relu=%d: worst |dev - ref| / sum|term| = %.3g' % (name, tuple(x.shape), x.dtype, relu_first,
                                                                          float(worst.max()) if worst.numel() else 0.))
        assert close(dev[ch], ref[ch], RTOL_STAT * mag[ch]), (name, tuple(x.shape), x.dtype, x.storage_offset())
    assert torch.equal(sums[2], (v64 > 0).sum(1).double()), (tuple(x.shape), x.dtype)
    # half 2
    s = sums.numpy()
    with np.errstate(all='ignore'):
        bias_ref = (s[0].astype(np.float32) - s[1].astype(np.float32)) / (s[2].astype(np.float32) + np.float32(1e-8))
    assert same(parts['bias'].cpu(), torch.from_numpy(bias_ref)), (tuple(x.shape), x.dtype)
    y_ref = (q + (q > 0).float() * parts['bias'].view(1, C, 1, 1)).to(x.dtype)
    assert same(y, y_ref), (tuple(x.shape), x.dtype, relu_first, x.storage_offset())
    # the hot form (the bias in the cached workspace) gives the same bits
    assert same(ops.qdq_bias_corrected_nhwc(x, qp, relu_first), y)
    assert (ops.LAYOUT_COPIES, iq.HALF_FALLBACKS) == before
    return y


def case(shape, dtype, offset, bits, positive, relu_first, kind, seed=0):
    x = cl(values(shape, seed=seed, positive=positive), dtype, offset)
    return check(x, params(calib_table(x.contiguous().float()), bits, positive, kind), relu_first)


# one slab and several, several column blocks (C = 2048 in fp32 at 7x7: 512 pieces), H*W = 2, C = 3 and 5; R = 98 ... 100352
SHAPES = [(N, C, H, W) for N in (1, 3, 32) for C in (3, 5, 64, 2048) for (H, W) in ((1, 2), (7, 7), (14, 14), (56, 56))
          if N * C * H * W <= (1 << 24)]
# (bits, positive, storage offset, relu first, parameters)
COMBOS = [(4, False, 0, False, 'laplace_ba'), (8, True, 1, True, 'no'), (2, False, 3, True, 'gaus')]


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_shapes(shape, dtype):
    for i, (bits, positive, offset, relu_first, kind) in enumerate(COMBOS):
        if shape[0] * shape[1] * shape[2] * shape[3] > (1 << 21) and i:
            continue                                        # the large tensors: one combination (the CPU reference is the cost)
        case(shape, dtype, offset, bits, positive, relu_first, kind, seed=bits + offset)


# Every piece width W of every dtype on both summation paths.  (C, storage offset in elements) -> W for fp32, W for bf16 / fp16:
WIDTH_CASES = [(6, 0, 2, 2), (10, 0, 2, 2), (12, 0, 4, 4), (20, 0, 4, 4), (64, 2, 2, 2), (64, 4, 4, 4), (64, 0, 4, 8), (7, 0, 1, 1)]


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('case_', WIDTH_CASES, ids=lambda c: 'C%d+%d' % c[:2])
def test_every_piece_width_on_both_summation_paths(case_, dtype):
    L, ops = mods()
    C, offset, w32, w16 = case_
    want = w32 if dtype == torch.float32 else w16
    out = (ctypes.c_int32 * 6)()
    # R = 6272 and 9408 take the four-row fp32 partial sums, R = 588 and 98 the fp64 sums (4096 rows is the border)
    for shape in ((8, C, 28, 28), (3, C, 56, 56), (3, C, 14, 14), (2, C, 7, 7)):
        for bits, positive, relu_first, kind in ((4, False, False, 'laplace_ba'), (4, True, True, 'no')):
            x = cl(values(shape, seed=C + offset + bits, positive=positive), dtype, offset)
            align = (x.data_ptr() | 16) & -(x.data_ptr() | 16)           # y is a fresh allocation: x's alignment decides
            assert L.load().cnnq_pc_route_aciq_nhwc(x.numel() // C, C, ops._DTYPE_CODES[dtype], align, out) == 0
            assert out[0] == want, (shape, dtype, offset, out[0], want)
            check(x, params(calib_table(x.contiguous().float()), bits, positive, kind), relu_first)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_leftover_rows_and_partial_steps(dtype):
    """Above the border a lane adds four rows at a time: slabs that leave it 0, 1, 2 and 3 rows over, and row counts that are no
    multiple of the rows per step (RS), so that the lanes of one piece walk different numbers of rows."""
    L, ops = mods()
    out = (ctypes.c_int32 * 6)()
    left = set()
    for shape in ((3, 64, 56, 56), (8, 64, 28, 28), (5, 64, 33, 31), (5, 64, 29, 31), (7, 24, 25, 27), (6, 40, 31, 29)):
        N, C, H, W = shape
        R = N * H * W
        assert R > 4096
        x = cl(values(shape, seed=R % 97), dtype, 0)
        assert L.load().cnnq_pc_route_aciq_nhwc(R, C, ops._DTYPE_CODES[dtype], 16, out) == 0
        w, S, rpw, loads = out[0], out[1], out[2], out[3]
        RS = 256 // min(C // w, 256)
        last = R - (S - 1) * rpw                                # rows of the last slab
        for slab_rows in {rpw if S > 1 else last, last}:
            for lr in range(RS):                                # the lane at row lr of a step walks ceil((rows - lr) / RS) rows
                if lr < slab_rows:
                    left.add(-(-(slab_rows - lr) // RS) % 4)
        check(x, params(calib_table(x.contiguous().float()), 4, False, 'laplace_ba'), True)
    assert left == {0, 1, 2, 3}, left


@pytest.mark.parametrize('shape', [(4, 8, 7, 7), (3, 20, 14, 14), (2, 5, 33, 31)])
@pytest.mark.parametrize('relu_first', [False, True])
def test_end_to_end_vs_oracle(shape, relu_first):
    """fp32, min/max parameters from the tensor's own extrema: iqm.py:188-196 as the oracle states it, with the tolerances of
    test_act_bias_correction_vs_oracle."""
    L, ops = mods()
    gen = torch.Generator().manual_seed(22)
    x = torch.randn(shape, generator=gen) * 2 + 0.4
    q_ref = O.act_per_channel_qdq(x, 4, half_range=relu_first)
    ref = O.act_bias_correction(x, q_ref.clone(), relu_first)
    xc = cl(x, torch.float32)
    table = torch.zeros((L.NSTAT, shape[1]), dtype=torch.float32, device='cuda')
    table[L.STAT_MIN] = xc.amin(dim=(0, 2, 3))
    table[L.STAT_MAX] = xc.amax(dim=(0, 2, 3))
    qp, _ = ops.pc_params(table, 4, relu_first, 'no', False)
    y = ops.qdq_bias_corrected_nhwc(xc, qp, relu_first)
    assert is_cl(y)
    out = y.contiguous().cpu()
    np.testing.assert_allclose(out.numpy(), ref.numpy(), rtol=1e-5, atol=1e-5)
    assert torch.equal(out == 0, ref == 0)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_all_bit_widths_and_modes(dtype):
    for offset, shape in ((0, (4, 24, 7, 7)), (1, (4, 24, 7, 7)), (3, (3, 10, 14, 14))):
        for positive in (False, True):
            x = cl(values(shape, seed=5 + offset, positive=positive), dtype, offset)
            table = calib_table(x.contiguous().float())
            for bits in (2, 4, 8):
                for kind in PARAMS:
                    for relu_first in (False, True):
                        check(x, params(table, bits, positive, kind), relu_first)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('relu_first', [False, True])
def test_special_values(dtype, relu_first):
    L, ops = mods()
    x = values((4, 16, 7, 7), seed=9)
    x[:, 5] = 1.5                                           # a constant channel
    x[:, 6] = -x[:, 6].abs() - 0.1                          # no positive element: count 0, the division by 1e-8
    if dtype == torch.float16:
        x[:, 4] = 60000.
        x[1:3, 4] = 65504.
    table = calib_table(cl(x, dtype).contiguous().float())
    x[1, 0, 2, 3] = float('nan')
    x[0, 1, 0, 0] = float('inf')
    x[2, 2, 1, 1] = float('-inf')
    x[3, 3, 4, 4] = float('inf')
    x[3, 3, 5, 5] = float('-inf')
    if dtype == torch.float16:
        # a calibration table may exceed the type's range: the level above 65504 becomes inf
        table[L.STAT_MIN, 4], table[L.STAT_MAX, 4] = 0., 150000.
    xc = cl(x, dtype, 1)
    regular = list(range(4, 16))
    for bits, kind in ((4, 'no'), (4, 'gaus'), (8, 'no')):
        qp = params(table, bits, False, kind)
        y = check(xc, qp, relu_first, sums_on=regular).contiguous()
        assert torch.isnan(y[:, 0]).all()                    # 0 * NaN: the whole channel, as in the reference expression
        assert torch.isfinite(y[:, 7:]).all() and torch.isfinite(y[:, 5]).all()
        _, parts = ops.qdq_bias_corrected_nhwc(xc, qp, relu_first, want_parts=True)
        assert float(parts['sums'][2, 6]) == 0
        if dtype == torch.float16 and kind == 'no' and bits == 4:
            q = ops.pc_qdq(xc.contiguous().float(), 4, 16, 49, qp)
            assert torch.isfinite(q[:, 4]).all() and float(q[:, 4].max()) > 65504
            assert torch.isinf(y[:, 4]).any() and not torch.isnan(y[:, 4]).any()


def run(x, relu_first=True, **kw):
    _, ops = mods()
    qp = params(calib_table(x.contiguous().float()), 4, False, 'laplace_ba')
    return ops.qdq_bias_corrected_nhwc(x, qp, relu_first, **kw)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_deterministic_and_out_placement(dtype):
    for shape, offset in (((16, 64, 14, 14), 0), ((3, 5, 56, 56), 1), ((32, 2048, 7, 7), 0)):
        x = cl(values(shape, seed=21), dtype, offset)
        y1, p1 = run(x, want_parts=True)
        y2, p2 = run(x, want_parts=True)
        assert same(y1, y2) and same64(p1['sums'], p2['sums']) and same(p1['bias'], p2['bias'])
        # another placement of y, with the alignment x has (the piece width is a function of both pointers' alignment)
        n, c, h, w = shape
        base = torch.zeros(x.numel() + 64 + offset, dtype=dtype, device='cuda')
        out = base.as_strided(x.shape, (h * w * c, 1, w * c, c), offset + 16 // x.element_size() * 3)
        y3, p3 = run(x, want_parts=True, out=out)
        assert y3 is out and same(y3, y1) and same64(p1['sums'], p3['sums']) and same(p1['bias'], p3['bias'])


def test_out_and_table_must_match():
    L, ops = mods()
    x = cl(values((2, 8, 7, 7)), torch.float32)
    with pytest.raises(L.CnnqError):
        run(x, out=torch.empty(x.shape, device='cuda'))           # NCHW
    with pytest.raises(L.CnnqError):
        run(x, out=x)
    with pytest.raises(L.CnnqError):
        run(x, out=torch.empty_like(x, dtype=torch.bfloat16))
    with pytest.raises(L.CnnqError):
        ops.qdq_bias_corrected_nhwc(x, torch.zeros(3, 9, device='cuda'), True)      # a table of another channel count
    with pytest.raises(L.CnnqError):
        ops.qdq_bias_corrected_nhwc(x[0], torch.zeros(3, 8, device='cuda'), True)   # not 4-D


def test_graph_capture_replays_eager():
    _, ops = mods()
    x = cl(values((16, 64, 14, 14), seed=2), torch.bfloat16)
    qp = params(calib_table(x.contiguous().float()), 4, False, 'laplace_ba')
    eager = ops.qdq_bias_corrected_nhwc(x, qp, True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.qdq_bias_corrected_nhwc(x, qp, True)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = ops.qdq_bias_corrected_nhwc(x, qp, True)
    x.copy_(cl(values((16, 64, 14, 14), seed=3), torch.bfloat16))
    graph.replay()
    torch.cuda.synchronize()
    assert is_cl(y) and same(y, ops.qdq_bias_corrected_nhwc(x, qp, True))
    assert not same(y, eager)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_ab_switch_and_nchw_take_the_existing_op(monkeypatch, dtype):
    """A tensor that is not 'nhwc', or CNNQ_NHWC=0: qdq_bias_corrected on the counted copy - float32 only, as before."""
    L, ops = mods()
    x = cl(values((4, 16, 14, 14), seed=4), dtype)
    qp = params(calib_table(x.contiguous().float()), 4, False, 'laplace_ba')
    monkeypatch.setenv('CNNQ_NHWC', '0')
    ops.reload_switches()
    try:
        before = ops.LAYOUT_COPIES
        if dtype == torch.float32:
            y, parts = ops.qdq_bias_corrected_nhwc(x, qp, True, want_parts=True)
            assert ops.LAYOUT_COPIES == before + 1 and y.is_contiguous()
            assert same(y, ops.qdq_bias_corrected(x.contiguous(), 4, 16, 196, qp, True))
            assert parts['sums'].shape == (3, 16) and parts['bias'].shape == (16,)
        else:
            with pytest.raises(L.CnnqError):
                ops.qdq_bias_corrected_nhwc(x, qp, True)
    finally:
        monkeypatch.delenv('CNNQ_NHWC')
        ops.reload_switches()
    if dtype == torch.float32:
        yn = ops.qdq_bias_corrected_nhwc(x.contiguous(), qp, True)
        assert yn.is_contiguous() and same(yn, ops.qdq_bias_corrected(x.contiguous(), 4, 16, 196, qp, True))
    assert is_cl(ops.qdq_bias_corrected_nhwc(x, qp, True))


def quantizer(**kw):
    return Q.quantizer(**dict(dict(clipping='laplace', pcq_act=True, bit_alloc_act=True, bcorr_act=True), **kw))


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32], ids=['bf16', 'f32'])
def test_quantizer_with_a_statistics_table(dtype):
    """-sm use -bca through the quantizer: the table it builds from the statistics manager, the correction folded in on the
    channels_last storage; without stat_id the route it took before."""
    L, ops = mods()
    iq = iq_mod()
    x = cl(values((4, 16, 14, 14), seed=8), dtype, 0 if dtype == torch.bfloat16 else 1)
    xf = x.float()
    C = 16
    stat = {'min': xf.amin(dim=(0, 2, 3)), 'max': xf.amax(dim=(0, 2, 3)) * 0.9, 'mean': xf.mean(dim=(0, 2, 3)),
            'std': xf.std(dim=(0, 2, 3)), 'b': (xf - xf.mean(dim=(0, 2, 3)).view(1, C, 1, 1)).abs().mean(dim=(0, 2, 3))}

    class SM:
        def get_tensor_stat(self, stat_id, name, kind='mean'):
            return stat[name].cpu().numpy()
    table = torch.zeros((L.NSTAT, C), dtype=torch.float32, device='cuda')
    for k, r in (('min', L.STAT_MIN), ('max', L.STAT_MAX), ('mean', L.STAT_MEAN), ('std', L.STAT_STD), ('b', L.STAT_B)):
        table[r] = stat[k]
    for clipping, ba, relu_first in (('laplace', True, True), ('gaus', False, False), ('no', False, True), ('no', True, False)):
        q = quantizer(clipping=clipping, bit_alloc_act=ba)
        q.sm = SM
        q.half_range = relu_first
        fb, copies = iq.HALF_FALLBACKS, ops.LAYOUT_COPIES
        q.fuse_bcorr, q.bcorr_fused = relu_first, False
        y = q(x, 'act', stat_id='layer0')
        assert q.fuse_bcorr is None and q.bcorr_fused
        assert is_cl(y) and y.dtype == dtype and y.shape == x.shape
        assert (iq.HALF_FALLBACKS, ops.LAYOUT_COPIES) == (fb, copies)
        qp, _ = ops.pc_params(table, 4, relu_first, clipping, ba, False, None, True)
        assert same(y, ops.qdq_bias_corrected_nhwc(x, qp, relu_first))
        # without a pending request: the routes of sections 12 and 14, no correction
        if not (clipping == 'no' and ba):                    # (min/max with bit allocation keeps its copy there)
            q.bcorr_fused = False
            y0 = q(x, 'act', stat_id='layer0')
            assert is_cl(y0) and not q.bcorr_fused and (iq.HALF_FALLBACKS, ops.LAYOUT_COPIES) == (fb, copies)
            assert same(y0, ops.pc_qdq(x, 4, C, 196, qp))
        # a pending request without stat_id: the counted copy (and the upcast of a half tensor), an NCHW result
        q.fuse_bcorr, q.bcorr_fused = relu_first, False
        yn = q(x, 'act')
        assert q.fuse_bcorr is None and q.bcorr_fused and yn.is_contiguous() and yn.dtype == dtype
        assert ops.LAYOUT_COPIES == copies + 1 and iq.HALF_FALLBACKS == fb + (dtype != torch.float32)


def test_resnet18_channels_last_bias_correction(tmp_path, monkeypatch):
    """The harness end to end on the paper's recipe: -sm collect (per channel, then per tensor), then -sm use -c laplace -baa -bca
    --channels-last --dtype bfloat16.  Every quantizer call on a dense channels_last activation returns a channels_last result
    of the same dtype without a layout copy or the upcast, and the per-channel conv activations fold the correction in."""
    _, ops = mods()
    iq = iq_mod()
    from cnn_quantization_amd.harness import inference_sim as H
    from cnn_quantization_amd.utils.misc import Singleton
    monkeypatch.setenv('HOME', str(tmp_path))
    base = ['-a', 'resnet18', '-b', '4', '--image-size', '64', '--qtype', 'int4', '-qw', 'int4', '-pcq_a', '-pcq_w']
    for argv in (base + ['-sm', 'collect'], [a for a in base if a != '-pcq_a'] + ['-sm', 'collect']):
        Singleton.reset()
        with contextlib.redirect_stdout(io.StringIO()):
            assert H.run(H.build_parser().parse_args(argv), quiet=True)['output_finite']
    orig = iq.IntQuantizer.__call__
    calls = []

    def wrapper(self, tensor, *a, **kw):
        nhwc = isinstance(tensor, torch.Tensor) and tensor.dim() == 4 and ops._layout(tensor) == 'nhwc'
        fb, copies, pending = iq.HALF_FALLBACKS, ops.LAYOUT_COPIES, self.fuse_bcorr is not None
        out = orig(self, tensor, *a, **kw)
        if nhwc:
            calls.append((out.is_contiguous(memory_format=torch.channels_last) and not out.is_contiguous(),
                          iq.HALF_FALLBACKS == fb, ops.LAYOUT_COPIES == copies, out.dtype == tensor.dtype,
                          self.clipping, bool(self.pcq_a), pending, self.bcorr_fused))
        return out
    monkeypatch.setattr(iq.IntQuantizer, '__call__', wrapper)
    Singleton.reset()
    args = H.build_parser().parse_args(base + ['-sm', 'use', '-c', 'laplace', '-baa', '-bca', '--channels-last', '--dtype', 'bfloat16'])
    with contextlib.redirect_stdout(io.StringIO()):
        res = H.run(args, quiet=True)
    Singleton.reset()
    assert res['output_finite']
    corrected = [c for c in calls if c[4] == 'laplace' and c[5] and c[6]]
    assert len(corrected) >= 10, len(corrected)                                   # the per-channel conv activations
    assert all(c[7] for c in corrected), 'a per-channel activation did not fold the correction in'
    assert all(c[0] for c in calls), 'an activation result is not channels_last'
    assert all(c[1] for c in calls), 'an activation call took the half-precision upcast'
    assert all(c[2] for c in calls), 'an activation call copied its input to NCHW'
    assert all(c[3] for c in calls), 'an activation result changed dtype'
