"""Activation bias correction (-bca, iqm.py:180-196) folded into the table-driven Q/DQ on CONTIGUOUS bf16 / fp16 activations
(DESIGN.md section 24): ops.qdq_bias_corrected_half on both of its routes - the single launch and the two passes.

The per-channel sums are added in an order fixed by the geometry and the route, so the contract has two halves:
  1. the sums: sum x' and sum q against fp64 on the CPU over x.float() and q = pc_qdq(x.float(), qp), within RTOL_STAT = 2e-6 of
     sum |term| per channel (at most seven fp32 additions per piece are about 4e-7 of it); the count exact;
  2. given the sums, bit for bit (NaN == NaN): bias == (float32(sum x') - float32(sum q)) / (float32(count) + 1e-8f), and
     y == (q + (q > 0) * bias).to(x.dtype), no layout copy and no upcast counted."""
import ctypes

import numpy as np
import pytest
import torch

import _half_bcorr as HB
from test_channels_last_gpu import same, values
from test_channels_last_bcorr_gpu import RTOL_STAT, calib_table, close, iq_mod, mods, params, rows, same64

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]
IDS = ['bf16', 'f16']


def place(x, dtype, offset=0):
    """x as a contiguous tensor of dtype on the GPU, `offset` elements into its storage."""
    base = torch.zeros(x.numel() + offset + 8, dtype=dtype, device='cuda')
    v = base[offset:offset + x.numel()].view(x.shape)
    v.copy_(x.to(dtype).cuda())
    assert v.is_contiguous() and v.storage_offset() == offset
    return v


def route_of(x, allow):
    L, _ = mods()
    out = (ctypes.c_int32 * 4)()
    N, C, H, W = x.shape
    align = (x.data_ptr() | 16) & -(x.data_ptr() | 16)
    assert L.load().cnnq_pc_route_qdq_bcorr_dt(N, C, H * W, 1 if x.dtype == torch.bfloat16 else 2, align, allow, out) == 0
    return tuple(out)


def routes(x):
    """The forced routes x has: the two passes always, the single launch where the channel fits."""
    return (False, True) if route_of(x, 2)[3] == 1 else (False,)


def check(x, qp, relu_first, single, sums_on=None):
    """Both halves of the contract for one call on one forced route; sums_on: the channels whose sums are compared (None: all)."""
    L, ops = mods()
    iq = iq_mod()
    N, C, H, W = x.shape
    before = (ops.LAYOUT_COPIES, iq.HALF_FALLBACKS)
    y, parts = ops.qdq_bias_corrected_half(x, qp, relu_first, want_parts=True, single_launch=single)
    assert (ops.LAYOUT_COPIES, iq.HALF_FALLBACKS) == before
    assert y.is_contiguous() and y.dtype == x.dtype and y.shape == x.shape
    xf = x.float()
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
        print('%s %s %s relu=%d single=%d: worst |dev - ref| / sum|term| = %.3g'
              % (name, tuple(x.shape), x.dtype, relu_first, single, float(worst.max()) if worst.numel() else 0.))
        assert close(dev[ch], ref[ch], RTOL_STAT * mag[ch]), (name, tuple(x.shape), x.dtype, x.storage_offset(), single)
    assert torch.equal(sums[2], (v64 > 0).sum(1).double()), (tuple(x.shape), x.dtype, single)
    # half 2
    s = sums.numpy()
    with np.errstate(all='ignore'):
        bias_ref = (s[0].astype(np.float32) - s[1].astype(np.float32)) / (s[2].astype(np.float32) + np.float32(1e-8))
    assert same(parts['bias'].cpu(), torch.from_numpy(bias_ref)), (tuple(x.shape), x.dtype, single)
    y_ref = (q + (q > 0).float() * parts['bias'].view(1, C, 1, 1)).to(x.dtype)
    assert same(y, y_ref), (tuple(x.shape), x.dtype, relu_first, x.storage_offset(), single)
    # the hot form (the bias in the cached workspace) and a second call give the same bits
    assert same(ops.qdq_bias_corrected_half(x, qp, relu_first, single_launch=single), y)
    y2, p2 = ops.qdq_bias_corrected_half(x, qp, relu_first, want_parts=True, single_launch=single)
    assert same(y2, y) and same64(p2['sums'], parts['sums']) and same(p2['bias'], parts['bias'])
    assert (ops.LAYOUT_COPIES, iq.HALF_FALLBACKS) == before
    return y


# (bits, positive, relu first, parameters), dealt over the shapes in turn
COMBOS = [(4, False, False, 'laplace_ba'), (8, True, True, 'no'), (4, False, True, 'gaus'), (4, True, False, 'no_ba'),
          (8, False, False, 'gaus'), (4, False, True, 'no_ba')]


def table_params(table, bits, positive, kind):
    _, ops = mods()
    if kind == 'no_ba':                                     # min/max with bit allocation
        return ops.pc_params(table, bits, positive, 'no', bits <= 4, False)[0]
    return params(table, bits, positive, kind)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('case', HB.CASES, ids=HB.IDS)
def test_every_branch_on_both_routes(case, dtype):
    shape, offset, (W, S, cs, fits) = case
    i = HB.CASES.index(case)
    for k in (i, i + 1):
        bits, positive, relu_first, kind = COMBOS[k % len(COMBOS)]
        x = place(values(shape, seed=sum(shape) + offset, positive=positive), dtype, offset)
        assert route_of(x, 2) == (W, S, cs, 1 if fits else 2), route_of(x, 2)
        assert routes(x) == ((False, True) if fits else (False,))
        qp = table_params(calib_table(x.float()), bits, positive, kind)
        for single in routes(x):
            check(x, qp, relu_first, single)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_all_bit_widths_and_modes(dtype):
    for offset, shape in ((0, (4, 24, 7, 7)), (0, (3, 10, 14, 14)), (2, (2, 6, 8, 12))):
        for positive in (False, True):
            x = place(values(shape, seed=5 + offset, positive=positive), dtype, offset)
            table = calib_table(x.float())
            for bits in (4, 8):
                for kind in ('laplace_ba', 'gaus', 'no_ba', 'no'):
                    for relu_first in (False, True):
                        for single in routes(x):
                            check(x, table_params(table, bits, positive, kind), relu_first, single)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('relu_first', [False, True])
def test_special_values(dtype, relu_first):
    L, ops = mods()
    x = values((4, 16, 6, 6), seed=9)
    x[:, 5] = 1.5                                           # a constant channel
    x[:, 6] = -x[:, 6].abs() - 0.1                          # no positive element: count 0, the division by 1e-8
    if dtype == torch.float16:
        x[:, 4] = 60000.
        x[1:3, 4] = 65504.
    table = calib_table(place(x, dtype).float())
    x[1, 0, 2, 3] = float('nan')
    x[0, 1, 0, 0] = float('inf')
    x[2, 2, 1, 1] = float('-inf')
    x[3, 3, 4, 4] = float('inf')
    x[3, 3, 5, 5] = float('-inf')
    if dtype == torch.float16:
        # a calibration table may exceed the type's range: the level above 65504 becomes inf
        table[L.STAT_MIN, 4], table[L.STAT_MAX, 4] = 0., 150000.
    regular = list(range(4, 16))
    for offset in (0, 1):                                   # W = 4 (both routes) and W = 1
        xc = place(x, dtype, offset)
        for bits, kind in ((4, 'no'), (4, 'gaus'), (8, 'no')):
            qp = table_params(table, bits, False, kind)
            for single in routes(xc):
                y = check(xc, qp, relu_first, single, sums_on=regular)
                assert torch.isnan(y[:, 0]).all()            # 0 * NaN: the whole channel, as in the reference expression
                assert torch.isfinite(y[:, 7:]).all() and torch.isfinite(y[:, 5]).all()
                _, parts = ops.qdq_bias_corrected_half(xc, qp, relu_first, want_parts=True, single_launch=single)
                assert float(parts['sums'][2, 6]) == 0
                if dtype == torch.float16 and kind == 'no' and bits == 4:
                    q = ops.pc_qdq(xc.float(), 4, 16, 36, qp)
                    assert torch.isfinite(q[:, 4]).all() and float(q[:, 4].max()) > 65504
                    assert torch.isinf(y[:, 4]).any() and not torch.isnan(y[:, 4]).any()


def run(x, relu_first=True, **kw):
    _, ops = mods()
    qp = params(calib_table(x.float()), 4, False, 'laplace_ba')
    return ops.qdq_bias_corrected_half(x, qp, relu_first, **kw)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_route_function_is_followed_and_out_is_accepted(dtype):
    _, ops = mods()
    # (the third shape is the smallest of the classes the route function gives the single launch: C = 256, N * HW >= 32768)
    for shape, offset in (((16, 64, 14, 14), 0), ((3, 5, 56, 56), 1), ((168, 256, 14, 14), 0), ((65, 1, 32, 64), 0)):
        x = place(values(shape, seed=21), dtype, offset)
        word = route_of(x, 1)[3]
        assert word == (1 if shape[1] == 256 else 2)
        y1, p1 = run(x, want_parts=True)
        y2, p2 = run(x, want_parts=True, single_launch=(word == 1))
        assert same(y1, y2) and same64(p1['sums'], p2['sums']) and same(p1['bias'], p2['bias'])
        # another placement of y, with the alignment x has (the piece width is a function of both pointers' alignment)
        base = torch.zeros(x.numel() + 64 + offset, dtype=dtype, device='cuda')
        out = base[offset + 24:offset + 24 + x.numel()].view(x.shape)
        y3, p3 = run(x, want_parts=True, out=out)
        assert y3 is out and same(y3, y1) and same64(p1['sums'], p3['sums']) and same(p1['bias'], p3['bias'])


def test_refusals_copy_nothing():
    L, ops = mods()
    iq = iq_mod()
    x = place(values((2, 8, 7, 7)), torch.bfloat16)
    qp = torch.zeros(3, 8, device='cuda')
    before = (ops.LAYOUT_COPIES, iq.HALF_FALLBACKS)
    for bad in (x.float(), x.to(memory_format=torch.channels_last), x[:, :, :, :5], x.cpu(), x[0], x.view(2, 8, 49)):
        with pytest.raises(L.CnnqError):
            ops.qdq_bias_corrected_half(bad, qp, True)
    for bad_qp in (torch.zeros(3, 9, device='cuda'), torch.zeros(3, 8, device='cuda', dtype=torch.float64), torch.zeros(3, 8),
                   torch.zeros(8, 3, device='cuda').t(), None):
        with pytest.raises(L.CnnqError):
            ops.qdq_bias_corrected_half(x, bad_qp, True)
    with pytest.raises(L.CnnqError):
        run(x, out=x)
    with pytest.raises(L.CnnqError):
        run(x, out=torch.empty_like(x, dtype=torch.float16))
    with pytest.raises(L.CnnqError):
        run(x, out=torch.empty_like(x).to(memory_format=torch.channels_last))
    with pytest.raises(L.CnnqError):
        run(x, single_launch=True)                           # W = 1: no single launch
    assert (ops.LAYOUT_COPIES, iq.HALF_FALLBACKS) == before


@pytest.mark.parametrize('single', [False, True], ids=['two-passes', 'single-launch'])
def test_graph_capture_replays_eager(single):
    _, ops = mods()
    x = place(values((16, 64, 14, 14), seed=2), torch.bfloat16)
    qp = params(calib_table(x.float()), 4, False, 'laplace_ba')
    eager = ops.qdq_bias_corrected_half(x, qp, True, single_launch=single)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.qdq_bias_corrected_half(x, qp, True, single_launch=single)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = ops.qdq_bias_corrected_half(x, qp, True, single_launch=single)
    x.copy_(values((16, 64, 14, 14), seed=3).to(torch.bfloat16).cuda())
    graph.replay()
    torch.cuda.synchronize()
    assert same(y, ops.qdq_bias_corrected_half(x, qp, True, single_launch=single))
    assert not same(y, eager)
