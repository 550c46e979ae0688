"""The `-kld` threshold on bf16 / fp16 activations where they lie: ops.kld_thresholds_half - the row extrema
of tensor_row_stats, cnnq_kld_hist_dt, cnnq_kld_search - against the oracle and the reference's recorded thresholds on the rounded
fixtures (tests/golden/kld_half.npz), and bit for bit against the route it replaces, ops.kld_thresholds on x.float().contiguous();
the per-tensor statistics manager with native_kld; and the harness, `-sm collect -kld --dtype bfloat16 [--channels-last]`.

Tiers: tests/test_kld_gpu.py's - the histogram is integer work, bit-exact; the divergences at rtol 2e-5 / atol 2e-7 against the
oracle's float32 sums; the threshold the reference's, under that file's near-tie rule.  Against the fp32 route everything is
bit-equal: the upconversion is exact, and behind the histogram the two routes are the same kernels."""
import contextlib
import glob
import importlib
import io
import os

import numpy as np
import pandas as pd
import pytest
import torch

from test_half_kld_cpu import CASES, DTYPES, upconverted
from test_kld_gpu import check_row
from test_tensor_collect_manager_gpu import TIERS

pytestmark = pytest.mark.gpu
HALF = [torch.bfloat16, torch.float16]
IDS = ['bf16', 'f16']


def mods():
    from cnn_quantization_amd import ops
    from cnn_quantization_amd.inference import statistic_manager as sm
    from cnn_quantization_amd.utils.misc import Singleton
    return ops, sm, Singleton, importlib.import_module('cnn_quantization_amd.qtypes.int_quantizer')


def bits(t):
    return t.contiguous().view(torch.int64) if t.dtype == torch.float64 else t


def same(a, b):
    """(out, hist, div) of two routes, bit for bit (a NaN equals itself)."""
    return all(x.shape == y.shape and x.dtype == y.dtype and torch.equal(bits(x), bits(y)) for x, y in zip(a, b))


def laplace(shape, dtype, seed):
    return torch.from_numpy(np.random.default_rng(seed).laplace(0.02, 0.9, shape).astype(np.float32)).to(dtype).cuda()


def both(x, rows=None):
    """The native result and the result of the route it replaces; the counters must not move on the native call."""
    ops, _, _, iq = mods()
    before = (ops.LAYOUT_COPIES, iq.HALF_FALLBACKS)
    got = ops.kld_thresholds_half(x, rows, want_parts=True)
    assert (ops.LAYOUT_COPIES, iq.HALF_FALLBACKS) == before
    want = ops.kld_thresholds(x.float().contiguous(), rows, want_parts=True)
    assert got[0].dtype == torch.float64 and got[0].shape == (got[1].shape[0], 3)
    return got, want


@pytest.mark.parametrize('dt,name', CASES)
def test_fixture_cases_as_one_row(golden, dt, name):
    ops = mods()[0]
    g = golden('kld_half')
    x_np = upconverted(g, dt, name)
    x = torch.from_numpy(np.ascontiguousarray(g.np('in_%s_%s' % (dt, name))).view(np.int16)).cuda().view(DTYPES[dt])
    assert np.array_equal(x.float().cpu().numpy(), x_np)
    out, hist, div = ops.kld_thresholds_half(x, 1, want_parts=True)
    th = check_row(x_np, out[0].cpu().numpy(), hist[0].cpu().numpy(), div[0].cpu().numpy())
    assert th == float(g.np('th_%s_%s' % (dt, name)))
    assert out[0, 0].item() == float(g.np('th_%s_%s' % (dt, name)))
    assert int(hist.sum()) == x_np.size


@pytest.mark.parametrize('dtype', HALF, ids=IDS)
@pytest.mark.parametrize('shape', [(3, 70001), (6, 3, 37, 41), (4, 8, 56, 56)], ids=['chunk_boundary_misaligned_rows', 'odd_short_tail', 'aligned'])
def test_bit_equal_to_the_float32_route(dtype, shape):
    x = laplace(shape, dtype, 5)
    if len(shape) == 4:
        x[1] = x[1].clamp(min=0)
    got, want = both(x)
    assert same(got, want)
    assert got[1].sum(1).tolist() == [x[0].numel()] * shape[0]                  # every element of a finite row is counted once


@pytest.mark.parametrize('dtype', HALF, ids=IDS)
def test_base_pointer_off_by_one_element_and_a_row_shorter_than_a_load(dtype):
    x = laplace((2, 40000), dtype, 6)
    v = x.flatten()[1:].reshape(1, -1)
    assert v.data_ptr() % 16 == 2 and v.is_contiguous()
    got, want = both(v, 1)
    assert same(got, want) and int(got[1].sum()) == v.numel()
    for n in (7, 1, 9):
        s = x.flatten()[3:3 + n]
        got, want = both(s, 1)
        assert same(got, want) and int(got[1].sum()) == n
    got, want = both(x.flatten()[5:5 + 6 * 7].reshape(6, 7))                    # rows of 7: every row at another alignment
    assert same(got, want) and got[1].sum(1).tolist() == [7] * 6


@pytest.mark.parametrize('dtype', HALF, ids=IDS)
def test_channels_last_is_read_where_it_lies(dtype):
    x = laplace((4, 9, 9, 24), dtype, 7).permute(0, 3, 1, 2)
    ops = mods()[0]
    assert ops._layout(x) == 'nhwc' and x.shape == (4, 24, 9, 9)
    for rows in (4, 1):
        got, want = both(x, rows)                       # want: the contiguous float32 twin's
        assert same(got, want)
        assert same(got, ops.kld_thresholds_half(x.contiguous(), rows, want_parts=True))
    assert same(ops.kld_thresholds_half(x, want_parts=True), both(x, 4)[1])     # rows None: the samples


@pytest.mark.parametrize('dtype', HALF, ids=IDS)
def test_zero_row_and_rows_without_a_range(dtype):
    ops = mods()[0]
    x = laplace((6, 3001), dtype, 8)
    x[2] = 0                                            # the widened range: every element in the middle bin
    got, want = both(x)
    assert same(got, want)
    assert got[1][2, 1000].item() == 3001 and int(got[1][2].sum()) == 3001
    clean = ops.kld_thresholds_half(x, want_parts=True)
    x = x.clone()
    x[1, 77] = float('nan')
    x[4, 3000] = float('inf')
    got, want = both(x)
    assert same(got, want)
    out, hist, div = got
    for r in (1, 4):
        assert int(hist[r].abs().sum()) == 0
        assert torch.isnan(out[r, :2]).all() and out[r, 2].item() == 0
    keep = [0, 2, 3, 5]
    assert same([t[keep] for t in got], [t[keep] for t in clean])
    assert hist[keep].sum(1).tolist() == [3001] * 4


def test_refusals():
    ops = mods()[0]
    from cnn_quantization_amd import _lib as L
    x = laplace((4, 8, 6, 6), torch.bfloat16, 9)
    cl = x.to(memory_format=torch.channels_last)
    for bad, rows in ((x.float(), None), (cl, 2), (x[:0], None), (x.cpu(), None), (x[:, 2:5], None), (x, 7), (x, 0)):
        with pytest.raises(L.CnnqError):
            ops.kld_thresholds_half(bad, rows)
    with pytest.raises(L.CnnqError):                   # kld_thresholds keeps refusing half tensors
        ops.kld_thresholds(x)
    old = os.environ.get('CNNQ_NHWC')
    try:
        os.environ['CNNQ_NHWC'] = '0'
        ops.reload_switches()
        with pytest.raises(L.CnnqError):
            ops.kld_thresholds_half(cl)
        assert ops.kld_thresholds_half(x).shape == (4, 3)
    finally:
        if old is None:
            os.environ.pop('CNNQ_NHWC', None)
        else:
            os.environ['CNNQ_NHWC'] = old
        ops.reload_switches()


def record(manager, x, through=None):
    manager.stats.clear()
    if through is None:
        manager.save_tensor_stats(x, 'activation', 'layer0')
    else:
        through(manager.save_tensor_stats, x, 'activation', 'layer0')
    return dict(zip(manager.stats_names, manager.stats['layer0'][0]))


@pytest.mark.parametrize('dtype', HALF, ids=IDS)
def test_manager_with_native_kld_records_the_upcast_route_threshold(dtype, tmp_path, monkeypatch):
    ops, sm, Singleton, iq = mods()
    monkeypatch.setenv('HOME', str(tmp_path))
    nchw = laplace((4, 16, 12, 12), dtype, 10)
    try:
        for x in (nchw, laplace((4, 12, 12, 16), dtype, 11).permute(0, 3, 1, 2), laplace((8, 100), dtype, 12)):
            Singleton.reset()
            manager = sm.StatisticManager('t', load_stats=False, kld_threshold=True, native_kld=True)
            assert manager.collect_route(x) == 'flat'
            before = (ops.LAYOUT_COPIES, iq.HALF_FALLBACKS)
            native = record(manager, x)
            assert (ops.LAYOUT_COPIES, iq.HALF_FALLBACKS) == before
            Singleton.reset()
            former = sm.StatisticManager('t', load_stats=False, kld_threshold=True)
            assert former.collect_route(x) is None
            ref = record(former, x, iq.upcast_fallback)             # what _route does with a tensor that has no route
            assert iq.HALF_FALLBACKS == before[1] + 1
            print(native, ref)
            assert native['kld_th'] == ref['kld_th'] and np.isfinite(native['kld_th']) and native['kld_th'] > 0
            assert native['kld_th'] == float(ops.kld_thresholds(x.float().contiguous())[:, 0].max())
            for name, (rtol, atol) in TIERS.items():
                np.testing.assert_allclose(native[name], ref[name], rtol=rtol, atol=atol, err_msg=name)
    finally:
        Singleton.reset()


@pytest.mark.parametrize('layout', [[], ['--channels-last']], ids=['contiguous', 'channels_last'])
def test_resnet18_bf16_collect_kld(layout, tmp_path, monkeypatch):
    """The harness on `-sm collect -kld --dtype bfloat16 [--channels-last]`: every activation takes the native route, no upcast and
    no layout copy on it, and the summary file's kld_th columns are those of a manager with native_kld off.  That second manager is
    fed the SAME activations in the same forward passes, through upcast_fallback as _route feeds it: two runs of the model are not
    the same bits on this stack (the convolutions' results differ in the last bits between identical runs), so a second run would
    compare the model with itself, not the routes."""
    ops, sm, Singleton, iq = mods()
    from cnn_quantization_amd.harness import inference_sim as H
    from cnn_quantization_amd.inference import inference_quantization_manager as iqm
    monkeypatch.setenv('HOME', str(tmp_path))
    base = ['-a', 'resnet18', '-b', '4', '--image-size', '64', '--qtype', 'int4', '-qw', 'int4', '-pcq_w', '--dtype', 'bfloat16',
            '-sm', 'collect', '-kld', '-sf', 'native'] + layout
    native, upcast, clean, shadow = [], [], [], []
    kld_half, fallback, save = ops.kld_thresholds_half, iqm.upcast_fallback, sm.StatisticManager.save_tensor_stats

    class Former(sm.StatisticManager):      # a manager of its own (the Singleton is per class) with the opt-in off
        pass

    def spy_kld(x, *a, **kw):
        before = (iq.HALF_FALLBACKS, ops.LAYOUT_COPIES)
        out = kld_half(x, *a, **kw)
        native.append((x.dtype, ops._layout(x), (iq.HALF_FALLBACKS, ops.LAYOUT_COPIES) == before))
        return out

    def spy_fallback(fn, *a, **kw):
        t = a[0] if a and isinstance(a[0], torch.Tensor) else None
        if getattr(fn, '__name__', '') == 'save_tensor_stats' and t is not None and t.dtype == torch.bfloat16:
            upcast.append(tuple(t.shape))
        return fallback(fn, *a, **kw)

    def save_both(self, tensor, tag, id, tensors_q={}, force_global_min_max=False, *, route=None):
        if isinstance(self, Former):
            return save(self, tensor, tag, id, tensors_q, force_global_min_max)
        before = (iq.HALF_FALLBACKS, ops.LAYOUT_COPIES)
        save(self, tensor, tag, id, tensors_q, force_global_min_max, route=route)
        clean.append((iq.HALF_FALLBACKS, ops.LAYOUT_COPIES) == before and route == 'flat' and self.native_kld)
        if not shadow:
            shadow.append(Former('former', load_stats=False, batch_avg=self.batch_avg, kld_threshold=True))
            assert shadow[0] is not self and not shadow[0].native_kld
        assert shadow[0].collect_route(tensor) is None
        fallback(shadow[0].save_tensor_stats, tensor, tag, id, force_global_min_max=force_global_min_max)

    def summary(folder):
        files = glob.glob(os.path.join(str(tmp_path), 'mxt-sim', 'statistics', folder + '*', '*_summary.csv'))
        assert len(files) == 1, files
        return pd.read_csv(files[0], index_col=0)
    try:
        monkeypatch.setattr(ops, 'kld_thresholds_half', spy_kld)
        monkeypatch.setattr(iqm, 'upcast_fallback', spy_fallback)
        monkeypatch.setattr(sm.StatisticManager, 'save_tensor_stats', save_both)
        Singleton.reset()
        copies = ops.LAYOUT_COPIES
        with contextlib.redirect_stdout(io.StringIO()):
            assert H.run(H.build_parser().parse_args(base), quiet=True)['output_finite']
        shadow[0].__exit__()
    finally:
        monkeypatch.undo()
        Singleton.reset()
    assert not upcast, 'a bf16 activation reached the per-tensor manager through the upcast: %r' % (upcast,)
    assert len(native) >= 10 and len(clean) == len(native) and all(clean)
    assert all(c[0] == torch.bfloat16 and c[2] for c in native), native
    if layout:
        assert sum(1 for c in native if c[1] == 'nhwc') >= 10, native
        assert ops.LAYOUT_COPIES == copies       # the former route reads the upcast channels_last copy where it lies, too
    got, want = summary('native'), summary('former')
    assert list(got.index) == list(want.index) and len(got) >= 10
    for col in ('min_kld_th', 'mean_kld_th', 'max_kld_th'):
        a, b = got[col].astype(float).values, want[col].astype(float).values
        assert np.array_equal(a, b, equal_nan=True), (col, a, b)
    assert bool(np.isfinite(got['mean_kld_th'].astype(float)).any())
    for col in ('mean_max', 'mean_min'):
        assert np.array_equal(got[col].astype(float).values, want[col].astype(float).values), col
