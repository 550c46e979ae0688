"""The `-kld` threshold on bf16 / fp16 activations, the part that needs no GPU: the oracle reproduces the
reference's recorded thresholds on the rounded fixtures (tests/golden/kld_half.npz, written by make_golden_kld_half.py);
cnnq_kld_hist_dt checks its arguments before any launch; collect_route answers 'flat' for a half tensor under kld_threshold exactly
when the manager opted in with native_kld, and what it answered before everywhere else; save_tensor_stats calls the entry points in
the order the route names; the inference manager opts in."""
import importlib.util
import inspect
import os

import numpy as np
import pytest
import torch

from oracle import kld_oracle as K

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
spec = importlib.util.spec_from_file_location('make_golden_collect_routes', os.path.join(GOLDEN, 'make_golden_collect_routes.py'))
G = importlib.util.module_from_spec(spec)
spec.loader.exec_module(G)

BASE = ['laplace', 'relu', 'gauss_outlier', 'band', 'zeros', 'tiny', 'grid', 'negskew']
CASES = [('bf16', n) for n in BASE + ['bf16_max']] + [('f16', n) for n in BASE + ['f16_edges']]
DTYPES = {'bf16': torch.bfloat16, 'f16': torch.float16}


def upconverted(g, dt, name):
    """The fixture's uint16 patterns as the exact float32 values they stand for."""
    bits = np.ascontiguousarray(g.np('in_%s_%s' % (dt, name)))
    return torch.from_numpy(bits.view(np.int16)).view(DTYPES[dt]).float().numpy()


def test_fixture_holds_every_case(golden):
    g = golden('kld_half')
    for dt, name in CASES:
        for k in ('in', 'min', 'max', 'div', 'th'):
            assert '%s_%s_%s' % (k, dt, name) in g
        assert g.np('in_%s_%s' % (dt, name)).dtype == np.uint16
    assert len([k for k in g.keys() if k.startswith('in_')]) == len(CASES)
    e = upconverted(g, 'f16', 'f16_edges')
    assert e.max() == 65504. and e.min() == -65504. and (np.abs(e[e != 0]) < 6.2e-5).sum() >= 6       # subnormals
    assert np.signbit(e[e == 0]).any() and not np.signbit(e[e == 0]).all()                           # -0.0 and +0.0
    b = upconverted(g, 'bf16', 'bf16_max')
    assert b.max() == -b.min() == np.array([0x7f7f0000], np.uint32).view(np.float32)[0]


@pytest.mark.parametrize('dt,name', CASES)
def test_oracle_reproduces_the_reference_on_rounded_inputs(golden, dt, name):
    g = golden('kld_half')
    key = '%s_%s' % (dt, name)
    mn, mx, dmin, th, hist, _, div = K.kld_threshold(upconverted(g, dt, name), full=True)
    assert mn == float(g.np('min_' + key)) and mx == float(g.np('max_' + key))
    assert th == float(g.np('th_' + key))
    want = float(g.np('div_' + key))
    assert (np.isnan(dmin) and np.isnan(want)) or dmin == want
    assert hist.sum() == g.np('in_' + key).size


def test_bf16_leaves_most_bins_empty(golden):
    """What this fixture adds for the search: 8 bits of mantissa put the values on few of the 2001 bins."""
    g = golden('kld_half')
    for name in ('laplace', 'gauss_outlier', 'negskew'):
        hist = K.histogram(upconverted(g, 'bf16', name))[2]
        assert (hist == 0).sum() > K.NUM_BINS // 2, name


def test_argument_validation_needs_no_device():
    from cnn_quantization_amd import _lib as L
    lib = L.load()
    for dt in (L.DTYPE_F32, L.DTYPE_BF16, L.DTYPE_F16):
        assert lib.cnnq_kld_hist_dt(None, dt, 1, 1, None, None, None) == -1          # CNNQ_EINVAL
        assert lib.cnnq_kld_hist_dt(8, dt, 1, 1, None, 8, None) == -1
        assert lib.cnnq_kld_hist_dt(8, dt, 1, 1, 8, None, None) == -1
        assert lib.cnnq_kld_hist_dt(8, dt, 0, 16, 8, 8, None) == -1
        assert lib.cnnq_kld_hist_dt(8, dt, 4, 0, 8, 8, None) == -1
        assert lib.cnnq_kld_hist_dt(8, dt, 70000, 16, 8, 8, None) == -2              # CNNQ_ERANGE: rows beyond the grid's y extent
        assert lib.cnnq_kld_hist_dt(8, dt, 4, 1 << 31, 8, 8, None) == -2             # row length >= 2^31
    for dt in (-1, L.NDTYPE, 7):
        assert lib.cnnq_kld_hist_dt(8, dt, 4, 16, 8, 8, None) == -1                  # outside cnnq_dtype


class FakeManager:
    def __init__(self, kld_threshold=False, group=None, **kw):
        self.kld_threshold, self.group = kld_threshold, group
        vars(self).update(kw)


def test_collect_route_over_kld_and_native_kld(monkeypatch):
    from cnn_quantization_amd import distributed as D
    from cnn_quantization_amd.inference.statistic_manager import collect_route
    xs = G.tensors()
    flat_half = 0
    for x in xs:
        half = isinstance(x, torch.Tensor) and x.dtype in (torch.bfloat16, torch.float16)
        today = {kld: collect_route(FakeManager(kld), x) for kld in (False, True)}          # no attribute: today's answers
        for kld in (False, True):
            assert collect_route(FakeManager(kld, native_kld=False), x) == today[kld]
            got = collect_route(FakeManager(kld, native_kld=True), x)
            if kld and half and today[False] == 'flat':
                # the tensor the route takes without -kld: with the opt-in it takes it under -kld too
                assert today[True] is None and got == 'flat', (x.shape, x.dtype, x.stride())
                flat_half += 1
            else:
                assert got == today[kld], (kld, x.shape, x.dtype, x.stride())
    assert flat_half >= 4       # contiguous and channels_last, bf16 and fp16, at least
    # the route word is asked last, about (rows, length, dtype), and only for a half tensor under kld with the opt-in; its no
    # sends the class back to the upcast route
    from cnn_quantization_amd import ops
    asked = []
    monkeypatch.setattr(ops, '_kld_half_native', lambda rows, length, dtype: asked.append((rows, length, dtype)) or False)
    for x in xs:
        half = isinstance(x, torch.Tensor) and x.dtype in (torch.bfloat16, torch.float16)
        for kld in (False, True):
            for native_kld in (False, True):
                del asked[:]
                got = collect_route(FakeManager(kld, native_kld=native_kld), x)
                want = collect_route(FakeManager(kld), x)
                assert got == want, (kld, native_kld, x.shape, x.dtype)
                takes = kld and native_kld and half and collect_route(FakeManager(False), x) == 'flat'
                rows = x.shape[0] if takes and x.dim() > 1 else 1
                assert asked == ([(rows, x.numel() // rows, x.dtype)] if takes else []), (asked, x.shape)
    # several ranks or a forced exchange: None again, with or without the opt-in, and the word is not asked
    for patch in ((D, 'world_size', lambda group=None: 2), (D, 'forced_exchange', lambda: True)):
        monkeypatch.setattr(*patch)
        del asked[:]
        for x in xs:
            for kld in (False, True):
                assert collect_route(FakeManager(kld, native_kld=True), x) is None
        assert not asked
        monkeypatch.undo()
        monkeypatch.setattr(ops, '_kld_half_native', lambda rows, length, dtype: asked.append((rows, length, dtype)) or False)
    monkeypatch.undo()


def test_route_word_keeps_the_measured_classes_and_is_cached():
    """profiles/half_kld.md: at 512 rows the two smallest ResNet-50 classes did not win beyond the spread; everything else did, and
    fewer rows were not measured."""
    from cnn_quantization_amd import ops
    ops._KLD_HALF_NATIVE.clear()
    for dtype in (torch.bfloat16, torch.float16):
        for C, hw, native in ((64, 112, True), (256, 56, True), (128, 56, True), (512, 28, True), (64, 56, True), (256, 28, True),
                              (1024, 14, True), (128, 28, True), (512, 14, True), (2048, 7, True), (256, 14, False), (512, 7, False)):
            assert ops._kld_half_native(512, C * hw * hw, dtype) is native, (C, hw)
            assert ops._kld_half_native(4, C * hw * hw, dtype) and ops._kld_half_native(64, C * hw * hw, dtype)
        assert ops._kld_half_native(1, 16, dtype) and not ops._kld_half_native(1024, 1000, dtype)
    assert (512, 256 * 14 * 14, torch.bfloat16) in ops._KLD_HALF_NATIVE
    ops._KLD_HALF_NATIVE[(3, 5, torch.bfloat16)] = False            # the cache answers
    assert ops._kld_half_native(3, 5, torch.bfloat16) is False
    ops._KLD_HALF_NATIVE.clear()
    assert ops._kld_half_native(3, 5, torch.bfloat16) is True


def test_real_manager_carries_the_attribute(monkeypatch, tmp_path):
    from cnn_quantization_amd.inference.statistic_manager import StatisticManager
    from cnn_quantization_amd.utils.misc import Singleton
    monkeypatch.setenv('HOME', str(tmp_path))
    try:
        Singleton.reset()
        assert StatisticManager('t', load_stats=False, kld_threshold=True).native_kld is False
        Singleton.reset()
        m = StatisticManager('t', load_stats=False, kld_threshold=True, native_kld=True)
        assert m.native_kld is True and m.stats_names[-1] == 'kld_th'
    finally:
        Singleton.reset()


def test_save_tensor_stats_call_sequence(monkeypatch, tmp_path):
    """A half tensor on the native route: tensor_stats, then kld_thresholds_half on the tensor as it lies, with rows = its samples;
    everything else: kld_thresholds, as before."""
    from cnn_quantization_amd import _lib as L, ops
    from cnn_quantization_amd.inference.statistic_manager import StatisticManager
    from cnn_quantization_amd.utils.misc import Singleton
    calls = []

    def tables(name):
        def fn(x, *a, **kw):
            calls.append((name, x.dtype, ops._layout(x)))
            return torch.ones(L.NSTAT, 1), torch.ones(L.NMOM, 1, dtype=torch.float64)
        return fn

    def kld(name):
        def fn(x, rows=None, want_parts=False):
            calls.append((name, x.dtype, ops._layout(x), rows))
            return torch.tensor([[1.5, 0.1, 3.], [2.5, 0.2, 4.]], dtype=torch.float64)[:rows]
        return fn
    monkeypatch.setattr(ops, 'tensor_stats', tables('tensor_stats'))
    monkeypatch.setattr(ops, 'pc_stats', tables('pc_stats'))
    monkeypatch.setattr(ops, 'kld_thresholds', kld('kld_thresholds'))
    monkeypatch.setattr(ops, 'kld_thresholds_half', kld('kld_thresholds_half'))
    monkeypatch.setenv('HOME', str(tmp_path))
    bf, f32 = torch.bfloat16, torch.float32
    nchw = torch.zeros(2, 8, 4, 4, dtype=bf)
    nhwc = torch.zeros(2, 8, 4, 4, dtype=bf).to(memory_format=torch.channels_last)
    try:
        Singleton.reset()
        m = StatisticManager('t', load_stats=False, kld_threshold=True, native_kld=True)
        for x, route, want in (
                (nchw, 'flat', [('tensor_stats', bf, 'nchw'), ('kld_thresholds_half', bf, 'nchw', 2)]),
                (nhwc, 'flat', [('tensor_stats', bf, 'nhwc'), ('kld_thresholds_half', bf, 'nhwc', 2)]),
                (torch.zeros(16, dtype=torch.float16), 'flat',
                 [('tensor_stats', torch.float16, 'nchw'), ('kld_thresholds_half', torch.float16, 'nchw', 1)]),
                (nhwc.float(), 'flat', [('tensor_stats', f32, 'nhwc'), ('kld_thresholds', f32, 'nhwc', 2)]),
                # no route (a CPU tensor here; on the device: what upcast_fallback hands over): the copy, the former entry points
                (nhwc.float(), None, [('pc_stats', f32, 'nchw'), ('kld_thresholds', f32, 'nchw', 2)]),
                (nchw.float(), None, [('pc_stats', f32, 'nchw'), ('kld_thresholds', f32, 'nchw', 2)])):
            del calls[:]
            m.save_tensor_stats(x, 'activation', 'l%d' % len(m.stats), route=route)
            assert calls == want, (calls, want)
        assert m.stats['l0'][0, m.stats_names.index('kld_th')] == 2.5       # the maximum over the samples
        assert m.stats['l2'][0, m.stats_names.index('kld_th')] == 1.5
    finally:
        Singleton.reset()


def test_ops_entry_refuses_without_a_device():
    from cnn_quantization_amd import _lib as L, ops
    with pytest.raises(L.CnnqError):
        ops.kld_thresholds_half(torch.zeros(4, 16, dtype=torch.bfloat16))       # a CPU tensor
    with pytest.raises(L.CnnqError):
        ops.kld_thresholds_half(None)


def test_inference_manager_opts_in():
    from cnn_quantization_amd.inference import inference_quantization_manager as iqm
    src = inspect.getsource(iqm.QuantizationManagerInference.__init__)
    call = src[src.index('StatisticManager(sf, load_stats=False'):]
    call = call[:call.index(')') + 1]
    assert 'kld_threshold=args.kld_threshold' in call and 'native_kld=True' in call
