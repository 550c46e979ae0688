"""The channels_last error columns without a device: the C entry points' argument checks and workspace
size, and the two opt-in routes - collect_route with native_err, _clip_route's row 'mix' with native_mix - over a small grid,
with the ops entry points stubbed.  Nothing is launched."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

from _quantizer import act, nhwc, quantizer

EINVAL, ERANGE = -1, -2
F32, BF16, F16 = 0, 1, 2


def _route(lib, N, HW, C, dtype, align=16):
    out = (ctypes.c_int32 * 4)()
    rc = lib.cnnq_pc_route_qerr_nhwc(N, HW, C, dtype, align, out)
    return rc, list(out)


def test_argument_validation_needs_no_device():
    from cnn_quantization_amd import _lib as L
    lib = L.load()
    assert (L.DTYPE_F32, L.DTYPE_BF16, L.DTYPE_F16) == (F32, BF16, F16)
    ok = dict(x=64, dtype=F32, N=2, HW=9, C=8, qp=64, K=3, mm=None, ws=64, err=64)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.cnnq_pc_qerr_nhwc(a['x'], a['dtype'], a['N'], a['HW'], a['C'], a['qp'], a['K'], a['mm'], a['ws'], a['err'], None)
    # (the dummy pointers are never dereferenced: every case is refused before anything touches the device)
    for bad in (dict(x=None), dict(qp=None), dict(ws=None), dict(err=None), dict(K=0), dict(K=4), dict(dtype=3), dict(dtype=-1),
                dict(N=0), dict(HW=0), dict(C=0), dict(N=-1), dict(ws=68), dict(C=(1 << 26) + 1)):
        assert call(**bad) == EINVAL, bad
    assert call(N=1 << 31) == ERANGE and call(HW=1 << 31) == ERANGE
    for bad in ((0, 9, 8, 3, F32), (2, 0, 8, 3, F32), (2, 9, 0, 3, F32), (2, 9, 8, 0, F32), (2, 9, 8, 4, F32), (2, 9, 8, 3, 3),
                (1 << 31, 9, 8, 3, F32), (2, 1 << 31, 8, 3, F32)):
        assert lib.cnnq_pc_qerr_nhwc_workspace(*bad) == 0, bad
    assert _route(lib, 2, 9, 8, F32, align=3)[0] == EINVAL
    assert _route(lib, 2, 9, 8, 7)[0] == EINVAL
    assert lib.cnnq_pc_route_qerr_nhwc(2, 9, 8, F32, 16, None) == EINVAL


def test_workspace_is_the_row_records_of_the_plan_the_route_reports():
    from cnn_quantization_amd import _lib as L
    lib = L.load()
    cut = 0
    shapes = [(2, 144, 64), (3, 45, 6), (3, 49, 5), (2, 49, 1040), (5, 9, 16), (1, 1600, 8), (2, 2304, 64), (512, 3136, 256),
              (1, 12544, 64), (8, 12544, 64), (512, 49, 2048)]
    for (N, HW, C), dtype, K in itertools.product(shapes, (F32, BF16, F16), (1, 2, 3)):
        rc, (w, nb, rows, native) = _route(lib, N, HW, C, dtype)
        assert rc == 0 and native == 1 and 1 <= w <= 2 and C % w == 0
        assert nb >= 1 and nb * rows >= HW                                   # the slabs cover the sample
        assert lib.cnnq_pc_qerr_nhwc_workspace(N, HW, C, K, dtype) == N * nb * (1 + 3 * K) * C * 8
        for align in (2, 4, 8):                                              # the record count does not depend on the alignment
            rc2, o2 = _route(lib, N, HW, C, dtype, align)
            assert rc2 == 0 and o2[1] == nb and o2[0] <= w
        cut += nb > 1
    assert cut > 0                                                           # some plan cuts a sample into several slabs
    assert _route(lib, 3, 49, 5, F32)[1][0] == 1 and _route(lib, 3, 45, 6, BF16)[1][0] == 2
    assert _route(lib, 2, 144, 64, BF16)[1][0] == 2 and _route(lib, 2, 144, 64, F32)[1][0] == 2    # no wider piece here
    assert _route(lib, 2, 144, 64, F32, align=4)[1][0] == 1                  # (an x aligned to one element only)


# ---- routes
def _managers(monkeypatch, tmp_path):
    from cnn_quantization_amd.inference import statistic_manager_perchannel as smpc
    from cnn_quantization_amd.utils.misc import Singleton
    monkeypatch.setenv('HOME', str(tmp_path))
    for collect_err, native_err, batch_avg in itertools.product((False, True), (False, True), (False, True)):
        Singleton.reset()
        yield smpc.StatisticManagerPerChannel('t', load_stats=False, collect_err=collect_err, batch_avg=batch_avg,
                                              native_err=native_err, err_settings=dict(num_bits=4))
    Singleton.reset()


TENSORS = [('nhwc_bf16', lambda: nhwc()), ('nhwc_f16', lambda: nhwc(torch.float16)), ('nhwc_f32', lambda: nhwc(torch.float32)),
           ('act_bf16', lambda: act()), ('act_f32', lambda: act(torch.float32)), ('nhwc_f64', lambda: nhwc(torch.float64)),
           ('fc', lambda: act(shape=(2, 8)))]


def _without_errors(manager, name, force):
    """collect_route's answer for a manager without error columns: the parent's table."""
    if manager.batch_avg and not force:
        return None
    return {'nhwc_bf16': 'nhwc', 'nhwc_f16': 'nhwc', 'nhwc_f32': 'nhwc', 'act_bf16': 'half'}.get(name)


def test_collect_route_answers_as_before_unless_native_err(monkeypatch, tmp_path):
    from cnn_quantization_amd import distributed as D, ops
    asked = []
    monkeypatch.setattr(ops, '_stats_nhwc_native', lambda *a: True)
    monkeypatch.setattr(ops, '_stats_half_native', lambda *a: True)
    monkeypatch.setattr(ops, '_qerr_nhwc_native', lambda *a: asked.append(a) or True)
    seen = set()
    for manager in _managers(monkeypatch, tmp_path):
        for (name, make), force in itertools.product(TENSORS, (False, True)):
            x = make()
            got = manager.collect_route(x, force)
            if not manager.collect_err:
                want = _without_errors(manager, name, force)
            elif not manager.native_err:
                want = None                                                   # as before: error columns take the copy route
            else:
                want = 'nhwc' if _without_errors(manager, name, force) == 'nhwc' else None
            assert got == want, (manager.collect_err, manager.native_err, manager.batch_avg, name, force, got)
            seen.add((manager.collect_err and manager.native_err, got))
            if manager.collect_err and manager.native_err and got == 'nhwc':
                assert asked[-1] == (2, 16, 8, x.dtype)                       # (N, HW, C, dtype) of the class of layer
    assert seen >= {(True, 'nhwc'), (True, None), (False, 'nhwc'), (False, 'half'), (False, None)}
    n_asked = len(asked)
    assert n_asked > 0

    # opted in, and still the copy route: several ranks, a forced exchange, either route word, the channels_last switch off
    from cnn_quantization_amd.inference import statistic_manager_perchannel as smpc
    from cnn_quantization_amd.utils.misc import Singleton
    Singleton.reset()
    manager = smpc.StatisticManagerPerChannel('t', load_stats=False, collect_err=True, native_err=True)
    x = nhwc()
    assert manager.collect_route(x) == 'nhwc'
    with monkeypatch.context() as m:
        m.setattr(D, 'world_size', lambda group=None: 2)
        assert manager.collect_route(x) is None
    with monkeypatch.context() as m:
        m.setattr(D, 'forced_exchange', lambda: True)
        assert manager.collect_route(x) is None
    with monkeypatch.context() as m:
        m.setattr(ops, '_stats_nhwc_native', lambda *a: False)
        assert manager.collect_route(x) is None
    with monkeypatch.context() as m:
        m.setattr(ops, '_qerr_nhwc_native', lambda *a: False)
        assert manager.collect_route(x) is None
    with monkeypatch.context() as m:
        m.setattr(ops, '_NHWC', False)
        assert manager.collect_route(x) is None
    assert manager.collect_route(x) == 'nhwc'
    Singleton.reset()


def test_save_tensor_stats_on_the_route_calls_the_channels_last_entry_points_in_order(monkeypatch, tmp_path):
    from cnn_quantization_amd import _lib as L, ops
    from cnn_quantization_amd.inference import statistic_manager_perchannel as smpc
    from cnn_quantization_amd.utils.misc import Singleton
    monkeypatch.setenv('HOME', str(tmp_path))
    calls = []
    C = 8
    table = torch.arange(L.NSTAT * C, dtype=torch.float32).view(L.NSTAT, C)
    err = -torch.arange(6 * C, dtype=torch.float32).view(6, C) - 1.

    def stats(x, **kw):
        calls.append(('pc_stats_nhwc', x.dtype, not x.is_contiguous(), kw['need_b']))
        return table, None

    def cands(t, **settings):
        calls.append(('mix_candidates', t is table, settings))
        return 'l', 'g', 'p'

    def errors(x, qps, mm=None):
        calls.append(('pc_quant_errors_nhwc', x.dtype, not x.is_contiguous(), tuple(qps), torch.equal(mm, table[[L.STAT_MIN, L.STAT_MAX]])))
        return err

    def refuse(*a, **kw):
        raise AssertionError('the copy route was taken')
    monkeypatch.setattr(ops, 'pc_stats_nhwc', stats)
    monkeypatch.setattr(ops, 'mix_candidates', cands)
    monkeypatch.setattr(ops, 'pc_quant_errors_nhwc', errors)
    monkeypatch.setattr(ops, 'pc_stats', refuse)
    monkeypatch.setattr(ops, 'pc_quant_errors', refuse)
    monkeypatch.setattr(ops, '_stats_nhwc_native', lambda *a: True)
    monkeypatch.setattr(ops, '_qerr_nhwc_native', lambda *a: True)
    Singleton.reset()
    try:
        manager = smpc.StatisticManagerPerChannel('t', load_stats=False, collect_err=True, native_err=True,
                                                  err_settings=lambda tag, half: dict(num_bits=4, positive=half))
        manager.save_tensor_stats(nhwc(), 'activation', 'conv0_activation', half_range=True)
        assert calls == [('pc_stats_nhwc', torch.bfloat16, True, True), ('mix_candidates', True, dict(num_bits=4, positive=True)),
                         ('pc_quant_errors_nhwc', torch.bfloat16, True, ('p', 'g', 'l'), True)]
        rec = manager.stats['conv0_activation']
        assert np.array_equal(rec['b'], table[L.STAT_B].numpy())
        for i, name in enumerate(smpc.ERR_NAMES):
            assert np.array_equal(rec[name], err[i].numpy()), name
    finally:
        Singleton.reset()


def _mix(**kw):
    return quantizer(clipping='mix', pcq_act=True, **kw)


def test_clip_route_gains_the_row_mix_only_when_opted_in(monkeypatch):
    from cnn_quantization_amd import distributed as D, ops
    tensors = dict(nhwc_bf16=nhwc(), nhwc_f16=nhwc(torch.float16), nhwc_f32=nhwc(torch.float32), act_bf16=act(), act_f16=act(torch.float16),
                   act_f32=act(torch.float32), fc=act(shape=(2, 8)), flat=act(shape=(2, 8, 1, 1)))
    native = {'nhwc_bf16', 'nhwc_f16', 'nhwc_f32', 'act_bf16', 'act_f16'}
    for opted, me, pending, stat_id, (name, x) in itertools.product((False, True), (False, True), (False, True), (None, 'conv0'),
                                                                    tensors.items()):
        q = _mix(measure_entropy=me)
        assert q.native_mix is False                                          # a directly constructed object: the parent's routes
        q.native_mix = opted
        q.fuse_bcorr = True if pending else None
        want = 'mix' if (opted and not me and not pending and stat_id is not None and name in native) else None
        assert q._asked(x, stat_id) == want, (opted, me, pending, stat_id, name)
        assert q._clip_route(x, 'mix', stat_id, q._att()) == want
        # the other clipping types do not see the attribute
        other = quantizer(clipping='laplace', pcq_act=True, measure_entropy=me)
        other.fuse_bcorr = q.fuse_bcorr
        before = other._asked(x, stat_id)
        other.native_mix = True
        assert other._asked(x, stat_id) == before
    q = _mix()
    q.native_mix = True
    x = nhwc()
    assert q._asked(x, 'conv0') == 'mix'
    with monkeypatch.context() as m:
        m.setattr(D, 'world_size', lambda group=None: 2)
        assert q._asked(x, 'conv0') is None
    with monkeypatch.context() as m:
        m.setattr(D, 'forced_exchange', lambda: True)
        assert q._asked(x, 'conv0') is None
    with monkeypatch.context() as m:
        m.setattr(ops, '_NHWC', False)
        assert q._asked(x, 'conv0') is None and q._asked(nhwc(torch.float32), 'conv0') is None
        assert q._asked(act(), 'conv0') == 'mix'                              # a contiguous half tensor does not ask the switch
    q.group = False                                                           # replicated data
    assert q._asked(x, 'conv0') is None
    per_tensor = quantizer(clipping='mix', pcq_act=False)
    per_tensor.native_mix = True
    assert per_tensor._asked(x, 'conv0') is None


def test_call_does_not_upcast_on_the_route(monkeypatch):
    """__call__ hands a half tensor on the route 'mix' to ops.act_qdq_mix as it is; off the route it upcasts first."""
    import importlib
    from cnn_quantization_amd import ops
    iq = importlib.import_module('cnn_quantization_amd.qtypes.int_quantizer')
    got = []

    class Stats:
        def get_tensor_stat(self, stat_id, stat, kind='mean'):
            return np.ones(8, dtype=np.float32)
    monkeypatch.setattr(ops, 'act_qdq_mix', lambda x, *a, **kw: got.append((x.dtype, not x.is_contiguous())) or x)
    for opted in (False, True):
        for x in (nhwc(), act()):
            q = _mix()
            q.sm = Stats
            q.native_mix = opted
            before = iq.HALF_FALLBACKS
            y = q(x, 'conv0', 'activation', stat_id='conv0')
            assert y.dtype == x.dtype
            assert iq.HALF_FALLBACKS - before == (0 if opted else 1)
            assert got[-1] == ((x.dtype, not x.is_contiguous()) if opted else (torch.float32, not x.is_contiguous()))


def test_the_inference_manager_opts_in():
    import inspect
    import types
    from _quantizer import PARAMS
    from cnn_quantization_amd.inference import inference_quantization_manager as iqm
    q = iqm.TruncationOpManagerInference._load(types.SimpleNamespace(group=None), 'int4', {'int': dict(PARAMS, clipping='mix', pcq_act=True)})
    assert q.native_mix is True and q._asked(nhwc(), 'conv0') == 'mix'
    assert 'native_err=True' in inspect.getsource(iqm.QuantizationManagerInference)     # (its constructor needs a harness's arguments)
