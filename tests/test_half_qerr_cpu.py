"""The error columns of contiguous bf16 / fp16 activations without a device: the C entry points' argument
checks and workspace size, collect_route with native_err_half over a small grid, and the call sequence of save_tensor_stats on
the route 'half', with the ops entry points stubbed.  Nothing is launched."""
import ctypes
import itertools

import numpy as np
import torch

from _quantizer import act, nhwc

EINVAL, ERANGE = -1, -2
F32, BF16, F16 = 0, 1, 2


def _route(lib, N, C, HW, dtype, align=16):
    out = (ctypes.c_int32 * 4)()
    rc = lib.cnnq_pc_route_qerr_dt(N, C, HW, dtype, align, out)
    return rc, list(out)


def test_argument_validation_needs_no_device():
    from cnn_quantization_amd import _lib as L
    lib = L.load()
    assert (L.DTYPE_F32, L.DTYPE_BF16, L.DTYPE_F16) == (F32, BF16, F16)
    ok = dict(x=64, dtype=BF16, N=2, C=8, HW=9, qp=64, K=3, mm=None, ws=64, err=64)

    def call(**kw):
        a = dict(ok, **kw)
        return lib.cnnq_pc_qerr_dt(a['x'], a['dtype'], a['N'], a['C'], a['HW'], a['qp'], a['K'], a['mm'], a['ws'], a['err'], None)
    # (the dummy pointers are never dereferenced: every case is refused before anything touches the device)
    for bad in (dict(x=None), dict(qp=None), dict(ws=None), dict(err=None), dict(K=0), dict(K=4), dict(dtype=3), dict(dtype=-1),
                dict(N=0), dict(HW=0), dict(C=0), dict(N=-1), dict(ws=68), dict(x=65), dict(x=65, dtype=F16)):
        assert call(**bad) == EINVAL, bad
    for dtype in (BF16, F16):
        assert call(N=1 << 31, dtype=dtype) == ERANGE and call(HW=1 << 31, dtype=dtype) == ERANGE
        assert call(C=1 << 16, HW=1 << 15, dtype=dtype) == ERANGE             # C * HW = 2^31
    # float32 forwards to cnnq_pc_qerr, whose refusals are the same ones
    for bad in (dict(x=None), dict(qp=None), dict(ws=None), dict(err=None), dict(K=0), dict(K=4), dict(N=0), dict(ws=68)):
        assert call(dtype=F32, **bad) == EINVAL, bad
    for bad in ((0, 8, 9, 3, BF16), (2, 0, 9, 3, BF16), (2, 8, 0, 3, BF16), (2, 8, 9, 0, BF16), (2, 8, 9, 4, BF16), (2, 8, 9, 3, 3),
                (2, 8, 9, 3, -1), (1 << 31, 8, 9, 3, BF16), (2, 8, 1 << 31, 3, F16), (2, 8, 9, 0, F32), (0, 8, 9, 3, F32)):
        assert lib.cnnq_pc_qerr_dt_workspace(*bad) == 0, bad
    assert lib.cnnq_pc_qerr_dt_workspace(2, 8, 9, 3, F32) == lib.cnnq_pc_qerr_workspace(2, 8, 9, 3) > 0
    assert _route(lib, 2, 8, 9, BF16, align=3)[0] == EINVAL
    assert _route(lib, 2, 8, 9, BF16, align=0)[0] == EINVAL
    assert _route(lib, 2, 8, 9, 7)[0] == EINVAL
    assert _route(lib, 0, 8, 9, BF16)[0] == EINVAL
    assert _route(lib, 1 << 31, 8, 9, BF16)[0] == ERANGE
    assert lib.cnnq_pc_route_qerr_dt(2, 8, 9, BF16, 16, None) == EINVAL
    rc, (w, nb, rows, native) = _route(lib, 2, 8, 16, F32)                    # float32: cnnq_pc_qerr's plan
    assert rc == 0 and w in (1, 4) and nb >= 1 and native == 1


SHAPES = [(2, 64, 144), (3, 6, 196), (3, 6, 30), (3, 6, 45), (3, 5, 49), (2, 1040, 49), (5, 16, 9), (1, 8, 1600), (2, 64, 2304),
          (512, 256, 3136), (1, 64, 12544), (512, 2048, 49)]


def test_workspace_is_the_row_records_of_the_plan_the_route_reports():
    from cnn_quantization_amd import _lib as L
    lib = L.load()
    cut = 0
    for (N, C, HW), dtype in itertools.product(SHAPES, (BF16, F16)):
        rc, (w, nb, rows, native) = _route(lib, N, C, HW, dtype)
        assert rc == 0 and w in (1, 2, 4, 8) and HW % w == 0
        assert native == (0 if (N, C, HW) == (512, 2048, 49) else 1)         # (a class the upcast route keeps: below)
        assert nb >= 1 and HW // w >= nb                                     # every column part holds a piece
        assert rows in (4, 8, 16, 32, 64, 128, 256)                          # a power-of-two segment of a wave per row
        for K in (1, 2, 3):
            assert lib.cnnq_pc_qerr_dt_workspace(N, C, HW, K, dtype) == N * nb * (1 + 3 * K) * C * 8
        last = w
        for align in (8, 4, 2):                                              # the record count does not depend on the alignment
            rc2, o2 = _route(lib, N, C, HW, dtype, align)
            assert rc2 == 0 and o2[1] == nb and o2[3] == native
            assert o2[0] <= last and HW % o2[0] == 0 and HW // o2[0] >= nb   # the pieces only shrink, and divide the row
            last = o2[0]
        assert last == 1                                                     # an x aligned to one element only
        assert _route(lib, N, C, HW, BF16)[1] == _route(lib, N, C, HW, F16)[1]
        cut += nb > 1
    assert cut > 0                                                           # some plan cuts a row into column parts
    assert _route(lib, 1, 8, 1600, BF16)[1][1] > 1 and _route(lib, 512, 256, 3136, BF16)[1][1] == 1
    # the native word: 0 where the measured step did not win - HW no multiple of 8, N * HW >= 16384, N * C * HW < 2^26
    word = lambda N, C, HW: _route(lib, N, C, HW, BF16)[1][3]
    assert [word(512, 512, 196), word(512, 256, 196), word(512, 512, 49), word(512, 2048, 49)] == [0, 0, 0, 0]
    assert [word(512, 1024, 196), word(512, 128, 784), word(512, 256, 3136), word(83, 512, 196), word(8, 512, 49)] == [1, 1, 1, 1, 1]
    # the widest of 8 / 4 / 2 / 1 that divides HW and the alignment
    assert [_route(lib, 3, 6, hw, BF16)[1][0] for hw in (144, 196, 30, 45, 49)] == [8, 4, 2, 1, 1]
    assert [_route(lib, 2, 64, 144, BF16, a)[1][0] for a in (16, 8, 4, 2)] == [8, 4, 2, 1]


def test_the_route_word_is_asked_once_per_class_and_is_patchable(monkeypatch):
    from cnn_quantization_amd import ops
    monkeypatch.setattr(ops, '_QERR_HALF_NATIVE', {})
    assert ops._qerr_half_native(2, 8, 16, torch.bfloat16) is True
    assert ops._QERR_HALF_NATIVE == {(2, 8, 16, torch.bfloat16): True}
    ops._QERR_HALF_NATIVE[(2, 8, 16, torch.bfloat16)] = False               # (the cache answers)
    assert ops._qerr_half_native(2, 8, 16, torch.bfloat16) is False


# ---- routes
def _managers(monkeypatch, tmp_path):
    from cnn_quantization_amd.inference import statistic_manager_perchannel as smpc
    from cnn_quantization_amd.utils.misc import Singleton
    monkeypatch.setenv('HOME', str(tmp_path))
    for collect_err, native_err, native_err_half, batch_avg in itertools.product((False, True), repeat=4):
        Singleton.reset()
        yield smpc.StatisticManagerPerChannel('t', load_stats=False, collect_err=collect_err, batch_avg=batch_avg, native_err=native_err,
                                              native_err_half=native_err_half, err_settings=dict(num_bits=4))
    Singleton.reset()


TENSORS = [('nhwc_bf16', lambda: nhwc()), ('nhwc_f16', lambda: nhwc(torch.float16)), ('nhwc_f32', lambda: nhwc(torch.float32)),
           ('act_bf16', lambda: act()), ('act_f16', lambda: act(torch.float16)), ('act_f32', lambda: act(torch.float32)),
           ('nhwc_f64', lambda: nhwc(torch.float64)), ('fc', lambda: act(shape=(2, 8))), ('flat', lambda: act(shape=(2, 8, 1, 1)))]
HALF = {'act_bf16', 'act_f16'}


def _parent(manager, name, force):
    """collect_route's answer before native_err_half existed (tests/test_nhwc_qerr_cpu.py holds the parent to it)."""
    if manager.batch_avg and not force:
        return None
    plain = {'nhwc_bf16': 'nhwc', 'nhwc_f16': 'nhwc', 'nhwc_f32': 'nhwc', 'act_bf16': 'half', 'act_f16': 'half'}.get(name)
    if not manager.collect_err:
        return plain
    return 'nhwc' if manager.native_err and plain == 'nhwc' else None


def test_collect_route_answers_half_only_with_both_flags(monkeypatch, tmp_path):
    from cnn_quantization_amd import distributed as D, ops
    asked = []
    monkeypatch.setattr(ops, '_stats_nhwc_native', lambda *a: True)
    monkeypatch.setattr(ops, '_stats_half_native', lambda *a: True)
    monkeypatch.setattr(ops, '_qerr_nhwc_native', lambda *a: True)
    monkeypatch.setattr(ops, '_qerr_half_native', lambda *a: asked.append(a) or True)
    gained = 0
    for manager in _managers(monkeypatch, tmp_path):
        for (name, make), force in itertools.product(TENSORS, (False, True)):
            x = make()
            n_asked = len(asked)
            got = manager.collect_route(x, force)
            new = (manager.collect_err and manager.native_err and manager.native_err_half and name in HALF
                   and (not manager.batch_avg or force))
            want = 'half' if new else _parent(manager, name, force)
            assert got == want, (manager.collect_err, manager.native_err, manager.native_err_half, manager.batch_avg, name, force, got)
            if new:
                assert _parent(manager, name, force) is None                   # (the cell the parent sends to the upcast route)
                assert asked[n_asked:] == [(2, 8, 16, x.dtype)]                # (N, C, HW, dtype) of the class of layer
                gained += 1
            else:
                assert len(asked) == n_asked                                   # nobody else asks the new word
    assert gained == 2 * 3                                                     # two tensors x (batch_avg off x force, batch_avg forced)

    # opted in, and still the upcast route: several ranks, a forced exchange, either route word
    from cnn_quantization_amd.inference import statistic_manager_perchannel as smpc
    from cnn_quantization_amd.utils.misc import Singleton
    Singleton.reset()
    manager = smpc.StatisticManagerPerChannel('t', load_stats=False, collect_err=True, native_err=True, native_err_half=True)
    x = act()
    assert manager.collect_route(x) == 'half' and smpc.collects_native_half(manager, x)
    with monkeypatch.context() as m:
        m.setattr(D, 'world_size', lambda group=None: 2)
        assert manager.collect_route(x) is None
    with monkeypatch.context() as m:
        m.setattr(D, 'forced_exchange', lambda: True)
        assert manager.collect_route(x) is None
    with monkeypatch.context() as m:
        m.setattr(ops, '_stats_half_native', lambda *a: False)
        assert manager.collect_route(x) is None
    with monkeypatch.context() as m:
        m.setattr(ops, '_qerr_half_native', lambda *a: False)
        assert manager.collect_route(x) is None
    with monkeypatch.context() as m:
        m.setattr(ops, '_NHWC', False)                                         # a contiguous half tensor does not ask the switch
        assert manager.collect_route(x) == 'half'
    manager.native_err = False                                                 # native_err_half alone opts into nothing
    assert manager.collect_route(x) is None and manager.collect_route(nhwc()) is None
    manager.native_err = True
    assert manager.collect_route(x) == 'half'
    # a default-constructed manager keeps the parent's attribute values
    Singleton.reset()
    plain = smpc.StatisticManagerPerChannel('t', load_stats=False, collect_err=True)
    assert plain.native_err is False and plain.native_err_half is False and plain.collect_route(x) is None
    Singleton.reset()


def test_save_tensor_stats_on_the_route_calls_the_half_entry_points_in_order(monkeypatch, tmp_path):
    from cnn_quantization_amd import _lib as L, ops
    from cnn_quantization_amd.inference import statistic_manager_perchannel as smpc
    from cnn_quantization_amd.utils.misc import Singleton
    monkeypatch.setenv('HOME', str(tmp_path))
    calls = []
    C = 8
    table = torch.arange(L.NSTAT * C, dtype=torch.float32).view(L.NSTAT, C)
    err = -torch.arange(6 * C, dtype=torch.float32).view(6, C) - 1.

    def stats(x, **kw):
        calls.append(('pc_stats_half', x.dtype, x.is_contiguous(), kw['need_b']))
        return table, None

    def cands(t, **settings):
        calls.append(('mix_candidates', t is table, settings))
        return 'l', 'g', 'p'

    def errors(x, qps, mm=None):
        calls.append(('pc_quant_errors_half', x.dtype, x.is_contiguous(), tuple(qps), torch.equal(mm, table[[L.STAT_MIN, L.STAT_MAX]])))
        return err

    def refuse(*a, **kw):
        raise AssertionError('another route was taken')
    monkeypatch.setattr(ops, 'pc_stats_half', stats)
    monkeypatch.setattr(ops, 'mix_candidates', cands)
    monkeypatch.setattr(ops, 'pc_quant_errors_half', errors)
    for name in ('pc_stats', 'pc_quant_errors', 'pc_stats_nhwc', 'pc_quant_errors_nhwc'):
        monkeypatch.setattr(ops, name, refuse)
    monkeypatch.setattr(ops, '_stats_half_native', lambda *a: True)
    monkeypatch.setattr(ops, '_qerr_half_native', lambda *a: True)
    Singleton.reset()
    try:
        manager = smpc.StatisticManagerPerChannel('t', load_stats=False, collect_err=True, native_err=True, native_err_half=True,
                                                  err_settings=lambda tag, half: dict(num_bits=4, positive=half))
        manager.save_tensor_stats(act(), 'activation', 'conv0_activation', half_range=True)
        assert calls == [('pc_stats_half', torch.bfloat16, True, True), ('mix_candidates', True, dict(num_bits=4, positive=True)),
                         ('pc_quant_errors_half', torch.bfloat16, True, ('p', 'g', 'l'), True)]
        del calls[:]
        manager.save_tensor_stats(act(torch.float16), 'activation', 'conv1_activation', route='half')   # a caller that has asked
        assert [c[:2] for c in calls] == [('pc_stats_half', torch.float16), ('mix_candidates', True), ('pc_quant_errors_half', torch.float16)]
        rec = manager.stats['conv0_activation']
        assert np.array_equal(rec['b'], table[L.STAT_B].numpy())
        for i, name in enumerate(smpc.ERR_NAMES):
            assert np.array_equal(rec[name], err[i].numpy()), name
    finally:
        Singleton.reset()


def test_the_inference_manager_opts_in():
    import inspect
    from cnn_quantization_amd.inference import inference_quantization_manager as iqm
    src = inspect.getsource(iqm.QuantizationManagerInference)                  # (its constructor needs a harness's arguments)
    assert 'native_err=True' in src and 'native_err_half=True' in src
