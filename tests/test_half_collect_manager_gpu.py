"""`-sm collect` on contiguous bf16 / fp16 activations through the per-channel statistics manager and the harness (DESIGN.md
section 23): StatisticManagerPerChannel.save_tensor_stats takes ops.pc_stats_half itself, _route hands such an output over
without the upcast, the excluded cases keep the former route (the upcast, counted, then ops.pc_stats), and ResNet-18 at batch 4
runs `-pcq_a -sm collect --dtype bfloat16` then `-sm use -c laplace -baa` on the file it wrote."""
import contextlib
import glob
import importlib
import io
import os
import pickle
import types

import numpy as np
import pytest
import torch

import _half_collect as HC
from test_channels_last_collect_gpu import check_tiers, ref64

pytestmark = pytest.mark.gpu
STATS = ['max', 'min', 'std', 'mean', 'kurtosis', 'b', 'std_pos']
ERR = dict(num_bits=4, positive=False, bit_alloc=False, prior_is_b=False, target=None, round_mode=True)


def mods():
    from cnn_quantization_amd import _lib as L, ops
    from cnn_quantization_amd.inference import inference_quantization_manager as iqm
    from cnn_quantization_amd.inference import statistic_manager_perchannel as smpc
    return L, ops, iqm, smpc, importlib.import_module('cnn_quantization_amd.qtypes.int_quantizer')


def manager(name, **kw):
    smpc = mods()[3]
    smpc.Singleton._instances.pop(smpc.StatisticManagerPerChannel, None)
    return smpc.StatisticManagerPerChannel(name, load_stats=False, stats=STATS, **kw)


def spies(monkeypatch, ops):
    calls = {'half': 0, 'fp32': 0}
    half, fp32 = ops.pc_stats_half, ops.pc_stats

    def spy_half(*a, **kw):
        calls['half'] += 1
        return half(*a, **kw)

    def spy_fp32(x, *a, **kw):
        calls['fp32'] += 1
        assert x.dtype == torch.float32
        kw.pop('group', None)
        return fp32(x, *a, group=False, **kw)     # this rank's table: the routing is what is watched here, not the collective
    monkeypatch.setattr(ops, 'pc_stats_half', spy_half)
    monkeypatch.setattr(ops, 'pc_stats', spy_fp32)
    return calls


def test_manager_takes_the_half_route_itself(tmp_path, monkeypatch):
    L, ops, iqm, smpc, iq = mods()
    monkeypatch.setenv('HOME', str(tmp_path))
    calls = spies(monkeypatch, ops)
    batches = [HC.values((4, 12, 14, 14), seed=30 + k).to(torch.bfloat16).cuda() for k in range(2)]
    order = [L.STAT_MIN, L.STAT_MAX, L.STAT_MEAN, L.STAT_STD, L.STAT_B, L.STAT_KURT, L.STAT_STD_POS]
    try:
        before = (ops.LAYOUT_COPIES, iq.HALF_FALLBACKS)
        sm = manager('native')
        for x in batches:
            assert smpc.collects_native_half(sm, x)
            sm.save_tensor_stats(x, 'activation', 'conv0_activation')
        assert calls == {'half': 2, 'fp32': 0} and (ops.LAYOUT_COPIES, iq.HALF_FALLBACKS) == before
        for k, x in enumerate(batches):
            table = torch.stack([torch.from_numpy(sm.stats['conv0_activation'][n][k])
                                 for n in ('min', 'max', 'mean', 'std', 'b', 'kurtosis', 'std_pos')])
            st = torch.zeros(L.NSTAT, 12)
            st[order] = table
            direct = ops.pc_stats_half(x, True, True, True)[0].cpu()
            assert np.array_equal(st.numpy().view(np.int32), direct.numpy().view(np.int32))      # the table of a direct call
            check_tiers(st, ref64(x))
        # the manager asks for the rows it records, no more
        sm = manager('few')
        sm.stats_names = ['max', 'min', 'mean', 'std']
        sm.save_tensor_stats(batches[0], 'activation', 'conv0_activation')
        assert set(sm.stats['conv0_activation']) == {'max', 'min', 'mean', 'std'}
        # outputs without a spatial extent are not collected at all; float32 keeps its route
        calls.update(half=0, fp32=0)
        sm = manager('other')
        sm.save_tensor_stats(torch.zeros(4, 12, 1, 1, dtype=torch.bfloat16, device='cuda'), 'activation', 'fc')
        assert calls == {'half': 0, 'fp32': 0} and not sm.stats
        sm.save_tensor_stats(batches[0].float(), 'activation', 'conv0_activation')
        assert calls == {'half': 0, 'fp32': 1}
    finally:
        smpc.Singleton._instances.pop(smpc.StatisticManagerPerChannel, None)


def route_once(iqm, sm, x, **kw):
    """x through the common tail of the patched layers' forward, with a collecting quantization manager around sm."""
    qm = types.SimpleNamespace(enabled=True, stats_mode=iqm.StatsMode.collect_stats, stats_manager=sm,
                               err_settings=lambda out_id, tag, half_range: dict(ERR))
    old = iqm.QMI
    iqm.QMI = lambda: qm
    try:
        return iqm._route(None, x, 'conv0_activation', 'activation', **kw)
    finally:
        iqm.QMI = old


def test_route_hands_over_without_the_upcast_and_excluded_cases_keep_the_former_route(tmp_path, monkeypatch):
    """collect_err, batch_avg without forced extrema and an exchanging group (CNNQ_FORCE_EXCHANGE=1 on an initialised group and a
    world of two ranks both answer through distributed.forced_exchange / world_size, patched here: the predicate asks nothing
    else) all arrive at ops.pc_stats as float32, counted by upcast_fallback."""
    L, ops, iqm, smpc, iq = mods()
    from cnn_quantization_amd import distributed as D
    monkeypatch.setenv('HOME', str(tmp_path))
    calls = spies(monkeypatch, ops)
    x = HC.values((4, 12, 14, 14), seed=40).to(torch.bfloat16).cuda()
    try:
        sm = manager('native')
        fb = iq.HALF_FALLBACKS
        assert route_once(iqm, sm, x) is x
        assert calls == {'half': 1, 'fp32': 0} and iq.HALF_FALLBACKS == fb
        native = {n: sm.stats['conv0_activation'][n].copy() for n in STATS}
        for kw in (dict(collect_err=True), dict(batch_avg=True)):
            calls.update(half=0, fp32=0)
            sm = manager('excluded', **kw)
            assert not smpc.collects_native_half(sm, x)
            fb = iq.HALF_FALLBACKS
            assert route_once(iqm, sm, x) is x
            assert calls['half'] == 0 and calls['fp32'] >= 1 and iq.HALF_FALLBACKS == fb + 1, (kw, calls)
            for n in ('std', 'mean', 'b', 'std_pos'):          # the same statistics either way
                np.testing.assert_allclose(sm.stats['conv0_activation'][n], native[n], rtol=2e-6, atol=2e-6, err_msg=n)
        # ... unless the caller forces the extrema of the whole batch
        calls.update(half=0, fp32=0)
        sm = manager('forced', batch_avg=True)
        fb = iq.HALF_FALLBACKS
        route_once(iqm, sm, x, force_global=True)
        assert calls == {'half': 1, 'fp32': 0} and iq.HALF_FALLBACKS == fb
        # an exchanging group: the forced exchange of one rank, two ranks
        for name, value in (('forced_exchange', lambda: True), ('world_size', lambda group=None: 2)):
            calls.update(half=0, fp32=0)
            sm = manager('group')
            fb = iq.HALF_FALLBACKS
            with monkeypatch.context() as m:
                m.setattr(D, name, value)
                m.setattr(D, 'xrank_checkpoint', lambda group=None: True)
                assert not smpc.collects_native_half(sm, x)
                route_once(iqm, sm, x)
            assert calls == {'half': 0, 'fp32': 1} and iq.HALF_FALLBACKS == fb + 1, (name, calls)
        # a class of layer the route function sends back
        calls.update(half=0, fp32=0)
        sm = manager('sent_back')
        with monkeypatch.context() as m:
            m.setattr(ops, '_stats_half_native', lambda N, C, HW, dtype: False)
            route_once(iqm, sm, x)
        assert calls == {'half': 0, 'fp32': 1}
    finally:
        smpc.Singleton._instances.pop(smpc.StatisticManagerPerChannel, None)


def test_resnet18_bf16_collect_then_use(tmp_path, monkeypatch):
    L, ops, iqm, smpc, iq = mods()
    from cnn_quantization_amd.harness import inference_sim as H
    from cnn_quantization_amd.utils.misc import Singleton
    monkeypatch.setenv('HOME', str(tmp_path))
    base = ['-a', 'resnet18', '-b', '4', '-pcq_w', '-pcq_a', '--qtype', 'int4', '-qw', 'int4', '--dtype', 'bfloat16']
    native, upcast = [], []
    stats_half, fallback = ops.pc_stats_half, iqm.upcast_fallback

    def spy_stats(x, *a, **kw):
        fb, copies = iq.HALF_FALLBACKS, ops.LAYOUT_COPIES
        out = stats_half(x, *a, **kw)
        native.append((x.dtype, x.dim(), x.is_contiguous(), iq.HALF_FALLBACKS == fb, ops.LAYOUT_COPIES == copies))
        return out

    def spy_fallback(fn, *a, **kw):
        t = a[0] if a and isinstance(a[0], torch.Tensor) else None
        if getattr(fn, '__name__', '') == 'save_tensor_stats' and t is not None and t.dim() == 4 and (t.shape[2] > 1 or t.shape[3] > 1):
            upcast.append(tuple(t.shape))
        return fallback(fn, *a, **kw)
    monkeypatch.setattr(ops, 'pc_stats_half', spy_stats)
    monkeypatch.setattr(iqm, 'upcast_fallback', spy_fallback)
    Singleton.reset()
    with contextlib.redirect_stdout(io.StringIO()):
        assert H.run(H.build_parser().parse_args(base + ['-sm', 'collect']), quiet=True)['output_finite']
    monkeypatch.undo()
    monkeypatch.setenv('HOME', str(tmp_path))
    assert len(native) >= 10, len(native)                                          # the per-channel conv activations
    assert all(c == (torch.bfloat16, 4, True, True, True) for c in native), native
    assert not upcast, 'a 4-D activation reached the statistics manager through the upcast: %r' % (upcast,)
    # the statistics file loads: per layer a frame of float32 columns, one row per channel
    files = glob.glob(os.path.join(str(tmp_path), 'mxt-sim', 'statistics', 'per_channel', '*', '*_summary.pkl'))
    assert len(files) == 1, files
    with open(files[0], 'rb') as f:
        summary = pickle.load(f)
    assert len(summary) >= 10
    for layer, df in summary.items():
        assert len(df) in (64, 128, 256, 512) and {'mean_max', 'mean_min', 'mean_std', 'mean_mean', 'mean_b'} <= set(df.columns), layer
        assert all(str(t) == 'float32' for t in df.dtypes), layer
        assert bool((df['mean_std'] >= 0).all()) and bool((df['mean_max'] >= df['mean_min']).all()), layer
    # (`-sm use` also loads the per-tensor file, for the layers that are not quantized per channel)
    Singleton.reset()
    with contextlib.redirect_stdout(io.StringIO()):
        assert H.run(H.build_parser().parse_args([a for a in base if a != '-pcq_a'] + ['-sm', 'collect']), quiet=True)['output_finite']
    Singleton.reset()
    with contextlib.redirect_stdout(io.StringIO()):
        res = H.run(H.build_parser().parse_args(base + ['-sm', 'use', '-c', 'laplace', '-baa']), quiet=True)
    Singleton.reset()
    assert res['output_finite'] and bool(torch.isfinite(res['logits'].float()).all())
