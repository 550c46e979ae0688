"""Per-channel clipping-error columns on the device (cnnq_pc_qerr / ops.pc_quant_errors, collect_err of the per-channel
statistics manager) against the CPU restatement tests/_qerr.py and the rows produced by the reference (tests/golden/qerr.npz).
Bounds: 2e-6 relative (the project's tier (ii) bound for sums) on mse and on cos - the restatement asserts on the CPU that no
dot product cancels (sum |x q| <= 2 |sum x q|), so the bound carries over to it."""
import argparse
import contextlib
import io
import os
import pickle

import numpy as np
import pytest
import torch

import _qerr

pytestmark = pytest.mark.gpu
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'qerr.npz'))
SETTINGS = [dict(num_bits=4, positive=False, bit_alloc=False), dict(num_bits=4, positive=True, bit_alloc=False),
            dict(num_bits=4, positive=False, bit_alloc=True), dict(num_bits=4, positive=True, bit_alloc=True, prior_is_b=True)]
# the load shapes and geometry classes of the statistics tests: (N, C, H, W, 4-byte offset of the pointer)
GEOS = [(2, 4, 112, 112, 0), (3, 8, 56, 56, 0), (4, 16, 28, 28, 0), (5, 24, 14, 14, 0), (6, 40, 7, 7, 0), (3, 5, 9, 5, 0),
        (2, 3, 20, 20, 0), (1, 6, 12, 12, 0), (4, 8, 28, 28, 1), (3, 300, 7, 7, 0)]


def _input(N, C, H, W, off, seed):
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(N, C, H, W, generator=g) * torch.exp(torch.randn(1, C, 1, 1, generator=g) * 0.5)
         + torch.randn(1, C, 1, 1, generator=g) * 0.3 + 0.4).float()
    buf = torch.empty(x.numel() + 4, dtype=torch.float32, device='cuda')
    xd = buf[off:off + x.numel()].view(x.shape)
    xd.copy_(x)
    assert xd.data_ptr() % 16 == 4 * off and xd.is_contiguous()
    return x, xd


def _device_case(x, xd, settings):
    from cnn_quantization_amd import _lib as L
    from cnn_quantization_amd import ops
    N, C, HW = ops.geometry(xd)
    table, _ = ops.pc_stats(xd, N, C, HW, need_b=True)
    qp_l, qp_g, qp_p = ops.mix_candidates(table, **settings)
    ref, _ = _qerr.mix_columns(x, _qerr.stats_dict(table), **settings)
    return (N, C, HW), (qp_p, qp_g, qp_l), table[[L.STAT_MIN, L.STAT_MAX]], ref


@pytest.mark.parametrize('geo', GEOS, ids=lambda g: '%dx%dx%dx%d+%d' % g)
@pytest.mark.parametrize('si', range(len(SETTINGS)))
def test_quant_errors_match_restatement(geo, si):
    from cnn_quantization_amd import ops
    x, xd = _input(*geo, seed=100 + si)
    (N, C, HW), qps, mm, ref = _device_case(x, xd, SETTINGS[si])
    for K in (1, 2, 3):
        sel = list(range(K)) + [3 + k for k in range(K)]
        a = ops.pc_quant_errors(xd, N, C, HW, qps[:K])
        b = ops.pc_quant_errors(xd, N, C, HW, qps[:K], mm=mm)
        a2 = ops.pc_quant_errors(xd, N, C, HW, qps[:K])
        assert a.shape == (2 * K, C) and a.dtype == torch.float32
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))      # with / without mm: bit for bit
        assert torch.equal(a.view(torch.int32), a2.view(torch.int32))     # run after run: bit for bit
        got = a.cpu().numpy()
        print(geo, si, K, 'mse rel %.3g cos rel %.3g' % (_qerr.rel_err(got[:K], ref[sel[:K]]), _qerr.rel_err(got[K:], ref[sel[K:]])))
        assert _qerr.close(got, ref[sel], 2e-6)


@pytest.mark.parametrize('case', ['qmax0', 'nan'])
def test_constant_qmax0_and_nan_channels(case):
    """A constant channel, an all-zero channel, and: a channel whose candidate has qmax == 0 (bit allocation; it runs on
    its own because a NaN statistic poisons the allocation of every channel, here as in the reference) / a channel holding a NaN."""
    from cnn_quantization_amd import _lib as L
    from cnn_quantization_amd import ops
    g = torch.Generator().manual_seed(5)
    N, C, H, W = 4, 8, 14, 14
    x = torch.randn(N, C, H, W, generator=g) * torch.tensor([1e-3, 1., 3., .01, 2., 1., 5., 1.]).view(1, C, 1, 1)
    x[:, 1] = 0.75                      # constant
    x[:, 2] = 0.                        # constant zero: every sum 0, cos 0 / 0
    if case == 'nan':
        x[1, 5, 3, 3] = float('nan')
    xd = x.cuda()
    settings = dict(num_bits=4, positive=False, bit_alloc=case == 'qmax0', target=2.)
    table, _ = ops.pc_stats(xd, N, C, H * W, need_b=True)
    qps = ops.mix_candidates(table, **settings)
    if case == 'qmax0':
        assert bool((torch.stack(qps)[:, L.QP_QMAX] == 0).any())        # bit allocation gave some channel 0 bits
    # values only: a 0-bit candidate is a constant, so its dot product with a zero-mean channel cancels by construction
    qs = [_qerr.candidate_q(x, _qerr.stats_dict(table), c, **settings) for c in _qerr.CANDS]
    ref = _qerr.error_columns(x, qs, check_no_cancellation=False)
    for mm in (None, table[[L.STAT_MIN, L.STAT_MAX]]):
        got = ops.pc_quant_errors(xd, N, C, H * W, (qps[2], qps[1], qps[0]), mm=mm).cpu().numpy()
        if case == 'nan':
            assert np.isnan(got[:, 5]).all() and np.isnan(ref[:, 5]).all()
        print(case, got, ref)
        assert _qerr.close(got, ref, 2e-6)
        post = _qerr.host_post(got)
        assert (post[3:, 2] == 1).all() and np.isfinite(post[3:]).all()
        if case == 'nan':
            assert (post[3:, 5] == 1).all()


@pytest.mark.parametrize('poison', [float('nan'), float('inf')])
def test_bit_allocation_poisoned_by_nan_or_inf(poison):
    """Bit allocation on and one NaN / Inf activation: the allocation's prior is poisoned, so EVERY channel's bit width, qmax
    (and, for Inf, some zero points) come out NaN while the healthy channels keep finite extrema.  The divide-free quotient
    clamps with v_med3, which treats a NaN bound unlike qdq1's compare+select: such channels must stay on the IEEE route.  The
    reference cannot build these candidates (its table lookup raises on a NaN bit width), so the expected rows are the
    restatement's formulas applied to what cnnq_pc_qdq stores for the same tables - which is what q_k is defined to be."""
    from cnn_quantization_amd import _lib as L
    from cnn_quantization_amd import ops
    g = torch.Generator().manual_seed(6)
    N, C, H, W = 4, 8, 14, 14
    x = torch.randn(N, C, H, W, generator=g) * torch.tensor([.5, 1., 3., .1, 2., 1., 5., 1.]).view(1, C, 1, 1)
    x[2, 4, 5, 5] = poison
    xd = x.cuda()
    table, _ = ops.pc_stats(xd, N, C, H * W, need_b=True)
    qps = ops.mix_candidates(table, num_bits=4, positive=False, bit_alloc=True)
    qps = (qps[2], qps[1], qps[0])
    assert bool(torch.isnan(torch.stack(qps)[:, L.QP_QMAX]).all())                  # poisoned: every channel
    assert bool(torch.isfinite(table[[L.STAT_MIN, L.STAT_MAX]][:, [0, 1, 2, 3, 5, 6, 7]]).all())
    ys = [ops.pc_qdq(xd, N, C, H * W, q).cpu() for q in qps]
    ref = _qerr.error_columns(x, ys, check_no_cancellation=False)
    a = ops.pc_quant_errors(xd, N, C, H * W, qps)
    b = ops.pc_quant_errors(xd, N, C, H * W, qps, mm=table[[L.STAT_MIN, L.STAT_MAX]])
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))                    # with / without mm: bit for bit
    print(poison, a.cpu().numpy(), ref)
    assert _qerr.close(a.cpu().numpy(), ref, 2e-6)


def test_rejects_what_the_statistics_ops_reject():
    from cnn_quantization_amd import _lib as L
    from cnn_quantization_amd import ops
    qp = torch.ones(3, 4, device='cuda')
    x = torch.randn(2, 4, 4, 4, device='cuda')
    for bad in (x.half(), x.to(memory_format=torch.channels_last), x.cpu()):
        with pytest.raises(L.CnnqError):
            ops.pc_quant_errors(bad, 2, 4, 16, [qp])
    with pytest.raises(L.CnnqError):
        ops.pc_quant_errors(x, 2, 4, 16, [qp] * 4)


def _manager(tmp_path, monkeypatch, name, **kw):
    from cnn_quantization_amd.inference import statistic_manager_perchannel as smpc
    from cnn_quantization_amd.utils.misc import Singleton
    monkeypatch.setenv('HOME', str(tmp_path))
    Singleton._instances.pop(smpc.StatisticManagerPerChannel, None)
    return smpc.StatisticManagerPerChannel(name, **kw)


@pytest.mark.parametrize('name', [str(n) for n in GOLD['names']])
def test_manager_reproduces_reference_rows(name, tmp_path, monkeypatch):
    half, baa = name[4] == '1', name[-1] == '1'
    xd = torch.from_numpy(GOLD['x']).cuda()
    plain = _manager(tmp_path, monkeypatch, 'plain', load_stats=False)
    plain.save_tensor_stats(xd, 'activation', 'conv0_activation')
    sm = _manager(tmp_path, monkeypatch, 'err', load_stats=False, collect_err=True,
                  err_settings=dict(num_bits=4, positive=half, bit_alloc=baa, prior_is_b=False, target=4, round_mode=True))
    sm.save_tensor_stats(xd, 'activation', 'conv0_activation')
    rec = sm.stats['conv0_activation']
    for s in ('max', 'min', 'std', 'mean', 'kurtosis', 'b', 'std_pos'):
        assert np.array_equal(rec[s].view(np.int32), plain.stats['conv0_activation'][s].view(np.int32)), s
    for en in _qerr.NAMES:
        print(name, en, 'rel %.3g' % _qerr.rel_err(rec[en], GOLD['%s_%s' % (name, en)]))
        assert _qerr.close(rec[en], GOLD['%s_%s' % (name, en)], 2e-6), en


def test_collect_then_use_mix_end_to_end(tmp_path, monkeypatch):
    """-sm collect with collect_err -> the pickle -> a fresh -sm use -c mix quantizer: the picks are the restatement's."""
    from cnn_quantization_amd import ops
    from cnn_quantization_amd.qtypes import int_quantizer
    x = _qerr.mixed_input()
    xd = x.cuda()
    C = x.shape[1]
    settings = dict(num_bits=4, positive=False, bit_alloc=False, prior_is_b=False, target=4, round_mode=True)
    sm = _manager(tmp_path, monkeypatch, 'e2e', load_stats=False, collect_err=True, err_settings=lambda tag, half: settings)
    for _ in range(2):
        sm.save_tensor_stats(xd, 'activation', 'conv0_activation')
    sm.__exit__()
    with open(os.path.join(sm.folder, 'e2e_statistics_perchannel_summary.pkl'), 'rb') as f:
        df = pickle.load(f)['conv0_activation']
    assert len(df.columns) == 13 * 3
    file_rows = np.stack([df['mean_' + n].values for n in _qerr.NAMES])
    assert np.isfinite(file_rows[:3]).all()                                                     # (a)
    stats = {k: df['mean_' + k].values.astype(np.float32) for k in ('min', 'max', 'mean', 'b', 'std')}
    ref, _ = _qerr.mix_columns(x, stats, num_bits=4, positive=False, bit_alloc=False)
    want, margin = _qerr.picks(ref)
    assert margin.min() >= 1e-3
    got, _ = _qerr.picks(file_rows)
    assert np.array_equal(got, want)                                                            # (b): every channel
    assert set(want.tolist()) == {0, 1, 2}                                                      # (c)
    use = _manager(tmp_path, monkeypatch, 'e2e', load_stats=True)
    q = int_quantizer('int4', dict(clipping='mix', stats_kind='mean', kld=False, pcq_weights=False, pcq_act=True,
                                   bit_alloc_act=False, bit_alloc_weight=False, bit_alloc_rmode='round', bit_alloc_prior='gaus',
                                   bit_alloc_target_act=None, bit_alloc_target_weight=None, bcorr_act=False, bcorr_weight=False,
                                   vcorr_weight=False, logger=None, measure_entropy=False, mtd_quant=False))
    y = q(xd, 'conv0_activation', 'activation', stat_id='conv0_activation')
    table = torch.zeros(7, C)
    for row, k in ((0, 'min'), (1, 'max'), (2, 'mean'), (3, 'std'), (4, 'b')):
        table[row] = torch.from_numpy(stats[k])
    mse = torch.from_numpy(np.stack([ref[2], ref[1], ref[0]]).astype(np.float32))               # rows laplace, gaus, lowp
    y_ref = ops.act_qdq_mix(xd, 4, table.cuda(), mse)
    assert torch.equal(y.view(torch.int32), y_ref.view(torch.int32))                            # (d)
    assert use is not None


def test_harness_collect_err_then_mix(tmp_path, monkeypatch):
    from cnn_quantization_amd.harness import inference_sim as H
    from cnn_quantization_amd.utils.misc import Singleton
    monkeypatch.setenv('HOME', str(tmp_path))
    base = ['-a', 'resnet18', '-b', '8', '-pcq_a', '-pcq_w', '--qtype', 'int4', '-qw', 'int4']
    # `-sm use` also loads the per-tensor file (pooling / classifier quantizers): the middle run collects it, as in the README
    for argv in (base + ['-sm', 'collect', '-ce'], [a for a in base if a != '-pcq_a'] + ['-sm', 'collect'],
                 base + ['-sm', 'use', '-c', 'mix']):
        Singleton.reset()
        with contextlib.redirect_stdout(io.StringIO()):
            res = H.main(argv)
        assert res['output_finite']
    path = os.path.join(str(tmp_path), 'mxt-sim', 'statistics', 'per_channel', 'resnet18', 'resnet18_statistics_perchannel_summary.pkl')
    with open(path, 'rb') as f:
        summ = pickle.load(f)
    convs = [k for k in summ if k.startswith('conv')]
    assert len(convs) >= 17
    for k in convs:
        assert len(summ[k].columns) == 13 * 3 and np.isfinite(summ[k][['mean_mse_lowp', 'mean_mse_gaus', 'mean_mse_laplace']].values).all()
    for bad in (base + ['-ce'], ['-a', 'resnet18', '--qtype', 'int4', '-sm', 'collect', '-ce']):
        with pytest.raises(SystemExit), contextlib.redirect_stderr(io.StringIO()):
            H.main(bad)
    Singleton.reset()
