"""The clipping-error columns of `-c mix` on contiguous bf16 / fp16 activations (cnnq_pc_qerr_dt / ops.pc_quant_errors_half, the
statistics manager's native_err_half) against the CPU restatement tests/_qerr.py on the exactly upconverted
tensor.  Bound: 2e-6 relative, the project's tier (ii) bound for sums, which the fp32 NCHW kernel (tests/test_qerr_gpu.py) and the
channels_last kernel (tests/test_nhwc_qerr_gpu.py) are held to; the restatement asserts on the CPU that no dot product cancels.
The inputs are _qerr.mixed_input's channels times a factor per SAMPLE, so that the nested root of the cosine tells a per-row
record from a per-channel one."""
import contextlib
import ctypes
import functools
import importlib
import io
import os
import pickle

import numpy as np
import pytest
import torch

import _qerr
from test_qerr_gpu import SETTINGS

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]
# (N, C, H, W): W = 8 and a row shorter than a wave (18 pieces over 4 lanes); W = 4; W = 2; W = 1 with an odd HW and N no multiple
# of the rows of a step (twice); many channels; rows of a few pieces; rows of several steps (cut into column parts, as every batch
# of fewer than 4096 rows of 1024 elements or more is); column parts of 66 and 67 pieces: a remainder; whole rows of several steps;
# single elements with a remainder for a segment of 32 lanes (169) and for a whole wave (289)
SHAPES = [(2, 64, 12, 12), (3, 6, 14, 14), (3, 6, 6, 5), (3, 6, 9, 5), (3, 5, 7, 7), (2, 1040, 7, 7), (5, 16, 3, 3), (2, 64, 48, 48),
          (1, 8, 40, 40), (4, 16, 24, 24), (3, 6, 13, 13), (3, 6, 17, 17)]
# the route's report at 16-byte alignment: (piece width, column parts, rows a workgroup takes per step)
PLAN = {(2, 64, 12, 12): (8, 1, 64), (3, 6, 14, 14): (4, 1, 32), (3, 6, 6, 5): (2, 1, 64), (3, 6, 9, 5): (1, 1, 32), (3, 5, 7, 7): (1, 1, 32),
        (2, 1040, 7, 7): (1, 1, 32), (5, 16, 3, 3): (1, 1, 64), (2, 64, 48, 48): (8, 4, 64), (1, 8, 40, 40): (8, 3, 64),
        (4, 16, 24, 24): (8, 1, 64), (3, 6, 13, 13): (1, 1, 8), (3, 6, 17, 17): (1, 1, 4)}
_ID = dict(ids=lambda s: '%dx%dx%dx%d' % s)
_DT = dict(ids=lambda d: str(d).replace('torch.', ''))


def _mods():
    from cnn_quantization_amd import _lib as L, ops
    return L, ops, importlib.import_module('cnn_quantization_amd.qtypes.int_quantizer')


@contextlib.contextmanager
def _still():
    """Neither a layout copy nor an upcast inside the block."""
    _, ops, iq = _mods()
    before = ops.LAYOUT_COPIES, iq.HALF_FALLBACKS
    yield
    assert (ops.LAYOUT_COPIES, iq.HALF_FALLBACKS) == before


def _values(N, C, H, W, seed):
    """_qerr.mixed_input's twelve channels, drawn again for every twelve of C (its scales grow with the channel index: a thousand
    channels in one draw would leave the bit allocation no bits for the first ones), times a factor per sample."""
    g = torch.Generator().manual_seed(seed + 1000)
    x = torch.cat([_qerr.mixed_input(seed + 7919 * j, N, min(12, C - j), H, W) for j in range(0, C, 12)], dim=1)
    return x * torch.exp(0.7 * torch.randn(N, 1, 1, 1, generator=g))


def _place(x, dtype, off=0):
    """(the upconverted values on the CPU, the contiguous tensor of `dtype` on the device, `off` elements into its buffer)."""
    buf = torch.empty(x.numel() + 8, dtype=dtype, device='cuda')
    xd = buf[off:off + x.numel()].view(x.shape)
    xd.copy_(x.to(dtype))
    assert xd.is_contiguous() and xd.data_ptr() % 16 == (2 * off) % 16
    return xd.float().cpu().contiguous(), xd


def _route(xd):
    L, ops, _ = _mods()
    out = (ctypes.c_int32 * 4)()
    align = 16 if xd.data_ptr() % 16 == 0 else xd.data_ptr() & -xd.data_ptr()
    assert L.load().cnnq_pc_route_qerr_dt(*ops.geometry(xd), ops._DTYPE_CODES[xd.dtype], align, out) == 0
    return list(out)


@functools.lru_cache(maxsize=None)
def _case(shape, dtype, si, off=0):
    """One placed input, its table and candidates, and the restatement's six columns - computed once, shared, never written to."""
    L, ops, _ = _mods()
    xf, xd = _place(_values(*shape, seed=100 + si), dtype, off)
    table, _ = ops.pc_stats_half(xd, need_b=True)
    qp_l, qp_g, qp_p = ops.mix_candidates(table, **SETTINGS[si])
    ref, _ = _qerr.mix_columns(xf, _qerr.stats_dict(table), **SETTINGS[si])
    return xf, xd, table, (qp_p, qp_g, qp_l), table[[L.STAT_MIN, L.STAT_MAX]], ref


def _check_columns(shape, dtype, si, Ks, off=0):
    _, ops, _ = _mods()
    xf, xd, table, qps, mm, ref = _case(shape, dtype, si, off)
    C = shape[1]
    for K in Ks:
        with _still():
            a = ops.pc_quant_errors_half(xd, qps[:K])
            b = ops.pc_quant_errors_half(xd, qps[:K], mm=mm)
            a2 = ops.pc_quant_errors_half(xd, qps[:K])
        assert a.shape == (2 * K, C) and a.dtype == torch.float32
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))          # with / without mm: bit for bit
        assert torch.equal(a.view(torch.int32), a2.view(torch.int32))         # run after run: bit for bit
        got = a.cpu().numpy()
        sel = list(range(K)) + [3 + k for k in range(K)]
        print(shape, dtype, si, K, off, 'mse rel %.3g cos rel %.3g' % (_qerr.rel_err(got[:K], ref[sel[:K]]),
                                                                       _qerr.rel_err(got[K:], ref[sel[K:]])))
        assert _qerr.close(got, ref[sel], 2e-6)


@pytest.mark.parametrize('dtype', DTYPES, **_DT)
@pytest.mark.parametrize('shape', SHAPES, **_ID)
def test_quant_errors_match_restatement(shape, dtype):
    w, nb, rows, native = _route(_case(shape, dtype, 0)[1])
    assert (w, nb, rows) == PLAN[shape] and native == 1                      # the branch the shape is here for
    assert PLAN[(1, 8, 40, 40)][1] > 1
    for si in range(len(SETTINGS)):
        _check_columns(shape, dtype, si, (3,))


@pytest.mark.parametrize('dtype', DTYPES, **_DT)
def test_one_and_two_candidates(dtype):
    _check_columns((3, 6, 14, 14), dtype, 0, (1,))
    _check_columns((2, 64, 12, 12), dtype, 2, (2,))


@pytest.mark.parametrize('dtype', DTYPES, **_DT)
def test_a_view_one_element_into_a_buffer_takes_single_elements(dtype):
    shape = (2, 64, 12, 12)
    xd = _case(shape, dtype, 1, 1)[1]
    assert xd.data_ptr() % 4 == 2 and _route(xd)[0] == 1
    _check_columns(shape, dtype, 1, (3,), off=1)
    # the same values, aligned: other pieces, another order of the additions, the same columns within the tier
    _, ops, _ = _mods()
    xf, _, _, qps, mm, _ = _case(shape, dtype, 1, 1)
    aligned = _place(xf, dtype)[1]
    a, b = ops.pc_quant_errors_half(xd, qps, mm=mm).cpu().numpy(), ops.pc_quant_errors_half(aligned, qps, mm=mm).cpu().numpy()
    assert _qerr.close(a, b, 2 * 2e-6)


@pytest.mark.parametrize('shape', SHAPES, **_ID)
def test_agrees_with_the_fp32_kernel_on_the_same_values(shape):
    """Both kernels are within the tier of the same fp64 value; equality is not promised."""
    L, ops, _ = _mods()
    x = _values(*shape, seed=7)
    x[0, shape[1] // 2, 1, 1] = float('nan')
    xf, xd = _place(x, torch.bfloat16)
    N, C, HW = ops.geometry(xd)
    table, _ = ops.pc_stats_half(xd, need_b=True)
    qp_l, qp_g, qp_p = ops.mix_candidates(table, **SETTINGS[0])
    with _still():
        got = ops.pc_quant_errors_half(xd, (qp_p, qp_g, qp_l)).cpu().numpy()
    want = ops.pc_quant_errors(xf.cuda(), N, C, HW, (qp_p, qp_g, qp_l)).cpu().numpy()
    assert np.isnan(want[:, shape[1] // 2]).all() and np.isnan(want).sum() == 6
    assert _qerr.close(got, want, 2 * 2e-6)                                   # the NaN columns are the same columns


@pytest.mark.parametrize('dtype', DTYPES, **_DT)
@pytest.mark.parametrize('case', ['qmax0', 'nan'])
def test_constant_qmax0_and_nan_channels(case, dtype):
    """test_nhwc_qerr_gpu's special channels on contiguous half storage: a constant channel, an all-zero channel, and a 0-bit
    candidate / a channel holding one NaN (only its columns are NaN)."""
    L, ops, _ = _mods()
    g = torch.Generator().manual_seed(5)
    N, C, H, W = 4, 8, 14, 14
    x = torch.randn(N, C, H, W, generator=g) * torch.tensor([1e-3, 1., 3., .01, 2., 1., 5., 1.]).view(1, C, 1, 1)
    x[:, 1] = 0.75
    x[:, 2] = 0.
    if case == 'nan':
        x[1, 5, 3, 3] = float('nan')
    xf, xd = _place(x, dtype)
    settings = dict(num_bits=4, positive=False, bit_alloc=case == 'qmax0', target=2.)
    table, _ = ops.pc_stats_half(xd, need_b=True)
    qps = ops.mix_candidates(table, **settings)
    if case == 'qmax0':
        assert bool((torch.stack(qps)[:, L.QP_QMAX] == 0).any())
    qs = [_qerr.candidate_q(xf, _qerr.stats_dict(table), c, **settings) for c in _qerr.CANDS]
    ref = _qerr.error_columns(xf, qs, check_no_cancellation=False)
    for mm in (None, table[[L.STAT_MIN, L.STAT_MAX]]):
        with _still():
            got = ops.pc_quant_errors_half(xd, (qps[2], qps[1], qps[0]), mm=mm).cpu().numpy()
        if case == 'nan':
            assert np.isnan(got[:, 5]).all() and np.isnan(ref[:, 5]).all()
            assert not np.isnan(np.delete(got, [2, 5], axis=1)).any()          # (the all-zero channel's cosines are 0 / 0)
        print(case, dtype, got, ref)
        assert _qerr.close(got, ref, 2e-6)
        post = _qerr.host_post(got)
        assert (post[3:, 2] == 1).all() and np.isfinite(post[3:]).all()
        if case == 'nan':
            assert (post[3:, 5] == 1).all()


@pytest.mark.parametrize('dtype', DTYPES, **_DT)
@pytest.mark.parametrize('poison', [float('nan'), float('inf')])
def test_bit_allocation_poisoned_by_nan_or_inf(poison, dtype):
    """Every channel's qmax is NaN: the divide-free quotient must not be taken.  Expected: the restatement's formulas on what
    ops.pc_qdq stores for the same tables in fp32 - which is what q_k is defined to be."""
    L, ops, _ = _mods()
    g = torch.Generator().manual_seed(6)
    N, C, H, W = 4, 8, 14, 14
    x = torch.randn(N, C, H, W, generator=g) * torch.tensor([.5, 1., 3., .1, 2., 1., 5., 1.]).view(1, C, 1, 1)
    x[2, 4, 5, 5] = poison
    xf, xd = _place(x, dtype)
    table, _ = ops.pc_stats_half(xd, need_b=True)
    qps = ops.mix_candidates(table, num_bits=4, positive=False, bit_alloc=True)
    qps = (qps[2], qps[1], qps[0])
    assert bool(torch.isnan(torch.stack(qps)[:, L.QP_QMAX]).all())
    assert bool(torch.isfinite(table[[L.STAT_MIN, L.STAT_MAX]][:, [0, 1, 2, 3, 5, 6, 7]]).all())
    ys = [ops.pc_qdq(xf.cuda(), N, C, H * W, q).cpu() for q in qps]
    ref = _qerr.error_columns(xf, ys, check_no_cancellation=False)
    with _still():
        a = ops.pc_quant_errors_half(xd, qps)
        b = ops.pc_quant_errors_half(xd, qps, mm=table[[L.STAT_MIN, L.STAT_MAX]])
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    print(poison, dtype, a.cpu().numpy(), ref)
    assert _qerr.close(a.cpu().numpy(), ref, 2e-6)


def test_refusals_copy_nothing():
    L, ops, _ = _mods()
    qp = torch.ones(3, 4, device='cuda')
    x = torch.randn(2, 4, 4, 4, device='cuda').to(torch.bfloat16)
    with _still():
        for bad in (x.float(), x.to(memory_format=torch.channels_last), x.cpu(), x[0], x[:, :, ::2], x.permute(0, 1, 3, 2)):
            with pytest.raises(L.CnnqError):
                ops.pc_quant_errors_half(bad, [qp])
        with pytest.raises(L.CnnqError):
            ops.pc_quant_errors_half(x, [qp] * 4)
        with pytest.raises(L.CnnqError):
            ops.pc_quant_errors_half(x, [qp[:, :3]])
        with pytest.raises(L.CnnqError):
            ops.pc_quant_errors_half(x, [qp], mm=torch.zeros(2, 3, device='cuda'))
        assert ops.pc_quant_errors_half(x, [qp]).shape == (2, 4)


def _manager(tmp_path, monkeypatch, name, **kw):
    from cnn_quantization_amd.inference import statistic_manager_perchannel as smpc
    from cnn_quantization_amd.utils.misc import Singleton
    monkeypatch.setenv('HOME', str(tmp_path))
    Singleton._instances.pop(smpc.StatisticManagerPerChannel, None)
    return smpc.StatisticManagerPerChannel(name, **kw)


SET4 = dict(num_bits=4, positive=False, bit_alloc=False, prior_is_b=False, target=4, round_mode=True)
STATS7 = ('max', 'min', 'std', 'mean', 'kurtosis', 'b', 'std_pos')


def test_manager_with_both_flags_records_the_restatements_rows_and_the_parents_picks(tmp_path, monkeypatch):
    _, ops, iq = _mods()
    xf, xd = _place(_qerr.mixed_input(seed=11), torch.bfloat16)
    with _still():
        plain = _manager(tmp_path, monkeypatch, 'plain', load_stats=False)
        assert plain.collect_route(xd) == 'half'
        plain.save_tensor_stats(xd, 'activation', 'conv0_activation')
        sm = _manager(tmp_path, monkeypatch, 'err', load_stats=False, collect_err=True, err_settings=SET4, native_err=True,
                      native_err_half=True)
        assert sm.collect_route(xd) == 'half'
        sm.save_tensor_stats(xd, 'activation', 'conv0_activation')
    rec = sm.stats['conv0_activation']
    for s in STATS7:
        assert np.array_equal(rec[s].view(np.int32), plain.stats['conv0_activation'][s].view(np.int32)), s
    ref, _ = _qerr.mix_columns(xf, {k: rec[k] for k in ('min', 'max', 'mean', 'b', 'std')}, num_bits=4, positive=False, bit_alloc=False)
    want, margin = _qerr.picks(ref)
    print('smallest pick margin %.3g' % margin.min())
    assert margin.min() >= 1e-5                                               # no channel is excluded: every pick is decided
    rows = np.stack([rec[n] for n in _qerr.NAMES])
    print('manager rel %.3g' % _qerr.rel_err(rows, _qerr.host_post(ref)))
    assert _qerr.close(rows, _qerr.host_post(ref), 2e-6)
    # the parent's route: the same manager without the flags answers None, so the tensor is upcast on its way to the fp32 kernels
    for flags in (dict(), dict(native_err=True)):
        old = _manager(tmp_path, monkeypatch, 'old', load_stats=False, collect_err=True, err_settings=SET4, **flags)
        assert old.collect_route(xd) is None
    before = iq.HALF_FALLBACKS
    iq.upcast_fallback(old.save_tensor_stats, xd, 'activation', 'conv0_activation')
    assert iq.HALF_FALLBACKS == before + 1
    old_rows = np.stack([old.stats['conv0_activation'][n] for n in _qerr.NAMES])
    assert np.array_equal(_qerr.picks(rows)[0], _qerr.picks(old_rows)[0]) and np.array_equal(_qerr.picks(rows)[0], want)
    assert set(want.tolist()) == {0, 1, 2}


def test_harness_collect_err_then_mix_in_bf16(tmp_path, monkeypatch):
    """The README's `-c mix` recipe under --dtype bfloat16: no conv output is upcast on its way to the statistics managers or
    through the quantizer (at this size every class of layer is one the route words keep native)."""
    from cnn_quantization_amd.harness import inference_sim as H
    from cnn_quantization_amd.inference import inference_quantization_manager as iqm
    from cnn_quantization_amd.utils.misc import Singleton
    _, ops, iq = _mods()
    monkeypatch.setenv('HOME', str(tmp_path))
    B = 8
    upcast = []

    def counting(real):
        def fallback(fn, *args, **kw):
            # conv outputs: 4-D half tensors of the batch with a spatial extent (no weight of resnet18 has B output channels)
            upcast.extend((getattr(fn, '__name__', str(fn)), tuple(a.shape)) for a in args
                          if isinstance(a, torch.Tensor) and a.dtype in iq.HALF_DTYPES and a.dim() == 4 and a.shape[0] == B
                          and a.shape[2] * a.shape[3] > 1)
            return real(fn, *args, **kw)
        return fallback
    monkeypatch.setattr(iqm, 'upcast_fallback', counting(iqm.upcast_fallback))
    monkeypatch.setattr(iq, 'upcast_fallback', counting(iq.upcast_fallback))
    base = ['-a', 'resnet18', '-b', str(B), '--image-size', '64', '-pcq_a', '-pcq_w', '--qtype', 'int4', '-qw', 'int4', '--dtype', 'bfloat16']
    for argv in (base + ['-sm', 'collect', '-ce'], [a for a in base if a != '-pcq_a'] + ['-sm', 'collect'],
                 base + ['-sm', 'use', '-c', 'mix']):
        Singleton.reset()
        with contextlib.redirect_stdout(io.StringIO()):
            res = H.main(argv)
        assert res['output_finite']
        assert upcast == [], (argv, upcast)
    path = os.path.join(str(tmp_path), 'mxt-sim', 'statistics', 'per_channel', 'resnet18', 'resnet18_statistics_perchannel_summary.pkl')
    with open(path, 'rb') as f:
        summ = pickle.load(f)
    convs = [k for k in summ if k.startswith('conv')]
    assert len(convs) >= 17
    for k in convs:
        assert len(summ[k].columns) == 13 * 3 and np.isfinite(summ[k][['mean_mse_lowp', 'mean_mse_gaus', 'mean_mse_laplace']].values).all()
    Singleton.reset()
