"""`-sm collect` on dense channels_last activations, fp32 / bf16 / fp16: ops.pc_stats_nhwc and the
per-channel statistics manager on top of it.

The reference is fp64 torch on the CPU over x.contiguous().float().double() (half values are exact in fp32, so one reference
serves the three dtypes; B and the kurtosis around the fp32-rounded mean and std, as the NCHW single launch's reference in
tests/test_stats_single_gpu.py).  The tiers are that file's (lines 132-141): extrema bit exact with torch's NaN rule, mean
2e-6 / 1e-7, std 2e-6, b and std_pos 3e-6 / 1e-7, kurtosis 2e-4 / 2e-4 on channels whose std is not 0 (a constant channel's
kurtosis is 0 / 0 and outside the contract).  tests/test_channels_last_collect_cpu.py shows on the CPU that an fp32
evaluation of the same formulas keeps these tiers on the inputs used here.

B is written whenever pass B runs - need_b or need_kurt - as cnnq_pc_stats writes it; every other row nobody asked for is zero."""
import ctypes
import glob
import importlib
import os
import pickle

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
IDS = ['f32', 'bf16', 'f16']
# (C, storage offset in elements) -> W for fp32, W for bf16 / fp16: the pairs of tests/test_channels_last_aciq_gpu.py
WIDTH_CASES = [(6, 0, 2, 2), (10, 0, 2, 2), (12, 0, 4, 4), (20, 0, 4, 4), (64, 2, 2, 2), (64, 4, 4, 4), (64, 0, 4, 8), (7, 0, 1, 1)]
ALL = (True, True, True)


def mods():
    from cnn_quantization_amd import _lib as L, ops
    return L, ops


def iq_mod():
    return importlib.import_module('cnn_quantization_amd.qtypes.int_quantizer')


def same(a, b):
    """Bitwise equality in NCHW order, every NaN equal to every NaN."""
    a, b = a.contiguous(), b.contiguous()
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    na, nb = torch.isnan(a), torch.isnan(b)
    if not torch.equal(na, nb):
        return False
    iv = {torch.float32: torch.int32, torch.float64: torch.int64}.get(a.dtype, torch.int16)
    return torch.equal(a.view(iv)[~na], b.view(iv)[~nb])


def values(shape, seed=0, positive=False):
    """Per-channel Laplace-like activations with a moderate mean (the generator of tests/test_channels_last_gpu.py)."""
    g = torch.Generator().manual_seed(seed)
    C = shape[1]
    x = torch.randn(shape, generator=g) * (0.2 + 3 * torch.rand(1, C, 1, 1, generator=g)) + torch.randn(1, C, 1, 1, generator=g)
    return x.relu() if positive else x


def cl(x, dtype, offset=0):
    """x as a dense channels_last tensor of dtype on the GPU, `offset` elements into its storage."""
    _, ops = mods()
    n, c, h, w = x.shape
    base = torch.zeros(x.numel() + offset + 8, dtype=dtype, device='cuda')
    v = base.as_strided(x.shape, (h * w * c, 1, w * c, c), offset)
    v.copy_(x.to(dtype).cuda())
    assert ops._layout(v) == 'nhwc' and v.storage_offset() == offset
    return v


def ref64(x):
    """The seven rows in fp64 on the CPU, [NSTAT, C]; min / max with torch's NaN rule."""
    L, _ = mods()
    xf = x.contiguous().float().cpu()
    C = xf.shape[1]
    t = xf.double().transpose(0, 1).reshape(C, -1)
    mean, std = t.mean(1), t.std(1, unbiased=True)
    out = torch.zeros(L.NSTAT, C, dtype=torch.float64)
    nan = torch.isnan(t).any(1)
    nanv = torch.full((C,), float('nan'), dtype=torch.float64)
    out[L.STAT_MIN] = torch.where(nan, nanv, t.min(1)[0])
    out[L.STAT_MAX] = torch.where(nan, nanv, t.max(1)[0])
    out[L.STAT_MEAN], out[L.STAT_STD] = mean, std
    m32, s32 = mean.float().double(), std.float().double()
    out[L.STAT_B] = (t - m32[:, None]).abs().mean(1)
    out[L.STAT_KURT] = (((t - m32[:, None]) / s32[:, None]) ** 4).mean(1) - 3
    out[L.STAT_STD_POS] = t.clamp(min=0).std(1, unbiased=True)
    return out


def check_tiers(st, ref, need=ALL, chans=None):
    """The table st against ref64's rows on the channels `chans` (default: all)."""
    L, _ = mods()
    need_b, need_kurt, need_relu = need
    st = st.cpu()
    idx = torch.arange(st.shape[1]) if chans is None else torch.as_tensor(chans)
    s, r = st[:, idx], ref[:, idx]
    figures = {n: float(((s[row].double() - r[row]).abs() / r[row].abs().clamp(min=1e-30)).max())
               for n, row in (('mean', L.STAT_MEAN), ('std', L.STAT_STD), ('b', L.STAT_B), ('std_pos', L.STAT_STD_POS))}
    print('max relative error per row', figures)
    assert same(s[L.STAT_MIN], r[L.STAT_MIN].float()) and same(s[L.STAT_MAX], r[L.STAT_MAX].float())
    np.testing.assert_allclose(s[L.STAT_MEAN].double(), r[L.STAT_MEAN], rtol=2e-6, atol=1e-7)
    live = r[L.STAT_STD] != 0
    np.testing.assert_allclose(s[L.STAT_STD].double()[live], r[L.STAT_STD][live], rtol=2e-6)
    if need_b or need_kurt:
        np.testing.assert_allclose(s[L.STAT_B].double(), r[L.STAT_B], rtol=3e-6, atol=1e-7)
    else:
        assert not s[L.STAT_B].any()
    if need_kurt:
        np.testing.assert_allclose(s[L.STAT_KURT].double()[live], r[L.STAT_KURT][live], rtol=2e-4, atol=2e-4)
    else:
        assert not s[L.STAT_KURT].any()
    if need_relu:
        np.testing.assert_allclose(s[L.STAT_STD_POS].double(), r[L.STAT_STD_POS], rtol=3e-6, atol=1e-7)
    else:
        assert not s[L.STAT_STD_POS].any()


def counters():
    _, ops = mods()
    return ops.LAYOUT_COPIES, iq_mod().HALF_FALLBACKS


def route(x):
    L, ops = mods()
    out = (ctypes.c_int32 * 4)()
    C = x.shape[1]
    align = (x.data_ptr() | 16) & -(x.data_ptr() | 16)
    assert L.load().cnnq_pc_route_stats_nhwc(x.numel() // C, C, ops._DTYPE_CODES[x.dtype], align, out) == 0
    return list(out)


# ---- 1. every piece width on both summation regimes
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('case', WIDTH_CASES, ids=lambda c: 'C%d+%d' % c[:2])
def test_every_piece_width_on_both_summation_regimes(case, dtype):
    L, ops = mods()
    C, offset, w32, w16 = case
    want = w32 if dtype == torch.float32 else w16
    # R = 6272 and 9408 take the four-row fp32 partial sums, R = 588 and 98 the fp64 sums (4096 rows is the border)
    for shape in ((8, C, 28, 28), (3, C, 56, 56), (3, C, 14, 14), (2, C, 7, 7)):
        x = cl(values(shape, seed=C + offset + shape[2]), dtype, offset)
        R = x.numel() // C
        rt = route(x)
        assert rt[0] == want and rt[3] == 1, (shape, dtype, offset, rt, want)
        before = counters()
        st, mom = ops.pc_stats_nhwc(x, *ALL)
        assert counters() == before
        assert st.shape == (L.NSTAT, C) and st.dtype == torch.float32 and mom.shape == (L.NMOM, C) and mom.dtype == torch.float64
        check_tiers(st, ref64(x))
        assert torch.equal(mom[L.MOM_COUNT].cpu(), torch.full((C,), float(R), dtype=torch.float64))
        t = x.contiguous().double().transpose(0, 1).reshape(C, -1)
        np.testing.assert_allclose(mom[L.MOM_SUM].cpu(), t.sum(1).cpu(), rtol=1e-7, atol=1e-3)
        np.testing.assert_allclose(mom[L.MOM_SUMSQ_RELU].cpu(), (t.clamp(min=0) ** 2).sum(1).cpu(), rtol=1e-7, atol=1e-6)


# ---- 2. flag subsets
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('shape', [(3, 10, 14, 14), (8, 12, 28, 28)], ids=lambda s: 'x'.join(map(str, s)))
def test_flag_subsets(shape, dtype):
    L, ops = mods()
    x = cl(values(shape, seed=17), dtype)
    full, mom_full = ops.pc_stats_nhwc(x, *ALL)
    ref = ref64(x)
    for bits in range(8):
        need = (bool(bits & 1), bool(bits & 2), bool(bits & 4))
        st, mom = ops.pc_stats_nhwc(x, *need)
        check_tiers(st, ref, need)
        rows = [L.STAT_MIN, L.STAT_MAX, L.STAT_MEAN, L.STAT_STD]
        rows += [L.STAT_B] if need[0] or need[1] else []
        rows += [L.STAT_KURT] if need[1] else []
        rows += [L.STAT_STD_POS] if need[2] else []
        assert same(st[rows], full[rows]), need
        for r in range(L.NSTAT):
            assert r in rows or not st[r].any(), (need, r)
        mrows = [L.MOM_MIN, L.MOM_MAX, L.MOM_SUM, L.MOM_SUMSQ, L.MOM_COUNT] + ([L.MOM_SUM_RELU, L.MOM_SUMSQ_RELU] if need[2] else [])
        assert same(mom[mrows], mom_full[mrows]), need
    _, parts = ops.aciq_qdq_nhwc(x, 4, clip='gaus', want_parts=True)
    assert same(ops.pc_stats_nhwc(x)[0], parts['stats'])


# ---- 3. against the NCHW route
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_against_the_nchw_route(dtype):
    L, ops = mods()
    for shape, offset in (((8, 12, 28, 28), 0), ((3, 10, 14, 14), 1), ((2, 64, 7, 7), 0), ((3, 6, 56, 56), 2)):
        N, C, H, W = shape
        x = cl(values(shape, seed=23 + C), dtype, offset)
        st, _ = ops.pc_stats_nhwc(x, *ALL)
        st0, _ = ops.pc_stats(x.contiguous().float(), N, C, H * W, need_b=True, need_kurt=True, need_relu=True)
        st, st0 = st.cpu(), st0.cpu()
        assert same(st[[L.STAT_MIN, L.STAT_MAX]], st0[[L.STAT_MIN, L.STAT_MAX]])
        rows = [r for r in range(L.NSTAT) if r != L.STAT_KURT]
        np.testing.assert_allclose(st[rows], st0[rows], rtol=2e-6, atol=2e-6)
        np.testing.assert_allclose(st[L.STAT_KURT], st0[L.STAT_KURT], rtol=2e-5, atol=2e-5)


# ---- 4. special values
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_special_values(dtype):
    L, ops = mods()
    x = values((2, 7, 7, 7), seed=9)
    x[1, 0, 2, 3] = float('nan')
    x[0, 1, 0, 0] = float('inf')
    x[1, 2, 1, 1] = float('-inf')
    x[:, 3] = 0.25                                          # constant: std 0, kurtosis 0 / 0
    x[:, 4] = -x[:, 4].abs() - 0.125                        # all negative: std_pos from zero rectified sums
    finite = [3, 4, 5, 6]
    xc = cl(x, dtype, 1)
    st, mom = ops.pc_stats_nhwc(xc, *ALL)
    st0, _ = ops.pc_stats(xc.contiguous().float(), 2, 7, 49, need_b=True, need_kurt=True, need_relu=True)
    st, st0 = st.cpu(), st0.cpu()
    for row in range(L.NSTAT):
        skip = [3] if row == L.STAT_KURT else []           # (the constant channel's kurtosis is outside the contract)
        keep = [c for c in range(7) if c not in skip]
        assert torch.equal(torch.isnan(st[row][keep]), torch.isnan(st0[row][keep])), row
        assert torch.equal(torch.isinf(st[row][keep]), torch.isinf(st0[row][keep])), row
    assert torch.isnan(st[[L.STAT_MIN, L.STAT_MAX, L.STAT_MEAN], 0]).all()
    assert st[L.STAT_MAX, 1] == float('inf') and st[L.STAT_MIN, 2] == float('-inf')
    assert st[L.STAT_STD_POS, 4] == 0 and st[L.STAT_STD, 3] == 0
    assert torch.equal(mom[L.MOM_COUNT].cpu(), torch.full((7,), 98., dtype=torch.float64))
    check_tiers(st, ref64(xc), chans=finite)


# ---- 5. determinism, graph capture, A/B switch, refusals
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_two_runs_give_the_same_bits(dtype):
    _, ops = mods()
    for shape, offset in (((8, 64, 28, 28), 0), ((3, 5, 14, 14), 1), ((4, 520, 7, 7), 0)):
        x = cl(values(shape, seed=21), dtype, offset)
        st1, mom1 = ops.pc_stats_nhwc(x, *ALL)
        st1, mom1 = st1.clone(), mom1.clone()
        ops.aciq_qdq_nhwc(x, 4)                             # (another user of the device in between)
        st2, mom2 = ops.pc_stats_nhwc(x, *ALL)
        assert same(st1, st2) and same(mom1, mom2)


def test_graph_capture_replays_eager():
    _, ops = mods()
    x = cl(values((8, 64, 14, 14), seed=2), torch.bfloat16)
    eager = ops.pc_stats_nhwc(x, *ALL)[0].clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.pc_stats_nhwc(x, *ALL)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st, mom = ops.pc_stats_nhwc(x, *ALL)
    graph.replay()
    torch.cuda.synchronize()
    assert same(st, eager)
    x.copy_(cl(values((8, 64, 14, 14), seed=3), torch.bfloat16))
    graph.replay()
    torch.cuda.synchronize()
    assert not same(st, eager) and same(st, ops.pc_stats_nhwc(x, *ALL)[0])


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_ab_switch_and_non_dense_tensors_take_the_copy(monkeypatch, dtype):
    L, ops = mods()
    x = cl(values((4, 12, 14, 14), seed=4), dtype)
    native = ops.pc_stats_nhwc(x, *ALL)[0]
    monkeypatch.setenv('CNNQ_NHWC', '0')
    ops.reload_switches()
    try:
        before = counters()
        if dtype == torch.float32:
            st = ops.pc_stats_nhwc(x, *ALL)[0]
            assert counters() == (before[0] + 1, before[1])
            assert same(st, ops.pc_stats(x.contiguous(), 4, 12, 196, need_b=True, need_kurt=True, need_relu=True)[0])
        else:
            with pytest.raises(L.CnnqError):
                ops.pc_stats_nhwc(x, *ALL)
            assert counters() == before                     # raised before anything was copied
    finally:
        monkeypatch.delenv('CNNQ_NHWC')
        ops.reload_switches()
    assert same(ops.pc_stats_nhwc(x, *ALL)[0], native)
    # a tensor that is not dense: the copy route (float32 only), and an NCHW tensor as it is
    part = x[:, 2:9]
    assert ops._layout(part) == 'copy'
    before = counters()
    if dtype == torch.float32:
        st = ops.pc_stats_nhwc(part, *ALL)[0]
        assert same(st, ops.pc_stats(part.contiguous(), 4, 7, 196, need_b=True, need_kurt=True, need_relu=True)[0])
        assert same(ops.pc_stats_nhwc(x.contiguous(), *ALL)[0], ops.pc_stats(x.contiguous(), 4, 12, 196, True, True, True)[0])
    else:
        with pytest.raises(L.CnnqError):
            ops.pc_stats_nhwc(part, *ALL)
    assert counters() == before                             # (only copies of dense channels_last tensors are counted)


def test_refusals():
    L, ops = mods()
    with pytest.raises(L.CnnqError):
        ops.pc_stats_nhwc(values((2, 4, 7, 7)))                                              # a CPU tensor
    with pytest.raises(L.CnnqError):
        ops.pc_stats_nhwc(torch.zeros(8, 16, device='cuda'))                                 # not 4-D
    with pytest.raises(L.CnnqError):
        ops.pc_stats_nhwc(cl(values((2, 4, 7, 7)), torch.float32).double())                  # no such kernels
    x = cl(values((2, 4, 7, 7)), torch.float32)
    p, lib = x.data_ptr(), L.load()
    ws = torch.empty(lib.cnnq_pc_stats_nhwc_workspace(98, 4, 0) + 8, dtype=torch.uint8, device='cuda')
    st = torch.empty(L.NSTAT, 4, device='cuda')
    assert lib.cnnq_pc_stats_nhwc(p, 0, 98, 4, 1, 1, 1, ws.data_ptr() + 4, None, st.data_ptr(), None) == -1      # CNNQ_EINVAL
    assert lib.cnnq_pc_stats_nhwc(p, 0, 98, 4, 1, 1, 1, ws.data_ptr(), None, st.data_ptr(), None) == 0      # mom may be NULL
    torch.cuda.synchronize()
    assert same(st, ops.pc_stats_nhwc(x, *ALL)[0])


# ---- 6. the reference's own numbers
def test_reference_collection_vectors(golden):
    """The inputs of tests/golden/collect.npz (the reference's statistic_manager_perchannel.py run on [4,6,5,7] batches) as
    channels_last tensors against the reference's rows, at the tier tests/test_hip_parity.py::test_stats_collect_set_vs_oracle
    holds the NCHW route to.  Set b1 was collected with batch_avg: its extrema are per-sample means, which this route leaves to
    the NCHW code - its other rows are the whole batch's."""
    L, ops = mods()
    g = golden('collect')
    for bi in (0, 1):
        for k in range(3):
            x = g.t('b%d_x%d' % (bi, k))
            st, mom = ops.pc_stats_nhwc(cl(x, torch.float32), *ALL)
            st = st.cpu().numpy()
            if bi == 0:
                assert np.array_equal(st[L.STAT_MIN], g.np('b0_min')[k]) and np.array_equal(st[L.STAT_MAX], g.np('b0_max')[k])
            for row, name, tol in ((L.STAT_MEAN, 'mean', 5e-6), (L.STAT_STD, 'std', 5e-6), (L.STAT_B, 'b', 5e-6),
                                   (L.STAT_STD_POS, 'std_pos', 5e-6)):
                np.testing.assert_allclose(st[row], g.np('b%d_%s' % (bi, name))[k], rtol=tol, atol=2e-6, err_msg=name)
            np.testing.assert_allclose(st[L.STAT_KURT], g.np('b%d_kurtosis' % bi)[k], rtol=1e-3, atol=5e-4, err_msg='kurtosis')
            assert torch.equal(mom[L.MOM_COUNT].cpu(), torch.full((6,), 140., dtype=torch.float64))


# ---- 7. through the manager
STATS = ['max', 'min', 'std', 'mean', 'kurtosis', 'b', 'std_pos']


def manager(name, **kw):
    from cnn_quantization_amd.inference import statistic_manager_perchannel as smpc
    smpc.Singleton._instances.pop(smpc.StatisticManagerPerChannel, None)
    return smpc.StatisticManagerPerChannel(name, load_stats=False, stats=STATS, **kw)


def summary(tmp_path, name):
    files = glob.glob(os.path.join(str(tmp_path), 'mxt-sim', 'statistics', 'per_channel', name, '*_summary.pkl'))
    assert len(files) == 1, files
    with open(files[0], 'rb') as f:
        return pickle.load(f)


def test_through_the_manager(tmp_path, monkeypatch):
    L, ops = mods()
    from cnn_quantization_amd.inference import statistic_manager_perchannel as smpc
    monkeypatch.setenv('HOME', str(tmp_path))
    calls = {'nhwc': 0, 'nchw': 0}
    nhwc, nchw = ops.pc_stats_nhwc, ops.pc_stats

    def spy_nhwc(*a, **kw):
        calls['nhwc'] += 1
        return nhwc(*a, **kw)

    def spy_nchw(*a, **kw):
        calls['nchw'] += 1
        return nchw(*a, **kw)
    monkeypatch.setattr(ops, 'pc_stats_nhwc', spy_nhwc)
    monkeypatch.setattr(ops, 'pc_stats', spy_nchw)
    batches = [cl(values((4, 12, 14, 14), seed=30 + k), torch.bfloat16) for k in range(2)]
    try:
        before = counters()
        sm = manager('native')
        for x in batches:
            assert smpc.collects_native_nhwc(sm, x)
            sm.save_tensor_stats(x, 'activation', 'conv0_activation')
        assert calls == {'nhwc': 2, 'nchw': 0} and counters() == before
        sm.__exit__()
        sm = manager('copied')
        for x in batches:
            sm.save_tensor_stats(x.contiguous().float(), 'activation', 'conv0_activation')
        assert calls == {'nhwc': 2, 'nchw': 2}
        sm.__exit__()
        a, b = summary(tmp_path, 'native')['conv0_activation'], summary(tmp_path, 'copied')['conv0_activation']
        assert list(a.columns) == list(b.columns) and list(a.dtypes) == list(b.dtypes) and a.shape == b.shape == (12, 21)
        for col in a.columns:
            kurt = col.endswith('kurtosis')
            if col.endswith('_max') or col.endswith('_min'):
                assert np.array_equal(a[col].values, b[col].values), col
            else:
                np.testing.assert_allclose(a[col].values, b[col].values, rtol=2e-5 if kurt else 2e-6, atol=2e-5 if kurt else 2e-6,
                                           err_msg=col)
        # against fp64, batch by batch: the rows the manager holds
        sm = manager('rows')
        for x in batches:
            sm.save_tensor_stats(x, 'activation', 'conv0_activation')
        for k, x in enumerate(batches):
            table = torch.stack([torch.from_numpy(sm.stats['conv0_activation'][n][k])
                                 for n in ('min', 'max', 'mean', 'std', 'b', 'kurtosis', 'std_pos')])
            order = [L.STAT_MIN, L.STAT_MAX, L.STAT_MEAN, L.STAT_STD, L.STAT_B, L.STAT_KURT, L.STAT_STD_POS]
            st = torch.zeros(L.NSTAT, 12)
            st[order] = table
            check_tiers(st, ref64(x))
        # batch_avg (the per-sample extrema) and collect_err (the error columns) keep today's route
        calls.update(nhwc=0, nchw=0)
        for kw in (dict(batch_avg=True), dict(collect_err=True, err_settings=dict(num_bits=4, positive=False, bit_alloc=False,
                                                                                 prior_is_b=False, target=None, round_mode=True))):
            sm = manager('other', **kw)
            assert not smpc.collects_native_nhwc(sm, batches[0])
            iq_mod().upcast_fallback(sm.save_tensor_stats, batches[0], 'activation', 'conv0_activation')      # as _route hands it over
            assert calls['nhwc'] == 0 and calls['nchw'] >= 1, (kw, calls)
            calls.update(nhwc=0, nchw=0)
        # ... unless the caller forces the extrema of the whole batch
        sm = manager('forced', batch_avg=True)
        sm.save_tensor_stats(batches[0], 'activation', 'conv0_activation', force_global_min_max=True)
        assert calls == {'nhwc': 1, 'nchw': 0}
    finally:
        smpc.Singleton._instances.pop(smpc.StatisticManagerPerChannel, None)
