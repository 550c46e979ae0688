"""The flat-row statistics on the GPU, fp32 / bf16 / fp16: ops.tensor_stats (cnnq_rows_stats) on contiguous
tensors, odd views and dense channels_last tensors, and the routes of ops.kld_thresholds and ops.row_sumsq built on it.

The reference is fp64 torch on the CPU over x.float().double() reshaped to [rows, len] (half values are exact in fp32, so the
reference sees the values the kernel sees; B and the kurtosis around the fp32-rounded mean and std, as the reference of
tests/test_channels_last_collect_gpu.py).  The tiers are that file's and tests/test_stats_single_gpu.py's: extrema bit exact with
torch's NaN rule, mean 2e-6 / 1e-7, std 2e-6, b and std_pos 3e-6 / 1e-7, kurtosis 2e-4 / 2e-4 on rows whose std is not 0, the
count exact, and the manager's mean_abs = (2 * sum relu - sum) / count within 3e-6 / 1e-7 of mean |x|.  Inputs, shapes and the
tier check live in tests/test_tensor_stats_cpu.py, which shows on the CPU that an emulation of the kernels' fp32 partial sums keeps
these tiers on these inputs."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

from test_tensor_stats_cpu import DTYPES, EXACT, IDS, LARGEST, SHAPES, check_tiers, ref64, values, widths

pytestmark = pytest.mark.gpu


def mods():
    from cnn_quantization_amd import _lib as L, ops
    return L, ops


def counters():
    _, ops = mods()
    return ops.LAYOUT_COPIES, importlib.import_module('cnn_quantization_amd.qtypes.int_quantizer').HALF_FALLBACKS


def route(x, rows):
    L, ops = mods()
    out = (ctypes.c_int32 * 4)()
    align = (x.data_ptr() | 16) & -(x.data_ptr() | 16)
    assert L.load().cnnq_rows_stats_route(rows, x.numel() // rows, ops._DTYPE_CODES[x.dtype], align, out) == 0
    return list(out)


def run(x, rows=1, need_dev=True):
    """ops.tensor_stats on x as it lies: neither counter moves."""
    _, ops = mods()
    before = counters()
    stats, mom = ops.tensor_stats(x, rows, need_dev)
    assert counters() == before
    assert stats.shape == (7, rows) and stats.dtype == torch.float32 and mom.shape == (7, rows) and mom.dtype == torch.float64
    return stats, mom


def check(x, rows, stats, mom, need_dev=True):
    """The table of x against fp64 on the values in storage order."""
    L, _ = mods()
    flat = x.detach().permute(0, 2, 3, 1) if (x.dim() == 4 and not x.is_contiguous()) else x
    t = flat.float().cpu().reshape(rows, -1)
    ref, mean_abs = ref64(t)
    m = mom.cpu()
    check_tiers(stats.cpu(), m[L.MOM_COUNT], m[L.MOM_SUM], m[L.MOM_SUM_RELU], ref, mean_abs, t.shape[1], need_dev)


def same(a, b):
    """Bitwise equality, every NaN equal to every NaN."""
    assert a.dtype == b.dtype and a.shape == b.shape
    iv = {torch.float32: torch.int32, torch.float64: torch.int64}[a.dtype]
    na, nb = torch.isnan(a), torch.isnan(b)
    return torch.equal(na, nb) and torch.equal(a.contiguous().view(iv)[~na], b.contiguous().view(iv)[~nb])


# ---- 1. the shapes: every width, both regimes, the ends of the lane walk, chunks, many rows
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_shapes_keep_the_tiers_on_the_route_they_were_chosen_for(dtype):
    esize = 4 if dtype == torch.float32 else 2
    for rows, length in SHAPES:
        x = values(rows, length).to(dtype).cuda()
        w, S, ppc, exact = route(x, rows)
        assert w == widths(length, esize)[0] and exact == (length <= EXACT), (rows, length, w, exact)
        if (rows, length) == (1, 3 * 65536 + 40):
            assert S == 3 and (length // w) % ppc != 0                     # several chunks, the last one uneven
        if (rows, length) == (3, 140001):
            assert (w, S) == (1, 2)                                        # chunks inside the rows
        stats, mom = run(x, rows)
        print(rows, length, 'W', w, 'S', S)
        check(x, rows, stats, mom)
    # the widths below 16 bytes on the fp32 regime too: 8 bytes (len % 4 == 2 elements of fp32, % 8 == 4 of half), 4 bytes
    for length, want in ((8194, 2), (8196, 4), (8198, 2)):
        x = values(1, length).to(dtype).cuda()
        assert route(x, 1)[0] == want == widths(length, esize)[0]
        check(x, 1, *run(x, 1))


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_view_at_an_odd_element_offset(dtype):
    for length in (8193, 70002):
        base = values(1, length + 1).to(dtype).cuda().reshape(-1)
        x = base[1:]
        assert x.data_ptr() % 16 == x.element_size() and x.is_contiguous()
        w, S, ppc, exact = route(x, 1)
        assert (w, exact) == (1, 0)                                            # one element per load: correct, not fast
        check(x.reshape(1, -1), 1, *run(x, 1))
    # the rows of a [2, len] view stay on their element alignment only
    base = values(1, 2 * 9001 + 1).to(dtype).cuda().reshape(-1)
    x = base[1:].reshape(2, 9001)
    assert route(x, 2)[0] == 1
    check(x, 2, *run(x, 2))


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_dense_channels_last_as_it_lies(dtype):
    _, ops = mods()
    n, c, h, w = 4, 24, 9, 9
    vals = values(n, c * h * w).to(dtype).cuda()                           # sample i = row i of the storage
    x = vals.reshape(n, h, w, c).permute(0, 3, 1, 2)
    assert ops._layout(x) == 'nhwc'
    xc = x.contiguous()
    for rows in (1, n):
        stats, mom = run(x, rows)
        check(x, rows, stats, mom)
        sc, mc = run(xc, rows)
        check(xc, rows, sc, mc)
        # the same elements in another order: the extrema and the count are the same bits
        assert same(stats[:2], sc[:2]) and same(mom[[0, 1, 4]], mc[[0, 1, 4]])
        rest = [2, 3, 4, 6]                                                # mean, std, b, std_pos: two summation orders
        np.testing.assert_allclose(stats[rest].cpu().double(), sc[rest].cpu().double(), rtol=2e-6, atol=1e-7)
        np.testing.assert_allclose(stats[5].cpu().double(), sc[5].cpu().double(), rtol=2e-5, atol=2e-5)
    # rows that are neither 1 nor N do not fit the channels_last storage: the counted copy
    copies = ops.LAYOUT_COPIES
    stats, _ = ops.tensor_stats(x, 2)
    assert ops.LAYOUT_COPIES == copies + 1
    assert same(stats, run(xc, 2)[0])


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_largest_tensor_takes_the_most_chunks(dtype):
    rows, length = LARGEST
    x = values(rows, length).to(dtype).cuda()
    w, S, ppc, exact = route(x, rows)
    assert (w, S, exact) == (16 // x.element_size(), 128, 0)
    stats, mom = run(x, rows)
    check(x, rows, stats, mom)
    # two runs give the same bits
    s2, m2 = run(x, rows)
    assert same(stats, s2) and same(mom, m2)
    # no hidden copy: with the workspace warm a call allocates its two small tables only
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.max_memory_allocated()
    run(x, rows)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base < x.numel() * x.element_size() // 2


# ---- 2. determinism, need_dev
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_two_runs_same_bits_and_need_dev_off(dtype):
    L, _ = mods()
    for rows, length in ((1, 3 * 65536 + 40), (5, 70001), (3, 4096), (300, 50)):
        x = values(rows, length).to(dtype).cuda()
        stats, mom = run(x, rows)
        s2, m2 = run(x, rows)
        assert same(stats, s2) and same(mom, m2)
        s0, m0 = run(x, rows, need_dev=False)
        assert not s0[L.STAT_B].any() and not s0[L.STAT_KURT].any()
        keep = [L.STAT_MIN, L.STAT_MAX, L.STAT_MEAN, L.STAT_STD, L.STAT_STD_POS]
        assert same(s0[keep], stats[keep]) and same(m0, mom)
        check(x, rows, s0, m0, need_dev=False)


# ---- 3. against the existing route: ops.pc_stats on the upcast contiguous tensor, rows as channels
def old_route(x, rows):
    _, ops = mods()
    xf = x.float().contiguous()
    return ops.pc_stats(xf, 1, rows, xf.numel() // rows, need_b=True, need_kurt=True, need_relu=True, local_only=True)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_agrees_with_the_per_channel_chain_on_one_channel(dtype):
    L, _ = mods()
    for rows, length in ((1, 3 * 65536 + 24), (5, 70001), (3, 4100), (300, 50), (1, 8)):
        x = values(rows, length).to(dtype).cuda()
        stats, mom = run(x, rows)
        so, mo = old_route(x, rows)
        # two summation orders of the same values (the tier of DESIGN.md section 18): 2e-6, kurtosis 2e-5
        assert same(stats[:2], so[:2]) and same(mom[L.MOM_COUNT], mo[L.MOM_COUNT])
        rest = [L.STAT_MEAN, L.STAT_STD, L.STAT_B, L.STAT_STD_POS]
        np.testing.assert_allclose(stats[rest].cpu().double(), so[rest].cpu().double(), rtol=2e-6, atol=1e-7)
        np.testing.assert_allclose(stats[L.STAT_KURT].cpu().double(), so[L.STAT_KURT].cpu().double(), rtol=2e-5, atol=2e-5)
        np.testing.assert_allclose(mom[[3, 6]].cpu(), mo[[3, 6]].cpu(), rtol=2e-6)     # the sums of squares


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('specials', [('nan',), ('inf',), ('inf', '-inf'), ('nan', 'inf', '-inf')], ids=lambda s: '+'.join(s))
def test_nan_and_inf_pattern_is_the_chains(dtype, specials):
    for rows, length, where in ((1, 3 * 65536 + 24, 70000), (1, 4000, 17), (5, 70001, 2 * 70001 + 69000)):
        x = values(rows, length).to(dtype).reshape(-1)
        for k, s in enumerate(specials):
            x[where + 3 * k] = float(s)
        x = x.reshape(rows, length).cuda()
        stats, mom = run(x, rows)
        so, mo = old_route(x, rows)
        for a, b in ((stats, so), (mom, mo)):
            assert torch.equal(torch.isnan(a), torch.isnan(b)), (specials, rows, length, a, b)
            assert torch.equal(torch.isposinf(a), torch.isposinf(b)) and torch.equal(torch.isneginf(a), torch.isneginf(b)), (specials, rows, a, b)
        if rows > 1:
            # the special values sit in row 2: every other row keeps the bits of the clean tensor
            clean = values(rows, length).to(dtype).cuda()
            sc, mc = run(clean, rows)
            others = [r for r in range(rows) if r != 2]
            assert same(stats[:, others], sc[:, others]) and same(mom[:, others], mc[:, others])
            assert not same(stats[:, 2], sc[:, 2])


# ---- 4. the ops routes built on it
def test_kld_thresholds_reads_channels_last_float32_as_it_lies():
    L, ops = mods()
    n, c, h, w = 4, 24, 9, 9
    x = values(n, c * h * w).cuda().reshape(n, h, w, c).permute(0, 3, 1, 2)
    assert ops._layout(x) == 'nhwc'
    for rows in (n, 1):
        before = counters()
        out, hist, div = ops.kld_thresholds(x, rows, want_parts=True)
        assert counters() == before
        oc, hc, dc = ops.kld_thresholds(x.contiguous(), rows, want_parts=True)
        assert same(out, oc) and torch.equal(hist, hc) and same(div, dc)
    with pytest.raises(L.CnnqError):
        ops.kld_thresholds(x.to(torch.bfloat16), n)                            # no half histogram
    copies = ops.LAYOUT_COPIES
    ops.kld_thresholds(x, 2)                                                   # rows that do not fit the storage: the counted copy
    assert ops.LAYOUT_COPIES == copies + 1


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_row_sumsq_half_and_channels_last(dtype):
    _, ops = mods()
    n, c, h, w = 4, 24, 9, 9
    vals = values(n, c * h * w).to(dtype).cuda()
    x = vals.reshape(n, h, w, c).permute(0, 3, 1, 2)
    want = (vals.cpu().double() ** 2).sum(1)
    before = counters()
    got = ops.row_sumsq(x, n)
    assert counters() == before and got.dtype == torch.float32 and got.shape == (n,)
    np.testing.assert_allclose(got.cpu().double(), want, rtol=2e-6)
    # a contiguous tensor: half takes the flat rows, float32 the code it took - the same sums
    flat = ops.row_sumsq(vals, n)
    assert counters() == before
    np.testing.assert_allclose(flat.cpu().double(), want, rtol=2e-6)
    if dtype == torch.float32:
        calls = []
        real = ops.pc_stats
        try:
            ops.pc_stats = lambda *a, **kw: calls.append(a[1:4]) or real(*a, **kw)
            ops.row_sumsq(vals, n)
        finally:
            ops.pc_stats = real
        assert calls == [(1, n, c * h * w)]


def test_refuses_what_it_cannot_view():
    L, ops = mods()
    x = torch.zeros(10, 7, device='cuda')
    stats, mom = ops.tensor_stats(x, 10)                                       # what it can: ten rows of seven zeros
    assert not stats[:4].any() and bool((mom[L.MOM_COUNT] == 7).all())         # (a constant row's kurtosis is 0 / 0)
    for rows in (0, 3, -1):
        with pytest.raises(L.CnnqError):
            ops.tensor_stats(x, rows)
    with pytest.raises(L.CnnqError):
        ops.tensor_stats(torch.zeros(0, 4, device='cuda'))
    with pytest.raises(L.CnnqError):
        ops.tensor_stats(x.double())
