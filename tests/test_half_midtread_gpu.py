"""Config 5 (mid-tread quantization with per-channel bin allocation, and the entropy of its codes) on contiguous bf16 / fp16
activations: ops.mid_tread_qdq_half on cnnq_pc_midtread_dt and cnnq_pc_midtread_qdq_dt.

The contract, on both routes (the chain, single_launch = 0; the resident form, single_launch = 2, where the channel fits) and in
both dtypes:
  1. the table: rows MIN / MAX of `stats` bit exact against x.float() with torch's NaN rule, MEAN / STD / B within the statistics
     tiers of fp64 (check_tiers and ref64 of tests/test_channels_last_collect_gpu.py: mean 2e-6 / 1e-7, std 2e-6, b 3e-6 / 1e-7), KURT
     and STD_POS zero;
  2. given the published table, bit for bit: rows OMEGA / ALPHA / DELTA / CMIN / CMAX of mt equal cnnq_pc_midtread_params on it (the
     chain: WSTART too; the resident form: WSTART an integer >= -MT_HIST_BINS / 2, the same in every channel); y equals the NCHW
     kernel (cnnq_pc_midtread_qdq on x.float() with the published mt) cast to x's dtype; and against that kernel's histogram the
     first MT_HIST_BINS + 2 + 2 * C words are equal word for word, the window bins summed over the replica tables are equal, the
     flag word is raised in both or in neither, the entropy equals cnnq_midtread_entropy on the NCHW histogram bit for bit, and
     every element was counted once.

The shapes (tests/_half_aciq.py: CASES) are the smallest that reach each branch, and every test asserts the plan through
cnnq_pc_route_midtread_dt, so a changed plan cannot silently stop covering a branch."""
import ctypes
import importlib

import pytest
import torch

import _half_collect as HC
import _half_midtread as HM
from test_channels_last_collect_gpu import check_tiers, ref64, same
from test_channels_last_midtread_gpu import REGIMES, entropy_of, laplace_like, mt_of, nchw_kernel, same_scalar
from test_half_collect_gpu import half

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]
IDS = ['bf16', 'f16']
TARGET = 5.3


def mods():
    from cnn_quantization_amd import _lib as L, ops
    return L, ops


def counters():
    _, ops = mods()
    return ops.LAYOUT_COPIES, importlib.import_module('cnn_quantization_amd.qtypes.int_quantizer').HALF_FALLBACKS


def run(x, target, sym, **kw):
    _, ops = mods()
    return ops.mid_tread_qdq_half(x, target, sym, **kw)


def route(x, hist, allow, y=None):
    L, ops = mods()
    out = (ctypes.c_int32 * 4)()
    N, C, HW = ops.geometry(x)
    p = x.data_ptr() | (y.data_ptr() if y is not None else 0) | 16
    assert L.load().cnnq_pc_route_midtread_dt(N, C, HW, ops._DTYPE_CODES[x.dtype], p & -p, int(hist), allow, out) == 0
    return tuple(out)


_INPUTS = {}


def case_input(case, dtype):
    """The case's tensor and its fp64 reference, made once per (case, dtype) and left unchanged."""
    key = (case[0], case[1], dtype)
    if key not in _INPUTS:
        shape, offset, _ = case
        x = half(HC.values(shape, HC.seed_of(shape, offset)), dtype, offset)
        _INPUTS[key] = (x, ref64(x))
    return _INPUTS[key]


def check_given_table(x, y, ent, parts, target, sym, resident):
    """Point 2 of the contract: everything behind the published table, bit for bit."""
    L, _ = mods()
    C = x.shape[1]
    mt, hist = parts['mt'], parts['hist']
    assert mt.shape == (L.NMT, C)
    mt0 = mt_of(parts['stats'], target, sym)
    rows = [L.MT_OMEGA, L.MT_ALPHA, L.MT_DELTA, L.MT_CMIN, L.MT_CMAX]
    assert same(mt[rows], mt0[rows]), 'mt is not cnnq_pc_midtread_params of the published table'
    w = mt[L.MT_WSTART]
    if resident:
        assert bool((w == w[0]).all()) and float(w[0]) == int(w[0]) and float(w[0]) >= -L.MT_HIST_BINS // 2
    else:
        assert same(w, mt0[L.MT_WSTART])
    assert y.dtype == x.dtype and y.shape == x.shape and y.is_contiguous()
    y_ref, _, h_ref, e_ref = nchw_kernel(x, mt, want_hist=hist is not None)
    assert same(y, y_ref), (tuple(x.shape), x.dtype, target, sym, x.storage_offset())
    if hist is None:
        assert ent is None
        return
    n = L.MT_HIST_BINS + 2 + 2 * C
    assert torch.equal(hist[:n], h_ref[:n])
    reps = hist[n:-1].view(L.MT_HIST_REPLICAS, L.MT_HIST_WINDOW).sum(0)
    assert torch.equal(reps, h_ref[n:-1].view(L.MT_HIST_REPLICAS, L.MT_HIST_WINDOW).sum(0))
    assert (int(hist[-1]) != 0) == (int(h_ref[-1]) != 0)
    assert same_scalar(ent, e_ref), (float(ent), float(e_ref))
    assert int(hist[:-1].sum()) == x.numel()


def check(x, ref, target, sym, want_entropy, allow, chans=None, **kw):
    """One call under both points of the contract; (y, entropy, parts)."""
    before = counters()
    resident = route(x, want_entropy, 1 if allow is None else allow, kw.get('out'))[3] == 3
    y, ent, parts = run(x, target, sym, want_entropy=want_entropy, want_parts=True, single_launch=allow, **kw)
    assert counters() == before
    if ref is not None:
        check_tiers(parts['stats'], ref, (True, False, False), chans=chans)
    check_given_table(x, y, ent, parts, target, sym, resident)
    return y, ent, parts


# ---- 1, 2. every branch, both routes, both ranges, with and without the histogram
# (case, single_launch): the chain on every case, the resident form where the channel fits
PAIRS = [(case, allow) for case in HM.CASES for allow in (0, 2) if allow == 0 or case[2][3]]
PAIR_IDS = ['%s-%s' % (i, 'resident' if allow else 'chain') for case, i in zip(HM.CASES, HM.IDS) for allow in (0, 2) if allow == 0 or case[2][3]]


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('case, allow', PAIRS, ids=PAIR_IDS)
def test_contract_on_every_branch_and_route(case, allow, dtype):
    shape, offset, (W, S, cs, fits) = case
    x, ref = case_input(case, dtype)
    for sym in (True, False):
        for want_entropy in (False, True):
            y = torch.empty_like(x)
            assert route(x, want_entropy, allow, y) == (W, S, cs, 3 if allow == 2 else 2), (shape, offset)
            res, _, parts = check(x, ref, TARGET, sym, want_entropy, allow, out=y)
            assert res is y


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_a_channel_that_does_not_fit_takes_the_chain_whatever_the_caller_allows(dtype):
    for case in (HM.CASES[3], HM.CASES[4], HM.CASES[8]):
        x, ref = case_input(case, dtype)
        assert route(x, True, 2)[3] == 2
        y2, e2, p2 = check(x, ref, TARGET, True, True, 2)
        y0, e0, p0 = run(x, TARGET, True, want_entropy=True, want_parts=True, single_launch=0)
        assert same(y2, y0) and same_scalar(e2, e0) and same(p2['stats'], p0['stats']) and same(p2['mt'], p0['mt'])


# ---- 3. repeatability and graphs
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_two_runs_give_the_same_bits(dtype):
    L, ops = mods()
    for case in (HM.CASES[0], HM.CASES[3], HM.CASES[5], HM.CASES[6]):
        x, _ = case_input(case, dtype)
        C = x.shape[1]
        n = L.MT_HIST_BINS + 2 + 2 * C
        for allow in (0, 2):
            y1, e1, p1 = run(x, TARGET, True, want_entropy=True, want_parts=True, single_launch=allow)
            ops.act_qdq_per_channel(x, 4)                               # (another user of the device in between)
            run(half(HC.values((3, 5, 14, 14), 21), dtype), 4, True)    # (and of the workspace)
            y2, e2, p2 = run(x, TARGET, True, want_entropy=True, want_parts=True, single_launch=allow)
            assert same(y1, y2) and same_scalar(e1, e2) and same(p1['stats'], p2['stats']) and same(p1['mt'], p2['mt'])
            assert torch.equal(p1['hist'][:n], p2['hist'][:n]) and int(p1['hist'][-1]) == int(p2['hist'][-1])
            # the hot forms (tables in the cached workspace; entropy without parts) give the same bits
            y3, e3 = run(x, TARGET, True, single_launch=allow)
            assert e3 is None and same(y3, y1)
            y4, e4 = run(x, TARGET, True, want_entropy=True, single_launch=allow)
            assert same(y4, y1) and same_scalar(e4, e1)


@pytest.mark.parametrize('allow, want_entropy', [(0, False), (2, False), (0, True), (2, True)], ids=['chain', 'resident', 'chain-me', 'resident-me'])
def test_graph_capture_replays_eager(allow, want_entropy):
    shape = (8, 12, 28, 28)
    x = half(HC.values(shape, seed=2), torch.bfloat16)
    kw = dict(want_entropy=want_entropy, single_launch=allow)
    eager, ent = run(x, TARGET, True, **kw)
    eager = eager.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run(x, TARGET, True, **kw)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y, e = run(x, TARGET, True, **kw)
    graph.replay()
    torch.cuda.synchronize()
    assert same(y, eager) and (not want_entropy or same_scalar(e, ent))
    keep = x.clone()
    x.copy_(half(HC.values(shape, seed=3), torch.bfloat16))
    graph.replay()
    torch.cuda.synchronize()
    y2, e2 = run(x, TARGET, True, **kw)
    assert not same(y, eager) and same(y, y2) and (not want_entropy or same_scalar(e, e2))
    x.copy_(keep)


# ---- 4. the histogram regimes
def check_entropy_against_unique(x, ent, parts):
    _, codes, _, _ = nchw_kernel(x, parts['mt'], want_codes=True)
    ref = entropy_of(codes)
    assert abs(float(ent) - ref) < 2e-4 * max(1.0, ref), (float(ent), ref)
    return ref


@pytest.mark.parametrize('allow', [0, 2], ids=['chain', 'resident'])
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('shape,target,sym,spread,flagged', REGIMES)
def test_histogram_regimes(shape, target, sym, spread, flagged, dtype, allow):
    L, _ = mods()
    x = half(laplace_like(shape, int(target * 100) + shape[1], spread, sym).cpu(), dtype)
    assert route(x, True, allow)[3] == (3 if allow else 2)
    y, ent, parts = check(x, None, target, sym, True, allow)
    assert (int(parts['hist'][-1]) != 0) == flagged
    assert (int(parts['mt'][L.MT_WSTART][0]) < 0) == sym
    check_entropy_against_unique(x, ent, parts)


@pytest.mark.parametrize('allow', [0, 2], ids=['chain', 'resident'])
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_zero_code_outside_the_window(dtype, allow):
    """A symmetric clip with ~512 bins per channel puts code 0 beyond the window: the register-counted zeros go to the global bins
    and raise the flag word (tests/test_midtread_hist_gpu.py's mostly-zero tensor)."""
    L, _ = mods()
    g = torch.Generator(device='cuda').manual_seed(11)
    x = torch.zeros(8, 16, 14, 14, device='cuda')
    mask = torch.rand(x.shape, device='cuda', generator=g) < 0.02
    x[mask] = torch.randn(int(mask.sum()), device='cuda', generator=g) * 0.01
    x = half(x.cpu(), dtype)
    y, ent, parts = check(x, None, 9.0, True, True, allow)
    assert int(parts['mt'][L.MT_WSTART][0]) + L.MT_HIST_WINDOW <= 0
    assert int(parts['hist'][-1]) != 0 and int(parts['hist'][L.MT_HIST_BINS // 2]) > 0
    assert check_entropy_against_unique(x, ent, parts) > 0.05


# ---- 5. hand-built channels
def hand_built(hw, which):
    xv = HC.values((4, 16) + hw, seed=9)
    if which == 'finite':
        xv[:, 0] = 1.25                                     # constant: std = b = 0, c_min == c_max - ONE value, counted once
        xv[:, 1] = 0.                                       # all zero
        return xv, [0, 1]
    xv[1, 2, 2, 3] = float('nan')
    xv[0, 3, 0, 0] = float('inf')
    xv[2, 4, 1, 1] = float('-inf')
    xv[3, 5, 4, 4] = float('inf')
    xv[3, 5, 5, 5] = float('-inf')
    return xv, [2, 3, 4, 5]


@pytest.mark.parametrize('allow', [0, 2], ids=['chain', 'resident'])
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('hw', [(7, 8), (7, 7)], ids=['7x8', '7x7'])
def test_hand_built_channels(hw, dtype, allow):
    L, ops = mods()
    HW = hw[0] * hw[1]
    want = (8 if HW % 8 == 0 else 1, 1, 1, 3 if allow == 2 and HW % 8 == 0 else 2)
    for which in ('finite', 'special'):
        xv, special = hand_built(hw, which)
        x = half(xv, dtype)
        ref = ref64(x)
        for sym in (True, False):
            assert route(x, True, allow) == want
            before = counters()
            y, ent, parts = run(x, 4, sym, want_entropy=True, want_parts=True, single_launch=allow)
            assert counters() == before
            st = parts['stats'].cpu()
            if which == 'finite':
                # a constant and an all-zero channel: the table in its tiers everywhere, every channel quantized as usual
                check_tiers(parts['stats'], ref, (True, False, False))
                assert st[L.STAT_STD, 0] == 0 and st[L.STAT_B, 0] == 0 and st[L.STAT_MEAN, 0] == 1.25 and not st[:, 1].any()
                assert torch.isfinite(y.float()).all()
                assert y[:, 0].float().unique().numel() == 1 and not y[:, 1].float().any()
            else:
                # NaN and +-inf: the extrema follow torch's rule, the other channels keep their statistics.  (The bin allocation
                # couples every channel to the sum of std^(2/3), which such a channel spoils: y is held to point 2 only.)
                check_tiers(parts['stats'], ref, (True, False, False), chans=[c for c in range(16) if c not in special])
                assert torch.isnan(st[[L.STAT_MIN, L.STAT_MAX, L.STAT_MEAN, L.STAT_STD], 2]).all()
                assert st[L.STAT_MAX, 3] == float('inf') and st[L.STAT_MIN, 4] == float('-inf')
                assert st[L.STAT_MAX, 5] == float('inf') and st[L.STAT_MIN, 5] == float('-inf')
                xf = x.float().cpu()
                assert same(st[L.STAT_MIN, 3], xf[:, 3].min()) and same(st[L.STAT_MAX, 4], xf[:, 4].max())
            check_given_table(x, y, ent, parts, 4, sym, want[3] == 3)
            if which == 'finite':
                check_entropy_against_unique(x, ent, parts)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('hw', [(7, 8), (7, 7)], ids=['7x8', '7x7'])
def test_a_clamp_bound_that_is_an_exact_integer(hw, dtype):
    """A channel whose mean is zero in the table: c_min = 0 and c_max = omega on the non-negative range, -+ omega / 2 on the
    symmetric one - integer codes, not values of their own - next to channels whose bounds are not integers."""
    L, ops = mods()
    x = half(HC.values((4, 16) + hw, seed=9), dtype)
    xf = x.float()
    C = 16
    table = torch.zeros((L.NSTAT, C), dtype=torch.float32, device='cuda')
    table[L.STAT_MIN], table[L.STAT_MAX] = xf.amin(dim=(0, 2, 3)), xf.amax(dim=(0, 2, 3))
    table[L.STAT_MEAN], table[L.STAT_STD] = xf.mean(dim=(0, 2, 3)), xf.std(dim=(0, 2, 3))
    table[L.STAT_B] = (xf - table[L.STAT_MEAN].view(1, C, 1, 1)).abs().mean(dim=(0, 2, 3)) * 0.3     # a narrow range: every bound is hit
    table[L.STAT_MEAN, 7] = 0.
    for sym in (True, False):
        mt = mt_of(table, 3, sym)
        hi, lo, omega = float(mt[L.MT_CMAX, 7]), float(mt[L.MT_CMIN, 7]), float(mt[L.MT_OMEGA, 7])
        integer = not sym or omega % 2 == 0
        assert (hi == int(hi) and lo == int(lo)) == integer, (hi, lo, omega)
        y, ent, parts = run(x, 3, sym, want_entropy=True, stats=table, want_parts=True)
        check_given_table(x, y, ent, parts, 3, sym, False)
        n = L.MT_HIST_BINS + 2
        if integer:
            assert int(parts['hist'][n + 7]) == 0 and int(parts['hist'][n + C + 7]) == 0       # counted as codes
        assert int(parts['hist'][n:n + 2 * C].sum()) > 0                                      # the others: values of their own
        assert torch.isfinite(y.float()).all()
        check_entropy_against_unique(x, ent, parts)


# ---- 6. stats= and out=
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_stats_table_form_and_out(dtype):
    L, ops = mods()
    for case in (HM.CASES[1], HM.CASES[3], HM.CASES[4]):
        x, _ = case_input(case, dtype)
        N, C, HW = ops.geometry(x)
        xf = x.float()
        table = torch.zeros((L.NSTAT, C), dtype=torch.float32, device='cuda')
        table[L.STAT_MIN] = xf.amin(dim=(0, 2, 3)) * 0.8
        table[L.STAT_MAX] = xf.amax(dim=(0, 2, 3)) * 0.9
        table[L.STAT_MEAN] = xf.mean(dim=(0, 2, 3))
        table[L.STAT_STD] = xf.std(dim=(0, 2, 3)) * 1.1
        table[L.STAT_B] = (xf - table[L.STAT_MEAN].view(1, C, 1, 1)).abs().mean(dim=(0, 2, 3)) * 0.9
        for sym, want_entropy in ((True, True), (False, False), (False, True)):
            before = counters()
            y, ent, parts = run(x, 4, sym, want_entropy=want_entropy, stats=table, want_parts=True)
            assert counters() == before and parts['stats'] is table
            assert same(parts['mt'], mt_of(table, 4, sym))                             # params ...
            check_given_table(x, y, ent, parts, 4, sym, False)                         # ... and the table-driven pass
            out = torch.empty_like(x)
            y2, ent2 = run(x, 4, sym, want_entropy=want_entropy, stats=table, out=out)
            assert y2 is out and same(out, y) and (ent is None or same_scalar(ent, ent2))
        # out= on the one-call form, at another alignment than x's: the piece width follows both pointers
        base = torch.zeros(x.numel() + 16, dtype=dtype, device='cuda')
        for off in (0, 1, 2):
            out = base[off:off + x.numel()].view(x.shape)
            base.zero_()
            y, ent, parts = check(x, None, 4, True, True, 2, out=out)
            assert y is out and not base[:off].any() and not base[off + x.numel():].any()      # nothing stored outside out


def test_inside_an_entropy_batch():
    _, ops = mods()
    a = half(HC.values((8, 32, 14, 14), seed=1), torch.bfloat16)
    b = half(HC.values((4, 20, 7, 7), seed=2), torch.float16, 1)
    ya, ea = run(a, 4, True, want_entropy=True, single_launch=2)
    yb, eb = run(b, 3, False, want_entropy=True)
    with ops.entropy_batch() as block:
        ya2, ea2 = run(a, 4, True, want_entropy=True, single_launch=2)
        yb2, eb2 = run(b, 3, False, want_entropy=True)
        assert len(block.mt) == 2                                       # nothing launched yet: they wait for the block's end
    assert same(ya2, ya) and same(yb2, yb) and same_scalar(ea2, ea) and same_scalar(eb2, eb)
    assert float(ea) > 0 and float(eb) > 0


# ---- 7. refusals
def test_refusals():
    L, ops = mods()
    x = half(HC.values((2, 4, 7, 8)), torch.bfloat16)
    table = torch.zeros((L.NSTAT, 4), dtype=torch.float32, device='cuda')
    before = counters()
    for bad in (x.float(),                                                       # float32 takes mid_tread_qdq
                x.cpu(),                                                         # there is no CPU path
                x[0],                                                            # not 4-D
                x[:, 1:3],                                                       # not contiguous
                x[:0],                                                           # empty
                x.to(memory_format=torch.channels_last),                         # dense channels_last: mid_tread_qdq_nhwc's
                None):
        with pytest.raises(L.CnnqError):
            run(bad, TARGET, True)
    for kw in (dict(stats=table[:, :3]), dict(stats=table[:3]), dict(stats=table.double()), dict(stats=table.cpu()),
               dict(out=torch.empty_like(x, dtype=torch.float16)), dict(out=torch.empty_like(x, dtype=torch.float32)),
               dict(out=torch.empty_like(x)[:, :, :5]), dict(out=x), dict(single_launch=5), dict(single_launch=-1)):
        with pytest.raises(L.CnnqError):
            run(x, TARGET, True, **kw)
    with pytest.raises(L.CnnqError):
        run(x, float('nan'), True)                                              # the C side refuses a target that is not finite
    assert counters() == before
    # mid_tread_qdq keeps refusing half tensors
    with pytest.raises(L.CnnqError):
        ops.mid_tread_qdq(x, TARGET, clip=True, sym=True, group=False)
    assert counters() == before


def test_float32_through_the_table_driven_entry_point():
    """CNNQ_DTYPE_F32 forwards cnnq_pc_midtread_qdq_dt to cnnq_pc_midtread_qdq (clip = 1, no codes); the one-call form answers
    CNNQ_ENOTSUP and enqueues nothing."""
    L, ops = mods()
    lib = L.load()
    x = HC.values((3, 10, 14, 14), 5).cuda()
    N, C, HW = ops.geometry(x)
    st, _ = ops.pc_stats(x, N, C, HW, need_b=True, local_only=True)
    mt = mt_of(st, 4, True)
    y = torch.empty_like(x)
    hist = torch.zeros(L.mt_hist_words(C), dtype=torch.int64, device='cuda')
    assert lib.cnnq_pc_midtread_qdq_dt(x.data_ptr(), y.data_ptr(), 0, N, C, HW, mt.data_ptr(), hist.data_ptr(), None) == 0
    torch.cuda.synchronize()
    y0, _, h0, _ = nchw_kernel(x, mt, want_hist=True)
    assert same(y, y0) and torch.equal(hist, h0)
    tabs = ops._midtread_tables(x.device)
    y.fill_(7.)
    ws = torch.empty(64, dtype=torch.float64, device='cuda')
    assert lib.cnnq_pc_midtread_dt(x.data_ptr(), y.data_ptr(), 0, N, C, HW, 4., 1, tabs.data_ptr(), tabs.shape[1], ws.data_ptr(),
                                   st.data_ptr(), mt.data_ptr(), None, 1, None) == -3
    torch.cuda.synchronize()
    assert bool((y == 7.).all())
