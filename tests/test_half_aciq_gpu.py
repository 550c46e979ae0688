"""Dynamic ACIQ clipping (config 3) on contiguous bf16 / fp16 activations: ops.aciq_qdq_half on
cnnq_pc_aciq_qdq_dt.

The contract, on every route and in both dtypes:
  * the table: rows MIN / MAX of `stats` bit exact against x.float() with torch's NaN rule, MEAN / STD / B within the statistics
    tiers of fp64 (check_tiers and ref64 of tests/test_channels_last_collect_gpu.py: mean 2e-6 / 1e-7, std 2e-6, b 3e-6 / 1e-7);
    rows nobody computed are zero (B without Laplace clipping or the b prior);
  * given the table: qp and diag equal ops.pc_params on the published table and y equals ops.pc_qdq on the published qp, bit for
    bit;
  * determinism: run after run the same bits; the routes forced with single_launch 0 / 2 each satisfy both points with their own
    table, and the two tables agree within the tier (both are within it of the same fp64 reference).

The shapes (tests/_half_aciq.py: CASES) are the smallest that reach each branch - every piece width, uneven batch splits, column
splits, a view at an odd element offset, the last population the resident form holds and the first it does not - and every test
asserts the plan through cnnq_pc_route_aciq_dt, so a changed plan cannot silently stop covering a branch."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import _half_aciq as HA
import _half_collect as HC
from test_channels_last_collect_gpu import check_tiers, ref64, same
from test_half_collect_gpu import half

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]
IDS = ['bf16', 'f16']

# (clip, bits, bit_alloc, prior_is_b, positive, target, round_mode)
CONFIGS = [('laplace', 4, True, False, False, None, True),       # the paper's: bit allocation on the std prior (route 3 where it fits)
           ('laplace', 4, True, True, False, None, True),        # ... on the b prior: the chain
           ('laplace', 4, False, False, False, None, True),      # no bit allocation (route 1 where it fits)
           ('gaus', 4, True, False, False, None, True),
           ('gaus', 4, False, False, False, None, True),         # no pass B at all
           ('laplace', 8, True, False, False, None, True),       # 8 bits: no allocation in effect
           ('gaus', 8, False, False, True, None, True),          # positive
           ('laplace', 4, False, False, True, None, True),
           ('laplace', 4, True, False, False, 3, True),          # target = 3
           ('gaus', 4, True, True, False, 3, False)]             # round_mode = False
CIDS = ['%s%d%s%s%s%s%s' % (c[0], c[1], '-ba' if c[2] else '', '-pb' if c[3] else '', '-pos' if c[4] else '',
                            '-t%d' % c[5] if c[5] else '', '' if c[6] else '-ceil') for c in CONFIGS]


def mods():
    from cnn_quantization_amd import _lib as L, ops
    return L, ops


def counters():
    _, ops = mods()
    return ops.LAYOUT_COPIES, importlib.import_module('cnn_quantization_amd.qtypes.int_quantizer').HALF_FALLBACKS


def kwargs(cfg):
    clip, bits, ba, prior, positive, target, rmode = cfg
    return dict(num_bits=bits, positive=positive, clip=clip, bit_alloc=ba, prior_is_b=prior, target=target, round_mode=rmode)


def route(x, cfg, allow, y=None):
    L, ops = mods()
    clip, bits, ba, prior, positive, target, rmode = cfg
    c = ops._params_cfg(bits, positive, clip, ba and bits <= 4, prior, target, rmode, False)
    out = (ctypes.c_int32 * 4)()
    N, C, HW = ops.geometry(x)
    p = x.data_ptr() | (y.data_ptr() if y is not None else 0) | 16
    assert L.load().cnnq_pc_route_aciq_dt(N, C, HW, ops._DTYPE_CODES[x.dtype], p & -p, ctypes.byref(c), allow, out) == 0
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


def check_contract(x, ref, cfg, y, parts, chans=None):
    """The two points of the contract on one result."""
    L, ops = mods()
    clip, bits, ba, prior, positive, target, rmode = cfg
    N, C, HW = ops.geometry(x)
    st, qp, diag = parts['stats'], parts['qp'], parts['diag']
    assert st.shape == (L.NSTAT, C) and qp.shape == (L.NQP, C) and diag.shape == (L.NDIAG, C)
    need_b = clip == 'laplace' or (ba and bits <= 4 and prior)
    check_tiers(st, ref, (need_b, False, False), chans=chans)
    qp0, diag0 = ops.pc_params(st, **kwargs(cfg))
    assert same(qp, qp0), 'qp is not pc_params of the published table'
    assert same(diag, diag0), 'diag is not pc_params of the published table'
    assert y.dtype == x.dtype and y.shape == x.shape and y.is_contiguous()
    assert same(y, ops.pc_qdq(x, N, C, HW, qp)), 'y is not pc_qdq on the published qp'


# ---- 1. every branch, every configuration, both routes
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('case', HA.CASES, ids=HA.IDS)
def test_contract_on_every_branch_and_route(case, dtype):
    L, ops = mods()
    x, ref = case_input(case, dtype)
    shape, offset, (W, S, cs, fits) = case
    before = counters()
    for cfg in CONFIGS:
        ba_on, prior = cfg[2] and cfg[1] <= 4, cfg[3]
        tables = {}
        for allow in (0, 2, None):
            y = torch.empty_like(x)
            want = route(x, cfg, 1 if allow is None else allow, y)
            assert want[:3] == (W, S, cs), (shape, offset, want)
            if allow == 0:
                assert want[3] == 2
            if allow == 2:
                # forced: the resident form wherever the channel fits - behind pass A with bit allocation, never on the b prior
                assert want[3] == ((2 if ba_on and prior else 3 if ba_on else 1) if fits else 2), (cfg, want)
            res, parts = ops.aciq_qdq_half(x, out=y, want_parts=True, single_launch=allow, **kwargs(cfg))
            assert res is y
            check_contract(x, ref, cfg, y, parts)
            tables[allow] = parts['stats'].clone()
        # the extrema are exact on both routes: the same bits (MEAN / STD / B: each within the tier of the same reference)
        assert same(tables[0][[L.STAT_MIN, L.STAT_MAX]], tables[2][[L.STAT_MIN, L.STAT_MAX]])
    assert counters() == before


# ---- 2. hand-built channels: constant, NaN, +-inf, all negative under `positive`
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('hw, w', [(7, 1), (8, 8), (6, 4)], ids=['W1', 'W8', 'W4'])
def test_hand_built_channels(hw, w, dtype):
    L, ops = mods()
    xv = HC.values((3, 7, hw, hw), seed=9)
    xv[:, 0] = 0.25                                         # constant: std = b = 0, the 1e-8 scale floor
    xv[1, 1, 2, 3] = float('nan')
    xv[0, 2, 0, 0] = float('inf')
    xv[2, 3, 1, 1] = float('-inf')
    xv[:, 4] = -xv[:, 4].abs() - 0.125                      # all negative
    finite = [0, 4, 5, 6]
    x = half(xv, dtype)
    ref = ref64(x)
    N, C, HW = ops.geometry(x)
    for cfg in (CONFIGS[0], CONFIGS[2], CONFIGS[4], CONFIGS[6], CONFIGS[7]):
        for allow in (0, 2):
            assert route(x, cfg, allow)[0] == w
            assert route(x, cfg, allow)[3] == (2 if allow == 0 or w == 1 else 3 if cfg[2] and cfg[1] <= 4 else 1)
            y, parts = ops.aciq_qdq_half(x, want_parts=True, single_launch=allow, **kwargs(cfg))
            st, qp = parts['stats'].cpu(), parts['qp'].cpu()
            need_b = cfg[0] == 'laplace'
            check_tiers(parts['stats'], ref, (need_b, False, False), chans=finite)
            xf = x.float().cpu()
            assert torch.isnan(st[[L.STAT_MIN, L.STAT_MAX, L.STAT_MEAN, L.STAT_STD], 1]).all()
            assert st[L.STAT_MAX, 2] == float('inf') and st[L.STAT_MIN, 3] == float('-inf')
            assert same(st[L.STAT_MIN, 2], xf[:, 2].min()) and same(st[L.STAT_MAX, 3], xf[:, 3].max())
            assert st[L.STAT_STD, 0] == 0 and st[L.STAT_B, 0] == 0 and st[L.STAT_MEAN, 0] == 0.25
            # given the table, everything else bit for bit - NaN and inf channels included
            qp0, diag0 = ops.pc_params(parts['stats'], **kwargs(cfg))
            assert same(parts['qp'], qp0) and same(parts['diag'], diag0)
            assert same(y, ops.pc_qdq(x, N, C, HW, parts['qp']))
            if not (cfg[2] and cfg[1] <= 4):
                # (with bit allocation a non-finite prior turns every channel's width into NaN; without it channels are independent)
                if not cfg[4]:
                    assert qp[L.QP_SCALE, 0] == np.float32(1e-8)        # (positive: the range reaches from 0 up to the mean)
                assert torch.isfinite(y[:, finite].float()).all()
                if cfg[4]:
                    # all negative under `positive`: clipped to the range [0, alpha], i.e. to zero
                    assert not y[:, 4].float().any()


# ---- 3. determinism
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_two_runs_give_the_same_bits(dtype):
    _, ops = mods()
    for case in (HA.CASES[0], HA.CASES[3], HA.CASES[5], HA.CASES[6]):
        x, _ = case_input(case, dtype)
        for cfg in (CONFIGS[0], CONFIGS[2]):
            for allow in (0, 2):
                y1, p1 = ops.aciq_qdq_half(x, want_parts=True, single_launch=allow, **kwargs(cfg))
                ops.act_qdq_per_channel(x, 4)                       # (another user of the device in between)
                ops.aciq_qdq_half(half(HC.values((3, 5, 14, 14), 21), dtype), 4)      # (and of the workspace)
                y2, p2 = ops.aciq_qdq_half(x, want_parts=True, single_launch=allow, **kwargs(cfg))
                assert same(y1, y2) and all(same(p1[k], p2[k]) for k in ('stats', 'qp', 'diag'))
                # without parts: the tables in the cached workspace, the same y
                assert same(y1, ops.aciq_qdq_half(x, single_launch=allow, **kwargs(cfg)))


# ---- 4. the op's surface: out=, stats=, refusals
def test_out_parts_and_stats():
    L, ops = mods()
    x, ref = case_input(HA.CASES[1], torch.bfloat16)
    N, C, HW = ops.geometry(x)
    cfg = CONFIGS[0]
    y0 = ops.aciq_qdq_half(x, **kwargs(cfg))
    assert isinstance(y0, torch.Tensor) and y0.dtype == x.dtype
    out = torch.empty_like(x)
    assert ops.aciq_qdq_half(x, out=out, **kwargs(cfg)) is out and same(out, y0)
    for bad in (torch.empty_like(x, dtype=torch.float16), torch.empty_like(x, dtype=torch.float32), torch.empty_like(x)[:, :, :7],
                torch.empty(x.shape, dtype=x.dtype), x):
        with pytest.raises(L.CnnqError):
            ops.aciq_qdq_half(x, out=bad, **kwargs(cfg))
    # stats given (-sm use): pc_params and the table-driven Q/DQ
    table, _ = ops.pc_stats_half(x, need_b=True)
    y, parts = ops.aciq_qdq_half(x, stats=table, want_parts=True, **kwargs(cfg))
    qp, diag = ops.pc_params(table, **kwargs(cfg))
    assert parts['stats'] is table and same(parts['qp'], qp) and same(parts['diag'], diag) and same(y, ops.pc_qdq(x, N, C, HW, qp))
    with pytest.raises(L.CnnqError):
        ops.aciq_qdq_half(x, stats=table[:, :3], **kwargs(cfg))
    with pytest.raises(L.CnnqError):
        ops.aciq_qdq_half(x, single_launch=3, **kwargs(cfg))


def test_refusals():
    L, ops = mods()
    x = half(HC.values((2, 4, 7, 8)), torch.bfloat16)
    before = counters()
    for bad in (x.float(),                                                       # float32 takes act_qdq_per_channel
                x.cpu(),                                                         # there is no CPU path
                x[0],                                                            # not 4-D
                x.to(memory_format=torch.channels_last),                         # not contiguous: dense channels_last
                x[:, 1:3],                                                       # not contiguous: not dense
                x.double(), None):
        with pytest.raises(L.CnnqError):
            ops.aciq_qdq_half(bad, 4)
    for clip in ('no', 'mix', '2std'):
        with pytest.raises(L.CnnqError):
            ops.aciq_qdq_half(x, 4, clip=clip)
    with pytest.raises(L.CnnqError):
        ops.aciq_qdq_half(x, 16)                                                 # the factor tables end at 8 bits
    assert counters() == before
    # act_qdq_per_channel's refusal of a half tensor under clipping is what it was
    with pytest.raises(L.CnnqError):
        ops.act_qdq_per_channel(x, 4, clip='laplace')


def test_float32_through_the_same_entry_point():
    """CNNQ_DTYPE_F32 forwards to cnnq_pc_aciq_qdq: its y, qp and diag, and a copy of its table."""
    L, ops = mods()
    lib = L.load()
    x = HC.values((3, 10, 14, 14), 5).cuda()
    N, C, HW = ops.geometry(x)
    cfg = ops._params_cfg(4, False, 'laplace', True, False, None, True, False)
    outs = []
    for dt_call in (True, False):
        ws = torch.empty(lib.cnnq_pc_aciq_dt_workspace(N, C, HW, 0), dtype=torch.uint8, device='cuda')
        y, st = torch.empty_like(x), torch.empty(L.NSTAT, C, device='cuda')
        qp, diag = torch.empty(L.NQP, C, device='cuda'), torch.empty(L.NDIAG, C, device='cuda')
        if dt_call:
            assert lib.cnnq_pc_aciq_qdq_dt(x.data_ptr(), y.data_ptr(), 0, N, C, HW, ctypes.byref(cfg), ws.data_ptr(), st.data_ptr(),
                                           qp.data_ptr(), diag.data_ptr(), 1, None) == 0
            torch.cuda.synchronize()
            st0, _ = ops.pc_stats(x, N, C, HW, need_b=True)
            assert same(st, st0)
        else:
            assert lib.cnnq_pc_aciq_qdq(x.data_ptr(), y.data_ptr(), N, C, HW, ctypes.byref(cfg), ws.data_ptr(), qp.data_ptr(),
                                        diag.data_ptr(), None) == 0
            torch.cuda.synchronize()
        outs.append((y, qp, diag))
    assert all(same(a, b) for a, b in zip(*outs))


# ---- 5. graph capture
def test_graph_capture_replays_eager():
    _, ops = mods()
    shape = (8, 12, 28, 28)
    x = half(HC.values(shape, seed=2), torch.bfloat16)
    for cfg, allow in ((CONFIGS[0], 2), (CONFIGS[2], 2), (CONFIGS[0], 0)):
        eager = ops.aciq_qdq_half(x, single_launch=allow, **kwargs(cfg)).clone()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            ops.aciq_qdq_half(x, single_launch=allow, **kwargs(cfg))
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            y = ops.aciq_qdq_half(x, single_launch=allow, **kwargs(cfg))
        graph.replay()
        torch.cuda.synchronize()
        assert same(y, eager)
        x2 = half(HC.values(shape, seed=3), torch.bfloat16)
        keep = x.clone()
        x.copy_(x2)
        graph.replay()
        torch.cuda.synchronize()
        assert not same(y, eager) and same(y, ops.aciq_qdq_half(x, single_launch=allow, **kwargs(cfg)))
        x.copy_(keep)
