"""The uniform per-channel Q/DQ that counts its codes (-me) on contiguous bf16 / fp16 activations:
cnnq_pc_qdq_hist_dt, cnnq_pc_minmax_qdq_hist_dt and cnnq_pc_aciq_qdq_hist_dt, ops.act_qdq_per_channel(want_entropy=True) and
ops.aciq_qdq_half(want_entropy=True) on them, and the quantizer's route 'half_entropy'.

The contract, everything bit for bit (NaN == NaN), no tolerances - min / max are exact and the Q/DQ is element by element:
  * given a table qp: y equals cnnq_pc_qdq_dt's and pc_qdq(x.float(), qp).to(x.dtype); the replica tables folded by
    cnnq_hist_replicas_fold equal, word for word, the histogram pc_qdq(x.float(), ..., hist=) fills; they sum to x.numel() and are
    zero after the fold or an entropy launch;
  * config 2: act_qdq_per_channel(x, bits, positive, want_entropy=True) returns y and an entropy that equal the same call on
    x.float() (y cast); qp / mm equal cnnq_pc_minmax_qdq_auto_dt's; the two routes give the same bits; HALF_FALLBACKS does not move;
  * config 3: the statistics table within section 25's tiers of fp64 (extrema exact); given that table, qp, diag, y, the histogram
    and the entropy are cnnq_pc_params' and the fp32 table-driven pass's.
The hand-built inputs (the construction of tests/test_code_hist_exact_gpu.py) have a histogram numpy knows: compared word for
word, the entropy within tests/_entropy.py's tier of its fp64 value.

The shapes (tests/_half_entropy.py: CASES) are the smallest that reach each branch and every test asserts the plan through
cnnq_pc_route_qdq_hist_dt, so a changed plan cannot silently stop covering a branch.  Needs an MI355X: `pytest -m gpu`."""
import ctypes

import numpy as np
import pytest
import torch

import _entropy as E
import _half_collect as HC
import _half_entropy as HE
import _quantizer as Q
from test_channels_last_bcorr_gpu import iq_mod, mods
from test_channels_last_collect_gpu import check_tiers, ref64, same
from test_code_hist_exact_gpu import exact_in, qp_table, uniform_input
from test_half_collect_gpu import half

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]
IDS = ['bf16', 'f16']
BITS = [(2, False), (2, True), (4, False), (4, True), (8, False), (8, True)]          # (num_bits, positive)


def same_scalar(a, b):
    return same(a.reshape(1).float(), b.reshape(1).float())


def replicas():
    L, _ = mods()
    return torch.zeros(L.load().cnnq_hist_replica_bytes() // 8, dtype=torch.int64, device='cuda')


def fold(rep):
    """The replica tables folded into one 256-word table; they are left zero."""
    L, ops = mods()
    out = torch.zeros(256, dtype=torch.int64, device='cuda')
    L.check(L.load().cnnq_hist_replicas_fold(ops._ptr(rep), ops._ptr(out), ops._stream(rep)), 'cnnq_hist_replicas_fold')
    assert int(rep.abs().sum()) == 0
    return out


def route(x, nbins, allow, y=None):
    L, ops = mods()
    out = (ctypes.c_int32 * 4)()
    N, C, HW = ops.geometry(x)
    p = x.data_ptr() | (y.data_ptr() if y is not None else 0) | 16
    assert L.load().cnnq_pc_route_qdq_hist_dt(N, C, HW, ops._DTYPE_CODES[x.dtype], p & -p, nbins, allow, out) == 0
    return tuple(out)


def counters():
    _, ops = mods()
    return ops.LAYOUT_COPIES, iq_mod().HALF_FALLBACKS


_INPUTS = {}


def case_input(case, dtype):
    """The case's tensor, made once per (case, dtype) and left unchanged."""
    key = (case[0], case[1], dtype)
    if key not in _INPUTS:
        shape, offset, _ = case
        _INPUTS[key] = half(HC.values(shape, HC.seed_of(shape, offset)), dtype, offset)
    return _INPUTS[key]


def auto_dt(x, bits, positive):
    """cnnq_pc_minmax_qdq_auto_dt on a workspace of the test's own: (y, qp, mm) - what config 2 without the count publishes."""
    L, ops = mods()
    lib = L.load()
    N, C, HW = ops.geometry(x)
    ws = torch.empty(lib.cnnq_pc_minmax_qdq_workspace(N, C, HW) // 4, dtype=torch.float32, device='cuda')
    y = torch.empty_like(x)
    L.check(lib.cnnq_pc_minmax_qdq_auto_dt(ops._ptr(x), ops._ptr(y), ops._DTYPE_CODES[x.dtype], N, C, HW, bits, int(positive), ops._ptr(ws),
                                           None, 0, 1, ops._stream(x)), 'cnnq_pc_minmax_qdq_auto_dt')
    return y, ws[:L.NQP * C].view(L.NQP, C).clone(), ws[L.NQP * C:(L.NQP + 2) * C].view(2, C).clone()


def table_pass(x, qp, nbins, rep=None):
    """cnnq_pc_qdq_hist_dt through the C ABI: (y, the replica tables)."""
    L, ops = mods()
    N, C, HW = ops.geometry(x)
    y = torch.empty_like(x)
    rep = replicas() if rep is None else rep
    L.check(L.load().cnnq_pc_qdq_hist_dt(ops._ptr(x), ops._ptr(y), ops._DTYPE_CODES[x.dtype], N, C, HW, ops._ptr(qp), nbins, ops._ptr(rep),
                                         ops._stream(x)), 'cnnq_pc_qdq_hist_dt')
    return y, rep


def minmax_pass(x, bits, positive, allow):
    """cnnq_pc_minmax_qdq_hist_dt through the C ABI on buffers of the test's own: (y, qp, mm, the replica tables)."""
    L, ops = mods()
    lib = L.load()
    N, C, HW = ops.geometry(x)
    ws = torch.empty(lib.cnnq_pc_minmax_qdq_workspace(N, C, HW) // 4, dtype=torch.float32, device='cuda')
    y, rep = torch.empty_like(x), replicas()
    qp = torch.full((L.NQP, C), -7.25, dtype=torch.float32, device='cuda')
    mm = torch.full((2, C), -7.25, dtype=torch.float32, device='cuda')
    L.check(lib.cnnq_pc_minmax_qdq_hist_dt(ops._ptr(x), ops._ptr(y), ops._DTYPE_CODES[x.dtype], N, C, HW, bits, int(positive), ops._ptr(ws),
                                           ops._ptr(qp), ops._ptr(mm), ops._ptr(rep), allow, ops._stream(x)), 'cnnq_pc_minmax_qdq_hist_dt')
    return y, qp, mm, rep


def f32_table(x, qp):
    """The fp32 table-driven pass on x.float(): (y cast to x's dtype, its plain 256-word histogram)."""
    _, ops = mods()
    N, C, HW = ops.geometry(x)
    hist = torch.zeros(256, dtype=torch.int64, device='cuda')
    y = ops.pc_qdq(x.float(), N, C, HW, qp, hist=hist)
    return y.to(x.dtype), hist


def check_given_table(x, qp, nbins, y, rep):
    """The first point of the contract on one result of a counting launch."""
    _, ops = mods()
    N, C, HW = ops.geometry(x)
    y_ref, h_ref = f32_table(x, qp)
    assert y.dtype == x.dtype and y.shape == x.shape and y.is_contiguous()
    assert same(y, y_ref), 'y is not the fp32 pass on x.float(), cast'
    assert same(y, ops.pc_qdq(x, N, C, HW, qp)), 'y is not cnnq_pc_qdq_dt on the same table'
    assert int(rep.sum()) == x.numel() and int(rep.min()) >= 0
    assert not rep.view(64, 256)[:, nbins:].any(), 'a count beyond the bins the launch keeps'
    got = fold(rep)
    assert torch.equal(got, h_ref), (got[:nbins].tolist(), h_ref[:nbins].tolist())


# ---- 1. the table-driven pass and config 2 on every branch, both routes
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('case', HE.CASES, ids=HE.IDS)
def test_contract_on_every_branch_and_route(case, dtype):
    _, ops = mods()
    x = case_input(case, dtype)
    shape, offset, (W, S, cs, fits) = case
    before = counters()
    for bits, positive in BITS:
        nbins = 1 << bits
        assert route(x, nbins, 2) == (W, S, cs, 1 if fits else 2), (shape, offset, route(x, nbins, 2))
        assert route(x, nbins, 0) == (W, S, cs, 2)
        y0, qp0, mm0 = auto_dt(x, bits, positive)
        # the table-driven pass, on config 2's table and with 256 bins too
        for nb in (nbins, 256):
            y, rep = table_pass(x, qp0, nb)
            check_given_table(x, qp0, nb, y, rep)
        # config 2: both routes
        for allow in (0, 2):
            y, qp, mm, rep = minmax_pass(x, bits, positive, allow)
            assert same(qp, qp0) and same(mm, mm0), (bits, positive, allow)
            assert same(y, y0), (bits, positive, allow)
            check_given_table(x, qp, nbins, y, rep)
        # the op: the same call on x.float(), y cast
        y, ent = ops.act_qdq_per_channel(x, bits, positive, want_entropy=True)
        yf, entf = ops.act_qdq_per_channel(x.float(), bits, positive, want_entropy=True)
        assert same(y, yf.to(dtype)) and same(y, y0) and same_scalar(ent, entf), (bits, positive, float(ent), float(entf))
        if fits:
            y2, ent2 = ops._minmax_qdq_half_entropy(x, *ops.geometry(x), bits, positive, None, single_launch=2)
            assert same(y2, y) and same_scalar(ent2, ent)
    assert counters() == before


def test_the_long_tile():
    """The one class of the cases that takes the long parts of the counting launch (32768 elements): three batch splits."""
    _, ops = mods()
    x = case_input(HE.LONG_TILE, torch.bfloat16)
    N, C, HW = ops.geometry(x)
    assert HE.hist_elems(N, C, HW) == 4 * HE.H_QDQ_ELEMS and route(x, 16, 0) == HE.LONG_TILE[2][:3] + (2,)
    y0, qp0, mm0 = auto_dt(x, 4, False)
    y, qp, mm, rep = minmax_pass(x, 4, False, 0)
    assert same(qp, qp0) and same(mm, mm0) and same(y, y0)
    check_given_table(x, qp, 16, y, rep)


# ---- 2. hand-built exact histograms
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('zp_kind', ['zero', 'qmax', 'mixed'])
@pytest.mark.parametrize('kind', ['all_codes', 'one_code', 'zero_point'])
def test_hand_built_histograms(kind, zp_kind, dtype):
    L, ops = mods()
    lib = L.load()
    for shape in ((2, 3, 5, 7), (2, 4, 8, 8), (3, 8, 1, 2), (8, 16, 28, 28), (3, 70, 2, 4)):
        for bits in (2, 4, 8):
            if kind == 'one_code' and bits == 2:
                continue                                                          # (the construction's one code is 5)
            qp = qp_table(shape[1], bits, zp_kind)
            xv, want = uniform_input(shape, qp, kind, seed=bits + shape[0])
            assert exact_in(xv, dtype)
            table = np.bincount(want.reshape(-1), minlength=256).astype(np.int64)
            h64 = E.entropy64(table, xv.size)
            x, qd = half(torch.from_numpy(xv), dtype), torch.from_numpy(qp).cuda()
            y, rep = table_pass(x, qd, 1 << bits)
            assert int(rep.sum()) == xv.size
            per_bin = rep.view(64, 256).sum(0).cpu().numpy()
            assert np.array_equal(per_bin, table), (shape, bits)
            out = torch.full((1,), -7.25, dtype=torch.float32, device='cuda')
            L.check(lib.cnnq_entropy_replicas(ops._ptr(rep), ops._ptr(out), ops._stream(rep)), 'cnnq_entropy_replicas')
            assert abs(float(out) - h64) <= E.tier(h64), (shape, bits, float(out), h64)
            assert int(rep.abs().sum()) == 0                                        # the entropy launch leaves the tables zero
            assert same(y, f32_table(x, qd)[0])


# ---- 3. special values
def special(dtype, hw):
    xv = HC.values((3, 8, hw, hw), seed=9)
    xv[:, 0] = 0.25                                         # constant: the 1e-8 scale floor
    xv[1, 1, 2, 3] = float('nan')                           # poisons its channel alone in config 2
    xv[0, 2, 0, 0] = float('inf')
    xv[2, 3, 1, 1] = float('-inf')
    xv[:, 4] = xv[:, 4].clamp(min=0)                        # post-ReLU: about half zeros
    xv[0, 5, 0, :3] = -0.0
    xv[:, 6] = 0.                                           # all zero: every element the zero point's code
    return half(xv, dtype)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('hw, w', [(7, 1), (8, 8), (6, 4)], ids=['W1', 'W8', 'W4'])
def test_special_values(hw, w, dtype):
    L, ops = mods()
    x = special(dtype, hw)
    N, C, HW = ops.geometry(x)
    finite = [0, 4, 5, 6, 7]
    for bits, positive in BITS:
        nbins = 1 << bits
        assert route(x, nbins, 2)[0] == w and route(x, nbins, 2)[3] == (2 if w == 1 else 1)
        y0, qp0, mm0 = auto_dt(x, bits, positive)
        for allow in (0, 2):
            y, qp, mm, rep = minmax_pass(x, bits, positive, allow)
            assert same(qp, qp0) and same(mm, mm0) and same(y, y0)
            q = qp.cpu()
            assert torch.isnan(q[L.QP_SCALE, 1]) and torch.isfinite(q[:, finite]).all()
            assert q[L.QP_SCALE, 0] == np.float32(1e-8) or positive
            # the NaN channel: every element's code is NaN - bin 0; the other channels are untouched by it
            assert int(rep.view(64, 256).sum(0)[0]) >= N * HW
            assert torch.isnan(y[:, 1].float()).all() and torch.isfinite(y[:, finite].float()).all()
            check_given_table(x, qp, nbins, y, rep)
        y, ent = ops.act_qdq_per_channel(x, bits, positive, want_entropy=True)
        yf, entf = ops.act_qdq_per_channel(x.float(), bits, positive, want_entropy=True)
        assert same(y, yf.to(dtype)) and same_scalar(ent, entf)
    # a table of the caller's that does not bound the values: the infinities clamp to the ends before the count
    qp, _ = ops.pc_params(ops.pc_stats(x.float().nan_to_num(0., 1., -1.), N, C, HW)[0], 4)
    y, rep = table_pass(x, qp, 16)
    check_given_table(x, qp, 16, y, rep)


# ---- 4. config 3: the chain with the counting pass last
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('case', [HE.CASES[i] for i in (1, 2, 4, 5, 7, 8)], ids=[HE.IDS[i] for i in (1, 2, 4, 5, 7, 8)])
def test_config3_given_the_table(case, dtype):
    L, ops = mods()
    x = case_input(case, dtype)
    ref = ref64(x)
    N, C, HW = ops.geometry(x)
    before = counters()
    # (clip, bits, bit_alloc, prior_is_b, positive)
    for clip, bits, ba, prior, positive in (('laplace', 4, False, False, False), ('gaus', 4, False, False, True),
                                            ('laplace', 4, True, False, False), ('gaus', 3, True, True, False),
                                            ('laplace', 8, False, False, False), ('gaus', 2, False, False, False)):
        kw = dict(num_bits=bits, positive=positive, clip=clip, bit_alloc=ba, prior_is_b=prior)
        use_ba = ba and bits <= 4
        nbins = 256 if use_ba else 1 << bits
        y, ent, parts = ops.aciq_qdq_half(x, want_parts=True, want_entropy=True, **kw)
        check_tiers(parts['stats'], ref, (clip == 'laplace' or (use_ba and prior), False, False))
        qp0, diag0 = ops.pc_params(parts['stats'], **kw)
        assert same(parts['qp'], qp0) and same(parts['diag'], diag0)
        # given the table: y, the histogram and the entropy are the fp32 table-driven pass's
        y_ref, h_ref = f32_table(x, parts['qp'])
        assert same(y, y_ref) and same(y, ops.pc_qdq(x, N, C, HW, parts['qp']))
        assert same_scalar(ent, ops.entropy_from_hist(h_ref)), (kw, float(ent))
        y1, rep = table_pass(x, parts['qp'], nbins)
        check_given_table(x, parts['qp'], nbins, y1, rep)
        # without the count: the same y; with the table handed in (-sm use): the same y and entropy
        assert same(y, ops.aciq_qdq_half(x, single_launch=0, **kw))
        y2, ent2 = ops.aciq_qdq_half(x, stats=parts['stats'], want_entropy=True, **kw)
        assert same(y2, y) and same_scalar(ent2, ent)
    assert counters() == before
    assert not ops._hist_replicas(x, ops._raw_stream(x.device.index)).any()          # zero at rest


def test_config3_through_the_c_abi():
    """cnnq_pc_aciq_qdq_hist_dt on buffers of the test's own: the tables it leaves, y and the counts."""
    L, ops = mods()
    lib = L.load()
    x = case_input(HE.CASES[6], torch.float16)
    N, C, HW = ops.geometry(x)
    for ba in (False, True):
        cfg = ops._params_cfg(4, False, 'laplace', ba, False, None, True, False)
        ws = torch.empty(lib.cnnq_pc_aciq_dt_workspace(N, C, HW, 2), dtype=torch.uint8, device='cuda')
        st, qp = torch.empty(L.NSTAT, C, device='cuda'), torch.empty(L.NQP, C, device='cuda')
        diag, y, rep = torch.empty(L.NDIAG, C, device='cuda'), torch.empty_like(x), replicas()
        L.check(lib.cnnq_pc_aciq_qdq_hist_dt(ops._ptr(x), ops._ptr(y), 2, N, C, HW, ctypes.byref(cfg), ops._ptr(ws), ops._ptr(st), ops._ptr(qp),
                                             ops._ptr(diag), ops._ptr(rep), ops._stream(x)), 'cnnq_pc_aciq_qdq_hist_dt')
        check_tiers(st, ref64(x), (True, False, False))
        qp0, diag0 = ops.pc_params(st, 4, False, 'laplace', ba)
        assert same(qp, qp0) and same(diag, diag0)
        check_given_table(x, qp, 256 if ba else 16, y, rep)


# ---- 5. entropy_batch, graph capture, the workspace
def test_entropy_batch_fills_at_the_end_of_the_block():
    _, ops = mods()
    a = case_input(HE.CASES[11], torch.bfloat16)            # the resident form
    b = case_input(HE.CASES[4], torch.float16)              # W = 1: the two launches
    c = case_input(HE.CASES[2], torch.bfloat16)
    assert route(a, 16, 1)[3] in (1, 2) and route(b, 4, 1)[3] == 2
    ya, ea = ops._minmax_qdq_half_entropy(a, *ops.geometry(a), 4, True, None, single_launch=2)
    yb, eb = ops.act_qdq_per_channel(b, 2, want_entropy=True)
    yc, ec = ops.aciq_qdq_half(c, 4, clip='laplace', want_entropy=True)
    with ops.entropy_batch() as block:
        ya2, ea2 = ops._minmax_qdq_half_entropy(a, *ops.geometry(a), 4, True, None, single_launch=2)
        yb2, eb2 = ops.act_qdq_per_channel(b, 2, want_entropy=True)
        yc2, ec2 = ops.aciq_qdq_half(c, 4, clip='laplace', want_entropy=True)
        assert block.n == 3                                 # nothing launched yet: they wait for the block's end
    assert same(ya2, ya) and same(yb2, yb) and same(yc2, yc)
    assert same_scalar(ea2, ea) and same_scalar(eb2, eb) and same_scalar(ec2, ec)
    assert 0 < float(ea) <= 4 and 0 < float(eb) <= 2 and 0 < float(ec) <= 4
    assert not ops._ENT_TABLES[(a.device.index, ops._raw_stream(a.device.index))].any()


@pytest.mark.parametrize('allow', [0, 2], ids=['two-launches', 'resident'])
def test_graph_capture_replays_eager(allow):
    """After one eager call on the capturing stream (the replica tables are zero-filled once, outside a capture) the counting
    launches are captured; two replays, the second on refreshed input, give the eager results."""
    _, ops = mods()
    shape = (8, 32, 14, 14)
    x = half(HC.values(shape, seed=2), torch.bfloat16)
    geo = ops.geometry(x)
    run = lambda: ops._minmax_qdq_half_entropy(x, *geo, 4, False, None, single_launch=allow)
    eager, e_eager = run()
    eager, e_eager = eager.clone(), e_eager.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    before = counters()
    with torch.cuda.graph(graph, stream=s):
        y, ent = run()
    assert counters() == before
    graph.replay()
    torch.cuda.synchronize()
    assert same(y, eager) and same_scalar(ent, e_eager)
    x.copy_(half(HC.values(shape, seed=3), torch.bfloat16))
    graph.replay()
    torch.cuda.synchronize()
    y_now, e_now = run()
    assert same(y, y_now) and same_scalar(ent, e_now) and not same(y, eager)


def test_first_use_under_a_capture_names_the_remedy(monkeypatch):
    """No replica table can be had for a stream under a capture: a CnnqError that says what to do, nothing launched."""
    L, ops = mods()
    x = case_input(HE.CASES[1], torch.bfloat16)
    monkeypatch.setattr(ops, '_HIST_REP', {})
    monkeypatch.setattr(torch.cuda, 'is_current_stream_capturing', lambda: True)
    for call in (lambda: ops.act_qdq_per_channel(x, 4, want_entropy=True), lambda: ops.aciq_qdq_half(x, 4, want_entropy=True)):
        with pytest.raises(L.CnnqError, match='one eager want_entropy call'):
            call()
    monkeypatch.undo()
    assert isinstance(ops.act_qdq_per_channel(x, 4, want_entropy=True), tuple)


def test_another_user_of_the_workspace_in_between():
    _, ops = mods()
    for case, dtype in ((HE.CASES[7], torch.bfloat16), (HE.CASES[11], torch.float16)):
        x = case_input(case, dtype)
        other = half(HC.values((3, 5, 14, 14), 21), dtype)
        for run in (lambda: ops.act_qdq_per_channel(x, 4, want_entropy=True),
                    lambda: ops.aciq_qdq_half(x, 4, want_entropy=True),
                    lambda: ops._minmax_qdq_half_entropy(x, *ops.geometry(x), 4, False, None, single_launch=2)):
            y1, e1 = run()
            ops.act_qdq_per_channel(other, 4)                           # (the same cached workspace)
            ops.act_qdq_per_channel(other, 8, want_entropy=True)        # (and the same replica tables)
            ops.aciq_qdq_half(other, 4)
            y2, e2 = run()
            assert same(y1, y2) and same_scalar(e1, e2)


def test_what_the_ops_still_refuse():
    L, ops = mods()
    x = case_input(HE.CASES[1], torch.bfloat16)
    before = counters()
    for kw in (dict(want_codes=True), dict(want_codes=True, want_entropy=True), dict(want_parts=True, want_entropy=True),
               dict(want_entropy=True, clip='laplace'), dict(want_entropy=True, bit_alloc=True), dict(want_entropy=True, bcorr=True),
               dict(want_entropy=True, whole_tensor=True), dict(want_entropy=True, per_channel_dim=0)):
        with pytest.raises(L.CnnqError):
            ops.act_qdq_per_channel(x, 4, **kw)
    with pytest.raises(L.CnnqError):
        ops.act_qdq_per_channel(x, 9, want_entropy=True)                # codes wider than a byte
    N, C, HW = ops.geometry(x)
    with pytest.raises(L.CnnqError):
        ops.pc_qdq(x, N, C, HW, auto_dt(x, 4, False)[1], hist=torch.zeros(256, dtype=torch.int64, device='cuda'))
    assert counters() == before
    # with a table (-sm use): the table-driven pass that counts
    st, _ = ops.pc_stats_half(x)
    y, ent = ops.act_qdq_per_channel(x, 4, stats=st, want_entropy=True)
    yf, entf = ops.act_qdq_per_channel(x.float(), 4, stats=st, want_entropy=True)
    assert same(y, yf.to(x.dtype)) and same_scalar(ent, entf)


# ---- 6. the quantizer
class Logger:
    def __init__(self):
        self.rows = []

    def log_metric(self, name, value, step=None, meterId=None, weight=None):
        self.rows.append((name, value, meterId, weight))


def counted(q, x, **kw):
    iq, (_, ops) = iq_mod(), mods()
    fb, copies = iq.HALF_FALLBACKS, ops.LAYOUT_COPIES
    y = q(x, 'act', **kw)
    return y, iq.HALF_FALLBACKS - fb, ops.LAYOUT_COPIES - copies


def calibration(x):
    L, _ = mods()
    xf = x.float()
    C = x.shape[1]
    stat = {'min': xf.amin(dim=(0, 2, 3)) * 0.8, 'max': xf.amax(dim=(0, 2, 3)) * 0.9, 'mean': xf.mean(dim=(0, 2, 3)),
            'std': xf.std(dim=(0, 2, 3)), 'b': (xf - xf.mean(dim=(0, 2, 3)).view(1, C, 1, 1)).abs().mean(dim=(0, 2, 3))}

    class SM:
        def get_tensor_stat(self, stat_id, name, kind='mean'):
            return stat[name].cpu().numpy()
    return SM


@pytest.mark.parametrize('clipping', ['no', 'laplace'])
@pytest.mark.parametrize('stat_id', [None, 'layer0'], ids=['dynamic', 'stat_id'])
def test_quantizer_takes_the_native_route_when_opted_in(stat_id, clipping, monkeypatch):
    """Config 2 (dynamic and from the calibration table): the upcast route's y and logged entropy, bit for bit, without the upcast.
    Config 3 from the table: the same (given the table everything is bit for bit); dynamic config 3 computes its statistics in
    another order than the fp32 chain, so it is compared with the op, whose contract test_config3_given_the_table checks."""
    _, ops = mods()
    x = HC.values((8, 32, 14, 14), seed=6).to(torch.bfloat16).cuda()
    log = Logger()
    q = Q.quantizer(pcq_act=True, measure_entropy=True, clipping=clipping, logger=log)
    q.sm = calibration(x)
    assert q.half_entropy is False
    # the default: one counted upcast, the fp32 route's result cast back - as before
    y0, n, copies = counted(q, x, stat_id=stat_id)
    assert (n, copies) == (1, 0) and y0.dtype == x.dtype
    e0 = log.rows[-1][1]
    del log.rows[:]
    q.half_entropy = True
    y, n, copies = counted(q, x, stat_id=stat_id)
    assert (n, copies) == (0, 0) and y.dtype == x.dtype and y.shape == x.shape and y.is_contiguous()
    assert len(log.rows) == 1 and log.rows[0][0] == 'act.entropy' and log.rows[0][2] == 'avg.entropy.act' and log.rows[0][3] == x.numel()
    if clipping == 'no' or stat_id is not None:
        assert same(y, y0) and log.rows[0][1] == e0, (log.rows[0][1], e0)
    else:
        y_op, e_op = ops.aciq_qdq_half(x, 4, clip='laplace', want_entropy=True)
        assert same(y, y_op) and log.rows[0][1] == float(e_op)
    y_nat, e_nat = y, log.rows[0][1]
    # the object's flag off again, the switch, a class of layer the route function sends back: the counter moves as before
    q.half_entropy = False
    yu, n, _ = counted(q, x, stat_id=stat_id)
    assert n == 1 and same(yu, y0)
    q.half_entropy = True
    monkeypatch.setenv('CNNQ_HALF_ENTROPY', '0')
    ops.reload_switches()
    try:
        yu, n, _ = counted(q, x, stat_id=stat_id)
        assert n == 1 and same(yu, y0)
    finally:
        monkeypatch.delenv('CNNQ_HALF_ENTROPY')
        ops.reload_switches()
    monkeypatch.setattr(ops, '_entropy_half_native', lambda *a: 0)
    yu, n, _ = counted(q, x, stat_id=stat_id)
    monkeypatch.undo()
    assert n == 1 and same(yu, y0)
    del log.rows[:]
    y, n, _ = counted(q, x, stat_id=stat_id)
    assert n == 0 and same(y, y_nat) and log.rows[0][1] == e_nat
    # inside an entropy_batch block the logger is called at its end, with the same value
    del log.rows[:]
    with ops.entropy_batch():
        y, n, _ = counted(q, x, stat_id=stat_id)
        assert n == 0 and not log.rows
    assert same(y, y_nat) and len(log.rows) == 1 and log.rows[0][1] == e_nat


def test_what_stays_on_its_route():
    """A pending correction, bit allocation without clipping, replicated data and a float32 tensor keep their routes with the opt-in
    set: the same upcast count and the same bits as without it."""
    x = HC.values((8, 32, 14, 14), seed=8).to(torch.bfloat16).cuda()
    SM = calibration(x)

    def both(t=x, stat_id=None, pending=None, group=None, **kw):
        out = []
        for opt in (False, True):
            q = Q.quantizer(**dict(dict(pcq_act=True, measure_entropy=True, logger=Logger()), **kw))
            q.sm, q.half_entropy, q.group = SM, opt, group
            q.fuse_bcorr, q.bcorr_fused = pending, False
            out.append(counted(q, t, stat_id=stat_id))
        (y0, n0, c0), (y1, n1, c1) = out
        assert (n0, c0) == (n1, c1) and same(y0, y1) and y1.dtype == t.dtype
        return n1

    assert both(pending=True) == 1 and both(pending=True, clipping='laplace') == 1
    assert both(bit_alloc_act=True) == 1
    assert both(group=False) == 1 and both(group=False, clipping='gaus') == 1
    assert both(x.float()) == 0 and both(x.float(), clipping='laplace') == 0


# ---- 7. one full-size layer, once on each route
def test_full_size_layer():
    _, ops = mods()
    x = case_input(((512, 256, 14, 14), 0, None), torch.bfloat16)
    assert route(x, 16, 2)[3] == 1 and route(x, 16, 0)[3] == 2 and route(x, 16, 0)[1] > 1
    y0, qp0, mm0 = auto_dt(x, 4, True)
    h_ref = None
    for allow in (0, 2):
        y, qp, mm, rep = minmax_pass(x, 4, True, allow)
        assert same(qp, qp0) and same(mm, mm0) and same(y, y0)
        assert int(rep.sum()) == x.numel()
        got = fold(rep)
        if h_ref is None:
            y_ref, h_ref = f32_table(x, qp)
            assert same(y, y_ref)
        assert torch.equal(got, h_ref)
