"""`-sm collect` on contiguous bf16 / fp16 activations: ops.pc_stats_half on cnnq_pc_stats_dt.

The reference is fp64 torch on the CPU over x.float().double() (half values are exact in fp32; B and the kurtosis around the
fp32-rounded mean and std: ref64 of tests/test_channels_last_collect_gpu.py).  The tiers are those of
tests/test_stats_single_gpu.py (check_tiers of the same file): extrema bit exact with torch's NaN rule, mean 2e-6 / 1e-7, std
2e-6, b and std_pos 3e-6 / 1e-7, kurtosis 2e-4 / 2e-4 on channels whose std is not 0.  tests/test_half_collect_cpu.py shows on
the CPU that a model of the kernels' summation keeps these tiers on the inputs used here.

The shapes (tests/_half_collect.py: CASES) are the smallest that reach each branch of the plan - every piece width, uneven batch
splits, column splits of the rows, both together, a view at an odd element offset - and every test asserts the plan through
cnnq_pc_route_stats_dt, so a changed plan cannot silently stop covering a branch.

B is written whenever pass B runs - need_b or need_kurt - as cnnq_pc_stats writes it; every other row nobody asked for is zero."""
import ctypes
import importlib

import numpy as np
import pytest
import torch

import _half_collect as HC
from test_channels_last_collect_gpu import check_tiers, ref64, same

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]
IDS = ['bf16', 'f16']
ALL = (True, True, True)


def mods():
    from cnn_quantization_amd import _lib as L, ops
    return L, ops


def counters():
    _, ops = mods()
    return ops.LAYOUT_COPIES, importlib.import_module('cnn_quantization_amd.qtypes.int_quantizer').HALF_FALLBACKS


def half(x, dtype, offset=0):
    """x as a contiguous tensor of dtype on the GPU, `offset` elements into a larger buffer."""
    base = torch.zeros(x.numel() + offset + 8, dtype=dtype, device='cuda')
    v = base[offset:offset + x.numel()].view(x.shape)
    v.copy_(x.to(dtype).cuda())
    assert v.is_contiguous() and v.storage_offset() == offset
    return v


def route(x):
    L, ops = mods()
    out = (ctypes.c_int32 * 4)()
    N, C, HW = ops.geometry(x)
    align = (x.data_ptr() | 16) & -(x.data_ptr() | 16)
    assert L.load().cnnq_pc_route_stats_dt(N, C, HW, ops._DTYPE_CODES[x.dtype], align, out) == 0
    return tuple(out)


def case_input(case, dtype):
    shape, offset, want = case
    x = half(HC.values(shape, HC.seed_of(shape, offset)), dtype, offset)
    assert route(x) == want + (HC.native(shape[0], shape[2] * shape[3]),), (shape, offset, route(x))
    return x


# ---- 1. every branch of the plan against fp64
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('case', HC.CASES, ids=HC.IDS)
def test_every_branch_against_fp64(case, dtype):
    L, ops = mods()
    x = case_input(case, dtype)
    N, C, HW = ops.geometry(x)
    before = counters()
    st, mom = ops.pc_stats_half(x, *ALL)
    assert counters() == before
    assert st.shape == (L.NSTAT, C) and st.dtype == torch.float32 and mom.shape == (L.NMOM, C) and mom.dtype == torch.float64
    check_tiers(st, ref64(x))
    assert torch.equal(mom[L.MOM_COUNT].cpu(), torch.full((C,), float(N * HW), dtype=torch.float64))
    t = x.cpu().double().transpose(0, 1).reshape(C, -1)
    np.testing.assert_allclose(mom[L.MOM_SUM].cpu(), t.sum(1), rtol=1e-7, atol=1e-3)
    np.testing.assert_allclose(mom[L.MOM_SUMSQ_RELU].cpu(), (t.clamp(min=0) ** 2).sum(1), rtol=1e-7, atol=1e-6)


# ---- 1b. the extrema's partials (k_h_minmax) on the same partition: batch splits, column splits, every piece width
def minmax_plan(N, HW, W, G):
    """(batch splits, column splits) of the extrema launch, h_minmax of csrc/cnnq_kernels.hip restated: ~H_MM_ELEMS elements per
    workgroup and at most the fp32 plan's G records per channel; batch splits first, then at most HW / W parts of a row."""
    total = max(1, min(-(-N * HW // HC.H_MM_ELEMS), N * HW, G))
    S = min(total, N)
    return S, min(total // S, HW // W)


def minmax_local(x):
    """([2, C] = {min, max} per channel, which records of pmm hold no NaN) through cnnq_pc_minmax_local_dt; pmm is sized by the
    fp32 plan's record count, as ops.tensor_row_stats sizes it, and filled with NaN first: a clean input writes none."""
    L, ops = mods()
    N, C, HW = ops.geometry(x)
    pmm = torch.full((ops._groups(N, C, HW, None), 2, C), float('nan'), dtype=torch.float32, device=x.device)
    local = torch.empty((2, C), dtype=torch.float32, device=x.device)
    torch.cuda.synchronize()
    L.check(L.load().cnnq_pc_minmax_local_dt(x.data_ptr(), ops._DTYPE_CODES[x.dtype], N, C, HW, pmm.data_ptr(), local.data_ptr(),
                                             None), 'cnnq_pc_minmax_local_dt')
    torch.cuda.synchronize()
    return local.cpu(), (~torch.isnan(pmm)).all(2).all(1).cpu().tolist()


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('case', HC.CASES, ids=HC.IDS)
def test_minmax_partials_on_every_branch(case, dtype):
    _, ops = mods()
    x = case_input(case, dtype)
    N, C, HW = ops.geometry(x)
    W, S, cs = case[2]
    # the extrema launch has a plan of its own; on these cases it cuts as the statistics launches do, so the branch the case
    # is named for is the branch k_h_minmax takes - restated here, and read back from the records the launch wrote
    G = ops._groups(N, C, HW, None)
    assert minmax_plan(N, HW, W, G) == (S, cs) and S * cs < G
    clean, written = minmax_local(x)
    assert written == [True] * (S * cs) + [False] * (G - S * cs)
    xf = x.float().cpu()
    assert torch.equal(clean[0], xf.amin((0, 2, 3))) and torch.equal(clean[1], xf.amax((0, 2, 3)))
    # a NaN in one channel: both of its entries NaN, no other entry changed
    c = C // 2
    x[-1, c, -1, -1] = float('nan')
    got, _ = minmax_local(x)
    assert torch.isnan(got[:, c]).all()
    keep = [i for i in range(C) if i != c]
    assert torch.equal(got[:, keep], clean[:, keep])


# ---- 2. against the existing route: the upcast and the fp32 chain
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('case', HC.CASES, ids=HC.IDS)
def test_against_the_upcast_route(case, dtype):
    L, ops = mods()
    x = case_input(case, dtype)
    N, C, HW = ops.geometry(x)
    st, mom = ops.pc_stats_half(x, *ALL)
    st0, mom0 = ops.pc_stats(x.float(), N, C, HW, need_b=True, need_kurt=True, need_relu=True)
    assert same(mom[L.MOM_COUNT], mom0[L.MOM_COUNT])
    st, st0 = st.cpu(), st0.cpu()
    assert same(st[[L.STAT_MIN, L.STAT_MAX]], st0[[L.STAT_MIN, L.STAT_MAX]])
    rows = [r for r in range(L.NSTAT) if r != L.STAT_KURT]
    np.testing.assert_allclose(st[rows], st0[rows], rtol=2e-6, atol=2e-6)
    np.testing.assert_allclose(st[L.STAT_KURT], st0[L.STAT_KURT], rtol=2e-5, atol=2e-5)


# ---- 3. flag subsets
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('case', [HC.CASES[1], HC.CASES[2], HC.CASES[4]], ids=[HC.IDS[1], HC.IDS[2], HC.IDS[4]])
def test_flag_subsets(case, dtype):
    L, ops = mods()
    x = case_input(case, dtype)
    full, mom_full = ops.pc_stats_half(x, *ALL)
    ref = ref64(x)
    for bits in range(8):
        need = (bool(bits & 1), bool(bits & 2), bool(bits & 4))
        st, mom = ops.pc_stats_half(x, *need)
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


# ---- 4. special values: the case of the channels_last test, on single elements (7x7) and on 16-byte pieces (8x8)
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('hw, w', [(7, 1), (8, 8)], ids=['W1', 'W8'])
def test_special_values(hw, w, dtype):
    L, ops = mods()
    x = HC.values((2, 7, hw, hw), seed=9)
    x[1, 0, 2, 3] = float('nan')
    x[0, 1, 0, 0] = float('inf')
    x[1, 2, 1, 1] = float('-inf')
    x[:, 3] = 0.25                                          # constant: std 0, kurtosis 0 / 0
    x[:, 4] = -x[:, 4].abs() - 0.125                        # all negative: std_pos from zero rectified sums
    finite = [3, 4, 5, 6]
    xh = half(x, dtype)
    assert route(xh)[0] == w
    st, mom = ops.pc_stats_half(xh, *ALL)
    st0, _ = ops.pc_stats(xh.float(), 2, 7, hw * hw, need_b=True, need_kurt=True, need_relu=True)
    st, st0 = st.cpu(), st0.cpu()
    for row in range(L.NSTAT):
        skip = [3] if row == L.STAT_KURT else []           # (the constant channel's kurtosis is outside the contract)
        keep = [c for c in range(7) if c not in skip]
        assert torch.equal(torch.isnan(st[row][keep]), torch.isnan(st0[row][keep])), row
        assert torch.equal(torch.isinf(st[row][keep]), torch.isinf(st0[row][keep])), row
    assert torch.isnan(st[[L.STAT_MIN, L.STAT_MAX, L.STAT_MEAN], 0]).all()
    assert st[L.STAT_MAX, 1] == float('inf') and st[L.STAT_MIN, 2] == float('-inf')
    assert st[L.STAT_STD_POS, 4] == 0 and st[L.STAT_STD, 3] == 0
    assert torch.equal(mom[L.MOM_COUNT].cpu(), torch.full((7,), 2. * hw * hw, dtype=torch.float64))
    check_tiers(st, ref64(xh), chans=finite)


# ---- 5. determinism, graph capture, refusals
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_two_runs_give_the_same_bits(dtype):
    _, ops = mods()
    for case in (HC.CASES[1], HC.CASES[5], HC.CASES[7], HC.CASES[8]):
        x = case_input(case, dtype)
        st1, mom1 = ops.pc_stats_half(x, *ALL)
        st1, mom1 = st1.clone(), mom1.clone()
        ops.act_qdq_per_channel(x, 4)                       # (another user of the device in between)
        ops.pc_stats_half(half(HC.values((3, 5, 14, 14), 21), dtype), *ALL)      # (and of the workspace)
        st2, mom2 = ops.pc_stats_half(x, *ALL)
        assert same(st1, st2) and same(mom1, mom2)


def test_graph_capture_replays_eager():
    _, ops = mods()
    shape = (5, 6, 80, 80)
    x = half(HC.values(shape, seed=2), torch.bfloat16)
    eager = ops.pc_stats_half(x, *ALL)[0].clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.pc_stats_half(x, *ALL)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        st, mom = ops.pc_stats_half(x, *ALL)
    graph.replay()
    torch.cuda.synchronize()
    assert same(st, eager)
    x.copy_(half(HC.values(shape, seed=3), torch.bfloat16))
    graph.replay()
    torch.cuda.synchronize()
    assert not same(st, eager) and same(st, ops.pc_stats_half(x, *ALL)[0])


def test_refusals():
    L, ops = mods()
    x = half(HC.values((2, 4, 7, 8)), torch.bfloat16)
    before = counters()
    for bad in (x.float(),                                                       # float32 takes pc_stats
                x.cpu(),                                                         # there is no CPU path
                x[0],                                                            # not 4-D
                x.to(memory_format=torch.channels_last),                         # not contiguous: dense channels_last
                x[:, 1:3],                                                       # not contiguous: not dense
                x.double(), None):
        with pytest.raises(L.CnnqError):
            ops.pc_stats_half(bad, *ALL)
    assert counters() == before
    p, lib = x.data_ptr(), L.load()
    ws = torch.empty(lib.cnnq_pc_stats_dt_workspace(2, 4, 56, 1) + 8, dtype=torch.uint8, device='cuda')
    st = torch.empty(L.NSTAT, 4, device='cuda')
    assert lib.cnnq_pc_stats_dt(p, 1, 2, 4, 56, 1, 1, 1, ws.data_ptr() + 4, None, st.data_ptr(), None) == -1      # CNNQ_EINVAL
    assert lib.cnnq_pc_stats_dt(p, 1, 2, 4, 56, 1, 1, 1, ws.data_ptr(), None, st.data_ptr(), None) == 0      # mom may be NULL
    torch.cuda.synchronize()
    assert same(st, ops.pc_stats_half(x, *ALL)[0])
    # float32 through the same entry point: cnnq_pc_stats' table
    xf = x.float()
    ws = torch.empty(lib.cnnq_pc_stats_dt_workspace(2, 4, 56, 0), dtype=torch.uint8, device='cuda')
    assert lib.cnnq_pc_stats_dt(xf.data_ptr(), 0, 2, 4, 56, 1, 1, 1, ws.data_ptr(), None, st.data_ptr(), None) == 0
    torch.cuda.synchronize()
    ws0 = torch.empty_like(ws)
    st0 = torch.empty_like(st)
    assert lib.cnnq_pc_stats(xf.data_ptr(), 2, 4, 56, 1, 1, 1, ws0.data_ptr(), None, st0.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert same(st, st0)
