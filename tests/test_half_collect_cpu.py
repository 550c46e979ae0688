"""CPU-only checks of `-sm collect` on contiguous bf16 / fp16 activations: the three entry points exist
and their ctypes prototypes match the header, bad arguments are refused before anything touches the device, the workspace covers
the documented records, the route function over a grid of (N, C, HW, dtype, alignment) with the plan enumerated in Python, the
manager's routing predicate as a truth table - and that a torch model of the kernels' summation keeps the tiers of
tests/test_half_collect_gpu.py on that file's inputs (were it not so, the inputs would be wrong, not the tiers)."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _half_collect as HC
from _quantizer import FakeCuda, act
from test_channels_last_collect_cpu import ctype_of, header_decls

FUNCS = ['cnnq_pc_stats_dt_workspace', 'cnnq_pc_route_stats_dt', 'cnnq_pc_stats_dt']
BAD = 0x1000   # a non-null pointer value that is never dereferenced: the argument checks come first
EINVAL, ERANGE = -1, -2


def lib():
    from cnn_quantization_amd import _lib as L
    return L.load()


def test_entry_points_exist_and_prototypes_match_header():
    from cnn_quantization_amd import _lib as L
    decls = header_decls()
    for name in FUNCS:
        assert hasattr(lib(), name), name
        ret, args = decls[name]
        res, argtypes = L.SIGNATURES[name]
        assert res is {'int': ctypes.c_int, 'size_t': ctypes.c_size_t}[ret], name
        assert len(args) == len(argtypes), name
        for a, t in zip(args, argtypes):
            want = ctype_of(a)
            if want == 'ptr':
                assert t is ctypes.c_void_p or issubclass(t, ctypes._Pointer), (name, a, t)
            else:
                assert t is want, (name, a, t)


def stats_args(dtype=1, N=2, C=8, HW=16):
    p = ctypes.c_void_p(BAD)
    return [p, dtype, N, C, HW, 1, 1, 1, p, p, p, None]     # x, dtype, N, C, HW, need_b, need_kurt, need_relu, ws, mom, stats, stream


@pytest.mark.parametrize('dtype, N, C, HW', [(-1, 2, 8, 16), (3, 2, 8, 16), (1 << 20, 2, 8, 16), (1, 0, 8, 16), (2, 2, 0, 16),
                                             (1, 2, 8, 0), (0, -3, 8, 16), (2, 2, -1, 16), (1, 2, 8, -5)])
def test_bad_geometry_is_einval(dtype, N, C, HW):
    out = (ctypes.c_int32 * 4)()
    assert lib().cnnq_pc_stats_dt_workspace(N, C, HW, dtype) == 0
    assert lib().cnnq_pc_route_stats_dt(N, C, HW, dtype, 16, out) == EINVAL
    assert lib().cnnq_pc_stats_dt(*stats_args(dtype, N, C, HW)) == EINVAL


@pytest.mark.parametrize('dtype', [0, 1, 2])
def test_bad_pointers_are_einval_and_geometries_beyond_the_plan_keep_its_code(dtype):
    for i in (0, 8, 10):                                    # x, ws, stats
        a = stats_args(dtype)
        a[i] = None
        assert lib().cnnq_pc_stats_dt(*a) == EINVAL, i
    for i in (8, 9):                                        # ws and mom hold doubles
        a = stats_args(dtype)
        a[i] = ctypes.c_void_p(BAD + 4)
        assert lib().cnnq_pc_stats_dt(*a) == EINVAL, i
    if dtype:
        a = stats_args(dtype)
        a[0] = ctypes.c_void_p(BAD + 1)                     # x not aligned to its element
        assert lib().cnnq_pc_stats_dt(*a) == EINVAL
    out = (ctypes.c_int32 * 4)()
    assert lib().cnnq_pc_route_stats_dt(2, 8, 16, dtype, 3, out) == EINVAL
    assert lib().cnnq_pc_route_stats_dt(2, 8, 16, dtype, 0, out) == EINVAL
    assert lib().cnnq_pc_route_stats_dt(2, 8, 16, dtype, 16, None) == EINVAL
    # cnnq_pc_groups' limits: a sample of 2^31 elements, 2^31 samples
    for N, C, HW in ((2, 1 << 16, 1 << 15), (1 << 31, 2, 4)):
        assert lib().cnnq_pc_groups(N, C, HW, 0) == ERANGE
        assert lib().cnnq_pc_stats_dt_workspace(N, C, HW, dtype) == 0
        assert lib().cnnq_pc_route_stats_dt(N, C, HW, dtype, 16, out) == ERANGE
        assert lib().cnnq_pc_stats_dt(*stats_args(dtype, N, C, HW)) == ERANGE


GRID = [(N, C, HW) for N in (1, 2, 3, 5, 8, 64, 512) for C in (1, 3, 64, 520, 2048)
        for HW in (1, 2, 7, 49, 98, 196, 784, 3136, 6400, 12544, 50176)]


@pytest.mark.parametrize('dtype', [1, 2])
@pytest.mark.parametrize('align', [2, 4, 8, 16, 64])
def test_route_and_workspace_over_a_grid(dtype, align):
    out = (ctypes.c_int32 * 4)()
    for N, C, HW in GRID:
        assert lib().cnnq_pc_route_stats_dt(N, C, HW, dtype, align, out) == 0, (N, C, HW)
        w, S, cs, native = out
        assert w == HC.piece(HW, align), (N, C, HW, align, w)
        assert (S, cs) == HC.splits(N, C, HW), (N, C, HW, S, cs)
        assert 1 <= S <= N and 1 <= cs <= HW // w and S * cs <= HC.H_ST_MAX_RECORDS and C * S * cs < 1 << 31
        assert native == HC.native(N, HW), (N, C, HW, native)
        # ws, doubles: part[G][NMOM][C], mom[NMOM][C], part2[G][NDEV][C] with G = S * cs, whatever the alignment
        ws = lib().cnnq_pc_stats_dt_workspace(N, C, HW, dtype)
        assert ws == (S * cs * (HC.NMOM + HC.NDEV) + HC.NMOM) * C * 8, (N, C, HW, ws)


@pytest.mark.parametrize('align', [2, 4, 16])
def test_the_plan_covers_every_sample_and_piece_once(align):
    out = (ctypes.c_int32 * 4)()
    shapes = [(s[0], s[2] * s[3]) for s, _, _ in HC.CASES] + [(N, HW) for N in (1, 2, 3, 7, 33) for HW in (7, 49, 196, 784, 12544, 50176)]
    for N, HW in shapes:
        assert lib().cnnq_pc_route_stats_dt(N, 4, HW, 1, align, out) == 0
        w, S, cs, _ = out
        seen = np.zeros((N, HW // w), dtype=np.int32)
        for samples, pieces in HC.owners(N, HW, w, S, cs):
            assert len(samples) >= 1 and len(pieces) >= 1, (N, HW, w, S, cs)
            seen[samples.start:samples.stop, pieces.start:pieces.stop] += 1
        assert (seen == 1).all(), (N, HW, w, S, cs)


def test_the_gpu_tests_cases_reach_their_branches():
    out = (ctypes.c_int32 * 4)()
    for shape, offset, want in HC.CASES:
        N, C, HW = shape[0], shape[1], shape[2] * shape[3]
        align = 2 if offset % 2 else 16
        assert lib().cnnq_pc_route_stats_dt(N, C, HW, 1, align, out) == 0
        assert tuple(out) == want + (HC.native(N, HW),), (shape, offset, tuple(out))


def test_float32_forwards_to_the_chain():
    out = (ctypes.c_int32 * 4)()
    for N, C, HW in ((8, 12, 784), (3, 10, 196), (2, 64, 49)):
        for align in (4, 16):
            assert lib().cnnq_pc_route_stats_dt(N, C, HW, 0, align, out) == 0
            assert list(out) == [0, lib().cnnq_pc_groups(N, C, HW, int(align >= 16)), 1, 1]
        assert lib().cnnq_pc_stats_dt_workspace(N, C, HW, 0) == max(lib().cnnq_pc_stats_workspace(N, C, HW, a) for a in (0, 1))


# ---- the manager's predicate
class FakeManager:
    def __init__(self, batch_avg=False, collect_err=False, group=None):
        self.batch_avg, self.collect_err, self.group = batch_avg, collect_err, group


def test_predicate_truth_table(monkeypatch):
    from cnn_quantization_amd import distributed as D, ops
    from cnn_quantization_amd.inference.statistic_manager_perchannel import collects_native_half as native
    x = act()
    for dtype in (torch.bfloat16, torch.float16):
        assert native(FakeManager(), act(dtype))
    # the tensor
    assert not native(FakeManager(), torch.zeros(2, 8, 4, 4, dtype=torch.bfloat16))             # on the CPU
    assert not native(FakeManager(), act(torch.float32)) and not native(FakeManager(), act(torch.float64))
    assert not native(FakeManager(), FakeCuda(torch.zeros(2, 8, 4, 4, dtype=torch.bfloat16).to(memory_format=torch.channels_last)))
    assert not native(FakeManager(), FakeCuda(torch.zeros(2, 12, 4, 4, dtype=torch.bfloat16)[:, 2:9]))   # not dense
    assert not native(FakeManager(), act(shape=(2, 8, 1, 1)))                                   # no spatial extent
    assert not native(FakeManager(), act(shape=(8, 16))) and not native(FakeManager(), act(shape=(2, 8, 16)))
    assert not native(FakeManager(), act(shape=(0, 8, 4, 4))) and not native(FakeManager(), None)
    assert native(FakeManager(), act(shape=(2, 8, 1, 7)))
    assert not native(FakeManager(), act(shape=(512, 8, 7, 7)))                                 # a class the route function sends back
    assert native(FakeManager(), act(shape=(4, 8, 7, 7)))
    # the manager's settings
    for batch_avg in (False, True):
        for collect_err in (False, True):
            for force in (False, True):
                want = not collect_err and (not batch_avg or force)
                assert native(FakeManager(batch_avg, collect_err), x, force) == want, (batch_avg, collect_err, force)
    # more than one process, or the forced exchange
    monkeypatch.setattr(D, 'world_size', lambda group=None: 2)
    assert not native(FakeManager(), x)
    monkeypatch.undo()
    monkeypatch.setattr(D, 'forced_exchange', lambda: True)
    assert not native(FakeManager(), x)
    monkeypatch.undo()
    assert native(FakeManager(), x)
    # a class of layer the route function sends back
    monkeypatch.setattr(ops, '_stats_half_native', lambda N, C, HW, dtype: False)
    assert not native(FakeManager(), x)
    monkeypatch.undo()
    assert native(FakeManager(), x)


def test_route_is_asked_once_per_class(monkeypatch):
    from cnn_quantization_amd import ops
    asked = []
    real = lib().cnnq_pc_route_stats_dt

    class Lib:
        def cnnq_pc_route_stats_dt(self, *a):
            asked.append(a[:4])
            return real(*a)
    monkeypatch.setattr(ops.L, 'load', lambda: Lib())
    monkeypatch.setattr(ops, '_STATS_HALF_NATIVE', {})
    for _ in range(3):
        assert ops._stats_half_native(2, 12, 49, torch.bfloat16) and ops._stats_half_native(2, 12, 49, torch.float16)
    assert asked == [(2, 12, 49, 1), (2, 12, 49, 2)]


def test_op_refuses_what_it_does_not_take():
    from cnn_quantization_amd import _lib as L, ops
    with pytest.raises(L.CnnqError):
        ops.pc_stats_half(torch.zeros(2, 8, 4, 4, dtype=torch.bfloat16))           # a CPU tensor: there is no CPU path
    with pytest.raises(L.CnnqError):
        ops.pc_stats_half(None)


# ---- the inputs of the GPU tests hold the tiers under the model of the kernels' summation
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'f16'])
@pytest.mark.parametrize('case', HC.CASES, ids=HC.IDS)
def test_model_of_the_summation_keeps_the_tiers_on_the_gpu_tests_inputs(case, dtype):
    shape, offset, (W, _, _) = case
    x = HC.values(shape, HC.seed_of(shape, offset)).to(dtype).float()
    mean, std, b, kurt, std_pos = HC.model(x, W)
    C = shape[1]
    t64 = x.double().transpose(0, 1).reshape(C, -1)
    m64, s64 = t64.mean(1), t64.std(1, unbiased=True)
    m32, s32 = m64.float().double(), s64.float().double()
    b64, p64 = (t64 - m32[:, None]).abs().mean(1), t64.clamp(min=0).std(1, unbiased=True)
    rel = lambda a, r: float(((a.double() - r).abs() / r.abs().clamp(min=1e-30)).max())
    print('max relative error', dict(mean=rel(mean, m64), std=rel(std, s64), b=rel(b, b64), std_pos=rel(std_pos, p64)))
    np.testing.assert_allclose(mean.double(), m64, rtol=2e-6, atol=1e-7)
    np.testing.assert_allclose(std.double(), s64, rtol=2e-6)
    np.testing.assert_allclose(b.double(), b64, rtol=3e-6, atol=1e-7)
    np.testing.assert_allclose(std_pos.double(), p64, rtol=3e-6, atol=1e-7)
    np.testing.assert_allclose(kurt.double(), (((t64 - m32[:, None]) / s32[:, None]) ** 4).mean(1) - 3, rtol=2e-4, atol=2e-4)
