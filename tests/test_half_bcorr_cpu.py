"""CPU-only checks of the table-driven Q/DQ with the activation bias correction on contiguous bf16 / fp16 activations (DESIGN.md
section 24): the three entry points exist and their ctypes prototypes match the header, bad arguments are refused before anything
touches the device, the workspace covers the documented records, the route function over a grid of (N, C, HW, dtype, alignment,
allow) with the plan enumerated in Python, the fp32 forward, and the quantizer's routing predicate as a truth table - next to
_half_native's answers for the same inputs, which it must not change."""
import ctypes

import pytest
import torch

import _half_bcorr as HB
import _quantizer as Q
from test_channels_last_collect_cpu import ctype_of, header_decls
from _quantizer import FakeCuda, act

FUNCS = ['cnnq_pc_qdq_bcorr_dt_workspace', 'cnnq_pc_route_qdq_bcorr_dt', 'cnnq_pc_qdq_bcorr_dt']
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


def call_args(dtype=1, N=2, C=8, HW=16):
    p = ctypes.c_void_p
    # x, y, dtype, N, C, HW, qp, relu_first, ws, sums, bias, allow_single_launch, stream
    return [p(BAD), p(2 * BAD), dtype, N, C, HW, p(3 * BAD), 1, p(4 * BAD), p(5 * BAD), p(6 * BAD), 1, None]


@pytest.mark.parametrize('dtype, N, C, HW', [(-1, 2, 8, 16), (3, 2, 8, 16), (1 << 20, 2, 8, 16), (1, 0, 8, 16), (2, 2, 0, 16),
                                             (1, 2, 8, 0), (0, -3, 8, 16), (2, 2, -1, 16), (1, 2, 8, -5)])
def test_bad_geometry_is_einval(dtype, N, C, HW):
    out = (ctypes.c_int32 * 4)()
    assert lib().cnnq_pc_qdq_bcorr_dt_workspace(N, C, HW, dtype) == 0
    assert lib().cnnq_pc_route_qdq_bcorr_dt(N, C, HW, dtype, 16, 1, out) == EINVAL
    assert lib().cnnq_pc_qdq_bcorr_dt(*call_args(dtype, N, C, HW)) == EINVAL


@pytest.mark.parametrize('dtype', [0, 1, 2])
def test_bad_pointers_are_einval_and_geometries_beyond_the_plan_keep_its_code(dtype):
    for i in (0, 1, 6, 8, 10):                              # x, y, qp, ws, bias
        a = call_args(dtype)
        a[i] = None
        assert lib().cnnq_pc_qdq_bcorr_dt(*a) == EINVAL, i
    for i in (8, 9):                                        # ws and sums hold doubles
        a = call_args(dtype)
        a[i] = ctypes.c_void_p(BAD + 4)
        assert lib().cnnq_pc_qdq_bcorr_dt(*a) == EINVAL, i
    for i in (0, 1, 6, 10):                                 # x and y not aligned to their element, the fp32 tables to theirs
        a = call_args(dtype)
        a[i] = ctypes.c_void_p(BAD + (2 if dtype == 0 or i in (6, 10) else 1))
        assert lib().cnnq_pc_qdq_bcorr_dt(*a) == EINVAL, i
    a = call_args(dtype)
    a[1] = a[0]                                             # in place
    assert lib().cnnq_pc_qdq_bcorr_dt(*a) == EINVAL
    out = (ctypes.c_int32 * 4)()
    assert lib().cnnq_pc_route_qdq_bcorr_dt(2, 8, 16, dtype, 3, 1, out) == EINVAL
    assert lib().cnnq_pc_route_qdq_bcorr_dt(2, 8, 16, dtype, 0, 1, out) == EINVAL
    assert lib().cnnq_pc_route_qdq_bcorr_dt(2, 8, 16, dtype, 16, 1, None) == EINVAL
    # cnnq_pc_groups' limits: a sample of 2^31 elements, 2^31 samples
    for N, C, HW in ((2, 1 << 16, 1 << 15), (1 << 31, 2, 4)):
        assert lib().cnnq_pc_groups(N, C, HW, 0) == ERANGE
        assert lib().cnnq_pc_qdq_bcorr_dt_workspace(N, C, HW, dtype) == 0
        assert lib().cnnq_pc_route_qdq_bcorr_dt(N, C, HW, dtype, 16, 1, out) == ERANGE
        assert lib().cnnq_pc_qdq_bcorr_dt(*call_args(dtype, N, C, HW)) == ERANGE


GRID = [(N, C, HW) for N in (1, 2, 3, 5, 8, 64, 512) for C in (1, 3, 64, 256, 520, 2048)
        for HW in (1, 2, 7, 49, 98, 196, 784, 3136, 6400, 12544, 50176)]


@pytest.mark.parametrize('dtype', [1, 2])
@pytest.mark.parametrize('align', [2, 4, 8, 16, 64])
def test_route_and_workspace_over_a_grid(dtype, align):
    out = (ctypes.c_int32 * 4)()
    for N, C, HW in GRID:
        for allow in (0, 1, 2):
            assert lib().cnnq_pc_route_qdq_bcorr_dt(N, C, HW, dtype, align, allow, out) == 0, (N, C, HW)
            assert tuple(out) == HB.route(N, C, HW, align, allow), (N, C, HW, align, allow, tuple(out))
            again = (ctypes.c_int32 * 4)()                   # a function of its arguments alone
            assert lib().cnnq_pc_route_qdq_bcorr_dt(N, C, HW, dtype, align, allow, again) == 0 and tuple(again) == tuple(out)
        w, S, cs, _ = out
        assert 1 <= S <= N and 1 <= cs <= max(1, HW // 8) and C * S * cs < 1 << 31
        if out[3] == 1:
            assert allow and w >= 2 and N * HW <= HB.WHOLE_CAP
        # ws, doubles: part3[G][3][C] with G = S * cs, whatever the alignment and the route
        assert lib().cnnq_pc_qdq_bcorr_dt_workspace(N, C, HW, dtype) == S * cs * 3 * C * 8, (N, C, HW)


def test_the_gpu_tests_cases_reach_their_branches():
    out = (ctypes.c_int32 * 4)()
    for shape, offset, (W, S, cs, fits) in HB.CASES:
        N, C, HW = shape[0], shape[1], shape[2] * shape[3]
        align = (2 * offset) & -(2 * offset) if offset else 16
        for dtype in (1, 2):
            assert lib().cnnq_pc_route_qdq_bcorr_dt(N, C, HW, dtype, align, 2, out) == 0
            assert tuple(out) == (W, S, cs, 1 if fits else 2), (shape, offset, tuple(out))
            assert lib().cnnq_pc_route_qdq_bcorr_dt(N, C, HW, dtype, align, 0, out) == 0
            assert tuple(out) == (W, S, cs, 2), (shape, offset, tuple(out))
    # one sample beyond the resident capacity: two passes whatever the caller allows
    for allow in (1, 2):
        assert lib().cnnq_pc_route_qdq_bcorr_dt(65, 1, 2048, 1, 16, allow, out) == 0 and out[3] == 2
        assert lib().cnnq_pc_route_qdq_bcorr_dt(64, 1, 2048, 1, 16, allow, out) == 0 and out[3] == HB.route(64, 1, 2048, 16, allow)[3]


def test_float32_forwards_to_the_chain():
    out = (ctypes.c_int32 * 4)()
    for N, C, HW in ((8, 12, 784), (3, 10, 196), (2, 64, 49)):
        G = max(lib().cnnq_pc_groups(N, C, HW, a) for a in (0, 1))
        for align in (4, 16):
            for allow in (0, 1, 2):
                assert lib().cnnq_pc_route_qdq_bcorr_dt(N, C, HW, 0, align, allow, out) == 0
                assert list(out) == [0, G, 1, 2]
        assert lib().cnnq_pc_qdq_bcorr_dt_workspace(N, C, HW, 0) == G * 3 * C * 8


# ---- the quantizer's predicate
def quantizer(**kw):
    return Q.quantizer(**dict(dict(clipping='laplace', pcq_act=True, bit_alloc_act=True, bcorr_act=True), **kw))


def test_predicate_truth_table(monkeypatch):
    from cnn_quantization_amd import distributed as D, ops
    x = act()

    def table(q, t=x, stat_id='layer0', override=None):
        att = q._att(override)
        return q._half_table(t, att('clipping'), stat_id, att)

    # the attributes: every combination, with and without a pending correction and stat_id
    for clipping in ('no', 'laplace', 'gaus', 'mix', '2std'):
        for ba in (False, True):
            for flags in range(32):
                pcq_a, pcq_w, mtd, kld, me = (bool(flags >> i & 1) for i in range(5))
                for pending in (None, True):
                    for stat_id in (None, 'layer0'):
                        q = quantizer(clipping=clipping, bit_alloc_act=ba, pcq_act=pcq_a, pcq_weights=pcq_w, mtd_quant=mtd, kld=kld,
                                      measure_entropy=me)
                        q.fuse_bcorr = pending
                        want = (stat_id is not None and pcq_a and clipping in ('no', 'laplace', 'gaus')
                                and not (clipping == 'no' and pcq_w) and not mtd and not kld and not me)
                        assert table(q, stat_id=stat_id) == want, (clipping, ba, flags, pending, stat_id)
                        # _half_native's answer for a contiguous half tensor is what it was
                        if kld:
                            old = False
                        elif clipping != 'no' or pcq_w:
                            old = False
                        elif pcq_a:
                            old = not mtd and not me and pending is None and not ba
                        else:
                            old = True
                        assert q._half_native(x, None, stat_id) == old, (clipping, ba, flags, pending, stat_id)
    q = quantizer()
    # __call__'s override pair wins over the attribute
    assert not table(q, override=('clipping', 'mix')) and not table(q, override=('mtd_quant', True))
    assert table(quantizer(clipping='mix'), override=('clipping', 'gaus'))
    # the tensor
    for dtype in (torch.bfloat16, torch.float16):
        assert table(q, act(dtype))
    assert not table(q, torch.zeros(2, 8, 4, 4, dtype=torch.bfloat16))                          # on the CPU
    assert not table(q, act(torch.float32)) and not table(q, act(torch.float64))
    assert not table(q, FakeCuda(torch.zeros(2, 8, 4, 4, dtype=torch.bfloat16).to(memory_format=torch.channels_last)))
    assert not table(q, FakeCuda(torch.zeros(2, 12, 4, 4, dtype=torch.bfloat16)[:, 2:9]))       # not dense
    assert not table(q, act(shape=(2, 8, 1, 1)))                                                # no spatial extent
    assert not table(q, act(shape=(8, 16))) and not table(q, act(shape=(2, 8, 16)))
    assert not table(q, act(shape=(0, 8, 4, 4)))
    assert table(q, act(shape=(2, 8, 1, 7))) and table(q, act(shape=(4, 8, 7, 7)))
    # replicated data, more than one process, the forced exchange
    q.group = False
    assert not table(q)
    q.group = None
    monkeypatch.setattr(D, 'world_size', lambda group=None: 2)
    assert not table(q)
    monkeypatch.undo()
    monkeypatch.setattr(D, 'forced_exchange', lambda: True)
    assert not table(q)
    monkeypatch.undo()
    assert table(q)
    # a class of layer the route function sends back; the single launch and the two passes are both native
    for word, want in ((0, False), (1, True), (2, True)):
        monkeypatch.setattr(ops, '_table_half_native', lambda N, C, HW, dtype, word=word: word)
        assert table(q) == want
        monkeypatch.undo()
    # the switch
    monkeypatch.setenv('CNNQ_HALF_TABLE', '0')
    ops.reload_switches()
    try:
        assert not table(q)
    finally:
        monkeypatch.delenv('CNNQ_HALF_TABLE')
        ops.reload_switches()
    assert table(q)


def test_route_is_asked_once_per_class(monkeypatch):
    from cnn_quantization_amd import ops
    asked = []
    real = lib().cnnq_pc_route_qdq_bcorr_dt

    class Lib:
        def cnnq_pc_route_qdq_bcorr_dt(self, *a):
            asked.append(a[:6])
            return real(*a)
    monkeypatch.setattr(ops.L, 'load', lambda: Lib())
    monkeypatch.setattr(ops, '_TABLE_HALF_NATIVE', {})
    for _ in range(3):
        for dtype, code in ((torch.bfloat16, 1), (torch.float16, 2)):
            assert ops._table_half_native(2, 12, 196, dtype) == 2
            assert ops._table_half_native(512, 256, 196, dtype) == 1      # one of the classes the single launch keeps
    assert asked == [(2, 12, 196, 1, 16, 1), (512, 256, 196, 1, 16, 1), (2, 12, 196, 2, 16, 1), (512, 256, 196, 2, 16, 1)]


def test_op_refuses_what_it_does_not_take():
    from cnn_quantization_amd import _lib as L, ops
    qp = torch.zeros(3, 8)
    with pytest.raises(L.CnnqError):
        ops.qdq_bias_corrected_half(torch.zeros(2, 8, 4, 4, dtype=torch.bfloat16), qp, True)   # a CPU tensor: there is no CPU path
    with pytest.raises(L.CnnqError):
        ops.qdq_bias_corrected_half(None, qp, True)
    for bad in (act(torch.float32), act(shape=(2, 8, 16)), act(shape=(0, 8, 4, 4)),
                FakeCuda(torch.zeros(2, 8, 4, 4, dtype=torch.bfloat16).to(memory_format=torch.channels_last))):
        with pytest.raises(L.CnnqError):
            ops.qdq_bias_corrected_half(bad, qp, True)
