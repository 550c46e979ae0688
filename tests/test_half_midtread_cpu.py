"""CPU-only checks of mid-tread quantization (config 5) on contiguous bf16 / fp16 activations: the entry
points exist and their ctypes prototypes match the header, bad arguments are refused before anything touches the device, the
workspace is cnnq_pc_stats_dt's, the route function equals its restatement in Python (tests/_half_midtread.py) over the GPU tests'
cases, the benchmark's classes and a grid, and the quantizer's opt-in route as a truth table."""
import ctypes
import inspect

import pytest
import torch

import _half_midtread as HM
import _quantizer as Q
from _quantizer import FakeCuda, act, nhwc
from test_channels_last_collect_cpu import ctype_of, header_decls

FUNCS = ['cnnq_pc_midtread_dt_workspace', 'cnnq_pc_route_midtread_dt', 'cnnq_pc_midtread_qdq_dt', 'cnnq_pc_midtread_dt']
BAD = 0x1000   # a non-null pointer value that is never dereferenced: the argument checks come first
EINVAL, ERANGE, ENOTSUP = -1, -2, -3
NMOM, NDEV = 7, 2


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
            want = ctypes.c_double if a.startswith('double ') else ctype_of(a)
            if want == 'ptr':
                assert t is ctypes.c_void_p or issubclass(t, ctypes._Pointer), (name, a, t)
            else:
                assert t is want, (name, a, t)


def call_args(dtype=1, N=2, C=8, HW=16):
    p = ctypes.c_void_p
    # x, y, dtype, N, C, HW, target, sym, tables, ntab, ws, stats, mt, hist, allow_single_launch, stream
    return [p(BAD), p(2 * BAD), dtype, N, C, HW, 5.3, 1, p(3 * BAD), 101, p(4 * BAD), p(5 * BAD), p(6 * BAD), p(7 * BAD), 1, None]


def qdq_args(dtype=1, N=2, C=8, HW=16):
    p = ctypes.c_void_p
    # x, y, dtype, N, C, HW, mt, hist, stream
    return [p(BAD), p(2 * BAD), dtype, N, C, HW, p(3 * BAD), p(4 * BAD), None]


@pytest.mark.parametrize('dtype, N, C, HW', [(-1, 2, 8, 16), (3, 2, 8, 16), (1 << 20, 2, 8, 16), (1, 0, 8, 16), (2, 2, 0, 16),
                                             (1, 2, 8, 0), (0, -3, 8, 16), (2, 2, -1, 16), (1, 2, 8, -5)])
def test_bad_geometry_is_einval(dtype, N, C, HW):
    out = (ctypes.c_int32 * 4)()
    assert lib().cnnq_pc_midtread_dt_workspace(N, C, HW, dtype) == 0
    assert lib().cnnq_pc_route_midtread_dt(N, C, HW, dtype, 16, 0, 1, out) == EINVAL
    assert lib().cnnq_pc_midtread_dt(*call_args(dtype, N, C, HW)) == EINVAL
    assert lib().cnnq_pc_midtread_qdq_dt(*qdq_args(dtype, N, C, HW)) == EINVAL


@pytest.mark.parametrize('dtype', [0, 1, 2])
def test_refusals_need_no_device(dtype):
    es = 4 if dtype == 0 else 2
    for i in (0, 1, 8, 10, 11, 12):                         # x, y, tables, ws, stats, mt
        a = call_args(dtype)
        a[i] = None
        assert lib().cnnq_pc_midtread_dt(*a) == EINVAL, i
    for i in (0, 1, 6):                                     # x, y, mt
        a = qdq_args(dtype)
        a[i] = None
        assert lib().cnnq_pc_midtread_qdq_dt(*a) == EINVAL, i
    for i, off in ((0, es // 2), (1, es // 2), (8, 4), (10, 4), (11, 2), (12, 2), (13, 4)):       # misaligned pointers
        a = call_args(dtype)
        a[i] = ctypes.c_void_p(a[i].value + off)
        assert lib().cnnq_pc_midtread_dt(*a) == EINVAL, i
    for i, off in ((0, es // 2), (1, es // 2), (6, 2), (7, 4)):
        a = qdq_args(dtype)
        a[i] = ctypes.c_void_p(a[i].value + off)
        assert lib().cnnq_pc_midtread_qdq_dt(*a) == EINVAL, i
    a = call_args(dtype)
    a[1] = a[0]                                             # in place
    assert lib().cnnq_pc_midtread_dt(*a) == EINVAL
    a = qdq_args(dtype)
    a[1] = a[0]
    assert lib().cnnq_pc_midtread_qdq_dt(*a) == EINVAL
    for ntab in (1, 0, -4):
        a = call_args(dtype)
        a[9] = ntab
        assert lib().cnnq_pc_midtread_dt(*a) == EINVAL
    for target in (float('nan'), float('inf')):
        a = call_args(dtype)
        a[6] = target
        assert lib().cnnq_pc_midtread_dt(*a) == EINVAL
    out = (ctypes.c_int32 * 4)()
    for align in (3, 0, -2, 24):
        assert lib().cnnq_pc_route_midtread_dt(2, 8, 16, dtype, align, 0, 1, out) == EINVAL
    assert lib().cnnq_pc_route_midtread_dt(2, 8, 16, dtype, 16, 0, 1, None) == EINVAL
    if dtype == 0:
        return
    # cnnq_pc_groups' limits: a sample of 2^31 elements, 2^31 samples
    for N, C, HW in ((2, 1 << 16, 1 << 15), (1 << 31, 2, 4)):
        assert lib().cnnq_pc_groups(N, C, HW, 0) == ERANGE
        assert lib().cnnq_pc_midtread_dt_workspace(N, C, HW, dtype) == 0
        assert lib().cnnq_pc_route_midtread_dt(N, C, HW, dtype, 16, 0, 1, out) == ERANGE
        assert lib().cnnq_pc_midtread_dt(*call_args(dtype, N, C, HW)) == ERANGE
        assert lib().cnnq_pc_midtread_qdq_dt(*qdq_args(dtype, N, C, HW)) == ERANGE


def test_float32_is_not_supported_by_the_one_call_form():
    """fp32 callers have cnnq_pc_midtread_qdq_single and the chain: CNNQ_ENOTSUP before any launch, no plan, no workspace."""
    out = (ctypes.c_int32 * 4)()
    assert lib().cnnq_pc_midtread_dt(*call_args(0)) == ENOTSUP
    a = call_args(0)
    a[13] = None                                            # with or without the histogram
    assert lib().cnnq_pc_midtread_dt(*a) == ENOTSUP
    assert lib().cnnq_pc_route_midtread_dt(2, 8, 16, 0, 16, 0, 1, out) == ENOTSUP
    assert lib().cnnq_pc_midtread_dt_workspace(2, 8, 16, 0) == 0


GRID = [(N, C, HW) for N in (1, 2, 3, 5, 8, 64, 512) for C in (1, 3, 64, 256, 520, 2048)
        for HW in (1, 2, 7, 49, 98, 196, 784, 3136, 6400, 12544, 50176)]


def check_route(N, C, HW, dtype, align):
    out = (ctypes.c_int32 * 4)()
    for allow in (0, 1, 2):
        for hist in (0, 1):
            assert lib().cnnq_pc_route_midtread_dt(N, C, HW, dtype, align, hist, allow, out) == 0, (N, C, HW)
            assert tuple(out) == HM.route(N, C, HW, align, allow, bool(hist)), (N, C, HW, align, allow, hist, tuple(out))
            if out[3] == 3:
                assert allow and out[0] >= 2 and N * HW <= HM.WHOLE_CAP
            if allow == 0:
                assert out[3] in (0, 2)
    return tuple(out)


@pytest.mark.parametrize('dtype', [1, 2])
@pytest.mark.parametrize('align', [2, 4, 16])
def test_route_equals_its_restatement(dtype, align):
    for N, C, HW in HM.CLASSES + [(s[0], s[1], s[2] * s[3]) for s, _, _ in HM.CASES] + GRID:
        w, S, cs, _ = check_route(N, C, HW, dtype, align)
        assert 1 <= S <= N and 1 <= cs <= max(1, HW // 8) and C * S * cs < 1 << 31
        # ws, doubles: part[G][NMOM][C], mom[NMOM][C], part2[G][NDEV][C] with G = S * cs, whatever the alignment and the route
        G = S * cs
        assert lib().cnnq_pc_midtread_dt_workspace(N, C, HW, dtype) == (G * NMOM + NMOM + G * NDEV) * C * 8, (N, C, HW)
        assert lib().cnnq_pc_midtread_dt_workspace(N, C, HW, dtype) == lib().cnnq_pc_stats_dt_workspace(N, C, HW, dtype)


def test_the_gpu_tests_cases_reach_their_branches():
    assert len(HM.CLASSES) == 17
    out = (ctypes.c_int32 * 4)()
    for shape, offset, (W, S, cs, fits) in HM.CASES:
        N, C, HW = shape[0], shape[1], shape[2] * shape[3]
        align = (2 * offset) & -(2 * offset) if offset else 16
        for dtype in (1, 2):
            for hist in (0, 1):
                assert lib().cnnq_pc_route_midtread_dt(N, C, HW, dtype, align, hist, 2, out) == 0
                assert tuple(out) == (W, S, cs, 3 if fits else 2), (shape, offset, tuple(out))
                assert lib().cnnq_pc_route_midtread_dt(N, C, HW, dtype, align, hist, 0, out) == 0
                assert tuple(out) == (W, S, cs, 2), (shape, offset, tuple(out))


# ---- the quantizer's route
def quantizer(half_midtread=True, **kw):
    q = Q.quantizer(**dict(dict(clipping='laplace', pcq_act=True, bit_alloc_act=True, bit_alloc_target_act=5.3, mtd_quant=True), **kw))
    assert q.half_midtread is False                         # opt-in: the constructor leaves it off
    q.half_midtread = half_midtread
    return q


def asked(q, t=None, override=None, stat_id=None):
    return q._asked(act() if t is None else t, stat_id, q._att(override))


def test_route_truth_table(monkeypatch):
    from cnn_quantization_amd import distributed as D, ops
    for clipping in ('no', 'laplace', 'gaus', 'mix'):
        for flags in range(32):
            pcq_a, pcq_w, mtd, kld, me = (bool(flags >> i & 1) for i in range(5))
            for pending in (None, True):
                kw = dict(clipping=clipping, pcq_act=pcq_a, pcq_weights=pcq_w, mtd_quant=mtd, kld=kld, measure_entropy=me)
                q = quantizer(**kw)
                q.fuse_bcorr = pending
                before = dict(vars(q))
                want = pcq_a and mtd and clipping != 'no' and not kld and pending is None
                assert (asked(q) == 'half_midtread') == want, (clipping, flags, pending)
                assert vars(q) == before                    # nothing is stored on the object
                # a directly constructed object, and one the ACIQ opt-in alone was set on, keep the upcast route
                off = quantizer(half_midtread=False, **kw)
                off.fuse_bcorr = pending
                off.half_dynamic = True
                assert asked(off) != 'half_midtread'
                if pcq_a and mtd and clipping != 'no' and not kld:
                    assert asked(off) is None
    q = quantizer()
    assert Q.quantizer(clipping='laplace', pcq_act=True, mtd_quant=True)._asked(act()) is None
    # __call__'s override pair wins over the attribute
    assert asked(quantizer(mtd_quant=False), override=('mtd_quant', True)) == 'half_midtread'
    assert asked(q, override=('mtd_quant', False)) != 'half_midtread'
    assert asked(q, override=('clipping', 'no')) is None and asked(q, override=('kld', True)) != 'half_midtread'
    assert asked(q, stat_id='layer0') == 'half_midtread'                                # mid-tread reads no calibration table
    # the tensor
    for dtype in (torch.bfloat16, torch.float16):
        assert asked(q, act(dtype)) == 'half_midtread'
    assert asked(q, nhwc()) == 'nhwc_midtread'                                                # channels_last comes first
    assert asked(q, torch.zeros(2, 8, 4, 4, dtype=torch.bfloat16)) is None                    # on the CPU
    assert asked(q, act(torch.float32)) is None
    assert asked(q, FakeCuda(torch.zeros(2, 12, 4, 4, dtype=torch.bfloat16)[:, 2:9])) is None  # not dense
    assert asked(q, act(shape=(0, 8, 4, 4))) is None
    assert asked(q, act(shape=(2, 8, 1, 1))) != 'half_midtread'                               # no spatial extent: per tensor
    assert asked(q, act(shape=(8, 16))) != 'half_midtread'
    assert asked(q, act(shape=(2, 8, 1, 7))) == 'half_midtread' and asked(q, act(shape=(4, 8, 7, 7))) == 'half_midtread'
    # replicated data, more than one process, the forced exchange
    q.group = False
    assert asked(q) is None
    q.group = None
    monkeypatch.setattr(D, 'world_size', lambda group=None: 2)
    assert asked(q) is None
    monkeypatch.undo()
    monkeypatch.setattr(D, 'forced_exchange', lambda: True)
    assert asked(q) is None
    monkeypatch.undo()
    assert asked(q) == 'half_midtread'
    # a class of layer the route function sends back; every other word is native.  Whether the codes are counted reaches it
    for word, want in ((0, None), (2, 'half_midtread'), (3, 'half_midtread')):
        monkeypatch.setattr(ops, '_midtread_half_native', lambda N, C, HW, dtype, hist=False, word=word: word)
        assert asked(q) == want
        monkeypatch.undo()
    seen = []
    monkeypatch.setattr(ops, '_midtread_half_native', lambda *a: seen.append(a) or 2)
    assert asked(quantizer()) and asked(quantizer(measure_entropy=True)) and asked(q, override=('measure_entropy', True))
    assert seen == [(2, 8, 16, torch.bfloat16, False), (2, 8, 16, torch.bfloat16, True), (2, 8, 16, torch.bfloat16, True)]
    monkeypatch.undo()
    # the switch
    monkeypatch.setenv('CNNQ_HALF_MIDTREAD', '0')
    ops.reload_switches()
    try:
        assert asked(q) is None
    finally:
        monkeypatch.delenv('CNNQ_HALF_MIDTREAD')
        ops.reload_switches()
    assert asked(q) == 'half_midtread'


def test_the_manager_opts_its_quantizers_in():
    from cnn_quantization_amd.inference import inference_quantization_manager as M
    src = inspect.getsource(M.TruncationOpManagerInference._load)
    assert 'half_midtread = True' in src and 'half_dynamic = True' in src


def test_route_is_asked_once_per_class(monkeypatch):
    from cnn_quantization_amd import ops
    seen = []
    real = lib().cnnq_pc_route_midtread_dt

    class Lib:
        def cnnq_pc_route_midtread_dt(self, *a):
            seen.append(a[:7])
            return real(*a)
    monkeypatch.setattr(ops.L, 'load', lambda: Lib())
    monkeypatch.setattr(ops, '_MIDTREAD_HALF_NATIVE', {})
    for _ in range(3):
        for dtype in (torch.bfloat16, torch.float16):
            for hist in (False, True):
                assert ops._midtread_half_native(2, 12, 196, dtype, hist) == HM.route(2, 12, 196, 16, 1, hist)[3]
                assert ops._midtread_half_native(512, 512, 49, dtype, hist) == 0
    assert seen == [(N, C, HW, code, 16, hist, 1) for code in (1, 2) for hist in (0, 1) for N, C, HW in ((2, 12, 196), (512, 512, 49))]


def test_op_refuses_what_it_does_not_take():
    from cnn_quantization_amd import _lib as L, ops
    with pytest.raises(L.CnnqError):
        ops.mid_tread_qdq_half(torch.zeros(2, 8, 4, 4, dtype=torch.bfloat16), 5.3, True)    # a CPU tensor: there is no CPU path
    with pytest.raises(L.CnnqError):
        ops.mid_tread_qdq_half(None, 5.3, True)
    for bad in (act(torch.float32), act(shape=(2, 8, 16)), act(shape=(0, 8, 4, 4)), nhwc()):
        with pytest.raises(L.CnnqError):
            ops.mid_tread_qdq_half(bad, 5.3, True)
