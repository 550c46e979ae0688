"""CPU-only checks of dynamic ACIQ clipping on contiguous bf16 / fp16 activations: the three entry points exist
and their ctypes prototypes match the header, bad arguments are refused before anything touches the device, the workspace covers
the documented records, the route function over a grid of (N, C, HW, dtype, alignment, allow, bit allocation, prior) with the plan
enumerated in Python, the fp32 forward, and the quantizer's opt-in routing predicate as a truth table - next to _half_native's
answers for the same inputs, which it must not change."""
import ctypes

import pytest
import torch

import _half_aciq as HA
import _quantizer as Q
from test_channels_last_collect_cpu import ctype_of, header_decls
from _quantizer import FakeCuda, act

FUNCS = ['cnnq_pc_aciq_dt_workspace', 'cnnq_pc_route_aciq_dt', 'cnnq_pc_aciq_qdq_dt']
BAD = 0x1000   # a non-null pointer value that is never dereferenced: the argument checks come first
EINVAL, ERANGE = -1, -2
NMOM, NDEV = 7, 2


def lib():
    from cnn_quantization_amd import _lib as L
    return L.load()


def cfg_of(num_bits=4, clip=1, bit_alloc=0, prior_is_b=0, positive=0, direct_range=0):
    from cnn_quantization_amd import _lib as L
    return L.ParamsCfg(num_bits=num_bits, positive=positive, clip=clip, pstd=0., bit_alloc=bit_alloc, prior_is_b=prior_is_b,
                       target=float(num_bits), round_mode=1, direct_range=direct_range)


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


def call_args(dtype=1, N=2, C=8, HW=16, cfg=None):
    p = ctypes.c_void_p
    # x, y, dtype, N, C, HW, cfg, ws, stats, qp, diag, allow_single_launch, stream
    return [p(BAD), p(2 * BAD), dtype, N, C, HW, ctypes.byref(cfg or cfg_of()), p(3 * BAD), p(4 * BAD), p(5 * BAD), p(6 * BAD), 1, None]


@pytest.mark.parametrize('dtype, N, C, HW', [(-1, 2, 8, 16), (3, 2, 8, 16), (1 << 20, 2, 8, 16), (1, 0, 8, 16), (2, 2, 0, 16),
                                             (1, 2, 8, 0), (0, -3, 8, 16), (2, 2, -1, 16), (1, 2, 8, -5)])
def test_bad_geometry_is_einval(dtype, N, C, HW):
    out = (ctypes.c_int32 * 4)()
    assert lib().cnnq_pc_aciq_dt_workspace(N, C, HW, dtype) == 0
    assert lib().cnnq_pc_route_aciq_dt(N, C, HW, dtype, 16, ctypes.byref(cfg_of()), 1, out) == EINVAL
    assert lib().cnnq_pc_aciq_qdq_dt(*call_args(dtype, N, C, HW)) == EINVAL


@pytest.mark.parametrize('dtype', [0, 1, 2])
def test_refusals_need_no_device(dtype):
    for i in (0, 1, 6, 7, 8, 9):                            # x, y, cfg, ws, stats, qp
        a = call_args(dtype)
        a[i] = None
        assert lib().cnnq_pc_aciq_qdq_dt(*a) == EINVAL, i
    a = call_args(dtype)
    a[10] = None                                            # diag may be NULL without bit allocation in effect: not refused for that
    a[0] = None
    assert lib().cnnq_pc_aciq_qdq_dt(*a) == EINVAL
    a = call_args(dtype)
    a[7] = ctypes.c_void_p(BAD + 4)                         # ws holds doubles
    assert lib().cnnq_pc_aciq_qdq_dt(*a) == EINVAL
    for i in (0, 1, 8, 9, 10):                              # x and y not aligned to their element, the fp32 tables to theirs
        a = call_args(dtype)
        a[i] = ctypes.c_void_p(BAD + (2 if dtype == 0 or i in (8, 9, 10) else 1))
        assert lib().cnnq_pc_aciq_qdq_dt(*a) == EINVAL, i
    a = call_args(dtype)
    a[1] = a[0]                                             # in place
    assert lib().cnnq_pc_aciq_qdq_dt(*a) == EINVAL
    out = (ctypes.c_int32 * 4)()
    bad_cfgs = [cfg_of(num_bits=0), cfg_of(num_bits=33), cfg_of(num_bits=16),          # check_cfg: the factor tables end at 8 bits
                cfg_of(clip=-1), cfg_of(clip=4), cfg_of(direct_range=1),
                cfg_of(clip=0), cfg_of(clip=3)]                                        # a clip other than Laplace / Gaussian
    for cfg in bad_cfgs:
        assert lib().cnnq_pc_aciq_qdq_dt(*call_args(dtype, cfg=cfg)) == EINVAL, (cfg.num_bits, cfg.clip, cfg.direct_range)
        assert lib().cnnq_pc_route_aciq_dt(2, 8, 16, dtype, 16, ctypes.byref(cfg), 1, out) == EINVAL
    a = call_args(dtype, cfg=cfg_of(bit_alloc=1))           # the bit table lives in diag
    a[10] = None
    assert lib().cnnq_pc_aciq_qdq_dt(*a) == EINVAL
    assert lib().cnnq_pc_route_aciq_dt(2, 8, 16, dtype, 3, ctypes.byref(cfg_of()), 1, out) == EINVAL
    assert lib().cnnq_pc_route_aciq_dt(2, 8, 16, dtype, 0, ctypes.byref(cfg_of()), 1, out) == EINVAL
    assert lib().cnnq_pc_route_aciq_dt(2, 8, 16, dtype, 16, ctypes.byref(cfg_of()), 1, None) == EINVAL
    assert lib().cnnq_pc_route_aciq_dt(2, 8, 16, dtype, 16, None, 1, out) == EINVAL
    # cnnq_pc_groups' limits: a sample of 2^31 elements, 2^31 samples
    for N, C, HW in ((2, 1 << 16, 1 << 15), (1 << 31, 2, 4)):
        assert lib().cnnq_pc_groups(N, C, HW, 0) == ERANGE
        assert lib().cnnq_pc_aciq_dt_workspace(N, C, HW, dtype) == 0
        assert lib().cnnq_pc_route_aciq_dt(N, C, HW, dtype, 16, ctypes.byref(cfg_of()), 1, out) == ERANGE
        assert lib().cnnq_pc_aciq_qdq_dt(*call_args(dtype, N, C, HW)) == ERANGE


GRID = [(N, C, HW) for N in (1, 2, 3, 5, 8, 64, 512) for C in (1, 3, 64, 256, 520, 2048)
        for HW in (1, 2, 7, 49, 98, 196, 784, 3136, 6400, 12544, 50176)]
CONFIGS = [(4, 0, 0), (4, 1, 0), (4, 1, 1), (8, 1, 0), (8, 1, 1), (4, 0, 1)]     # (bits, bit_alloc, prior_is_b); 8 bits: no allocation in effect


@pytest.mark.parametrize('dtype', [1, 2])
@pytest.mark.parametrize('align', [2, 4, 8, 16, 64])
def test_route_and_workspace_over_a_grid(dtype, align):
    out = (ctypes.c_int32 * 4)()
    for N, C, HW in GRID:
        for bits, ba, prior in CONFIGS:
            for clip in (1, 2):
                cfg = cfg_of(num_bits=bits, clip=clip, bit_alloc=ba, prior_is_b=prior)
                for allow in (0, 1, 2):
                    assert lib().cnnq_pc_route_aciq_dt(N, C, HW, dtype, align, ctypes.byref(cfg), allow, out) == 0, (N, C, HW)
                    want = HA.route(N, C, HW, align, allow, bool(ba) and bits <= 4, bool(prior))
                    assert tuple(out) == want, (N, C, HW, align, allow, bits, ba, prior, tuple(out))
                    if out[3] in (1, 3):
                        assert allow and out[0] >= 2 and N * HW <= HA.WHOLE_CAP and (out[3] == 3) == (bool(ba) and bits <= 4)
        w, S, cs, _ = out
        assert 1 <= S <= N and 1 <= cs <= max(1, HW // 8) and C * S * cs < 1 << 31
        # ws, doubles: part[G][NMOM][C], mom[NMOM][C], part2[G][NDEV][C] with G = S * cs, whatever the alignment and the route
        G = S * cs
        assert lib().cnnq_pc_aciq_dt_workspace(N, C, HW, dtype) == (G * NMOM + NMOM + G * NDEV) * C * 8, (N, C, HW)
        assert lib().cnnq_pc_aciq_dt_workspace(N, C, HW, dtype) == lib().cnnq_pc_stats_dt_workspace(N, C, HW, dtype)


def test_the_gpu_tests_cases_reach_their_branches():
    out = (ctypes.c_int32 * 4)()
    for shape, offset, (W, S, cs, fits) in HA.CASES:
        N, C, HW = shape[0], shape[1], shape[2] * shape[3]
        align = (2 * offset) & -(2 * offset) if offset else 16
        for dtype in (1, 2):
            for ba, prior, resident in ((0, 0, 1), (1, 0, 3), (1, 1, 2)):
                cfg = cfg_of(bit_alloc=ba, prior_is_b=prior)
                assert lib().cnnq_pc_route_aciq_dt(N, C, HW, dtype, align, ctypes.byref(cfg), 2, out) == 0
                assert tuple(out) == (W, S, cs, resident if fits else 2), (shape, offset, ba, prior, tuple(out))
                assert lib().cnnq_pc_route_aciq_dt(N, C, HW, dtype, align, ctypes.byref(cfg), 0, out) == 0
                assert tuple(out) == (W, S, cs, 2), (shape, offset, tuple(out))


def test_float32_answers_the_chain():
    out = (ctypes.c_int32 * 4)()
    for N, C, HW in ((8, 12, 784), (3, 10, 196), (2, 64, 49)):
        G = max(lib().cnnq_pc_groups(N, C, HW, a) for a in (0, 1))
        for align in (4, 16):
            for allow in (0, 1, 2):
                for ba in (0, 1):
                    assert lib().cnnq_pc_route_aciq_dt(N, C, HW, 0, align, ctypes.byref(cfg_of(bit_alloc=ba)), allow, out) == 0
                    assert list(out) == [0, G, 1, 2]
        assert lib().cnnq_pc_aciq_dt_workspace(N, C, HW, 0) == max(lib().cnnq_pc_aciq_workspace(N, C, HW, a) for a in (0, 1))


# ---- the quantizer's predicate
def quantizer(half_dynamic=True, **kw):
    q = Q.quantizer(**dict(dict(clipping='laplace', pcq_act=True, bit_alloc_act=True), **kw))
    assert q.half_dynamic is False                          # opt-in: the constructor leaves it off
    q.half_dynamic = half_dynamic
    return q


def test_predicate_truth_table(monkeypatch):
    from cnn_quantization_amd import distributed as D, ops
    x = act()

    def dyn(q, t=x, stat_id=None, override=None):
        att = q._att(override)
        return q._half_aciq(t, att('clipping'), stat_id, att)

    # the attributes: every combination, with and without a pending correction, stat_id and the opt-in
    for clipping in ('no', 'laplace', 'gaus', 'mix', '2std'):
        for ba in (False, True):
            for flags in range(32):
                pcq_a, pcq_w, mtd, kld, me = (bool(flags >> i & 1) for i in range(5))
                for pending in (None, True):
                    for stat_id in (None, 'layer0'):
                        kw = dict(clipping=clipping, bit_alloc_act=ba, pcq_act=pcq_a, pcq_weights=pcq_w, mtd_quant=mtd, kld=kld,
                                  measure_entropy=me)
                        q = quantizer(**kw)
                        q.fuse_bcorr = pending
                        want = (stat_id is None and pcq_a and clipping in ('laplace', 'gaus') and not mtd and not kld and not me
                                and pending is None)
                        assert dyn(q, stat_id=stat_id) == want, (clipping, ba, flags, pending, stat_id)
                        off = quantizer(half_dynamic=False, **kw)
                        off.fuse_bcorr = pending
                        assert not dyn(off, stat_id=stat_id)
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
    assert not dyn(q, override=('clipping', 'mix')) and not dyn(q, override=('mtd_quant', True))
    assert dyn(quantizer(clipping='mix'), override=('clipping', 'gaus'))
    # the tensor
    for dtype in (torch.bfloat16, torch.float16):
        assert dyn(q, act(dtype))
    assert not dyn(q, torch.zeros(2, 8, 4, 4, dtype=torch.bfloat16))                          # on the CPU
    assert not dyn(q, act(torch.float32)) and not dyn(q, act(torch.float64))
    assert not dyn(q, FakeCuda(torch.zeros(2, 8, 4, 4, dtype=torch.bfloat16).to(memory_format=torch.channels_last)))
    assert not dyn(q, FakeCuda(torch.zeros(2, 12, 4, 4, dtype=torch.bfloat16)[:, 2:9]))       # not dense
    assert not dyn(q, act(shape=(2, 8, 1, 1)))                                                # no spatial extent
    assert not dyn(q, act(shape=(8, 16))) and not dyn(q, act(shape=(2, 8, 16)))
    assert not dyn(q, act(shape=(0, 8, 4, 4)))
    assert dyn(q, act(shape=(2, 8, 1, 7))) and dyn(q, act(shape=(4, 8, 7, 7)))
    # replicated data, more than one process, the forced exchange
    q.group = False
    assert not dyn(q)
    q.group = None
    monkeypatch.setattr(D, 'world_size', lambda group=None: 2)
    assert not dyn(q)
    monkeypatch.undo()
    monkeypatch.setattr(D, 'forced_exchange', lambda: True)
    assert not dyn(q)
    monkeypatch.undo()
    assert dyn(q)
    # a class of layer the route function sends back; every other word is native.  The bit allocation in effect and its prior
    # reach the route function
    for word, want in ((0, False), (1, True), (2, True), (3, True)):
        monkeypatch.setattr(ops, '_aciq_half_native', lambda N, C, HW, dtype, ba=False, prior=False, word=word: word)
        assert dyn(q) == want
        monkeypatch.undo()
    asked = []
    monkeypatch.setattr(ops, '_aciq_half_native', lambda *a: asked.append(a) or 2)
    assert dyn(quantizer()) and dyn(quantizer(bit_alloc_prior='laplace')) and dyn(quantizer(bit_alloc_act=False, bit_alloc_prior='laplace'))
    q8 = quantizer()
    q8.num_bits = 8                                                                           # no allocation in effect above 4 bits
    assert dyn(q8)
    assert asked == [(2, 8, 16, torch.bfloat16, True, False), (2, 8, 16, torch.bfloat16, True, True),
                     (2, 8, 16, torch.bfloat16, False, False), (2, 8, 16, torch.bfloat16, False, False)]
    monkeypatch.undo()
    # the switch
    monkeypatch.setenv('CNNQ_HALF_ACIQ', '0')
    ops.reload_switches()
    try:
        assert not dyn(q)
    finally:
        monkeypatch.delenv('CNNQ_HALF_ACIQ')
        ops.reload_switches()
    assert dyn(q)


def test_the_manager_opts_its_quantizers_in():
    from cnn_quantization_amd.inference import inference_quantization_manager as M
    src = M.TruncationOpManagerInference._load
    import inspect
    assert 'half_dynamic = True' in inspect.getsource(src)


def test_route_is_asked_once_per_class(monkeypatch):
    from cnn_quantization_amd import ops
    asked = []
    real = lib().cnnq_pc_route_aciq_dt

    class Lib:
        def cnnq_pc_route_aciq_dt(self, *a):
            asked.append(a[:5] + (a[5]._obj.bit_alloc, a[5]._obj.prior_is_b, a[6]))
            return real(*a)
    monkeypatch.setattr(ops.L, 'load', lambda: Lib())
    monkeypatch.setattr(ops, '_ACIQ_HALF_NATIVE', {})
    for _ in range(3):
        for dtype in (torch.bfloat16, torch.float16):
            assert ops._aciq_half_native(2, 12, 196, dtype) == HA.route(2, 12, 196, 16, 1)[3]
            assert ops._aciq_half_native(2, 12, 196, dtype, True, False) == HA.route(2, 12, 196, 16, 1, True, False)[3]
            assert ops._aciq_half_native(2, 12, 196, dtype, True, True) == 2
    assert asked == [(2, 12, 196, code, 16, ba, prior, 1) for code in (1, 2) for ba, prior in ((0, 0), (1, 0), (1, 1))]


def test_op_refuses_what_it_does_not_take():
    from cnn_quantization_amd import _lib as L, ops
    with pytest.raises(L.CnnqError):
        ops.aciq_qdq_half(torch.zeros(2, 8, 4, 4, dtype=torch.bfloat16), 4)            # a CPU tensor: there is no CPU path
    with pytest.raises(L.CnnqError):
        ops.aciq_qdq_half(None, 4)
    for bad in (act(torch.float32), act(shape=(2, 8, 16)), act(shape=(0, 8, 4, 4)),
                FakeCuda(torch.zeros(2, 8, 4, 4, dtype=torch.bfloat16).to(memory_format=torch.channels_last))):
        with pytest.raises(L.CnnqError):
            ops.aciq_qdq_half(bad, 4)
    for clip in ('no', 'mix', '2std'):
        with pytest.raises(L.CnnqError):
            ops.aciq_qdq_half(act(), 4, clip=clip)
