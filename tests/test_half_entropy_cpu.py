"""CPU-only checks of the uniform Q/DQ that counts its codes (-me) on contiguous bf16 / fp16 activations:
the entry points exist and their ctypes prototypes match the header, bad arguments are refused before anything touches the device,
the route function equals its restatement in Python (tests/_half_entropy.py) over the GPU tests' cases, the benchmark's classes
and a grid, and the quantizer's opt-in route over the attribute grid: with the flag off every answer is the parent's."""
import ctypes
import inspect

import pytest
import torch

import _half_entropy as HE
import _quantizer as Q
from _quantizer import FakeCuda, act, nhwc
from test_channels_last_collect_cpu import ctype_of, header_decls

FUNCS = ['cnnq_pc_route_qdq_hist_dt', 'cnnq_pc_qdq_hist_dt', 'cnnq_pc_minmax_qdq_hist_dt', 'cnnq_pc_aciq_qdq_hist_dt']
BAD = 0x1000   # a non-null pointer value that is never dereferenced: the argument checks come first
EINVAL, ERANGE, ENOTSUP = -1, -2, -3


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


def cfg(bits=4, clip='laplace', bit_alloc=False):
    from cnn_quantization_amd import ops
    c = ops._params_cfg(min(bits, 8), False, clip, bit_alloc, False, None, True, False)
    c.num_bits = bits                                       # (ops itself refuses clipping beyond 8 bits)
    return c


def table_args(dtype=1, N=2, C=8, HW=16, nbins=16):
    p = ctypes.c_void_p
    # x, y, dtype, N, C, HW, qp, nbins, hist_rep, stream
    return [p(BAD), p(2 * BAD), dtype, N, C, HW, p(3 * BAD), nbins, p(4 * BAD), None]


def minmax_args(dtype=1, N=2, C=8, HW=16, bits=4, allow=1):
    p = ctypes.c_void_p
    # x, y, dtype, N, C, HW, num_bits, positive, ws, qp, mm, hist_rep, allow_single_launch, stream
    return [p(BAD), p(2 * BAD), dtype, N, C, HW, bits, 0, p(3 * BAD), p(4 * BAD), p(5 * BAD), p(6 * BAD), allow, None]


def aciq_args(dtype=1, N=2, C=8, HW=16, c=None):
    p = ctypes.c_void_p
    # x, y, dtype, N, C, HW, cfg, ws, stats, qp, diag, hist_rep, stream
    return [p(BAD), p(2 * BAD), dtype, N, C, HW, ctypes.byref(c or cfg()), p(3 * BAD), p(4 * BAD), p(5 * BAD), p(6 * BAD), p(7 * BAD), None]


@pytest.mark.parametrize('dtype, N, C, HW', [(-1, 2, 8, 16), (3, 2, 8, 16), (1 << 20, 2, 8, 16), (1, 0, 8, 16), (2, 2, 0, 16),
                                             (1, 2, 8, 0), (0, -3, 8, 16), (2, 2, -1, 16), (1, 2, 8, -5)])
def test_bad_geometry_is_einval(dtype, N, C, HW):
    out = (ctypes.c_int32 * 4)()
    assert lib().cnnq_pc_route_qdq_hist_dt(N, C, HW, dtype, 16, 16, 1, out) == EINVAL
    assert lib().cnnq_pc_qdq_hist_dt(*table_args(dtype, N, C, HW)) == EINVAL
    assert lib().cnnq_pc_minmax_qdq_hist_dt(*minmax_args(dtype, N, C, HW)) == EINVAL
    assert lib().cnnq_pc_aciq_qdq_hist_dt(*aciq_args(dtype, N, C, HW)) == EINVAL


@pytest.mark.parametrize('dtype', [0, 1, 2])
def test_refusals_need_no_device(dtype):
    """Every refusal comes before the dtype's own answer: float32 too is told CNNQ_EINVAL for a bad argument."""
    for i in (0, 1, 6, 8):                                  # x, y, qp, hist_rep
        a = table_args(dtype)
        a[i] = None
        assert lib().cnnq_pc_qdq_hist_dt(*a) == EINVAL, i
    a = table_args(dtype)
    a[8] = ctypes.c_void_p(a[8].value + 4)                  # a misaligned hist_rep
    assert lib().cnnq_pc_qdq_hist_dt(*a) == EINVAL
    a = table_args(dtype)
    a[1] = a[0]                                             # in place
    assert lib().cnnq_pc_qdq_hist_dt(*a) == EINVAL
    for nbins in (0, 1, 3, 12, 24, 255, 257, 512, -16):
        assert lib().cnnq_pc_qdq_hist_dt(*table_args(dtype, nbins=nbins)) == EINVAL, nbins
    for i in (0, 1, 8, 9, 11):                              # x, y, ws, qp, hist_rep (mm may be NULL)
        a = minmax_args(dtype)
        a[i] = None
        assert lib().cnnq_pc_minmax_qdq_hist_dt(*a) == EINVAL, i
    for i, off in ((8, 2), (11, 4)):                        # a misaligned ws / hist_rep
        a = minmax_args(dtype)
        a[i] = ctypes.c_void_p(a[i].value + off)
        assert lib().cnnq_pc_minmax_qdq_hist_dt(*a) == EINVAL, i
    a = minmax_args(dtype)
    a[1] = a[0]
    assert lib().cnnq_pc_minmax_qdq_hist_dt(*a) == EINVAL
    for bits in (0, -1, 9, 16, 32):
        assert lib().cnnq_pc_minmax_qdq_hist_dt(*minmax_args(dtype, bits=bits)) == EINVAL, bits
    for i in (0, 1, 6, 7, 8, 9, 11):                        # x, y, cfg, ws, stats, qp, hist_rep (diag may be NULL without bit allocation)
        a = aciq_args(dtype)
        a[i] = None
        assert lib().cnnq_pc_aciq_qdq_hist_dt(*a) == EINVAL, i
    for i, off in ((7, 4), (11, 4)):                        # a misaligned ws / hist_rep
        a = aciq_args(dtype)
        a[i] = ctypes.c_void_p(a[i].value + off)
        assert lib().cnnq_pc_aciq_qdq_hist_dt(*a) == EINVAL, i
    a = aciq_args(dtype)
    a[1] = a[0]
    assert lib().cnnq_pc_aciq_qdq_hist_dt(*a) == EINVAL
    a = aciq_args(dtype, c=cfg(bit_alloc=True))
    a[10] = None                                            # the bit table lives in diag
    assert lib().cnnq_pc_aciq_qdq_hist_dt(*a) == EINVAL
    for c in (cfg(bits=9), cfg(bits=16), cfg(clip='no')):
        assert lib().cnnq_pc_aciq_qdq_hist_dt(*aciq_args(dtype, c=c)) == EINVAL, (c.num_bits, c.clip)
    out = (ctypes.c_int32 * 4)()
    for align in (3, 0, -2, 24):
        assert lib().cnnq_pc_route_qdq_hist_dt(2, 8, 16, dtype, align, 16, 1, out) == EINVAL
    assert lib().cnnq_pc_route_qdq_hist_dt(2, 8, 16, dtype, 16, 16, 1, None) == EINVAL
    for nbins in (0, 1, 3, 12, 257, 512):
        assert lib().cnnq_pc_route_qdq_hist_dt(2, 8, 16, dtype, 16, nbins, 1, out) == EINVAL, nbins
    if dtype == 0:
        return
    # cnnq_pc_groups' limits: a sample of 2^31 elements, 2^31 samples
    for N, C, HW in ((2, 1 << 16, 1 << 15), (1 << 31, 2, 4)):
        assert lib().cnnq_pc_groups(N, C, HW, 0) == ERANGE
        assert lib().cnnq_pc_route_qdq_hist_dt(N, C, HW, dtype, 16, 16, 1, out) == ERANGE
        assert lib().cnnq_pc_qdq_hist_dt(*table_args(dtype, N, C, HW)) == ERANGE
        assert lib().cnnq_pc_minmax_qdq_hist_dt(*minmax_args(dtype, N, C, HW)) == ERANGE
        assert lib().cnnq_pc_aciq_qdq_hist_dt(*aciq_args(dtype, N, C, HW)) == ERANGE


def test_float32_is_not_supported():
    """fp32 callers have cnnq_pc_qdq with hist and the single-launch kernels: CNNQ_ENOTSUP, nothing enqueued."""
    out = (ctypes.c_int32 * 4)()
    assert lib().cnnq_pc_route_qdq_hist_dt(2, 8, 16, 0, 16, 16, 1, out) == ENOTSUP
    assert lib().cnnq_pc_qdq_hist_dt(*table_args(0)) == ENOTSUP
    for allow in (0, 1, 2):
        assert lib().cnnq_pc_minmax_qdq_hist_dt(*minmax_args(0, allow=allow)) == ENOTSUP
    assert lib().cnnq_pc_aciq_qdq_hist_dt(*aciq_args(0)) == ENOTSUP


def test_the_plain_table_pass_keeps_its_contract():
    """cnnq_pc_qdq_dt: hist must be NULL on a half tensor."""
    p = ctypes.c_void_p
    for dtype in (1, 2):
        assert lib().cnnq_pc_qdq_dt(p(BAD), p(2 * BAD), dtype, 2, 8, 16, p(3 * BAD), None, p(4 * BAD), 0, None) == ENOTSUP
        assert lib().cnnq_pc_qdq_dt(p(BAD), p(2 * BAD), dtype, 2, 8, 16, p(3 * BAD), p(4 * BAD), None, 0, None) == ENOTSUP


GRID = [(N, C, HW) for N in (1, 2, 3, 5, 8, 64, 512) for C in (1, 3, 64, 256, 520, 2048)
        for HW in (1, 2, 7, 49, 98, 196, 784, 3136, 6400, 12544, 50176)]


def records(N, C, HW):
    return max(lib().cnnq_pc_groups(N, C, HW, 1), lib().cnnq_pc_groups(N, C, HW, 0))


def check_route(N, C, HW, dtype, align):
    out = (ctypes.c_int32 * 4)()
    G = records(N, C, HW)
    for allow in (0, 1, 2):
        for nbins in (4, 16, 256):
            assert lib().cnnq_pc_route_qdq_hist_dt(N, C, HW, dtype, align, nbins, allow, out) == 0, (N, C, HW)
            assert tuple(out) == HE.route(N, C, HW, align, allow, nbins, G), (N, C, HW, align, allow, nbins, tuple(out))
            if out[3] == 1:
                assert allow and out[0] >= 2 and N * HW <= HE.WHOLE_CAP
            if allow == 0:
                assert out[3] in (0, 2)
    return tuple(out)


@pytest.mark.parametrize('dtype', [1, 2])
@pytest.mark.parametrize('align', [2, 4, 16])
def test_route_equals_its_restatement(dtype, align):
    cases = HE.CASES + [HE.LONG_TILE]
    for N, C, HW in HE.CLASSES + [(s[0], s[1], s[2] * s[3]) for s, _, _ in cases] + GRID:
        w, S, cs, _ = check_route(N, C, HW, dtype, align)
        assert 1 <= S <= N and 1 <= cs <= max(1, HW // w) and C * S < 1 << 31


def test_the_gpu_tests_cases_reach_their_branches():
    assert len(HE.CLASSES) == 17
    out = (ctypes.c_int32 * 4)()
    for shape, offset, (W, S, cs, fits) in HE.CASES + [HE.LONG_TILE]:
        N, C, HW = shape[0], shape[1], shape[2] * shape[3]
        align = (2 * offset) & -(2 * offset) if offset else 16
        for dtype in (1, 2):
            for nbins in (4, 16, 256):
                assert lib().cnnq_pc_route_qdq_hist_dt(N, C, HW, dtype, align, nbins, 2, out) == 0
                assert tuple(out) == (W, S, cs, 1 if fits else 2), (shape, offset, tuple(out))
                assert lib().cnnq_pc_route_qdq_hist_dt(N, C, HW, dtype, align, nbins, 0, out) == 0
                assert tuple(out) == (W, S, cs, 2), (shape, offset, tuple(out))
    # the tile of the counting launch: the long one only on long rows that leave more than 2048 workgroups
    N, C, H, W = HE.LONG_TILE[0]
    assert HE.hist_elems(N, C, H * W) == 4 * HE.H_QDQ_ELEMS
    assert all(HE.hist_elems(s[0], s[1], s[2] * s[3]) == HE.H_QDQ_ELEMS for s, _, _ in HE.CASES)
    assert sum(C * S > 64 for (N, C, H, W), _, (_, S, _, _) in HE.CASES) >= 2          # replica tables shared
    assert any(S > 1 for _, _, (_, S, _, _) in HE.CASES) and any(cs > 1 for _, _, (_, _, cs, _) in HE.CASES)
    assert {W for _, _, (W, _, _, _) in HE.CASES} == {1, 2, 4, 8}


# ---- the quantizer's route
ATTS = [('clipping', 'no'), ('clipping', 'laplace'), ('clipping', 'gaus'), ('clipping', 'mix'), ('mtd_quant', True), ('kld', True),
        ('pcq_a', False), ('pcq_w', True), ('measure_entropy', True), ('measure_entropy', False), ('bit_alloc_act', True),
        ('bit_alloc_act', False), ('num_bits', 2), ('num_bits', 8), ('num_bits', 9)]
OBJECTS = [dict(pcq_act=True, measure_entropy=True), dict(pcq_act=True), dict(pcq_act=True, measure_entropy=True, clipping='laplace'),
           dict(pcq_act=True, measure_entropy=True, clipping='gaus', bit_alloc_act=True), dict(pcq_act=True, clipping='laplace'),
           dict(pcq_act=True, measure_entropy=True, bit_alloc_act=True), dict(pcq_act=True, measure_entropy=True, bits=8),
           dict(pcq_act=True, measure_entropy=True, bits=9), dict(pcq_act=True, measure_entropy=True, clipping='mix'),
           dict(pcq_act=True, measure_entropy=True, clipping='laplace', mtd_quant=True, bit_alloc_act=True),
           dict(pcq_act=True, measure_entropy=True, kld=True), dict(pcq_act=True, measure_entropy=True, pcq_weights=True),
           dict(measure_entropy=True), dict(measure_entropy=True, clipping='laplace')]


def tensors():
    return [act(), act(torch.float16), act(torch.float32), nhwc(), act(shape=(4, 8, 7, 7)), act(shape=(2, 8, 1, 1)), act(shape=(8, 16)),
            torch.zeros(2, 8, 4, 4, dtype=torch.bfloat16), FakeCuda(torch.zeros(2, 12, 4, 4, dtype=torch.bfloat16)[:, 2:9]),
            act(shape=(0, 8, 4, 4))]


def expected(q, att, t, stat_id, pending):
    """The conditions of the route, restated from DESIGN.md section 26's rows."""
    from cnn_quantization_amd import distributed as D
    half = (t.is_cuda and t.dtype in (torch.bfloat16, torch.float16) and t.dim() == 4 and t.is_contiguous() and t.numel() > 0)
    if not half or not (t.shape[2] > 1 or t.shape[3] > 1):
        return False
    common = (att('pcq_a') and att('measure_entropy') and att('num_bits') <= 8 and pending is None and not att('kld')
              and q.group is not False and D.world_size(q.group) == 1)
    if att('clipping') == 'no':
        return bool(common and not att('pcq_w') and not att('mtd_quant') and not (att('bit_alloc_act') and att('num_bits') <= 4))
    return bool(common and att('clipping') in ('laplace', 'gaus') and not att('mtd_quant'))


def test_route_over_the_attribute_grid():
    """Flag off: the parent's answer everywhere (no 'half_entropy', and the other routes as with the flag on wherever that is not
    'half_entropy' - where it is, the parent's answer is None: -me on a contiguous half tensor had no route).  Flag on: exactly the
    restated conditions; an override_att pair switches the route as the attribute would."""
    for kw in OBJECTS:
        for pending in (None, True):
            for stat_id in (None, 'layer0'):
                for t in tensors():
                    for pair in [None] + ATTS:
                        on, off = Q.quantizer(**kw), Q.quantizer(**kw)
                        assert on.half_entropy is False             # opt-in: the constructor leaves it off
                        on.half_entropy = True
                        on.fuse_bcorr = off.fuse_bcorr = pending
                        before = dict(vars(on))
                        a_on = on._asked(t, stat_id, on._att(pair))
                        a_off = off._asked(t, stat_id, off._att(pair))
                        assert vars(on) == before                   # nothing is stored on the object
                        assert a_off != 'half_entropy'
                        want = expected(on, on._att(pair), t, stat_id, pending)
                        assert (a_on == 'half_entropy') == want, (kw, pending, stat_id, tuple(t.shape), t.dtype, pair, a_on)
                        assert a_off == (None if want else a_on), (kw, pending, stat_id, pair, a_on, a_off)
                        if pair is not None:
                            # the attribute itself gives the same answer
                            key = {'num_bits': 'bits', 'pcq_a': 'pcq_act', 'pcq_w': 'pcq_weights'}.get(pair[0], pair[0])
                            direct = Q.quantizer(**dict(kw, **{key: pair[1]}))
                            direct.half_entropy, direct.fuse_bcorr = True, pending
                            assert direct._asked(t, stat_id) == a_on, (kw, pair)
    # the opt-ins of the other half routes do not open this one
    q = Q.quantizer(pcq_act=True, measure_entropy=True)
    q.half_dynamic = q.half_midtread = True
    assert q._asked(act()) is None
    # the earlier predicates keep their answers with the flag on
    q.half_entropy = True
    assert q._asked(act()) == 'half_entropy' and not q._half_native(act()) and not q._nhwc_entropy(act())
    assert q._asked(nhwc()) == 'nhwc_entropy'                                                  # channels_last comes first


def test_route_word_switch_and_exchange(monkeypatch):
    from cnn_quantization_amd import distributed as D, ops
    q = Q.quantizer(pcq_act=True, measure_entropy=True)
    qc = Q.quantizer(pcq_act=True, measure_entropy=True, clipping='laplace', bit_alloc_act=True)
    q.half_entropy = qc.half_entropy = True
    asked = lambda o: o._asked(act())
    assert asked(q) == asked(qc) == 'half_entropy'
    # a class of layer the route function sends back; every other word is native
    for word, want in ((0, None), (1, 'half_entropy'), (2, 'half_entropy')):
        monkeypatch.setattr(ops, '_entropy_half_native', lambda N, C, HW, dtype, nbins=256, word=word: word)
        assert asked(q) == want and asked(qc) == want
        monkeypatch.undo()
    # the bins reach it: 2^num_bits, 256 under bit allocation
    seen = []
    monkeypatch.setattr(ops, '_entropy_half_native', lambda *a: seen.append(a) or 2)
    assert asked(q) and asked(qc) and q._asked(act(), None, q._att(('num_bits', 8)))
    assert seen == [(2, 8, 16, torch.bfloat16, 16), (2, 8, 16, torch.bfloat16, 256), (2, 8, 16, torch.bfloat16, 256)]
    monkeypatch.undo()
    # replicated data, more than one process, the forced exchange
    q.group = False
    assert asked(q) is None
    q.group = None
    monkeypatch.setattr(D, 'world_size', lambda group=None: 2)
    assert asked(q) is None and asked(qc) is None
    monkeypatch.undo()
    monkeypatch.setattr(D, 'forced_exchange', lambda: True)
    assert asked(q) is None and asked(qc) is None
    monkeypatch.undo()
    # the switch
    monkeypatch.setenv('CNNQ_HALF_ENTROPY', '0')
    ops.reload_switches()
    try:
        assert asked(q) is None and asked(qc) is None
    finally:
        monkeypatch.delenv('CNNQ_HALF_ENTROPY')
        ops.reload_switches()
    assert asked(q) == asked(qc) == 'half_entropy'


def test_the_manager_opts_its_quantizers_in():
    from cnn_quantization_amd.inference import inference_quantization_manager as M
    src = inspect.getsource(M.TruncationOpManagerInference._load)
    assert 'half_entropy = True' in src


def test_route_is_asked_once_per_class(monkeypatch):
    from cnn_quantization_amd import ops
    seen = []
    real = lib().cnnq_pc_route_qdq_hist_dt

    class Lib:
        def cnnq_pc_route_qdq_hist_dt(self, *a):
            seen.append(a[:7])
            return real(*a)
    monkeypatch.setattr(ops.L, 'load', lambda: Lib())
    monkeypatch.setattr(ops, '_ENTROPY_HALF_NATIVE', {})
    for _ in range(3):
        for dtype in (torch.bfloat16, torch.float16):
            for nbins in (16, 256):
                assert ops._entropy_half_native(2, 12, 196, dtype, nbins) == HE.route(2, 12, 196, 16, 1, nbins, 1)[3]
                assert ops._entropy_half_native(512, 512, 49, dtype, nbins) == (2 if HE.native(512, 512, 49, nbins) else 0)
    assert seen == [(N, C, HW, code, 16, nbins, 1) for code in (1, 2) for nbins in (16, 256) for N, C, HW in ((2, 12, 196), (512, 512, 49))]


def test_ops_refuse_what_they_do_not_take():
    from cnn_quantization_amd import _lib as L, ops
    x = torch.zeros(2, 8, 4, 4, dtype=torch.bfloat16)
    with pytest.raises(L.CnnqError):
        ops.act_qdq_per_channel(x, 4, want_entropy=True)                                   # a CPU tensor: there is no CPU path
    with pytest.raises(L.CnnqError):
        ops.aciq_qdq_half(x, 4, want_entropy=True)
    with pytest.raises(L.CnnqError):
        ops.aciq_qdq_half(act(), 9, want_entropy=True)                                     # the factor tables end at 8 bits
