"""CPU-only checks of `-sm collect` on channels_last storage: the three entry points exist and their
ctypes prototypes match the header, bad arguments are refused before anything touches the device, the workspace covers the
documented records, the route function over a grid of (R, C, dtype, alignment), the manager's routing predicate as a truth
table - and that an fp32 evaluation of the kernels' formulas keeps the tiers of tests/test_channels_last_collect_gpu.py on
that file's inputs (were it not so, the inputs would be wrong, not the tiers)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ['cnnq_pc_stats_nhwc_workspace', 'cnnq_pc_route_stats_nhwc', 'cnnq_pc_stats_nhwc']
BAD = 0x1000   # a non-null pointer value that is never dereferenced: the argument checks come first
EINVAL, ERANGE = -1, -2
NMOM, NDEV, TPB = 7, 2, 256
CL_MM_ELEMS, CL_MM_MAX_WGS, CL_PMM_MAX = 65536, 2048, 1 << 19
CHANNELS = list(range(1, 34)) + [48, 63, 64, 96, 128, 256, 512, 1000, 1024, 2048]


def lib():
    from cnn_quantization_amd import _lib as L
    return L.load()


def header_decls():
    text = open(os.path.join(ROOT, 'include', 'cnnq_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return {name: (ret, [a.strip() for a in args.split(',')])
            for ret, name, args in re.findall(r'\b(int|size_t)\s+(cnnq_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', text)}


def ctype_of(decl):
    if decl.endswith(']'):                                                          # an array parameter: a pointer
        return 'ptr'
    decl = re.sub(r'\s*\b[A-Za-z_][A-Za-z_0-9]*$', '', decl.strip())                 # drop the parameter name
    if '*' in decl:
        return 'ptr'
    return {'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'size_t': ctypes.c_size_t}[decl.replace('const ', '')]


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


def stats_args(dtype=0, R=4, C=8):
    p = ctypes.c_void_p(BAD)
    return [p, dtype, R, C, 1, 1, 1, p, p, p, None]                  # x, dtype, R, C, need_b, need_kurt, need_relu, ws, mom, stats, stream


@pytest.mark.parametrize('dtype, R, C', [(-1, 4, 8), (3, 4, 8), (1 << 20, 4, 8), (0, 0, 8), (1, 4, 0), (2, -3, 8), (0, 4, -1),
                                         (0, 4, (1 << 26) + 1)])
def test_bad_geometry_is_einval(dtype, R, C):
    out = (ctypes.c_int32 * 4)()
    assert lib().cnnq_pc_stats_nhwc_workspace(R, C, dtype) == 0
    assert lib().cnnq_pc_route_stats_nhwc(R, C, dtype, 16, out) == EINVAL
    assert lib().cnnq_pc_stats_nhwc(*stats_args(dtype, R, C)) == EINVAL


@pytest.mark.parametrize('dtype', [0, 1, 2])
def test_bad_pointers_are_einval_and_huge_slabs_erange(dtype):
    for i in (0, 7, 9):                                     # x, ws, stats
        a = stats_args(dtype)
        a[i] = None
        assert lib().cnnq_pc_stats_nhwc(*a) == EINVAL, i
    for i in (7, 8):                                        # ws and mom hold doubles
        a = stats_args(dtype)
        a[i] = ctypes.c_void_p(BAD + 4)
        assert lib().cnnq_pc_stats_nhwc(*a) == EINVAL, i
    out = (ctypes.c_int32 * 4)()
    assert lib().cnnq_pc_route_stats_nhwc(4, 8, dtype, 3, out) == EINVAL
    assert lib().cnnq_pc_route_stats_nhwc(4, 8, dtype, 0, out) == EINVAL
    assert lib().cnnq_pc_route_stats_nhwc(4, 8, dtype, 16, None) == EINVAL
    # the 2^31 checks of the plan: an element-wise grid of 2^31 workgroups (512 column blocks), and a slab of 2^31 rows (one
    # channel: at most 2048 slabs)
    assert lib().cnnq_pc_route_stats_nhwc(1 << 40, 1 << 19, dtype, 16, out) == ERANGE
    assert lib().cnnq_pc_stats_nhwc(*stats_args(dtype, 1 << 40, 1 << 19)) == ERANGE
    assert lib().cnnq_pc_route_stats_nhwc(1 << 45, 1, dtype, 16, out) == ERANGE
    assert lib().cnnq_pc_stats_nhwc(*stats_args(dtype, 1 << 45, 1)) == ERANGE


def geo(R, C, w):
    """The statistics geometry of csrc/cnnq_nhwc.hip.h (cl_geo_mm), restated: (slabs, rows per slab)."""
    P = C // w
    CP = min(P, TPB)
    RS, nb = TPB // CP, -(-P // CP)
    rstep = -(-R // RS)
    steps = -(-CL_MM_ELEMS // (CP * w * RS))
    s = -(-rstep // steps)
    if s * nb > CL_MM_MAX_WGS:
        s = -(-CL_MM_MAX_WGS // nb)
    s = max(1, min(s, max(1, CL_PMM_MAX // C)))
    rpw = -(-rstep // s) * RS
    return -(-R // rpw), rpw


@pytest.mark.parametrize('dtype', [0, 1, 2])
@pytest.mark.parametrize('align', [2, 4, 8, 16])
def test_route_and_workspace_over_a_grid(dtype, align):
    out, ref = (ctypes.c_int32 * 4)(), (ctypes.c_int32 * 6)()
    esize = 4 if dtype == 0 else 2
    for C in CHANNELS:
        for R in (1, 2, 49, 98, 1000, 4096, 4097, 25088, 512 * 56 * 56, 512 * 112 * 112):
            assert lib().cnnq_pc_route_stats_nhwc(R, C, dtype, align, out) == 0, (R, C)
            w, S, rpw, native = out
            # the widest piece of at most 16 bytes that divides C and the alignment
            want = next((v for v in (8, 4, 2) if v * esize <= 16 and C % v == 0 and align % (v * esize) == 0), 1)
            assert w == want, (R, C, w, want)
            assert (S, rpw) == geo(R, C, w) and (S - 1) * rpw < R <= S * rpw, (R, C, S, rpw)
            assert native == 1
            # config 3's plan: the same records serve both
            assert lib().cnnq_pc_route_aciq_nhwc(R, C, dtype, align, ref) == 0
            assert [w, S, rpw] == list(ref)[:3]
            # ws, doubles: part[S][NMOM][C], mom[NMOM][C], part2[S][NDEV][C] for the widest slab count over the piece widths
            ws = lib().cnnq_pc_stats_nhwc_workspace(R, C, dtype)
            smax = max(geo(R, C, v)[0] for v in (8, 4, 2, 1) if v * esize <= 16 and C % v == 0)
            assert ws == (smax * (NMOM + NDEV) + NMOM) * C * 8, (R, C, ws, smax)
            assert ws == lib().cnnq_pc_aciq_nhwc_workspace(R, C, dtype)


# ---- the manager's predicate
class FakeManager:
    def __init__(self, batch_avg=False, collect_err=False, group=None):
        self.batch_avg, self.collect_err, self.group = batch_avg, collect_err, group


def nhwc(dtype=torch.bfloat16, shape=(2, 8, 4, 4)):
    n, c, h, w = shape
    return torch.zeros(n * c * h * w, dtype=dtype).as_strided(shape, (h * w * c, 1, w * c, c))


def test_predicate_truth_table(monkeypatch):
    from cnn_quantization_amd import distributed as D, ops
    from cnn_quantization_amd.inference.statistic_manager_perchannel import collects_native_nhwc as native
    x = nhwc()
    assert ops._layout(x) == 'nhwc'
    for dtype in (torch.float32, torch.bfloat16, torch.float16):
        assert native(FakeManager(), nhwc(dtype))
    # the layout
    assert not native(FakeManager(), torch.zeros(2, 8, 4, 4, dtype=torch.bfloat16))            # contiguous
    assert not native(FakeManager(), x[:, 2:5])                                                 # not dense
    assert not native(FakeManager(), nhwc(shape=(2, 8, 1, 1)))                                  # dense in both layouts
    assert not native(FakeManager(), torch.zeros(8, 16))                                        # not 4-D
    assert not native(FakeManager(), nhwc(torch.float64)) and not native(FakeManager(), None)
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
    monkeypatch.setattr(ops, '_stats_nhwc_native', lambda R, C, dtype: False)
    assert not native(FakeManager(), x)
    monkeypatch.undo()
    # the A/B switch
    old = os.environ.get('CNNQ_NHWC')
    try:
        os.environ['CNNQ_NHWC'] = '0'
        ops.reload_switches()
        assert not native(FakeManager(), x)
    finally:
        if old is None:
            os.environ.pop('CNNQ_NHWC', None)
        else:
            os.environ['CNNQ_NHWC'] = old
        ops.reload_switches()
    assert native(FakeManager(), x)


def test_route_is_asked_once_per_class(monkeypatch):
    from cnn_quantization_amd import ops
    asked = []
    real = lib().cnnq_pc_route_stats_nhwc

    class Lib:
        def cnnq_pc_route_stats_nhwc(self, *a):
            asked.append(a[:3])
            return real(*a)
    monkeypatch.setattr(ops.L, 'load', lambda: Lib())
    monkeypatch.setattr(ops, '_STATS_NHWC_NATIVE', {})
    for _ in range(3):
        assert ops._stats_nhwc_native(98, 12, torch.bfloat16) and ops._stats_nhwc_native(98, 12, torch.float32)
    assert asked == [(98, 12, 1), (98, 12, 0)]


def test_op_and_manager_leave_other_tensors_where_they_were():
    from cnn_quantization_amd import _lib as L, ops
    with pytest.raises(L.CnnqError):
        ops.pc_stats_nhwc(nhwc(torch.float32))                      # a CPU tensor: there is no CPU path
    with pytest.raises(L.CnnqError):
        ops.pc_stats_nhwc(torch.zeros(8, 16))


# ---- the inputs of the GPU tests hold the tiers under an fp32 evaluation of the kernels' formulas
def values(shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    C = shape[1]
    return torch.randn(shape, generator=g) * (0.2 + 3 * torch.rand(1, C, 1, 1, generator=g)) + torch.randn(1, C, 1, 1, generator=g)


def fold4(v, exact):
    """Per-channel sums of v [C, R] (fp32): fp64 element by element, or four-row fp32 partials folded into fp64."""
    if exact:
        return v.double().sum(1)
    n = v.shape[1] // 4 * 4
    q = v[:, :n].reshape(v.shape[0], -1, 4)
    return ((q[:, :, 0] + q[:, :, 1]) + (q[:, :, 2] + q[:, :, 3])).double().sum(1) + v[:, n:].double().sum(1)


def table32(t):
    """The seven rows of t [C, R] (fp32 values) as the kernels form them: fp32 per element, fp32 four-row partials above 4096
    rows, fp64 merges, fp32 rows."""
    R = t.shape[1]
    exact = R <= 4096
    s, ss = fold4(t, exact), (t.double() ** 2).sum(1) if exact else fold4(t * t, False)
    mean64 = s / R
    mean = mean64.float()
    std = ((ss - s * mean64) / (R - 1)).clamp(min=0).sqrt().float()
    r = t.clamp(min=0)
    rs, rss = fold4(r, exact), (r.double() ** 2).sum(1) if exact else fold4(r * r, False)
    std_pos = ((rss - rs * (rs / R)) / (R - 1)).clamp(min=0).sqrt().float()
    d = t - mean[:, None]
    b = (fold4(d.abs(), exact) / R).float()
    z = d * (1.0 / std)[:, None]
    z2 = z * z
    kurt = (fold4(z2 * z2, exact) / R - 3.).float()
    return mean, std, b, kurt, std_pos


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16, torch.float16], ids=['f32', 'bf16', 'f16'])
def test_fp32_evaluation_keeps_the_tiers_on_the_gpu_tests_inputs(dtype):
    cases = [((8, C, 28, 28), C + off + 28) for C, off in ((6, 0), (10, 0), (12, 0), (20, 0), (64, 2), (64, 4), (64, 0), (7, 0))]
    cases += [((3, C, 56, 56), C + off + 56) for C, off in ((6, 0), (64, 0), (7, 0))]
    cases += [((3, C, 14, 14), C + off + 14) for C, off in ((6, 0), (64, 2), (7, 0))] + [((2, C, 7, 7), C + 7) for C in (6, 64, 7)]
    cases += [((3, 10, 14, 14), 17), ((8, 12, 28, 28), 17), ((4, 12, 14, 14), 30), ((4, 12, 14, 14), 31)]
    for shape, seed in cases:
        C = shape[1]
        t = values(shape, seed).to(dtype).float().transpose(0, 1).reshape(C, -1)
        mean, std, b, kurt, std_pos = table32(t)
        t64 = t.double()
        m64, s64 = t64.mean(1), t64.std(1, unbiased=True)
        m32, s32 = m64.float().double(), s64.float().double()
        np.testing.assert_allclose(mean.double(), m64, rtol=2e-6, atol=1e-7)
        np.testing.assert_allclose(std.double(), s64, rtol=2e-6)
        np.testing.assert_allclose(b.double(), (t64 - m32[:, None]).abs().mean(1), rtol=3e-6, atol=1e-7)
        np.testing.assert_allclose(std_pos.double(), t64.clamp(min=0).std(1, unbiased=True), rtol=3e-6, atol=1e-7)
        np.testing.assert_allclose(kurt.double(), (((t64 - m32[:, None]) / s32[:, None]) ** 4).mean(1) - 3, rtol=2e-4, atol=2e-4)
