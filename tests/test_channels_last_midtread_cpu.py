"""CPU-only checks of the channels_last route of config 5: the three entry points exist and their ctypes
prototypes match the header, bad arguments are refused before anything touches the device, the statistics launches share
config 3's plan, the workspace covers their records, and the quantizer's dispatch conditions (shape, strides and attributes
only) - with _half_native's answers unchanged next to them."""
import ctypes
import os

import pytest
import torch

import _quantizer as Q
from test_channels_last_cpu import BAD, EINVAL, CHANNELS, cl, ctype_of, header_decls

MT_FUNCS = ['cnnq_pc_route_midtread_nhwc', 'cnnq_pc_midtread_qdq_nhwc', 'cnnq_pc_midtread_nhwc']
NMOM, NDEV = 7, 2
CL_QDQ_ELEMS, CL_MT_HIST_ELEMS = 8192, 65536


def lib():
    from cnn_quantization_amd import _lib as L
    return L.load()


def test_entry_points_exist_and_prototypes_match_header():
    from cnn_quantization_amd import _lib as L
    decls = header_decls()
    for name in MT_FUNCS:
        assert hasattr(lib(), name), name
        ret, args = decls[name]
        res, argtypes = L.SIGNATURES[name]
        assert res is ctypes.c_int and ret == 'int', name
        assert len(args) == len(argtypes), name
        for a, t in zip(args, argtypes):
            want = ctypes.c_double if a.startswith('double ') else ctype_of(a)
            if want == 'ptr':
                assert t is ctypes.c_void_p or issubclass(t, ctypes._Pointer), (name, a, t)
            else:
                assert t is want, (name, a, t)


def table_args(dtype=0, R=4, C=8):
    p = ctypes.c_void_p(BAD)
    return [p, ctypes.c_void_p(BAD + 0x1000), dtype, R, C, p, p, None]                    # x, y, dtype, R, C, mt, hist, stream


def dynamic_args(dtype=0, R=4, C=8, target=4.0):
    p = ctypes.c_void_p(BAD)
    # x, y, dtype, R, C, target, sym, tables, ntab, ws, stats, mt, hist, stream
    return [p, ctypes.c_void_p(BAD + 0x1000), dtype, R, C, target, 1, p, 101, p, p, p, p, None]


@pytest.mark.parametrize('dtype, R, C', [(-1, 4, 8), (3, 4, 8), (1 << 20, 4, 8), (0, 0, 8), (1, 4, 0), (2, -3, 8), (0, 4, -1)])
def test_bad_geometry_is_einval(dtype, R, C):
    out = (ctypes.c_int32 * 6)()
    for hist in (0, 1):
        assert lib().cnnq_pc_route_midtread_nhwc(R, C, dtype, 16, hist, out) == EINVAL
    assert lib().cnnq_pc_midtread_qdq_nhwc(*table_args(dtype, R, C)) == EINVAL
    assert lib().cnnq_pc_midtread_nhwc(*dynamic_args(dtype, R, C)) == EINVAL


@pytest.mark.parametrize('dtype', [0, 1, 2])
def test_bad_pointers_and_targets_are_einval(dtype):
    p = ctypes.c_void_p(BAD)
    for i in (0, 1, 5):                                     # x, y, mt
        a = table_args(dtype)
        a[i] = None
        assert lib().cnnq_pc_midtread_qdq_nhwc(*a) == EINVAL, i
    a = table_args(dtype)
    a[6] = ctypes.c_void_p(BAD + 4)                         # hist holds 64-bit words
    assert lib().cnnq_pc_midtread_qdq_nhwc(*a) == EINVAL
    a = table_args(dtype)
    a[1] = p                                                # x == y
    assert lib().cnnq_pc_midtread_qdq_nhwc(*a) == EINVAL
    for i in (0, 1, 7, 9, 10, 11):                          # x, y, tables, ws, stats, mt
        a = dynamic_args(dtype)
        a[i] = None
        assert lib().cnnq_pc_midtread_nhwc(*a) == EINVAL, i
    for i in (9, 12):                                       # ws holds doubles, hist 64-bit words
        a = dynamic_args(dtype)
        a[i] = ctypes.c_void_p(BAD + 4)
        assert lib().cnnq_pc_midtread_nhwc(*a) == EINVAL, i
    a = dynamic_args(dtype)
    a[1] = p
    assert lib().cnnq_pc_midtread_nhwc(*a) == EINVAL
    a = dynamic_args(dtype)
    a[8] = 1                                                # an interpolation table has two entries at least
    assert lib().cnnq_pc_midtread_nhwc(*a) == EINVAL
    for target in (float('nan'), float('inf'), float('-inf')):
        assert lib().cnnq_pc_midtread_nhwc(*dynamic_args(dtype, target=target)) == EINVAL, target
    out = (ctypes.c_int32 * 6)()
    assert lib().cnnq_pc_route_midtread_nhwc(4, 8, dtype, 3, 0, out) == EINVAL
    assert lib().cnnq_pc_route_midtread_nhwc(4, 8, dtype, 0, 1, out) == EINVAL
    assert lib().cnnq_pc_route_midtread_nhwc(4, 8, dtype, 16, 1, None) == EINVAL


@pytest.mark.parametrize('dtype', [0, 1, 2])
@pytest.mark.parametrize('align', [2, 4, 8, 16])
def test_plan_is_config_3s_for_the_statistics_and_the_workspace_covers_it(dtype, align):
    out, hout, ref = (ctypes.c_int32 * 6)(), (ctypes.c_int32 * 6)(), (ctypes.c_int32 * 6)()
    for C in CHANNELS:
        for R in (1, 2, 49, 1000, 25088, 512 * 56 * 56, 512 * 112 * 112):
            assert lib().cnnq_pc_route_aciq_nhwc(R, C, dtype, align, ref) == 0
            assert lib().cnnq_pc_route_midtread_nhwc(R, C, dtype, align, 0, out) == 0, (R, C)
            assert lib().cnnq_pc_route_midtread_nhwc(R, C, dtype, align, 1, hout) == 0, (R, C)
            # the same W, slabs, rows per slab and loads per lane; without the histogram config 3's Q/DQ grid; native
            assert list(out) == list(ref), (R, C, list(out), list(ref))
            assert list(hout)[:4] == list(ref)[:4] and hout[5] == 1
            w, S = out[0], out[1]
            # the Q/DQ grids: column blocks x row slabs of whole row steps, at least the geometry's elements per workgroup
            P = C // w
            CP = min(P, 256)
            RS, nb = 256 // CP, -(-P // CP)
            for wgs, per in ((out[4], CL_QDQ_ELEMS), (hout[4], CL_MT_HIST_ELEMS)):
                steps = -(-per // (CP * w * RS))
                slabs = -(-(-(-R // RS)) // steps)
                assert wgs % nb == 0 and 1 <= wgs // nb <= slabs, (R, C, wgs, nb, slabs)
            assert hout[4] <= out[4]
            ws = lib().cnnq_pc_aciq_nhwc_workspace(R, C, dtype)
            assert ws >= (S * (NMOM + NDEV) + NMOM) * C * 8, (R, C, ws, S)


def quantizer(**kw):
    return Q.quantizer(**dict(dict(clipping='laplace', pcq_act=True, bit_alloc_act=True, bit_alloc_target_act=5.3, measure_entropy=True, mtd_quant=True), **kw))


def nhwc_bf16():
    x = cl((2, 8, 4, 4)).bfloat16()
    x = x.as_strided(x.shape, (128, 1, 32, 8))
    return x


def test_dispatch_conditions_on_cpu_tensors():
    from cnn_quantization_amd import ops
    x = nhwc_bf16()
    assert ops._layout(x) == 'nhwc' and x.dtype == torch.bfloat16
    nchw = torch.zeros(2, 8, 4, 4, dtype=torch.bfloat16)
    q = quantizer()
    assert q._nhwc_midtread(x) and q._nhwc_midtread(x.float().as_strided(x.shape, x.stride()))
    assert quantizer(measure_entropy=False)._nhwc_midtread(x) and quantizer(clipping='gaus')._nhwc_midtread(x)
    # _half_native keeps every answer it gave: never for mid-tread
    assert not q._half_native(x) and not quantizer(measure_entropy=False)._half_native(x)
    # every condition
    assert not quantizer(mtd_quant=False)._nhwc_midtread(x)
    assert not quantizer(clipping='no')._nhwc_midtread(x)
    assert not quantizer(pcq_act=False)._nhwc_midtread(x)
    assert not quantizer(kld=True)._nhwc_midtread(x)
    assert not q._nhwc_midtread(nchw) and not q._half_native(nchw)
    assert not q._nhwc_midtread(x[:, 2:5]) and not q._half_native(x[:, 2:5])                   # not dense
    flat = torch.zeros(2, 8, 1, 1, dtype=torch.bfloat16)                                        # no spatial extent: per tensor
    assert not q._nhwc_midtread(flat)
    assert not q._nhwc_midtread(torch.zeros(8, 16, dtype=torch.bfloat16))                       # not 4-D
    # __call__'s override pair is looked at (through _att, the lookup the predicates share)
    assert not q._nhwc_midtread(x, q._att(('clipping', 'no'))) and not q._nhwc_midtread(x, q._att(('mtd_quant', False)))
    assert not q._nhwc_midtread(x, q._att(('kld', True))) and not q._nhwc_midtread(x, q._att(('pcq_a', False)))
    qn = quantizer(mtd_quant=False)
    assert qn._nhwc_midtread(x, qn._att(('mtd_quant', True))) and q._nhwc_midtread(x, q._att(('num_bits', 8)))
    q.fuse_bcorr = True                                                                         # a pending bias correction
    assert not q._nhwc_midtread(x) and not q._half_native(x)
    q.fuse_bcorr = None
    q.group = False                                                                             # replicated data: never this route
    assert not q._nhwc_midtread(x)
    q.group = None
    assert q._nhwc_midtread(x)
    # the answers of the other configurations are what they were
    q3 = quantizer(mtd_quant=False, measure_entropy=False)
    assert q3._half_native(x) and not q3._nhwc_midtread(x) and not q3._half_native(nchw)
    q2 = quantizer(mtd_quant=False, measure_entropy=False, clipping='no', bit_alloc_act=False)
    assert q2._half_native(x) and q2._half_native(nchw) and not q2._nhwc_midtread(x)


def test_forced_exchange_and_the_nhwc_switch_turn_the_route_off(monkeypatch):
    from cnn_quantization_amd import distributed as D, ops
    x = nhwc_bf16()
    q = quantizer()
    monkeypatch.setattr(D, 'forced_exchange', lambda: True)
    assert not q._nhwc_midtread(x)
    monkeypatch.undo()
    assert q._nhwc_midtread(x)
    old = os.environ.get('CNNQ_NHWC')
    try:
        os.environ['CNNQ_NHWC'] = '0'
        ops.reload_switches()
        assert not q._nhwc_midtread(x) and not q._half_native(x)
    finally:
        if old is None:
            os.environ.pop('CNNQ_NHWC', None)
        else:
            os.environ['CNNQ_NHWC'] = old
        ops.reload_switches()
    assert q._nhwc_midtread(x)


def test_op_refuses_cpu_tensors():
    from cnn_quantization_amd import _lib as L, ops
    with pytest.raises(L.CnnqError):
        ops.mid_tread_qdq_nhwc(cl((2, 3, 4, 4)), 4, True)
