"""CPU-only checks of the channels_last route of config 3: the three entry points exist and their ctypes
prototypes match the header, bad arguments are refused before anything touches the device, the workspace covers the records of
every piece width, every (R, C, dtype, alignment) has a route whose slabs cover every row exactly once, and the quantizer's
dispatch conditions (shape, strides and attributes only)."""
import ctypes

import pytest
import torch

import _quantizer as Q
from test_channels_last_cpu import BAD, EINVAL, CHANNELS, cl, ctype_of, header_decls

ACIQ_FUNCS = ['cnnq_pc_aciq_nhwc_workspace', 'cnnq_pc_route_aciq_nhwc', 'cnnq_pc_aciq_qdq_nhwc']
NMOM, NDEV = 7, 2


def lib_and_cfg(**kw):
    from cnn_quantization_amd import _lib as L
    cfg = L.ParamsCfg()
    cfg.num_bits, cfg.positive, cfg.clip, cfg.pstd, cfg.bit_alloc, cfg.prior_is_b = 4, 0, 1, 0., 0, 0
    cfg.target, cfg.round_mode, cfg.direct_range = 4., 1, 0
    for k, v in kw.items():
        setattr(cfg, k, v)
    return L.load(), cfg


def test_entry_points_exist_and_prototypes_match_header():
    from cnn_quantization_amd import _lib as L
    lib = L.load()
    decls = header_decls()
    for name in ACIQ_FUNCS:
        assert hasattr(lib, name), name
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
    # the older route report is what it was: four words
    assert len(decls['cnnq_pc_route_nhwc'][1]) == 5 and decls['cnnq_pc_route_nhwc'][1][-1].endswith('out[4]')


@pytest.mark.parametrize('dtype, R, C', [(-1, 4, 8), (3, 4, 8), (1 << 20, 4, 8), (0, 0, 8), (1, 4, 0), (2, -3, 8), (0, 4, -1)])
def test_bad_geometry_is_einval(dtype, R, C):
    lib, cfg = lib_and_cfg()
    p = ctypes.c_void_p(BAD)
    out = (ctypes.c_int32 * 6)()
    assert lib.cnnq_pc_aciq_nhwc_workspace(R, C, dtype) == 0
    assert lib.cnnq_pc_route_aciq_nhwc(R, C, dtype, 16, out) == EINVAL
    assert lib.cnnq_pc_aciq_qdq_nhwc(p, p, dtype, R, C, ctypes.byref(cfg), p, p, p, p, None) == EINVAL


@pytest.mark.parametrize('dtype', [0, 1, 2])
def test_bad_pointers_and_configurations_are_einval(dtype):
    lib, cfg = lib_and_cfg()
    p = ctypes.c_void_p(BAD)
    ok = [p, p, dtype, 4, 8, ctypes.byref(cfg), p, p, p, p, None]
    for i in (0, 1, 5, 6, 7, 8):                            # x, y, cfg, ws, stats, qp
        a = list(ok)
        a[i] = None
        assert lib.cnnq_pc_aciq_qdq_nhwc(*a) == EINVAL, i
    a = list(ok)
    a[6] = ctypes.c_void_p(BAD + 4)                          # ws holds doubles
    assert lib.cnnq_pc_aciq_qdq_nhwc(*a) == EINVAL
    for kw in (dict(num_bits=0), dict(num_bits=33), dict(num_bits=9), dict(num_bits=9, clip=2), dict(clip=-1), dict(clip=4),
               dict(direct_range=1)):
        _, bad = lib_and_cfg(**kw)
        a = list(ok)
        a[5] = ctypes.byref(bad)
        assert lib.cnnq_pc_aciq_qdq_nhwc(*a) == EINVAL, kw
    # bit allocation keeps its bit table in diag
    _, ba = lib_and_cfg(bit_alloc=1)
    a = list(ok)
    a[5], a[9] = ctypes.byref(ba), None
    assert lib.cnnq_pc_aciq_qdq_nhwc(*a) == EINVAL
    out = (ctypes.c_int32 * 6)()
    assert lib.cnnq_pc_route_aciq_nhwc(4, 8, dtype, 3, out) == EINVAL
    assert lib.cnnq_pc_route_aciq_nhwc(4, 8, dtype, 0, out) == EINVAL
    assert lib.cnnq_pc_route_aciq_nhwc(4, 8, dtype, 16, None) == EINVAL


@pytest.mark.parametrize('dtype', [0, 1, 2])
@pytest.mark.parametrize('align', [2, 4, 8, 16])
def test_every_geometry_has_a_route_and_its_slabs_cover_the_rows(dtype, align):
    lib, _ = lib_and_cfg()
    esize = 4 if dtype == 0 else 2
    out, old = (ctypes.c_int32 * 6)(), (ctypes.c_int32 * 4)()
    for C in CHANNELS:
        for R in (1, 2, 49, 1000, 25088, 512 * 56 * 56, 512 * 112 * 112):
            assert lib.cnnq_pc_route_aciq_nhwc(R, C, dtype, align, out) == 0, (R, C)
            w, S, rpw, loads, wgs, native = list(out)
            assert w in (1, 2, 4, 8) and w * esize <= 16 and C % w == 0, (C, w)
            assert w == 1 or (w * esize) <= align, (C, align, w)
            assert C % (2 * w) or 2 * w * esize > min(align, 16), (C, align, w)
            assert native == 1 and wgs >= 1 and loads >= 1
            # slab s owns rows [s * rpw, min((s + 1) * rpw, R)): none empty, every row in exactly one
            assert S >= 1 and rpw >= 1 and (S - 1) * rpw < R <= S * rpw, (R, C, S, rpw)
            # a lane walks its slab in steps of RS rows: rpw is a whole number of steps
            P = C // w
            RS = 256 // min(P, 256)
            assert rpw == loads * RS, (R, C, rpw, loads, RS)
            assert S * C <= max(1 << 19, C), (R, C, S)
            # the statistics launches share the geometry of config 2's
            assert lib.cnnq_pc_route_nhwc(R, C, dtype, align, old) == 0
            assert (old[0], old[1], old[3], old[2]) == (w, S, loads, wgs)
            ws = lib.cnnq_pc_aciq_nhwc_workspace(R, C, dtype)
            assert ws >= (S * (NMOM + NDEV) + NMOM) * C * 8, (R, C, ws, S)


def quantizer(**kw):
    return Q.quantizer(**dict(dict(clipping='laplace', pcq_act=True, bit_alloc_act=True), **kw))


def test_dispatch_conditions_on_cpu_tensors():
    from cnn_quantization_amd import ops
    x = cl((2, 8, 4, 4)).bfloat16()
    x = x.as_strided(x.shape, (128, 1, 32, 8))
    assert ops._layout(x) == 'nhwc' and x.dtype == torch.bfloat16
    nchw = torch.zeros(2, 8, 4, 4, dtype=torch.bfloat16)
    q = quantizer()
    assert q._nhwc_aciq(x, 'laplace') and q._nhwc_aciq(x, 'gaus') and q._half_native(x)
    assert q._nhwc_aciq(x.float(), 'laplace')
    # everything else behaves as before: the fallback for half tensors, the copy route for fp32
    assert not q._nhwc_aciq(nchw, 'laplace') and not q._half_native(nchw)
    assert not q._nhwc_aciq(x, 'mix') and not q._nhwc_aciq(x, '2std') and not q._nhwc_aciq(x, 'no')
    assert not q._nhwc_aciq(x[:, 2:5], 'laplace') and not q._half_native(x[:, 2:5])          # not dense
    flat = torch.zeros(2, 8, 1, 1, dtype=torch.bfloat16)                                      # no spatial extent: per tensor
    assert not q._nhwc_aciq(flat, 'laplace') and not q._half_native(flat)
    assert not quantizer(measure_entropy=True)._half_native(x)
    assert not quantizer(mtd_quant=True)._half_native(x)
    assert not quantizer(kld=True)._half_native(x)
    assert not quantizer(pcq_act=False)._half_native(x)
    assert not quantizer(clipping='mix')._half_native(x)
    assert not q._half_native(x, ('clipping', 'mix')) and not q._half_native(x, ('measure_entropy', True))
    assert quantizer(clipping='no', bit_alloc_act=False)._half_native(x, ('clipping', 'gaus'))
    q.fuse_bcorr = True
    assert not q._nhwc_aciq(x, 'laplace') and not q._half_native(x)
    q.fuse_bcorr = None
    q.group = False                                                                             # replicated data: never this route
    assert not q._half_native(x)
    q.group = None
    # config 2's answers are what they were
    q2 = quantizer(clipping='no', bit_alloc_act=False)
    assert q2._half_native(x) and q2._half_native(nchw) and not quantizer(clipping='no')._half_native(x)


def test_nhwc_switch_turns_the_route_off():
    import os
    from cnn_quantization_amd import ops
    x = cl((2, 8, 4, 4))
    q = quantizer()
    old = os.environ.get('CNNQ_NHWC')
    try:
        os.environ['CNNQ_NHWC'] = '0'
        ops.reload_switches()
        assert not q._nhwc_aciq(x, 'laplace') and not q._half_native(x.bfloat16().as_strided(x.shape, x.stride()))
    finally:
        if old is None:
            os.environ.pop('CNNQ_NHWC', None)
        else:
            os.environ['CNNQ_NHWC'] = old
        ops.reload_switches()
    assert q._nhwc_aciq(x, 'laplace')


def test_op_refuses_other_clippings_and_cpu_tensors():
    from cnn_quantization_amd import _lib as L, ops
    for clip in ('no', 'mix', '2std', 'kld'):
        with pytest.raises(L.CnnqError):
            ops.aciq_qdq_nhwc(cl((2, 3, 4, 4)), 4, clip=clip)
    with pytest.raises(L.CnnqError):
        ops.aciq_qdq_nhwc(cl((2, 3, 4, 4)), 4)
