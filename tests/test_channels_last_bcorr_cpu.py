"""CPU-only checks of the channels_last bias correction: the two entry points exist and their ctypes
prototypes match the header, bad arguments are refused before anything touches the device, the workspace holds the records of
every piece width, and the quantizer's dispatch conditions (shape, strides and attributes only) - including that without a
stat_id every answer is what it was."""
import ctypes

import pytest
import torch

import _quantizer as Q
from test_channels_last_cpu import BAD, EINVAL, CHANNELS, cl, ctype_of, header_decls

BCORR_FUNCS = ['cnnq_pc_qdq_bcorr_nhwc_workspace', 'cnnq_pc_qdq_bcorr_nhwc']


def lib():
    from cnn_quantization_amd import _lib as L
    return L.load()


def test_entry_points_exist_and_prototypes_match_header():
    from cnn_quantization_amd import _lib as L
    decls = header_decls()
    for name in BCORR_FUNCS:
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


@pytest.mark.parametrize('dtype, R, C', [(-1, 4, 8), (3, 4, 8), (1 << 20, 4, 8), (0, 0, 8), (1, 4, 0), (2, -3, 8), (0, 4, -1),
                                         (0, 4, (1 << 26) + 1)])
def test_bad_geometry_is_einval(dtype, R, C):
    p = ctypes.c_void_p(BAD)
    q = ctypes.c_void_p(BAD + 0x100000)
    assert lib().cnnq_pc_qdq_bcorr_nhwc_workspace(R, C, dtype) == 0
    assert lib().cnnq_pc_qdq_bcorr_nhwc(p, q, dtype, R, C, p, 1, p, p, p, None) == EINVAL


@pytest.mark.parametrize('dtype', [0, 1, 2])
def test_bad_pointers_are_einval(dtype):
    p = ctypes.c_void_p(BAD)
    ok = [p, ctypes.c_void_p(BAD + 0x100000), dtype, 4, 8, p, 1, p, None, p, None]
    for i in (0, 1, 5, 7, 9):                               # x, y, qp, ws, bias
        a = list(ok)
        a[i] = None
        assert lib().cnnq_pc_qdq_bcorr_nhwc(*a) == EINVAL, i
    a = list(ok)
    a[1] = a[0]                                             # x == y
    assert lib().cnnq_pc_qdq_bcorr_nhwc(*a) == EINVAL
    for i in (7, 8):                                        # ws and sums hold doubles
        a = list(ok)
        a[i] = ctypes.c_void_p(BAD + 4)
        assert lib().cnnq_pc_qdq_bcorr_nhwc(*a) == EINVAL, i


@pytest.mark.parametrize('dtype', [0, 1, 2])
def test_workspace_holds_the_records_of_every_piece_width(dtype):
    out = (ctypes.c_int32 * 6)()
    for C in CHANNELS:
        for R in (1, 2, 49, 1000, 25088, 512 * 56 * 56, 512 * 112 * 112):
            ws = lib().cnnq_pc_qdq_bcorr_nhwc_workspace(R, C, dtype)
            for align in (2, 4, 8, 16):
                assert lib().cnnq_pc_route_aciq_nhwc(R, C, dtype, align, out) == 0        # the sums share config 3's slabs
                assert ws >= out[1] * 3 * C * 8, (R, C, align, ws, out[1])


def quantizer(**kw):
    return Q.quantizer(**dict(dict(clipping='laplace', pcq_act=True, bit_alloc_act=True, bcorr_act=True), **kw))


def nhwc_bf16():
    x = cl((2, 8, 4, 4)).bfloat16()
    return x.as_strided(x.shape, (128, 1, 32, 8))


def test_route_conditions_on_cpu_tensors():
    from cnn_quantization_amd import ops
    x = nhwc_bf16()
    assert ops._layout(x) == 'nhwc' and x.dtype == torch.bfloat16
    nchw = torch.zeros(2, 8, 4, 4, dtype=torch.bfloat16)
    q = quantizer()
    # no pending request: never this route
    assert not q._nhwc_bcorr(x, 'laplace', 'id') and q._half_native(x, None, 'id')           # (config 3's own route)
    for flag in (True, False):                                                                  # the relu-first flag, either value
        q.fuse_bcorr = flag
        for clip in ('laplace', 'gaus', 'no'):
            assert q._nhwc_bcorr(x, clip, 'id') and q._nhwc_bcorr(x.float(), clip, 'id')
        assert q._half_native(x, None, 'id') and q._half_native(x, ('clipping', 'no'), 'id')
        assert not q._nhwc_bcorr(x, 'mix', 'id') and not q._nhwc_bcorr(x, '2std', 'id')
        assert not q._half_native(x, ('clipping', 'mix'), 'id')
        assert not q._nhwc_bcorr(nchw, 'laplace', 'id') and not q._half_native(nchw, None, 'id')
        assert not q._nhwc_bcorr(x[:, 2:5], 'laplace', 'id') and not q._half_native(x[:, 2:5], None, 'id')      # not dense
        flat = torch.zeros(2, 8, 1, 1, dtype=torch.bfloat16)                                   # no spatial extent: per tensor
        assert not q._nhwc_bcorr(flat, 'laplace', 'id')
        for att in (('measure_entropy', True), ('mtd_quant', True), ('kld', True), ('pcq_a', False)):
            assert not q._half_native(x, att, 'id'), att
            assert not q._nhwc_bcorr(x, 'laplace', 'id', lambda k, att=att: att[1] if k == att[0] else getattr(q, k)), att
        # min/max with per-channel weights is the weight branch of the dispatch
        assert not q._nhwc_bcorr(x, 'no', 'id', lambda k: True if k == 'pcq_w' else getattr(q, k))
    q.group = False                                                                             # replicated data
    assert not q._nhwc_bcorr(x, 'laplace', 'id') and not q._half_native(x, None, 'id')
    q.group = None
    q2 = quantizer(clipping='no', bit_alloc_act=False)
    q2.fuse_bcorr = True
    assert q2._nhwc_bcorr(x, 'no', 'id') and q2._half_native(x, None, 'id')
    q3 = quantizer(clipping='no')                                                               # with bit allocation too
    q3.fuse_bcorr = True
    assert q3._half_native(x, None, 'id') and not q3._half_native(x)


def test_without_stat_id_every_answer_is_unchanged():
    x = nhwc_bf16()
    nchw = torch.zeros(2, 8, 4, 4, dtype=torch.bfloat16)
    for kw in (dict(), dict(clipping='gaus'), dict(clipping='no', bit_alloc_act=False), dict(clipping='no'),
               dict(measure_entropy=True), dict(mtd_quant=True), dict(kld=True), dict(pcq_act=False)):
        q = quantizer(**kw)
        for pending in (None, True, False):
            q.fuse_bcorr = pending
            for t in (x, x.float(), nchw):
                assert not q._nhwc_bcorr(t, q.clipping, None)
                # what the parent's _half_native computes, restated
                if q.kld:
                    want = False
                elif q.clipping != 'no':
                    want = not q.mtd_quant and q._nhwc_aciq(t, q.clipping)
                elif q.pcq_a:
                    want = (not q.mtd_quant and not q.measure_entropy and pending is None
                            and not (q.bit_alloc_act and q.num_bits <= 4))
                else:
                    want = True
                assert q._half_native(t) == want and q._half_native(t, None) == want and q._half_native(t, None, None) == want
            # a pending request keeps config 3's route closed, as the existing tests pin
            if pending is not None:
                assert not q._nhwc_aciq(x, 'laplace') and not q._nhwc_aciq(x, 'laplace', None)


def test_nhwc_switch_turns_the_route_off():
    import os
    from cnn_quantization_amd import ops
    x = nhwc_bf16()
    q = quantizer()
    q.fuse_bcorr = True
    old = os.environ.get('CNNQ_NHWC')
    try:
        os.environ['CNNQ_NHWC'] = '0'
        ops.reload_switches()
        assert not q._nhwc_bcorr(x, 'laplace', 'id') and not q._half_native(x, None, 'id')
    finally:
        if old is None:
            os.environ.pop('CNNQ_NHWC', None)
        else:
            os.environ['CNNQ_NHWC'] = old
        ops.reload_switches()
    assert q._nhwc_bcorr(x, 'laplace', 'id')


def test_op_refuses_cpu_tensors():
    from cnn_quantization_amd import _lib as L, ops
    with pytest.raises(L.CnnqError):
        ops.qdq_bias_corrected_nhwc(cl((2, 3, 4, 4)), torch.zeros(3, 3), True)
