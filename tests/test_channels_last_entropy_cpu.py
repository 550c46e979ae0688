"""CPU-only checks of the channels_last route of the uniform Q/DQ that counts its codes (-me): the four entry
points exist and their ctypes prototypes match the header, bad arguments are refused before anything touches the device, the
route function agrees with config 2's piece width and reports the counting launch, and the quantizer's dispatch condition
(shape, strides and attributes only) - with the four earlier predicates' answers unchanged next to it."""
import ctypes
import os

import pytest
import torch

import _quantizer as Q
from test_channels_last_cpu import BAD, EINVAL, CHANNELS, cl, ctype_of, header_decls

HIST_FUNCS = ['cnnq_pc_route_qdq_hist_nhwc', 'cnnq_pc_qdq_hist_nhwc', 'cnnq_pc_minmax_qdq_hist_nhwc', 'cnnq_pc_aciq_qdq_hist_nhwc']
HREP, CL_HIST_ELEMS = 32, 65536


def lib():
    from cnn_quantization_amd import _lib as L
    return L.load()


def test_entry_points_exist_and_prototypes_match_header():
    from cnn_quantization_amd import _lib as L
    decls = header_decls()
    for name in HIST_FUNCS:
        assert hasattr(lib(), name), name
        ret, args = decls[name]
        res, argtypes = L.SIGNATURES[name]
        assert res is ctypes.c_int and ret == 'int', name
        assert len(args) == len(argtypes), name
        for a, t in zip(args, argtypes):
            want = ctype_of(a)
            if want == 'ptr':
                assert t is ctypes.c_void_p or issubclass(t, ctypes._Pointer), (name, a, t)
            else:
                assert t is want, (name, a, t)


def cfg(num_bits=4, clip=1, bit_alloc=0):
    from cnn_quantization_amd import _lib as L
    return L.ParamsCfg(num_bits, 0, clip, 0.0, bit_alloc, 0, 4.0, 1, 0)


def table_args(dtype=0, R=4, C=8, nbins=16):
    p = ctypes.c_void_p(BAD)
    return [p, ctypes.c_void_p(BAD + 0x1000), dtype, R, C, p, nbins, p, None]             # x, y, dtype, R, C, qp, nbins, hist_rep, stream


def minmax_args(dtype=0, R=4, C=8, bits=4):
    p = ctypes.c_void_p(BAD)
    # x, y, dtype, R, C, num_bits, positive, ws, qp, mm, hist_rep, stream
    return [p, ctypes.c_void_p(BAD + 0x1000), dtype, R, C, bits, 0, p, p, None, p, None]


def aciq_args(dtype=0, R=4, C=8, c=None):
    p = ctypes.c_void_p(BAD)
    # x, y, dtype, R, C, cfg, ws, stats, qp, diag, hist_rep, stream
    return [p, ctypes.c_void_p(BAD + 0x1000), dtype, R, C, ctypes.byref(c or cfg()), p, p, p, p, p, None]


@pytest.mark.parametrize('dtype, R, C', [(-1, 4, 8), (3, 4, 8), (1 << 20, 4, 8), (0, 0, 8), (1, 4, 0), (2, -3, 8), (0, 4, -1)])
def test_bad_geometry_is_einval(dtype, R, C):
    out = (ctypes.c_int32 * 4)()
    assert lib().cnnq_pc_route_qdq_hist_nhwc(R, C, dtype, 16, 16, out) == EINVAL
    assert lib().cnnq_pc_qdq_hist_nhwc(*table_args(dtype, R, C)) == EINVAL
    assert lib().cnnq_pc_minmax_qdq_hist_nhwc(*minmax_args(dtype, R, C)) == EINVAL
    assert lib().cnnq_pc_aciq_qdq_hist_nhwc(*aciq_args(dtype, R, C)) == EINVAL


@pytest.mark.parametrize('dtype', [0, 1, 2])
def test_bad_pointers_bins_and_bits_are_einval(dtype):
    p = ctypes.c_void_p(BAD)
    odd = ctypes.c_void_p(BAD + 4)
    # the table-driven pass: x, y, qp, hist_rep; hist_rep holds 64-bit words; x == y; nbins a power of two in [2, 256]
    for i in (0, 1, 5, 7):
        a = table_args(dtype)
        a[i] = None
        assert lib().cnnq_pc_qdq_hist_nhwc(*a) == EINVAL, i
    a = table_args(dtype)
    a[7] = odd
    assert lib().cnnq_pc_qdq_hist_nhwc(*a) == EINVAL
    a = table_args(dtype)
    a[1] = p
    assert lib().cnnq_pc_qdq_hist_nhwc(*a) == EINVAL
    for nbins in (-4, 0, 1, 3, 12, 255, 257, 512, 1 << 20):
        assert lib().cnnq_pc_qdq_hist_nhwc(*table_args(dtype, nbins=nbins)) == EINVAL, nbins
    # config 2, dynamic: x, y, ws, qp, hist_rep (mm may be NULL); ws holds floats; num_bits in [1, 8]
    for i in (0, 1, 7, 8, 10):
        a = minmax_args(dtype)
        a[i] = None
        assert lib().cnnq_pc_minmax_qdq_hist_nhwc(*a) == EINVAL, i
    a = minmax_args(dtype)
    a[7] = ctypes.c_void_p(BAD + 2)
    assert lib().cnnq_pc_minmax_qdq_hist_nhwc(*a) == EINVAL
    a = minmax_args(dtype)
    a[10] = odd
    assert lib().cnnq_pc_minmax_qdq_hist_nhwc(*a) == EINVAL
    a = minmax_args(dtype)
    a[1] = p
    assert lib().cnnq_pc_minmax_qdq_hist_nhwc(*a) == EINVAL
    for bits in (-1, 0, 9, 16, 32, 33):
        assert lib().cnnq_pc_minmax_qdq_hist_nhwc(*minmax_args(dtype, bits=bits)) == EINVAL, bits
    # config 3, dynamic: x, y, cfg, ws, stats, qp, hist_rep; ws holds doubles; the cfg checks of cnnq_pc_aciq_qdq_nhwc
    for i in (0, 1, 5, 6, 7, 8, 10):
        a = aciq_args(dtype)
        a[i] = None
        assert lib().cnnq_pc_aciq_qdq_hist_nhwc(*a) == EINVAL, i
    for i in (6, 10):
        a = aciq_args(dtype)
        a[i] = odd
        assert lib().cnnq_pc_aciq_qdq_hist_nhwc(*a) == EINVAL, i
    a = aciq_args(dtype)
    a[1] = p
    assert lib().cnnq_pc_aciq_qdq_hist_nhwc(*a) == EINVAL
    a = aciq_args(dtype, c=cfg(bit_alloc=1))
    a[9] = None                                              # the bit table lives in diag
    assert lib().cnnq_pc_aciq_qdq_hist_nhwc(*a) == EINVAL
    for c in (cfg(num_bits=0), cfg(num_bits=9), cfg(num_bits=16, clip=0), cfg(num_bits=33, clip=0), cfg(clip=4), cfg(clip=-1)):
        assert lib().cnnq_pc_aciq_qdq_hist_nhwc(*aciq_args(dtype, c=c)) == EINVAL, (c.num_bits, c.clip)
    # the route function
    out = (ctypes.c_int32 * 4)()
    assert lib().cnnq_pc_route_qdq_hist_nhwc(4, 8, dtype, 3, 16, out) == EINVAL
    assert lib().cnnq_pc_route_qdq_hist_nhwc(4, 8, dtype, 0, 16, out) == EINVAL
    assert lib().cnnq_pc_route_qdq_hist_nhwc(4, 8, dtype, 16, 16, None) == EINVAL
    for nbins in (0, 1, 3, 100, 512):
        assert lib().cnnq_pc_route_qdq_hist_nhwc(4, 8, dtype, 16, nbins, out) == EINVAL, nbins


@pytest.mark.parametrize('dtype', [0, 1, 2])
@pytest.mark.parametrize('align', [2, 4, 8, 16])
def test_route_report_is_consistent_with_config_2s(dtype, align):
    out, ref = (ctypes.c_int32 * 4)(), (ctypes.c_int32 * 4)()
    for C in CHANNELS:
        for R in (1, 2, 49, 1000, 25088, 512 * 56 * 56, 512 * 112 * 112):
            assert lib().cnnq_pc_route_nhwc(R, C, dtype, align, ref) == 0
            for nbins in (2, 4, 16, 256):
                assert lib().cnnq_pc_route_qdq_hist_nhwc(R, C, dtype, align, nbins, out) == 0, (R, C, nbins)
                w, wgs, lds, native = list(out)
                assert w == ref[0] and native == 1
                assert lds == nbins * HREP * 4
                # column blocks x row slabs of whole row steps, at least CL_HIST_ELEMS elements per workgroup: never more
                # workgroups than the plain Q/DQ launch
                P = C // w
                CP = min(P, 256)
                RS, nb = 256 // CP, -(-P // CP)
                steps = -(-CL_HIST_ELEMS // (CP * w * RS))
                slabs = -(-(-(-R // RS)) // steps)
                assert wgs % nb == 0 and 1 <= wgs // nb <= slabs, (R, C, wgs, nb, slabs)
                assert wgs <= ref[2]


def quantizer(**kw):
    return Q.quantizer(**dict(dict(pcq_act=True, measure_entropy=True), **kw))


def nhwc_bf16():
    x = cl((2, 8, 4, 4)).bfloat16()
    return x.as_strided(x.shape, (128, 1, 32, 8))


def test_dispatch_conditions_on_cpu_tensors():
    from cnn_quantization_amd import ops
    x = nhwc_bf16()
    assert ops._layout(x) == 'nhwc' and x.dtype == torch.bfloat16
    nchw = torch.zeros(2, 8, 4, 4, dtype=torch.bfloat16)
    q = quantizer()
    assert q._nhwc_entropy(x) and q._nhwc_entropy(x.float().as_strided(x.shape, x.stride()))
    assert quantizer(bits=8)._nhwc_entropy(x) and quantizer(bits=2)._nhwc_entropy(x)
    assert quantizer(bits=8, bit_alloc_act=True)._nhwc_entropy(x)                               # bit allocation is in effect up to 4 bits
    # _half_native keeps its answer: never with the entropy measurement
    assert not q._half_native(x) and not q._half_native(x, None, 'id')
    # every condition
    assert not quantizer(measure_entropy=False)._nhwc_entropy(x)
    assert not quantizer(pcq_act=False)._nhwc_entropy(x)
    assert not quantizer(clipping='laplace')._nhwc_entropy(x) and not quantizer(clipping='gaus')._nhwc_entropy(x)
    assert not quantizer(pcq_weights=True)._nhwc_entropy(x)
    assert not quantizer(mtd_quant=True)._nhwc_entropy(x)
    assert not quantizer(bit_alloc_act=True)._nhwc_entropy(x)
    assert not quantizer(bits=9)._nhwc_entropy(x) and not quantizer(bits=32)._nhwc_entropy(x)
    assert not quantizer(kld=True)._nhwc_entropy(x)
    assert not q._nhwc_entropy(nchw)
    assert not q._nhwc_entropy(x[:, 2:5])                                                       # not dense
    assert not q._nhwc_entropy(torch.zeros(2, 8, 1, 1, dtype=torch.bfloat16))                   # no spatial extent: per tensor
    assert not q._nhwc_entropy(torch.zeros(8, 16, dtype=torch.bfloat16))                        # not 4-D
    # __call__'s override pair is looked at (through _att, the lookup the predicates share)
    for att in (('measure_entropy', False), ('clipping', 'laplace'), ('pcq_w', True), ('mtd_quant', True), ('kld', True),
                ('pcq_a', False), ('bit_alloc_act', True), ('num_bits', 16)):
        assert not q._nhwc_entropy(x, q._att(att)), att
    qn = quantizer(measure_entropy=False)
    assert qn._nhwc_entropy(x, qn._att(('measure_entropy', True)))
    q.fuse_bcorr = True                                                                         # a pending bias correction: the layer corrects afterwards
    assert not q._nhwc_entropy(x)
    q.fuse_bcorr = None
    q.group = False                                                                             # replicated data: never this route
    assert not q._nhwc_entropy(x)
    q.group = None
    assert q._nhwc_entropy(x)


def test_the_four_earlier_predicates_answer_as_before():
    """What _half_native, _nhwc_aciq, _nhwc_bcorr and _nhwc_midtread compute on the parent, restated."""
    x = nhwc_bf16()
    nchw = torch.zeros(2, 8, 4, 4, dtype=torch.bfloat16)
    for kw in (dict(), dict(measure_entropy=False), dict(clipping='laplace'), dict(clipping='laplace', measure_entropy=False),
               dict(clipping='gaus', bit_alloc_act=True), dict(bit_alloc_act=True), dict(mtd_quant=True, clipping='laplace'),
               dict(mtd_quant=True), dict(kld=True), dict(pcq_act=False), dict(pcq_weights=True), dict(bits=8)):
        q = quantizer(**kw)
        for pending in (None, True):
            q.fuse_bcorr = pending
            for t in (x, x.float().as_strided(x.shape, x.stride()), nchw):
                nhwc = not t.is_contiguous()
                clipped = q.clipping in ('laplace', 'gaus')
                aciq = bool(q.pcq_a and clipped and nhwc and not q.measure_entropy and pending is None)
                assert bool(q._nhwc_aciq(t, q.clipping)) == aciq, (kw, pending)
                mid = bool(q.mtd_quant and q.clipping != 'no' and not q.kld and q.pcq_a and nhwc and pending is None)
                assert bool(q._nhwc_midtread(t)) == mid, (kw, pending)
                for stat_id in (None, 'id'):
                    bc = bool(stat_id is not None and pending is not None and q.pcq_a and not (q.clipping == 'no' and q.pcq_w)
                              and nhwc and not q.mtd_quant and not q.kld and not q.measure_entropy)
                    assert bool(q._nhwc_bcorr(t, q.clipping, stat_id)) == bc, (kw, pending, stat_id)
                    if q.kld:
                        want = False
                    elif bc:
                        want = True
                    elif q.clipping != 'no':
                        want = not q.mtd_quant and aciq
                    elif q.pcq_w:
                        want = False
                    elif q.pcq_a:
                        want = (not q.mtd_quant and not q.measure_entropy and pending is None
                                and not (q.bit_alloc_act and q.num_bits <= 4))
                    else:
                        want = True
                    assert bool(q._half_native(t, None, stat_id)) == want, (kw, pending, stat_id)


def test_forced_exchange_and_the_nhwc_switch_turn_the_route_off(monkeypatch):
    from cnn_quantization_amd import distributed as D, ops
    x = nhwc_bf16()
    q = quantizer()
    monkeypatch.setattr(D, 'forced_exchange', lambda: True)
    assert not q._nhwc_entropy(x)
    monkeypatch.undo()
    assert q._nhwc_entropy(x)
    old = os.environ.get('CNNQ_NHWC')
    try:
        os.environ['CNNQ_NHWC'] = '0'
        ops.reload_switches()
        assert not q._nhwc_entropy(x) and not q._half_native(x)
    finally:
        if old is None:
            os.environ.pop('CNNQ_NHWC', None)
        else:
            os.environ['CNNQ_NHWC'] = old
        ops.reload_switches()
    assert q._nhwc_entropy(x)


def test_ops_refuse_cpu_tensors():
    from cnn_quantization_amd import _lib as L, ops
    with pytest.raises(L.CnnqError):
        ops.act_qdq_per_channel(cl((2, 3, 4, 4)), 4, want_entropy=True)
    with pytest.raises(L.CnnqError):
        ops.aciq_qdq_nhwc(cl((2, 3, 4, 4)), 4, want_entropy=True)
