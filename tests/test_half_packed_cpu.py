"""CPU-only checks of the stored-code entry points for contiguous bf16 / fp16 activations: they exist, their
ctypes prototypes match the header's declarations, bad arguments are refused before anything touches the device, the route
function reports the family's piece widths, and the ops functions take nothing but what _admit_half takes."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCS = ['cnnq_pc_route_packed_dt', 'cnnq_pc_quantize_packed_dt', 'cnnq_pc_dequantize_packed_dt', 'cnnq_pc_minmax_quantize_packed_dt',
         'cnnq_pc_aciq_quantize_packed_dt']
P = ctypes.c_void_p(0x1000)    # a non-null, 4-byte aligned pointer value that is never dereferenced: the checks come first
ODD = ctypes.c_void_p(0x1002)  # 2-byte aligned only
EINVAL = -1


def lib():
    from cnn_quantization_amd import _lib as L
    return L, L.load()


def ctype_of(decl):
    if '*' in decl or '[' in decl:
        return ctypes.c_void_p
    return {'int': ctypes.c_int, 'int64_t': ctypes.c_int64}[decl.replace('const ', '').rsplit(' ', 1)[0].strip()]


def test_entry_points_exist_and_prototypes_match_header():
    L, l = lib()
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'cnnq_hip.h')).read(), flags=re.S)
    decls = {name: [a.strip() for a in args.split(',')] for name, args in re.findall(r'\bint\s+(cnnq_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', text)}
    for name in FUNCS:
        assert hasattr(l, name), name
        res, argtypes = L.SIGNATURES[name]
        assert res is ctypes.c_int
        want = [ctype_of(a) for a in decls[name]]
        got = [ctypes.c_void_p if isinstance(t, type) and issubclass(t, ctypes._Pointer) else t for t in argtypes]
        assert got == want, name


def calls(l, dtype=1, x=P, packed=P, num_bits=4, ws=P, fronts_only=False):
    """The device entry points with one argument made bad; fronts_only: the bad argument is one only the two one-call fronts take."""
    from cnn_quantization_amd import ops
    c = ops._params_cfg(4, False, 'laplace', True, False, None, True, False)
    c.num_bits = num_bits
    rcs = [l.cnnq_pc_minmax_quantize_packed_dt(x, dtype, 4, 8, 16, num_bits, 0, ws, P, P, packed, None),
           l.cnnq_pc_aciq_quantize_packed_dt(x, dtype, 4, 8, 16, ctypes.byref(c), ws, P, P, P, P, packed, None)]
    if not fronts_only:
        rcs += [l.cnnq_pc_quantize_packed_dt(x, dtype, 4, 8, 16, P, P, P, packed, None),
                l.cnnq_pc_dequantize_packed_dt(packed, x, dtype, 4, 8, 16, P, P, P, None)]
    return rcs


@pytest.mark.parametrize('bad', [dict(dtype=-1), dict(dtype=3), dict(x=None), dict(packed=None), dict(packed=ODD),
                                 dict(ws=None, fronts_only=True), dict(num_bits=0, fronts_only=True), dict(num_bits=9, fronts_only=True)],
                         ids=['dtype-1', 'dtype3', 'null-x', 'null-packed', 'misaligned-packed', 'null-ws', 'num_bits0', 'num_bits9'])
def test_bad_arguments_are_einval_with_nothing_enqueued(bad):
    _, l = lib()
    assert set(calls(l, **bad)) == {EINVAL}
    out = (ctypes.c_int32 * 4)()
    assert l.cnnq_pc_route_packed_dt(0, 8, 16, 1, 16, out) == EINVAL and l.cnnq_pc_route_packed_dt(4, 8, 16, 1, 16, None) == EINVAL


@pytest.mark.parametrize('HW,align,w', [(64, 16, 8), (196, 16, 4), (30, 16, 2), (49, 16, 1), (64, 2, 1)])
def test_route_reports_the_piece_width(HW, align, w):
    L, l = lib()
    out = (ctypes.c_int32 * 4)()
    for dtype in (L.DTYPE_BF16, L.DTYPE_F16):
        assert l.cnnq_pc_route_packed_dt(512, 64, HW, dtype, align, out) == 0
        ppr = HW // w
        assert out[0] == w and out[1] >= 64 and out[2] == (0 if ppr > 64 else 64 // ppr) and out[3] in (0, 1)
    assert l.cnnq_pc_route_packed_dt(512, 64, HW, L.DTYPE_F32, align, out) == 0 and tuple(out) == (0, 0, 0, 1)


@pytest.mark.parametrize('x,move', [(torch.zeros(2, 3, 4, 4), True), (torch.zeros(2, 3, 4, 4, dtype=torch.bfloat16), False),
                                    (torch.zeros(2, 3, 4, 4, dtype=torch.float16).to(memory_format=torch.channels_last), True),
                                    (torch.zeros(2, 3, 16, dtype=torch.bfloat16), True)], ids=['float32', 'cpu', 'channels_last', '3-D'])
def test_ops_refuse_what_admit_half_refuses(x, move):
    L, _ = lib()
    from cnn_quantization_amd import ops
    if move and torch.cuda.is_available():      # on a machine with a GPU the refusal is of the dtype / layout / rank itself
        x = x.cuda()
    qp = torch.zeros(L.NQP, 3, device=x.device)
    for fn in (lambda: ops.quantize_packed_half(x, qp, 4), lambda: ops.minmax_quantize_packed_half(x, 4),
               lambda: ops.aciq_quantize_packed_half(x, 4)):
        with pytest.raises(L.CnnqError):
            fn()
