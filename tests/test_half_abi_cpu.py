"""CPU-only checks of the bf16 / fp16 entry points of include/cnnq_hip.h: they exist, their ctypes prototypes match the
header's declarations, a dtype outside cnnq_dtype is refused before anything touches the device; the host-side pieces
(the upcast fallback, the harness flag) behave without a GPU."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DT_FUNCS = ['cnnq_pc_minmax_qdq_auto_dt', 'cnnq_pc_qdq_dt', 'cnnq_pc_minmax_local_dt', 'cnnq_pt_qdq_dt']
BAD = 0x1000   # a non-null pointer value that is never dereferenced: the dtype check comes first


def header_decls():
    text = open(os.path.join(ROOT, 'include', 'cnnq_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    out = {}
    for ret, name, args in re.findall(r'\b(int|size_t)\s+(cnnq_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', text):
        out[name] = (ret, [a.strip() for a in args.split(',')])
    return out


def ctype_of(decl):
    decl = re.sub(r'\s*\b[A-Za-z_][A-Za-z_0-9]*$', '', decl.strip())    # drop the parameter name
    if '*' in decl:
        return ctypes.c_void_p
    return {'int': ctypes.c_int, 'int64_t': ctypes.c_int64, 'size_t': ctypes.c_size_t}[decl.replace('const ', '')]


def test_entry_points_exist_and_prototypes_match_header():
    from cnn_quantization_amd import _lib as L
    lib = L.load()
    decls = header_decls()
    for name in DT_FUNCS:
        assert hasattr(lib, name), name
        ret, args = decls[name]
        res, argtypes = L.SIGNATURES[name]
        assert res is ctypes.c_int and ret == 'int', name
        assert [ctype_of(a) for a in args] == argtypes, name
    assert 'int dtype' in decls['cnnq_pc_qdq_dt'][1]
    assert (L.DTYPE_F32, L.DTYPE_BF16, L.DTYPE_F16, L.NDTYPE) == (0, 1, 2, 3)


@pytest.mark.parametrize('dtype', [-1, 3, 7, 1 << 20])
def test_bad_dtype_is_einval(dtype):
    from cnn_quantization_amd import _lib as L
    lib = L.load()
    ws = ctypes.c_void_p(BAD)
    assert lib.cnnq_pc_minmax_qdq_auto_dt(ws, ws, dtype, 4, 8, 16, 4, 0, ws, None, 0, 1, None) == -1
    assert lib.cnnq_pc_qdq_dt(ws, ws, dtype, 4, 8, 16, ws, None, None, 0, None) == -1
    assert lib.cnnq_pc_minmax_local_dt(ws, dtype, 4, 8, 16, ws, ws, None) == -1
    assert lib.cnnq_pt_qdq_dt(ws, ws, dtype, 64, ws, None, None) == -1


@pytest.mark.parametrize('dtype', [0, 1, 2])
def test_bad_arguments_need_no_device(dtype):
    from cnn_quantization_amd import _lib as L
    lib = L.load()
    p = ctypes.c_void_p(BAD)
    assert lib.cnnq_pc_minmax_qdq_auto_dt(None, p, dtype, 4, 8, 16, 4, 0, p, None, 0, 1, None) == -1
    assert lib.cnnq_pc_minmax_qdq_auto_dt(p, p, dtype, 4, 8, 16, 0, 0, p, None, 0, 1, None) == -1     # num_bits 0
    assert lib.cnnq_pc_qdq_dt(p, p, dtype, 4, 8, 16, None, None, None, 0, None) == -1
    assert lib.cnnq_pc_minmax_local_dt(p, dtype, 4, 8, 16, None, p, None) == -1
    assert lib.cnnq_pt_qdq_dt(p, p, dtype, 0, p, None, None) == -1
    if dtype != L.DTYPE_F32:
        # codes / histogram from a half input: no kernel, nothing enqueued
        assert lib.cnnq_pc_qdq_dt(p, p, dtype, 4, 8, 16, p, p, None, 0, None) == L.ENOTSUP


def test_upcast_fallback_counts_and_casts_back():
    import sys
    import cnn_quantization_amd.qtypes  # noqa: F401
    iq = sys.modules['cnn_quantization_amd.qtypes.int_quantizer']
    seen = []

    def fn(a, b, k=1):
        seen.append((a.dtype, b))
        return a * k

    before = iq.HALF_FALLBACKS
    x = torch.tensor([1.0, 2.5, -3.0])
    assert torch.equal(iq.upcast_fallback(fn, x, 'tag', k=2), x * 2)
    assert iq.HALF_FALLBACKS == before                          # float32: called as is, not counted
    for dt in (torch.bfloat16, torch.float16):
        y = iq.upcast_fallback(fn, x.to(dt), 'tag', k=3)
        assert y.dtype == dt and torch.equal(y, (x * 3).to(dt))
        assert seen[-1] == (torch.float32, 'tag')               # fn computed on the upcast tensor
        z = iq.upcast_fallback(fn, x.to(dt), 'tag', cast_back=False)
        assert z.dtype == torch.float32
    assert iq.HALF_FALLBACKS == before + 4


def route(N, C, HW, align=16, single=1):
    from cnn_quantization_amd import _lib as L
    out = (ctypes.c_int32 * 4)()
    assert L.load().cnnq_pc_route_dt(N, C, HW, align, single, out) == 0
    return tuple(out)


def test_config2_routes():
    """The half routes of the ResNet-50 b512 geometries: the single launch for the 14x14 layers, the chain elsewhere."""
    assert route(512, 2048, 49)[:3] == (2, 1, 0)           # 7x7: 2-byte elements, the chain
    assert route(512, 1024, 196)[:3] == (1, 4, 32)         # 100352, 8-byte pieces
    assert route(512, 512, 784)[:3] == (2, 8, 0)           # 401408: two launches
    assert route(512, 64, 12544)[0] == 2
    assert route(512, 1024, 196, align=2)[:2] == (2, 1)    # 2-byte aligned pointer: 2-byte elements, the chain
    assert route(4, 16, 14, align=4)[:2] == (1, 2)         # 4-byte pieces
    assert route(512, 1024, 196, single=0)[0] == 2         # single launch not allowed: the chain
    assert route(512, 1024, 196)[3] == 1024                # one workgroup per channel
    from cnn_quantization_amd import _lib as L
    out = (ctypes.c_int32 * 4)()
    assert L.load().cnnq_pc_route_dt(4, 8, 16, 3, 1, out) == -1     # alignment not a power of two


def test_harness_dtype_flag():
    from cnn_quantization_amd.harness import inference_sim as H
    assert H.build_parser().parse_args([]).dtype == 'float32'
    assert H.build_parser().parse_args(['--dtype', 'bfloat16']).dtype == 'bfloat16'
    with pytest.raises(SystemExit):
        H.build_parser().parse_args(['--dtype', 'int8'])
