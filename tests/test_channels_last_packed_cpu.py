"""The channels_last packed format without a GPU: the numpy restatement tests/_packed_nhwc.py pinned on the
worked examples of include/cnnq_hip.h, and the host side - symbols and prototypes, the refusals that happen before the device is
touched, the capacity arithmetic, the route report, and the ops' refusals (no silent copy)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import _packed_nhwc as PK

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ['cnnq_pc_packed_nhwc_capacity', 'cnnq_pc_packed_layout_nhwc', 'cnnq_pc_route_packed_nhwc', 'cnnq_pc_quantize_packed_nhwc',
       'cnnq_pc_dequantize_packed_nhwc', 'cnnq_pc_minmax_quantize_packed_nhwc', 'cnnq_pc_aciq_quantize_packed_nhwc']
EINVAL, ENOTSUP = -1, -3
F32, BF16 = 0, 1
P = 64       # a dummy non-null, 8-byte aligned pointer: never dereferenced


def mods():
    from cnn_quantization_amd import _lib as L, ops
    return L, ops


# ---- the restatement
def test_worked_example_three_channels():
    assert PK.pack(np.array([[5, 0, 17]]), [3, 0, 5]) == bytes([0x8D, 0, 0, 0])
    assert PK.unpack(bytes([0x8D, 0, 0, 0]), [3, 0, 5], 1, 3).tolist() == [[5, 0, 17]]


def test_worked_example_straddles_a_dword():
    bits = [8, 8, 8, 7, 3]
    assert PK.coloff(bits).tolist() == [0, 8, 16, 24, 31, 34]
    assert PK.rowbytes(bits) == 8
    # the last channel's code 0b101: its lowest bit is bit 31 of dword 0, the other two bits 0 and 1 of dword 1
    buf = PK.pack(np.array([[0, 0, 0, 0, 5], [255, 1, 2, 127, 7]]), bits)
    assert buf[:8] == bytes([0, 0, 0, 0x80, 0x02, 0, 0, 0])
    assert buf[8:] == bytes([255, 1, 2, 0xFF, 0x03, 0, 0, 0])


def test_uniform_widths_are_the_same_format():
    codes = np.arange(16).reshape(2, 8) % 16
    assert PK.coloff([4] * 8).tolist() == [4 * c for c in range(9)]
    assert PK.pack(codes, [4] * 8) == bytes([0x10, 0x32, 0x54, 0x76, 0x98, 0xBA, 0xDC, 0xFE])
    assert PK.pack(codes, [8] * 8) == bytes(range(16))
    assert PK.pack(codes, [0] * 8) == b''


@pytest.mark.parametrize('C', [1, 3, 5, 31, 32, 33, 300])
def test_round_trip_random_width_tables(C):
    rng = np.random.default_rng(C)
    seen = set()
    for trial in range(12):
        bits = rng.integers(0, 9, size=C)
        if C >= 9:
            bits[rng.permutation(C)[:9]] = np.arange(9)          # every width in every table
        seen.update(bits.tolist())
        R = int(rng.integers(1, 7))
        codes = rng.integers(0, 256, size=(R, C)) & ((1 << bits) - 1)
        buf = PK.pack(codes, bits)
        assert len(buf) == R * PK.rowbytes(bits)
        assert (PK.unpack(buf, bits, R, C) == codes).all()
        # a code wider than its channel never touches a neighbour's bits
        assert PK.pack(codes | (0xFFF & ~((1 << bits) - 1)), bits) == buf
    assert seen == set(range(9)) or C < 9


# ---- the C ABI
def prototypes():
    text = open(os.path.join(ROOT, 'include', 'cnnq_hip.h')).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    out = {}
    for ret, name, args in re.findall(r'\b(size_t|int)\s+(cnnq_[a-z0-9_]+)\s*\(([^)]*)\)\s*;', text):
        out[name] = (ret, [a.strip() for a in args.split(',')])
    return out


def test_symbols_exist_and_prototypes_match_the_header():
    L, _ = mods()
    lib = L.load()
    protos = prototypes()

    def ctype_of(arg):
        if '*' in arg or '[' in arg:
            return 'ptr'
        return {'int64_t': ctypes.c_int64, 'int': ctypes.c_int, 'size_t': ctypes.c_size_t}[arg.split()[-2] if len(arg.split()) > 1 else arg]

    for name in NEW:
        assert hasattr(lib, name), name
        ret, args = protos[name]
        res, sig = L.SIGNATURES[name]
        assert res is (ctypes.c_size_t if ret == 'size_t' else ctypes.c_int), name
        assert len(sig) == len(args), (name, args)
        for a, s in zip(args, sig):
            want = ctype_of(a)
            if want == 'ptr':
                assert s is ctypes.c_void_p or issubclass(s, ctypes._Pointer), (name, a)
            else:
                assert s is want, (name, a, s)


def test_capacity():
    L, ops = mods()
    lib = L.load()
    for R, C in [(1, 1), (3, 5), (49, 2048), (392, 20), (7, 8192), (1 << 20, 300), (5, 8193)]:
        assert lib.cnnq_pc_packed_nhwc_capacity(R, C) == R * 4 * ((8 * C + 31) // 32)
        assert lib.cnnq_pc_packed_nhwc_capacity(R, C) == R * PK.rowbytes([8] * C)
    assert lib.cnnq_pc_packed_nhwc_capacity(0, 4) == 0 and lib.cnnq_pc_packed_nhwc_capacity(4, 0) == 0
    assert ops.packed_capacity_nhwc((2, 20, 7, 7)) == lib.cnnq_pc_packed_nhwc_capacity(98, 20) == 98 * 20
    assert ops.packed_capacity_nhwc((2, 5, 5, 9)) == 90 * 8


def test_bad_arguments_return_before_the_device_is_touched():
    L, _ = mods()
    lib = L.load()
    big = (1 << 26) + 1                                              # beyond CL_C_MAX
    # the layout
    assert lib.cnnq_pc_packed_layout_nhwc(P, 0, 4, None, None) == EINVAL
    assert lib.cnnq_pc_packed_layout_nhwc(P, 0, 0, P, None) == EINVAL
    assert lib.cnnq_pc_packed_layout_nhwc(P, 0, big, P, None) == EINVAL
    assert lib.cnnq_pc_packed_layout_nhwc(None, 9, 4, P, None) == EINVAL
    assert lib.cnnq_pc_packed_layout_nhwc(None, -1, 4, P, None) == EINVAL
    # quantize: x, dtype, R, C, qp, mm, coloff, packed
    q = lib.cnnq_pc_quantize_packed_nhwc
    assert q(None, F32, 4, 4, P, None, P, P, None) == EINVAL
    assert q(P, F32, 4, 4, None, None, P, P, None) == EINVAL
    assert q(P, F32, 4, 4, P, None, None, P, None) == EINVAL
    assert q(P, F32, 4, 4, P, None, P, None, None) == EINVAL
    assert q(P, F32, 0, 4, P, None, P, P, None) == EINVAL
    assert q(P, F32, 4, 0, P, None, P, P, None) == EINVAL
    assert q(P, F32, 4, big, P, None, P, P, None) == EINVAL
    assert q(P, 3, 4, 4, P, None, P, P, None) == EINVAL
    assert q(P, -1, 4, 4, P, None, P, P, None) == EINVAL
    assert q(P, F32, 4, 4, P, None, P, P + 2, None) == EINVAL        # packed not 4-byte aligned
    assert q(P, F32, 4, 8193, P, None, P, P, None) == ENOTSUP        # a row image beyond the kernel's: before any launch
    assert q(P, BF16, 4, 8200, P, P, P, P, None) == ENOTSUP
    # dequantize: packed, y, dtype, R, C, qp, coloff
    d = lib.cnnq_pc_dequantize_packed_nhwc
    assert d(None, P, F32, 4, 4, P, P, None) == EINVAL
    assert d(P, None, F32, 4, 4, P, P, None) == EINVAL
    assert d(P, P, F32, 4, 4, None, P, None) == EINVAL
    assert d(P, P, F32, 4, 4, P, None, None) == EINVAL
    assert d(P, P, F32, 0, 4, P, P, None) == EINVAL
    assert d(P, P, F32, 4, 0, P, P, None) == EINVAL
    assert d(P, P, F32, 4, big, P, P, None) == EINVAL
    assert d(P, P, 7, 4, 4, P, P, None) == EINVAL
    assert d(P + 1, P, F32, 4, 4, P, P, None) == EINVAL
    # config 2 in one call: x, dtype, R, C, num_bits, positive, ws, qp, mm, coloff, packed
    m = lib.cnnq_pc_minmax_quantize_packed_nhwc
    assert m(None, F32, 4, 4, 4, 0, P, P, None, P, P, None) == EINVAL
    assert m(P, F32, 4, 4, 4, 0, None, P, None, P, P, None) == EINVAL
    assert m(P, F32, 4, 4, 4, 0, P, None, None, P, P, None) == EINVAL
    assert m(P, F32, 4, 4, 4, 0, P, P, None, None, P, None) == EINVAL
    assert m(P, F32, 4, 4, 4, 0, P, P, None, P, None, None) == EINVAL
    assert m(P, F32, 4, 4, 4, 0, P, P, None, P, P + 2, None) == EINVAL
    assert m(P, F32, 4, 4, 4, 0, P + 2, P, None, P, P, None) == EINVAL     # ws holds floats
    assert m(P, F32, 0, 4, 4, 0, P, P, None, P, P, None) == EINVAL
    assert m(P, F32, 4, 0, 4, 0, P, P, None, P, P, None) == EINVAL
    assert m(P, F32, 4, big, 4, 0, P, P, None, P, P, None) == EINVAL
    assert m(P, 3, 4, 4, 4, 0, P, P, None, P, P, None) == EINVAL
    for nb in (0, 9, -1, 32):
        assert m(P, F32, 4, 4, nb, 0, P, P, None, P, P, None) == EINVAL
    assert m(P, F32, 4, 8193, 4, 0, P, P, None, P, P, None) == ENOTSUP
    # config 3 in one call: x, dtype, R, C, cfg, ws, stats, qp, diag, coloff, packed
    a = lib.cnnq_pc_aciq_quantize_packed_nhwc

    def cfg(**kw):
        f = dict(num_bits=4, positive=0, clip=1, pstd=0., bit_alloc=0, prior_is_b=0, target=4., round_mode=1, direct_range=0)
        f.update(kw)
        return ctypes.byref(L.ParamsCfg(**f))

    assert a(P, F32, 4, 8193, cfg(), P, P, P, P, P, P, None) == ENOTSUP
    assert a(None, F32, 4, 4, cfg(), P, P, P, P, P, P, None) == EINVAL
    assert a(P, F32, 4, 4, None, P, P, P, P, P, P, None) == EINVAL
    assert a(P, F32, 4, 4, cfg(), None, P, P, P, P, P, None) == EINVAL
    assert a(P, F32, 4, 4, cfg(), P + 4, P, P, P, P, P, None) == EINVAL     # ws holds doubles
    assert a(P, F32, 4, 4, cfg(), P, None, P, P, P, P, None) == EINVAL
    assert a(P, F32, 4, 4, cfg(), P, P, None, P, P, P, None) == EINVAL
    assert a(P, F32, 4, 4, cfg(bit_alloc=1), P, P, P, None, P, P, None) == EINVAL   # the widths live in diag
    assert a(P, F32, 4, 4, cfg(), P, P, P, P, None, P, None) == EINVAL
    assert a(P, F32, 4, 4, cfg(), P, P, P, P, P, None, None) == EINVAL
    assert a(P, F32, 4, 4, cfg(), P, P, P, P, P, P + 2, None) == EINVAL
    assert a(P, F32, 0, 4, cfg(), P, P, P, P, P, P, None) == EINVAL
    assert a(P, F32, 4, 0, cfg(), P, P, P, P, P, P, None) == EINVAL
    assert a(P, F32, 4, big, cfg(), P, P, P, P, P, P, None) == EINVAL
    assert a(P, 5, 4, 4, cfg(), P, P, P, P, P, P, None) == EINVAL
    assert a(P, F32, 4, 4, cfg(num_bits=0), P, P, P, P, P, P, None) == EINVAL
    assert a(P, F32, 4, 4, cfg(num_bits=9, clip=0), P, P, P, P, P, P, None) == EINVAL
    assert a(P, F32, 4, 4, cfg(direct_range=1), P, P, P, P, P, P, None) == EINVAL


def test_route_report_matches_the_qdq_route():
    L, _ = mods()
    lib = L.load()
    for dtype, esize in ((0, 4), (1, 2), (2, 2)):
        for R, C in [(784, 64), (98, 20), (135, 6), (90, 5), (3, 8), (32, 300), (18, 1028), (18, 2056), (25088, 2048), (7, 8192),
                     (1 << 22, 64)]:
            for align in (16, 8, 4, 2):
                if align < esize:
                    continue
                a = (ctypes.c_int32 * 4)()
                b = (ctypes.c_int32 * 4)()
                assert lib.cnnq_pc_route_packed_nhwc(R, C, dtype, align, a) == 0
                assert lib.cnnq_pc_route_nhwc(R, C, dtype, align, b) == 0
                W, wgs, rpw, native = list(a)
                assert W == b[0] and native == 1
                assert C % W == 0 and (W * esize) <= align
                # whole rows per workgroup, every row owned once
                assert rpw >= 1 and wgs == (R + rpw - 1) // rpw
    a = (ctypes.c_int32 * 4)()
    assert lib.cnnq_pc_route_packed_nhwc(4, 8196, 0, 16, a) == 0 and list(a) == [4, 0, 0, 0]
    assert lib.cnnq_pc_route_packed_nhwc(0, 4, 0, 16, a) == EINVAL
    assert lib.cnnq_pc_route_packed_nhwc(4, 4, 9, 16, a) == EINVAL
    assert lib.cnnq_pc_route_packed_nhwc(4, 4, 0, 12, a) == EINVAL
    assert lib.cnnq_pc_route_packed_nhwc(4, 4, 0, 16, None) == EINVAL


# ---- ops: no silent copy
def test_ops_refuse_what_is_not_a_dense_channels_last_device_tensor():
    L, ops = mods()
    nhwc = torch.zeros(2, 8, 3, 3).contiguous(memory_format=torch.channels_last)
    assert ops._layout(nhwc) == 'nhwc'
    qp = torch.zeros(L.NQP, 8)
    coloff = torch.zeros(9, dtype=torch.int32)
    bad = {
        'a CPU tensor': (nhwc, 'CUDA/HIP'),
        'NCHW': (torch.zeros(2, 8, 3, 3), 'channels_last'),
        'not dense': (torch.zeros(2, 16, 3, 3).contiguous(memory_format=torch.channels_last)[:, ::2], 'channels_last'),
        'not 4-D': (torch.zeros(8, 8), 'channels_last'),
        'float64': (nhwc.double(), 'float32, bfloat16 or float16'),
        'int8': (nhwc.to(torch.int8), 'float32, bfloat16 or float16'),
        'not a tensor': (np.zeros((2, 8, 3, 3), dtype=np.float32), 'tensor'),
    }
    before = ops.LAYOUT_COPIES
    for what, (x, msg) in bad.items():
        for call in (lambda: ops.quantize_packed_nhwc(x, qp, 4),
                     lambda: ops.quantize_packed_nhwc(x, qp, torch.full((8,), 4.)),
                     lambda: ops.minmax_quantize_packed_nhwc(x, 4),
                     lambda: ops.aciq_quantize_packed_nhwc(x, 4),
                     lambda: ops.aciq_quantize_packed_nhwc(x, 4, bit_alloc=True)):
            with pytest.raises(L.CnnqError, match=msg):
                call()
    with pytest.raises(L.CnnqError):
        ops.dequantize_packed_nhwc(torch.zeros(64, dtype=torch.uint8), (2, 8, 3, 3), torch.float32, qp, coloff)
    with pytest.raises(L.CnnqError):
        ops.packed_layout_nhwc(torch.full((8,), 4.), 8)              # a CPU width table
    with pytest.raises(L.CnnqError):
        ops.packed_layout_nhwc(9, 8)
    assert ops.LAYOUT_COPIES == before
    # the fp32 NCHW functions and their refusals are as they were
    with pytest.raises(L.CnnqError):
        ops.quantize_u8(nhwc, qp)
