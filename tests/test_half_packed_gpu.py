"""Stored codes on contiguous bf16 / fp16 activations against the format's words in plain fp32 torch on the
CPU: q = x.float() / scale + zp, clamped into [0, qmax] and rounded (int_quantizer.py:573-584), y = ((q - zp) * scale).to(dtype), row
(n, c) the little-endian bit stream of its codes at bits[c] bits each, padded to 4 bytes.  qp and bits are hand-built: the widths
0, 1, 3, 4, 5, 8 all occur, qmax = 2^b - 1, channel 0 is all negative and channel 1 constant."""
import numpy as np
import pytest
import torch

from test_half_aciq_gpu import check_tiers, ref64, same    # the statistics tier of the config-3 tests, not restated here

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]
IDS = ['bf16', 'f16']
# (shape, element offset of the view in a flat buffer): W = 8 with a full step and a 64-element tail per row; W = 8, several rows per
# step, C no multiple of 4; W = 4, the last group half full, H*W*b no multiple of 32; W = 2; W = 1 twice; a long ragged row; W = 1
# from the alignment alone
CASES = [((3, 5, 24, 24), 0), ((3, 5, 8, 8), 0), ((2, 6, 14, 14), 0), ((3, 4, 5, 6), 0), ((3, 7, 7, 7), 0), ((2, 3, 3, 3), 0),
         ((2, 2, 1, 1030), 0), ((3, 5, 8, 8), 1)]
CIDS = ['%s+%d' % ('x'.join(map(str, s)), o) for s, o in CASES]
WIDTHS = [4, 3, 0, 8, 5, 1]
FILL = 0xA5


def mods():
    from cnn_quantization_amd import _lib as L, ops
    return L, ops


def on_gpu(x, dtype, offset=0):
    flat = torch.zeros(x.numel() + offset, dtype=dtype, device='cuda')
    flat[offset:] = x.reshape(-1).to(dtype)
    return flat[offset:].view(x.shape)


def codes_of(x, qp, ba):
    """(codes, y in fp32) of the format's words for the half tensor x (CPU) and the table qp [NQP, C]."""
    sc, zp, qm = (qp[i].view(1, -1, 1, 1) for i in range(3))
    q = x.float() / sc + zp
    q = torch.where(q > qm, qm, q).clamp(min=0).round() if ba else torch.minimum(q.clamp(min=0), qm).round()
    return q, (q - zp) * sc


def stream_of(codes, bits):
    out = bytearray()
    for n in range(codes.shape[0]):
        for c in range(codes.shape[1]):
            v = codes[n, c].reshape(-1, 1).numpy().astype(np.uint8)
            row = np.packbits(np.unpackbits(v, axis=1, bitorder='little')[:, :int(bits[c])].reshape(-1), bitorder='little').tobytes()
            out += row + bytes(-len(row) % 4)
    return torch.frombuffer(out, dtype=torch.uint8) if out else torch.empty(0, dtype=torch.uint8)


_REF = {}


def case(shape, offset, dtype):
    """x on the GPU, its hand-built tables and the reference's codes, floats and bytes: computed once, never changed."""
    key = (shape, offset, dtype)
    if key not in _REF:
        g = torch.Generator().manual_seed(sum(shape) + offset)
        C = shape[1]
        x = torch.randn(shape, generator=g) * (0.3 + 2 * torch.rand(1, C, 1, 1, generator=g)) + torch.randn(1, C, 1, 1, generator=g)
        x[:, 0] = -x[:, 0].abs() - 0.5
        x[:, 1] = 1.25
        x = x.to(dtype)
        bits = torch.tensor([WIDTHS[(c + len(shape) * shape[2]) % 6] for c in range(C)], dtype=torch.float32)
        qm = 2 ** bits - 1
        t = x.float().transpose(0, 1).reshape(C, -1)
        mn, mx = t.min(1)[0], t.max(1)[0]
        sc = torch.where(qm > 0, (mx - mn) / qm.clamp(min=1), torch.ones(C)).clamp(min=1e-8)
        qp = torch.stack([sc, -mn / sc, qm])
        q, y32 = codes_of(x, qp, False)
        _REF[key] = dict(x=on_gpu(x, dtype, offset), qp=qp.cuda(), bits=bits.cuda(), y32=y32, y=y32.to(dtype), stream=stream_of(q, bits))
    return _REF[key]


def packed_into_filled(fn, shape):
    """fn(out=...) into a capacity-sized buffer prefilled with FILL -> the whole buffer on the CPU, rowoff."""
    _, ops = mods()
    buf = torch.full((ops.packed_capacity(shape),), FILL, dtype=torch.uint8, device='cuda')
    packed, rowoff = fn(buf)[:2]
    assert packed.data_ptr() == buf.data_ptr()
    return buf.cpu(), rowoff


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('shape,offset', CASES, ids=CIDS)
def test_bytes_decode_and_one_format(shape, offset, dtype):
    L, ops = mods()
    r = case(shape, offset, dtype)
    x, qp, bits = r['x'], r['qp'], r['bits']
    got, rowoff = packed_into_filled(lambda b: ops.quantize_packed_half(x, qp, bits, out=b), shape)
    used = shape[0] * int(rowoff[shape[1]])
    assert used == r['stream'].numel()
    assert torch.equal(got[:used], r['stream']) and bool((got[used:] == FILL).all())
    again, _ = packed_into_filled(lambda b: ops.quantize_packed_half(x, qp, bits, out=b, rowoff=rowoff), shape)
    assert torch.equal(again, got)
    # decode: the reference's y, 0-bit channels (0 - zp) * scale
    y = ops.dequantize_packed_half(got.cuda(), shape, dtype, qp, bits, rowoff)
    assert y.dtype == dtype and same(y.cpu(), r['y'])
    zero = (bits == 0).cpu()
    if zero.any():
        const = ((0 - qp[L.QP_ZP]) * qp[L.QP_SCALE]).to(dtype).cpu()
        assert same(y.cpu()[:, zero], const[zero].view(1, -1, 1, 1).expand(shape[0], -1, *shape[2:]))
    # one format: the fp32 encoder writes the same buffer, the fp32 decoder reads this one
    f32, _ = packed_into_filled(lambda b: ops.quantize_packed(x.float(), qp, bits, out=b, rowoff=rowoff), shape)
    assert torch.equal(f32, got)
    assert same(ops.dequantize_packed(got.cuda(), shape, qp, bits, rowoff).cpu(), r['y32'])
    assert same(ops.dequantize_packed_half(f32.cuda(), shape, dtype, qp, bits, rowoff).cpu(), r['y'])


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_uniform_width(dtype):
    """An integer width is the format with a constant table; the buffer is sized exactly."""
    L, ops = mods()
    shape = (3, 5, 8, 8)
    r = case(shape, 0, dtype)
    qp = r['qp'].clone()
    qp[L.QP_QMAX] = 15.
    packed, rowoff = ops.quantize_packed_half(r['x'], qp, 4)
    q, y32 = codes_of(r['x'].cpu(), qp.cpu(), False)
    assert torch.equal(packed.cpu(), stream_of(q, [4] * shape[1]))
    assert same(ops.dequantize_packed_half(packed, shape, dtype, qp, 4, rowoff).cpu(), y32.to(dtype))


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_mask_keeps_a_wide_code_inside_its_row(dtype):
    """A channel whose qp says qmax = 15 while bits[c] = 2: its neighbours' rows and its own padding are what a correct table gives."""
    L, ops = mods()
    shape = (2, 6, 14, 14)
    r = case(shape, 0, dtype)
    N, C, HW = shape[0], shape[1], shape[2] * shape[3]
    k = 3
    bits = r['bits'].clone()
    bits[k] = 2.
    good, wide = r['qp'].clone(), r['qp'].clone()
    good[L.QP_QMAX, k], wide[L.QP_QMAX, k] = 3., 15.
    for t in (good, wide):           # codes up to 15 before the clamp
        t[L.QP_SCALE, k] /= 15
        t[L.QP_ZP, k] *= 15
    a, rowoff = packed_into_filled(lambda b: ops.quantize_packed_half(r['x'], good, bits, out=b), shape)
    b, _ = packed_into_filled(lambda b: ops.quantize_packed_half(r['x'], wide, bits, out=b, rowoff=rowoff), shape)
    ro = rowoff.cpu().tolist()
    own = torch.zeros(a.numel(), dtype=torch.bool)
    for n in range(N):
        own[n * ro[C] + ro[k]:n * ro[C] + ro[k + 1]] = True
        row = int.from_bytes(bytes(b[n * ro[C] + ro[k]:n * ro[C] + ro[k + 1]].tolist()), 'little')
        assert row >> (2 * HW) == 0 and (ro[k + 1] - ro[k]) * 8 > 2 * HW
    assert torch.equal(a[~own], b[~own]) and not torch.equal(a[own], b[own])


@pytest.mark.parametrize('positive', [False, True], ids=['full', 'positive'])
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('shape', [(5, 6, 14, 14), (3, 8, 7, 7)], ids=['14x14', '7x7'])
def test_config2_front(shape, dtype, positive):
    _, ops = mods()
    from oracle import quant_oracle as O
    x = case(shape, 0, dtype)['x']
    packed, rowoff, qp = ops.minmax_quantize_packed_half(x, 4, positive)
    assert packed.numel() == shape[0] * int(rowoff[shape[1]])
    y = ops.dequantize_packed_half(packed, shape, dtype, qp, 4, rowoff)
    assert same(y.cpu(), O.act_per_channel_qdq(x.float().cpu(), 4, half_range=positive).to(dtype))


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_config3_front(dtype):
    L, ops = mods()
    shape = (8, 16, 14, 14)
    x = case(shape, 0, dtype)['x']
    bufs = [torch.full((ops.packed_capacity(shape),), FILL, dtype=torch.uint8, device='cuda') for _ in range(2)]
    packed, rowoff, parts = ops.aciq_quantize_packed_half(x, 4, bit_alloc=True, out=bufs[0])
    ops.aciq_quantize_packed_half(x, 4, bit_alloc=True, out=bufs[1])
    check_tiers(parts['stats'], ref64(x), (True, False, False))      # MIN / MAX exact, MEAN / STD / B within the tier of fp64
    bits = parts['diag'][L.DIAG_BITS]
    q, y32 = codes_of(x.cpu(), parts['qp'].cpu(), True)
    stream = stream_of(q, bits.cpu())
    assert stream.numel() == shape[0] * int(rowoff[shape[1]])
    assert torch.equal(bufs[0].cpu()[:stream.numel()], stream) and torch.equal(bufs[0], bufs[1])
    assert same(ops.dequantize_packed_half(packed, shape, dtype, parts['qp'], bits, rowoff).cpu(), y32.to(dtype))
