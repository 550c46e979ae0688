"""ops.max_pool_codes / ops.avg_pool_codes / ops.avg_pool_codes_q against plain fp64 torch on the CPU.

The maximum is exact on integers: F.max_pool2d of the unpacked codes as float64, torch.equal.  The average, per case:
(a) the fp32 output equals ((S / HW - zx) * sx).float() of fp64 tensors, bit for bit; (b) it lies within
2^-24 |ref| + (8 + HW) 2^-53 sx (255 + |zx|) of the fp64 mean of the decoded codes - derived: one fp32 rounding, the quotient, the
difference and the product at 2^-53 each, the reference's own HW additions, the rest room; (c) the _q bytes are todays_codes on the
fp32 entry's own output; (d) every _q code lies within 0.5 + tol / sy + 2^-14 of the fp64 clamp(ref / sy + zy, 0, top).
A thread of the average takes pixels g, g + G, ..: at 56 x 56 x 16 that is 13 (u8, G = 256) or 25 (pack4) pixels, so the widening of
the 16-bit lanes after 257 pixels of ONE thread is reached by the 257 x 257 x 8 case alone (516 / 258 pixels per thread)."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

from test_conv_codes_gpu import operands, stored
from test_requant_codes_gpu import table, todays_codes, unpacked

pytestmark = pytest.mark.gpu

# (N, H, W, C), kernel, stride, padding
MAX = [((1, 5, 5, 8), 3, 2, 1),                     # one tile, padding on every border, the dword path
       ((2, 9, 7, 24), 3, 2, 1),                    # an image boundary, C not whole 16-byte pieces
       ((2, 6, 6, 64), 2, 2, 0),                    # the VGG pool, the 16-byte path
       ((1, 4, 6, 16), (4, 6), None, 0),            # a window that is the whole image
       ((1, 9, 19, 136), (2, 5), (1, 2), (1, 2))]   # 10 x 10 outputs, 34 / 17 channel dwords: see test_max_pool_spans_tiles
AVG = [(1, 1, 1, 8), (3, 7, 7, 40), (2, 56, 56, 16), (2, 3, 5, 136), (1, 257, 257, 8)]


def codes(shape, fmt, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, 256 if fmt == 'u8' else 16, shape, generator=g, dtype=torch.uint8)


@pytest.mark.parametrize('fmt', ['u8', 'pack4'])
@pytest.mark.parametrize('shape,k,s,p', MAX, ids=str)
def test_max_pool_is_the_maximum_of_the_codes(shape, k, s, p, fmt):
    from cnn_quantization_amd import ops
    xq = codes(shape, fmt, sum(shape))
    ref = F.max_pool2d(xq.double().permute(0, 3, 1, 2), k, s, p).permute(0, 2, 3, 1)
    out = ops.max_pool_codes(stored(xq, fmt).cuda(), k, s, p, x_format=fmt)
    assert out.dtype == torch.uint8 and out.is_contiguous() and out.shape == ref.shape[:3] + (shape[3] // (1 if fmt == 'u8' else 2),)
    assert torch.equal(unpacked(out, fmt, shape[3]).double(), ref.reshape(-1, shape[3]))
    if shape == MAX[1][0] and fmt == 'u8':      # the output keeps the input's table: a non-integer zero point, bit for bit
        N, H, W, C = shape
        qp = torch.stack([torch.linspace(0.0371, 0.9, C), torch.linspace(-3.25, 255.5, C), torch.full((C,), 255.)]).cuda()
        dec = lambda c: ops.dequantize_packed_nhwc(c.flatten(), (c.shape[0], C) + tuple(c.shape[1:3]), torch.float32, qp, ops.packed_layout_nhwc(8, C))
        assert torch.equal(dec(out), F.max_pool2d(dec(xq.cuda()), k, s, p))


def test_max_pool_spans_tiles():
    """The last shape of MAX spans more than one workgroup tile in each tiled direction: the route gives tiles of 8 x 8 output
    pixels x 64 channel bytes; the output is 10 x 10 pixels x 136 (u8) / 68 (pack4) bytes."""
    from cnn_quantization_amd import _lib as L
    (N, H, W, C), k, s, p = MAX[4]
    out = (ctypes.c_int32 * 6)()
    for fmt, nbytes in ((L.CODES_U8, C), (L.CODES_PACK4, C // 2)):
        assert L.load().cnnq_max_pool_codes_route((ctypes.c_int64 * 10)(N, H, W, C, *k, *s, *p), fmt, 16, out) == 0
        assert list(out) == [8, 8, 64, 0, 10, 10] and nbytes > 64


@functools.lru_cache(maxsize=None)
def average(shape, fmt):
    """The CPU side of one case, computed once: codes, qpx, (a)'s expression, the fp64 mean of the decoded codes, (b)'s bound.
    The input's zero point is 0.13 below the table entry's smallest channel mean (non-integer), as a calibrated table's would be: the
    means then spread from 0.13 sx upwards and the output table built on their 97 % quantile spreads the codes over its range."""
    N, H, W, C = shape
    xq, top = codes(shape, fmt, sum(shape)), (255 if fmt == 'u8' else 15)
    S = xq.reshape(N, H * W, C).sum(1, dtype=torch.int64)
    Cx = N if shape == AVG[1] else 1
    zx = (S.double() / (H * W)).reshape(Cx, -1).min(1).values - 0.13
    qpx = torch.stack([torch.linspace(0.0371, 0.9, Cx), zx.float(), torch.full((Cx,), float(top))])
    sx, zx = qpx[0].double()[:, None], qpx[1].double()[:, None]
    pinned = ((S.double() / (H * W) - zx) * sx).float()
    ref = ((xq.double().reshape(N, H * W, C) - zx[:, None]) * sx[:, None]).mean(1)
    tol = 2.0 ** -24 * ref.abs() + (8 + H * W) * 2.0 ** -53 * sx * (255 + zx.abs())
    return xq, qpx, pinned, ref, tol


@pytest.mark.parametrize('fmt', ['u8', 'pack4'])
@pytest.mark.parametrize('shape', AVG, ids=str)
def test_avg_pool_matches_fp64_and_todays_route(shape, fmt):
    from cnn_quantization_amd import ops
    xq, qpx, pinned, ref, tol = average(shape, fmt)
    N, C = shape[0], shape[3]
    dev = stored(xq, fmt).cuda()
    y = ops.avg_pool_codes(dev, qpx.cuda(), x_format=fmt).cpu()
    assert torch.equal(y, pinned)                                                           # (a)
    err = (y.double() - ref).abs()
    print('max |y - ref| / tol = %.3g' % float((err / tol).max()))
    assert bool((err <= tol).all())                                                         # (b)
    for fy in ('u8', 'pack4'):
        top = 255 if fy == 'u8' else 15
        qpy, sy, zy = table(ref, 1, top, per_row=shape == AVG[1])
        out = ops.avg_pool_codes_q(dev, qpx.cuda(), qpy.cuda(), x_format=fmt, y_format=fy)
        assert out.dtype == torch.uint8 and out.shape == (N, C // (1 if fy == 'u8' else 2))
        got = unpacked(out, fy, C).double()
        assert torch.equal(got, todays_codes(y, sy, zy, top, False).double())               # (c)
        t = (ref / sy + zy).clamp(0, top)
        assert bool(((got - t).abs() <= 0.5 + tol / sy + 2.0 ** -14).all())                 # (d)
        assert got.max() == top and float(((got > 0) & (got < top)).double().mean()) >= 0.5


def test_codes_from_the_stem_to_the_logits():
    """conv_codes_q -> max_pool_codes -> avg_pool_codes_q -> linear_codes, every tensor passed on as it is: the logits of the same
    calls fed with CPU-built codes of each stage."""
    from cnn_quantization_amd import ops
    shape = (1, 12, 12, 4, 16, 7, 7, 2, 2, 3, 3)
    xq, wq, qpx, qpw, bias = (t.cuda() for t in operands(shape, 'u8', 'u8', seed=39))
    q1, q2 = torch.tensor([[7.3], [3.37], [255.]]), torch.tensor([[7.0], [1.63], [255.]])      # the stem's 97 % quantile is 1822
    _, wl, _, qpl, bl = (t.cuda() for t in operands((1, 1, 2, 16, 8, 1, 1), 'u8', 'u8', seed=40))
    fc = lambda c: ops.linear_codes(c.cuda(), wl.view(8, 16), q2.cuda(), qpl, bias=bl)
    a = ops.conv_codes_q(xq, wq, qpx, qpw, q1.cuda(), bias=bias, relu=True, stride=2, padding=3)
    b = ops.max_pool_codes(a, 3, 2, 1)
    c = ops.avg_pool_codes_q(b, q1.cuda(), q2.cuda())
    assert a.shape == (1, 6, 6, 16) and b.shape == (1, 3, 3, 16) and c.shape == (1, 16)
    y32 = ops.conv_codes(xq, wq, qpx, qpw, bias=bias, stride=2, padding=3).cpu().permute(0, 2, 3, 1).contiguous()
    a_cpu = todays_codes(y32, q1[0], q1[1], 255, True)
    b_cpu = F.max_pool2d(a_cpu.double().permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).to(torch.uint8)
    y32 = ((b_cpu.double().sum((1, 2)) / 9 - q1[1].double()) * q1[0].double()).float()
    c_cpu = todays_codes(y32, q2[0], q2[1], 255, False)
    assert c_cpu.min() < 64 and c_cpu.max() > 192        # the CPU-built pooled codes reach both ends of the range
    for got, built in ((a, a_cpu), (b, b_cpu), (c, c_cpu)):
        assert torch.equal(got.cpu(), built)
    assert torch.equal(fc(c), fc(c_cpu)) and torch.equal(fc(c), fc(ops.avg_pool_codes_q(ops.max_pool_codes(a_cpu.cuda(), 3, 2, 1), q1.cuda(), q2.cuda())))
