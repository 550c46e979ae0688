"""ops.dwconv_codes / ops.dwconv_codes_q against plain fp64 torch on the CPU: both operands dequantized,
(code - zp) * scale, and torch.nn.functional.conv2d(groups=C) with the same stride and zero padding.

1. fp32: the device value is one fp64 combination of four exact integers per channel and output pixel, rounded once, so the bound
   is test_conv_codes_gpu's with K = KH KW: |y - ref| <= ulp32(ref) + (16 + K) 2^-53 mag + 4 * 2^-53 |bias|, the integer fields
   from grouped fp64 conv2d on the raw codes and all-ones tensors.
2. _q: the bytes of today's route on dwconv_codes' own output (test_requant_codes_gpu.todays_codes), and every code within 0.5 +
   tol / sy + 2^-14 of the fp64 clamp(relu(ref) / sy + zy, 0, top).  The range: the top code and the lowest (0, or with ReLU the
   code of 0.0) occur and a quarter of the codes lie strictly inside - without ReLU about half of these zero-centred outputs clamp
   at 0 (not asserted on the all-255 shape, whose outputs take a handful of values).
3. The MobileNetV2 block: conv_codes_q (1 x 1) -> dwconv_codes_q -> conv_codes_q with residual=, each stage against CPU-built codes.
136 channel bytes are not whole 16-byte pieces, so S3 spans tiles and slabs on the dword path; the 16-byte path is taken by S4, S5
(u8, 16 bytes a pixel) and S7 (pack4, 16 bytes a pixel)."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import test_conv_codes_gpu as CC
import test_requant_codes_gpu as RQ

pytestmark = pytest.mark.gpu

# (N, H, W, C, KH, KW, sh, sw, ph, pw)
S1 = (1, 4, 4, 8, 3, 3, 1, 1, 1, 1)           # one tile, padding on every border, the dword path
S2 = (2, 7, 5, 24, 3, 3, 2, 2, 1, 1)          # stride 2, an image boundary, channels that are not whole 16-byte pieces
S3 = (2, 9, 19, 136, 3, 3, 1, 1, 1, 1)        # more than one tile each way, several slabs, a per-image qpx
S4 = (1, 5, 9, 16, 1, 7, 2, 1, 0, 3)          # an asymmetric kernel, stride and padding
S5 = (1, 2, 2, 16, 5, 5, 1, 1, 2, 2)          # a kernel larger than the image: Kv differs per pixel
S6 = (1, 3, 3, 8, 8, 8, 1, 1, 4, 4)           # all-255 codes on both sides at 64 taps: the largest sums
S7 = (1, 6, 6, 32, 3, 3, 1, 1, 1, 1)          # pack4 with 16 channel bytes a pixel: its 16-byte path
CASES = ([(fx, fw, s) for s in (S1, S2) for fx, fw in CC.FORMATS] + [('u8', 'u8', s) for s in (S3, S4, S5, S6)]
         + [('pack4', 'pack4', S7), ('pack4', 'u8', S7)])
IDS = lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else v


@functools.lru_cache(maxsize=None)
def layer(fx, fw, shape):
    """The CPU side of one case, computed once: device operands (xq, wq, qpx, qpw), bias, keywords, {bias?: (ref, tol)}."""
    N, H, W, C, KH, KW = shape[:6]
    g = torch.Generator().manual_seed(sum(shape))
    qx, qw = (255 if fx == 'u8' else 15), (255 if fw == 'u8' else 15)
    xq = torch.randint(0, qx + 1, (N, H, W, C), generator=g, dtype=torch.uint8)
    wq = torch.randint(0, qw + 1, (KH, KW, C), generator=g, dtype=torch.uint8)
    wq[..., 0], wq[..., 1], xq[0, 0, 0], xq[0, 0, 1] = 0, qw, 0, qx
    if shape == S6:
        xq[:], wq[:] = 255, 255
    Cx = N if shape == S3 else 1
    qpx = torch.stack([torch.linspace(0.0371, 0.9, Cx), torch.linspace(-3.25, qx + 0.5, Cx) if Cx > 1 else torch.full((1,), 127.5),
                       torch.full((Cx,), float(qx))])
    qpw = torch.stack([torch.logspace(-3, np.log10(3.0), C), torch.rand(C, generator=g) * (qw + 20) - 10.3, torch.full((C,), float(qw))])
    bias = torch.randn(C, generator=g) * 3
    geo = dict(stride=shape[6:8], padding=shape[8:10])
    X, Wt = xq.double().permute(0, 3, 1, 2), wq.double().permute(2, 0, 1).unsqueeze(1)
    sx, zx = (qpx[k].double().view(-1, 1, 1, 1) for k in (0, 1))
    sw, zw = (qpw[k].double().view(1, -1, 1, 1) for k in (0, 1))
    conv = lambda a, b: F.conv2d(a, b, groups=C, **geo)
    S, Rx, RwV, Kv = conv(X, Wt), conv(X, torch.ones_like(Wt)), conv(torch.ones_like(X), Wt), conv(torch.ones_like(X), torch.ones_like(Wt))
    mag = sx * sw * (S.abs() + (zw * Rx).abs() + (zx * RwV).abs() + Kv * (zx * zw).abs())
    refs = {}
    for b in (bias, None):
        bb = b.double().view(1, -1, 1, 1) if b is not None else torch.zeros(1, C, 1, 1, dtype=torch.float64)
        ref = conv((X - zx) * sx, (Wt - zw.view(-1, 1, 1, 1)) * sw.view(-1, 1, 1, 1)) + bb
        ulp = torch.from_numpy(np.spacing(ref.abs().numpy().astype(np.float32)).astype(np.float64))
        refs[b is not None] = (ref, ulp + (16 + KH * KW) * 2.0 ** -53 * mag + 4 * 2.0 ** -53 * bb.abs())
    dev = [t.cuda() for t in (CC.stored(xq, fx), CC.stored(wq, fw), qpx, qpw)]
    return dev, bias.cuda(), dict(geo, x_format=fx, w_format=fw), refs


@pytest.mark.parametrize('fx,fw,shape', CASES, ids=IDS)
def test_dwconv_codes_matches_fp64_reference(fx, fw, shape):
    from cnn_quantization_amd import _lib as L, ops
    dev, bias, kw, refs = layer(fx, fw, shape)
    for b in (True, False):
        y = ops.dwconv_codes(*dev, bias=bias if b else None, **kw)
        assert y.dtype == torch.float32 and y.shape[:2] == (shape[0], shape[3]) and y.is_contiguous(memory_format=torch.channels_last)
        CC.check(y.cpu(), *refs[b], 'bias' if b else 'no bias')
    if shape == S3:       # it does span tiles both ways and several slabs
        route = (ctypes.c_int32 * 6)()
        assert L.load().cnnq_dwconv_codes_route((ctypes.c_int64 * 10)(*shape), 0, 0, 16, route) == 0
        assert route[0] < route[4] and route[1] < route[5] and route[2] < shape[3], list(route)


@pytest.mark.parametrize('relu', [False, True], ids=['linear', 'relu'])
@pytest.mark.parametrize('fy', ['u8', 'pack4'])
@pytest.mark.parametrize('fx,fw,shape', CASES, ids=IDS)
def test_codes_match_fp64_and_todays_route(fx, fw, shape, fy, relu):
    from cnn_quantization_amd import ops
    dev, bias, kw, refs = layer(fx, fw, shape)
    top, C = (255 if fy == 'u8' else 15), shape[3]
    ref, tol = (t.permute(0, 2, 3, 1).reshape(-1, C) for t in refs[True])
    qpy, sy, zy = RQ.table(ref, ref.shape[0] // shape[0], top, per_row=shape == S3)
    out = ops.dwconv_codes_q(*dev, qpy.cuda(), bias=bias, relu=relu, y_format=fy, **kw)
    assert out.dtype == torch.uint8 and out.is_contiguous() and out.shape[-1] == (C if fy == 'u8' else C // 2) and out.shape[0] == shape[0]
    codes = RQ.unpacked(out, fy, C).double()
    t = ((ref.relu() if relu else ref) / sy + zy).clamp(0, top)
    err, allowed = (codes - t).abs(), 0.5 + tol / sy + 2.0 ** -14
    print('max |code - t| = %.6f, max |code - t| / allowed = %.4f' % (float(err.max()), float((err / allowed).max())))
    assert bool((err <= allowed).all()), 'element %d: code %g, t %.6f' % (int((err - allowed).argmax()), codes.flatten()[(err - allowed).argmax()], t.flatten()[(err - allowed).argmax()])
    if shape != S6:
        share = float(((codes > 0) & (codes < top)).double().mean())
        assert codes.min() == (round(float(zy.min())) if relu else 0) and codes.max() == top and share >= 0.25, (codes.min(), codes.max(), share)
    y32 = ops.dwconv_codes(*dev, bias=bias, **kw).cpu().permute(0, 2, 3, 1).reshape(-1, C)
    assert torch.equal(codes, RQ.todays_codes(y32, sy, zy, top, relu).double())


def test_mobilenetv2_block_stays_on_codes():
    """Expansion (1 x 1, ReLU) -> depthwise 3 x 3 (ReLU) -> projection (1 x 1, linear, + the block's input): each stage's bytes are
    today's route on the fp32 layer's output for the CPU-built codes of the stage before."""
    from cnn_quantization_amd import ops
    N, H, W, Cin, Cmid = 2, 6, 6, 16, 32
    xq, w1, qpx, qpw1, b1 = CC.operands((N, H, W, Cin, Cmid, 1, 1, 1, 1, 0, 0), 'u8', 'u8', seed=11)
    _, w3, _, qpw3, b3 = CC.operands((N, H, W, Cmid, Cin, 1, 1, 1, 1, 0, 0), 'u8', 'u8', seed=12)
    (_, wd, _, qpwd), bd, kwd, _ = layer('u8', 'u8', (N, H, W, Cmid, 3, 3, 1, 1, 1, 1))
    x, w1, qpx, qpw1, b1, w3, qpw3, b3 = (t.cuda() for t in (xq, w1, qpx, qpw1, b1, w3, qpw3, b3))
    nhwc = lambda y: y.cpu().permute(0, 2, 3, 1).reshape(N * H * W, -1)

    def stage(y32, relu):       # (qpy on the device, the CPU-built codes as an NHWC device tensor)
        qpy, sy, zy = RQ.table(y32.double(), N * H * W, 255, per_row=False)
        return qpy.cuda(), RQ.todays_codes(y32, sy, zy, 255, relu).reshape(N, H, W, -1).cuda()

    q1, c1 = stage(nhwc(ops.conv_codes(x, w1, qpx, qpw1, bias=b1)), True)
    g1 = ops.conv_codes_q(x, w1, qpx, qpw1, q1, bias=b1, relu=True)
    assert torch.equal(g1, c1)
    q2, c2 = stage(nhwc(ops.dwconv_codes(c1, wd, q1, qpwd, bias=bd, **kwd)), True)
    g2 = ops.dwconv_codes_q(g1, wd, q1, qpwd, q2, bias=bd, relu=True, **kwd)
    assert torch.equal(g2, c2)
    res = (xq.reshape(N * H * W, Cin).float() - qpx[1, 0].cpu()) * qpx[0, 0].cpu()       # rq_add_res: three fp32 roundings
    q3, c3 = stage(nhwc(ops.conv_codes(c2, w3, q2, qpw3, bias=b3)) + res, False)
    assert torch.equal(ops.conv_codes_q(g2, w3, q2, qpw3, q3, bias=b3, residual=x, qpr=qpx), c3)
