"""ops.conv_codes_q / ops.linear_codes_q: the integer layers that write codes.

Operands, input tables, the fp64 reference `ref` and its derived bound `tol` are those of test_conv_codes_gpu / test_linear_codes_gpu
(the largest shape of each kind with the per-image / per-sample input table those tests give their largest shape).  The output table:
zero points 0.37 + top / 100 .. 0.37 + top / 50 (non-integer; without ReLU the negative outputs clamp at 0), scale = the reference's
97 % quantile / (top - zp), so that 3 % of the outputs clamp at the top code; per tensor, on the largest shapes per image / sample.

1. Against fp64: t = clamp(relu(ref) / sy + zy, 0, qmax); every code has |code - t| <= 0.5 + tol / sy + 2^-14 - derived: the
   rounding to an integer, the fp32 value's own bound carried through the division, and two fp32 roundings (quotient, sum) of values
   below 1024, 2^-15 each; larger quotients clamp identically on both sides as |zy| <= 300.
2. Bit for bit the codes of today's route: conv_codes / linear_codes' own fp32 output, ReLU, and round(clamp(y / sy + zy, 0, qmax))
   in separately rounded fp32 operations on the CPU.
3. On the largest shapes, splits of 1, 2, 3 and a held rw / taps give the same bytes.
The range: the top code occurs and at least half the codes lie strictly between 0 and it; without ReLU code 0 occurs.  With ReLU
every non-positive output is the ONE code of 0.0, half of all codes: were that code 0 (zy < 0.5), half the codes could not lie inside
the range; it lies inside, so no code is below it, and the lowest code that occurs is asserted to be it."""
import functools

import pytest
import torch

import test_conv_codes_gpu as CC
import test_linear_codes_gpu as LC

pytestmark = pytest.mark.gpu

CONV = ((1, 4, 4, 16, 16, 3, 3, 1, 1, 1, 1), (2, 7, 5, 32, 40, 3, 3, 2, 2, 1, 1), (2, 9, 9, 64, 136, 3, 3, 1, 1, 1, 1))
LIN = ((1, 16, 64), (17, 40, 136), (130, 264, 320))
CASES = [(shapes, i, fx, fw) for shapes in (CONV, LIN) for i in range(3) for fx, fw in (CC.FORMATS if i == 0 else CC.FORMATS[:1])]


@functools.lru_cache(maxsize=None)
def layer(shapes, i, fx, fw):
    """The CPU side of one case, computed once: (device operands, call keywords, ref [M, N], tol [M, N], rows per table entry)."""
    shape, conv, big = shapes[i], shapes is CONV, i == 2
    xq, wq, qpx, qpw, bias = CC.operands(shape, fx, fw, seed=sum(shape)) if conv else LC.operands(*shape, fx, fw, seed=shape[0] * 1000 + shape[1])
    if big:         # per image / per sample, as the fp32 tests' largest shapes
        qx, C = float(qpx[2, 0]), shape[0]
        qpx = torch.stack([torch.linspace(0.0371, 0.9, C), torch.linspace(-3.25, qx + 0.5, C), torch.full((C,), qx)])
    if conv:
        ref, tol = CC.reference(shape, xq, wq, qpx, qpw, bias)
        rows = ref.shape[2] * ref.shape[3]
        ref, tol = (t.permute(0, 2, 3, 1).reshape(-1, shape[4]) for t in (ref, tol))
        kw = dict(stride=shape[7:9], padding=shape[9:11])
    else:
        (ref, tol), rows, kw = LC.reference(xq, wq, qpx, qpw, bias), 1, {}
    dev = [t.cuda() for t in (CC.stored(xq, fx), CC.stored(wq, fw), qpx, qpw)]
    return dev, dict(kw, bias=bias.cuda(), x_format=fx, w_format=fw), ref, tol, rows


def table(ref, rows, top, per_row):
    """qpy [3, Cy] from the reference, and its scale and zero point per row of ref as fp64 columns."""
    Cy = ref.shape[0] // rows if per_row else 1
    zy = torch.linspace(0.37 + top / 100, 0.37 + top / 50, Cy, dtype=torch.float64)
    qpy = torch.stack([float(ref.flatten().quantile(0.97)) / (top - zy), zy, torch.full_like(zy, top)]).float()
    sy, zy = (qpy[k].double().repeat_interleave(ref.shape[0] // Cy)[:, None] for k in (0, 1))
    return qpy, sy, zy


def unpacked(codes, fy, N):
    c = codes.cpu().reshape(-1, N // (2 if fy == 'pack4' else 1))
    return c if fy == 'u8' else torch.stack([c & 15, c >> 4], -1).flatten(1)


def todays_codes(y32, sy, zy, top, relu):
    q = (y32.relu() if relu else y32) / sy.float() + zy.float()
    q = torch.where(q > top, torch.tensor(float(top)), q)
    return torch.where(q < 0, torch.tensor(0.), q).round().to(torch.uint8)


@pytest.mark.parametrize('relu', [False, True], ids=['linear', 'relu'])
@pytest.mark.parametrize('fy', ['u8', 'pack4'])
@pytest.mark.parametrize('shapes,i,fx,fw', CASES, ids=lambda v: 'conv' if v is CONV else 'lin' if v is LIN else str(v))
def test_codes_match_fp64_and_todays_route(shapes, i, fx, fw, fy, relu):
    from cnn_quantization_amd import ops
    dev, kw, ref, tol, rows = layer(shapes, i, fx, fw)
    f32, fq = (ops.conv_codes, ops.conv_codes_q) if shapes is CONV else (ops.linear_codes, ops.linear_codes_q)
    top, N = (255 if fy == 'u8' else 15), ref.shape[1]
    qpy, sy, zy = table(ref, rows, top, per_row=i == 2)
    run = lambda **more: fq(*dev, qpy.cuda(), relu=relu, y_format=fy, **kw, **more)
    out = run()
    assert out.dtype == torch.uint8 and out.is_contiguous() and out.shape[-1] == (N if fy == 'u8' else N // 2) and out.numel() // out.shape[-1] == ref.shape[0]
    codes = unpacked(out, fy, N).double()
    # 1. the fp64 reference
    t = ((ref.relu() if relu else ref) / sy + zy).clamp(0, top)
    err, allowed = (codes - t).abs(), 0.5 + tol / sy + 2.0 ** -14
    print('max |code - t| = %.6f, max |code - t| / allowed = %.4f' % (float(err.max()), float((err / allowed).max())))
    assert bool((err <= allowed).all()), 'element %d: code %g, t %.6f' % (int((err - allowed).argmax()), codes.flatten()[(err - allowed).argmax()], t.flatten()[(err - allowed).argmax()])
    lowest = round(float(zy.min())) if relu else 0
    share = float(((codes > 0) & (codes < top)).double().mean())
    print('codes: lowest %d, top %.3f, inside %.3f' % (int(codes.min()), float((codes == top).double().mean()), share))
    assert codes.min() == lowest and codes.max() == top and share >= 0.5
    # 2. today's route, bit for bit
    y32 = f32(*dev, **kw).cpu()
    y32 = y32.permute(0, 2, 3, 1).reshape(-1, N) if shapes is CONV else y32
    assert torch.equal(codes, todays_codes(y32, sy, zy, top, relu).double())
    # 3. integers underneath
    if i == 2:
        held = dict(taps=ops.conv_codes_tapsums(dev[1], fw)) if shapes is CONV else dict(rw=ops.linear_codes_rowsums(dev[1], fw))
        for more in (dict(splits=1), dict(splits=2), dict(splits=3), held, dict(held, splits=2)):
            assert torch.equal(run(**more), out), '%s changes the bytes' % more.keys()


@pytest.mark.parametrize('fy', ['u8', 'pack4'])
def test_codes_are_the_next_layers_operand(fy):
    """The returned tensor, as it is, is the xq of the next conv_codes with qpx = qpy: the fp32 result of passing CPU-built codes;
    and (u8) the uniform 8-bit stream that dequantize_packed_nhwc decodes to (code - zy) * sy."""
    from cnn_quantization_amd import ops
    dev, kw, ref, tol, rows = layer(CONV, 1, 'u8', 'u8')
    top, (N, OH, OW, C) = (255 if fy == 'u8' else 15), (2, 4, 3, 40)
    qpy, sy, zy = table(ref, rows, top, per_row=False)
    out = ops.conv_codes_q(*dev, qpy.cuda(), relu=True, y_format=fy, **kw)
    y32 = ops.conv_codes(*dev, **kw).cpu().permute(0, 2, 3, 1).reshape(-1, C)
    built = todays_codes(y32, sy, zy, top, True).reshape(N, OH, OW, C)
    _, wq2, _, qpw2, bias2 = CC.operands((N, OH, OW, C, 16, 1, 1, 1, 1, 0, 0), fy, 'u8', seed=3)
    nxt = lambda xq: ops.conv_codes(xq, wq2.cuda(), qpy.cuda(), qpw2.cuda(), bias=bias2.cuda(), x_format=fy)
    assert torch.equal(nxt(out), nxt(CC.stored(built, fy).cuda()))
    if fy == 'u8':
        qp = qpy.expand(3, C).contiguous().cuda()
        dec = ops.dequantize_packed_nhwc(out.flatten(), (N, C, OH, OW), torch.float32, qp, ops.packed_layout_nhwc(8, C))
        assert torch.equal(dec.cpu().permute(0, 2, 3, 1), (built.float() - qpy[1]) * qpy[0])
