"""ops.conv_codes_q(..., residual=, qpr=, r_format=).  Operands, `ref` and `tol` are test_conv_codes_gpu's; the
output table (on the fp64 sum ref + rref), the unpacking and today's quantizer test_requant_codes_gpu's.  The residual: codes uniform
over 0 .. top_r, zr from 0.37 + top_r / 3 to 0.37 + top_r / 2, sr = 2 std(ref) / top_r (x 1 .. 1.5 across images); rref in fp64.
1. Against fp64: |code - clamp(relu(ref + rref) / sy + zy, 0, top)| <= 0.5 + tol' / sy + 2^-14, tol' = tol + 2^-22 (|ref| + |rref|):
   tol is the fp32 value's bound; the decode's two roundings and the sum's one, 2^-24 each of values <= |ref| + |rref|.
2. Bit for bit today's route: conv_codes' fp32 output + the CPU decode (code.float() - zr) * sr, one fp32 add, ReLU, todays_codes.
3. Largest shape: splits 1, 2, 3, held taps, out= the residual itself: the same bytes; smallest: two splits in every format pair.
4. The range: the top code occurs, >= 0.4 of the codes strictly inside (0, top), >= 0.25 differ from the call without the residual."""
import functools

import pytest
import torch

import test_conv_codes_gpu as CC
import test_requant_codes_gpu as RQ

pytestmark = pytest.mark.gpu

SHAPES = RQ.CONV + ((1, 6, 6, 16, 64, 1, 1, 1, 1, 0, 0),)     # ... and whole 16-byte residual pieces, several per row, rows beyond M = 36
PAIRS = [('u8', 'u8'), ('pack4', 'pack4'), ('u8', 'pack4'), ('pack4', 'u8')]
CASES = [(i, fr, fy) for i in range(4) for fr, fy in (PAIRS if i == 0 else PAIRS[:2])]


@functools.lru_cache(maxsize=None)
def layer(i):
    """The CPU side of one shape, computed once: (operands, call keywords, ref [M, Cout], tol [M, Cout], (N, OH, OW))."""
    shape, big = SHAPES[i], i == 2
    xq, wq, qpx, qpw, bias = CC.operands(shape, 'u8', 'u8', seed=sum(shape))
    if big:         # per image, as the fp32 tests' largest shape
        qpx = torch.stack([torch.linspace(0.0371, 0.9, shape[0]), torch.linspace(-3.25, 255.5, shape[0]), torch.full((shape[0],), 255.)])
    ref, tol = CC.reference(shape, xq, wq, qpx, qpw, bias)
    nhw = (ref.shape[0], ref.shape[2], ref.shape[3])
    ref, tol = (t.permute(0, 2, 3, 1).reshape(-1, shape[4]) for t in (ref, tol))
    return (xq, wq, qpx, qpw), dict(stride=shape[7:9], padding=shape[9:11], bias=bias), ref, tol, nhw


@functools.lru_cache(maxsize=None)
def residual(i, fr):
    """(codes [M, Cout], qpr [3, Cr], rref [M, Cout] fp64, sr and zr per row as fp32 columns)."""
    ref = layer(i)[2]
    top, Cr = (255 if fr == 'u8' else 15), (SHAPES[i][0] if i == 2 else 1)
    codes = torch.randint(0, top + 1, ref.shape, generator=torch.Generator().manual_seed(40 + i), dtype=torch.uint8)
    zr = torch.linspace(0.37 + top / 3, 0.37 + top / 2, Cr, dtype=torch.float64)
    qpr = torch.stack([2 * float(ref.std()) / top * torch.linspace(1, 1.5, Cr, dtype=torch.float64), zr, torch.full_like(zr, top)]).float()
    sr, zr = (qpr[k].repeat_interleave(ref.shape[0] // Cr)[:, None] for k in (0, 1))
    return codes, qpr, (codes.double() - zr.double()) * sr.double(), sr, zr


def expected(i, fr, fy, relu):
    """(qpy, sy, zy, t, allowed): the output table on the fp64 sum, the unrounded code and check 1's bound."""
    _, _, ref, tol, nhw = layer(i)
    rref, top = residual(i, fr)[2], (255 if fy == 'u8' else 15)
    qpy, sy, zy = RQ.table(ref + rref, nhw[1] * nhw[2], top, per_row=i == 2)
    t = (((ref + rref).relu() if relu else ref + rref) / sy + zy).clamp(0, top)
    return qpy, sy, zy, t, 0.5 + (tol + 2.0 ** -22 * (ref.abs() + rref.abs())) / sy + 2.0 ** -14


@pytest.mark.parametrize('relu', [False, True], ids=['linear', 'relu'])
@pytest.mark.parametrize('i,fr,fy', CASES)
def test_codes_match_fp64_and_todays_route(i, fr, fy, relu):
    from cnn_quantization_amd import ops
    (xq, wq, qpx, qpw), kw, ref, tol, nhw = layer(i)
    rcodes, qpr, rref, sr, zr = residual(i, fr)
    qpy, sy, zy, t, allowed = expected(i, fr, fy, relu)
    top, (M, N) = (255 if fy == 'u8' else 15), ref.shape
    dev = [CC.stored(xq, 'u8').cuda(), CC.stored(wq, 'u8').cuda(), qpx.cuda(), qpw.cuda(), qpy.cuda()]
    kw = dict(kw, bias=kw['bias'].cuda(), relu=relu, y_format=fy)
    rq = CC.stored(rcodes.reshape(*nhw, N), fr).cuda()
    run = lambda **more: ops.conv_codes_q(*dev, **kw, **dict(dict(residual=rq, qpr=qpr.cuda(), r_format=fr), **more))
    out = run()
    assert out.dtype == torch.uint8 and out.is_contiguous() and out.shape[-1] == (N if fy == 'u8' else N // 2) and out.numel() // out.shape[-1] == M
    codes = RQ.unpacked(out, fy, N).double()
    err = (codes - t).abs()
    print('max |code - t| = %.6f, max |code - t| / allowed = %.4f' % (float(err.max()), float((err / allowed).max())))
    assert bool((err <= allowed).all()), 'element %d: code %g, t %.6f' % (int((err - allowed).argmax()), codes.flatten()[(err - allowed).argmax()], t.flatten()[(err - allowed).argmax()])
    plain = RQ.unpacked(ops.conv_codes_q(*dev, **kw), fy, N).double()
    inside, differ = float(((codes > 0) & (codes < top)).double().mean()), float((codes != plain).double().mean())
    print('codes: top %.3f, inside %.3f, differing from the call without the residual %.3f' % (float((codes == top).double().mean()), inside, differ))
    assert codes.max() == top and inside >= 0.4 and differ >= 0.25
    y32 = ops.conv_codes(*dev[:4], **{k: v for k, v in kw.items() if k not in ('relu', 'y_format')}).cpu().permute(0, 2, 3, 1).reshape(M, N)
    assert torch.equal(codes, RQ.todays_codes(y32 + (rcodes.float() - zr) * sr, sy, zy, top, relu).double())
    if i == 2:
        held = dict(taps=ops.conv_codes_tapsums(dev[1], 'u8'))
        for more in (dict(splits=1), dict(splits=2), dict(splits=3), held, dict(held, splits=2)):
            assert torch.equal(run(**more), out), '%s changes the bytes' % more.keys()
        for s in (1, 2):
            both = rq.clone()
            assert run(residual=both, out=both, splits=s) is both and torch.equal(both, out), 'in place, %d split(s)' % s
    elif i == 0:
        assert torch.equal(run(splits=2), out)


@pytest.mark.parametrize('fy', ['u8', 'pack4'])
def test_codes_are_the_next_layers_operand(fy):
    """The returned tensor, as it is, is the xq of the next conv_codes with qpx = qpy: the fp32 result of passing CPU-built codes."""
    from cnn_quantization_amd import ops
    (xq, wq, qpx, qpw), kw, ref, tol, (N, OH, OW) = layer(1)
    (rcodes, qpr, rref, sr, zr), (qpy, sy, zy, _, _) = residual(1, fy), expected(1, fy, fy, True)
    top, C = (255 if fy == 'u8' else 15), ref.shape[1]
    dev = [CC.stored(xq, 'u8').cuda(), CC.stored(wq, 'u8').cuda(), qpx.cuda(), qpw.cuda()]
    kw = dict(kw, bias=kw['bias'].cuda())
    out = ops.conv_codes_q(*dev, qpy.cuda(), relu=True, y_format=fy, residual=CC.stored(rcodes.reshape(N, OH, OW, C), fy).cuda(), qpr=qpr.cuda(),
                           r_format=fy, **kw)
    y32 = ops.conv_codes(*dev, **kw).cpu().permute(0, 2, 3, 1).reshape(-1, C)
    built = RQ.todays_codes(y32 + (rcodes.float() - zr) * sr, sy, zy, top, True).reshape(N, OH, OW, C)
    _, wq2, _, qpw2, bias2 = CC.operands((N, OH, OW, C, 16, 1, 1, 1, 1, 0, 0), fy, 'u8', seed=3)
    nxt = lambda xq: ops.conv_codes(xq, wq2.cuda(), qpy.cuda(), qpw2.cuda(), bias=bias2.cuda(), x_format=fy)
    assert torch.equal(nxt(out), nxt(CC.stored(built, fy).cuda()))
