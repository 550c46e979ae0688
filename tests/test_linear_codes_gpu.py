"""ops.linear_codes against plain fp64 torch on the CPU, from the same hand-built codes and tables.

The device value is the fp64 combination of exact integers rounded once to fp32, so per element
    |y - ref| <= ulp32(ref) + 16 * 2^-53 * sx sw[n] (|S| + |zw Rx| + |zx Rw| + K |zx zw|) + 4 * 2^-53 |bias[n]|
evaluated from the reference's own terms - derived, not measured.  Within the library S, Rx and Rw are integers: forced splits of
1, 2 and 3, and a caller-held rw, give the same bits.  The shapes are the issue's: the macro tiles are 16 x 128, 64 x 64 and
128 x 128, and (130, 257, 320) is more than one of the largest each way, so none had to grow.  One had to move: pack4 admits
K % 8 == 0 only, so the cases with a pack4 operand run the ragged shape as (17, 33, 136) - still K % 16 != 0, the dword path - where
u8 / u8 keeps the issue's (17, 33, 132)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FORMATS = [('u8', 'u8'), ('u8', 'pack4'), ('pack4', 'u8'), ('pack4', 'pack4')]
COMMON = [(16, 16, 64), (1, 16, 64), (17, 33, 132), (8, 24, 136)]
CASES = [(fx, fw, (17, 33, 136) if s == (17, 33, 132) and 'pack4' in (fx, fw) else s) for fx, fw in FORMATS for s in COMMON] + [('u8', 'u8', (130, 257, 320)), ('u8', 'u8', (33, 48, 1024))]
PER_SAMPLE = {(17, 33, 132), (17, 33, 136), (130, 257, 320)}        # Cx = M on these, Cx = 1 elsewhere


def stored(codes, fmt):
    """The bytes of a code matrix in its stored format: pack4 is two codes per byte, the even element in the low nibble."""
    c = codes.numpy()
    return torch.from_numpy(c if fmt == 'u8' else (c[:, 0::2] | (c[:, 1::2] << 4)))


def operands(M, N, K, fx, fw, seed):
    g = torch.Generator().manual_seed(seed)
    qx, qw = (255 if fx == 'u8' else 15), (255 if fw == 'u8' else 15)
    xq = torch.randint(0, qx + 1, (M, K), generator=g, dtype=torch.uint8)
    wq = torch.randint(0, qw + 1, (N, K), generator=g, dtype=torch.uint8)
    wq[0], wq[1] = 0, qw
    if M > 2:
        xq[0], xq[1] = 0, qx
    Cx = M if (M, N, K) in PER_SAMPLE else 1
    qpx = torch.empty(3, Cx)
    qpx[0] = torch.linspace(0.0371, 0.9, Cx)
    qpx[1] = torch.linspace(-3.25, qx + 0.5, Cx) if Cx > 1 else 127.5
    qpx[2] = qx
    qpw = torch.empty(3, N)
    qpw[0] = torch.logspace(-8, np.log10(3.0), N)
    qpw[1] = torch.rand(N, generator=g) * (qw + 20) - 10.3
    qpw[1, 0], qpw[1, 1] = 127.5, -7.3
    qpw[2] = qw
    return xq, wq, qpx, qpw, torch.randn(N, generator=g) * 3


def reference(xq, wq, qpx, qpw, bias):
    """(ref, tolerance) in fp64, per element."""
    K = xq.shape[1]
    X, W = xq.double(), wq.double()
    sx, zx, sw, zw = qpx[0].double()[:, None], qpx[1].double()[:, None], qpw[0].double()[None, :], qpw[1].double()[None, :]
    b = bias.double()[None, :] if bias is not None else torch.zeros(1, wq.shape[0], dtype=torch.float64)
    ref = ((X - zx) * sx) @ ((W - zw.T) * sw.T).T + b
    Rx, Rw = X.sum(1, keepdim=True), W.sum(1)[None, :]
    mag = sx * sw * ((X @ W.T).abs() + (zw * Rx).abs() + (zx * Rw).abs() + K * (zx * zw).abs())
    ulp = torch.from_numpy(np.spacing(ref.abs().numpy().astype(np.float32)).astype(np.float64))
    return ref, ulp + 16 * 2.0 ** -53 * mag + 4 * 2.0 ** -53 * b.abs()


def run(xq, wq, qpx, qpw, bias, fx, fw, **kw):
    from cnn_quantization_amd import ops
    d = [t.cuda() if t is not None else None for t in (stored(xq, fx), stored(wq, fw), qpx, qpw, bias)]
    y = ops.linear_codes(d[0], d[1], d[2], d[3], bias=d[4], x_format=fx, w_format=fw, **kw)
    assert y.dtype == torch.float32 and y.shape == (xq.shape[0], wq.shape[0])
    return y.cpu()


def check(y, ref, tol, what):
    err = (y.double() - ref).abs()
    worst = int((err - tol).argmax())
    print('%s: max |y - ref| / tol = %.3g' % (what, float((err / tol).max())))
    assert bool((err <= tol).all()), '%s: element %d is off by %.3e, allowed %.3e' % (what, worst, float(err.flatten()[worst]), float(tol.flatten()[worst]))


@pytest.mark.parametrize('fx,fw,shape', CASES, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else v)
def test_linear_codes_matches_fp64_reference(fx, fw, shape):
    from cnn_quantization_amd import ops
    M, N, K = shape
    xq, wq, qpx, qpw, bias = operands(M, N, K, fx, fw, seed=M * 1000 + N)
    forced = 3 if shape == (33, 48, 1024) else 0
    for b in (bias, None):
        ref, tol = reference(xq, wq, qpx, qpw, b)
        y = run(xq, wq, qpx, qpw, b, fx, fw, splits=forced)
        check(y, ref, tol, 'bias' if b is not None else 'no bias')
    # integers underneath: the split count and a held rw change no bit (y: the last run, without bias)
    for s in (1, 2, 3):
        assert torch.equal(run(xq, wq, qpx, qpw, None, fx, fw, splits=s), y), 'splits = %d changes the result' % s
    rw = ops.linear_codes_rowsums(stored(wq, fw).cuda(), fw)
    assert torch.equal(rw.cpu(), wq.sum(1, dtype=torch.int32))
    assert torch.equal(run(xq, wq, qpx, qpw, None, fx, fw, rw=rw), y), 'a held rw changes the result'


@pytest.mark.parametrize('wcode', [0, 255])
def test_extreme_accumulation(wcode):
    """Every activation code 255 against every weight code 0 / 255 over K = 4096: the signed re-centring at both ends of the byte
    and 4096 * 127 * 127 in one int32 accumulator."""
    M, N, K = 16, 16, 4096
    xq, wq = torch.full((M, K), 255, dtype=torch.uint8), torch.full((N, K), wcode, dtype=torch.uint8)
    qpx = torch.tensor([[0.0371], [127.5], [255.]])
    qpw = torch.stack([torch.logspace(-8, np.log10(3.0), N), torch.linspace(-7.3, 250.7, N), torch.full((N,), 255.)])
    ref, tol = reference(xq, wq, qpx, qpw, None)
    check(run(xq, wq, qpx, qpw, None, 'u8', 'u8'), ref, tol, 'wq = %d' % wcode)
