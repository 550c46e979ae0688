"""Config 1's parameter kernel and Q/DQ on hand-built inputs: k_pt_setup from row tables and host scalars against
tests/_params.pt_params_ref (kernels/gemmlowp.cu:30-41 and iq.py:361-379, 613 restated; the batch mean as DESIGN.md 3 states
it: an fp64 sum, one division, one rounding), the power-of-two scale (int_exp) against the exact ceiling, k_pt_qdq / k_h_pt_qdq -
stochastic-rounding noise, every alignment of x, y and noise, special values, denormal and huge scales - against
oracle.quant_oracle.float2gemmlowp, and the dynamic chain and the one-launch form (its ptp_out included) against
O.gemmlowp_minmax_qdq on tensors of every sign pattern.  Everything bit for bit, NaN == NaN.  Needs an MI355X: `pytest -m gpu`."""
import math

import numpy as np
import pytest
import torch

import _params as P
from cnn_quantization_amd import _lib as L
from oracle import quant_oracle as O

pytestmark = pytest.mark.gpu

WORDS = ('scale', 'shift', 'qmax', 'true-zero flag', 'pass flag', 'range', 'offset')


@pytest.fixture(scope='module')
def ops():
    from cnn_quantization_amd import ops as _ops
    return _ops


def check_ptp(got, want, what):
    got = P.f32(got)
    for i, nm in enumerate(WORDS):
        assert P.same_bits(got[i:i + 1], want[i:i + 1]), '%s: %s is %r, the reference has %r' % (what, nm, float(got[i]), float(want[i]))


def assert_exact_sum(v, what):
    """The guard that makes bit equality of the batch mean a fair demand: the fp64 sum of these fp32 values is exact, so it
    does not depend on the order (math.fsum == the naive fp64 sum forwards and backwards)."""
    v = [float(e) for e in P.f32(v)]
    fwd = bwd = 0.
    for e in v:
        fwd += e
    for e in reversed(v):
        bwd += e
    assert math.fsum(v) == fwd == bwd, what


# ------------------------------------------------------------------------------------------------ k_pt_setup from tables
KINDS = ('mixed', 'all_pos', 'all_neg', 'max0', 'min0', 'const', 'nan_row', 'pinf_row', 'ninf_row')


def row_table(kind, rows, gen):
    """Per-row (min, max); magnitudes in [1, 901): within a factor 2^10 of each other."""
    lo = 1 + torch.rand(rows, generator=gen) * 900
    hi = 1 + torch.rand(rows, generator=gen) * 900
    if kind == 'all_pos':
        mn, mx = torch.minimum(lo, hi), torch.maximum(lo, hi)
    elif kind == 'all_neg':
        mn, mx = -torch.maximum(lo, hi), -torch.minimum(lo, hi)
    elif kind == 'max0':
        mn, mx = -lo, torch.zeros(rows)
    elif kind == 'min0':
        mn, mx = torch.zeros(rows), hi
    elif kind == 'const':
        mn, mx = torch.full((rows,), 37.5), torch.full((rows,), 37.5)
    else:
        mn, mx = -lo, hi
    r = rows // 2
    if kind == 'nan_row':
        mn[r] = mx[r] = float('nan')
    elif kind == 'pinf_row':
        mx[r] = float('inf')
    elif kind == 'ninf_row':
        mn[r] = float('-inf')
    return mn, mx


@pytest.mark.parametrize('rows', [1, 2, 63, 64, 65, 1000, 1024, 4096])
def test_pt_setup_from_tables(ops, rows):
    gen = torch.Generator().manual_seed(rows)
    for kind in KINDS:
        mn, mx = row_table(kind, rows, gen)
        if kind in KINDS[:6]:
            assert_exact_sum(mn, (kind, rows))
            assert_exact_sum(mx, (kind, rows))
        tables = []
        for stride in (rows, rows + 37):
            # a table wider than `rows`: NaN beyond the rows, so a read at the wrong stride or past `rows` shows
            t = torch.full((L.NSTAT, stride), float('nan'))
            t[L.STAT_MIN, :rows], t[L.STAT_MAX, :rows] = mn, mx
            tables.append(t.cuda())
        for rows_mode in (0, 1):
            for zero_min in (False, True):
                for etz in (True, False):
                    for bits in (2, 4, 8, 16):
                        want = P.pt_params_ref(mn, mx, rows_mode, zero_min, bits, False, etz)
                        for t in tables:
                            got = ops.pt_setup('cuda', bits, stats=t, rows=rows, rows_mode=rows_mode, zero_min=zero_min,
                                               enforce_true_zero=etz).cpu()
                            check_ptp(got, want, (kind, rows, t.shape[1], rows_mode, zero_min, etz, bits))
        if kind == 'const':
            assert P.pt_params_ref(mn, mx, 0, False, 8, False, True)[4] == 1.     # the pass flag was among them


def test_pt_setup_host_scalars(ops):
    for rng, off in ((63.75, -10.25), (0., 1.5), (0., 0.), (-1., 0.), (-0.5, -3.), (1e-30, 0.), (3e38, -1e38)):
        for etz in (True, False):
            for bits in (2, 8, 16):
                got = ops.pt_setup('cuda', bits, range_offset=(rng, off), enforce_true_zero=etz).cpu()
                want = P.pt_params_host_ref(rng, off, bits, False, etz)
                check_ptp(got, want, (rng, off, etz, bits))
                assert float(got[4]) == (1. if rng <= 0 else 0.)


# ------------------------------------------------------------------------------------------------ int_exp
def _scale_of(ops, rng, bits):
    return float(ops.pt_setup('cuda', bits, range_offset=(float(rng), 0.), int_exp=True).cpu()[0])


def test_int_exp_powers_of_two_are_kept(ops):
    """range = qmax * 2^k: the quotient is 2^k exactly and must come back as 2^k (one step up halves the resolution)."""
    for bits in (1, 4, 8):
        qmax = np.float32((1 << bits) - 1)
        for k in range(-20, 21):
            rng = np.float32(qmax * np.float32(2. ** k))
            assert np.float32(rng / qmax) == np.float32(2. ** k)
            assert _scale_of(ops, rng, bits) == 2. ** k, (bits, k)


def test_int_exp_interior_scales_round_up(ops):
    """Scales whose exact log2 has a fractional part at least 1e-5 away from 0 and from 1: 2^ceil(log2 s).  One bit (qmax 1)
    makes the scale the range itself."""
    for k in range(-20, 21):
        for f in (1e-4, 0.01, 0.3, 0.5, 0.9, 0.999, 1 - 1e-4):
            s = np.float32(2. ** (k + f))
            assert 1e-5 <= P.log2_frac(s) <= 1 - 1e-5                             # a condition on the input
            assert _scale_of(ops, s, 1) == 2. ** (k + 1), (k, f)
    for bits, rng in ((8, 63.7), (4, 11.3), (2, 0.0071)):                         # through the division by qmax
        s = np.float32(np.float32(rng) / np.float32((1 << bits) - 1))
        assert 1e-5 <= P.log2_frac(s) <= 1 - 1e-5
        assert _scale_of(ops, rng, bits) == 2. ** P.exact_ceil_log2(s), (bits, rng)


def test_int_exp_neighbours_of_powers_of_two(ops):
    """The +-1 and +-2 ulp neighbours of 2^k: a correctly rounded fp32 log2 and its own +-1 ulp neighbours disagree on the
    ceiling for most of them, so they cannot separate a right implementation from a wrong one - membership in {2^k, 2^(k+1)}
    is all that is asserted, for every one of them (none is dropped)."""
    for k in range(-20, 21):
        p = np.float32(2. ** k)
        below1 = np.nextafter(p, np.float32(0.))
        above1 = np.nextafter(p, np.float32(np.inf))
        for s in (np.nextafter(below1, np.float32(0.)), below1, above1, np.nextafter(above1, np.float32(np.inf))):
            assert _scale_of(ops, s, 1) in (2. ** k, 2. ** (k + 1)), (k, float(s))


# ------------------------------------------------------------------------------------------------ pt_qdq against float2gemmlowp
DTYPES = {'fp32': torch.float32, 'bf16': torch.bfloat16, 'fp16': torch.float16}
GUARD = 12288.                            # exact in bf16 and fp16 too


def settings(bits):
    """(range, offset): a quarter step with a zero point inside the range; a denormal scale; a huge one."""
    qmax = (1 << bits) - 1
    return [(qmax * 0.25, -0.25 * (qmax // 3) - 0.0625), (qmax * 2. ** -140, -(qmax // 3) * 2. ** -140), (3e38, -1e38)]


def values(n, rng, offset, bits, etz, gen):
    """x and noise [n]: specials first (so that the shortest vectors see some), then ties, integer quotients with +-0.5 noise,
    quotients pushed across the clamps by the noise, then uniform values with uniform noise in (-0.5, 0.5)."""
    qmax = (1 << bits) - 1
    scale = np.float32(np.float32(rng) / np.float32(qmax))
    off = np.float32(offset)
    with np.errstate(all='ignore'):
        zp = O.roundf_np(np.asarray([-off / scale], dtype=np.float32))[0]
    at = (lambda q: (np.float32(q) - zp) * scale) if etz else (lambda q: off + np.float32(q) * scale)   # x whose quotient is q
    xs, zs = [], []
    with np.errstate(all='ignore'):
        for i, v in enumerate((float('nan'), float('inf'), float('-inf'), -0.0, 0.0, 1e-42, -1e-42, 1e30, -1e30)):
            xs.append(v)
            zs.append((0.25, -0.25, 0.)[i % 3])
        for q in (0, 1, qmax // 2, qmax - 1, qmax):
            xs += [at(q + 0.5), at(q - 0.5), at(q), at(q)]
            zs += [0.125, -0.125, 0.5, -0.5]
        # the clamp comes after the noise
        xs += [at(qmax + 3), at(qmax + 0.25), at(-3), at(-0.25), at(qmax), at(0)]
        zs += [-4., -0.5, 4., 0.5, 3., -3.]
    m = len(xs)
    x = (torch.rand(max(n, m), generator=gen) * 1.2 - 0.1) * float(np.float32(rng)) + float(off)
    z = torch.rand(max(n, m), generator=gen) - 0.5
    z[z == -0.5] = 0.
    order = torch.randperm(m, generator=gen)[:n] if n < m else torch.arange(m)
    x[:len(order)] = torch.tensor(np.asarray(xs, dtype=np.float32))[order]
    z[:len(order)] = torch.tensor(np.asarray(zs, dtype=np.float32))[order]
    return x[:n].clone(), z[:n].clone()


def placed(v, off, fill=GUARD):
    """v at element 8 + off of a fresh device buffer (8 elements are 16 or 32 bytes: off = 0 is 16-byte aligned, off = 1 is
    not), guard elements before and after."""
    buf = torch.full((v.numel() + 24,), fill, dtype=v.dtype).cuda()
    assert buf.data_ptr() % 16 == 0
    view = buf[8 + off:8 + off + v.numel()]
    view.copy_(v)
    return buf, view


def equal_out(got, want):
    """Finite outputs bit for bit, NaN in the same places."""
    got, want = got.cpu(), want.cpu()
    gn, wn = torch.isnan(got), torch.isnan(want)
    it = torch.int32 if got.dtype == torch.float32 else torch.int16
    return bool(torch.equal(gn, wn) and torch.equal(got.view(it)[~gn], want.view(it)[~wn]))


@pytest.mark.parametrize('n', [1, 3, 4, 5, 7, 8, 9, 1023, 4101])
@pytest.mark.parametrize('dt', list(DTYPES))
def test_pt_qdq_against_float2gemmlowp(ops, dt, n):
    dtype = DTYPES[dt]
    gen = torch.Generator().manual_seed(n)
    for bits in (2, 4, 8):
        for si, (rng, offset) in enumerate(settings(bits)):
            for etz in (True, False):
                ptp = ops.pt_setup('cuda', bits, range_offset=(rng, offset), enforce_true_zero=etz)
                x, z = values(n, rng, offset, bits, etz, gen)
                x = x.to(dtype)
                refs = {False: O.float2gemmlowp(x.float(), rng, offset, bits, False, etz).to(dtype),
                        True: O.float2gemmlowp(x.float(), rng, offset, bits, False, etz, noise=z).to(dtype)}
                for ox, oy, oz in ((0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0), (0, 0, 1), (1, 0, 1), (0, 1, 1), (1, 1, 1)):
                    for with_noise in ((False, True) if oz == 0 else (True,)):
                        _, xv = placed(x, ox)
                        ybuf, yv = placed(torch.zeros(n, dtype=dtype), oy)
                        yv.fill_(GUARD)
                        zv = placed(z, oz)[1] if with_noise else None
                        out = ops.pt_qdq(xv, ptp, noise=zv, out=yv)
                        assert out.data_ptr() == yv.data_ptr()
                        what = (dt, n, bits, si, etz, ox, oy, oz, with_noise)
                        assert equal_out(yv, refs[with_noise]), what
                        g = ybuf.cpu().float()
                        assert bool((g[:8 + oy] == GUARD).all()) and bool((g[8 + oy + n:] == GUARD).all()), what


@pytest.mark.parametrize('dt', list(DTYPES))
def test_pt_qdq_passes_the_input_through(ops, dt):
    """range <= 0: the input's bits come back, NaN and -0.0 included (kernels/gemmlowp.cu:31-32), with and without noise."""
    dtype = DTYPES[dt]
    it = torch.int32 if dtype == torch.float32 else torch.int16
    gen = torch.Generator().manual_seed(2)
    for n in (1, 7, 9, 4101):
        x, z = values(n, 63.75, -10.25, 8, True, gen)
        x = x.to(dtype)
        for rng, offset in ((0., 1.5), (-1., 0.)):
            ptp = ops.pt_setup('cuda', 8, range_offset=(rng, offset))
            for ox, oy, oz, with_noise in ((0, 0, 0, False), (1, 1, 0, False), (0, 0, 0, True), (0, 0, 1, True), (1, 0, 1, True)):
                _, xv = placed(x, ox)
                ybuf, yv = placed(torch.zeros(n, dtype=dtype), oy)
                ops.pt_qdq(xv, ptp, noise=placed(z, oz)[1] if with_noise else None, out=yv)
                assert torch.equal(yv.cpu().view(it), x.view(it)), (dt, n, rng, ox, oy, oz, with_noise)
                g = ybuf.cpu().float()
                assert bool((g[:8 + oy] == GUARD).all()) and bool((g[8 + oy + n:] == GUARD).all())


# ------------------------------------------------------------------------------------------------ the dynamic chain and the one launch
def grid_tensor(kind, shape, gen):
    """Values on a grid of 2^-6 below 2^4 in magnitude: every fp64 sum of row extrema is exact."""
    a = (torch.randn(shape, generator=gen) * 1.5 + 0.2).clamp(-15, 15)
    if kind == 'pos':
        a = a.abs() + 0.5
    elif kind == 'neg':
        a = -(a.abs() + 0.5)
    elif kind == 'max0':
        a = -a.abs()
        a.view(shape[0], -1)[:, 1] = 0.
    elif kind == 'const':
        a = torch.full(shape, 1.25)
    return torch.round(a * 64) / 64 + 0.            # + 0.: no -0.0 (the sign of max(-0., +0.) is nobody's contract)


def fused(ops, x, rows, rows_mode, zero_min, bits, int_exp, etz):
    st = ops._raw_stream(x.device.index)
    gws = ops._group_workspace(x, st)
    assert gws is not None
    y = torch.empty_like(x)
    ptp = torch.full((8,), -1., device='cuda')
    rc = L.load().cnnq_pt_minmax_qdq_fused(x.data_ptr(), y.data_ptr(), x.numel(), rows, rows_mode, int(zero_min), bits,
                                           int(int_exp), int(etz), gws, ops.GROUP_WS_BYTES, ptp.data_ptr(), st)
    assert rc == 0, rc
    return y, ptp


@pytest.mark.parametrize('shape', [(6, 4, 9, 12), (5, 1000), (64, 8, 4, 4), (1, 3, 8, 8), (1024, 4)])
def test_dynamic_per_tensor_chain_and_one_launch(ops, shape):
    gen = torch.Generator().manual_seed(shape[0])
    rows = shape[0]
    ops.group_status(torch.empty(1, device='cuda'), clear=True)
    for kind in ('mixed', 'pos', 'neg', 'max0', 'const'):
        x = grid_tensor(kind, shape, gen)
        xd = x.cuda()
        mins, maxs = x.view(rows, -1).min(dim=1)[0], x.view(rows, -1).max(dim=1)[0]
        assert_exact_sum(mins, (kind, shape))
        assert_exact_sum(maxs, (kind, shape))
        table = ops.tensor_row_stats(xd, rows)
        assert P.same_bits(table[0].cpu(), mins) and P.same_bits(table[1].cpu(), maxs), (kind, shape)
        for avg in (True, False):
            mode = 0 if avg else 1
            mn, mx = P.pt_extrema(mins, maxs, mode, False)
            for zero_min in (False, True):
                # the power-of-two scale only where the range is positive; the scale must then be a power of two or interior
                int_exps = (False, True) if (mx - (0. if zero_min else mn)) > 0 else (False,)
                for etz in (True, False):
                    for bits in (2, 4, 8):
                        for int_exp in int_exps:
                            what = (kind, shape, avg, zero_min, etz, bits, int_exp)
                            want_p = P.pt_params_ref(mins, maxs, mode, zero_min, bits, int_exp, etz)
                            if int_exp:
                                frac = P.log2_frac(np.float32(want_p[5]) / np.float32((1 << bits) - 1))
                                assert frac == 0. or 1e-5 <= frac <= 1 - 1e-5, what    # a condition on the input
                            want = O.gemmlowp_minmax_qdq(x, bits, half_range=zero_min, enforce_true_zero=etz, int_exp=int_exp,
                                                         min_=mn, max_=mx)
                            ptp = ops.pt_setup('cuda', bits, stats=table, rows=rows, rows_mode=mode, zero_min=zero_min,
                                               int_exp=int_exp, enforce_true_zero=etz)
                            check_ptp(ptp.cpu(), want_p, what)
                            y = ops.minmax_qdq_per_tensor(xd, bits, avg, zero_min=zero_min, int_exp=int_exp,
                                                          enforce_true_zero=etz, fused=False)
                            assert equal_out(y, want), what
                            yf, ptp_f = fused(ops, xd, rows, mode, zero_min, bits, int_exp, etz)
                            assert equal_out(yf, want), what
                            assert P.same_bits(ptp_f.cpu(), ptp.cpu()), what
    assert ops.group_status(xd) == 0
