"""CPU restatement of the per-channel clipping-error columns (smpc.py:80-100, utils/misc.py:23-34) for the tests: the three
candidate quantizations of `-c mix` come from oracle.quant_oracle (bit-exact with the reference, tests/test_oracle_golden.py),
the sums are taken in fp64."""
import numpy as np
import torch

from oracle import quant_oracle as qo

NAMES = ('mse_lowp', 'mse_gaus', 'mse_laplace', 'cos_lowp', 'cos_gaus', 'cos_laplace')   # smpc.py:24-32
CANDS = ('lowp', 'gaus', 'laplace')
# error columns that make iq.py:310-323 pick one candidate for every channel
_FORCE = {'laplace': dict(laplace=1., gaus=2., lowp=3.), 'gaus': dict(laplace=2., gaus=1., lowp=3.),
          'lowp': dict(laplace=3., gaus=2., lowp=1.)}


def candidate_q(x, stats, cand, num_bits, positive=False, bit_alloc=False, prior_is_b=False, target=None, round_mode=True):
    """q (NCHW fp32) of candidate `cand` for the statistics `stats` (dict of [C] arrays min, max, mean, b, std)."""
    C = x.shape[1]
    mse = {k: np.full(C, v, dtype=np.float32) for k, v in _FORCE[cand].items()}
    return qo.act_clipping_mix_qdq(x, num_bits, stats, mse, half_range=positive, bit_alloc_act=bit_alloc,
                                   bit_alloc_prior='b' if prior_is_b else 'gaus', bit_alloc_target=target,
                                   bit_alloc_round=round_mode)


def error_columns(x, qs, check_no_cancellation=True):
    """[2K, C] float64: mse rows then cos rows of the quantized tensors `qs` (smpc.py:84, 96-98).  Each term is formed in
    fp32 as torch forms it, then summed in fp64.  The cosine is utils/misc.py:23-34 with dims = [-1, 0] as written: the square
    root is taken inside the loop over the dimensions."""
    N, C = x.shape[0], x.shape[1]
    xr = x.detach().reshape(N, C, -1)
    mse, cos = [], []
    with np.errstate(invalid='ignore', divide='ignore'):
        nx = np.sqrt(np.sqrt((xr * xr).double().sum(-1).numpy()).sum(0))
        for q in qs:
            qr = q.detach().reshape(N, C, -1)
            d = xr - qr
            mse.append((d * d).double().sum(-1).numpy().__truediv__(xr.shape[-1]).sum(0) / N)
            xq = (xr * qr).double()
            dot = xq.sum(-1).sum(0).numpy()
            if check_no_cancellation:
                ab = xq.abs().sum(-1).sum(0).numpy()
                fin = np.isfinite(dot)
                assert (ab[fin] <= 2 * np.abs(dot[fin])).all(), 'sum |x q| > 2 |sum x q|: the dot product cancels'
            nq = np.sqrt(np.sqrt((qr * qr).double().sum(-1).numpy()).sum(0))
            cos.append(dot / (nx * nq))
    return np.stack(mse + cos)


def host_post(rows):
    """smpc.py:113-115 on the cos rows (the second half)."""
    rows = np.array(rows, dtype=np.float32)
    K = rows.shape[0] // 2
    c = np.nan_to_num(rows[K:])
    c[c == 0] = 1.
    rows[K:] = c
    return rows


def mix_columns(x, stats, **settings):
    """The six columns in NAMES' order for the three candidates of `stats`, and the candidates' q."""
    qs = [candidate_q(x, stats, c, **settings) for c in CANDS]
    return error_columns(x, qs), qs


def stats_dict(table):
    """{min, max, mean, b, std} from a [NSTAT, C] table (rows MIN, MAX, MEAN, STD, B = 0, 1, 2, 3, 4)."""
    t = table.detach().cpu().numpy() if isinstance(table, torch.Tensor) else np.asarray(table)
    return dict(min=t[0].copy(), max=t[1].copy(), mean=t[2].copy(), std=t[3].copy(), b=t[4].copy())


def close(a, b, rel=2e-6):
    """a within rel of b where b is finite, NaN / inf where b is."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    fin = np.isfinite(b)
    same = np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~fin & ~np.isnan(b)], b[~fin & ~np.isnan(b)])
    return same and bool((np.abs(a[fin] - b[fin]) <= rel * np.abs(b[fin])).all())


def rel_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    fin = np.isfinite(b) & (b != 0)
    return float(np.max(np.abs(a[fin] - b[fin]) / np.abs(b[fin]))) if fin.any() else 0.


def mixed_input(seed=11, N=8, C=12, H=16, W=16):
    """Channels drawn from Laplace, Gaussian and uniform distributions in turn (differing scales and offsets)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.empty(N, C, H, W)
    for c in range(C):
        scale, off = 0.5 + 0.25 * c, 0.1 * (c % 5 - 2)
        if c % 3 == 0:
            u = torch.rand(N, H, W, generator=g) - 0.5
            v = -torch.sign(u) * torch.log1p(-2 * u.abs())
        elif c % 3 == 1:
            v = torch.randn(N, H, W, generator=g)
        else:
            v = torch.rand(N, H, W, generator=g) * 2 - 1
        x[:, c] = v * scale + off
    return x.float().contiguous()


def picks(mse_rows):
    """0 laplace, 1 gaus, 2 lowp per channel from rows in NAMES' order (iq.py:310-323), and the smaller of the two
    comparisons' relative margins per channel."""
    lowp, gaus, lap = (np.asarray(mse_rows[i], dtype=np.float64) for i in range(3))
    p = np.where(gaus < lap, 1, 0)
    p = np.where(lowp < gaus, 2, p)
    m1 = np.abs(gaus - lap) / np.maximum(np.abs(gaus), np.abs(lap))
    m2 = np.abs(lowp - gaus) / np.maximum(np.abs(lowp), np.abs(gaus))
    return p, np.minimum(m1, m2)
