"""What tests/test_half_collect_cpu.py and tests/test_half_collect_gpu.py share: the inputs, the plan of
cnnq_pc_stats_dt restated in Python, and a torch model of the kernels' summation."""
import torch

H_MM_ELEMS, H_ST_MAX_RECORDS = 16384, 2048        # csrc/cnnq_half.hip.h, csrc/cnnq_half_stats.hip.h
NMOM, NDEV = 7, 2

# (shape, storage offset in elements) -> (W, batch splits S, column splits): the smallest shapes that reach each branch
CASES = [((8, 12, 28, 28), 0, (8, 1, 1)),           # W = 8
         ((5, 6, 80, 80), 0, (8, 2, 1)),            # W = 8, two uneven batch splits (2 and 3 samples)
         ((3, 10, 14, 14), 0, (4, 1, 1)),           # W = 4
         ((3, 6, 7, 14), 0, (2, 1, 1)),             # W = 2
         ((2, 64, 7, 7), 0, (1, 1, 1)),             # W = 1
         ((4, 520, 7, 7), 0, (1, 1, 1)),            # W = 1, many channels
         ((1, 4, 224, 224), 0, (8, 1, 4)),          # column splits of the rows
         ((2, 3, 224, 224), 0, (8, 2, 3)),          # batch splits and uneven column splits together
         ((8, 12, 28, 28), 1, (1, 1, 1)),           # a view at an odd element offset: W = 1
         ((3, 5, 7, 7), 0, (1, 1, 1)),              # W = 1, C * HW odd
         ((3, 5, 7, 7), 1, (1, 1, 1)),              # ... at an odd element offset
         ((1, 3, 225, 225), 0, (1, 1, 4)),          # W = 1 with column splits (a class the route keeps on the upcast)
         ((3, 4, 1, 7), 0, (1, 1, 1))]              # W = 1 on very short rows
IDS = ['%s+%d' % ('x'.join(map(str, s)), o) for s, o, _ in CASES]


def seed_of(shape, offset):
    return shape[0] + shape[1] + shape[2] + offset


def values(shape, seed=0):
    """Per-channel Laplace-like activations with a moderate mean: the generator of tests/test_channels_last_collect_gpu.py."""
    g = torch.Generator().manual_seed(seed)
    C = shape[1]
    return torch.randn(shape, generator=g) * (0.2 + 3 * torch.rand(1, C, 1, 1, generator=g)) + torch.randn(1, C, 1, 1, generator=g)


def piece(HW, align, esize=2):
    """The widest of 8 / 4 / 2 / 1 elements that divides HW and the alignment (h_piece)."""
    return next((w for w in (8, 4, 2) if HW % w == 0 and align % (w * esize) == 0), 1)


def splits(N, C, HW):
    """(batch splits S, column splits) of h_stats_splits: ~H_MM_ELEMS elements per workgroup, at most H_ST_MAX_RECORDS records per
    channel and a grid below 2^31; batch splits first, then at most HW / 8 parts of a row."""
    total = max(1, min(-(-N * HW // H_MM_ELEMS), N * HW, H_ST_MAX_RECORDS))
    while total > 1 and C * total >= 1 << 31:
        total -= 1
    S = min(total, N)
    return S, min(total // S, max(1, HW // 8))


def owners(N, HW, W, S, cs):
    """For every record s of a channel the (samples, pieces) it owns, as h_part cuts them."""
    ppr = HW // W
    out = []
    for s in range(S * cs):
        sn, sp = divmod(s, cs)
        out.append((range(sn * N // S, (sn + 1) * N // S), range(sp * ppr // cs, (sp + 1) * ppr // cs)))
    return out


def native(N, HW):
    """The "native" word of cnnq_pc_route_stats_dt (h_stats_native): rows of an odd length load single elements whatever the
    alignment, and where a channel's population fills a whole workgroup they did not win against the upcast route."""
    return int(not (HW % 2 == 1 and N * HW >= H_MM_ELEMS))


def piece_sum(v):
    """The fp32 sum of the last axis (W values of a piece) in the kernels' order: pairs (0,1) + (2,3) + ... lane by lane, then
    the two halves; a single value as it is."""
    W = v.shape[-1]
    if W == 1:
        return v[..., 0]
    p = v[..., 0:2].clone()
    for i in range(2, W, 2):
        p = p + v[..., i:i + 2]
    return p[..., 0] + p[..., 1]


def model(x, W):
    """(mean, std, b, kurtosis, std_pos) of x [N, C, H, W'] (fp32 values) as the kernels form them: fp32 piece sums (squares in
    fp64 at W = 1), fp64 accumulation and merges, fp32 rows; d = x - mean in fp32, |d| and (d * (1 / std))^4 into fp64 element by
    element."""
    N, C = x.shape[:2]
    t = x.reshape(N, C, -1, W).transpose(0, 1).reshape(C, -1, W)
    R = t.shape[1] * W
    r = t.clamp(min=0)
    s, rs = piece_sum(t).double().sum(1), piece_sum(r).double().sum(1)
    if W == 1:
        ss, rss = (t.double() ** 2).sum((1, 2)), (r.double() ** 2).sum((1, 2))
    else:
        ss, rss = piece_sum(t * t).double().sum(1), piece_sum(r * r).double().sum(1)
    mean64 = s / R
    mean = mean64.float()
    std = ((ss - s * mean64) / (R - 1)).clamp(min=0).sqrt().float()
    std_pos = ((rss - rs * (rs / R)) / (R - 1)).clamp(min=0).sqrt().float()
    d = t - mean[:, None, None]
    b = (d.abs().double().sum((1, 2)) / R).float()
    z = d * (1.0 / std)[:, None, None]
    z2 = z * z
    kurt = ((z2 * z2).double().sum((1, 2)) / R - 3.).float()
    return mean, std, b, kurt, std_pos
