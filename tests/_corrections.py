"""The two correction chains of csrc/cnnq_corrections.hip.h restated on the CPU, and the inputs that make their tests exact -
helper, no tests.

Activation bias correction (iqm.py:188-196, include/cnnq_hip.h "Activation bias correction"): sums64 is the per-channel sums in
float64, bias32 / apply32 the reference's float32 expressions with every operation rounded on its own.  Weight correction
(iqm.py:374-391): weight32.  Nothing here is computed in any other precision, and nothing takes a tolerance.

dyadic() draws activations on multiples of 1/8 in [-8, 8] and parameter tables whose every Q/DQ value is a multiple of 1/4 below
2^9: whatever partial sums a kernel forms of them - float32 quads, float64 lanes, LDS folds, records - are exact, so the merged
sums must EQUAL sums64 (test_corrections_cpu.py proves the premise in integers).  The *_wrong functions restate the expressions the
way a plausible slip in a kernel would; the CPU test demands that the hand-built inputs tell them from the right ones, so that a
case cannot pass on the device by having nothing at stake."""
import numpy as np
import torch

F = np.float32
EPS = F(1e-8)
RTOL_SUMS = 2e-6                     # |sum - fp64| <= RTOL_SUMS * sum |term|: DESIGN.md section 15, item 1
QP_SCALE, QP_ZP, QP_QMAX, NQP = 0, 1, 2, 3
STAT_MEAN, STAT_STD, NSTAT = 2, 3, 7        # pinned to _lib in the CPU test


def f32(a):
    return np.ascontiguousarray(a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a, dtype=F)


def rows(t):
    """[N, C, H, W] -> the [C, N*H*W] view a channel's reduction runs over"""
    t = np.asarray(t)
    return np.moveaxis(t.reshape(t.shape[0], t.shape[1], -1), 1, 0).reshape(t.shape[1], -1)


def same(a, b):
    """Bit equality with NaN == NaN (float32 or float64): the device and x86 sign the NaN of 0 * inf differently."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype or a.dtype not in (np.float32, np.float64):
        return False
    bits = np.uint32 if a.dtype == np.float32 else np.uint64
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(bits)[~na], b.view(bits)[~nb]))


def where_differ(a, b):
    """the first few positions where `same` fails, for an assertion message"""
    a, b = np.asarray(a), np.asarray(b)
    bad = ~((a == b) & (np.signbit(a) == np.signbit(b)) | (np.isnan(a) & np.isnan(b)))
    idx = np.argwhere(bad)[:4]
    return [(tuple(int(j) for j in i), a[tuple(i)], b[tuple(i)]) for i in idx]


# ------------------------------------------------------------------------------------------ activation bias correction
def relu32(x):
    """fmaxf(x, 0): a NaN is dropped, as k_bcorr_sums does"""
    return np.fmax(f32(x), F(0))


def sums64(x, q, relu_first):
    """([3, C] float64: sum x', sum q, count(x' > 0); [2, C] float64: sum |x'|, sum |q|), x' = fmaxf(x, 0) when relu_first"""
    x, q = f32(x), f32(q)
    v = rows(relu32(x) if relu_first else x).astype(np.float64)
    w = rows(q).astype(np.float64)
    sums = np.stack([v.sum(1), w.sum(1), (v > 0).sum(1).astype(np.float64)])
    return sums, np.stack([np.abs(v).sum(1), np.abs(w).sum(1)])


def bias32(sums):
    """(f32(sum x') - f32(sum q)) / (f32(count) + 1e-8f), three float32 operations (iqm.py:192-194)"""
    s = np.asarray(sums, dtype=np.float64)
    with np.errstate(all='ignore'):
        d = s[0].astype(F) - s[1].astype(F)
        return (d / (s[2].astype(F) + EPS)).astype(F)


def bias32_wrong(sums):
    """the difference taken in float64 and rounded once"""
    s = np.asarray(sums, dtype=np.float64)
    with np.errstate(all='ignore'):
        return ((s[0] - s[1]).astype(F) / (s[2].astype(F) + EPS)).astype(F)


def bias32_wrong_count(sums):
    """the count kept in float64 until the division"""
    s = np.asarray(sums, dtype=np.float64)
    with np.errstate(all='ignore'):
        d = (s[0].astype(F) - s[1].astype(F)).astype(np.float64)
        return (d / (s[2] + np.float64(EPS))).astype(F)


def apply32(q, bias):
    """q + (q > 0) * bias[c] in float32, the product first (iqm.py:196)"""
    q, b = f32(q), f32(bias).reshape(1, -1, 1, 1)
    with np.errstate(all='ignore'):
        return (q + (q > 0).astype(F) * b).astype(F)


def qdq32(x, qp):
    """the Q/DQ of include/cnnq_hip.h (iq.py:573-592) with a table qp[NQP][C], float32, one rounding per operation"""
    x, qp = f32(x), f32(qp)
    sc, zp, qm = (qp[r].reshape(1, -1, 1, 1) for r in (QP_SCALE, QP_ZP, QP_QMAX))
    with np.errstate(all='ignore'):
        c = x / sc
        c = c + zp
        c = np.where(c > qm, qm, c)
        c = np.where(c < 0, F(0), c)
        c = np.rint(c)
        return ((c - zp) * sc).astype(F)


# ------------------------------------------------------------------------------------------ weight correction
def weight32(wq, mean_w, std_w, mean_q, std_q, vcorr, bcorr):
    """iqm.py:374-391 on wq[C][HW] in float32: vc = std_w / (std_q + 1e-8f); vcorr: v = (v - mean_q) * vc + mean_q; bcorr:
    v = v - mean_q + mean_w, left to right; every operation rounded on its own"""
    v = f32(wq).copy()
    mw, sw, mq, sq = (f32(t).reshape(-1, 1) for t in (mean_w, std_w, mean_q, std_q))
    with np.errstate(all='ignore'):
        vc = sw / (sq + EPS)
        if vcorr:
            v = (v - mq) * vc + mq
        if bcorr:
            v = (v - mq) + mw
    return v.astype(F)


def weight32_fma(wq, mean_w, std_w, mean_q, std_q, vcorr, bcorr):
    """weight32 with the variance correction as one fused multiply-add (the product of two float32 is exact in float64)"""
    v = f32(wq).copy()
    mw, sw, mq, sq = (f32(t).reshape(-1, 1) for t in (mean_w, std_w, mean_q, std_q))
    with np.errstate(all='ignore'):
        vc = sw / (sq + EPS)
        if vcorr:
            v = ((v - mq).astype(np.float64) * vc.astype(np.float64) + mq.astype(np.float64)).astype(F)
        if bcorr:
            v = (v - mq) + mw
    return v.astype(F)


def weight32_assoc(wq, mean_w, std_w, mean_q, std_q, vcorr, bcorr):
    """weight32 with the mean correction as v - (mean_q - mean_w)"""
    v = f32(wq).copy()
    mw, sw, mq, sq = (f32(t).reshape(-1, 1) for t in (mean_w, std_w, mean_q, std_q))
    with np.errstate(all='ignore'):
        vc = sw / (sq + EPS)
        if vcorr:
            v = (v - mq) * vc + mq
        if bcorr:
            v = v - (mq - mw)
    return v.astype(F)


def stat_table(C, mean, std):
    """[NSTAT, C] float32 with the MEAN and STD rows filled and NaN everywhere else: k_weight_correct reads those two rows alone"""
    t = np.full((NSTAT, C), np.nan, dtype=F)
    t[STAT_MEAN], t[STAT_STD] = f32(mean), f32(std)
    return t


# (C, HW): one element; odd both; a linear layer; the 7x7x3 stem; bx capped at 64 -> a second, ragged sweep of the grid-stride
# loop (64 * 256 = 16384 < 16389); the widest legal grid
WEIGHT_CASES = [(1, 1), (3, 9), (10, 64), (24, 147), (5, 16389), (65535, 1)]
# what a channel's table entries are chosen for, by channel index modulo len(WEIGHT_KINDS)
WEIGHT_KINDS = ('plain', 'std_q_zero', 'std_w_zero', 'mean_q_is_element', 'plain', 'negative_means')


def weight_case(C, HW, seed):
    """wq[C][HW] like 4-bit weights (a 16-level grid per channel, so (v - mean_q) * vc + mean_q rounds in earnest) and the four
    table rows; channel c is of kind WEIGHT_KINDS[c % 6]"""
    rng = np.random.default_rng(seed)
    step = (0.004 + 0.01 * rng.random(C)).astype(F).reshape(C, 1)
    lo = (-0.06 + 0.02 * rng.standard_normal(C)).astype(F).reshape(C, 1)
    wq = (rng.integers(0, 16, size=(C, HW)).astype(F) * step + lo).astype(F)
    mean_q = (wq.astype(np.float64).mean(1) + 1e-4 * rng.standard_normal(C)).astype(F)
    mean_w = (mean_q + (2e-3 * rng.standard_normal(C)).astype(F)).astype(F)
    std_q = (0.03 + 0.02 * rng.random(C)).astype(F)
    std_w = (std_q * (0.8 + 0.4 * rng.random(C)).astype(F)).astype(F)
    for c in range(C):
        kind = WEIGHT_KINDS[c % len(WEIGHT_KINDS)]
        if kind == 'std_q_zero':
            std_q[c] = 0.                                   # vc = std_w / 1e-8f
        elif kind == 'std_w_zero':
            std_w[c] = 0.                                   # vc = 0: every element becomes mean_q (then mean_w)
        elif kind == 'mean_q_is_element':
            mean_q[c] = wq[c, (c // len(WEIGHT_KINDS)) % HW]   # (v - mean_q) = 0 there
        elif kind == 'negative_means':
            mean_q[c], mean_w[c] = -abs(mean_q[c]) - F(0.01), -abs(mean_w[c]) - F(0.02)
    return wq, mean_w, std_w, mean_q, std_q


# ------------------------------------------------------------------------------------------ inputs
def dyadic(shape, seed):
    """x[N][C][H][W] float32 on multiples of 1/8 in [-8, 8], drawn per element, with an exact +0.0 and -0.0 in channel 0 and -
    C > 1 - the last channel all negative (count 0); qp[NQP][C]: scale in {1/4, 1/2, 1}, integer zero point 0..8, qmax in
    {0, 3, 15, 255}, so that every (code - zp) * scale is a multiple of 1/4 of magnitude below 2^9"""
    N, C, H, W = shape
    assert H * W >= 2
    rng = np.random.default_rng(seed)
    x = (rng.integers(-64, 65, size=shape).astype(np.float64) / 8.).astype(F)
    if C > 1:
        x[:, C - 1] = -np.abs(x[:, C - 1]) - F(0.125)
        x[:, C - 1] = np.maximum(x[:, C - 1], F(-8))
    flat = x[0, 0].reshape(-1)
    flat[0], flat[1] = F(0.), F(-0.)
    qp = np.empty((NQP, C), dtype=F)
    qp[QP_SCALE] = np.asarray([0.25, 0.5, 1.], dtype=F)[rng.integers(0, 3, size=C)]
    qp[QP_ZP] = rng.integers(0, 9, size=C).astype(F)
    qp[QP_QMAX] = np.asarray([0., 3., 15., 255.], dtype=F)[rng.integers(0, 4, size=C)]
    return x, qp


def gaussian(shape, seed):
    """randn * U(0.2, 3.2) per channel + randn per channel, as tests/test_fuzz_gpu.py::make"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g) * (0.2 + 3 * torch.rand(1, shape[1], 1, 1, generator=g)) \
        + torch.randn(1, shape[1], 1, 1, generator=g)
    return f32(x)


# The load shapes of k_bcorr_sums / k_bcorr_apply / k_qdq_bias (with_shape of cnnq_plan.hip.h), each crossed with the fold it can
# take.  (N, C, H, W), element offset of the base pointer, the words of cnnq_plan_describe(N, C, HW, aligned16, 0) the case stands
# for: vec, A, J, mode, nb, k, ncb, S and - mode 1 - w.
CLASSES = [
    ((3, 5, 7, 7), 0, dict(vec=1, A=1, J=4, mode=2, nb=1, k=20, ncb=1, S=3)),             # C*HW no multiple of 4: scalar loads
    ((4, 16, 14, 14), 1, dict(vec=1, A=1, J=4, mode=2, nb=1, k=5, ncb=4, S=4)),           # the aligned shape forced scalar
    ((2, 3, 33, 35), 0, dict(vec=1, A=1, J=4, mode=1, nb=2, w=578, k=1, ncb=6, S=2)),     # scalar, two workgroups per channel
    ((3, 8, 7, 7), 0, dict(vec=4, A=4, J=1, mode=2, nb=1, k=20, ncb=1, S=3)),             # straddle, m = 4
    ((2, 6, 5, 10), 0, dict(vec=4, A=4, J=1, mode=2, nb=1, k=20, ncb=1, S=2)),            # straddle, m = 2
    ((4, 16, 14, 14), 0, dict(vec=4, A=1, J=1, mode=2, nb=1, k=5, ncb=4, S=4)),
    ((3, 2, 40, 52), 0, dict(vec=4, A=1, J=1, mode=1, nb=3, w=174, k=1, ncb=6, S=3)),     # 520 = 174 + 174 + 172 columns
    ((2, 3, 72, 72), 0, dict(vec=4, A=1, J=4, mode=1, nb=2, w=648, k=1, ncb=6, S=2)),
    ((64, 320, 14, 14), 0, dict(vec=4, A=1, J=2, mode=2, nb=1, k=10, ncb=32, S=64)),      # 4 M elements: the smallest J = 2 in mode 2
    ((64, 640, 14, 14), 0, dict(vec=4, A=1, J=4, mode=2, nb=1, k=20, ncb=32, S=64)),      # 8 M elements: the smallest J = 4 in mode 2
    ((70, 5, 3, 3), 0, dict(vec=1, A=1, J=4, mode=2, nb=1, k=113, ncb=1, S=64)),          # 70 samples over 64 splits: 1 or 2 each
    ((130, 7, 1, 3), 0, dict(vec=1, A=1, J=4, mode=2, nb=1, k=256, ncb=1, S=64)),         # 2 or 3 samples each, k capped at MAXCH
    ((16, 520, 2, 2), 0, dict(vec=4, A=1, J=1, mode=2, nb=1, k=256, ncb=3, S=16)),        # k = MAXCH, the last block holds 8 channels
    ((5, 1, 6, 6), 0, dict(vec=4, A=1, J=1, mode=2, nb=1, k=28, ncb=1, S=5)),             # C = 1
    ((1, 300, 4, 4), 0, dict(vec=4, A=1, J=1, mode=2, nb=1, k=64, ncb=5, S=1)),           # N = 1
]
BIG = 1 << 20                                                                   # the two cases above it run the sums alone
PLAN_WORDS = ('vec', 'A', 'J', 'mode', 'nb', 'w', 'k', 'ncb', 'S', 'threads', 'G')


def class_id(case):
    shape, off, want = case
    return 'x'.join(map(str, shape)) + ('+%d' % off if off else '')


# ------------------------------------------------------------------------------------------ hand-built merge records
MERGE_G = (1, 2, 63, 64, 65, 130, 256)       # one record; fewer than a wave; 64 +- 1: a lane's second record; 256 = MAXG * nb
MERGE_C = (1, 3, 4, 5, 1031)                 # four waves per workgroup, a channel each: C % 4 != 0 leaves the last workgroup short
# named channels: (sum x', sum q, count) the records of the channel add up to
NAMED = {
    'two_roundings': (2. ** 25 + 1, 2. ** 25, 4.),           # f32(a) - f32(b) = 0, f32(a - b) = 1
    'count_zero': (5., 0., 0.),                              # 5 / 1e-8f
    'count_2p24_plus_1': (2. ** 24, 0., 2. ** 24 + 1),       # f32(count) = 2^24: bias 1, not 0.99999994
    'equal_sums': (12345., 12345., 7.),                      # +0
    'nan_record': (float('nan'), 3., 2.),
    'negative': (3., 10., 7.),
}
NAMES = tuple(NAMED)


def record_value(g, c, row):
    """an integer below 2^21 that tells (g, c, row) apart from its neighbours in every direction"""
    return float((g * 257 + c * 19 + row * 7) % 1999 + row + 1)


def merge_records(G, C, rot=0):
    """part3[G][3][C] float64 of integer values (any order of addition is exact), and {channel: name} of the named channels:
    channels 0..5 and the last six of C > 12 take the six names, rotated by rot; their record 0 is what is left of the named
    total after records 1..G-1, so every record still differs from its neighbours"""
    g, r, c = np.meshgrid(np.arange(G), np.arange(3), np.arange(C), indexing='ij')
    part = ((g * 257 + c * 19 + r * 7) % 1999 + r + 1).astype(np.float64)
    named = {}
    chans = list(range(min(C, len(NAMES)))) + (list(range(C - len(NAMES), C)) if C > 2 * len(NAMES) else [])
    for i, ch in enumerate(chans):
        name = NAMES[(i + rot) % len(NAMES)]
        named[ch] = name
        for row, total in enumerate(NAMED[name]):
            part[0, row, ch] = total - part[1:, row, ch].sum()
    return part, named


# ------------------------------------------------------------------------------------------ hand-built bias and y
# positive, negative, +0, -0, one that carries every q of a Gaussian channel across zero, inf, NaN, a float32 denormal
BIAS_VALUES = np.asarray([1.25, -0.75, 0., -0., -1000., np.inf, np.nan, 3e-39], dtype=F)


def hand_bias(C, rot=0):
    return BIAS_VALUES[(np.arange(C) + rot) % len(BIAS_VALUES)].copy()


def hand_y(shape, seed):
    """Gaussian values (so q + bias rounds in earnest) with +0.0, -0.0, a float32 denormal and a NaN written over the first
    elements of the first sample's channel 0 and - spread over the tensor - over one element in 13"""
    y = gaussian(shape, seed)
    special = np.asarray([0., -0., 1e-40, np.nan, -1e-40], dtype=F)
    flat = y.reshape(-1)
    n = min(len(special), shape[2] * shape[3])
    flat[:n] = special[:n]
    idx = np.arange(11, flat.size, 13)
    flat[idx] = special[np.arange(idx.size) % len(special)]
    return y
