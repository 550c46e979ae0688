"""Config 2's per-channel parameter arithmetic restated in numpy float32, the table of named channels that reaches its edges, and
the builder of tensors whose per-channel extrema are that table.

The arithmetic (iq.py = pytorch_quantizer/quantization/qtypes/int_quantizer.py of the reference) is written out by hand at seven
sites of the library - k_minmax_params, gathered_params, k_mmq_group, k_mmq_flat, the resident kernel, h_params and, through
k_minmax_params, the channels_last front.  test_minmax_params_cpu.py pins this file to the oracle and proves that every named
channel has something at stake; test_minmax_params_table_gpu.py holds every site to it bit for bit.  No tolerance anywhere."""
import numpy as np
import torch

F32 = np.float32
H = float.fromhex
FLOOR = F32(1e-8)
P70, P30 = F32(2.0 ** 70), F32(2.0 ** 30)


# ------------------------------------------------------------------------------------------ the restatement
def qmax_ref(num_bits):
    return F32(2. ** num_bits - 1.)                       # iq.py:560 - a Python double, rounded once when it meets the tensor


def params_ref(mn, mx, num_bits, positive):
    """(scale, zp, qmax) of channels with extrema mn, mx: one operation per line, every one rounded to float32."""
    mn = np.asarray(mn, dtype=F32)
    mx = np.asarray(mx, dtype=F32)
    with np.errstate(all='ignore'):
        qmax = qmax_ref(num_bits)                         # iq.py:560
        offset = np.zeros_like(mn) if positive else mn    # iq.py:411-416: min_ = 0 under half_range / force_positive
        delta = mx - offset                               # iq.py:447: max_ - min_
        scale = delta / qmax                              # iq.py:561 (qmin = 0), an fp32 division
        scale = np.maximum(scale, FLOOR)                  # iq.py:566: torch.max propagates NaN, and so does np.maximum
        q = offset / scale                                # iq.py:570
        zp = np.rint(F32(0) - q)                          # iq.py:570,572: round(qmin - q), half to even; 0 - (+0) is +0
    return scale.astype(F32), zp.astype(F32), qmax


def fast_domain_ref(mn, mx, scale):
    """qdq_fast_domain in its words: |min|, |max| <= 2^70 and scale <= 2^30; false for NaN / inf extrema."""
    mn, mx, scale = (np.asarray(v, dtype=F32) for v in (mn, mx, scale))
    with np.errstate(all='ignore'):
        return (np.abs(mn) <= P70) & (np.abs(mx) <= P70) & (scale <= P30)


def qdq_ref(x, scale, zp, qmax):
    """(y, codes as float32) for x [N, C, ...] and per-channel scale / zp [C]: every rounding of oracle.quant_oracle.qdq_core."""
    x = np.asarray(x, dtype=F32)
    shape = (1, -1) + (1,) * (x.ndim - 2)
    s, z = np.asarray(scale, dtype=F32).reshape(shape), np.asarray(zp, dtype=F32).reshape(shape)
    with np.errstate(all='ignore'):
        q = x / s                                         # iq.py:573
        q = q + z                                         # iq.py:574
        q = np.where(q < F32(0), F32(0), q)               # iq.py:580 clamp_: NaN passes, as torch.clamp passes it
        q = np.where(q > qmax, qmax, q)
        q = np.rint(q).astype(F32)                        # iq.py:580 round_: half to even
        y = q + (-z)                                      # iq.py:591
        y = y * s                                         # iq.py:592
    return y.astype(F32), q


def same_bits(a, b):
    """float32 words equal bit for bit, NaN as a class (a NaN's sign and payload are not pinned)."""
    a, b = np.ascontiguousarray(a, dtype=F32), np.ascontiguousarray(b, dtype=F32)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na], b.view(np.uint32)[~nb]))


def first_diff(a, b):
    a, b = np.ascontiguousarray(a, dtype=F32), np.ascontiguousarray(b, dtype=F32)
    if a.shape != b.shape:
        return 'shapes', a.shape, b.shape
    na, nb = np.isnan(a), np.isnan(b)
    bad = (na != nb) | (~na & ~nb & (a.view(np.uint32) != b.view(np.uint32)))
    idx = np.argwhere(bad)
    if not len(idx):
        return None
    i = tuple(idx[0])
    return len(idx), i, float(a[i]).hex() if not na[i] else 'nan', float(b[i]).hex() if not nb[i] else 'nan'


# ------------------------------------------------------------------------------------------ the named channels
# (name, mn, mx), every value exact in float32.  A table belongs to one (num_bits, positive): the arithmetic a name is about
# depends on both.  The 1e-8 floor at 4 bits: f32(delta / 15) is 0x1.5798ecp-27, 0x1.5798eep-27 = f32(1e-8) and 0x1.5798f2p-27 for
# three consecutive floats delta - 0x1.5798f0p-27, the float just above the floor, is the quotient of no float32 by 15, so
# floor_above is the smallest scale above the floor that 4 bits can reach (asserted on the CPU).
_D_BELOW, _D_AT, _D_ABOVE = F32(H('0x1.421f5ep-23')), F32(H('0x1.421f60p-23')), F32(H('0x1.421f62p-23'))
_M23 = F32(2.0 ** -23)
_INF, _NAN = F32(np.inf), F32(np.nan)
_BIG = F32(H('0x1.cp127'))                               # 2.98e38, exact in bfloat16: twice it overflows float32

_COMMON = [
    ('mixed', -1.75, 3.5),
    ('all_pos', 0.5, 6.0),
    ('const_quarter', 0.25, 0.25),                       # delta 0: the floor, zero point -2.5e7 (0 under positive)
    ('const_zero', 0.0, 0.0),
    ('const_2p70', 2.0 ** 70, 2.0 ** 70),                # inside the fast domain at the floor: a quotient of 1.2e29 against -1.2e29
    ('denormal', -(2.0 ** -133), 2.0 ** -132),           # -9.2e-41, 1.8e-40
    ('pinf', -1.0, _INF),
    ('ninf', -_INF, 1.0),
    ('nan', _NAN, _NAN),
]
TABLES = {
    (4, False): _COMMON + [
        ('all_neg', -7.25, -0.125),
        ('floor_below', -_M23, _D_BELOW - _M23),
        ('floor_at', -_M23, _D_AT - _M23),
        ('floor_above', -_M23, _D_ABOVE - _M23),
        ('tie_down', -1.5, 13.5),                        # offset / scale = -1.5: half-even 2, half-away 2
        ('tie_up', -2.5, 12.5),                          # -2.5: half-even 2, half-away 3
        ('neg_zero_zp', 0.125, 15.125),                  # 0 < mn << scale = 1: round(0 - 0.125) is -0
        ('scale_at_2p30', -(2.0 ** 30), 14 * 2.0 ** 30),
        ('scale_above_2p30', -(2.0 ** 30), 14 * 2.0 ** 30 + 2.0 ** 26),
        ('overflow', -_BIG, _BIG),                       # delta = +inf from finite extrema: scale inf, zp +0, y NaN
    ],
    (4, True): _COMMON + [
        ('neg_under_positive', -7.25, -0.125),           # delta < 0: the floor
        ('floor_below', 0.0, _D_BELOW),
        ('floor_at', 0.0, _D_AT),
        ('floor_above', 0.0, _D_ABOVE),
        ('scale_at_2p30', -3.0, 15 * 2.0 ** 30),
        ('scale_above_2p30', -3.0, 15 * 2.0 ** 30 + 2.0 ** 26),
        ('big_under_positive', -_BIG, _BIG),             # delta = mx here: finite, far outside the fast domain
    ],
    # 2^70 as an extremum of a channel that is not constant: the next float down is 2^46 away, so scale <= 2^30 needs qmax 2^32
    (32, False): [
        ('wide', -1024.0, 3072.0),
        ('wide_pos', 16.0, 4096.0),
        ('const_2p70', 2.0 ** 70, 2.0 ** 70),
        ('abs_at_2p70', 2.0 ** 70 - 2.0 ** 50, 2.0 ** 70),
        ('abs_above_2p70', 2.0 ** 70 - 2.0 ** 50, 2.0 ** 70 + 2.0 ** 47),
        ('neg_abs_at_2p70', -(2.0 ** 70), -(2.0 ** 70) + 2.0 ** 50),
        ('neg_abs_above_2p70', -(2.0 ** 70) - 2.0 ** 47, -(2.0 ** 70) + 2.0 ** 50),
        ('pinf', -1.0, _INF),
        ('nan', _NAN, _NAN),
    ],
}
MODES = sorted(TABLES)
DTYPES = {'f32': torch.float32, 'bf16': torch.bfloat16, 'f16': torch.float16}


def _exact_in(v, dtype):
    t = torch.tensor([float(v)], dtype=torch.float32)
    back = t.to(dtype).to(torch.float32)
    return bool(torch.isnan(t).all()) or bool((back == t).all())


def table(mode, dtype=torch.float32):
    """[(name, mn, mx)] of a mode (num_bits, positive): the whole table in float32, the sub-table whose extrema are exact in bf16 /
    fp16 otherwise."""
    rows = [(n, F32(a), F32(b)) for n, a, b in TABLES[mode]]
    for _, a, b in TABLES[mode]:
        assert all(v != v or float(F32(v)) == float(v) for v in (a, b)), 'exact in float32'
    return [r for r in rows if _exact_in(r[1], dtype) and _exact_in(r[2], dtype)]


def split(mode, dtype=torch.float32):
    """(fast table, slow table): a channel is fast when fast_domain_ref holds for it.  k_mmq_group and the resident kernel go slow
    for a whole workgroup as soon as one of its channels is outside the domain, so a border channel that shares a tensor with pinf
    never runs the divide-free path: the fast table runs alone, too."""
    rows = table(mode, dtype)
    mn, mx = (np.array([r[i] for r in rows], dtype=F32) for i in (1, 2))
    fast = fast_domain_ref(mn, mx, params_ref(mn, mx, mode[0], mode[1])[0])
    return [r for r, f in zip(rows, fast) if f], [r for r, f in zip(rows, fast) if not f]


def mixed(mode, dtype=torch.float32):
    """both tables, a slow channel behind every fast one as long as there are slow ones"""
    fast, slow = split(mode, dtype)
    out = []
    for i in range(max(len(fast), len(slow))):
        out += fast[i:i + 1] + slow[i:i + 1]
    return out


def windows(rows, C, skip=()):
    """The table cut into tensors of C channels: window k holds rows k*C ... wrapped around, so every row passes.  skip: names a
    one-channel window need not repeat."""
    n = -(-len(rows) // C)
    out = []
    for k in range(n):
        w = [rows[(k * C + i) % len(rows)] for i in range(C)]
        if C == 1 and w[0][0] in skip:
            continue
        out.append(w)
    return out


def all_named():
    """every named channel of every mode once, for the parameter kernel alone: [(name, mn, mx)]"""
    seen, out = set(), []
    for mode in MODES:
        for n, a, b in table(mode):
            key = (a.tobytes(), b.tobytes())
            if key not in seen:
                seen.add(key)
                out.append(('%s@%d%s' % (n, mode[0], 'p' if mode[1] else ''), a, b))
    return out


# ------------------------------------------------------------------------------------------ the tensor builder
def _inside(lo, hi, dtype):
    """the smallest value above lo and the largest below hi that dtype holds (as float32)"""
    if dtype == torch.float32:
        return np.nextafter(lo, F32(np.inf)), np.nextafter(hi, F32(-np.inf))
    if dtype == torch.float16:
        return (F32(np.nextafter(np.float16(lo), np.float16(np.inf))), F32(np.nextafter(np.float16(hi), np.float16(-np.inf))))
    def step(v, up):                                     # bfloat16: the upper half of the float32 word, sign and magnitude
        if v == 0:
            return F32(2.0 ** -133) if up else F32(-(2.0 ** -133))
        word = int(np.array([v], dtype=F32).view(np.uint32)[0])
        word += 0x10000 if up == (v > 0) else -0x10000
        return np.array([word], dtype=np.uint32).view(F32)[0]
    return step(lo, True), step(hi, False)


def positions(N, HW):
    """The six places (n, hw) an extremum rotates over: the first element of the channel; the last element of the last sample; the
    last element of the first sample; the first element of the last sample; the last column of a middle row (a row that is not a
    whole number of float4 ends in a straddling one); the element just before the first 256-float4 tile boundary of the channel's
    flattened (n, hw) population (its middle when it is shorter)."""
    f = 1023 if N * HW > 1024 else max(N * HW // 2 - 1, 0)
    return [(0, 0), (N - 1, HW - 1), (0, HW - 1), (N - 1, 0), (N // 2, HW - 1), (f // HW, f % HW)]


def place(shape, c):
    """((n, hw) of the minimum, (n, hw) of the maximum) of channel c: rotating, never the same element, and never the same float4
    of memory where the channel has more than one."""
    N, C, H, W = shape
    HW = H * W
    pos = positions(N, HW)
    addr = lambda p: (p[0] * C + c) * HW + p[1]          # noqa: E731
    a = pos[c % 6]
    rest = [pos[(c + 3 + k) % 6] for k in range(6)]
    for want_other_f4 in (True, False):                  # (a channel of four elements in one float4 has no other float4)
        for b in rest + [(n, hw) for n in range(min(N, 2)) for hw in range(min(HW, 8))]:
            if b != a and (not want_other_f4 or addr(b) // 4 != addr(a) // 4):
                return a, b
    raise AssertionError('a channel of one element has no room for two extrema')


def tensor_with_extrema(shape, mn, mx, seed, dtype=torch.float32):
    """x [N, C, H, W] (CPU, contiguous, dtype) whose channel c has minimum mn[c] at exactly one element and maximum mx[c] at exactly
    one, at place(shape, c); everything else lies strictly inside (mn, mx): drawn in float64, rounded to dtype, then clipped.  A
    constant channel is all one value; a NaN channel holds one NaN (at the minimum's place) in a fill of (-1, 1); an infinite
    extremum stands alone among finite values."""
    N, C, H, W = shape
    HW = H * W
    assert len(mn) == C and len(mx) == C
    rng = np.random.default_rng(seed)
    x = np.empty((N, C, HW), dtype=F32)
    for c in range(C):
        a, b = F32(mn[c]), F32(mx[c])
        pa, pb = place(shape, c)
        if a != a:
            lo, hi = F32(-1), F32(1)
        else:
            lo = a if np.isfinite(a) else F32(-1000)
            hi = b if np.isfinite(b) else F32(1000)
        if lo == hi:
            x[:, c] = lo
            continue
        u = rng.uniform(0.05, 0.95, size=(N, HW))
        fill = np.float64(lo) + (np.float64(hi) - np.float64(lo)) * u
        fill = torch.from_numpy(fill).to(torch.float32).to(dtype).to(torch.float32).numpy()
        inlo, inhi = _inside(lo, hi, dtype)
        assert lo < inlo <= inhi < hi, (lo, hi, dtype)
        x[:, c] = np.clip(fill, inlo, inhi)
        x[pa[0], c, pa[1]] = a
        if a == a:
            x[pb[0], c, pb[1]] = b
    t = torch.from_numpy(x.reshape(N, C, H, W)).to(dtype)
    assert dtype == torch.float32 or same_bits(t.to(torch.float32).numpy(), x.reshape(N, C, H, W))
    return t


def window_tensor(shape, rows, seed, dtype=torch.float32):
    """the builder on a window of the table: (x, mn [C], mx [C])"""
    mn = np.array([r[1] for r in rows], dtype=F32)
    mx = np.array([r[2] for r in rows], dtype=F32)
    return tensor_with_extrema(shape, mn, mx, seed, dtype), mn, mx


# ------------------------------------------------------------------------------------------ mutants of params_ref
def _round_half_away(v):
    with np.errstate(all='ignore'):
        return (np.sign(v) * np.floor(np.abs(v) + F32(0.5))).astype(F32)


def params_mutant(kind, mn, mx, num_bits, positive):
    """params_ref with one slip a hand-written copy could hold -> (scale, zp, qmax)"""
    mn = np.asarray(mn, dtype=F32)
    mx = np.asarray(mx, dtype=F32)
    with np.errstate(all='ignore'):
        qmax = qmax_ref(num_bits)
        if kind == 'qmax_powf':
            qmax = F32(F32(F32(2.0) ** F32(num_bits)) - F32(1))     # 2^b is exact: 2^b - 1 rounds the same way in one step or two
        if kind == 'qmax_int32':
            qmax = F32(np.array([(1 << num_bits) & 0xFFFFFFFF], dtype=np.uint32).view(np.int32)[0] - 1)   # (1 << bits) - 1 in an int
        offset = np.zeros_like(mn) if positive else mn
        if kind == 'offset_mn_under_positive':
            offset = mn
        delta = mx - offset
        if kind == 'delta_mx_minus_mn_under_positive':
            delta = mx - mn
        scale = delta / qmax
        if kind == 'floor_drops_nan':
            scale = np.fmax(scale, FLOOR)
        elif kind == 'floor_le':
            scale = np.where(scale <= FLOOR, FLOOR, scale)       # the kernels' select, `<=` for `<`: NaN passes it as well
        else:
            scale = np.maximum(scale, FLOOR)
        q = offset / scale
        zp = np.rint(-q) if kind == 'rint_of_minus_q' else np.rint(F32(0) - q)
        if kind == 'round_half_away':
            zp = _round_half_away(F32(0) - q)
    return scale.astype(F32), zp.astype(F32), qmax


def fast_domain_mutant(kind, mn, mx, scale, num_bits, positive):
    mn, mx, scale = (np.asarray(v, dtype=F32) for v in (mn, mx, scale))
    with np.errstate(all='ignore'):
        if kind == 'domain_on_delta':
            delta = mx - (np.zeros_like(mn) if positive else mn)
            return (np.abs(mn) <= P70) & (np.abs(mx) <= P70) & (delta <= P30)
        if kind == 'domain_lt':
            return (np.abs(mn) < P70) & (np.abs(mx) < P70) & (scale < P30)
    raise KeyError(kind)


PARAM_MUTANTS = ['round_half_away', 'floor_drops_nan', 'floor_le', 'rint_of_minus_q', 'qmax_powf', 'qmax_int32', 'offset_mn_under_positive',
                 'delta_mx_minus_mn_under_positive']
# the same bits as params_ref for every input (asserted in test_minmax_params_cpu.py): no test can, or need, catch them
EQUIVALENT_MUTANTS = ['floor_le', 'qmax_powf']
DOMAIN_MUTANTS = ['domain_on_delta', 'domain_lt']
