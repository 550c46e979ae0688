"""CPU-only checks of the flat-row statistics: the three entry points exist and their ctypes prototypes
match the header, bad arguments are refused before anything touches the device, the workspace covers the documented records,
the route function over a grid of (rows, len, dtype, alignment), the per-tensor manager's routing predicate as a truth table -
and that a numpy emulation of the fp32 four-value partial sums keeps the tiers of tests/test_tensor_stats_gpu.py on that file's
inputs (were it not so, the inputs would be wrong, not the tiers).  The GPU file imports its inputs and shapes from here."""
import ctypes
import math

import numpy as np
import pytest
import torch

from test_channels_last_collect_cpu import BAD, EINVAL, ERANGE, ctype_of, header_decls, lib

FUNCS = ['cnnq_rows_stats_workspace', 'cnnq_rows_stats_route', 'cnnq_rows_stats']
NMOM, NDEV, TPB = 7, 2, 256
ELEMS, MAX_WGS, PMM_MAX, EXACT = 65536, 2048, 1 << 19, 4096
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
IDS = ['f32', 'bf16', 'f16']

# ---- the inputs and shapes of the GPU file
# Row lengths at the ends of the lane walk: 256 * W * k +- 1 and +- W for the 16-byte widths (W = 4 elements of fp32, 8 of bf16 /
# fp16) and k = 8 / 4 (8192: whole steps of four pieces per lane) and 10 / 5 (10240: half a step left over)
WALK = sorted({b + d for b in (8192, 10240) for d in (0, -1, 1, -4, 4, -8, 8)})
# (rows, len): 1, 7, 8; the regime border on both sides; several chunks and an uneven last one; odd lengths (one element per load)
# with one and with two chunks inside every row; many short rows
SHAPES = [(1, 1), (1, 7), (1, 8), (1, 4096), (1, 4100), (3, 4096), (3, 4100)] + [(1, n) for n in WALK] \
    + [(1, 3 * 65536 + 24), (1, 3 * 65536 + 40), (5, 70001), (3, 140001), (300, 50)]
LARGEST = (1, 1 << 23)            # 128 chunks of 65536 elements


def values(rows, length, seed=0):
    """[rows, length] float32: per row Laplace-distributed values of scale 0.2 .. 3.2 around a mean within +-3, so the
    conditioning k = 1 + mean^2 / var stays below 1 + 9 / 0.08 = 114 (DESIGN.md section 12 assumes k <= 300)."""
    g = torch.Generator().manual_seed(1000 * rows + length % 1000 + seed)
    u = torch.rand((rows, length), generator=g, dtype=torch.float64) - 0.5
    lap = -torch.sign(u) * torch.log1p(-2 * u.abs().clamp(max=0.5 - 1e-12))
    scale = 0.2 + 3 * torch.rand((rows, 1), generator=g, dtype=torch.float64)
    mean = torch.randn((rows, 1), generator=g, dtype=torch.float64).clamp(-3, 3)
    return (lap * scale + mean).float()


def ref64(t):
    """The seven rows of t [rows, len] (fp32 values) in fp64, [7, rows], and mean |x|: B and the kurtosis around the fp32-rounded
    mean and std (the reference of tests/test_channels_last_collect_gpu.py); min / max with torch's NaN rule."""
    t = t.double()
    rows = t.shape[0]
    if t.shape[1] == 1:                 # no standard deviation: NaN rows, written out (torch.std warns about 0 degrees of freedom)
        nan = torch.full((rows,), float('nan'), dtype=torch.float64)
        return torch.stack([t[:, 0], t[:, 0], t[:, 0], nan, torch.zeros(rows, dtype=torch.float64), nan, nan]), t.abs().mean(1)
    mean, std = t.mean(1), t.std(1, unbiased=True)
    out = torch.zeros(7, rows, dtype=torch.float64)
    nan = torch.isnan(t).any(1)
    nanv = torch.full((rows,), float('nan'), dtype=torch.float64)
    out[0] = torch.where(nan, nanv, t.min(1)[0])
    out[1] = torch.where(nan, nanv, t.max(1)[0])
    out[2], out[3] = mean, std
    m32, s32 = mean.float().double(), std.float().double()
    out[4] = (t - m32[:, None]).abs().mean(1)
    out[5] = (((t - m32[:, None]) / s32[:, None]) ** 4).mean(1) - 3
    out[6] = t.clamp(min=0).std(1, unbiased=True)
    return out, t.abs().mean(1)


def check_tiers(stats, count, sum_, sum_relu, ref, mean_abs, length, need_dev=True):
    """stats [7, rows] f32 and the moment rows against ref64's: the tiers of tests/test_channels_last_collect_gpu.py /
    tests/test_stats_single_gpu.py.  A row of one element has no standard deviation (0 / 0 on both sides)."""
    stats = stats.double()
    assert torch.equal(stats[0].float(), ref[0].float()) and torch.equal(stats[1].float(), ref[1].float())
    assert bool((count == length).all())
    np.testing.assert_allclose(stats[2], ref[2], rtol=2e-6, atol=1e-7)
    np.testing.assert_allclose((2. * sum_relu - sum_) / count, mean_abs, rtol=3e-6, atol=1e-7)
    if need_dev:
        np.testing.assert_allclose(stats[4], ref[4], rtol=3e-6, atol=1e-7)
    if length == 1:
        assert bool(torch.isnan(stats[3]).all())
        return
    live = ref[3] != 0
    np.testing.assert_allclose(stats[3][live], ref[3][live], rtol=2e-6)
    np.testing.assert_allclose(stats[6], ref[6], rtol=3e-6, atol=1e-7)
    if need_dev:
        np.testing.assert_allclose(stats[5][live], ref[5][live], rtol=2e-4, atol=2e-4)


# ---- the C ABI
def test_entry_points_exist_and_prototypes_match_header():
    from cnn_quantization_amd import _lib as L
    decls = header_decls()
    for name in FUNCS:
        assert hasattr(lib(), name), name
        ret, args = decls[name]
        res, argtypes = L.SIGNATURES[name]
        assert res is {'int': ctypes.c_int, 'size_t': ctypes.c_size_t}[ret], name
        assert len(args) == len(argtypes), name
        for a, t in zip(args, argtypes):
            want = ctype_of(a)
            if want == 'ptr':
                assert t is ctypes.c_void_p or issubclass(t, ctypes._Pointer), (name, a, t)
            else:
                assert t is want, (name, a, t)


def stats_args(dtype=0, rows=4, length=8):
    p = ctypes.c_void_p(BAD)
    return [p, dtype, rows, length, 1, p, p, p, None]                # x, dtype, rows, len, need_dev, ws, mom, stats, stream


@pytest.mark.parametrize('dtype, rows, length', [(-1, 4, 8), (3, 4, 8), (1 << 20, 4, 8), (0, 0, 8), (1, 4, 0), (2, -3, 8), (0, 4, -1)])
def test_bad_geometry_is_einval(dtype, rows, length):
    out = (ctypes.c_int32 * 4)()
    assert lib().cnnq_rows_stats_workspace(rows, length, dtype) == 0
    assert lib().cnnq_rows_stats_route(rows, length, dtype, 16, out) == EINVAL
    assert lib().cnnq_rows_stats(*stats_args(dtype, rows, length)) == EINVAL


@pytest.mark.parametrize('dtype', [0, 1, 2])
def test_bad_pointers_are_einval_and_huge_shapes_erange(dtype):
    for i in (0, 5, 7):                                     # x, ws, stats
        a = stats_args(dtype)
        a[i] = None
        assert lib().cnnq_rows_stats(*a) == EINVAL, i
    for i in (5, 6):                                        # ws and mom hold doubles
        a = stats_args(dtype)
        a[i] = ctypes.c_void_p(BAD + 4)
        assert lib().cnnq_rows_stats(*a) == EINVAL, i
    a = stats_args(dtype)
    a[0] = ctypes.c_void_p(BAD + (2 if dtype == 0 else 1))  # x is not aligned to its element size
    assert lib().cnnq_rows_stats(*a) == EINVAL
    a[6] = None                                             # mom may be NULL: the misaligned x still refuses
    assert lib().cnnq_rows_stats(*a) == EINVAL
    out = (ctypes.c_int32 * 4)()
    esize = 4 if dtype == 0 else 2
    assert lib().cnnq_rows_stats_route(4, 8, dtype, 3, out) == EINVAL
    assert lib().cnnq_rows_stats_route(4, 8, dtype, 0, out) == EINVAL
    assert lib().cnnq_rows_stats_route(4, 8, dtype, esize // 2, out) == EINVAL
    assert lib().cnnq_rows_stats_route(4, 8, dtype, 16, None) == EINVAL
    # 2^31 rows (the merge kernels' column index), a chunk of 2^31 pieces (2048 rows leave one chunk per row), byte offsets past 63 bits
    for rows, length in ((1 << 31, 8), (2048, 1 << 50), (4, 1 << 60)):
        assert lib().cnnq_rows_stats_route(rows, length, dtype, 16, out) == ERANGE, (rows, length)
        assert lib().cnnq_rows_stats(*stats_args(dtype, rows, length)) == ERANGE, (rows, length)
    assert lib().cnnq_rows_stats_workspace(1 << 31, 8, dtype) == 0
    # a long row as such is fine: 2^40 elements in 2048 chunks of 2^29 elements
    assert lib().cnnq_rows_stats_route(1, 1 << 40, dtype, 16, out) == 0 and out[1] == 2048


def widths(length, esize, align=16):
    return [w for w in (8, 4, 2) if w * esize <= 16 and length % w == 0 and align % (w * esize) == 0] + [1]


def geo(rows, length, w):
    """The geometry of csrc/cnnq_rows.hip.h (rows_geo), restated: (chunks per row, pieces per chunk)."""
    P = length // w
    s = max(1, min(P // -(-ELEMS // w), MAX_WGS // rows))
    ppc = -(-P // s)
    return -(-P // ppc), ppc


@pytest.mark.parametrize('dtype', [0, 1, 2])
@pytest.mark.parametrize('align', [2, 4, 8, 16])
def test_route_and_workspace_over_a_grid(dtype, align):
    esize = 4 if dtype == 0 else 2
    if align < esize:
        return
    out = (ctypes.c_int32 * 4)()
    lengths = [1, 2, 3, 7, 8, 50, 4095, 4096, 4097, 4100, 65535, 65536, 65537, 70001, 131072, 3 * 65536 + 24, 1 << 20, (1 << 23) + 6,
               512 * 64 * 112 * 112, 512 * 64 * 112 * 112 + 1, (1 << 33) + 8]
    for rows in (1, 2, 5, 32, 300, 512, 2048, 2049, 1 << 19):
        for length in lengths:
            if geo(rows, length, widths(length, esize, align)[0])[1] >= 1 << 31:     # out[2] would not hold the pieces per chunk
                assert lib().cnnq_rows_stats_route(rows, length, dtype, align, out) == ERANGE, (rows, length)
                continue
            assert lib().cnnq_rows_stats_route(rows, length, dtype, align, out) == 0, (rows, length)
            w, S, ppc, exact = out
            # the widest piece of at most 16 bytes that divides the row and the alignment: every row starts on a piece
            assert w == widths(length, esize, align)[0] and length % w == 0 and align % (w * esize) == 0, (rows, length, w)
            P = length // w
            assert (S, ppc) == geo(rows, length, w), (rows, length, S, ppc)
            assert (S - 1) * ppc < P <= S * ppc                     # the chunks cover every piece exactly once
            assert ppc * w >= min(ELEMS, length)                    # a full chunk is 65536 elements at least, or the row is shorter
            assert P - (S - 1) * ppc > ppc - S                      # and the last one is short of it by fewer than S pieces
            assert min(rows * S, MAX_WGS) <= MAX_WGS and (rows * S <= MAX_WGS or S == 1)
            assert S * rows <= PMM_MAX
            assert exact == (1 if length <= EXACT else 0)
            # ws, doubles: part[S][NMOM][rows], mom[NMOM][rows], part2[S][NDEV][rows] for the largest S over the piece widths
            smax = max(geo(rows, length, v)[0] for v in widths(length, esize))
            assert lib().cnnq_rows_stats_workspace(rows, length, dtype) == (smax * (NMOM + NDEV) + NMOM) * rows * 8, (rows, length)
    # the shapes of the GPU file take the width and the regime they were chosen for (alignment 16)
    if align == 16:
        for rows, length in SHAPES + [LARGEST]:
            assert lib().cnnq_rows_stats_route(rows, length, dtype, 16, out) == 0
            assert out[0] == widths(length, esize)[0] and out[3] == (length <= EXACT)
        assert lib().cnnq_rows_stats_route(5, 70001, dtype, 16, out) == 0 and list(out) == [1, 1, 70001, 0]
        assert lib().cnnq_rows_stats_route(3, 140001, dtype, 16, out) == 0 and list(out) == [1, 2, 70001, 0]
        assert lib().cnnq_rows_stats_route(1, 3 * 65536 + 24, dtype, 16, out) == 0 and (out[0], out[1]) == (16 // esize, 3)
        assert lib().cnnq_rows_stats_route(1, 1 << 23, dtype, 16, out) == 0 and (out[0], out[1]) == (16 // esize, 128)


# ---- the manager's predicate
class FakeManager:
    def __init__(self, kld_threshold=False, group=None):
        self.kld_threshold, self.group = kld_threshold, group


class OnGpu(torch.Tensor):
    """A CPU tensor that says it is a CUDA tensor: the predicate reads shape, strides, dtype and attributes only."""
    @property
    def is_cuda(self):
        return True


def gpu(t):
    return t.as_subclass(OnGpu)


def nhwc(dtype=torch.bfloat16, shape=(2, 8, 4, 4)):
    n, c, h, w = shape
    return torch.zeros(n * c * h * w, dtype=dtype).as_strided(shape, (h * w * c, 1, w * c, c))


def test_predicate_truth_table(monkeypatch):
    import os
    from cnn_quantization_amd import distributed as D, ops
    from cnn_quantization_amd.inference.statistic_manager import collects_native_flat as native
    for dtype in DTYPES:
        half = dtype != torch.float32
        assert native(FakeManager(), gpu(nhwc(dtype)))                                          # dense channels_last: all three
        assert native(FakeManager(), gpu(torch.zeros(2, 8, 4, 4, dtype=dtype))) == half         # contiguous: not float32
        assert native(FakeManager(), gpu(torch.zeros(8, 100, dtype=dtype))) == half
        assert native(FakeManager(), gpu(nhwc(dtype, (2, 8, 1, 1)))) == half                    # dense in both layouts: contiguous
        assert not native(FakeManager(), gpu(nhwc(dtype))[:, 2:5])                              # not dense
        assert not native(FakeManager(), gpu(torch.zeros(8, 100, dtype=dtype).t()))
        assert not native(FakeManager(), nhwc(dtype))                                           # a CPU tensor
        assert not native(FakeManager(), gpu(torch.zeros(0, 4, dtype=dtype)))                   # nothing to reduce
        # the KLD threshold has no half kernel
        assert native(FakeManager(kld_threshold=True), gpu(nhwc(dtype))) == (not half)
        assert not native(FakeManager(kld_threshold=True), gpu(torch.zeros(8, 100, dtype=dtype)))
    assert not native(FakeManager(), gpu(nhwc(torch.float64))) and not native(FakeManager(), None)
    x = gpu(nhwc())
    # more than one process, or the forced exchange
    monkeypatch.setattr(D, 'world_size', lambda group=None: 2)
    assert not native(FakeManager(), x)
    monkeypatch.undo()
    monkeypatch.setattr(D, 'forced_exchange', lambda: True)
    assert not native(FakeManager(), x)
    monkeypatch.undo()
    assert native(FakeManager(), x)
    # the A/B switch sends channels_last tensors back; a contiguous half tensor has no layout to keep
    old = os.environ.get('CNNQ_NHWC')
    try:
        os.environ['CNNQ_NHWC'] = '0'
        ops.reload_switches()
        assert not native(FakeManager(), x)
        assert native(FakeManager(), gpu(torch.zeros(8, 100, dtype=torch.float16)))
    finally:
        if old is None:
            os.environ.pop('CNNQ_NHWC', None)
        else:
            os.environ['CNNQ_NHWC'] = old
        ops.reload_switches()
    assert native(FakeManager(), x)


def test_ops_have_no_cpu_path():
    from cnn_quantization_amd import _lib as L, ops
    with pytest.raises(L.CnnqError):
        ops.tensor_stats(torch.zeros(8, 16))
    with pytest.raises(L.CnnqError):
        ops.tensor_stats(nhwc(torch.float32), 2)
    with pytest.raises(L.CnnqError):
        ops.row_sumsq(nhwc(torch.bfloat16))
    with pytest.raises(L.CnnqError):
        ops.kld_thresholds(nhwc(torch.float32))


# ---- the inputs of the GPU tests hold the tiers under an emulation of the kernels' two summation regimes
def fold4(v, exact):
    """Per-row sums of v [rows, len] (fp32): fp64 element by element, or four-value fp32 partials (v0 + v1) + (v2 + v3) folded into
    fp64 with the leftovers in fp64."""
    if exact:
        return v.astype(np.float64).sum(1)
    n = v.shape[1] // 4 * 4
    q = v[:, :n].reshape(v.shape[0], -1, 4)
    part = (q[:, :, 0] + q[:, :, 1]) + (q[:, :, 2] + q[:, :, 3])
    assert part.dtype == np.float32
    return part.astype(np.float64).sum(1) + v[:, n:].astype(np.float64).sum(1)


def table32(t):
    """The rows of t [rows, len] (fp32 values, numpy) as the kernels form them: fp32 per element, four-value fp32 partials above
    4096 elements, fp64 merges, fp32 rows; and the manager's mean_abs."""
    n = t.shape[1]
    exact = n <= EXACT
    sq = lambda a: (a.astype(np.float64) ** 2).sum(1) if exact else fold4(a * a, False)
    s, ss = fold4(t, exact), sq(t)
    mean64 = s / n
    mean = mean64.astype(np.float32)
    std = np.sqrt(np.maximum((ss - s * mean64) / (n - 1), 0)).astype(np.float32)
    r = np.maximum(t, np.float32(0))
    rs, rss = fold4(r, exact), sq(r)
    std_pos = np.sqrt(np.maximum((rss - rs * (rs / n)) / (n - 1), 0)).astype(np.float32)
    d = t - mean[:, None]
    b = (fold4(np.abs(d), exact) / n).astype(np.float32)
    z = d * (np.float32(1) / std)[:, None]
    z2 = z * z
    kurt = (fold4(z2 * z2, exact) / n - 3.).astype(np.float32)
    stats = np.stack([t.min(1), t.max(1), mean, std, b, kurt, std_pos])
    return torch.from_numpy(stats), torch.from_numpy(s), torch.from_numpy(rs)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_fp32_emulation_keeps_the_tiers_on_the_gpu_tests_inputs(dtype):
    for rows, length in [s for s in SHAPES if s[1] > 1] + [(4, 24 * 81), (1, 4 * 24 * 81), LARGEST]:
        t = values(rows, length).to(dtype).float()
        stats, s, rs = table32(t.numpy())
        ref, mean_abs = ref64(t)
        count = torch.full((rows,), float(length), dtype=torch.float64)
        check_tiers(stats, count, s, rs, ref, mean_abs, length)
    # the conditioning the derivation of the border assumes
    t = values(300, 50).double()
    assert float((1 + t.mean(1) ** 2 / t.var(1)).max()) <= 300 and math.isfinite(float(t.sum()))
