"""The uniform per-channel Q/DQ that counts its codes (-me) on dense channels_last activations, fp32 / bf16 /
fp16.  The references are this library's own NCHW kernels on x.contiguous().float():
  A. given a table qp, bit for bit (NaN == NaN): y equals cnnq_pc_qdq_nhwc's and pc_qdq's cast to x's dtype; the replica tables
     folded by cnnq_hist_replicas_fold equal, word for word, the histogram pc_qdq fills; every element is counted once; the
     replica tables are zero afterwards;
  B. config 2, dynamic: act_qdq_per_channel(x, bits, positive, want_entropy=True) returns y and an entropy bit-equal to the same
     call on x.contiguous().float() (the extrema are exact), with no layout copy;
  C. config 3 at ops level: with stats= as A and B; dynamic, the statistics table by check_table of
     tests/test_channels_last_aciq_gpu.py (MIN / MAX bit-equal, MEAN / STD / B within RTOL_STAT = 2e-6 and its floors) and
     everything behind it bit for bit given that table."""
import ctypes
import importlib

import pytest
import torch

import _quantizer as Q
from test_channels_last_aciq_gpu import check_table
from test_channels_last_gpu import DTYPES, IDS, cl, is_cl, same, values

pytestmark = pytest.mark.gpu


def mods():
    from cnn_quantization_amd import _lib as L, ops
    return L, ops


def same_scalar(a, b):
    return same(a.reshape(1).float(), b.reshape(1).float())


def geom(x):
    N, C, H, W = x.shape
    return N, C, H * W


def replicas():
    L, _ = mods()
    return torch.zeros(L.load().cnnq_hist_replica_bytes() // 8, dtype=torch.int64, device='cuda')


def fold(rep):
    """cnnq_hist_replicas_fold into a zeroed 256-word table; the replica tables are zero afterwards."""
    L, ops = mods()
    hist = torch.zeros(256, dtype=torch.int64, device='cuda')
    L.check(L.load().cnnq_hist_replicas_fold(ops._ptr(rep), ops._ptr(hist), ops._stream(rep)), 'cnnq_hist_replicas_fold')
    assert not rep.any()
    return hist


def nchw_ref(x, qp):
    """pc_qdq with the table on x.contiguous().float(): (y in x's dtype, the histogram it fills, its entropy)."""
    L, ops = mods()
    N, C, HW = geom(x)
    hist = torch.zeros(256, dtype=torch.int64, device='cuda')
    y = ops.pc_qdq(x.contiguous().float(), N, C, HW, qp, hist=hist)
    return y.to(x.dtype), hist, ops.entropy_from_hist(hist)


def table_pass(x, qp, nbins, out=None):
    """cnnq_pc_qdq_hist_nhwc through the C ABI on tables of the test's own: (y, the folded histogram)."""
    L, ops = mods()
    N, C, HW = geom(x)
    y = torch.empty_like(x) if out is None else out
    rep = replicas()
    L.check(L.load().cnnq_pc_qdq_hist_nhwc(ops._ptr(x), ops._ptr(y), ops._DTYPE_CODES[x.dtype], N * HW, C, ops._ptr(qp), nbins, ops._ptr(rep),
                                           ops._stream(x)), 'cnnq_pc_qdq_hist_nhwc')
    return y, fold(rep)


def check_a(x, qp, nbins, out=None):
    L, ops = mods()
    y, hist = table_pass(x, qp, nbins, out)
    assert is_cl(y) and y.dtype == x.dtype and y.shape == x.shape
    assert same(y, ops._pc_qdq_nhwc(x, qp, None)), (tuple(x.shape), x.dtype, nbins, x.storage_offset())
    y_ref, h_ref, _ = nchw_ref(x, qp)
    assert same(y, y_ref), (tuple(x.shape), x.dtype, nbins, x.storage_offset())
    assert torch.equal(hist, h_ref), (tuple(x.shape), x.dtype, nbins, hist.tolist(), h_ref.tolist())
    assert int(hist.sum()) == x.numel()
    return y, hist


def minmax_table(x, bits, positive):
    """config 2's parameter table of x, from the NCHW route."""
    L, ops = mods()
    _, parts = ops.act_qdq_per_channel(x.contiguous().float(), bits, positive=positive, want_parts=True)
    return parts['qp']


def check_b(x, bits, positive):
    L, ops = mods()
    before = ops.LAYOUT_COPIES
    y, ent = ops.act_qdq_per_channel(x, bits, positive=positive, want_entropy=True)
    y2, ent2 = ops.act_qdq_per_channel(x, bits, positive=positive, want_entropy=True)       # the tables are zero at rest
    assert ops.LAYOUT_COPIES == before
    assert is_cl(y) and y.dtype == x.dtype and y.shape == x.shape
    y_ref, e_ref = ops.act_qdq_per_channel(x.contiguous().float(), bits, positive=positive, want_entropy=True)
    assert same(y, y_ref.to(x.dtype)), (tuple(x.shape), x.dtype, bits, positive, x.storage_offset())
    assert same_scalar(ent, e_ref), (float(ent), float(e_ref), tuple(x.shape), x.dtype, bits, positive)
    assert same(y2, y) and same_scalar(ent2, ent)
    return y, ent


def route(x, nbins, align=None):
    L, ops = mods()
    out = (ctypes.c_int32 * 4)()
    C = x.shape[1]
    if align is None:
        align = (x.data_ptr() | 16) & -(x.data_ptr() | 16)             # y is a fresh allocation: x's alignment decides
    assert L.load().cnnq_pc_route_qdq_hist_nhwc(x.numel() // C, C, ops._DTYPE_CODES[x.dtype], align, nbins, out) == 0
    return list(out)


# (C, storage offset in elements, W in fp32, W in bf16 / fp16): every piece width, a second column block at W = 1 (P = 260 > 256),
# and RS = 1 (C = 256 W: no two lanes share a piece) next to many lanes per piece (C = 3)
WIDTH_CASES = [(3, 0, 1, 1), (5, 0, 1, 1), (6, 0, 2, 2), (12, 0, 4, 4), (24, 0, 4, 8), (260, 1, 1, 1), (1024, 0, 4, 8), (2048, 0, 4, 8)]


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('case', WIDTH_CASES, ids=lambda c: 'C%d+%d' % c[:2])
def test_every_piece_width(case, dtype):
    C, offset, w32, w16 = case
    want = w32 if dtype == torch.float32 else w16
    shape = (3, C, 7, 7) if C < 1024 else (2, C, 3, 3)                  # R = 147: not a multiple of RS
    for bits, positive in ((4, True), (2, False), (8, False)):
        x = cl(values(shape, seed=C + bits, positive=positive), dtype, offset)
        r = route(x, 1 << bits)
        assert r[0] == want and r[2] == (1 << bits) * 32 * 4 and r[3] == 1, (shape, dtype, offset, r, want)
        check_a(x, minmax_table(x, bits, positive), 1 << bits)
        check_b(x, bits, positive)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_ragged_rows_slabs_and_a_table_that_clips(dtype):
    L, ops = mods()
    # (3, 5, 7, 7): R = 147 rows at RS = 51; (4, 20, 32, 32): 81920 elements, two slabs of the counting launch
    for shape, offset, wgs in (((3, 5, 7, 7), 3, 1), ((4, 20, 32, 32), 0, 2), ((1, 2, 1, 2), 1, 1)):
        for bits, positive in ((4, True), (4, False), (8, True)):
            x = cl(values(shape, seed=bits + offset, positive=positive), dtype, offset)
            assert route(x, 1 << bits)[1] == wgs
            qp = minmax_table(x, bits, positive)
            check_a(x, qp, 1 << bits)
            # a calibration table does not bound the values: both clamps are taken; and more bins than the codes need
            qp2 = qp.clone()
            qp2[L.QP_SCALE] *= 0.6
            check_a(x, qp2, 1 << bits)
            check_a(x, qp2, 256)
            check_b(x, bits, positive)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_special_values_and_a_constant_channel(dtype):
    L, ops = mods()
    x = values((4, 16, 7, 7), seed=9)
    x[1, 0, 2, 3] = float('nan')
    x[0, 1, 0, 0] = float('inf')
    x[2, 2, 1, 1] = float('-inf')
    x[:, 5] = 1.25                                                      # a constant channel
    x[:, 6] = 0.0
    xc = cl(x, dtype, 1)
    for bits, positive in ((4, False), (4, True), (2, False), (8, True)):
        check_b(xc, bits, positive)
        qp = minmax_table(xc, bits, positive)                           # NaN / inf parameters in channels 0, 1, 2
        check_a(xc, qp, 1 << bits)
        # finite parameters under the special values: NaN counts in bin 0, +inf in qmax's, -inf in bin 0
        qp2 = qp.clone()
        qp2[:, :3] = qp[:, 3:4]
        _, hist = check_a(xc, qp2, 1 << bits)
        assert int(hist[(1 << bits):].sum()) == 0


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_bit_allocated_table_takes_256_bins(dtype):
    """Bit allocation gives the channels of one piece different qmax: the host cannot know them, so the pass keeps 256 bins."""
    L, ops = mods()
    for shape, offset in (((4, 24, 14, 14), 0), ((3, 10, 7, 7), 1)):
        x = cl(values(shape, seed=13, positive=True), dtype, offset)
        N, C, HW = geom(x)
        stats, _ = ops.pc_stats(x.contiguous().float(), N, C, HW, need_b=True)
        qp, diag = ops.pc_params(stats, 4, True, 'laplace', True, False, None, True)
        assert len(set(qp[L.QP_QMAX].tolist())) > 1
        check_a(x, qp, 256)


def test_replica_index_wraps_beyond_64_workgroups():
    """(8, 64, 96, 96): 4.7 M elements, 72 counting workgroups on 64 replica tables."""
    L, ops = mods()
    g = torch.Generator(device='cuda').manual_seed(5)
    shape = (8, 64, 96, 96)
    x = torch.empty(shape, dtype=torch.bfloat16, device='cuda', memory_format=torch.channels_last)
    x.copy_((torch.randn(shape, generator=g, device='cuda') * (0.2 + 3 * torch.rand(1, 64, 1, 1, generator=g, device='cuda'))).relu())
    assert route(x, 16)[1] > 64
    check_a(x, minmax_table(x, 4, True), 16)
    check_b(x, 4, True)


@pytest.mark.parametrize('dtype', [torch.float32, torch.bfloat16], ids=['f32', 'bf16'])
def test_out_at_another_alignment_narrows_the_piece(dtype):
    """A 16-byte aligned x with C % 8 == 0 and an `out` one element (then two) further into its storage: the piece width follows
    the alignment BOTH pointers share."""
    L, ops = mods()
    shape = (4, 64, 14, 14)
    n, c, h, w = shape
    x = cl(values(shape, seed=31, positive=True), dtype, 0)
    es = x.element_size()
    base = torch.zeros(x.numel() + 64, dtype=dtype, device='cuda')
    assert x.data_ptr() % 16 == 0 and base.data_ptr() % 16 == 0
    qp = minmax_table(x, 4, True)
    y0, h0 = check_a(x, qp, 16)
    for shift, want in ((1, 1), (2, 2)):
        base.zero_()
        out = base.as_strided(x.shape, (h * w * c, 1, w * c, c), shift)
        assert route(x, 16, 16)[0] == 16 // es and route(x, 16, shift * es)[0] == want
        y, hist = check_a(x, qp, 16, out=out)
        assert y is out and same(y, y0) and torch.equal(hist, h0)
        assert not base[:shift].any() and not base[x.numel() + shift:].any()       # nothing stored outside out
        before = ops.LAYOUT_COPIES
        y2, ent = ops.act_qdq_per_channel(x, 4, positive=True, want_entropy=True, out=out)
        assert y2 is out and same(y2, y0) and ops.LAYOUT_COPIES == before
        assert same_scalar(ent, nchw_ref(x, qp)[2])


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_dynamic_entry_points_through_the_c_abi(dtype):
    """cnnq_pc_minmax_qdq_hist_nhwc and cnnq_pc_aciq_qdq_hist_nhwc on buffers of the test's own: the tables they leave, y and the
    histogram word for word given those tables."""
    L, ops = mods()
    lib = L.load()
    for shape, offset, bits, positive in (((3, 12, 7, 7), 0, 4, True), ((4, 20, 32, 32), 1, 8, False), ((2, 6, 5, 5), 2, 2, False)):
        x = cl(values(shape, seed=17 + bits, positive=positive), dtype, offset)
        N, C, HW = geom(x)
        R, dt, st = N * HW, ops._DTYPE_CODES[dtype], ops._stream(x)
        y, rep = torch.empty_like(x), replicas()
        ws = torch.zeros(lib.cnnq_pc_nhwc_workspace(R, C, dt) // 4, dtype=torch.float32, device='cuda')
        qp = torch.empty((L.NQP, C), dtype=torch.float32, device='cuda')
        mm = torch.empty((2, C), dtype=torch.float32, device='cuda')
        L.check(lib.cnnq_pc_minmax_qdq_hist_nhwc(ops._ptr(x), ops._ptr(y), dt, R, C, bits, int(positive), ops._ptr(ws), ops._ptr(qp), ops._ptr(mm),
                                                 ops._ptr(rep), st), 'cnnq_pc_minmax_qdq_hist_nhwc')
        xf = x.contiguous().float()
        assert same(mm[0], xf.amin(dim=(0, 2, 3))) and same(mm[1], xf.amax(dim=(0, 2, 3)))
        assert same(qp, minmax_table(x, bits, positive))
        y_ref, h_ref, _ = nchw_ref(x, qp)
        assert is_cl(y) and same(y, y_ref) and torch.equal(fold(rep), h_ref)
        if bits > 4:
            continue
        for clip, ba in (('laplace', False), ('gaus', True)):
            cfg = ops._params_cfg(bits, positive, clip, ba, False, None, True, False)
            ws3 = torch.zeros(lib.cnnq_pc_aciq_nhwc_workspace(R, C, dt) // 8, dtype=torch.float64, device='cuda')
            tabs = torch.empty(L.NSTAT + L.NQP + L.NDIAG, C, dtype=torch.float32, device='cuda')
            stats, qp3, diag = tabs[:L.NSTAT], tabs[L.NSTAT:L.NSTAT + L.NQP], tabs[L.NSTAT + L.NQP:]
            L.check(lib.cnnq_pc_aciq_qdq_hist_nhwc(ops._ptr(x), ops._ptr(y), dt, R, C, ctypes.byref(cfg), ops._ptr(ws3), ops._ptr(stats),
                                                   ops._ptr(qp3), ops._ptr(diag), ops._ptr(rep), st), 'cnnq_pc_aciq_qdq_hist_nhwc')
            check_table(x, stats, clip == 'laplace')
            qp_ref, diag_ref = ops.pc_params(stats.contiguous(), bits, positive, clip, ba, False, None, True)
            assert same(qp3.contiguous(), qp_ref) and same(diag.contiguous(), diag_ref)
            y_ref, h_ref, _ = nchw_ref(x, qp_ref)
            hist = fold(rep)
            assert same(y, y_ref) and torch.equal(hist, h_ref) and int(hist.sum()) == x.numel()


def aciq(x, bits, **kw):
    L, ops = mods()
    return ops.aciq_qdq_nhwc(x, bits, **kw)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_config_3_at_ops_level(dtype):
    L, ops = mods()
    for shape, offset in (((8, 24, 14, 14), 0), ((3, 5, 7, 7), 1), ((4, 20, 32, 32), 3)):
        for bits, positive, clip, ba in ((4, True, 'laplace', False), (4, False, 'gaus', True), (3, True, 'laplace', True), (8, False, 'gaus', False)):
            x = cl(values(shape, seed=bits + offset, positive=positive), dtype, offset)
            N, C, HW = geom(x)
            xf = x.contiguous().float()
            # dynamic: the table within its tier, everything behind it bit for bit
            before = ops.LAYOUT_COPIES
            y, ent, parts = aciq(x, bits, positive=positive, clip=clip, bit_alloc=ba, want_entropy=True, want_parts=True)
            assert ops.LAYOUT_COPIES == before and is_cl(y) and y.dtype == dtype
            use_ba = ba and bits <= 4
            check_table(x, parts['stats'], clip == 'laplace')
            qp_ref, diag_ref = ops.pc_params(parts['stats'].contiguous(), bits, positive, clip, use_ba, False, None, True)
            assert same(parts['qp'].contiguous(), qp_ref) and same(parts['diag'].contiguous(), diag_ref)
            y_ref, _, e_ref = nchw_ref(x, qp_ref)
            assert same(y, y_ref) and same_scalar(ent, e_ref)
            y2, ent2 = aciq(x, bits, positive=positive, clip=clip, bit_alloc=ba, want_entropy=True)     # the hot form, the tables at rest
            assert same(y2, y) and same_scalar(ent2, ent)
            assert same(aciq(x, bits, positive=positive, clip=clip, bit_alloc=ba), y)                   # and without the counting
            # with stats=: against today's route on the NCHW tensor
            table = parts['stats'].contiguous().clone()
            table[L.STAT_STD] *= 1.1
            table[L.STAT_B] = (xf - table[L.STAT_MEAN].view(1, C, 1, 1)).abs().mean(dim=(0, 2, 3)) * 0.9
            before = ops.LAYOUT_COPIES
            ys, es = aciq(x, bits, positive=positive, clip=clip, bit_alloc=ba, stats=table, want_entropy=True)
            assert ops.LAYOUT_COPIES == before and is_cl(ys) and ys.dtype == dtype
            yr, er = ops.act_qdq_per_channel(xf, bits, positive=positive, clip=clip, bit_alloc=ba, stats=table, want_entropy=True, group=False)
            assert same(ys, yr.to(dtype)) and same_scalar(es, er)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_config_2_with_a_statistics_table(dtype):
    L, ops = mods()
    for shape, offset, bits, positive in (((8, 24, 14, 14), 0, 4, True), ((4, 7, 7, 7), 1, 2, False), ((2, 64, 28, 28), 3, 8, False)):
        x = cl(values(shape, seed=11, positive=positive), dtype, offset)
        xf = x.contiguous().float()
        table = torch.zeros((L.NSTAT, shape[1]), dtype=torch.float32, device='cuda')
        table[L.STAT_MIN] = xf.amin(dim=(0, 2, 3)) * 0.8
        table[L.STAT_MAX] = xf.amax(dim=(0, 2, 3)) * 0.9
        before = ops.LAYOUT_COPIES
        y, ent = ops.act_qdq_per_channel(x, bits, positive=positive, stats=table, want_entropy=True)
        assert ops.LAYOUT_COPIES == before and is_cl(y) and y.dtype == dtype
        y_ref, e_ref = ops.act_qdq_per_channel(xf, bits, positive=positive, stats=table, want_entropy=True)
        assert same(y, y_ref.to(dtype)) and same_scalar(ent, e_ref)
        qp, _ = ops.pc_params(table, bits, positive, 'no', False, False, None, True)
        check_a(x, qp, 1 << bits)


def test_inside_an_entropy_batch():
    """Two channels_last tensors and one NCHW tensor in one block: all three results are filled by the one launch at its end."""
    L, ops = mods()
    a = cl(values((8, 32, 14, 14), seed=1, positive=True), torch.bfloat16)
    b = cl(values((4, 20, 7, 7), seed=2), torch.float32, 1)
    c = values((4, 16, 14, 14), seed=3).cuda()
    ya, ea = ops.act_qdq_per_channel(a, 4, positive=True, want_entropy=True)
    yb, eb = aciq(b, 3, want_entropy=True)
    yc, ec = ops.act_qdq_per_channel(c, 4, want_entropy=True)
    copies = ops.LAYOUT_COPIES
    with ops.entropy_batch() as block:
        ya2, ea2 = ops.act_qdq_per_channel(a, 4, positive=True, want_entropy=True)
        yb2, eb2 = aciq(b, 3, want_entropy=True)
        yc2, ec2 = ops.act_qdq_per_channel(c, 4, want_entropy=True)
        assert block.n >= 2                                             # nothing launched yet: they wait for the block's end
    assert ops.LAYOUT_COPIES == copies
    assert same(ya2, ya) and same(yb2, yb) and same(yc2, yc)
    assert same_scalar(ea2, ea) and same_scalar(eb2, eb) and same_scalar(ec2, ec)
    assert 0 < float(ea) <= 4 and 0 < float(eb) <= 3
    assert not ops._ENT_TABLES[(a.device.index, ops._raw_stream(a.device.index))].any()


def test_graph_capture_replays_eager():
    """After one eager call on the capturing stream (the replica tables are zero-filled once, outside a capture) the counting
    route is captured; the replay on refreshed input gives the eager result."""
    L, ops = mods()
    shape = (16, 64, 14, 14)
    x = cl(values(shape, seed=2, positive=True), torch.bfloat16)
    eager, e_eager = ops.act_qdq_per_channel(x, 4, positive=True, want_entropy=True)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.act_qdq_per_channel(x, 4, positive=True, want_entropy=True)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    copies = ops.LAYOUT_COPIES
    with torch.cuda.graph(graph, stream=s):
        y, ent = ops.act_qdq_per_channel(x, 4, positive=True, want_entropy=True)
    assert ops.LAYOUT_COPIES == copies
    x.copy_(cl(values(shape, seed=3, positive=True), torch.bfloat16))
    graph.replay()
    torch.cuda.synchronize()
    y_now, e_now = ops.act_qdq_per_channel(x, 4, positive=True, want_entropy=True)
    assert is_cl(y) and same(y, y_now) and same_scalar(ent, e_now)
    assert not same(y, eager)


def test_ab_switch_codes_and_parts_take_the_counted_copy(monkeypatch):
    L, ops = mods()
    x = cl(values((4, 16, 14, 14), seed=4, positive=True), torch.float32)
    y_ref, e_ref = ops.act_qdq_per_channel(x.contiguous(), 4, positive=True, want_entropy=True)
    monkeypatch.setenv('CNNQ_NHWC', '0')
    ops.reload_switches()
    try:
        before = ops.LAYOUT_COPIES
        y, ent = ops.act_qdq_per_channel(x, 4, positive=True, want_entropy=True)
        assert ops.LAYOUT_COPIES == before + 1 and y.is_contiguous()
        assert same(y, y_ref) and same_scalar(ent, e_ref)
        y3, e3 = aciq(x, 4, positive=True, want_entropy=True)
        assert ops.LAYOUT_COPIES == before + 2 and y3.is_contiguous()
    finally:
        monkeypatch.delenv('CNNQ_NHWC')
        ops.reload_switches()
    # want_codes / want_parts stay excluded
    before = ops.LAYOUT_COPIES
    y, codes = ops.act_qdq_per_channel(x, 4, positive=True, want_codes=True)
    assert ops.LAYOUT_COPIES == before + 1 and y.is_contiguous()
    y, parts = ops.act_qdq_per_channel(x, 4, positive=True, want_parts=True)
    assert ops.LAYOUT_COPIES == before + 2 and y.is_contiguous()


class Logger:
    def __init__(self):
        self.rows = []

    def log_metric(self, name, value, step=None, meterId=None, weight=None):
        self.rows.append((name, value, meterId, weight))


def quantizer(**kw):
    return Q.quantizer(**dict(dict(pcq_act=True, measure_entropy=True), **kw))


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float32], ids=['bf16', 'f32'])
def test_through_the_quantizer(dtype):
    """IntQuantizer(4, clipping='no', pcq_act, no bit allocation, measure_entropy) on a channels_last activation: quantized where it
    lies, dynamic and with a stat_id."""
    L, ops = mods()
    iq = importlib.import_module('cnn_quantization_amd.qtypes.int_quantizer')
    x = cl(values((8, 32, 14, 14), seed=6), dtype, 0 if dtype == torch.bfloat16 else 1)
    xf = x.contiguous().float()
    log = Logger()
    q = quantizer(logger=log)
    fb, copies = iq.HALF_FALLBACKS, ops.LAYOUT_COPIES
    y = q(x, 'act')
    assert is_cl(y) and y.dtype == dtype and y.shape == x.shape
    assert iq.HALF_FALLBACKS == fb and ops.LAYOUT_COPIES == copies
    y_ref, e_ref = ops.act_qdq_per_channel(xf, 4, want_entropy=True)
    assert same(y, y_ref.to(dtype))
    assert len(log.rows) == 1 and log.rows[0][0] == 'act.entropy' and log.rows[0][2] == 'avg.entropy.act'
    assert log.rows[0][1] == float(e_ref) and log.rows[0][3] == x.numel()
    q.force_positive = True
    xp = cl(values((8, 32, 14, 14), seed=6, positive=True), dtype)
    yp_ref, ep_ref = ops.act_qdq_per_channel(xp.contiguous().float(), 4, positive=True, want_entropy=True)
    yp = q(xp, 'act')
    assert is_cl(yp) and same(yp, yp_ref.to(dtype)) and log.rows[-1][1] == float(ep_ref)
    q.force_positive = False
    # with a stat_id and a stub statistics manager
    rows = {'min': xf.amin(dim=(0, 2, 3)) * 0.8, 'max': xf.amax(dim=(0, 2, 3)) * 0.9}

    class SM:
        def get_tensor_stat(self, stat_id, stat, kind='mean'):
            return rows[stat].cpu().numpy()
    q.sm = SM
    ys = q(x, 'act', stat_id='layer0')
    assert is_cl(ys) and ys.dtype == dtype
    assert iq.HALF_FALLBACKS == fb and ops.LAYOUT_COPIES == copies
    table = torch.zeros((L.NSTAT, 32), dtype=torch.float32, device='cuda')
    table[L.STAT_MIN], table[L.STAT_MAX] = rows['min'], rows['max']
    ys_ref, es_ref = ops.act_qdq_per_channel(xf, 4, stats=table, want_entropy=True)
    assert same(ys, ys_ref.to(dtype)) and log.rows[-1][1] == float(es_ref)
    # config 3 with the entropy measurement still makes its one counted copy (tests/test_channels_last_aciq_gpu.py pins it)
    half = int(dtype != torch.float32)
    q3 = quantizer(clipping='laplace', bit_alloc_act=True)
    fb, copies = iq.HALF_FALLBACKS, ops.LAYOUT_COPIES
    y3 = q3(x, 'act')
    assert (iq.HALF_FALLBACKS, ops.LAYOUT_COPIES) == (fb + half, copies + 1) and y3.is_contiguous() and y3.dtype == dtype
    # an NCHW tensor behaves as before
    fb, copies = iq.HALF_FALLBACKS, ops.LAYOUT_COPIES
    yn = q(x.contiguous(), 'act')
    assert yn.is_contiguous() and (iq.HALF_FALLBACKS, ops.LAYOUT_COPIES) == (fb + half, copies)
