"""Per-tensor clipping and per-tensor mid-tread over flat storage, fp32 / bf16 / fp16, contiguous and dense
channels_last.  The contract:
  1. given the table, bit for bit: clip_qdq_tensor(x, stats=t) equals act_qdq_per_channel(x.float().contiguous(), whole_tensor=True,
     stats=t) cast to x's dtype, read in x's logical order, NaN positions and signed zeros included; cnnq_flat_midtread_qdq equals
     cnnq_pc_midtread_qdq on N = 1, C = 1 with the same mt;
  2. the dynamic form: its statistics are ops.tensor_stats' (the same kernels in the same order), its parameters pc_params' of that
     table, its y the table-driven call's on that table - equalities, no tolerance;
  3. against the oracle on fp32 inputs, the condition tests/test_hip_parity.py::test_per_tensor_clipping_vs_oracle holds the
     fp32 route to (the scalar statistics differ in the last bits: tests/test_tensor_clip_cpu.py shows that one ulp in them
     keeps the oracle itself inside the cap on these shapes)."""
import numpy as np
import pytest
import torch

from test_channels_last_gpu import cl, is_cl, same
from test_tensor_clip_cpu import CHANNELS_LAST, CLIPS, CONTIGUOUS, DTYPES, IDS, OFFSET_VIEW, oracle_cap, values

pytestmark = pytest.mark.gpu

CASES = [('c', s) for s in CONTIGUOUS] + [('view', (OFFSET_VIEW,))] + [('cl', s) for s in CHANNELS_LAST]
CASE_IDS = ['%s-%s' % (k, 'x'.join(map(str, s))) for k, s in CASES]


def mods():
    from cnn_quantization_amd import _lib as L, ops
    return L, ops


def place(kind, v, dtype):
    """The fp32 CPU values v on the device as dtype: contiguous, a view one element into its storage, or dense channels_last."""
    if kind == 'cl':
        return cl(v, dtype)
    if kind == 'view':
        base = torch.zeros(v.numel() + 1, dtype=dtype, device='cuda')
        x = base[1:]
        x.copy_(v.to(dtype))
        assert x.is_contiguous() and x.storage_offset() == 1
        return x
    return v.to(dtype).cuda()


def make(kind, shape, dtype, seed=0):
    return place(kind, values(shape, seed), dtype)


def table_of(x):
    """A whole-tensor statistics table [NSTAT, 1] for x: the device's own."""
    return mods()[1].tensor_stats(x, 1)[0]


def ref_clip(x, bits, positive, clip, t):
    """The fp32 route on the same values with the same table (contract item 1's right-hand side) -> (y as x.dtype, parts)."""
    L, ops = mods()
    y, parts = ops.act_qdq_per_channel(x.float().contiguous(), bits, positive=positive, clip=clip, whole_tensor=True, stats=t,
                                       want_parts=True, group=False)
    return y.view(x.shape).to(x.dtype), parts


def poisoned(x):
    """A result buffer like x, full of NaN: an element the kernel does not store cannot look right by what the allocator left there."""
    y = torch.full_like(x, float('nan'))
    assert y.stride() == x.stride()
    return y


def flat_call(fn, x, tab):
    """cnnq_flat_qdq / cnnq_flat_midtread_qdq on x's storage with a device table."""
    L, ops = mods()
    y = poisoned(x)
    rc = getattr(L.load(), fn)(x.data_ptr(), y.data_ptr(), ops._DTYPE_CODES[x.dtype], x.numel(), tab.data_ptr(), ops._stream(x))
    assert rc == 0, (fn, rc)
    return y


def ref_flat_qdq(x, qp):
    _, ops = mods()
    xf = x.float().contiguous()
    return ops.pc_qdq(xf.view(-1), 1, 1, xf.numel(), qp).view(x.shape).to(x.dtype)


def ref_flat_midtread(x, mt):
    L, ops = mods()
    xf = x.float().contiguous()
    y = torch.empty_like(xf)
    L.check(L.load().cnnq_pc_midtread_qdq(xf.data_ptr(), y.data_ptr(), 1, 1, xf.numel(), mt.data_ptr(), 1, None, None, ops._stream(xf)),
            'cnnq_pc_midtread_qdq')
    return y.view(x.shape).to(x.dtype)


def mt_of(stats, target, sym):
    L, ops = mods()
    tabs = ops._midtread_tables(stats.device)
    mt = torch.empty((L.NMT, 1), dtype=torch.float32, device=stats.device)
    L.check(L.load().cnnq_pc_midtread_params(stats.data_ptr(), 1, float(target), 1, int(sym), tabs.data_ptr(), tabs.shape[1], mt.data_ptr(),
                                             ops._stream(stats)), 'cnnq_pc_midtread_params')
    return mt


def kept(x, y):
    assert y.dtype == x.dtype and y.shape == x.shape and y.stride() == x.stride()


# ---- contract items 1 and 2
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('case', CASES, ids=CASE_IDS)
def test_clipping_given_the_table_and_dynamic(case, dtype):
    L, ops = mods()
    x = make(case[0], case[1], dtype)
    t = table_of(x)
    copies = ops.LAYOUT_COPIES
    for bits in (4, 8):
        for clip in CLIPS:
            for positive in (False, True):
                what = (case, dtype, bits, clip, positive)
                # 1. given the table
                y, parts = ops.clip_qdq_tensor(x, bits, positive=positive, clip=clip, stats=t, want_parts=True, out=poisoned(x))
                kept(x, y)
                y_ref, p_ref = ref_clip(x, bits, positive, clip, t)
                assert same(parts['qp'], p_ref['qp']) and same(parts['diag'], p_ref['diag']), what
                assert same(y, y_ref), what
                # 2. the dynamic form
                yd, pd = ops.clip_qdq_tensor(x, bits, positive=positive, clip=clip, want_parts=True, out=poisoned(x))
                kept(x, yd)
                assert same(pd['stats'], ops.tensor_stats(x, 1, need_dev=clip == 'laplace')[0]), what
                rows = [L.STAT_MIN, L.STAT_MAX, L.STAT_MEAN, L.STAT_STD, L.STAT_STD_POS] + ([L.STAT_B, L.STAT_KURT] if clip == 'laplace' else [])
                assert same(pd['stats'][rows], t[rows]), what
                qp, diag = ops.pc_params(pd['stats'], bits, positive, clip, direct_range=True)
                assert same(pd['qp'], qp) and same(pd['diag'], diag), what
                assert same(yd, ops.clip_qdq_tensor(x, bits, positive=positive, clip=clip, stats=pd['stats'].contiguous())), what
                assert same(yd, ops.clip_qdq_tensor(x, bits, positive=positive, clip=clip)), what          # without parts: the same
    assert ops.LAYOUT_COPIES == copies


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('case', CASES, ids=CASE_IDS)
def test_midtread_given_the_table_and_dynamic(case, dtype):
    L, ops = mods()
    x = make(case[0], case[1], dtype, seed=1)
    t = table_of(x)
    copies = ops.LAYOUT_COPIES
    for target in (2, 4):
        for sym in (True, False):
            what = (case, dtype, target, sym)
            mt = mt_of(t, target, sym)
            y = flat_call('cnnq_flat_midtread_qdq', x, mt)
            assert same(y, ref_flat_midtread(x, mt)), what
            yd, pd = ops.mid_tread_qdq_tensor(x, target, sym, want_parts=True, out=poisoned(x))
            kept(x, yd)
            assert same(pd['stats'], t), what
            assert same(pd['mt'], mt), what
            assert same(yd, y), what
            assert same(yd, ops.mid_tread_qdq_tensor(x, target, sym)), what
    assert ops.LAYOUT_COPIES == copies


# ---- hand-built values
def hand_values():
    """scale 0.25, zero point 3, 4 bits: every exact .5 tie of x / scale + zp from below the lower to above the upper clamp bound,
    values far beyond both, +-0, denormals, NaN and +-inf - all exact in bf16 and fp16; 45 elements: pieces and a tail."""
    ties = [(k + 0.5 - 3) * 0.25 for k in range(-3, 19)]
    whole = [(k - 3) * 0.25 for k in range(-2, 18)]
    return torch.tensor(ties + whole + [-100., 1000., 0., -0., 2. ** -20, -2. ** -20, float('nan'), float('inf'), -float('inf')],
                        dtype=torch.float32)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('kind', ['c', 'view'])
def test_hand_built_ties_clamps_zeros_and_non_finite(kind, dtype):
    v = hand_values()
    x = place(kind, v, dtype)
    assert torch.equal(x.float().cpu().nan_to_num(7.), v.nan_to_num(7.))                  # exact in every dtype
    for scale, zp, qmax in ((0.25, 3., 15.), (0.25, 0., 15.), (0.1, 7., 255.), (1e-8, 0., 15.)):
        qp = torch.tensor([[scale], [zp], [qmax]], dtype=torch.float32, device='cuda')
        y = flat_call('cnnq_flat_qdq', x, qp)
        assert same(y, ref_flat_qdq(x, qp)), (scale, zp, qmax)
        if scale == 0.25 and zp == 3.:
            # what the arithmetic is, spelled out on the CPU: half to even, clamp before round, NaN kept
            q = torch.clamp(v / 0.25 + 3., 0., 15.).round()
            want = ((q - 3.) * 0.25).to(dtype)
            assert same(y.cpu(), want)
    # mid-tread: a non-integer upper bound, ties of x / delta
    for delta, lo, hi in ((0.25, -3.5, 4.), (0.25, -2., 2.5), (0.1, -8., 7.)):
        mt = torch.tensor([[delta], [lo], [hi], [0.], [0.], [0.]], dtype=torch.float32, device='cuda')
        y = flat_call('cnnq_flat_midtread_qdq', x, mt)
        assert same(y, ref_flat_midtread(x, mt)), (delta, lo, hi)
        if delta == 0.25:
            tq = (v / 0.25).round()
            tq = torch.where(tq < hi, tq, torch.full_like(tq, hi))
            tq = torch.where(tq > lo, tq, torch.full_like(tq, lo))
            tq = torch.where(torch.isnan(v), v, tq)
            assert same(y.cpu(), (tq * 0.25).to(dtype))


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_constant_and_non_finite_tensors_follow_the_fp32_route(dtype):
    L, ops = mods()
    const = torch.full((3, 5, 7), 0.75, dtype=dtype, device='cuda')
    nan = make('c', (8, 37), dtype, seed=3)
    nan.view(-1)[17] = float('nan')
    inf = make('c', (8, 37), dtype, seed=4)
    inf.view(-1)[5], inf.view(-1)[200] = float('inf'), -float('inf')
    for x in (const, nan, inf):
        for clip in CLIPS:
            for positive in (False, True):
                y, p = ops.clip_qdq_tensor(x, 4, positive=positive, clip=clip, want_parts=True)
                y_ref, p_ref = ref_clip(x, 4, positive, clip, p['stats'].contiguous())
                assert same(p['qp'], p_ref['qp']) and same(y, y_ref), (clip, positive)
        yd, pd = ops.mid_tread_qdq_tensor(x, 4, True, want_parts=True)
        assert same(yd, ref_flat_midtread(x, pd['mt'].contiguous()))
    # range 0: the scale is the 1e-8 floor
    _, p = ops.clip_qdq_tensor(const, 4, clip='gaus', want_parts=True)
    assert float(p['qp'][L.QP_SCALE][0]) == float(np.float32(1e-8))
    # a finite table on a tensor with non-finite elements
    t = table_of(make('c', (8, 37), dtype, seed=3))
    for x in (nan, inf):
        y = ops.clip_qdq_tensor(x, 4, stats=t)
        assert same(y, ref_clip(x, 4, False, 'laplace', t)[0])
        assert torch.equal(torch.isnan(y), torch.isnan(x))


# ---- contract item 3
@pytest.mark.parametrize('case', [c for c in CASES if c[1] != (1,)], ids=[i for c, i in zip(CASES, CASE_IDS) if c[1] != (1,)])
def test_clipping_vs_oracle(case):
    """One element has no standard deviation (NaN in the oracle and here): the other shapes."""
    from oracle import quant_oracle as O
    L, ops = mods()
    v = values(case[1])
    x = place(case[0], v, torch.float32)
    for clip in CLIPS:
        for half in (False, True):
            ref, parts = O.act_clipping_qdq(v, 4, clip_type=clip, half_range=half, pcq_a=False, return_parts=True)
            y, p = ops.clip_qdq_tensor(x, 4, positive=half, clip=clip, want_parts=True)
            diag = p['diag'].cpu()
            step = float(p['qp'][0][0])
            d = (y.cpu() - ref).abs()
            print(case, clip, half, 'range', float(diag[L.DIAG_DELTA][0]), float(parts['range']), 'offset', float(diag[L.DIAG_OFFSET][0]),
                  float(parts['offset']), 'max', float(d.max()), 'step', step, 'share', float((d > 1e-5).float().mean()))
            np.testing.assert_allclose(float(diag[L.DIAG_DELTA][0]), float(parts['range']), rtol=3e-6)
            np.testing.assert_allclose(float(diag[L.DIAG_OFFSET][0]), float(parts['offset']), rtol=3e-6, atol=1e-7)
            assert oracle_cap(y.cpu(), ref, step) == (True, True), (case, clip, half)


# ---- determinism, graphs
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_same_call_twice_gives_equal_bytes(dtype):
    _, ops = mods()
    for kind, shape in (('c', (8, 64, 28, 28)), ('cl', (3, 5, 7, 9)), ('view', (OFFSET_VIEW,))):
        x = make(kind, shape, dtype, seed=5)
        iv = torch.int32 if dtype == torch.float32 else torch.int16
        for f in (lambda: ops.clip_qdq_tensor(x, 4, want_parts=True), lambda: ops.mid_tread_qdq_tensor(x, 4, True, want_parts=True)):
            (a, pa), (b, pb) = f(), f()
            assert torch.equal(a.contiguous().view(iv), b.contiguous().view(iv))
            for k in pa:
                assert torch.equal(pa[k].contiguous().view(torch.int32), pb[k].contiguous().view(torch.int32)), k


@pytest.mark.parametrize('form', ['clip', 'midtread'])
def test_graph_capture_replays_eager(form):
    _, ops = mods()
    run = (lambda t: ops.clip_qdq_tensor(t, 4)) if form == 'clip' else (lambda t: ops.mid_tread_qdq_tensor(t, 4, True))
    x = make('cl', (16, 64, 14, 14), torch.bfloat16, seed=2)
    eager = run(x)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run(x)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        y = run(x)
    x.copy_(make('cl', (16, 64, 14, 14), torch.bfloat16, seed=3))
    graph.replay()
    torch.cuda.synchronize()
    assert is_cl(y) and same(y, run(x))
    assert not same(y, eager)


def test_out_argument_and_refusals():
    L, ops = mods()
    x = make('cl', (2, 8, 4, 4), torch.float16)
    out = torch.empty_like(x)
    assert ops.clip_qdq_tensor(x, 4, out=out) is out and same(out, ops.clip_qdq_tensor(x, 4))
    assert ops.mid_tread_qdq_tensor(x, 4, False, out=out) is out and same(out, ops.mid_tread_qdq_tensor(x, 4, False))
    copies = ops.LAYOUT_COPIES
    for bad in (dict(out=x), dict(out=torch.empty(x.shape, dtype=x.dtype, device='cuda')), dict(clip='no'), dict(clip='mix'),
                dict(stats=torch.zeros(L.NSTAT, 2, device='cuda')), dict(stats=torch.zeros(L.NSTAT, 1))):
        with pytest.raises(L.CnnqError):
            ops.clip_qdq_tensor(x, 4, **bad)
    for t in (x[:, 2:5], x.double(), torch.zeros(8, 16, device='cuda').t()):
        with pytest.raises(L.CnnqError):
            ops.clip_qdq_tensor(t, 4)
        with pytest.raises(L.CnnqError):
            ops.mid_tread_qdq_tensor(t, 4, True)
    with pytest.raises(L.CnnqError):
        ops.clip_qdq_tensor(x, 9, clip='laplace')
    assert ops.LAYOUT_COPIES == copies
