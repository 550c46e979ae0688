"""CPU-only checks of per-tensor clipping and mid-tread over flat storage: the five entry points exist
and their ctypes prototypes match the header, bad arguments are refused before anything touches the device, the workspace is
the flat-row statistics', the quantizer's three routing predicates as truth tables with _half_native's answers unchanged next to
them, the ops functions' refusals - and that the oracle, fed statistics one fp32 ulp off, stays inside the cap that
tests/test_tensor_clip_gpu.py holds the kernels to on that file's shapes (were it not so, the cap would be wrong for them).
The GPU file imports its shapes and inputs from here."""
import ctypes
import os

import numpy as np
import pytest
import torch

import _quantizer as Q
from test_channels_last_collect_cpu import BAD, EINVAL, ERANGE, ctype_of, header_decls, lib

FUNCS = ['cnnq_flat_qdq', 'cnnq_flat_midtread_qdq', 'cnnq_pt_clip_workspace', 'cnnq_pt_clip_qdq', 'cnnq_pt_midtread']
DTYPES = [torch.float32, torch.bfloat16, torch.float16]
IDS = ['f32', 'bf16', 'f16']

# ---- the shapes and inputs of the GPU file
# contiguous: one element (all tail), 7 (no whole 16-byte piece of bf16), 4099 (whole workgroups' worth of lanes plus an odd
# tail), the three shapes of test_per_tensor_clipping_vs_oracle, and many workgroups plus a tail
CONTIGUOUS = [(1,), (7,), (4099,), (8, 37), (16, 1000), (4, 6, 5, 5), (8, 64, 28, 28)]
OFFSET_VIEW = 1 + 4 * 6 * 49          # flat[1:] of this many elements: an unaligned base, one-element pieces
CHANNELS_LAST = [(3, 5, 7, 9), (2, 8, 4, 4)]
CLIPS = ['laplace', 'gaus', '2std']


def values(shape, seed=0):
    """The inputs of tests/test_hip_parity.py::test_per_tensor_clipping_vs_oracle: randn * 1.3 + 0.2, float32."""
    n = int(np.prod(shape))
    gen = torch.Generator().manual_seed(len(shape) * 7 + n % 1000 + seed)
    return torch.randn(shape, generator=gen) * 1.3 + 0.2


def oracle_cap(y, ref, step):
    """Contract item 3's condition on the values: (max |y - ref| <= 1.01 step, share off by more than 1e-5 below 2e-3); NaN
    positions have to agree."""
    y, ref = y.double().reshape(-1), ref.double().reshape(-1)
    assert torch.equal(torch.isnan(y), torch.isnan(ref))
    d = (y - ref).abs()
    d = d[~torch.isnan(d)]
    if d.numel() == 0:
        return True, True
    return float(d.max()) <= 1.01 * step, float((d > 1e-5).double().mean()) < 2e-3


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
            want = ctypes.c_double if a.startswith('double ') else ctype_of(a)
            if want == 'ptr':
                assert t is ctypes.c_void_p or issubclass(t, ctypes._Pointer), (name, a, t)
            else:
                assert t is want, (name, a, t)


def cfg(num_bits=4, clip=1, bit_alloc=0):
    from cnn_quantization_amd import _lib as L
    return L.ParamsCfg(num_bits, 0, clip, 2.0, bit_alloc, 0, 4.0, 1, 1)


P, Y = ctypes.c_void_p(BAD), ctypes.c_void_p(BAD + 0x1000)
TABLES = ctypes.c_void_p(BAD + 0x2000)


def flat_args(dtype=0, n=100):
    return [P, Y, dtype, n, P, None]                                         # x, y, dtype, n, table, stream


def clip_args(dtype=0, n=100, c=None):
    return [P, Y, dtype, n, ctypes.byref(c or cfg()), P, P, P, P, None]      # x, y, dtype, n, cfg, ws, stats, qp, diag, stream


def mt_args(dtype=0, n=100, target=4.0, ntab=101):
    return [P, Y, dtype, n, target, 1, TABLES, ntab, P, P, P, None]          # x, y, dtype, n, target, sym, tables, ntab, ws, stats, mt, stream


def every(dtype=0, n=100):
    L = lib()
    return [(L.cnnq_flat_qdq, flat_args(dtype, n)), (L.cnnq_flat_midtread_qdq, flat_args(dtype, n)),
            (L.cnnq_pt_clip_qdq, clip_args(dtype, n)), (L.cnnq_pt_midtread, mt_args(dtype, n))]


@pytest.mark.parametrize('dtype, n', [(-1, 100), (3, 100), (1 << 20, 100), (0, 0), (1, -5), (2, 0)])
def test_bad_dtype_or_size_is_einval(dtype, n):
    assert lib().cnnq_pt_clip_workspace(n, dtype) == 0
    for fn, a in every(dtype, n):
        assert fn(*a) == EINVAL, fn.__name__


@pytest.mark.parametrize('dtype', [0, 1, 2])
def test_bad_pointers_are_einval_and_huge_sizes_erange(dtype):
    esize = 4 if dtype == 0 else 2
    for fn, a in every(dtype):
        for i in (0, 1):                                                     # x, y: NULL, not aligned to the element, the same
            b = list(a)
            b[i] = None
            assert fn(*b) == EINVAL, (fn.__name__, i)
            b = list(a)
            b[i] = ctypes.c_void_p(BAD + 0x100 * i + esize // 2)
            assert fn(*b) == EINVAL, (fn.__name__, i)
        b = list(a)
        b[1] = b[0]
        assert fn(*b) == EINVAL, fn.__name__
        for n in ((1 << 60) + 1, (1 << 62), (1 << 63) - 1):                  # byte offsets beyond 63 bits
            b = list(a)
            b[3] = n
            assert fn(*b) == ERANGE, (fn.__name__, n)
    # 2^31 workgroups of 1024 one-element pieces (x two bytes off a 16-byte boundary: fp32 is refused before, as misaligned)
    if dtype != 0:
        for fn, a in every(dtype, 1 << 42):
            a[0] = ctypes.c_void_p(BAD + 2)
            assert fn(*a) == ERANGE, fn.__name__
    for i in (4,):                                                           # the table of the table-driven passes
        for fn in (lib().cnnq_flat_qdq, lib().cnnq_flat_midtread_qdq):
            a = flat_args(dtype)
            a[i] = None
            assert fn(*a) == EINVAL
    for i in (4, 5, 6, 7):                                                   # cfg, ws, stats, qp (diag may be NULL)
        a = clip_args(dtype)
        a[i] = None
        assert lib().cnnq_pt_clip_qdq(*a) == EINVAL, i
    a = clip_args(dtype)
    a[5] = ctypes.c_void_p(BAD + 4)                                          # ws holds doubles
    assert lib().cnnq_pt_clip_qdq(*a) == EINVAL
    for c in (cfg(clip=0), cfg(bit_alloc=1), cfg(num_bits=0), cfg(num_bits=9), cfg(num_bits=9, clip=2), cfg(num_bits=33, clip=3),
              cfg(clip=4), cfg(clip=-1)):
        assert lib().cnnq_pt_clip_qdq(*clip_args(dtype, c=c)) == EINVAL, (c.num_bits, c.clip, c.bit_alloc)
    for i in (6, 8, 9, 10):                                                  # tables, ws, stats, mt
        a = mt_args(dtype)
        a[i] = None
        assert lib().cnnq_pt_midtread(*a) == EINVAL, i
    a = mt_args(dtype)
    a[8] = ctypes.c_void_p(BAD + 4)
    assert lib().cnnq_pt_midtread(*a) == EINVAL
    for ntab in (-1, 0, 1):
        assert lib().cnnq_pt_midtread(*mt_args(dtype, ntab=ntab)) == EINVAL
    for target in (float('nan'), float('inf'), -float('inf')):
        assert lib().cnnq_pt_midtread(*mt_args(dtype, target=target)) == EINVAL


@pytest.mark.parametrize('dtype', [0, 1, 2])
def test_workspace_is_the_flat_row_statistics(dtype):
    for n in (1, 7, 8, 4096, 4099, 65536, 3 * 65536 + 24, 1 << 23, 512 * 64 * 112 * 112):
        want = lib().cnnq_rows_stats_workspace(1, n, dtype)
        assert want > 0 and lib().cnnq_pt_clip_workspace(n, dtype) == want, n


# ---- the quantizer's predicates
on_device = Q.FakeCuda


def quantizer(**kw):
    return Q.quantizer(**dict(dict(clipping='laplace'), **kw))


def tensors():
    """(name, tensor, dense layout or None, 4-D with a spatial extent) over dtype x layout x rank."""
    out = []
    for dt in DTYPES:
        z = lambda *s: torch.zeros(*s, dtype=dt)
        out += [('nchw', z(2, 8, 4, 4), 'nchw', True),
                ('nhwc', z(2, 8, 4, 4).to(memory_format=torch.channels_last), 'nhwc', True),
                ('2d', z(8, 16), 'nchw', False),
                ('1x1', z(2, 8, 1, 1), 'nchw', False),
                ('view', z(2, 8, 4, 4)[:, 2:5], None, True),
                ('empty', z(0, 8), 'nchw', False)]
    return out


def half_native_of_the_parent(q, t, stat_id, pending):
    """_half_native as the parent commit computes it, restated (tests/test_channels_last_entropy_cpu.py does the same)."""
    from cnn_quantization_amd import ops
    pc = len(t.shape) > 3 and (t.shape[2] > 1 or t.shape[3] > 1)
    nhwc = t.dim() == 4 and not t.is_contiguous() and t.is_contiguous(memory_format=torch.channels_last) and ops._NHWC
    one_gpu = q._one_gpu()
    if q.kld:
        return False
    bc = bool(stat_id is not None and pending is not None and q.pcq_a and pc and q.clipping in ('no', 'laplace', 'gaus')
              and not (q.clipping == 'no' and q.pcq_w) and nhwc and not q.mtd_quant and not q.measure_entropy and one_gpu)
    if bc:
        return True
    if q.clipping != 'no':
        return bool(not q.mtd_quant and q.pcq_a and pc and q.clipping in ('laplace', 'gaus') and nhwc and not q.measure_entropy
                    and pending is None and one_gpu)
    if q.pcq_w:
        return False
    if q.pcq_a and pc:
        return bool(not q.mtd_quant and not q.measure_entropy and pending is None and not (q.bit_alloc_act and q.num_bits <= 4)
                    and one_gpu)
    return True


CONFIGS = [dict(clipping=c, pcq_act=p, mtd_quant=m, kld=k)
           for c in ('no', 'laplace', 'gaus', '2std', 'mix') for p in (False, True) for m in (False, True) for k in (False, True)]


@pytest.mark.parametrize('cuda', [True, False])
def test_predicate_truth_table(cuda):
    for kw in CONFIGS:
        q = quantizer(**kw)
        for name, t, layout, pc in tensors():
            x = on_device(t) if cuda else t
            half = t.dtype != torch.float32
            flat = cuda and t.numel() > 0 and layout is not None and (half or layout == 'nhwc')
            per_tensor = not (q.pcq_a and pc)
            want_clip = bool(flat and per_tensor and q.clipping in ('laplace', 'gaus', '2std') and not q.mtd_quant and not q.kld)
            want_mt = bool(flat and per_tensor and q.clipping != 'no' and q.mtd_quant and not q.kld)
            want_kld = bool(cuda and q.kld and half and layout is not None)
            assert bool(q._flat_clip(x)) == want_clip, (kw, name, t.dtype)
            assert bool(q._flat_midtread(x)) == want_mt, (kw, name, t.dtype)
            assert bool(q._flat_kld(x)) == want_kld, (kw, name, t.dtype)
            # at most one of them, and never together with a route that was there before
            assert want_clip + want_mt + want_kld <= 1
            if want_clip or want_mt or want_kld:
                assert not q._half_native(x) and not q._nhwc_midtread(x) and not q._nhwc_entropy(x), (kw, name, t.dtype)


def test_half_native_answers_as_before():
    for kw in CONFIGS + [dict(clipping='no', pcq_act=True, measure_entropy=True), dict(clipping='laplace', pcq_act=True, bits=8),
                         dict(clipping='no', pcq_act=True, bit_alloc_act=True), dict(clipping='no', pcq_weights=True)]:
        q = quantizer(**kw)
        for pending in (None, True):
            q.fuse_bcorr = pending
            for name, t, layout, pc in tensors():
                for stat_id in (None, 'id'):
                    for x in (t, on_device(t)):
                        assert bool(q._half_native(x, None, stat_id)) == half_native_of_the_parent(q, t, stat_id, pending), \
                            (kw, pending, name, t.dtype, stat_id)


def test_override_pair_sharding_and_switches(monkeypatch):
    from cnn_quantization_amd import distributed as D, ops
    x = on_device(torch.zeros(2, 8, 4, 4, dtype=torch.bfloat16).to(memory_format=torch.channels_last))
    q = quantizer()
    assert q._flat_clip(x) and not q._flat_midtread(x) and not q._flat_kld(x)
    # __call__'s override pair is looked at (through _att)
    for att in (('clipping', 'no'), ('clipping', 'mix'), ('mtd_quant', True), ('kld', True), ('pcq_a', True)):
        assert not q._flat_clip(x, q._att(att)), att
    assert q._flat_midtread(x, q._att(('mtd_quant', True))) and q._flat_kld(x, q._att(('kld', True)))
    qn = quantizer(clipping='no')
    assert not qn._flat_clip(x) and qn._flat_clip(x, qn._att(('clipping', 'gaus')))
    # replicated data, a sharded batch, a forced exchange: the code they take today
    qm = quantizer(mtd_quant=True)
    q.group = qm.group = False
    assert not q._flat_clip(x) and not qm._flat_midtread(x)
    q.group = qm.group = None
    monkeypatch.setattr(D, 'world_size', lambda group=None: 2)
    assert not q._flat_clip(x) and not qm._flat_midtread(x)
    monkeypatch.undo()
    monkeypatch.setattr(D, 'forced_exchange', lambda: True)
    assert not q._flat_clip(x) and not qm._flat_midtread(x)
    monkeypatch.undo()
    assert q._flat_clip(x) and qm._flat_midtread(x)
    # CNNQ_NHWC=0: a channels_last tensor is no flat tensor to the quantizer (it takes the counted copy); a contiguous half one stays
    c = on_device(torch.zeros(8, 16, dtype=torch.float16))
    old = os.environ.get('CNNQ_NHWC')
    try:
        os.environ['CNNQ_NHWC'] = '0'
        ops.reload_switches()
        assert not q._flat_clip(x) and not qm._flat_midtread(x) and q._flat_clip(c)
    finally:
        if old is None:
            os.environ.pop('CNNQ_NHWC', None)
        else:
            os.environ['CNNQ_NHWC'] = old
        ops.reload_switches()
    assert q._flat_clip(x)


# ---- the ops functions refuse what they do not take, without copying
def test_ops_refuse_cpu_float64_and_non_dense_tensors():
    from cnn_quantization_amd import _lib as L, ops
    before = ops.LAYOUT_COPIES
    bad = [torch.zeros(2, 8, 4, 4), torch.zeros(2, 8, 4, 4).to(memory_format=torch.channels_last),      # CPU
           torch.zeros(2, 8, 4, 4, dtype=torch.bfloat16), torch.zeros(8, 16, dtype=torch.float64),        # CPU, float64
           torch.zeros(2, 8, 4, 4)[:, 2:5], torch.zeros(8, 16).t(), torch.zeros(64)[::2],                  # not dense
           torch.zeros(0, 4), torch.zeros(8, 16, dtype=torch.int32), [1., 2.]]
    for t in bad:
        for x in ([t, on_device(t)] if isinstance(t, torch.Tensor) and (t.dtype == torch.float64 or ops._layout(t) == 'copy') else [t]):
            with pytest.raises(L.CnnqError):
                ops.clip_qdq_tensor(x, 4)
            with pytest.raises(L.CnnqError):
                ops.mid_tread_qdq_tensor(x, 4, True)
    assert ops.LAYOUT_COPIES == before


# ---- contract item 3's cap on this file's shapes
@pytest.mark.parametrize('clip', CLIPS)
@pytest.mark.parametrize('half', [False, True])
def test_oracle_with_statistics_one_ulp_off_stays_inside_the_cap(clip, half):
    """The kernels' whole-tensor mean / b / std are promised within the statistics tier, not equal to the oracle's.  What one fp32
    ulp in each of them does to the oracle's own result bounds what the cap of contract item 3 has to allow: on every shape of
    the GPU file, both directions, it stays inside the cap (range and offset inside rtol 3e-6 a fortiori)."""
    from oracle import quant_oracle as O
    for shape in CONTIGUOUS[1:] + [(OFFSET_VIEW,)] + CHANNELS_LAST:          # one element has no standard deviation: NaN either way
        x = values(shape)
        st = O.act_stats(x, ['min', 'max', 'mean'])
        mn, mx, mean = (np.float32(float(st[k])) for k in ('min', 'max', 'mean'))
        name = 'b' if clip == 'laplace' else 'std'
        prior = np.float32(float(O.act_stats(x, [name])[name]))
        factor = O.aciq_factor(4, clip, half) if clip in ('laplace', 'gaus') else float(clip.replace('std', ''))

        def run(mean_, prior_):
            rng, off = O.alpha_to_delta_offset(float(prior_) * factor, float(mx), float(mn), float(mean_), half)
            return O.qdq_core(x.contiguous(), O._as_f32(rng), O._as_f32(off), num_bits=4), float(rng)
        ref, rng = run(mean, prior)
        step = rng / 15
        for dm in (-1, 0, 1):
            for dp in (-1, 0, 1):
                m = np.nextafter(mean, np.float32(np.inf * dm)) if dm else mean
                p = np.nextafter(prior, np.float32(np.inf * dp)) if dp else prior
                y, r = run(m, p)
                assert abs(r - rng) <= 3e-6 * abs(rng)
                assert oracle_cap(y, ref, step) == (True, True), (shape, clip, half, dm, dp)
