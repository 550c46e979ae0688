"""bf16 / fp16 activations for configs 1 and 2: every native path returns, bit for bit,
    y == fp32_path(x.float()).to(x.dtype)
(statistics of the exactly upconverted values, fp32 arithmetic, one round-to-nearest-even into the input type).  NaN positions
must agree; every other element is compared by its 16 bits."""
import pytest
import torch
from hypothesis import HealthCheck, given, settings
from hypothesis import strategies as st

from oracle import quant_oracle as O

pytestmark = pytest.mark.gpu
DTYPES = [torch.bfloat16, torch.float16]


def same(a, b):
    """Bitwise equality of two half tensors, every NaN equal to every NaN."""
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    na, nb = torch.isnan(a), torch.isnan(b)
    if not torch.equal(na, nb):
        return False
    return torch.equal(a.view(torch.int16)[~na], b.view(torch.int16)[~nb])


def make(shape, dtype, seed=0, offset=0, positive_shift=False):
    """A half tensor on the GPU; offset elements into a larger buffer (offset 1: a 2-byte aligned data_ptr)."""
    g = torch.Generator().manual_seed(seed)
    C = shape[1]
    x = torch.randn(shape, generator=g) * (0.2 + 3 * torch.rand(1, C, 1, 1, generator=g)) + torch.randn(1, C, 1, 1, generator=g)
    if positive_shift:
        x = x.relu()
    n = x.numel()
    base = torch.empty(n + 8, dtype=dtype, device='cuda')
    view = base[offset:offset + n].view(shape)
    view.copy_(x.to(dtype).cuda())
    return view


def cfg2(x, bits, positive, **kw):
    from cnn_quantization_amd import ops
    return ops.act_qdq_per_channel(x, bits, positive=positive, **kw)


def contract_cfg2(x, bits, positive, **kw):
    return cfg2(x.float(), bits, positive, **kw).to(x.dtype)


def routes(N, C, HW):
    """Which fp32 single-launch forms the geometry has (whole-channel, group exchange): the fp32 side of the contract."""
    from cnn_quantization_amd import _lib as L
    import ctypes
    lib = L.load()
    d = (ctypes.c_int32 * 8)()
    return dict(whole=lib.cnnq_pc_resident_describe(N, C, HW, d) == 0, group=lib.cnnq_pc_group_describe(N, C, HW, d) == 0)


def half_route(x):
    """(route, piece width) cnnq_pc_minmax_qdq_auto_dt takes for x: 1 the single launch k_h_whole, 2 the chain."""
    from cnn_quantization_amd import _lib as L
    import ctypes
    p = x.data_ptr()
    out = (ctypes.c_int32 * 4)()
    N, C = x.shape[0], x.shape[1]
    assert L.load().cnnq_pc_route_dt(N, C, x.numel() // (N * C), min(16, p & -p), 1, out) == 0
    return out[0], out[1]


SHAPES = [(4, 64, 7, 7), (64, 33, 7, 7), (1, 512, 7, 7), (4, 17, 14, 14), (64, 256, 14, 14), (4, 128, 28, 28),
          (64, 32, 28, 28), (1, 64, 56, 56), (4, 5, 56, 56), (64, 3, 112, 112), (1, 7, 112, 112), (4, 9, 3, 5), (64, 11, 1, 9),
          (8, 6, 2, 7)]


@pytest.mark.parametrize('dtype', DTYPES, ids=['bf16', 'f16'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_cfg2_every_geometry_matches_contract(shape, dtype):
    N, C, H, W = shape
    for bits in (2, 4, 8):
        for positive in (False, True):
            for offset in ((0, 1) if bits == 4 else (0,)):
                x = make(shape, dtype, seed=bits * 7 + positive + offset, offset=offset, positive_shift=positive)
                assert half_route(x)[0] in (1, 2)
                y = cfg2(x, bits, positive)
                assert y.dtype == dtype and y.shape == x.shape
                assert same(y, contract_cfg2(x, bits, positive)), (shape, bits, positive, offset)
                # the contract holds against the fp32 three-launch chain as well (every fp32 route gives the same bits)
                from cnn_quantization_amd import ops
                ych = ops.minmax_qdq_fused(x.float(), N, C, H * W, bits, positive, chain=True).to(dtype)
                assert same(y, ych)


def test_cfg2_geometries_cover_both_half_routes():
    """The geometries above take the single launch and the chain on the half side, at every piece width that occurs."""
    make((1, 1, 1, 1), torch.bfloat16)                    # the device is up
    seen = set()
    for N, C, H, W in SHAPES:
        for offset in (0, 1):
            seen.add(half_route(make((N, C, H, W), torch.bfloat16, offset=offset)))
    assert seen >= {(1, 8), (1, 4), (1, 2), (2, 8), (2, 1)}, seen


def test_cfg2_geometries_cover_every_fp32_route():
    """The geometries above reach the whole-channel and the group-exchange single launches and the chain on the fp32 side."""
    seen = {'whole': False, 'group': False, 'chain': False}
    for N, C, H, W in SHAPES:
        r = routes(N, C, H * W)
        seen['whole'] |= r['whole']
        seen['group'] |= r['group'] and not r['whole']
        seen['chain'] |= not (r['whole'] or r['group'])
    assert all(seen.values()), seen


@pytest.mark.parametrize('dtype', DTYPES, ids=['bf16', 'f16'])
def test_special_values(dtype):
    shape = (4, 8, 8, 8)
    x = make(shape, dtype, seed=3).clone()
    x[1, 0, 2, 3] = float('nan')                  # channel 0: NaN -> the whole channel NaN
    x[0, 1, 0, 0] = float('inf')                  # channel 1: +inf
    x[2, 2, 5, 1] = float('-inf')                 # channel 2: -inf
    x[:, 3] = 0.0                                 # channel 3: +-0 only
    x[:, 3, ::2] = -0.0
    tiny = torch.finfo(dtype).tiny
    x[:, 4] = (torch.arange(64, device='cuda').view(8, 8) - 32).to(dtype) * (tiny / 4)   # channel 4: subnormals
    x[:, 5] = 1.25                                # channel 5: constant (range 0)
    if dtype == torch.float16:
        x[3, 6, 7, 7] = 65504.0                   # channel 6: max at the fp16 maximum (values above it overflow to inf)
        x[0, 7, 0, 0] = -65504.0
    for bits in (2, 4, 8):
        for positive in (False, True):
            y = cfg2(x, bits, positive)
            assert same(y, contract_cfg2(x, bits, positive)), (bits, positive)
    assert torch.isnan(cfg2(x, 4, False)[:, 0]).all()


@pytest.mark.parametrize('dtype', DTYPES, ids=['bf16', 'f16'])
def test_golden_act_pc_cases(golden, dtype):
    """The act_pc golden inputs cast to the dtype, against the oracle's fp32 outputs on the upcast input."""
    g = golden('act_pc')
    i = 0
    while 'x%d' % i in g:
        xh = g.t('x%d' % i).to(dtype)
        for bits, half in ((4, False), (4, True), (8, False)):
            ref = O.act_per_channel_qdq(xh.float(), bits, half_range=half).to(dtype)
            y = cfg2(xh.cuda(), bits, half).cpu()
            assert same(y, ref), (i, bits, half)
        i += 1
    assert i >= 5


@pytest.mark.parametrize('dtype', DTYPES, ids=['bf16', 'f16'])
def test_stats_table_pc_qdq(dtype):
    """-sm use: the parameters from a calibration table ([NSTAT, C], rows MIN / MAX), the half pc_qdq."""
    from cnn_quantization_amd import _lib as L
    from cnn_quantization_amd import ops
    for shape, offset in (((8, 24, 14, 14), 0), ((4, 7, 7, 7), 1), ((2, 16, 28, 28), 1)):
        x = make(shape, dtype, seed=11, offset=offset)
        C = shape[1]
        table = torch.zeros((L.NSTAT, C), dtype=torch.float32, device='cuda')
        xf = x.float()
        table[L.STAT_MIN] = xf.amin(dim=(0, 2, 3)) * 0.8
        table[L.STAT_MAX] = xf.amax(dim=(0, 2, 3)) * 0.9
        for positive in (False, True):
            y = ops.act_qdq_per_channel(x, 4, positive=positive, stats=table)
            assert same(y, ops.act_qdq_per_channel(xf, 4, positive=positive, stats=table).to(dtype))
        # pc_qdq straight from a parameter table, with a caller's out buffer
        qp, _ = ops.pc_params(table, 4)
        out = torch.empty_like(x)
        N, C, HW = ops.geometry(x)
        assert ops.pc_qdq(x, N, C, HW, qp, out=out) is out
        assert same(out, ops.pc_qdq(xf, N, C, HW, qp).to(dtype))


@pytest.mark.parametrize('dtype', DTYPES, ids=['bf16', 'f16'])
def test_config1_per_tensor(dtype):
    from cnn_quantization_amd import int_quantization, ops
    for shape, offset in (((8, 16, 14, 14), 0), ((4, 3, 7, 7), 1), ((32, 1000), 0), ((5, 3, 9, 11), 1)):
        x = make(shape if len(shape) == 4 else (shape[0], shape[1], 1, 1), dtype, seed=5, offset=offset).view(shape)
        for args in ((2.5, -1.0, 4, False, True), (3.0, 0.0, 8, False, True), (1.7, -0.4, 2, True, False), (0.0, 0.0, 4, False, True)):
            y = int_quantization.float2gemmlowp(x, *args)
            assert same(y, int_quantization.float2gemmlowp(x.float(), *args).to(dtype)), args
        noise = (torch.rand(x.shape, device='cuda') - 0.5)
        y = int_quantization.float2gemmlowp(x, 2.0, -1.0, 4, False, True, noise)
        assert same(y, int_quantization.float2gemmlowp(x.float(), 2.0, -1.0, 4, False, True, noise).to(dtype))
        for avg in (False, True):
            for zero_min in (False, True):
                y = ops.minmax_qdq_per_tensor(x, 4, avg_over_batch=avg, zero_min=zero_min)
                ref = ops.minmax_qdq_per_tensor(x.float(), 4, avg_over_batch=avg, zero_min=zero_min).to(dtype)
                assert same(y, ref), (shape, avg, zero_min)
        rows = x.shape[0]
        assert torch.equal(ops.tensor_row_stats(x, rows), ops.tensor_row_stats(x.float(), rows))


@pytest.mark.parametrize('shape', [(512, 64, 112, 112), (512, 256, 56, 56)], ids=['112', '56'])
def test_full_size_bf16(shape):
    from cnn_quantization_amd import ops
    x = make((shape[0], shape[1], 1, 1), torch.bfloat16)      # per-channel offsets / scales, then the full tensor
    g = torch.Generator(device='cuda').manual_seed(9)
    x = (torch.randn(shape, generator=g, device='cuda') * (x[:1].float().abs() + 0.1) + x[:1].float()).to(torch.bfloat16)
    N, C, H, W = shape
    y = ops.minmax_qdq_fused(x, N, C, H * W, 4, False)
    ref = ops.minmax_qdq_fused(x.float(), N, C, H * W, 4, False).to(torch.bfloat16)
    assert same(y, ref)
    del y, ref
    y = ops.minmax_qdq_fused(x, N, C, H * W, 4, True)
    assert same(y, ops.minmax_qdq_fused(x.float(), N, C, H * W, 4, True).to(torch.bfloat16))


CFG = dict(max_examples=60, deadline=None, derandomize=True, suppress_health_check=list(HealthCheck))
shapes = st.tuples(st.integers(1, 6), st.integers(1, 40), st.integers(1, 19), st.integers(1, 19)).filter(lambda s: s[2] * s[3] > 1)


@settings(**CFG)
@given(shape=shapes, seed=st.integers(0, 2 ** 16), bits=st.sampled_from([2, 3, 4, 8]), half=st.booleans(),
       offset=st.integers(0, 7))
def test_bf16_random_geometry(shape, seed, bits, half, offset):
    x = make(shape, torch.bfloat16, seed=seed, offset=offset)
    assert same(cfg2(x, bits, half), contract_cfg2(x, bits, half))


def _params(**kw):
    p = dict(clipping='no', stats_kind='mean', true_zero=False, kld=False, pcq_weights=False, pcq_act=True,
             bit_alloc_act=False, bit_alloc_weight=False, bit_alloc_rmode='round', bit_alloc_prior='gaus',
             bit_alloc_target_act=None, bit_alloc_target_weight=None, bcorr_act=False, bcorr_weight=False,
             vcorr_weight=False, logger=None, measure_entropy=False, mtd_quant=False)
    p.update(kw)
    return p


@pytest.mark.parametrize('dtype', DTYPES, ids=['bf16', 'f16'])
def test_quantizer_configs_1_and_2_take_no_fallback(dtype):
    import sys
    from cnn_quantization_amd.qtypes import int_quantizer
    iq = sys.modules['cnn_quantization_amd.qtypes.int_quantizer']
    x = make((8, 24, 14, 14), dtype, seed=2)
    before = iq.HALF_FALLBACKS
    q2 = int_quantizer('int4', _params())
    y2 = q2(x, 'conv0_activation', 'activation')
    q1 = int_quantizer('int8', _params(pcq_act=False))
    y1 = q1(x, 'conv0_activation', 'activation')
    assert iq.HALF_FALLBACKS == before, 'configs 1 / 2 went through the upcast fallback'
    assert same(y2, q2(x.float(), 'conv0_activation', 'activation').to(dtype))
    assert same(y1, q1(x.float(), 'conv0_activation', 'activation').to(dtype))
    q3 = int_quantizer('int4', _params(clipping='laplace'))
    y3 = q3(x, 'conv0_activation', 'activation')
    assert iq.HALF_FALLBACKS == before + 1
    assert y3.dtype == dtype and same(y3, q3(x.float(), 'conv0_activation', 'activation').to(dtype))


def test_other_ops_refuse_half():
    from cnn_quantization_amd import _lib as L
    from cnn_quantization_amd import ops
    x = make((4, 8, 14, 14), torch.bfloat16)
    with pytest.raises(L.CnnqError):
        ops.pc_stats(x, 4, 8, 196)
    with pytest.raises(L.CnnqError):
        ops.act_qdq_per_channel(x, 4, clip='laplace')
    with pytest.raises(L.CnnqError):
        ops.act_qdq_per_channel(x, 4, want_codes=True)
    with pytest.raises(L.CnnqError):
        ops.quantize_u8(x, torch.zeros((L.NQP, 8), device='cuda'))
    with pytest.raises(L.CnnqError):                      # out= must match the input dtype
        ops.act_qdq_per_channel(x, 4, out=torch.empty(x.shape, device='cuda'))
