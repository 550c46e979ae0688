"""Every route of IntQuantizer's route table once through __call__, on (2, 8, 4, 4) activations - bf16
contiguous for the half routes, bf16 and fp32 dense channels_last for the channels_last ones, (2, 8, 1, 1) for config 1: the ops entry
point the table names is the one reached and no other, nothing is upcast or copied, dtype and layout are kept, and the result is bit
for bit what that entry point returns for the arguments the table implies.  Then one call per branch whose route is None on a bf16
tensor: exactly one counted upcast."""
import importlib

import pytest
import torch

from _quantizer import quantizer
from test_channels_last_gpu import cl, same, values

pytestmark = pytest.mark.gpu

SHAPE = (2, 8, 4, 4)
# what a branch method can call into, natively or on its fp32 path
ENTRIES = ('act_qdq_per_channel', 'pc_qdq', 'qdq_bias_corrected_nhwc', 'qdq_bias_corrected_half', 'aciq_qdq_nhwc', 'aciq_qdq_half',
           'clip_qdq_tensor', 'mid_tread_qdq', 'mid_tread_qdq_nhwc', 'mid_tread_qdq_tensor', 'minmax_qdq_per_tensor', 'pt_qdq',
           'act_qdq_mix')
NHWC = [('nhwc', torch.bfloat16), ('nhwc', torch.float32)]
HALF = [('nchw', torch.bfloat16)]


def mods():
    from cnn_quantization_amd import _lib as L, ops
    return L, ops, importlib.import_module('cnn_quantization_amd.qtypes.int_quantizer')


@pytest.fixture(scope='module')
def inputs():
    """{(layout, dtype): tensor} of one set of values, the fp32 statistics of those values, and a statistics class serving them per
    channel (any stat_id) or for the whole tensor (stat_id 'tensor')."""
    v = values(SHAPE, seed=26)
    xs = {('nchw', torch.bfloat16): v.bfloat16().cuda(), ('nhwc', torch.bfloat16): cl(v, torch.bfloat16),
          ('nhwc', torch.float32): cl(v, torch.float32)}
    t = v.transpose(0, 1).reshape(SHAPE[1], -1)
    per_channel = {'min': t.min(1)[0] * 0.8, 'max': t.max(1)[0] * 0.9, 'mean': t.mean(1), 'std': t.std(1),
                   'b': (t - t.mean(1, keepdim=True)).abs().mean(1)}
    whole = {'min': v.min() * 0.8, 'max': v.max() * 0.9, 'mean': v.mean(), 'std': v.std(), 'b': (v - v.mean()).abs().mean(),
             'kld_th': v.abs().max() * 0.6}

    class SM:
        def get_tensor_stat(self, stat_id, name, kind='mean'):
            return (whole if stat_id == 'tensor' else per_channel)[name].numpy()
    return xs, per_channel, whole, SM


def table_of(stat, C, rows=('min', 'max', 'mean', 'std', 'b')):
    L, _, _ = mods()
    table = torch.zeros((L.NSTAT, C), dtype=torch.float32, device='cuda')
    for k in rows:
        table[getattr(L, 'STAT_' + k.upper())] = stat[k]
    return table


def routed(monkeypatch, q, x, **kw):
    """(q(x, **kw), the ops entry points it reached from outside ops, counted upcasts, counted layout copies)."""
    _, ops, iq = mods()
    reached, depth = [], [0]

    def recorder(name, fn):
        def call(*a, **k):
            if not depth[0]:
                reached.append(name)
            depth[0] += 1
            try:
                return fn(*a, **k)
            finally:
                depth[0] -= 1
        return call
    with monkeypatch.context() as m:
        for name in ENTRIES:
            m.setattr(ops, name, recorder(name, getattr(ops, name)))
        fb, copies = iq.HALF_FALLBACKS, ops.LAYOUT_COPIES
        y = q(x, 'act', **kw)
        return y, reached, iq.HALF_FALLBACKS - fb, ops.LAYOUT_COPIES - copies


def check(monkeypatch, q, x, route, entry, direct, **kw):
    att = q._att(kw.get('override_att'))
    assert q._route(q._branch(att, x), x, kw.get('stat_id'), att) == route
    y, reached, upcasts, copies = routed(monkeypatch, q, x, **kw)
    assert reached == [entry] and upcasts == 0 and copies == 0, (route, reached, upcasts, copies)
    assert y.dtype == x.dtype and y.shape == x.shape and y.is_contiguous() == x.is_contiguous(), route
    assert y.is_contiguous(memory_format=torch.channels_last) == x.is_contiguous(memory_format=torch.channels_last), route
    want = direct()
    assert same(y, want[0] if isinstance(want, tuple) else want), route


def aciq_kw(q, clip):
    return dict(positive=False, clip=clip, bit_alloc=q.bit_alloc_act, prior_is_b=q.bit_alloc_prior != 'gaus',
                target=q.bit_alloc_target_act, round_mode=q.bit_alloc_round)


def params(q, table, clip):
    _, ops, _ = mods()
    return ops.pc_params(table, 4, False, clip, bool(q.bit_alloc_act), q.bit_alloc_prior != 'gaus', q.bit_alloc_target_act,
                         q.bit_alloc_round)[0]


@pytest.mark.parametrize('clip, ba', [('laplace', True), ('no', False)])
@pytest.mark.parametrize('key', NHWC, ids=['bf16', 'f32'])
def test_nhwc_bcorr(monkeypatch, inputs, key, clip, ba):
    _, ops, _ = mods()
    xs, per_channel, _, SM = inputs
    q = quantizer(clipping=clip, pcq_act=True, bit_alloc_act=ba)
    q.sm, q.fuse_bcorr = SM, True
    qp = params(q, table_of(per_channel, SHAPE[1]), clip)
    check(monkeypatch, q, xs[key], 'nhwc_bcorr', 'qdq_bias_corrected_nhwc', lambda: ops.qdq_bias_corrected_nhwc(xs[key], qp, True),
          stat_id='layer0')
    assert q.fuse_bcorr is None and q.bcorr_fused


@pytest.mark.parametrize('clip, ba, pending', [('laplace', True, None), ('gaus', False, False), ('no', True, None), ('no', False, True)])
def test_half_table(monkeypatch, inputs, clip, ba, pending):
    _, ops, _ = mods()
    xs, per_channel, _, SM = inputs
    x = xs[HALF[0]]
    q = quantizer(clipping=clip, pcq_act=True, bit_alloc_act=ba)
    q.sm, q.fuse_bcorr = SM, pending
    qp = params(q, table_of(per_channel, SHAPE[1]), clip)
    if pending is None:
        check(monkeypatch, q, x, 'half_table', 'pc_qdq', lambda: ops.pc_qdq(x, 2, 8, 16, qp), stat_id='layer0')
    else:
        check(monkeypatch, q, x, 'half_table', 'qdq_bias_corrected_half', lambda: ops.qdq_bias_corrected_half(x, qp, pending),
              stat_id='layer0')
        assert q.fuse_bcorr is None and q.bcorr_fused


@pytest.mark.parametrize('stat_id', [None, 'layer0'])
@pytest.mark.parametrize('key', NHWC, ids=['bf16', 'f32'])
def test_nhwc_aciq(monkeypatch, inputs, key, stat_id):
    _, ops, _ = mods()
    xs, per_channel, _, SM = inputs
    q = quantizer(clipping='laplace', pcq_act=True, bit_alloc_act=True)
    q.sm = SM
    table = table_of(per_channel, SHAPE[1]) if stat_id else None
    check(monkeypatch, q, xs[key], 'nhwc_aciq', 'aciq_qdq_nhwc',
          lambda: ops.aciq_qdq_nhwc(xs[key], 4, stats=table, **aciq_kw(q, 'laplace')), stat_id=stat_id)


def test_half_aciq(monkeypatch, inputs):
    _, ops, _ = mods()
    x = inputs[0][HALF[0]]
    q = quantizer(clipping='no', pcq_act=True, bit_alloc_act=True)
    q.half_dynamic = True
    check(monkeypatch, q, x, 'half_aciq', 'aciq_qdq_half', lambda: ops.aciq_qdq_half(x, 4, **aciq_kw(q, 'gaus')),
          override_att=('clipping', 'gaus'))


@pytest.mark.parametrize('stat_id', [None, 'tensor'])
@pytest.mark.parametrize('key', HALF + NHWC, ids=['bf16', 'nhwc-bf16', 'nhwc-f32'])
def test_flat_clip(monkeypatch, inputs, key, stat_id):
    _, ops, _ = mods()
    xs, _, whole, SM = inputs
    q = quantizer(clipping='laplace')
    q.sm = SM
    table = table_of(whole, 1) if stat_id else None
    check(monkeypatch, q, xs[key], 'flat_clip', 'clip_qdq_tensor',
          lambda: ops.clip_qdq_tensor(xs[key], 4, positive=False, clip='laplace', stats=table), stat_id=stat_id)


@pytest.mark.parametrize('key', HALF + NHWC, ids=['bf16', 'nhwc-bf16', 'nhwc-f32'])
def test_mid_tread(monkeypatch, inputs, key):
    _, ops, _ = mods()
    x = inputs[0][key]
    q = quantizer(clipping='laplace', mtd_quant=True, bit_alloc_target_act=3)
    check(monkeypatch, q, x, 'flat_midtread', 'mid_tread_qdq_tensor', lambda: ops.mid_tread_qdq_tensor(x, 3, sym=True))
    if key[0] == 'nhwc':
        for me in (False, True):
            q = quantizer(clipping='laplace', mtd_quant=True, bit_alloc_target_act=3, pcq_act=True, measure_entropy=me)
            check(monkeypatch, q, x, 'nhwc_midtread', 'mid_tread_qdq_nhwc',
                  lambda: ops.mid_tread_qdq_nhwc(x, 3, sym=True, want_entropy=me))


def cfg2_kw(q, table=None):
    return dict(positive=False, clip='no', bit_alloc=q.bit_alloc_act, prior_is_b=q.bit_alloc_prior != 'gaus',
                target=q.bit_alloc_target_act, round_mode=q.bit_alloc_round, group=None, stats=table,
                want_entropy=q.measure_entropy, bcorr=None)


@pytest.mark.parametrize('key', HALF + NHWC, ids=['bf16', 'nhwc-bf16', 'nhwc-f32'])
def test_per_channel_min_max(monkeypatch, inputs, key):
    _, ops, _ = mods()
    xs, per_channel, _, SM = inputs
    x = xs[key]
    q = quantizer(pcq_act=True)
    q.sm = SM
    check(monkeypatch, q, x, 'minmax_pc', 'act_qdq_per_channel', lambda: ops.act_qdq_per_channel(x, 4, **cfg2_kw(q)))
    table = table_of(per_channel, SHAPE[1], ('min', 'max'))             # the rows plain min/max asks the statistics for
    check(monkeypatch, q, x, 'half_minmax' if key[0] == 'nchw' else 'minmax_pc', 'act_qdq_per_channel',
          lambda: ops.act_qdq_per_channel(x, 4, **cfg2_kw(q, table)), stat_id='layer0')
    if key[0] == 'nhwc':
        q = quantizer(pcq_act=True, measure_entropy=True)
        check(monkeypatch, q, x, 'nhwc_entropy', 'act_qdq_per_channel', lambda: ops.act_qdq_per_channel(x, 4, **cfg2_kw(q)))


def test_per_tensor_min_max_and_kld(monkeypatch, inputs):
    _, ops, _ = mods()
    from cnn_quantization_amd import int_quantization
    xs, _, whole, SM = inputs
    x1 = values((2, 8, 1, 1), seed=3).bfloat16().cuda()
    for q, x in ((quantizer(pcq_act=True), x1), (quantizer(), xs[HALF[0]])):
        check(monkeypatch, q, x, 'minmax_pt', 'minmax_qdq_per_tensor',
              lambda: ops.minmax_qdq_per_tensor(x, 4, avg_over_batch=False, zero_min=False, int_exp=False, enforce_true_zero=True,
                                                group=None))
    for key in HALF + NHWC[:1]:
        q = quantizer(kld=True, clipping='laplace', pcq_act=True)
        q.sm = SM
        rng, off = (float(v) for v in q.alpha2DeltaOffset(*(whole[k].numpy() for k in ('kld_th', 'max', 'min', 'mean'))))
        check(monkeypatch, q, xs[key], 'kld', 'pt_qdq',
              lambda: int_quantization.float2gemmlowp(xs[key], rng, off, 4, False, rng + off > 0 and off < 0, None), stat_id='tensor')


def test_a_branch_without_a_route_upcasts_once(monkeypatch, inputs):
    xs, _, whole, SM = inputs
    x = xs[HALF[0]]
    w = values((8, 4, 3, 3), seed=5).bfloat16().cuda()
    cases = [('kld', quantizer(kld=True), torch.zeros(2, 12, 4, 4, dtype=torch.bfloat16, device='cuda')[:, 2:10], 'pt_qdq', 'tensor'),
             ('clip', quantizer(clipping='laplace', pcq_act=True, measure_entropy=True), x, 'act_qdq_per_channel', None),
             ('midtread', quantizer(clipping='laplace', mtd_quant=True, pcq_act=True, bit_alloc_target_act=3), x, 'mid_tread_qdq', None),
             ('midtread_w', quantizer(pcq_weights=True, mtd_quant=True, bit_alloc_target_weight=3), w, 'mid_tread_qdq', None),
             ('weights', quantizer(pcq_weights=True), w, 'act_qdq_per_channel', None),
             ('midtread_pc', quantizer(pcq_act=True, mtd_quant=True, bit_alloc_target_act=3), x, 'mid_tread_qdq', None),
             ('pc', quantizer(pcq_act=True, bit_alloc_act=True), x, 'act_qdq_per_channel', None)]
    for branch, q, t, entry, stat_id in cases:
        q.sm = SM
        att = q._att()
        assert q._branch(att, t) == branch and q._route(branch, t, stat_id, att) is None
        y, reached, upcasts, _ = routed(monkeypatch, q, t, stat_id=stat_id)
        assert upcasts == 1 and reached == [entry] and y.dtype == torch.bfloat16 and y.shape == t.shape, (branch, reached, upcasts)
