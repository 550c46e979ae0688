"""The host front the native entry points of both storage forms share - dense channels_last (*_nhwc) and
contiguous bf16 / fp16 (*_half): where a call's tables live does not change its bits, both layouts of an operation make the same
sequence of C calls up to the suffix of their names, and the shared checks refuse bad tables and dtypes.  The tensors are
[2, C, 4, 4]-sized: the host layer is what is under test.  (The channels_last cases of the first and the last of these, and the
ask-once test of the channels_last route functions, are tests/test_channels_last_front_gpu.py's.)"""
import pytest
import torch

from test_channels_last_gpu import cl, same, values

pytestmark = pytest.mark.gpu
LAYOUTS = [('nhwc', torch.float32), ('nhwc', torch.bfloat16), ('half', torch.bfloat16), ('half', torch.float16)]
LIDS = ['nhwc-f32', 'nhwc-bf16', 'half-bf16', 'half-f16']
HALVES, HIDS = [torch.bfloat16, torch.float16], ['bf16', 'f16']
SUFFIX = {'nhwc': '_nhwc', 'half': '_dt'}


def mods():
    from cnn_quantization_amd import _lib as L, ops
    return L, ops


def act(layout, dtype, shape, seed):
    x = values(shape, seed=seed)
    return cl(x, dtype) if layout == 'nhwc' else x.to(dtype).cuda().contiguous()


@pytest.mark.parametrize('single_launch', [0, 2], ids=['chain', 'resident'])    # N*HW = 32 fits the resident form: both routes run
@pytest.mark.parametrize('dtype', HALVES, ids=HIDS)
@pytest.mark.parametrize('C', [8, 7])
def test_tables_kept_or_behind_the_workspace_same_bits_half(dtype, C, single_launch):
    L, ops = mods()
    x = act('half', dtype, (2, C, 4, 4), 3)
    for ba in (False, True):
        y_kept, parts = ops.aciq_qdq_half(x, 4, bit_alloc=ba, want_parts=True, single_launch=single_launch)
        assert set(parts) == {'stats', 'qp', 'diag'}
        assert [tuple(parts[k].shape) for k in ('stats', 'qp', 'diag')] == [(L.NSTAT, C), (L.NQP, C), (L.NDIAG, C)]
        assert same(ops.aciq_qdq_half(x, 4, bit_alloc=ba, single_launch=single_launch), y_kept)
    for sym in (True, False):
        y_kept, ent, parts = ops.mid_tread_qdq_half(x, 4., sym, want_parts=True, single_launch=single_launch)
        assert ent is None and parts['hist'] is None
        assert tuple(parts['stats'].shape) == (L.NSTAT, C) and tuple(parts['mt'].shape) == (L.NMT, C)
        y, ent = ops.mid_tread_qdq_half(x, 4., sym, single_launch=single_launch)
        assert ent is None and same(y, y_kept)


@pytest.mark.parametrize('layout, dtype', LAYOUTS, ids=LIDS)
@pytest.mark.parametrize('C', [8, 7])
def test_bias_correction_tables_kept_or_behind_the_workspace_same_bits(layout, dtype, C):
    L, ops = mods()
    x = act(layout, dtype, (2, C, 4, 4), 4)
    stats, _ = getattr(ops, 'pc_stats_' + layout)(x, need_b=True)
    qp, _ = ops.pc_params(stats, 4, clip='laplace')
    bcorr = getattr(ops, 'qdq_bias_corrected_' + layout)
    for kw in ([{}] if layout == 'nhwc' else [dict(single_launch=False), dict(single_launch=True)]):
        y_kept, parts = bcorr(x, qp, True, want_parts=True, **kw)
        assert set(parts) == {'sums', 'bias'} and tuple(parts['sums'].shape) == (3, C) and tuple(parts['bias'].shape) == (C,)
        assert same(bcorr(x, qp, True, **kw), y_kept)


@pytest.mark.parametrize('dtype', HALVES, ids=HIDS)
def test_collect_and_config3_share_the_statistics_front_half(dtype):
    """As test_channels_last_front_gpu.py's: without need_kurt and need_relu, pc_stats_half is the front of config 3's chain."""
    L, ops = mods()
    x = act('half', dtype, (3, 12, 5, 5), 5)                # HW = 25: piece width 1, the chain whatever is allowed
    stats, _ = ops.pc_stats_half(x, need_b=True)
    _, parts = ops.aciq_qdq_half(x, 4, clip='laplace', want_parts=True, single_launch=0)
    assert same(stats, parts['stats'])
    assert stats[L.STAT_B].any() and not stats[L.STAT_KURT].any() and not stats[L.STAT_STD_POS].any()


# What every entry point launches: the C calls of one invocation in order, `*` for the layout's suffix (_nhwc / _dt); written out
# by hand from the entry points.  Workspace-size, route and other cached queries are left out.
ENT, MT_ENT = 'cnnq_entropy_replicas', 'cnnq_midtread_entropy'
CALLS = {   # (entry point, stats given, want_entropy): C calls (want_parts never changes them)
    ('pc_stats', False, False): ['cnnq_pc_stats*'],
    ('aciq_qdq', False, False): ['cnnq_pc_aciq_qdq*'],
    ('aciq_qdq', False, True): ['cnnq_pc_aciq_qdq_hist*', ENT],
    ('aciq_qdq', True, False): ['cnnq_pc_params', 'cnnq_pc_qdq*'],
    ('aciq_qdq', True, True): ['cnnq_pc_params', 'cnnq_pc_qdq_hist*', ENT],
    ('qdq_bias_corrected', True, False): ['cnnq_pc_qdq_bcorr*'],
    ('mid_tread_qdq', False, False): ['cnnq_pc_midtread*'],
    ('mid_tread_qdq', False, True): ['cnnq_pc_midtread*', MT_ENT],
    ('mid_tread_qdq', True, False): ['cnnq_pc_midtread_params', 'cnnq_pc_midtread_qdq*'],
    ('mid_tread_qdq', True, True): ['cnnq_pc_midtread_params', 'cnnq_pc_midtread_qdq*', MT_ENT],
    ('act_qdq_per_channel', True, False): ['cnnq_pc_params', 'cnnq_pc_qdq*'],
    ('act_qdq_per_channel', True, True): ['cnnq_pc_params', 'cnnq_pc_qdq_hist*', ENT],
}


def cached_query(name):
    return (name.endswith('_workspace') or name.startswith('cnnq_pc_route_')
            or name in ('cnnq_pc_groups', 'cnnq_hist_replica_bytes', 'cnnq_version'))


@pytest.mark.parametrize('layout, dtype', LAYOUTS, ids=LIDS)
def test_both_layouts_make_the_same_c_calls_up_to_the_suffix(monkeypatch, layout, dtype):
    L, ops = mods()
    lib = L.load()
    x = act(layout, dtype, (2, 8, 4, 4), 7)
    table, _ = getattr(ops, 'pc_stats_' + layout)(x, need_b=True)
    qp, _ = ops.pc_params(table, 4, clip='laplace')
    made = []
    for name in L.SIGNATURES:
        if name.startswith('cnnq_') and not cached_query(name):
            def recorded(*a, _name=name, _real=getattr(lib, name)):
                made.append(_name)
                return _real(*a)
            monkeypatch.setattr(lib, name, recorded)
    before = ops.LAYOUT_COPIES
    for (entry, given, want_entropy), want in CALLS.items():
        fn = ops.act_qdq_per_channel if entry == 'act_qdq_per_channel' else getattr(ops, '%s_%s' % (entry, layout))
        for want_parts in (False, True):
            kw = {}
            if entry == 'pc_stats':
                args, n = (x, True), 2
            elif entry == 'qdq_bias_corrected':
                args, kw, n = (x, qp, True), dict(want_parts=want_parts), 1 + want_parts
            elif entry == 'mid_tread_qdq':
                kw = dict(want_entropy=want_entropy, stats=table if given else None, want_parts=want_parts)
                args, n = (x, 4., True), 2 + want_parts
            elif entry == 'aciq_qdq':
                kw = dict(want_entropy=want_entropy, stats=table if given else None, want_parts=want_parts)
                args, n = (x, 4), 1 + want_entropy + want_parts
            elif want_parts:
                continue                                    # (config 2 from a table keeps no parts on these storage forms)
            else:
                args, kw, n = (x, 4), dict(stats=table, want_entropy=want_entropy), 1 + want_entropy
            del made[:]
            res = fn(*args, **kw)
            assert (len(res) if isinstance(res, tuple) else 1) == n, (entry, given, want_entropy, want_parts)
            assert made == [c.replace('*', SUFFIX[layout]) for c in want], (entry, given, want_entropy, want_parts)
    assert ops.LAYOUT_COPIES == before


def test_tables_and_dtypes_are_refused_by_the_shared_checks_half():
    """test_channels_last_front_gpu.py's, for the contiguous bf16 / fp16 entry points."""
    L, ops = mods()
    x = act('half', torch.bfloat16, (2, 8, 4, 4), 9)
    stats, _ = ops.pc_stats_half(x, need_b=True)
    qp, _ = ops.pc_params(stats, 4, clip='laplace')
    for bad in (None, qp.cpu(), qp.double(), qp[:, :7], qp.t().contiguous().t()):
        with pytest.raises(L.CnnqError, match='qp must be a contiguous float32'):
            ops.qdq_bias_corrected_half(x, bad, True)
    for bad in (stats.cpu(), stats.double(), stats[:, :7]):
        with pytest.raises(L.CnnqError, match='stats must be a contiguous float32'):
            ops.mid_tread_qdq_half(x, 4., True, stats=bad)
        with pytest.raises(L.CnnqError, match='stats must be a contiguous float32'):
            ops.aciq_qdq_half(x, 4, stats=bad)
    for f in (lambda t: ops.mid_tread_qdq_half(t, 4., True), lambda t: ops.aciq_qdq_half(t, 4), ops.pc_stats_half):
        with pytest.raises(L.CnnqError, match='x must be bfloat16 or float16'):
            f(x.double())


def test_config3_refuses_a_bad_statistics_table_on_channels_last():
    """aciq_qdq_nhwc's `stats` gets the check its three siblings have where the tensor runs native; a tensor on the copy route
    hands its `stats` to act_qdq_per_channel as before."""
    L, ops = mods()
    x = cl(values((2, 8, 4, 4), seed=9), torch.float32)
    stats, _ = ops.pc_stats_nhwc(x, need_b=True)
    for bad in (stats.cpu(), stats.double(), stats[:, :7]):
        with pytest.raises(L.CnnqError, match='stats must be a contiguous float32'):
            ops.aciq_qdq_nhwc(x, 4, stats=bad)
    assert same(ops.aciq_qdq_nhwc(x.contiguous(), 4, stats=stats), ops.act_qdq_per_channel(x.contiguous(), 4, clip='laplace', stats=stats))
