"""The host front the channels_last entry points share: where a call's tables live does not change its
bits, the statistics front is one function whatever its flags, and every family asks its route function once per class of layer.
The tensors are [2, C, 4, 4]-sized: the host layer is what is under test.  (The bias correction's hot form against its
want_parts form is compared in tests/test_channels_last_bcorr_gpu.py's `check`.)"""
import pytest
import torch

from test_channels_last_gpu import cl, same, values

pytestmark = pytest.mark.gpu
DTYPES, IDS = [torch.float32, torch.bfloat16], ['f32', 'bf16']


def mods():
    from cnn_quantization_amd import _lib as L, ops
    return L, ops


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
@pytest.mark.parametrize('C', [8, 7])           # a full piece; piece width 1
def test_tables_kept_or_behind_the_workspace_same_bits(dtype, C):
    L, ops = mods()
    x = cl(values((2, C, 4, 4), seed=3), dtype)
    before = ops.LAYOUT_COPIES
    for ba in (False, True):
        y_kept, parts = ops.aciq_qdq_nhwc(x, 4, bit_alloc=ba, want_parts=True)
        assert set(parts) == {'stats', 'qp', 'diag'}
        assert [tuple(parts[k].shape) for k in ('stats', 'qp', 'diag')] == [(L.NSTAT, C), (L.NQP, C), (L.NDIAG, C)]
        assert same(ops.aciq_qdq_nhwc(x, 4, bit_alloc=ba), y_kept)
    for sym in (True, False):
        y_kept, ent, parts = ops.mid_tread_qdq_nhwc(x, 4., sym, want_parts=True)
        assert ent is None and parts['hist'] is None
        assert tuple(parts['stats'].shape) == (L.NSTAT, C) and tuple(parts['mt'].shape) == (L.NMT, C)
        y, ent = ops.mid_tread_qdq_nhwc(x, 4., sym)
        assert ent is None and same(y, y_kept)
    assert ops.LAYOUT_COPIES == before


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_collect_and_config3_share_the_statistics_front(dtype):
    """Without need_kurt and need_relu, pc_stats_nhwc is config 3's front: the same launches, the same table bits.  Both entry
    points run one function now, so this pins only that they keep doing so (the flags, the workspace, the caller's `mom`); that the
    front computes the right table is the business of the parity tests against pc_stats (test_channels_last_collect_gpu.py) and
    against fp64 (test_channels_last_aciq_gpu.py)."""
    L, ops = mods()
    x = cl(values((3, 12, 5, 5), seed=5), dtype)            # R = 75 rows, ragged against the slab
    stats, _ = ops.pc_stats_nhwc(x, need_b=True)
    _, parts = ops.aciq_qdq_nhwc(x, 4, clip='laplace', want_parts=True)
    assert same(stats, parts['stats'])
    assert stats[L.STAT_B].any() and not stats[L.STAT_KURT].any() and not stats[L.STAT_STD_POS].any()


def test_every_family_asks_its_route_function_once(monkeypatch):
    L, ops = mods()
    lib = L.load()
    asked = []
    for fn, _, _, _ in ops._NHWC_ROUTES.values():
        def counted(*a, _fn=fn, _real=getattr(lib, fn)):
            asked.append(_fn)
            return _real(*a)
        monkeypatch.setattr(lib, fn, counted)
    monkeypatch.setattr(ops, '_NHWC_NATIVE', {})            # every shape is new
    monkeypatch.setattr(ops, '_STATS_NHWC_NATIVE', {})      # ('stats' keeps its cache under the name the collect tests use)
    x = cl(values((2, 8, 4, 4), seed=7), torch.float32)
    qp, _ = ops.pc_params(ops.pc_stats_nhwc(x, need_b=True)[0], 4, clip='laplace')
    calls = (lambda: ops.pc_stats_nhwc(x), lambda: ops.act_qdq_per_channel(x, 4, want_entropy=True),
             lambda: ops.aciq_qdq_nhwc(x, 4, want_entropy=True), lambda: ops.mid_tread_qdq_nhwc(x, 4., True),
             lambda: ops.act_qdq_per_channel(x, 4), lambda: ops.aciq_qdq_nhwc(x, 4), lambda: ops.qdq_bias_corrected_nhwc(x, qp, True))
    for f in calls:
        f()
    assert sorted(asked) == sorted(fn for fn, _, _, _ in ops._NHWC_ROUTES.values())
    assert sorted(ops._NHWC_NATIVE) == [('hist', 32, 8, torch.float32), ('midtread', 32, 8, torch.float32)]
    assert list(ops._STATS_NHWC_NATIVE) == [(32, 8, torch.float32)]
    for f in calls:
        f()
    assert len(asked) == len(ops._NHWC_ROUTES)


def test_tables_and_dtypes_are_refused_by_the_shared_checks():
    """The errors DESIGN.md section 20 lists: a table that is no contiguous float32 device tensor of the right shape on x's
    device is refused before the C call reads through its pointer, and a float64 tensor gets the dtype message."""
    L, ops = mods()
    x = cl(values((2, 8, 4, 4), seed=9), torch.float32)
    stats, _ = ops.pc_stats_nhwc(x, need_b=True)
    qp, _ = ops.pc_params(stats, 4, clip='laplace')
    for bad in (None, qp.cpu(), qp.double(), qp[:, :7], qp.t().contiguous().t()):
        with pytest.raises(L.CnnqError, match='qp must be a contiguous float32'):
            ops.qdq_bias_corrected_nhwc(x, bad, True)
    for bad in (stats.cpu(), stats.double(), stats[:, :7]):
        with pytest.raises(L.CnnqError, match='stats must be a contiguous float32'):
            ops.mid_tread_qdq_nhwc(x, 4., True, stats=bad)
    with pytest.raises(L.CnnqError, match='x must be float32 or bfloat16 or float16'):
        ops.mid_tread_qdq_nhwc(cl(values((2, 8, 4, 4)), torch.float64), 4., True)
