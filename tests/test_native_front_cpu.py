"""The host front of the native storage forms, the part that needs no GPU: every `_*_native` function asks
its C route function once per class of layer and again once its cache is emptied by name, and `_ws_bytes` hands on what the C
workspace function says, rounded up to 16, or raises the library's refusal."""
import pytest
import torch

from cnn_quantization_amd import _lib as L, ops

BF16, F32 = torch.bfloat16, torch.float32
# (the ops function, its arguments, the cache it keeps, the C route function, the words of its report, the word it casts, the cast)
ROUTES = [
    ('_nhwc_native', ('hist', 32, 8, F32), '_NHWC_NATIVE', 'cnnq_pc_route_qdq_hist_nhwc', 4, 3, bool),
    ('_nhwc_native', ('midtread', 32, 8, BF16), '_NHWC_NATIVE', 'cnnq_pc_route_midtread_nhwc', 6, 5, bool),
    ('_nhwc_native', ('stats', 32, 8, F32), '_STATS_NHWC_NATIVE', 'cnnq_pc_route_stats_nhwc', 4, 3, bool),
    ('_stats_nhwc_native', (98, 12, BF16), '_STATS_NHWC_NATIVE', 'cnnq_pc_route_stats_nhwc', 4, 3, bool),
    ('_stats_half_native', (2, 8, 16, BF16), '_STATS_HALF_NATIVE', 'cnnq_pc_route_stats_dt', 4, 3, bool),
    ('_aciq_half_native', (2, 8, 16, BF16, True, False), '_ACIQ_HALF_NATIVE', 'cnnq_pc_route_aciq_dt', 4, 3, int),
    ('_aciq_half_native', (8, 64, 784, torch.float16), '_ACIQ_HALF_NATIVE', 'cnnq_pc_route_aciq_dt', 4, 3, int),
    ('_table_half_native', (2, 8, 16, BF16), '_TABLE_HALF_NATIVE', 'cnnq_pc_route_qdq_bcorr_dt', 4, 3, int),
    ('_midtread_half_native', (2, 8, 16, BF16, True), '_MIDTREAD_HALF_NATIVE', 'cnnq_pc_route_midtread_dt', 4, 3, int),
    ('_entropy_half_native', (2, 8, 16, BF16, 16), '_ENTROPY_HALF_NATIVE', 'cnnq_pc_route_qdq_hist_dt', 4, 3, int),
]


@pytest.mark.parametrize('name, args, cache, fn, words, word, cast', ROUTES, ids=['%s-%s' % (r[0], r[3]) for r in ROUTES])
def test_a_class_of_layer_asks_its_route_function_once(monkeypatch, name, args, cache, fn, words, word, cast):
    lib = L.load()
    reports = []

    def counted(*a, _real=getattr(lib, fn)):
        rc = _real(*a)
        reports.append(list(a[-1]))
        return rc
    monkeypatch.setattr(lib, fn, counted)
    monkeypatch.setattr(ops, cache, {})                     # every class is new
    ask = getattr(ops, name)
    v = ask(*args)
    assert len(reports) == 1 and len(reports[0]) == words
    assert type(v) is cast and v == cast(reports[0][word])
    assert ask(*args) == v and len(reports) == 1            # the second call of the class is answered from the cache
    assert getattr(ops, cache)
    getattr(ops, cache).clear()                             # emptied by name, as the tests and tools do
    assert ask(*args) == v and len(reports) == 2


WS = [      # (kind, the C function, (N, C, HW, arg) as _ws_bytes takes them, the C function's own arguments)
    ('nhwc', 'cnnq_pc_nhwc_workspace', (75, 12, 1, 1), (75, 12, 1)),
    ('aciq_nhwc', 'cnnq_pc_aciq_nhwc_workspace', (75, 12, 1, 0), (75, 12, 0)),
    ('bcorr_nhwc', 'cnnq_pc_qdq_bcorr_nhwc_workspace', (32, 7, 1, 2), (32, 7, 2)),
    ('stats_nhwc', 'cnnq_pc_stats_nhwc_workspace', (32, 8, 1, 1), (32, 8, 1)),
    ('rows', 'cnnq_rows_stats_workspace', (5, 1000, 1, 0), (5, 1000, 0)),
    ('pt_clip', 'cnnq_pt_clip_workspace', (4096, 1, 1, 1), (4096, 1)),
    ('aciq', 'cnnq_pc_aciq_workspace', (3, 10, 196, 1), (3, 10, 196, 1)),
    ('stats', 'cnnq_pc_stats_workspace', (3, 10, 196, 0), (3, 10, 196, 0)),
    ('cfg2', 'cnnq_pc_minmax_qdq_workspace', (3, 10, 196, 0), (3, 10, 196)),
    ('stats_half', 'cnnq_pc_stats_dt_workspace', (3, 12, 25, 1), (3, 12, 25, 1)),
    ('bcorr_half', 'cnnq_pc_qdq_bcorr_dt_workspace', (2, 7, 16, 2), (2, 7, 16, 2)),
    ('aciq_half', 'cnnq_pc_aciq_dt_workspace', (2, 8, 16, 1), (2, 8, 16, 1)),
    ('midtread_half', 'cnnq_pc_midtread_dt_workspace', (8, 64, 784, 2), (8, 64, 784, 2)),
]


@pytest.mark.parametrize('kind, fn, args, c_args', WS, ids=[w[0] for w in WS])
def test_ws_bytes_is_the_c_functions_answer_rounded_up_to_16(monkeypatch, kind, fn, args, c_args):
    monkeypatch.setattr(ops, '_WS_BYTES', {})
    asked = []

    def counted(*a, _real=getattr(L.load(), fn)):
        asked.append(a)
        return _real(*a)
    monkeypatch.setattr(L.load(), fn, counted)
    want = getattr(L.load(), fn)(*c_args)
    assert want > 0
    assert ops._ws_bytes(kind, *args) == (want + 15) // 16 * 16
    assert ops._ws_bytes(kind, *args) == (want + 15) // 16 * 16
    assert asked == [c_args, c_args]                        # the test's own question, then one for both calls


@pytest.mark.parametrize('kind, args, message', [
    ('aciq_nhwc', (0, 8, 1, 1), r'cnnq_pc_aciq_nhwc_workspace\(0, 8, 1\): bad arguments'),
    ('stats_nhwc', (32, 8, 1, 3), r'cnnq_pc_stats_nhwc_workspace\(32, 8, 3\): bad arguments'),
    ('rows', (0, 1000, 1, 0), r'cnnq_rows_stats_workspace\(0, 1000, 0\): bad arguments'),
    ('pt_clip', (0, 1, 1, 0), r'cnnq_pt_clip_workspace\(0, 0\): bad arguments'),
    ('aciq_half', (0, 8, 16, 1), r'cnnq_pc_aciq_dt_workspace\(0,8,16,1\) failed: CNNQ_EINVAL'),
    ('stats_half', (2, 1 << 16, 1 << 15, 1), r'cnnq_pc_stats_dt_workspace\(2,65536,32768,1\) failed: CNNQ_ERANGE'),
    ('bcorr_half', (1 << 31, 2, 4, 2), r'cnnq_pc_qdq_bcorr_dt_workspace\(2147483648,2,4,2\) failed: CNNQ_ERANGE'),
    ('midtread_half', (2, 0, 16, 1), r'cnnq_pc_midtread_dt_workspace\(2,0,16,1\) failed: CNNQ_EINVAL'),
    ('cfg2', (0, 8, 16, 0), r'cnnq_pc_groups\(0,8,16\) failed: CNNQ_EINVAL'),
    ('stats', (2, 1 << 16, 1 << 15, 1), r'cnnq_pc_groups\(2,65536,32768\) failed: CNNQ_ERANGE'),
])
def test_ws_bytes_raises_for_a_geometry_without_a_plan(monkeypatch, kind, args, message):
    monkeypatch.setattr(ops, '_WS_BYTES', {})
    with pytest.raises(L.CnnqError, match=message):
        ops._ws_bytes(kind, *args)
    assert not ops._WS_BYTES                                # a refusal is not cached
