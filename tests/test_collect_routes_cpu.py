"""The `-sm collect` route decision against the truth table recorded before the decision was gathered in one
function per manager (tests/golden/collect_routes.npz, written by tests/golden/make_golden_collect_routes.py): at every point of the
recorded grid the three predicates answer, and _route hands the tensor over, bit for bit as recorded; the managers' collect_route agrees
with the three views; MeasureStatistics.save_measure chooses as recorded; and _route decides once.  Nothing is launched."""
import importlib.util
import os
import types

import numpy as np
import torch

from _quantizer import act, nhwc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
spec = importlib.util.spec_from_file_location('make_golden_collect_routes', os.path.join(GOLDEN, 'make_golden_collect_routes.py'))
G = importlib.util.module_from_spec(spec)
spec.loader.exec_module(G)


def test_predicates_and_route_answer_as_recorded_and_the_route_function_agrees_with_its_views():
    from cnn_quantization_amd import ops
    gold = np.load(os.path.join(GOLDEN, 'collect_routes.npz'))
    want_pred, want_routed = gold['predicates'].tolist(), gold['routed'].tolist()
    n, names = 0, set()
    for manager, force, x, what in G.points():
        assert n < len(want_pred), 'more points than recorded'
        pred, routed = G.predicates(manager, force, x), G.routed(manager, force, x)
        assert pred == want_pred[n] and routed == want_routed[n], (n, what, pred, want_pred[n], routed, want_routed[n])
        n += 1
        # the route function against its views: the views of the manager's own module name the route, the others are False or
        # ask an attribute this manager does not have
        route = manager.collect_route(x, force)
        names.add((what[0], route))
        if what[0] == 'pc':
            assert route == ('nhwc' if pred[0] == 1 else 'half' if pred[1] == 1 else None) and pred[0] + pred[1] < 2, (what, route, pred)
        else:
            assert route == ('flat' if pred[2] == 1 else None), (what, route, pred)
        # _route hands over directly exactly when there is a route, and then the tensor as it is
        assert (routed[0] == G.DIRECT) == (route is not None), (what, route, routed)
        if route is not None:
            assert routed[:3] == [G.DIRECT] + G.arrival(ops, x), (what, routed)
    assert n == len(want_pred)
    assert names == {('pc', 'nhwc'), ('pc', 'half'), ('pc', None), ('pt', 'flat'), ('pt', None)}


def test_save_measure_chooses_as_recorded():
    want = np.load(os.path.join(GOLDEN, 'collect_routes.npz'))['measured'].tolist()
    got = [(G.measured(x), what) for x, what in G.measure_points()]
    assert len(got) == len(want)
    for (m, what), w in zip(got, want):
        assert m == w, (what, m, w)


def test_route_decides_once_and_keeps_nothing_on_the_manager(monkeypatch):
    """The storage class, the group and the route function are asked once per layer output: _route passes what it learned on."""
    from cnn_quantization_amd import _lib as L, distributed as D, ops
    from cnn_quantization_amd.inference import inference_quantization_manager as iqm
    from cnn_quantization_amd.inference import statistic_manager as sm, statistic_manager_perchannel as smpc
    from cnn_quantization_amd.utils.misc import Singleton
    asked = {'nhwc': 0, 'half': 0, 'group': 0}
    table = torch.zeros(L.NSTAT, 8)

    def count(key, answer):
        def fn(*a, **kw):
            asked[key] += 1
            return answer
        return fn
    monkeypatch.setattr(ops, '_stats_nhwc_native', count('nhwc', True))
    monkeypatch.setattr(ops, '_stats_half_native', count('half', True))
    monkeypatch.setattr(D, 'forced_exchange', count('group', False))
    for name in ('pc_stats_nhwc', 'pc_stats_half'):
        monkeypatch.setattr(ops, name, lambda x, **kw: (table, None))
    monkeypatch.setattr(ops, 'tensor_stats', lambda x, rows: (torch.ones(L.NSTAT, 1), torch.ones(L.NMOM, 1, dtype=torch.float64)))
    monkeypatch.setenv('HOME', '/nonexistent')
    try:
        for cls, x, want in ((smpc.StatisticManagerPerChannel, nhwc(), dict(nhwc=1, half=0, group=1)),
                             (smpc.StatisticManagerPerChannel, act(), dict(nhwc=0, half=1, group=1)),
                             (sm.StatisticManager, nhwc(), dict(nhwc=0, half=0, group=1)),
                             (sm.StatisticManager, act(), dict(nhwc=0, half=0, group=1))):
            Singleton.reset()
            manager = cls('t', load_stats=False)
            before = {k: v for k, v in vars(manager).items() if k != 'stats' and k != 'metadata'}
            qm = types.SimpleNamespace(enabled=True, stats_mode=iqm.StatsMode.collect_stats, stats_manager=manager)
            monkeypatch.setattr(iqm, 'QMI', lambda: qm)
            asked.update(nhwc=0, half=0, group=0)
            assert iqm._route(None, x, 'conv0_activation', 'activation') is x
            assert asked == want, (cls.__name__, asked)
            assert list(manager.stats) == ['conv0_activation']
            assert {k: v for k, v in vars(manager).items() if k != 'stats' and k != 'metadata'} == before
    finally:
        Singleton.reset()
