"""Records the truth table of the `-sm collect` route decision in tests/golden/collect_routes.npz: at every point of the grid below, the
answers of the three routing predicates (collects_native_nhwc, collects_native_half, collects_native_flat; an exception is recorded as
a code) and what inference_quantization_manager._route does with the tensor in collect mode - whether save_tensor_stats is handed the
tensor directly or through upcast_fallback, the dtype and layout it arrives in and the keywords that come with it.  A second, small
table holds MeasureStatistics.save_measure's choice.  Nothing is launched: the tensors are CPU tensors that say they are on the device,
save_tensor_stats and ops.row_sumsq are recorders, and upcast_fallback records and then calls through.

    python tests/golden/make_golden_collect_routes.py        (re)writes collect_routes.npz from the code as it is

tests/test_collect_routes_cpu.py imports this module and replays the same points on the code under test."""
import contextlib
import itertools
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]

from make_golden_routes import grid_tensors, patched, variety_tensors     # noqa: E402

PREDICATES = ('collects_native_nhwc', 'collects_native_half', 'collects_native_flat')
DTYPES = (torch.float32, torch.bfloat16, torch.float16, torch.float64)
LAYOUTS = ('nchw', 'nhwc', 'copy')
ERRORS = (AttributeError, TypeError, IndexError, RuntimeError)     # answer 2 + index; anything else: 2 + len(ERRORS)
NONE, DIRECT, UPCAST, RAISED = range(4)
BOOLS = (False, True)
ERR = dict(num_bits=4, positive=False, bit_alloc=False, prior_is_b=False, target=None, round_mode=True)


def tensors():
    return grid_tensors() + variety_tensors()


def error_code(e):
    return 2 + next((i for i, c in enumerate(ERRORS) if type(e) is c), len(ERRORS))


def code(fn, *a):
    """0 / 1: fn(*a) as a boolean; 2 and up: the exception it raised."""
    try:
        return int(bool(fn(*a)))
    except Exception as e:      # noqa: BLE001 - the exception's class is the answer
        return error_code(e)


@contextlib.contextmanager
def temporary_home():
    old = os.environ.get('HOME')
    with tempfile.TemporaryDirectory() as home:
        os.environ['HOME'] = home
        try:
            yield
        finally:
            if old is None:
                del os.environ['HOME']
            else:
                os.environ['HOME'] = old


def arrival(ops, t):
    return [DTYPES.index(t.dtype), LAYOUTS.index(ops._layout(t))]


def managers():
    """Yields (kind, manager, force_global_min_max) over the managers' settings: 'pc' the per-channel manager, 'pt' the per-tensor one
    (with kld_threshold); a fresh Singleton each."""
    from cnn_quantization_amd.inference import statistic_manager as sm, statistic_manager_perchannel as smpc
    from cnn_quantization_amd.utils.misc import Singleton
    for collect_err, batch_avg, force in itertools.product(BOOLS, repeat=3):
        Singleton.reset()
        yield 'pc', smpc.StatisticManagerPerChannel('g', load_stats=False, batch_avg=batch_avg, collect_err=collect_err,
                                                    err_settings=dict(ERR)), force
        for kld in BOOLS:
            Singleton.reset()
            yield 'pt', sm.StatisticManager('g', load_stats=False, batch_avg=batch_avg, collect_err=collect_err,
                                            kld_threshold=kld), force
    Singleton.reset()


def points():
    """Yields (manager, force, tensor, description) in a fixed order; the patches of a point are in effect while it is consumed."""
    from cnn_quantization_amd import distributed as D, ops
    xs = tensors()
    with temporary_home():
        for kind, manager, force in managers():
            for world, forced, nhwc_on, nhwc_fn, half_fn in itertools.product((1, 2), BOOLS, (True, False), BOOLS, BOOLS):
                with contextlib.ExitStack() as s:
                    s.enter_context(patched(D, 'world_size', lambda group=None, world=world: world))
                    s.enter_context(patched(D, 'forced_exchange', lambda forced=forced: forced))
                    s.enter_context(patched(ops, '_NHWC', nhwc_on))
                    s.enter_context(patched(ops, '_stats_nhwc_native', lambda R, C, dtype, a=nhwc_fn: a))
                    s.enter_context(patched(ops, '_stats_half_native', lambda N, C, HW, dtype, a=half_fn: a))
                    for i, x in enumerate(xs):
                        yield manager, force, x, (kind, dict(collect_err=manager.collect_err, batch_avg=manager.batch_avg, force=force,
                                                             kld=getattr(manager, 'kld_threshold', None), world=world,
                                                             forced_exchange=forced, nhwc=nhwc_on, nhwc_fn=nhwc_fn, half_fn=half_fn), i,
                                                  tuple(x.shape), x.dtype, x.stride(), x.is_cuda)


def predicates(manager, force, x):
    from cnn_quantization_amd.inference import statistic_manager as sm, statistic_manager_perchannel as smpc
    return [code(smpc.collects_native_nhwc, manager, x, force), code(smpc.collects_native_half, manager, x, force),
            code(sm.collects_native_flat, manager, x)]


def routed(manager, force, x):
    """[how, dtype, layout, keywords, calls] of x through _route in collect mode: how - DIRECT, UPCAST or RAISED (then the rest is the
    exception's code and zeros); dtype and layout of the tensor save_tensor_stats receives; keywords - bit 0 force_global_min_max, bit 1
    half_range given, bit 2 err_settings given; calls - how often save_tensor_stats ran."""
    from cnn_quantization_amd import ops
    from cnn_quantization_amd.inference import inference_quantization_manager as iqm
    seen, through = [], []

    def save_tensor_stats(tensor, tag, id, tensors_q={}, force_global_min_max=False, **kw):
        assert (tag, id) == ('name', 'conv0_activation') and not tensors_q
        seen.append(arrival(ops, tensor) + [int(bool(force_global_min_max)) | 2 * ('half_range' in kw) | 4 * ('err_settings' in kw)])

    def fallback(fn, *a, **kw):
        assert fn.__name__ == 'save_tensor_stats'
        through.append(1)
        return real(fn, *a, **kw)
    real = iqm.upcast_fallback
    qm = types.SimpleNamespace(enabled=True, stats_mode=iqm.StatsMode.collect_stats, stats_manager=manager,
                               err_settings=lambda out_id, tag, half_range: dict(ERR))
    manager.save_tensor_stats = save_tensor_stats
    try:
        with patched(iqm, 'QMI', lambda: qm), patched(iqm, 'upcast_fallback', fallback):
            try:
                out = iqm._route(None, x, 'conv0_activation', 'activation', collect_tag='name', force_global=force)
            except Exception as e:      # noqa: BLE001
                return [RAISED, error_code(e), 0, 0, len(seen)]
        assert out is x and len(through) <= 1
        return ([UPCAST if through else DIRECT] + seen[0] if seen else [NONE, 0, 0, 0]) + [len(seen)]
    finally:
        del manager.save_tensor_stats


def measured(x):
    """[how, dtype, layout, rows] of x through MeasureStatistics.save_measure, as routed()."""
    from cnn_quantization_amd import ops
    from cnn_quantization_amd.inference import inference_quantization_manager as iqm
    seen, through = [], []

    def row_sumsq(t, rows=None):
        seen.append(arrival(ops, t) + [int(rows)])
        return torch.zeros(int(rows))

    def fallback(fn, *a, **kw):
        assert fn is row_sumsq and kw == dict(cast_back=False)
        through.append(1)
        return real(fn, *a, **kw)
    real = iqm.upcast_fallback
    ms = iqm.MeasureStatistics('g')
    with patched(ops, 'row_sumsq', row_sumsq), patched(iqm, 'upcast_fallback', fallback):
        try:
            ms.save_measure(x, 'l')
        except Exception as e:      # noqa: BLE001
            return [RAISED, error_code(e), 0, 0]
    assert len(seen) == 1 and list(ms.stats) == ['l']
    return [UPCAST if through else DIRECT] + seen[0]


def measure_points():
    from cnn_quantization_amd import ops
    for nhwc_on in (True, False):
        with temporary_home(), patched(ops, '_NHWC', nhwc_on):
            for i, x in enumerate(tensors()):
                yield x, (nhwc_on, i, tuple(x.shape), x.dtype, x.stride(), x.is_cuda)


def record():
    """{'predicates': int8 [points, 3], 'routed': int8 [points, 5], 'measured': int16 [measure points, 4]} of the code as it is."""
    pred, rout = [], []
    for manager, force, x, _ in points():
        pred.append(predicates(manager, force, x))
        rout.append(routed(manager, force, x))
    return {'predicates': np.asarray(pred, dtype=np.int8), 'routed': np.asarray(rout, dtype=np.int8),
            'measured': np.asarray([measured(x) for x, _ in measure_points()], dtype=np.int16)}


if __name__ == '__main__':
    out = record()
    np.savez_compressed(os.path.join(HERE, 'collect_routes.npz'), **out)
    p, r, m = out['predicates'], out['routed'], out['measured']
    print('collect_routes.npz: %d points; predicates true %s, raised %d; direct %d, upcast %d, raised %d; measure: direct %d, upcast %d, '
          'raised %d' % (len(p), (p == 1).sum(0).tolist(), (p > 1).sum(), (r[:, 0] == DIRECT).sum(), (r[:, 0] == UPCAST).sum(),
                         (r[:, 0] == RAISED).sum(), (m[:, 0] == DIRECT).sum(), (m[:, 0] == UPCAST).sum(), (m[:, 0] == RAISED).sum()))
