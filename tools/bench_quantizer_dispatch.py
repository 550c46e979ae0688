"""Host time of IntQuantizer's routing decision, without a GPU: __call__'s upcast condition, its dispatch, and the questions the
branch method asks before it calls into ops.  The ops entry points are replaced by stubs that hand the tensor back, the tensors are CPU
tensors that say they are on the device, and an upcast hands __call__ a float32 twin made beforehand - so what is timed is the Python
the decision costs on every layer of every forward, and nothing else.

    python tools/bench_quantizer_dispatch.py [--repeats 7] [--calls 20000]

Config 2, config 3 with -baa and config 5, each on a contiguous and on a dense channels_last bf16 activation of (2, 8, 4, 4); per case
the median and the min-max of the repeats, in microseconds per decision.

    python tools/bench_quantizer_dispatch.py --collect

times the `-sm collect` side instead: the collect branch of inference_quantization_manager._route and the statistics manager's own
decision behind it, on the four storage classes (bf16 and fp32, contiguous and channels_last) and both managers, with the ops
functions replaced by stubs that return ready host tables."""
import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

from _quantizer import PARAMS, act, nhwc     # noqa: E402

CONFIGS = [('config 2', dict(clipping='no')), ('config 3 -baa', dict(clipping='laplace', bit_alloc_act=True)),
           ('config 5', dict(clipping='laplace', mtd_quant=True, measure_entropy=True, bit_alloc_target_act=5.3))]


def stub_ops(ops):
    """Every ops entry point the three configs can reach returns its tensor (with the entropy slot where the caller unpacks one)."""
    def one(x, *a, want_entropy=False, **kw):
        return (x, None) if want_entropy else x

    def two(x, *a, **kw):
        return x, None
    for name in ('act_qdq_per_channel', 'aciq_qdq_nhwc', 'aciq_qdq_half', 'clip_qdq_tensor', 'mid_tread_qdq_tensor'):
        setattr(ops, name, one)
    for name in ('mid_tread_qdq', 'mid_tread_qdq_nhwc'):
        setattr(ops, name, two)


def collect(args):
    import types
    from cnn_quantization_amd import _lib as L, ops
    from cnn_quantization_amd.inference import inference_quantization_manager as iqm
    from cnn_quantization_amd.inference.statistic_manager import StatisticManager
    from cnn_quantization_amd.inference.statistic_manager_perchannel import StatisticManagerPerChannel
    from cnn_quantization_amd.utils.misc import Singleton

    def tables(C):
        return torch.zeros(L.NSTAT, C), torch.ones(L.NMOM, C, dtype=torch.float64)
    per_channel, per_tensor = tables(8), tables(1)
    for name in ('pc_stats_nhwc', 'pc_stats_half'):
        setattr(ops, name, lambda x, **kw: per_channel)
    ops.pc_stats = lambda x, N, C, HW, **kw: per_channel if C > 1 else per_tensor
    ops.tensor_stats = lambda x, rows=1, need_dev=True: per_tensor
    twins = {}
    iqm.upcast_fallback = lambda fn, t, *a, **kw: fn(twins[id(t)], *a, **kw)
    print('| manager, tensor | median us | min us | max us |')
    print('|---|---|---|---|')
    for cls in (StatisticManagerPerChannel, StatisticManager):
        for dtype in (torch.bfloat16, torch.float32):
            for layout, make in (('contiguous', act), ('channels_last', nhwc)):
                Singleton.reset()
                manager = cls('bench', load_stats=False)
                manager._record = lambda id, table: None        # (the per-channel manager's copy to the host)
                qm = types.SimpleNamespace(enabled=True, stats_mode=iqm.StatsMode.collect_stats, stats_manager=manager)
                iqm.QMI = lambda: qm
                x = make(dtype)
                twins[id(x)] = x.float()
                per_call = []
                for _ in range(args.repeats):
                    t0 = time.perf_counter()
                    for _ in range(args.calls):
                        iqm._route(None, x, 'conv0_activation', 'activation')
                        manager.stats.clear()
                    per_call.append((time.perf_counter() - t0) / args.calls * 1e6)
                print('| %s, %s %s | %.2f | %.2f | %.2f |' % ('per channel' if cls is StatisticManagerPerChannel else 'per tensor',
                                                            str(dtype).replace('torch.', ''), layout, statistics.median(per_call),
                                                            min(per_call), max(per_call)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--calls', type=int, default=20000)
    ap.add_argument('--collect', action='store_true', help='time the -sm collect route decision instead')
    args = ap.parse_args()
    if args.collect:
        return collect(args)
    from cnn_quantization_amd import ops
    from cnn_quantization_amd.qtypes.int_quantizer import IntQuantizer
    iq = sys.modules[IntQuantizer.__module__]
    stub_ops(ops)
    twins = {}
    iq.upcast_fallback = lambda fn, t, *a, **kw: fn(twins[id(t)], *a, **kw)
    print('| case | median us | min us | max us | upcasts |')
    print('|---|---|---|---|---|')
    for name, kw in CONFIGS:
        for layout, x in (('contiguous', act()), ('channels_last', nhwc())):
            q = IntQuantizer(4, dict(PARAMS, pcq_act=True, **kw))
            q.half_dynamic = True
            twins[id(x)] = x.float()
            seen = []
            iq.upcast_fallback, keep = (lambda fn, t, *a, **kw: seen.append(1) or fn(twins[id(t)], *a, **kw)), iq.upcast_fallback
            q(x, 'layer')
            iq.upcast_fallback = keep
            per_call = []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                for _ in range(args.calls):
                    q(x, 'layer')
                per_call.append((time.perf_counter() - t0) / args.calls * 1e6)
            print('| %s, bf16 %s | %.2f | %.2f | %.2f | %s |' % (name, layout, statistics.median(per_call), min(per_call),
                                                               max(per_call), 'yes' if seen else 'no'))


if __name__ == '__main__':
    main()
