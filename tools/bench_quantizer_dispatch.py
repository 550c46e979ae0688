"""Host time of IntQuantizer's routing decision, without a GPU: __call__'s upcast condition, its dispatch, and the questions the
branch method asks before it calls into ops.  The ops entry points are replaced by stubs that hand the tensor back, the tensors are CPU
tensors that say they are on the device, and an upcast hands __call__ a float32 twin made beforehand - so what is timed is the Python
the decision costs on every layer of every forward, and nothing else.

    python tools/bench_quantizer_dispatch.py [--repeats 7] [--calls 20000]

Config 2, config 3 with -baa and config 5, each on a contiguous and on a dense channels_last bf16 activation of (2, 8, 4, 4); per case
the median and the min-max of the repeats, in microseconds per decision."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--calls', type=int, default=20000)
    args = ap.parse_args()
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
