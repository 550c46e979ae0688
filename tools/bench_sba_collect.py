#!/usr/bin/env python3
"""`-pcq_a -sm collect -sba` (the seven per-channel statistics, max / min the mean over the batch of the per-sample extrema,
smpc.py:72-78) over the 12 classes of ResNet-50 conv outputs of bench.py's headline workload, one tensor per class, as contiguous
bf16, channels_last bf16 and channels_last fp32, in two routes timed in one process, alternating step by step:
    native  a manager with native_batch_avg: the native statistics of the storage, ops.pc_sample_extrema_half / _nhwc, the shared
            batch_extrema_sums;
    former  a manager without the keyword, fed as _route feeds it: the upcast x.float() of upcast_fallback, .contiguous(),
            ops.pc_stats, ops.pc_stats once more on the (n, c) rows, batch_extrema_sums.
Both are whole save_tensor_stats calls, the device->host copy of the table included.  Per class and route the mean step time of
--steps steps after --warmup (HIP events) with the minimum and maximum as the spread, and the same for the whole set weighted by the
layers per class.  The yardstick is the former route of the same run; a class counts as won when native's maximum is under the
former route's minimum (a class that does not win gets native = 0 in its route function).  The extrema pass alone is timed too, as
achieved bytes per second of one read of x, for the contiguous form next to ops.tensor_row_stats on the [N * C, HW] view (a
256-lane workgroup per row).  Before anything is timed every class is checked: no layout copy and no upcast on the native route, max /
min rows bit-equal to the former route's (exit status 1 otherwise).  Prints one JSON line.

    tools/bench_sba_collect.py [--batch 512] [--steps 20] [--warmup 3] [--forms bf16,bf16_nhwc,fp32_nhwc]"""
import argparse
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUTES = ('native', 'former')
FORMS = {'bf16': (torch.bfloat16, False), 'fp16': (torch.float16, False), 'bf16_nhwc': (torch.bfloat16, True),
         'fp16_nhwc': (torch.float16, True), 'fp32_nhwc': (torch.float32, True)}
BYTES_PER_ELEM = {'bf16': 6, 'fp16': 6, 'bf16_nhwc': 6, 'fp16_nhwc': 6, 'fp32_nhwc': 12}   # expected from the code: two statistics passes and the extrema pass


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def alternate(legs, steps, warmup):
    """ms[name] = the `steps` step times of each leg, the legs alternating step by step after `warmup` rounds."""
    for _ in range(warmup):
        for f in legs.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(steps):
        for k, f in legs.items():
            ms[k].append(timed(f))
    return ms


def spread(ms):
    return dict(us_mean=round(sum(ms) / len(ms) * 1e3, 1), us_min=round(min(ms) * 1e3, 1), us_max=round(max(ms) * 1e3, 1))


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--batch', type=int, default=512)
    p.add_argument('--steps', type=int, default=20)
    p.add_argument('--warmup', type=int, default=3)
    p.add_argument('--forms', default='bf16,bf16_nhwc,fp32_nhwc')
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_sba_collect.py needs a GPU')
    import bench
    from cnn_quantization_amd import ops
    from cnn_quantization_amd.inference import inference_quantization_manager as iqm
    from cnn_quantization_amd.inference import statistic_manager_perchannel as smpc
    iq = importlib.import_module('cnn_quantization_amd.qtypes.int_quantizer')
    dev = torch.device('cuda')

    def manager(**kw):
        smpc.Singleton._instances.pop(smpc.StatisticManagerPerChannel, None)
        return smpc.StatisticManagerPerChannel('bench_sba', load_stats=False, batch_avg=True, **kw)
    managers = dict(native=manager(native_batch_avg=True), former=manager())
    smpc.Singleton._instances.pop(smpc.StatisticManagerPerChannel, None)

    def step(route, x, cls):
        m = managers[route]
        m.stats.clear()
        if route == 'native':
            m.save_tensor_stats(x, 'activation', 'layer', route=cls)
        else:
            iqm.upcast_fallback(m.save_tensor_stats, x, 'activation', 'layer')
        return m.stats['layer']

    res = {}
    ok = True
    for form in a.forms.split(','):
        dt, nhwc = FORMS[form]
        cls = 'nhwc' if nhwc else 'half'
        extrema = ops.pc_sample_extrema_nhwc if nhwc else ops.pc_sample_extrema_half
        classes = {}
        tot = {r: [0.0] * a.steps for r in ROUTES}
        elems = 0
        for k, (C, hw, _, count) in enumerate(bench.RESNET50_CONV_OUTPUTS):
            x = bench.laplace_activation((a.batch, C, hw, hw), 12345 + k, dev).to(dt)
            if nhwc:
                x = x.contiguous(memory_format=torch.channels_last)
            torch.cuda.empty_cache()
            # the contract of this class
            before = (ops.LAYOUT_COPIES, iq.HALF_FALLBACKS)
            got = {n: v.copy() for n, v in step('native', x, cls).items()}
            clean = (ops.LAYOUT_COPIES, iq.HALF_FALLBACKS) == before
            want = step('former', x, cls)
            same = all(got[n].tobytes() == want[n].tobytes() for n in ('max', 'min'))
            ok = ok and clean and same
            ms = alternate({r: (lambda r=r: step(r, x, cls)) for r in ROUTES}, a.steps, a.warmup)
            c = dict(layers=count, elements=x.numel(), contract=bool(clean and same),
                     harness_route=managers['native'].collect_route(x))     # None: a route word keeps this class on the former route
            for r in ROUTES:
                c[r] = spread(ms[r])
                for i in range(a.steps):
                    tot[r][i] += ms[r][i] * count
            c['native_wins_beyond_spread'] = c['native']['us_max'] < c['former']['us_min']
            # the extrema pass alone: one read of x
            legs = dict(extrema=lambda: extrema(x))
            if not nhwc:
                N = x.shape[0]
                legs['tensor_row_stats'] = lambda: ops.tensor_row_stats(x, N * C)
            nbytes = x.numel() * x.element_size()
            for name, v in alternate(legs, a.steps, a.warmup).items():
                c[name] = dict(spread(v), TB_per_s=round(nbytes / (sum(v) / len(v) * 1e-3) / 1e12, 3))
            classes['%dx%dx%d' % (C, hw, hw)] = c
            elems += x.numel() * count
            del x
            torch.cuda.empty_cache()
        out = {r: dict(ms_mean=round(sum(tot[r]) / a.steps, 4), ms_min=round(min(tot[r]), 4), ms_max=round(max(tot[r]), 4)) for r in ROUTES}
        res[form] = dict(all_53_layers=out, native_over_former=round(out['native']['ms_mean'] / out['former']['ms_mean'], 4),
                         native_wins_beyond_spread=out['native']['ms_max'] < out['former']['ms_min'],
                         native_bytes_per_elem_expected=BYTES_PER_ELEM[form], elements=elems, classes=classes,
                         classes_not_won=[k for k, c in classes.items() if not c['native_wins_beyond_spread']])
    print(json.dumps(dict(workload='resnet50 b%d -pcq_a -sm collect -sba, whole save_tensor_stats steps (12 classes, weighted by their 53 '
                                   'layers)' % a.batch,
                          steps=a.steps, warmup=a.warmup, device=torch.cuda.get_device_name(0), contract=bool(ok), results=res)))
    if not ok:
        sys.exit(1)


if __name__ == '__main__':
    main()
