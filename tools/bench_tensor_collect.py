#!/usr/bin/env python3
"""The per-tensor `-sm collect` table (min, max, mean, std, b, kurtosis and the rectified sums behind mean_abs of the WHOLE tensor)
over the 12 classes of ResNet-50 conv outputs of bench.py's headline workload, one tensor per class, in three forms - bfloat16 and
float32 dense channels_last, bfloat16 contiguous - and two routes timed in one process, alternating step by step:
    native  the tensor where it lies on the flat-row kernels (ops.tensor_stats(x, 1) -> cnnq_rows_stats);
    copy    the route without them (what StatisticManager.save_tensor_stats did before): for bf16 the upcast x.float() that
            upcast_fallback makes, then x.contiguous(), then ops.pc_stats(x, 1, 1, n) - the per-channel chain on one channel.
Per class and route the median step time of --steps steps after --warmup (HIP events) with the minimum and maximum as the spread,
the same for the whole set weighted by the layers per class, and the bytes native moves at least (x read twice).  A class counts
as won when native's maximum is below the copy route's minimum.  Before anything is timed every class is checked: no layout copy
and no upcast on the native route and extrema bit-equal to the copy route's (exit status 1 otherwise); the largest relative
deviation of every other row from the copy route's is reported.  Prints one JSON line.

    tools/bench_tensor_collect.py [--batch 512] [--steps 10] [--warmup 3] [--forms bfloat16:nhwc,float32:nhwc,bfloat16:nchw]"""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUTES = ('native', 'copy')
NEED = dict(need_b=True, need_kurt=True, need_relu=True)


def run_route(ops, route, x):
    if route == 'native':
        return ops.tensor_stats(x, 1)[0]
    x = (x.float() if x.dtype != torch.float32 else x).contiguous()
    return ops.pc_stats(x, 1, 1, x.numel(), group=False, **NEED)[0]


def spread(v):
    return dict(us_median=round(statistics.median(v) * 1e3, 1), us_min=round(min(v) * 1e3, 1), us_max=round(max(v) * 1e3, 1))


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--batch', type=int, default=512)
    p.add_argument('--steps', type=int, default=10)
    p.add_argument('--warmup', type=int, default=3)
    p.add_argument('--forms', default='bfloat16:nhwc,float32:nhwc,bfloat16:nchw')
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_tensor_collect.py needs a GPU')
    import bench
    from cnn_quantization_amd import _lib as L, ops
    iq = importlib.import_module('cnn_quantization_amd.qtypes.int_quantizer')
    dev = torch.device('cuda')
    res = {}
    ok = True
    for form in a.forms.split(','):
        name, layout = form.split(':')
        dt = getattr(torch, name)
        es = torch.empty(0, dtype=dt).element_size()
        classes = {}
        tot = {r: [0.0] * a.steps for r in ROUTES}
        elems = 0
        for k, (C, hw, _, count) in enumerate(bench.RESNET50_CONV_OUTPUTS):
            x = bench.laplace_activation((a.batch, C, hw, hw), 12345 + k, dev).to(dt)
            if layout == 'nhwc':
                x = x.to(memory_format=torch.channels_last)
            torch.cuda.empty_cache()
            # the contract of this class
            before = (ops.LAYOUT_COPIES, iq.HALF_FALLBACKS)
            st = run_route(ops, 'native', x)
            clean = (ops.LAYOUT_COPIES, iq.HALF_FALLBACKS) == before
            st0 = run_route(ops, 'copy', x)
            close = torch.equal(st[[L.STAT_MIN, L.STAT_MAX]], st0[[L.STAT_MIN, L.STAT_MAX]])
            dev_rel = {n: float(((st[r] - st0[r]).abs() / st0[r].abs().clamp(min=1e-6)).max())
                       for n, r in (('mean', L.STAT_MEAN), ('std', L.STAT_STD), ('b', L.STAT_B), ('kurtosis', L.STAT_KURT),
                                    ('std_pos', L.STAT_STD_POS))}
            ok = ok and clean and close
            for _ in range(a.warmup):
                for r in ROUTES:
                    run_route(ops, r, x)
            torch.cuda.synchronize()
            ms = {r: [] for r in ROUTES}
            for _ in range(a.steps):
                for r in ROUTES:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    run_route(ops, r, x)
                    e1.record()
                    torch.cuda.synchronize()
                    ms[r].append(e0.elapsed_time(e1))
            c = dict(layers=count, elements=x.numel(), contract=bool(clean and close),
                     max_rel_dev_vs_copy={n: float('%.2e' % v) for n, v in dev_rel.items()})
            for r in ROUTES:
                c[r] = spread(ms[r])
                for i in range(a.steps):
                    tot[r][i] += ms[r][i] * count
            c['native_TB_per_s'] = round(x.numel() * 2 * es / (c['native']['us_median'] * 1e-6) / 1e12, 3)
            c['native_wins_beyond_spread'] = c['native']['us_max'] < c['copy']['us_min']
            c['native_loses_beyond_spread'] = c['native']['us_min'] > c['copy']['us_max']
            classes['%dx%dx%d' % (C, hw, hw)] = c
            elems += x.numel() * count
            del x, st, st0
            torch.cuda.empty_cache()
        out = {r: dict(ms_median=round(statistics.median(tot[r]), 4), ms_min=round(min(tot[r]), 4), ms_max=round(max(tot[r]), 4)) for r in ROUTES}
        res[form] = dict(all_53_layers=out, native_over_copy=round(out['native']['ms_median'] / out['copy']['ms_median'], 4),
                         native_bytes_per_elem=2 * es, elements=elems, classes=classes,
                         classes_not_won=[k for k, c in classes.items() if not c['native_wins_beyond_spread']],
                         classes_lost=[k for k, c in classes.items() if c['native_loses_beyond_spread']])
    print(json.dumps(dict(workload='resnet50 b%d per-tensor -sm collect (12 classes, weighted by their 53 layers)' % a.batch,
                          steps=a.steps, warmup=a.warmup, device=torch.cuda.get_device_name(0), contract=bool(ok), results=res)))
    if not ok:
        sys.exit(1)


if __name__ == '__main__':
    main()
