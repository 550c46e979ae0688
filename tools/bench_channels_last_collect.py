#!/usr/bin/env python3
"""`-sm collect` (all seven per-channel statistics: min, max, mean, std, b, kurtosis, std_pos) over the 12 classes of ResNet-50
conv outputs of bench.py's headline workload as dense channels_last tensors, one tensor per class, in two routes timed in one
process, alternating step by step:
    native  the channels_last tensor on the NHWC kernels (ops.pc_stats_nhwc -> cnnq_pc_stats_nhwc);
    copy    the route without them (what the statistics manager did before): for bf16 / fp16 the upcast x.float() that
            upcast_fallback makes, then x.contiguous(), then ops.pc_stats on the NCHW copy.
Per class and route the mean step time of --steps steps after --warmup (HIP events) with the minimum and maximum as the spread,
the same for the whole set weighted by the layers per class, and the bytes native moves at least (x read twice).  A class counts
as won when native's maximum is below the copy route's minimum.  Before anything is timed every class is checked: no layout
copy and no upcast on the native route and extrema bit-equal to the copy route's (exit status 1 otherwise); the largest relative
deviation of every other row from the copy route's is reported.  Prints one JSON line.

    tools/bench_channels_last_collect.py [--batch 512] [--steps 20] [--warmup 3] [--dtypes float32,bfloat16]"""
import argparse
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUTES = ('native', 'copy')
NEED = dict(need_b=True, need_kurt=True, need_relu=True)


def run_route(ops, route, xc):
    if route == 'native':
        return ops.pc_stats_nhwc(xc, **NEED)[0]
    x = (xc.float() if xc.dtype != torch.float32 else xc).contiguous()
    N, C = x.shape[:2]
    return ops.pc_stats(x, N, C, x.numel() // (N * C), group=False, **NEED)[0]


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--batch', type=int, default=512)
    p.add_argument('--steps', type=int, default=20)
    p.add_argument('--warmup', type=int, default=3)
    p.add_argument('--dtypes', default='float32,bfloat16')
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_channels_last_collect.py needs a GPU')
    import bench
    from cnn_quantization_amd import _lib as L, ops
    iq = importlib.import_module('cnn_quantization_amd.qtypes.int_quantizer')
    dev = torch.device('cuda')
    res = {}
    ok = True
    for name in a.dtypes.split(','):
        dt = getattr(torch, name)
        es = torch.empty(0, dtype=dt).element_size()
        classes = {}
        tot = {r: [0.0] * a.steps for r in ROUTES}
        elems = 0
        for k, (C, hw, _, count) in enumerate(bench.RESNET50_CONV_OUTPUTS):
            xc = bench.laplace_activation((a.batch, C, hw, hw), 12345 + k, dev).to(dt).to(memory_format=torch.channels_last)
            torch.cuda.empty_cache()
            # the contract of this class
            before = (ops.LAYOUT_COPIES, iq.HALF_FALLBACKS)
            st = run_route(ops, 'native', xc)
            clean = (ops.LAYOUT_COPIES, iq.HALF_FALLBACKS) == before
            st0 = run_route(ops, 'copy', xc)
            close = torch.equal(st[[L.STAT_MIN, L.STAT_MAX]], st0[[L.STAT_MIN, L.STAT_MAX]])
            dev_rel = {n: float(((st[r] - st0[r]).abs() / st0[r].abs().clamp(min=1e-6)).max())
                       for n, r in (('mean', L.STAT_MEAN), ('std', L.STAT_STD), ('b', L.STAT_B), ('kurtosis', L.STAT_KURT),
                                    ('std_pos', L.STAT_STD_POS))}
            ok = ok and clean and close
            for _ in range(a.warmup):
                for r in ROUTES:
                    run_route(ops, r, xc)
            torch.cuda.synchronize()
            ms = {r: [] for r in ROUTES}
            for _ in range(a.steps):
                for r in ROUTES:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    run_route(ops, r, xc)
                    e1.record()
                    torch.cuda.synchronize()
                    ms[r].append(e0.elapsed_time(e1))
            c = dict(layers=count, elements=xc.numel(), contract=bool(clean and close), max_rel_dev_vs_copy={n: float('%.2e' % v) for n, v in dev_rel.items()})
            for r in ROUTES:
                c[r] = dict(us_mean=round(sum(ms[r]) / a.steps * 1e3, 1), us_min=round(min(ms[r]) * 1e3, 1), us_max=round(max(ms[r]) * 1e3, 1))
                for i in range(a.steps):
                    tot[r][i] += ms[r][i] * count
            c['native_TB_per_s'] = round(xc.numel() * 2 * es / (c['native']['us_mean'] * 1e-6) / 1e12, 3)
            c['native_wins_beyond_spread'] = c['native']['us_max'] < c['copy']['us_min']
            classes['%dx%dx%d' % (C, hw, hw)] = c
            elems += xc.numel() * count
            del xc, st, st0
            torch.cuda.empty_cache()
        out = {r: dict(ms_mean=round(sum(tot[r]) / a.steps, 4), ms_min=round(min(tot[r]), 4), ms_max=round(max(tot[r]), 4)) for r in ROUTES}
        res[name] = dict(all_53_layers=out, native_over_copy=round(out['native']['ms_mean'] / out['copy']['ms_mean'], 4),
                         native_bytes_per_elem=2 * es, elements=elems, classes=classes,
                         classes_not_won=[k for k, c in classes.items() if not c['native_wins_beyond_spread']])
    print(json.dumps(dict(workload='resnet50 b%d -sm collect, seven statistics (12 classes, weighted by their 53 layers)' % a.batch,
                          steps=a.steps, warmup=a.warmup, device=torch.cuda.get_device_name(0), contract=bool(ok), results=res)))
    if not ok:
        sys.exit(1)


if __name__ == '__main__':
    main()
