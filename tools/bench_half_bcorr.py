#!/usr/bin/env python3
"""`-sm use -c laplace -baa -bca` (the table-driven Q/DQ with the activation bias correction folded in) over the 12 classes of
ResNet-50 conv outputs of bench.py's headline workload as contiguous bf16 (or fp16) tensors, one tensor per class, in up to three
routes timed in one process, alternating step by step:
    two_passes  the tensor in its own dtype on the half kernels (ops.qdq_bias_corrected_half, single_launch=False): the sums, the
                bias, the fused quantize + correct pass - 6 B/elem;
    single      the same call in one launch (single_launch=True) where a channel's batch population fits one workgroup's
                registers - 4 B/elem;
    former      the route without them (what the quantizer did before): the upcast x.float() that upcast_fallback makes,
                ops.act_qdq_per_channel(stats=table, clip='laplace', bit_alloc=True, bcorr=...) on the fp32 copy, .to(dtype).
The parameter table comes from the tensor's own statistics (ops.pc_stats_half) and is made once per class, outside the timed part,
for all routes (ops.pc_params on a [NSTAT, C] table is the same launch on every route).  Per class and route the mean step time of
--steps steps after --warmup (HIP events) with the minimum and maximum as the spread, and the same for the whole set weighted by
the layers per class with every class on the best native route.  A route counts as won against another when its maximum is below
the other's minimum.  Before anything is timed every class is checked: no layout copy and no upcast on the native routes (exit
status 1 otherwise); the share of elements that differ from the former route's result (the sums are added in another order, so a
bias may differ in its last bits) is reported.  Prints one JSON line.

    tools/bench_half_bcorr.py [--batch 512] [--steps 20] [--warmup 3] [--dtypes bfloat16,float16] [--bits 4]"""
import argparse
import ctypes
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RELU_FIRST = True


def run_route(ops, route, x, table, qp, bits):
    if route == 'former':
        return ops.act_qdq_per_channel(x.float(), bits, clip='laplace', bit_alloc=True, stats=table, group=False, bcorr=RELU_FIRST).to(x.dtype)
    return ops.qdq_bias_corrected_half(x, qp, RELU_FIRST, single_launch=(route == 'single'))


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def wins(a, b):
    return a['us_max'] < b['us_min']


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--batch', type=int, default=512)
    p.add_argument('--steps', type=int, default=20)
    p.add_argument('--warmup', type=int, default=3)
    p.add_argument('--dtypes', default='bfloat16,float16')
    p.add_argument('--bits', type=int, default=4)
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_half_bcorr.py needs a GPU')
    import bench
    from cnn_quantization_amd import _lib as L, ops
    iq = importlib.import_module('cnn_quantization_amd.qtypes.int_quantizer')
    dev = torch.device('cuda')
    res = {}
    ok = True
    for name in a.dtypes.split(','):
        dt = getattr(torch, name)
        classes = {}
        tot = {r: [0.0] * a.steps for r in ('native', 'former')}
        for k, (C, hw, _, count) in enumerate(bench.RESNET50_CONV_OUTPUTS):
            x = bench.laplace_activation((a.batch, C, hw, hw), 12345 + k, dev).to(dt)
            torch.cuda.empty_cache()
            table = ops.pc_stats_half(x, need_b=True)[0]
            qp = ops.pc_params(table, a.bits, False, 'laplace', a.bits <= 4, False)[0]
            word = (ctypes.c_int32 * 4)()
            L.check(L.load().cnnq_pc_route_qdq_bcorr_dt(a.batch, C, hw * hw, ops._HALF_DTYPES[dt], 16, 2, word), 'cnnq_pc_route_qdq_bcorr_dt')
            routes = ['two_passes'] + (['single'] if word[3] == 1 else []) + ['former']
            # the contract of this class
            before = (ops.LAYOUT_COPIES, iq.HALF_FALLBACKS)
            ys = {r: run_route(ops, r, x, table, qp, a.bits) for r in routes if r != 'former'}
            clean = (ops.LAYOUT_COPIES, iq.HALF_FALLBACKS) == before
            y0 = run_route(ops, 'former', x, table, qp, a.bits)
            differ = {r: float((y != y0).float().mean()) for r, y in ys.items()}
            ok = ok and clean
            del ys, y0
            for _ in range(a.warmup):
                for r in routes:
                    run_route(ops, r, x, table, qp, a.bits)
            torch.cuda.synchronize()
            ms = {r: [] for r in routes}
            for _ in range(a.steps):
                for r in routes:
                    ms[r].append(timed(lambda: run_route(ops, r, x, table, qp, a.bits)))
            c = dict(layers=count, elements=x.numel(), route_words=list(word), contract=bool(clean),
                     share_of_elements_differing_from_former={r: float('%.2e' % v) for r, v in differ.items()})
            for r in routes:
                c[r] = dict(us_mean=round(sum(ms[r]) / a.steps * 1e3, 1), us_min=round(min(ms[r]) * 1e3, 1), us_max=round(max(ms[r]) * 1e3, 1))
            c['two_passes_wins_over_former_beyond_spread'] = wins(c['two_passes'], c['former'])
            best = 'two_passes'
            if 'single' in routes:
                c['single_wins_over_two_passes_beyond_spread'] = wins(c['single'], c['two_passes'])
                c['single_wins_over_former_beyond_spread'] = wins(c['single'], c['former'])
                if c['single_wins_over_two_passes_beyond_spread']:
                    best = 'single'
            c['best_native'] = best
            c['native_TB_per_s'] = round(x.numel() * x.element_size() * (2 if best == 'single' else 3) / (c[best]['us_mean'] * 1e-6) / 1e12, 3)
            for i in range(a.steps):
                tot['native'][i] += ms[best][i] * count
                tot['former'][i] += ms['former'][i] * count
            classes['%dx%dx%d' % (C, hw, hw)] = c
            del x
            torch.cuda.empty_cache()
        out = {r: dict(ms_mean=round(sum(tot[r]) / a.steps, 4), ms_min=round(min(tot[r]), 4), ms_max=round(max(tot[r]), 4)) for r in tot}
        res[name] = dict(all_53_layers=out, native_over_former=round(out['native']['ms_mean'] / out['former']['ms_mean'], 4),
                         native_wins_beyond_spread=out['native']['ms_max'] < out['former']['ms_min'], classes=classes,
                         classes_not_won=[k for k, c in classes.items()
                                          if not wins(c[c['best_native']], c['former'])])
    print(json.dumps(dict(workload='resnet50 b%d -sm use -c laplace -baa -bca on contiguous half tensors (12 classes, weighted by their '
                                   '53 layers)' % a.batch,
                          bits=a.bits, steps=a.steps, warmup=a.warmup, device=torch.cuda.get_device_name(0), contract=bool(ok), results=res)))
    if not ok:
        sys.exit(1)


if __name__ == '__main__':
    main()
