#!/usr/bin/env python3
"""The `-sm collect -ce` step (the statistics table with b, the three candidates of `-c mix`, their six error columns) over the 12
classes of ResNet-50 conv outputs of bench.py's headline workload as contiguous bf16 / fp16 tensors, one tensor per class, in two
routes timed in one process, alternating step by step:
    native  the tensor in its own dtype (ops.pc_stats_half -> ops.mix_candidates -> ops.pc_quant_errors_half);
    upcast  the route without the half error kernel (what the statistics manager did before): the x.float() that upcast_fallback
            makes, then ops.pc_stats, ops.mix_candidates and ops.pc_quant_errors on the float32 copy.
Per class and route the median step time of --steps steps after --warmup (HIP events) with the minimum and maximum as the spread,
the same for the whole set weighted by the layers per class.  A class counts as won when native's maximum is below the upcast
route's minimum.  The error calls alone (K = 3, with the extrema; kernel and fold) are timed the same way: ops.pc_quant_errors_half
on the tensor, ops.pc_quant_errors on a float32 copy made outside the timed region; their rate is the bytes of x over the time of
the call.  Before anything is timed every class is checked: no upcast on the native route, the same bits with and without the
extrema, and columns within 2 * 2e-6 of the float32 kernel's columns of the same table (exit status 1 otherwise); the largest
relative deviation is reported, and whether the route words keep the class native (kept_native).  Prints one JSON line.

    tools/bench_half_qerr.py [--batch 512] [--steps 10] [--warmup 2] [--dtypes bfloat16,float16]"""
import argparse
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUTES = ('native', 'upcast')
SETTINGS = dict(num_bits=4, positive=False, bit_alloc=False)


def run_route(ops, L, route, xc):
    if route == 'native':
        table, _ = ops.pc_stats_half(xc, need_b=True)
        qp_l, qp_g, qp_p = ops.mix_candidates(table, **SETTINGS)
        return torch.cat([table, ops.pc_quant_errors_half(xc, (qp_p, qp_g, qp_l), mm=table[[L.STAT_MIN, L.STAT_MAX]])])
    x = xc.float()
    N, C = x.shape[:2]
    HW = x.numel() // (N * C)
    table, _ = ops.pc_stats(x, N, C, HW, need_b=True, group=False)
    qp_l, qp_g, qp_p = ops.mix_candidates(table, **SETTINGS)
    return torch.cat([table, ops.pc_quant_errors(x, N, C, HW, (qp_p, qp_g, qp_l), mm=table[[L.STAT_MIN, L.STAT_MAX]])])


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def median(v):
    s = sorted(v)
    return (s[(len(s) - 1) // 2] + s[len(s) // 2]) / 2


def us(ms):
    return dict(us_median=round(median(ms) * 1e3, 1), us_min=round(min(ms) * 1e3, 1), us_max=round(max(ms) * 1e3, 1))


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--batch', type=int, default=512)
    p.add_argument('--steps', type=int, default=10)
    p.add_argument('--warmup', type=int, default=2)
    p.add_argument('--dtypes', default='bfloat16,float16')
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_half_qerr.py needs a GPU')
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
        for k, (C, hw, _, count) in enumerate(bench.RESNET50_CONV_OUTPUTS):
            xc = bench.laplace_activation((a.batch, C, hw, hw), 12345 + k, dev).to(dt)
            torch.cuda.empty_cache()
            # the contract of this class
            before = (ops.LAYOUT_COPIES, iq.HALF_FALLBACKS)
            got = run_route(ops, L, 'native', xc)
            table = got[:L.NSTAT].contiguous()
            qp_l, qp_g, qp_p = ops.mix_candidates(table, **SETTINGS)
            qps, mm = (qp_p, qp_g, qp_l), table[[L.STAT_MIN, L.STAT_MAX]]
            plain = ops.pc_quant_errors_half(xc, qps)
            clean = (ops.LAYOUT_COPIES, iq.HALF_FALLBACKS) == before
            same = torch.equal(plain.view(torch.int32), got[L.NSTAT:].contiguous().view(torch.int32))
            x32 = xc.float()
            N, HW = a.batch, hw * hw
            want = ops.pc_quant_errors(x32, N, C, HW, qps, mm=mm)
            dev_rel = float(((plain - want).abs() / want.abs()).max())
            good = bool(clean and same and dev_rel <= 4e-6)
            ok = ok and good
            c = dict(layers=count, elements=xc.numel(), contract=good,
                     kept_native=bool(ops._stats_half_native(N, C, HW, dt) and ops._qerr_half_native(N, C, HW, dt)), max_rel_dev_vs_fp32_kernel=float('%.2e' % dev_rel))
            # the kernels alone
            c['errors_native'] = us(timed(lambda: ops.pc_quant_errors_half(xc, qps, mm=mm), a.steps, a.warmup))
            c['errors_native_TB_per_s'] = round(xc.numel() * es / (c['errors_native']['us_median'] * 1e-6) / 1e12, 3)
            c['errors_fp32'] = us(timed(lambda: ops.pc_quant_errors(x32, N, C, HW, qps, mm=mm), a.steps, a.warmup))
            c['errors_fp32_TB_per_s'] = round(xc.numel() * 4 / (c['errors_fp32']['us_median'] * 1e-6) / 1e12, 3)
            del x32, want, plain, got
            torch.cuda.empty_cache()
            # the collect step, both routes alternating
            for _ in range(a.warmup):
                for r in ROUTES:
                    run_route(ops, L, r, xc)
            torch.cuda.synchronize()
            ms = {r: [] for r in ROUTES}
            for _ in range(a.steps):
                for r in ROUTES:
                    ms[r] += timed(lambda: run_route(ops, L, r, xc), 1, 0)
            for r in ROUTES:
                c[r] = us(ms[r])
                for i in range(a.steps):
                    tot[r][i] += ms[r][i] * count
            c['native_wins_beyond_spread'] = c['native']['us_max'] < c['upcast']['us_min']
            classes['%dx%dx%d' % (C, hw, hw)] = c
            del xc
            torch.cuda.empty_cache()
        out = {r: dict(ms_median=round(median(tot[r]), 4), ms_min=round(min(tot[r]), 4), ms_max=round(max(tot[r]), 4)) for r in ROUTES}
        res[name] = dict(all_53_layers=out, native_over_upcast=round(out['native']['ms_median'] / out['upcast']['ms_median'], 4), classes=classes,
                         classes_not_won=[k for k, c in classes.items() if not c['native_wins_beyond_spread']])
    print(json.dumps(dict(workload='resnet50 b%d -sm collect -ce (12 classes, weighted by their 53 layers)' % a.batch,
                          steps=a.steps, warmup=a.warmup, device=torch.cuda.get_device_name(0), contract=bool(ok), results=res)))
    if not ok:
        sys.exit(1)


if __name__ == '__main__':
    main()
