#!/usr/bin/env python3
"""`-sm collect` (all seven per-channel statistics: min, max, mean, std, b, kurtosis, std_pos) over the 12 classes of ResNet-50
conv outputs of bench.py's headline workload as contiguous bf16 (or fp16) tensors, one tensor per class, in two routes timed in
one process, alternating step by step:
    native  the tensor in its own dtype on the half kernels (ops.pc_stats_half -> cnnq_pc_stats_dt);
    former  the route without them (what the statistics manager did before): the upcast x.float() that upcast_fallback makes,
            then ops.pc_stats on the fp32 copy.
Per class and route the mean step time of --steps steps after --warmup (HIP events) with the minimum and maximum as the spread,
the same for the whole set weighted by the layers per class, and the bytes native moves at least (x read twice).  A class counts
as won when native's maximum is below the former route's minimum.  Before anything is timed every class is checked: no layout
copy and no upcast on the native route and extrema bit-equal to the former route's (exit status 1 otherwise); the largest
relative deviation of every other row from the former route's is reported.
On [batch,256,56,56] pass A (with its merge) and pass B (with its merge: the full call minus pass A) are timed next to the
extrema launch of config 2 (k_h_minmax with its merge, cnnq_pc_minmax_local_dt) on the same tensor, as achieved bytes per second
of one read of x.  Prints one JSON line.

    tools/bench_half_collect.py [--batch 512] [--steps 20] [--warmup 3] [--dtypes bfloat16,float16]"""
import argparse
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUTES = ('native', 'former')
NEED = dict(need_b=True, need_kurt=True, need_relu=True)


def run_route(ops, route, x):
    if route == 'native':
        return ops.pc_stats_half(x, **NEED)[0]
    xf = x.float()
    N, C = xf.shape[:2]
    return ops.pc_stats(xf, N, C, xf.numel() // (N * C), group=False, **NEED)[0]


def timed(fn, steps):
    ms = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms


def passes(ops, L, x, steps, warmup):
    """Pass A, pass B and config 2's extrema launch on x, alternating step by step: the mean time of each and the bytes per
    second of one read of x."""
    N, C = x.shape[:2]
    HW = x.numel() // (N * C)
    lib = L.load()
    G = max(lib.cnnq_pc_groups(N, C, HW, 1), lib.cnnq_pc_groups(N, C, HW, 0))
    pmm = torch.empty((G, 2, C), dtype=torch.float32, device=x.device)
    local = torch.empty((2, C), dtype=torch.float32, device=x.device)
    dt = ops._HALF_DTYPES[x.dtype]
    st = torch.cuda.current_stream().cuda_stream

    def minmax():
        L.check(lib.cnnq_pc_minmax_local_dt(x.data_ptr(), dt, N, C, HW, pmm.data_ptr(), local.data_ptr(), st), 'cnnq_pc_minmax_local_dt')
    legs = dict(pass_a=lambda: ops.pc_stats_half(x, need_relu=True), full=lambda: ops.pc_stats_half(x, **NEED), k_h_minmax=minmax)
    for _ in range(warmup):
        for f in legs.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(steps):
        for k, f in legs.items():
            ms[k] += timed(f, 1)
    mean = {k: sum(v) / steps for k, v in ms.items()}
    mean['pass_b'] = mean['full'] - mean['pass_a']
    nbytes = x.numel() * x.element_size()
    return {k: dict(us_mean=round(mean[k] * 1e3, 1), TB_per_s=round(nbytes / (mean[k] * 1e-3) / 1e12, 3))
            for k in ('pass_a', 'pass_b', 'k_h_minmax')}


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--batch', type=int, default=512)
    p.add_argument('--steps', type=int, default=20)
    p.add_argument('--warmup', type=int, default=3)
    p.add_argument('--dtypes', default='bfloat16')
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_half_collect.py needs a GPU')
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
        one_pass = None
        for k, (C, hw, _, count) in enumerate(bench.RESNET50_CONV_OUTPUTS):
            x = bench.laplace_activation((a.batch, C, hw, hw), 12345 + k, dev).to(dt)
            torch.cuda.empty_cache()
            # the contract of this class
            before = (ops.LAYOUT_COPIES, iq.HALF_FALLBACKS)
            st = run_route(ops, 'native', x)
            clean = (ops.LAYOUT_COPIES, iq.HALF_FALLBACKS) == before
            st0 = run_route(ops, 'former', x)
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
                    ms[r] += timed(lambda: run_route(ops, r, x), 1)
            c = dict(layers=count, elements=x.numel(), contract=bool(clean and close),
                     max_rel_dev_vs_former={n: float('%.2e' % v) for n, v in dev_rel.items()})
            for r in ROUTES:
                c[r] = dict(us_mean=round(sum(ms[r]) / a.steps * 1e3, 1), us_min=round(min(ms[r]) * 1e3, 1), us_max=round(max(ms[r]) * 1e3, 1))
                for i in range(a.steps):
                    tot[r][i] += ms[r][i] * count
            c['native_TB_per_s'] = round(x.numel() * 2 * es / (c['native']['us_mean'] * 1e-6) / 1e12, 3)
            c['native_wins_beyond_spread'] = c['native']['us_max'] < c['former']['us_min']
            classes['%dx%dx%d' % (C, hw, hw)] = c
            elems += x.numel() * count
            if (C, hw) == (256, 56):
                one_pass = passes(ops, L, x, a.steps, a.warmup)
            del x, st, st0
            torch.cuda.empty_cache()
        out = {r: dict(ms_mean=round(sum(tot[r]) / a.steps, 4), ms_min=round(min(tot[r]), 4), ms_max=round(max(tot[r]), 4)) for r in ROUTES}
        res[name] = dict(all_53_layers=out, native_over_former=round(out['native']['ms_mean'] / out['former']['ms_mean'], 4),
                         native_wins_beyond_spread=out['native']['ms_max'] < out['former']['ms_min'],
                         native_bytes_per_elem=2 * es, elements=elems, classes=classes,
                         classes_not_won=[k for k, c in classes.items() if not c['native_wins_beyond_spread']],
                         one_read_of_256x56x56=one_pass)
    print(json.dumps(dict(workload='resnet50 b%d -sm collect on contiguous half tensors, seven statistics (12 classes, weighted by '
                                   'their 53 layers)' % a.batch,
                          steps=a.steps, warmup=a.warmup, device=torch.cuda.get_device_name(0), contract=bool(ok), results=res)))
    if not ok:
        sys.exit(1)


if __name__ == '__main__':
    main()
