#!/usr/bin/env python3
"""Per-tensor Laplace clipping (layer-wise ACIQ, int4: `-c laplace` without -pcq_a) over the 12 classes of ResNet-50 conv outputs
of bench.py's headline workload, one tensor per class, in three forms - bfloat16 and float32 dense channels_last, bfloat16
contiguous - two modes - dynamic statistics, and a statistics table (-sm use) - and two routes timed in one process, alternating
step by step:
    native  the tensor where it lies (ops.clip_qdq_tensor -> cnnq_pt_clip_qdq, or pc_params + cnnq_flat_qdq with the table);
    former  the route without it (what IntQuantizer did before): upcast_fallback's x.float() for bf16, the counted copy to NCHW,
            ops.act_qdq_per_channel(whole_tensor=True) - the per-channel chain on one channel - and the cast back.
Per class, mode and route the median step time of --steps steps after --warmup (HIP events) with the minimum and maximum as the
spread, the same for the whole set weighted by the layers per class, and the rate of the bytes the table-driven native pass moves
at least (x read, y written).  A class counts as won when native's maximum is below the former route's minimum.  Before anything
is timed every class is checked: no layout copy and no upcast on the native route, and with the table the two routes' results
bit-equal (exit status 1 otherwise); for the dynamic mode the share of elements that differ is reported (the scalar statistics of
the two routes differ in their last bits).  Prints one JSON line.

    tools/bench_tensor_clip.py [--batch 512] [--steps 10] [--warmup 3] [--forms bfloat16:nhwc,float32:nhwc,bfloat16:nchw]"""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUTES = ('native', 'former')
MODES = ('dynamic', 'table')
BITS, CLIP = 4, 'laplace'


def run_route(ops, iq, route, x, table):
    if route == 'native':
        return ops.clip_qdq_tensor(x, BITS, clip=CLIP, stats=table)
    return iq.upcast_fallback(lambda t: ops.act_qdq_per_channel(t, BITS, clip=CLIP, whole_tensor=True, stats=table, group=False).view(t.shape), x)


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
        sys.exit('bench_tensor_clip.py needs a GPU')
    import bench
    from cnn_quantization_amd import ops
    iq = importlib.import_module('cnn_quantization_amd.qtypes.int_quantizer')
    dev = torch.device('cuda')
    res = {}
    ok = True
    for form in a.forms.split(','):
        name, layout = form.split(':')
        dt = getattr(torch, name)
        es = torch.empty(0, dtype=dt).element_size()
        classes = {}
        tot = {(m, r): [0.0] * a.steps for m in MODES for r in ROUTES}
        elems = 0
        for k, (C, hw, _, count) in enumerate(bench.RESNET50_CONV_OUTPUTS):
            x = bench.laplace_activation((a.batch, C, hw, hw), 12345 + k, dev).to(dt)
            if layout == 'nhwc':
                x = x.to(memory_format=torch.channels_last)
            torch.cuda.empty_cache()
            table = ops.tensor_stats(x, 1)[0]
            tables = dict(dynamic=None, table=table)
            # the contract of this class
            before = (ops.LAYOUT_COPIES, iq.HALF_FALLBACKS)
            yt, yd = run_route(ops, iq, 'native', x, table), run_route(ops, iq, 'native', x, None)
            clean = (ops.LAYOUT_COPIES, iq.HALF_FALLBACKS) == before and yt.stride() == x.stride() and yt.dtype == x.dtype
            equal = torch.equal(yt, run_route(ops, iq, 'former', x, table))
            differ = float((yd != run_route(ops, iq, 'former', x, None)).float().mean())
            ok = ok and clean and equal
            del yt, yd
            c = dict(layers=count, elements=x.numel(), contract=bool(clean and equal), dynamic_share_differing_from_former=float('%.2e' % differ))
            for m in MODES:
                for _ in range(a.warmup):
                    for r in ROUTES:
                        run_route(ops, iq, r, x, tables[m])
                torch.cuda.synchronize()
                ms = {r: [] for r in ROUTES}
                for _ in range(a.steps):
                    for r in ROUTES:
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        run_route(ops, iq, r, x, tables[m])
                        e1.record()
                        torch.cuda.synchronize()
                        ms[r].append(e0.elapsed_time(e1))
                cm = {r: spread(ms[r]) for r in ROUTES}
                for r in ROUTES:
                    for i in range(a.steps):
                        tot[(m, r)][i] += ms[r][i] * count
                cm['native_wins_beyond_spread'] = cm['native']['us_max'] < cm['former']['us_min']
                cm['native_loses_beyond_spread'] = cm['native']['us_min'] > cm['former']['us_max']
                c[m] = cm
            c['table_native_TB_per_s'] = round(x.numel() * 2 * es / (c['table']['native']['us_median'] * 1e-6) / 1e12, 3)
            classes['%dx%dx%d' % (C, hw, hw)] = c
            elems += x.numel() * count
            del x
            torch.cuda.empty_cache()
        out = {}
        for m in MODES:
            o = {r: dict(ms_median=round(statistics.median(tot[(m, r)]), 4), ms_min=round(min(tot[(m, r)]), 4),
                         ms_max=round(max(tot[(m, r)]), 4)) for r in ROUTES}
            o['native_over_former'] = round(o['native']['ms_median'] / o['former']['ms_median'], 4)
            o['classes_not_won'] = [k for k, c in classes.items() if not c[m]['native_wins_beyond_spread']]
            o['classes_lost'] = [k for k, c in classes.items() if c[m]['native_loses_beyond_spread']]
            out[m] = o
        res[form] = dict(all_53_layers=out, table_native_bytes_per_elem=2 * es, elements=elems, classes=classes)
    print(json.dumps(dict(workload='resnet50 b%d per-tensor %s clipping int%d (12 classes, weighted by their 53 layers)' % (a.batch, CLIP, BITS),
                          steps=a.steps, warmup=a.warmup, device=torch.cuda.get_device_name(0), contract=bool(ok), results=res)))
    if not ok:
        sys.exit(1)


if __name__ == '__main__':
    main()
