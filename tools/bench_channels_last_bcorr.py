#!/usr/bin/env python3
"""The paper's recipe under calibrated statistics (-sm use -c laplace -baa -bca: per-channel int4, Laplace clipping, bit allocation,
activation bias correction) over the 53 ResNet-50 conv outputs of bench.py's headline workload as dense channels_last tensors, in
three routes timed in one process, alternating step by step:
    native  the channels_last tensors where they lie (pc_params + ops.qdq_bias_corrected_nhwc -> cnnq_pc_qdq_bcorr_nhwc),
            channels_last result;
    parent  the route before it (what a pending correction still takes without a statistics table): x.contiguous(), then pc_params
            + qdq_bias_corrected on the NCHW copy; for bf16 / fp16 the upcast in front and the downcast behind, as upcast_fallback
            does.  The conversion of the NCHW result back to channels_last, which a channels_last model pays downstream, is not
            counted;
    nchw    the same values as NCHW tensors (for bf16 / fp16 through the upcast, the only route they have).
Per route the median, minimum and maximum step time of --steps steps after --warmup (HIP events), the times per class of layer
(channels x extent), and the bytes native moves at least (x read twice, y written once).  Before anything is timed the largest
layer is checked against the contract: no layout copy, and y == (q + (q > 0) * bias).to(dtype) bit for bit, with q =
pc_qdq(x.contiguous().float(), qp) and the bias the device reduced.  Prints one JSON line; exit status 1 if that check fails.

    tools/bench_channels_last_bcorr.py [--batch 512] [--steps 10] [--warmup 3] [--dtypes float32,bfloat16]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUTES = ('native', 'parent', 'nchw')
BITS = 4


def same(a, b):
    a, b = a.contiguous(), b.contiguous()
    na, nb = torch.isnan(a), torch.isnan(b)
    if not torch.equal(na, nb):
        return False
    iv = torch.int32 if a.dtype == torch.float32 else torch.int16
    return torch.equal(a.view(iv)[~na], b.view(iv)[~nb])


def run_route(ops, route, L, dt):
    if route == 'native':
        qp, _ = ops.pc_params(L['table'], BITS, L['half'], 'laplace', True)
        return ops.qdq_bias_corrected_nhwc(L['xc'], qp, L['half'], out=L['yc'])
    kw = dict(positive=L['half'], clip='laplace', bit_alloc=True, stats=L['table'], bcorr=L['half'], group=False)
    x = L['xc'] if route == 'parent' else L['x']
    if dt == torch.float32:
        return ops.act_qdq_per_channel(x, BITS, out=L['y'], **kw)
    return ops.act_qdq_per_channel(x.float(), BITS, **kw).to(dt)


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--batch', type=int, default=512)
    p.add_argument('--steps', type=int, default=10)
    p.add_argument('--warmup', type=int, default=3)
    p.add_argument('--dtypes', default='float32,bfloat16')
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_channels_last_bcorr.py needs a GPU')
    from cnn_quantization_amd import ops
    import bench
    dev = torch.device('cuda')
    res = {}
    for name in a.dtypes.split(','):
        dt = getattr(torch, name)
        layers = []
        for L in bench.build_workload(a.batch, dev):
            x = L['x'].to(dt)
            N, C, H, W = x.shape
            # the calibration table: this tensor's own statistics (of the values the routes see)
            table, _ = ops.pc_stats(x.float(), N, C, H * W, need_b=True, local_only=True)
            xc = x.to(memory_format=torch.channels_last)
            layers.append(dict(x=x, y=torch.empty_like(x), xc=xc, yc=torch.empty_like(xc), half=L['half'], shape=list(x.shape),
                               table=table))
            del L
        torch.cuda.empty_cache()
        elems = sum(L['x'].numel() for L in layers)
        big = max(range(len(layers)), key=lambda i: layers[i]['x'].numel())

        def step(route, evs=None):
            ops._NHWC = route != 'parent'
            for i, L in enumerate(layers):
                if evs is not None:
                    evs[i].record()
                run_route(ops, route, L, dt)
            if evs is not None:
                evs[-1].record()

        # the contract on the largest layer, and that native never copies
        L = layers[big]
        ops._NHWC = True
        before = ops.LAYOUT_COPIES
        qp, _ = ops.pc_params(L['table'], BITS, L['half'], 'laplace', True)
        y, parts = ops.qdq_bias_corrected_nhwc(L['xc'], qp, L['half'], want_parts=True)
        step('native')
        no_copy = ops.LAYOUT_COPIES == before
        N, C, H, W = L['shape']
        q = ops.pc_qdq(L['xc'].contiguous().float(), N, C, H * W, qp)
        q += (q > 0).float() * parts['bias'].view(1, C, 1, 1)
        ref = q.to(dt)
        exact = same(y, ref) and same(L['yc'], ref)
        del y, q, ref, parts
        torch.cuda.empty_cache()
        for _ in range(a.warmup):
            for r in ROUTES:
                step(r)
        torch.cuda.synchronize()
        per = {r: [0.0] * len(layers) for r in ROUTES}
        tot = {r: [] for r in ROUTES}
        for _ in range(a.steps):
            for r in ROUTES:
                evs = [torch.cuda.Event(enable_timing=True) for _ in range(len(layers) + 1)]
                step(r, evs)
                torch.cuda.synchronize()
                for i in range(len(layers)):
                    per[r][i] += evs[i].elapsed_time(evs[i + 1])
                tot[r].append(evs[0].elapsed_time(evs[-1]))
        ops.reload_switches()
        es = torch.empty(0, dtype=dt).element_size()
        out = {}
        for r in ROUTES:
            ms = statistics.median(tot[r])
            out[r] = dict(ms_per_step_median=round(ms, 4), ms_min=round(min(tot[r]), 4), ms_max=round(max(tot[r]), 4),
                          G_elem_per_s=round(elems / ms / 1e6, 2))
        out['native']['bytes_per_elem'] = 3 * es
        out['native']['TB_per_s'] = round(elems * 3 * es / (out['native']['ms_per_step_median'] * 1e-3) / 1e12, 3)
        classes = {}
        for i, L in enumerate(layers):
            key = '%dx%dx%d' % (L['shape'][1], L['shape'][2], L['shape'][3])
            c = classes.setdefault(key, dict(layers=0, **{r: 0.0 for r in ROUTES}))
            c['layers'] += 1
            for r in ROUTES:
                c[r] += per[r][i] / a.steps * 1e3
        for c in classes.values():
            for r in ROUTES:
                c[r] = round(c[r], 1)
        # native is slower than the parent route only beyond the spread both report
        slower = out['native']['ms_min'] > out['parent']['ms_max']
        res[name] = dict(routes=out, native_over_parent=round(out['native']['ms_per_step_median'] / out['parent']['ms_per_step_median'], 4),
                         native_over_nchw=round(out['native']['ms_per_step_median'] / out['nchw']['ms_per_step_median'], 4),
                         native_slower_than_parent_beyond_spread=bool(slower), classes_us=classes,
                         classes_native_slower_than_parent=[k for k, c in classes.items() if c['native'] > c['parent']],
                         largest_layer_contract=bool(exact), native_no_copies=bool(no_copy), elements=elems)
        del layers
        torch.cuda.empty_cache()
    print(json.dumps(dict(workload='resnet50 b%d -sm use -c laplace -baa -bca int%d (53 conv outputs)' % (a.batch, BITS),
                          steps=a.steps, warmup=a.warmup, device=torch.cuda.get_device_name(0), results=res)))
    if not all(r['largest_layer_contract'] and r['native_no_copies'] for r in res.values()):
        sys.exit(1)


if __name__ == '__main__':
    main()
