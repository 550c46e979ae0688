#!/usr/bin/env python3
"""Config 2 (per-channel int4, dynamic min/max) over the 53 ResNet-50 conv outputs of bench.py's headline workload, in three
routes timed in one process, alternating step by step:
    nchw    the NCHW tensors (today's path);
    copy    the same values as channels_last tensors through the copy route (CNNQ_NHWC=0: x.contiguous(), then the NCHW
            path; the NCHW result's conversion back, which a channels_last model pays downstream, is not counted);
    native  the channels_last tensors on the NHWC kernels (cnnq_pc_minmax_qdq_nhwc), channels_last result.
Mean step time of --steps steps after --warmup (HIP events), per-layer times, the element rate and the fraction of 8 TB/s on
the bytes each route moves at least (nchw: read x, write y; copy: + read and write the copy; native: x read twice, y written
once).  The largest layer of every dtype is checked against the contract (native == nchw on x.contiguous(), bit for bit)
before anything is timed.  Prints one JSON line.

    tools/bench_channels_last.py [--batch 512] [--steps 10] [--warmup 3] [--dtypes float32,bfloat16]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

ROUTES = ('nchw', 'copy', 'native')


def same(a, b):
    a, b = a.contiguous(), b.contiguous()
    na, nb = torch.isnan(a), torch.isnan(b)
    if not torch.equal(na, nb):
        return False
    iv = torch.int32 if a.dtype == torch.float32 else torch.int16
    return torch.equal(a.view(iv)[~na], b.view(iv)[~nb])


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--batch', type=int, default=512)
    p.add_argument('--steps', type=int, default=10)
    p.add_argument('--warmup', type=int, default=3)
    p.add_argument('--dtypes', default='float32,bfloat16')
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_channels_last.py needs a GPU')
    from cnn_quantization_amd import ops
    dev = torch.device('cuda')
    res = {}
    for name in a.dtypes.split(','):
        dt = getattr(torch, name)
        layers = []
        for L in bench.build_workload(a.batch, dev):
            x = L['x'].to(dt)
            xc = x.to(memory_format=torch.channels_last)
            layers.append(dict(x=x, y=torch.empty_like(x), xc=xc, yc=torch.empty_like(xc), half=L['half'],
                               shape=list(x.shape)))
            del L
        torch.cuda.empty_cache()
        elems = sum(L['x'].numel() for L in layers)
        big = max(range(len(layers)), key=lambda i: layers[i]['x'].numel())

        def step(route, evs=None):
            ops._NHWC = route != 'copy'
            for i, L in enumerate(layers):
                if evs is not None:
                    evs[i].record()
                if route == 'nchw':
                    ops.act_qdq_per_channel(L['x'], 4, positive=L['half'], out=L['y'])
                elif route == 'copy':
                    ops.act_qdq_per_channel(L['xc'], 4, positive=L['half'], out=L['y'])
                else:
                    ops.act_qdq_per_channel(L['xc'], 4, positive=L['half'], out=L['yc'])
            if evs is not None:
                evs[-1].record()

        L = layers[big]
        step('native')
        before = ops.LAYOUT_COPIES
        step('native')
        no_copy = ops.LAYOUT_COPIES == before
        native = L['yc'].clone()
        step('nchw')
        exact = same(native, L['y']) and same(native, ops.act_qdq_per_channel(L['xc'].contiguous(), 4, positive=L['half']))
        del native
        for _ in range(a.warmup):
            for r in ROUTES:
                step(r)
        torch.cuda.synchronize()
        per = {r: [0.0] * len(layers) for r in ROUTES}
        tot = {r: 0.0 for r in ROUTES}
        for _ in range(a.steps):
            for r in ROUTES:
                evs = [torch.cuda.Event(enable_timing=True) for _ in range(len(layers) + 1)]
                step(r, evs)
                torch.cuda.synchronize()
                for i in range(len(layers)):
                    per[r][i] += evs[i].elapsed_time(evs[i + 1])
                tot[r] += evs[0].elapsed_time(evs[-1])
        ops.reload_switches()
        es = torch.empty(0, dtype=dt).element_size()
        bpe = dict(nchw=2 * es, copy=4 * es, native=3 * es)
        out = {}
        for r in ROUTES:
            ms = tot[r] / a.steps
            out[r] = dict(ms_per_step=round(ms, 4), G_elem_per_s=round(elems / ms / 1e6, 2), bytes_per_elem=bpe[r],
                          frac_of_8TBs=round(elems * bpe[r] / (ms * 1e-3) / 8e12, 4))
        layer_rows = []
        for i, L in enumerate(layers):
            layer_rows.append(dict(shape=L['shape'], **{r: round(per[r][i] / a.steps * 1e3, 1) for r in ROUTES}))
        slower = [i for i, row in enumerate(layer_rows) if row['native'] > row['copy']]
        res[name] = dict(routes=out, native_over_copy=round(out['native']['ms_per_step'] / out['copy']['ms_per_step'], 4),
                         native_over_nchw=round(out['native']['ms_per_step'] / out['nchw']['ms_per_step'], 4),
                         layers_us=layer_rows, layers_native_slower_than_copy=slower, largest_layer_exact=bool(exact),
                         native_no_copies=bool(no_copy), elements=elems)
        del layers
        torch.cuda.empty_cache()
    print(json.dumps(dict(workload='resnet50 b%d config 2 (53 conv outputs)' % a.batch, steps=a.steps, warmup=a.warmup,
                          results=res)))
    if not all(r['largest_layer_exact'] and r['native_no_copies'] for r in res.values()):
        sys.exit(1)


if __name__ == '__main__':
    main()
