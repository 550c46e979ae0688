#!/usr/bin/env python3
"""The stored-code format on channels_last storage over the 53 ResNet-50 conv outputs of bench.py's headline
workload as dense channels_last tensors, four legs timed in one process, alternating step by step:
    native_u4  the pack pass in its config 2 form: uniform 4 bits, config 2's table and extrema (ops.quantize_packed_nhwc);
    native_ba  the pack pass in its config 3 form: the bit-allocated widths and table of -c laplace -baa;
    copy_ba    the route without it: x.float().contiguous() (for fp32 only the transpose), then ops.quantize_packed with the same
               table and widths - the NCHW stream, the only one the library had;
    qdq        the channels_last Q/DQ alone (k_cl_qdq through ops.pc_qdq) with the same table: the rate yardstick.
The tables and layouts are computed once, outside the timed region (the one-call fronts add the statistics launches the other
benchmarks time).  Per leg the median, minimum and maximum step time of --steps steps after --warmup (HIP events) and the times per
class of layer (channels x extent).  Before anything is timed the largest layer is checked against the contract: no layout copy,
and the round trip equals pc_qdq on the channels_last tensor bit for bit.  Prints one JSON line; exit status 1 if that check fails.

    tools/bench_channels_last_packed.py [--batch 512] [--steps 10] [--warmup 3] [--dtypes float32,bfloat16]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = ('native_u4', 'native_ba', 'copy_ba', 'qdq')
BITS = 4


def run_leg(ops, leg, L):
    xc = L['xc']
    if leg == 'native_u4':
        return ops.quantize_packed_nhwc(xc, L['qp2'], BITS, mm=L['mm'], out=L['buf'], coloff=L['co4'])
    if leg == 'native_ba':
        return ops.quantize_packed_nhwc(xc, L['qp3'], L['bits'], out=L['buf'], coloff=L['coba'])
    if leg == 'copy_ba':
        return ops.quantize_packed(xc.float().contiguous(), L['qp3'], L['bits'], out=L['buf2'], rowoff=L['rowoff'])
    N, C, H, W = L['shape']
    return ops.pc_qdq(xc, N, C, H * W, L['qp3'], out=L['yc'])


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--batch', type=int, default=512)
    p.add_argument('--steps', type=int, default=10)
    p.add_argument('--warmup', type=int, default=3)
    p.add_argument('--dtypes', default='float32,bfloat16')
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_channels_last_packed.py needs a GPU')
    from cnn_quantization_amd import _lib as Lib, ops
    import bench
    dev = torch.device('cuda')
    res = {}
    for name in a.dtypes.split(','):
        dt = getattr(torch, name)
        layers = []
        for W in bench.build_workload(a.batch, dev):
            xc = W['x'].to(dt).to(memory_format=torch.channels_last)
            shape = list(xc.shape)
            half = W['half']
            del W
            C = shape[1]
            _, p2 = ops.minmax_quantize_packed_nhwc(xc, BITS, positive=half)
            _, p3 = ops.aciq_quantize_packed_nhwc(xc, BITS, positive=half, clip='laplace', bit_alloc=True)
            bits = p3['diag'][Lib.DIAG_BITS].contiguous()
            layers.append(dict(xc=xc, yc=torch.empty_like(xc), shape=shape, qp2=p2['qp'], mm=p2['mm'], co4=p2['coloff'],
                               qp3=p3['qp'].contiguous(), bits=bits, coba=p3['coloff'],
                               rowoff=ops.packed_layout(bits, shape[2] * shape[3]),
                               buf=torch.empty(ops.packed_capacity_nhwc(shape), dtype=torch.uint8, device=dev),
                               buf2=torch.empty(ops.packed_capacity(shape), dtype=torch.uint8, device=dev)))
        torch.cuda.empty_cache()
        elems = sum(L['xc'].numel() for L in layers)
        big = max(range(len(layers)), key=lambda i: layers[i]['xc'].numel())

        def step(leg, evs=None):
            for i, L in enumerate(layers):
                if evs is not None:
                    evs[i].record()
                run_leg(ops, leg, L)
            if evs is not None:
                evs[-1].record()

        L = layers[big]
        before = ops.LAYOUT_COPIES
        N, C, H, W = L['shape']
        exact = True
        for leg, qp, co in (('native_u4', L['qp2'], L['co4']), ('native_ba', L['qp3'], L['coba'])):
            run_leg(ops, leg, L)
            y = ops.dequantize_packed_nhwc(L['buf'], L['shape'], dt, qp, co)
            exact = exact and torch.equal(y, ops.pc_qdq(L['xc'], N, C, H * W, qp))
            del y
        no_copy = ops.LAYOUT_COPIES == before
        used = sum(int(L['coba'][-1].item() + 31) // 32 * 4 * (L['xc'].numel() // L['shape'][1]) for L in layers)
        torch.cuda.empty_cache()
        for _ in range(a.warmup):
            for r in LEGS:
                step(r)
        torch.cuda.synchronize()
        per = {r: [0.0] * len(layers) for r in LEGS}
        tot = {r: [] for r in LEGS}
        for _ in range(a.steps):
            for r in LEGS:
                evs = [torch.cuda.Event(enable_timing=True) for _ in range(len(layers) + 1)]
                step(r, evs)
                torch.cuda.synchronize()
                for i in range(len(layers)):
                    per[r][i] += evs[i].elapsed_time(evs[i + 1])
                tot[r].append(evs[0].elapsed_time(evs[-1]))
        out = {}
        for r in LEGS:
            ms = statistics.median(tot[r])
            out[r] = dict(ms_per_step_median=round(ms, 4), ms_min=round(min(tot[r]), 4), ms_max=round(max(tot[r]), 4),
                          G_elem_per_s=round(elems / ms / 1e6, 2))
        classes = {}
        for i, L in enumerate(layers):
            key = '%dx%dx%d' % (L['shape'][1], L['shape'][2], L['shape'][3])
            c = classes.setdefault(key, dict(layers=0, **{r: 0.0 for r in LEGS}))
            c['layers'] += 1
            for r in LEGS:
                c[r] += per[r][i] / a.steps * 1e3
        for c in classes.values():
            for r in LEGS:
                c[r] = round(c[r], 1)
        res[name] = dict(legs=out, native_ba_over_copy=round(out['native_ba']['ms_per_step_median'] / out['copy_ba']['ms_per_step_median'], 4),
                         native_ba_over_qdq=round(out['native_ba']['ms_per_step_median'] / out['qdq']['ms_per_step_median'], 4),
                         native_u4_over_qdq=round(out['native_u4']['ms_per_step_median'] / out['qdq']['ms_per_step_median'], 4),
                         native_slower_than_copy_beyond_spread=bool(out['native_ba']['ms_min'] > out['copy_ba']['ms_max']),
                         classes_us=classes, classes_native_slower_than_copy=[k for k, c in classes.items() if c['native_ba'] > c['copy_ba']],
                         largest_layer_contract=bool(exact), native_no_copies=bool(no_copy), elements=elems,
                         stored_bytes_per_elem_ba=round(used / elems, 4))
        del layers
        torch.cuda.empty_cache()
    print(json.dumps(dict(workload='resnet50 b%d stored codes, int%d and -c laplace -baa (53 conv outputs)' % (a.batch, BITS), steps=a.steps,
                          warmup=a.warmup, device=torch.cuda.get_device_name(0), results=res)))
    if not all(r['largest_layer_contract'] and r['native_no_copies'] for r in res.values()):
        sys.exit(1)


if __name__ == '__main__':
    main()
