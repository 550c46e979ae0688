#!/usr/bin/env python3
"""The stored-code format on contiguous bf16 / fp16 storage over the 53 ResNet-50 conv outputs of bench.py's
headline workload, seven legs timed in one process, alternating step by step:
    native_u4   the pack pass with config 2's table at uniform 4 bits (ops.quantize_packed_half);
    native_ba   the pack pass with the bit-allocated widths and table of -c laplace -baa;
    upcast_u4 / upcast_ba   the route without it: ops.quantize_packed(x.float(), ...) with the same table, the upcast timed with it;
    qdq         k_h_qdq alone (ops.pc_qdq on the half tensor) with the same table: the rate yardstick;
    unpack      the decoder (ops.dequantize_packed_half) on the bit-allocated buffer;
    upcast_unpack   ops.dequantize_packed into fp32, then .to(dtype).
The tables and layouts are computed once, outside the timed region.  Per leg the median, minimum and maximum step time of --steps
steps after --warmup (HIP events), and per class of layer (channels x extent) the median with minimum - maximum of the native and
upcast bit-allocated legs: a class whose native minimum is not below its upcast maximum is listed under classes_not_faster - the
candidates for a 0 in cnnq_pc_route_packed_dt.  Before anything is timed the largest layer is checked: no layout copy, the bytes of
both routes equal.  Prints one JSON line; exit status 1 if that check fails.

    tools/bench_half_packed.py [--batch 512] [--steps 10] [--warmup 3] [--dtypes bfloat16,float16]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = ('native_u4', 'native_ba', 'upcast_u4', 'upcast_ba', 'qdq', 'unpack', 'upcast_unpack')
BITS = 4


def run_leg(ops, leg, L):
    x = L['x']
    if leg == 'native_u4':
        return ops.quantize_packed_half(x, L['qp2'], L['bits4'], out=L['buf'], rowoff=L['ro4'])
    if leg == 'native_ba':
        return ops.quantize_packed_half(x, L['qp3'], L['bits'], out=L['buf'], rowoff=L['roba'])
    if leg == 'upcast_u4':
        return ops.quantize_packed(x.float(), L['qp2'], L['bits4'], out=L['buf2'], rowoff=L['ro4'])
    if leg == 'upcast_ba':
        return ops.quantize_packed(x.float(), L['qp3'], L['bits'], out=L['buf2'], rowoff=L['roba'])
    if leg == 'unpack':
        return ops.dequantize_packed_half(L['buf'], L['shape'], x.dtype, L['qp3'], L['bits'], L['roba'], out=L['y'])
    if leg == 'upcast_unpack':
        return ops.dequantize_packed(L['buf'], L['shape'], L['qp3'], L['bits'], L['roba']).to(x.dtype)
    N, C, H, W = L['shape']
    return ops.pc_qdq(x, N, C, H * W, L['qp3'], out=L['y'])


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--batch', type=int, default=512)
    p.add_argument('--steps', type=int, default=10)
    p.add_argument('--warmup', type=int, default=3)
    p.add_argument('--dtypes', default='bfloat16,float16')
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_half_packed.py needs a GPU')
    from cnn_quantization_amd import _lib as Lib, ops
    import bench
    dev = torch.device('cuda')
    res = {}
    for name in a.dtypes.split(','):
        dt = getattr(torch, name)
        layers = []
        for W in bench.build_workload(a.batch, dev):
            x = W['x'].to(dt)
            half = W['half']
            del W
            shape = list(x.shape)
            C, HW = shape[1], shape[2] * shape[3]
            _, ro4, qp2 = ops.minmax_quantize_packed_half(x, BITS, positive=half)
            _, roba, p3 = ops.aciq_quantize_packed_half(x, BITS, positive=half, clip='laplace', bit_alloc=True)
            layers.append(dict(x=x, y=torch.empty_like(x), shape=shape, qp2=qp2, ro4=ro4, qp3=p3['qp'].contiguous(), roba=roba,
                               bits=p3['diag'][Lib.DIAG_BITS].contiguous(), bits4=torch.full((C,), float(BITS), device=dev),
                               buf=torch.empty(ops.packed_capacity(shape), dtype=torch.uint8, device=dev),
                               buf2=torch.empty(ops.packed_capacity(shape), dtype=torch.uint8, device=dev)))
        torch.cuda.empty_cache()
        elems = sum(L['x'].numel() for L in layers)
        big = max(range(len(layers)), key=lambda i: layers[i]['x'].numel())

        def step(leg, evs=None):
            for i, L in enumerate(layers):
                if evs is not None:
                    evs[i].record()
                run_leg(ops, leg, L)
            if evs is not None:
                evs[-1].record()

        L = layers[big]
        before = ops.LAYOUT_COPIES
        same = True
        for nat, up in (('native_u4', 'upcast_u4'), ('native_ba', 'upcast_ba')):
            L['buf'].zero_()
            L['buf2'].zero_()
            run_leg(ops, nat, L)
            copies = ops.LAYOUT_COPIES
            run_leg(ops, up, L)
            same = same and torch.equal(L['buf'], L['buf2'])
        no_copy = copies == before
        for _ in range(a.warmup):
            for r in LEGS:
                step(r)
        torch.cuda.synchronize()
        per = {r: [[] for _ in layers] for r in LEGS}
        tot = {r: [] for r in LEGS}
        for _ in range(a.steps):
            for r in LEGS:
                evs = [torch.cuda.Event(enable_timing=True) for _ in range(len(layers) + 1)]
                step(r, evs)
                torch.cuda.synchronize()
                for i in range(len(layers)):
                    per[r][i].append(evs[i].elapsed_time(evs[i + 1]))
                tot[r].append(evs[0].elapsed_time(evs[-1]))
        out = {}
        for r in LEGS:
            ms = statistics.median(tot[r])
            out[r] = dict(ms_per_step_median=round(ms, 4), ms_min=round(min(tot[r]), 4), ms_max=round(max(tot[r]), 4),
                          G_elem_per_s=round(elems / ms / 1e6, 2))
        classes = {}
        for i, L in enumerate(layers):
            key = '%dx%dx%d' % (L['shape'][1], L['shape'][2], L['shape'][3])
            c = classes.setdefault(key, dict(layers=0, **{r: [0.0] * a.steps for r in LEGS}))
            c['layers'] += 1
            for r in LEGS:
                c[r] = [s + t * 1e3 for s, t in zip(c[r], per[r][i])]
        for c in classes.values():
            for r in LEGS:
                c[r] = [round(statistics.median(c[r]), 1), round(min(c[r]), 1), round(max(c[r]), 1)]      # us: median, min, max
        ratio = lambda u, v: round(out[u]['ms_per_step_median'] / out[v]['ms_per_step_median'], 4)
        res[name] = dict(legs=out, native_ba_over_upcast=ratio('native_ba', 'upcast_ba'), native_u4_over_upcast=ratio('native_u4', 'upcast_u4'),
                         native_ba_over_qdq=ratio('native_ba', 'qdq'), unpack_over_upcast=ratio('unpack', 'upcast_unpack'),
                         classes_us_median_min_max=classes,
                         classes_not_faster=[k for k, c in classes.items() if c['native_ba'][1] >= c['upcast_ba'][2]],
                         largest_layer_same_bytes=bool(same), native_no_copies=bool(no_copy), elements=elems)
        del layers
        torch.cuda.empty_cache()
    print(json.dumps(dict(workload='resnet50 b%d stored codes on bf16 / fp16, int%d and -c laplace -baa (53 conv outputs)' % (a.batch, BITS),
                          steps=a.steps, warmup=a.warmup, device=torch.cuda.get_device_name(0), results=res)))
    if not all(r['largest_layer_same_bytes'] and r['native_no_copies'] for r in res.values()):
        sys.exit(1)


if __name__ == '__main__':
    main()
