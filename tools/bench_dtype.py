#!/usr/bin/env python3
"""Config 2 (per-channel int4, dynamic min/max) over the 53 ResNet-50 conv outputs of bench.py's headline workload, in
float32, bfloat16 and float16, in one process: mean step time of --steps steps after --warmup (HIP events), the element
rate and the fraction of 8 TB/s on the bytes the path must move (one read and one write of each element: 8 B/elem for
float32, 4 B/elem for the 2-byte types).  The largest layer of every dtype is checked against the contract
    y == fp32_path(x.float()).to(x.dtype)   (bit for bit, NaN == NaN)
before anything is timed.  Prints one JSON line.

    tools/bench_dtype.py [--batch 512] [--steps 20] [--warmup 5] [--dtypes float32,bfloat16,float16]"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def same(a, b):
    na, nb = torch.isnan(a), torch.isnan(b)
    if not torch.equal(na, nb):
        return False
    if a.dtype == torch.float32:
        return torch.equal(a.view(torch.int32)[~na], b.view(torch.int32)[~nb])
    return torch.equal(a.view(torch.int16)[~na], b.view(torch.int16)[~nb])


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--batch', type=int, default=512)
    p.add_argument('--steps', type=int, default=20)
    p.add_argument('--warmup', type=int, default=5)
    p.add_argument('--dtypes', default='float32,bfloat16,float16')
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_dtype.py needs a GPU')
    from cnn_quantization_amd import ops
    dev = torch.device('cuda')
    base = bench.build_workload(a.batch, dev)
    elems = sum(L['x'].numel() for L in base)
    big = max(range(len(base)), key=lambda i: base[i]['x'].numel())
    res = {}
    for name in a.dtypes.split(','):
        dt = getattr(torch, name)
        if dt == torch.float32:
            layers = base
        else:
            layers = [dict(L, x=L['x'].to(dt), y=torch.empty(L['x'].shape, dtype=dt, device=dev)) for L in base]
        bench.run_step(ops, layers, None)
        L = layers[big]
        ref = ops.act_qdq_per_channel(L['x'].float(), 4, positive=L['half']).to(dt)
        exact = same(L['y'], ref)
        del ref
        for _ in range(a.warmup):
            bench.run_step(ops, layers, None)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.steps):
            bench.run_step(ops, layers, None)
        t1.record()
        torch.cuda.synchronize()
        ms = t0.elapsed_time(t1) / a.steps
        bpe = 2 * torch.empty(0, dtype=dt).element_size()
        res[name] = dict(ms_per_step=round(ms, 4), G_elem_per_s=round(elems / ms / 1e6, 2),
                         frac_of_8TBs=round(elems * bpe / (ms * 1e-3) / 8e12, 4), bytes_per_elem=bpe,
                         largest_layer_exact=bool(exact))
        if dt != torch.float32:
            del layers
    out = dict(workload='resnet50 b%d config 2 (53 conv outputs)' % a.batch, elements=elems, steps=a.steps, warmup=a.warmup,
               results=res)
    if 'float32' in res:
        for name in res:
            if name != 'float32':
                out['%s_over_float32' % name] = round(res[name]['ms_per_step'] / res['float32']['ms_per_step'], 4)
    print(json.dumps(out))
    if not all(r['largest_layer_exact'] for r in res.values()):
        sys.exit(1)


if __name__ == '__main__':
    main()
