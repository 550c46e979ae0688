#!/usr/bin/env python3
"""Pooling on the stored codes on ResNet-50's two pools - the stem's MaxPool2d(3, 2, 1) on N x 112 x 112 x 64
and the global average on N x 7 x 7 x 2048 - at the given batches, u8 and pack4, two legs timed in one process, alternating call by
call:
    codes    ops.max_pool_codes / ops.avg_pool_codes_q: codes in, codes out, one launch, the output held;
    former   what a holder of codes did without them: ops.dequantize_packed_nhwc, torch max_pool2d / mean over the pixels,
             ops.quantize_packed_nhwc at a uniform 8 / 4 bits, with the fp32 buffer, the packed buffer, the tables and coloff held.
Per leg the median, minimum and maximum time of --steps calls after --warmup (HIP events); for the maximum also the achieved rate
(input + output bytes) / median.  A case whose `codes` median is not below the `former` median is listed under not_faster; run the
command twice and count a case as faster only when its slower `codes` median beats the faster `former` median.  Before anything is
timed the results are checked - on decoded values, not bytes (quantize(dequantize(c)) == c is no contract): the two routes' decoded
maxima are equal; ops.avg_pool_codes equals ((S / HW - zx) * sx).float() of fp64 tensors computed on the CPU.  Prints one JSON line;
exit status 1 if a check fails.

    tools/bench_pool_codes.py [--batches 64,1] [--steps 20] [--warmup 5]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = (('stem_maxpool', 'max', 112, 64), ('final_avgpool', 'avg', 7, 2048))


def make(ops, kind, fmt, N, H, C, dev, gen):
    top = 255 if fmt == 'u8' else 15
    c = torch.randint(0, top + 1, (N, H, H, C), generator=gen, dtype=torch.uint8)
    L = dict(kind=kind, fmt=fmt, codes=c, xq=(c if fmt == 'u8' else c[..., 0::2] | (c[..., 1::2] << 4)).contiguous().to(dev), bits=8 if fmt == 'u8' else 4)
    L['qpx'] = torch.tensor([[0.05], [top / 3 + 0.37], [float(top)]], device=dev)
    L['x32'] = torch.empty((N, C, H, H), dtype=torch.float32, device=dev, memory_format=torch.channels_last)
    L['qpc'], L['coloff'] = L['qpx'].expand(3, C).contiguous(), ops.packed_layout_nhwc(L['bits'], C)
    if kind == 'max':
        L['out'] = torch.empty((N, H // 2, H // 2, L['xq'].shape[3]), dtype=torch.uint8, device=dev)
    else:   # the output table: the means lie near the middle code; [N, C] is quantized as the channels_last tensor [1, C / 2, 2 N, 1]
        L['qpy'] = torch.tensor([[0.05], [top / 2 + 0.37], [float(top)]], device=dev)
        L['qph'], L['coloff_h'] = L['qpy'].expand(3, C // 2).contiguous(), ops.packed_layout_nhwc(L['bits'], C // 2)
        L['out'] = torch.empty((N, L['xq'].shape[3]), dtype=torch.uint8, device=dev)
    L['packed'] = torch.empty(L['out'].numel(), dtype=torch.uint8, device=dev)
    return L


def run_leg(ops, leg, L):
    if leg == 'codes':
        if L['kind'] == 'max':
            return ops.max_pool_codes(L['xq'], 3, 2, 1, x_format=L['fmt'], out=L['out'])
        return ops.avg_pool_codes_q(L['xq'], L['qpx'], L['qpy'], x_format=L['fmt'], y_format=L['fmt'], out=L['out'])
    x = ops.dequantize_packed_nhwc(L['xq'].view(-1), L['x32'].shape, torch.float32, L['qpc'], L['coloff'], out=L['x32'])
    if L['kind'] == 'max':
        return ops.quantize_packed_nhwc(torch.nn.functional.max_pool2d(x, 3, 2, 1), L['qpc'], L['bits'], out=L['packed'], coloff=L['coloff'])[0]
    N, C = x.shape[:2]
    y = x.mean((2, 3)).view(1, 2 * N, 1, C // 2).permute(0, 3, 1, 2)
    return ops.quantize_packed_nhwc(y, L['qph'], L['bits'], out=L['packed'], coloff=L['coloff_h'])[0]


def check(ops, L):
    """Decoded values: the two routes' maxima; the fp32 average against the fp64 expression."""
    if L['kind'] == 'max':
        new = run_leg(ops, 'codes', L)
        shape = (new.shape[0], L['codes'].shape[3]) + tuple(new.shape[1:3])
        dec = lambda b: ops.dequantize_packed_nhwc(b.reshape(-1), shape, torch.float32, L['qpc'], L['coloff'])
        return bool(torch.equal(dec(new), dec(run_leg(ops, 'former', L).clone())))
    N, H, W, C = L['codes'].shape
    S = L['codes'].reshape(N, H * W, C).sum(1, dtype=torch.int64).double()
    want = ((S / (H * W) - L['qpx'][1].cpu().double()) * L['qpx'][0].cpu().double()).float()
    return bool(torch.equal(ops.avg_pool_codes(L['xq'], L['qpx'], x_format=L['fmt']).cpu(), want))


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--batches', default='64,1')
    p.add_argument('--steps', type=int, default=20)
    p.add_argument('--warmup', type=int, default=5)
    a = p.parse_args()
    LEGS = ('codes', 'former')
    if not torch.cuda.is_available():
        sys.exit('bench_pool_codes.py needs a GPU')
    from cnn_quantization_amd import ops
    dev = torch.device('cuda')
    gen = torch.Generator().manual_seed(1234)
    res, ok = {}, True
    for N in (int(b) for b in a.batches.split(',')):
        for name, kind, H, C in CASES:
            for fmt in ('u8', 'pack4'):
                L = make(ops, kind, fmt, N, H, C, dev, gen)
                same = check(ops, L)
                ok = ok and same
                for _ in range(a.warmup):
                    for leg in LEGS:
                        run_leg(ops, leg, L)
                torch.cuda.synchronize()
                t = {leg: [] for leg in LEGS}
                for _ in range(a.steps):
                    for leg in LEGS:
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        run_leg(ops, leg, L)
                        e1.record()
                        torch.cuda.synchronize()
                        t[leg].append(e0.elapsed_time(e1) * 1e3)
                us = {leg: [round(statistics.median(t[leg]), 1), round(min(t[leg]), 1), round(max(t[leg]), 1)] for leg in LEGS}
                r = {'us_median_min_max': us, 'codes_over_former': round(us['codes'][0] / us['former'][0], 4), 'results_agree': same}
                if kind == 'max':
                    r['codes_GB_per_s'] = round((L['xq'].numel() + L['out'].numel()) / us['codes'][0] / 1e3, 1)
                res['%s b%d %s' % (name, N, fmt)] = r
                del L
                torch.cuda.empty_cache()
    print(json.dumps(dict(workload='pooling on stored codes: ResNet-50 stem max pool and final average pool', steps=a.steps, warmup=a.warmup,
                          device=torch.cuda.get_device_name(0), results=res,
                          not_faster=[k for k, r in res.items() if r['us_median_min_max']['codes'][0] >= r['us_median_min_max']['former'][0]])))
    if not ok:
        sys.exit(1)


if __name__ == '__main__':
    main()
