#!/usr/bin/env python3
"""The depthwise convolution on the stored codes on MobileNetV2's distinct depthwise layers - 3 x 3, padding 1,
stride 1 and 2, from 112 x 112 x 32 to 7 x 7 x 960 - with ReLU, at the given batches, u8 and pack4 (operands and output alike), two
legs timed in one process, alternating call by call:
    codes    ops.dwconv_codes_q: codes in, codes out, one launch, the output held;
    former   what a holder of codes did without it: ops.dequantize_packed_nhwc, torch conv2d(groups=C) on the held fp32 weight,
             relu_, ops.quantize_packed_nhwc at a uniform 8 / 4 bits, with the fp32 buffer, the packed buffer, the tables and coloff
             held.
Per leg the median, minimum and maximum time of --steps calls after --warmup (HIP events), and for `codes` the achieved rate (input +
output bytes) / median.  A case whose `codes` median is not below the `former` median is listed under not_faster; run the command
twice and count a case as faster only when its slower `codes` median beats the faster `former` median.  Before anything is timed the
bytes are compared: `codes` must equal ReLU and the quantizer on ops.dwconv_codes' own fp32 output bit for bit (exit status 1 if
not); against `former`, whose fp32 convolution rounds every product, the share of equal bytes and the largest code difference are
reported (a difference above 1 fails too).  Prints one JSON line.

    tools/bench_dwconv_codes.py [--batches 64,1] [--steps 20] [--warmup 5]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (H = W, C, stride)
LAYERS = ((112, 32, 1), (112, 96, 2), (56, 144, 1), (56, 144, 2), (28, 192, 1), (28, 192, 2), (14, 384, 1), (14, 576, 1), (14, 576, 2), (7, 960, 1))


def pack(c, fmt):
    return (c if fmt == 'u8' else c[..., 0::2] | (c[..., 1::2] << 4)).contiguous()


def unpack(b, fmt):
    return b if fmt == 'u8' else torch.stack([b & 15, b >> 4], -1).flatten(-2)


def make(ops, fmt, N, H, C, s, dev, gen):
    top, bits = (255, 8) if fmt == 'u8' else (15, 4)
    x = torch.randint(0, top + 1, (N, H, H, C), generator=gen, dtype=torch.uint8)
    w = torch.randint(0, top + 1, (3, 3, C), generator=gen, dtype=torch.uint8)
    OH = (H - 1) // s + 1
    L = dict(fmt=fmt, bits=bits, s=s, C=C, xq=pack(x, fmt).to(dev), wq=pack(w, fmt).to(dev))
    L['qpx'] = torch.tensor([[0.05], [top / 3 + 0.37], [float(top)]], device=dev)
    qpw = torch.stack([torch.linspace(0.01, 0.03, C), torch.linspace(top / 2 - 2.3, top / 2 + 2.3, C), torch.full((C,), float(top))])
    L['qpw'], L['bias'] = qpw.to(dev), torch.linspace(-1, 1, C).to(dev)
    L['w32'] = ((w.float() - qpw[1]) * qpw[0]).permute(2, 0, 1).unsqueeze(1).contiguous().to(dev)
    # the output table: ReLU's range [0, 6 sigma] of the decoded products, zero point 0.37
    sigma = 0.05 * 0.02 * (top / 3) * (top / 4) * 3
    L['qpy'] = torch.tensor([[6 * sigma / top], [0.37], [float(top)]], device=dev)
    L['x32'] = torch.empty((N, C, H, H), dtype=torch.float32, device=dev, memory_format=torch.channels_last)
    L['qpc'], L['coloff'] = L['qpx'].expand(3, C).contiguous(), ops.packed_layout_nhwc(bits, C)
    L['qpyc'] = L['qpy'].expand(3, C).contiguous()
    L['out'] = torch.empty((N, OH, OH, L['xq'].shape[3]), dtype=torch.uint8, device=dev)
    L['packed'] = torch.empty(L['out'].numel(), dtype=torch.uint8, device=dev)
    return L


def run_leg(ops, leg, L):
    if leg == 'codes':
        return ops.dwconv_codes_q(L['xq'], L['wq'], L['qpx'], L['qpw'], L['qpy'], bias=L['bias'], relu=True, stride=L['s'], padding=1,
                                  x_format=L['fmt'], w_format=L['fmt'], y_format=L['fmt'], out=L['out'])
    x = ops.dequantize_packed_nhwc(L['xq'].view(-1), L['x32'].shape, torch.float32, L['qpc'], L['coloff'], out=L['x32'])
    y = torch.nn.functional.conv2d(x, L['w32'], L['bias'], L['s'], 1, 1, L['C']).relu_().contiguous(memory_format=torch.channels_last)
    return ops.quantize_packed_nhwc(y, L['qpyc'], L['bits'], out=L['packed'], coloff=L['coloff'])[0]


def check(ops, L):
    """(the contract holds, share of bytes equal to the former route's, largest code difference to it)"""
    new = run_leg(ops, 'codes', L).clone()
    y32 = ops.dwconv_codes(L['xq'], L['wq'], L['qpx'], L['qpw'], bias=L['bias'], stride=L['s'], padding=1, x_format=L['fmt'], w_format=L['fmt'])
    own = ops.quantize_packed_nhwc(y32.relu_(), L['qpyc'], L['bits'], coloff=L['coloff'])[0]
    old = run_leg(ops, 'former', L)
    diff = (unpack(new.view(-1), L['fmt']).int() - unpack(old.view(-1), L['fmt']).int()).abs()
    return bool(torch.equal(new.view(-1), own.view(-1))), float((diff == 0).float().mean()), int(diff.max())


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--batches', default='64,1')
    p.add_argument('--steps', type=int, default=20)
    p.add_argument('--warmup', type=int, default=5)
    a = p.parse_args()
    LEGS = ('codes', 'former')
    if not torch.cuda.is_available():
        sys.exit('bench_dwconv_codes.py needs a GPU')
    from cnn_quantization_amd import ops
    dev = torch.device('cuda')
    gen = torch.Generator().manual_seed(1234)
    res, ok = {}, True
    for N in (int(b) for b in a.batches.split(',')):
        for H, C, s in LAYERS:
            for fmt in ('u8', 'pack4'):
                L = make(ops, fmt, N, H, C, s, dev, gen)
                same, share, worst = check(ops, L)
                ok = ok and same and worst <= 1
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
                res['%dx%dx%d s%d b%d %s' % (H, H, C, s, N, fmt)] = {
                    'us_median_min_max': us, 'codes_over_former': round(us['codes'][0] / us['former'][0], 4), 'bytes_are_todays_route': same,
                    'equal_to_former': round(share, 5), 'max_code_diff_to_former': worst,
                    'codes_GB_per_s': round((L['xq'].numel() + L['out'].numel()) / us['codes'][0] / 1e3, 1)}
                del L
                torch.cuda.empty_cache()
    print(json.dumps(dict(workload='depthwise 3 x 3 + ReLU on stored codes: MobileNetV2 layers', steps=a.steps, warmup=a.warmup,
                          device=torch.cuda.get_device_name(0), results=res,
                          not_faster=[k for k, r in res.items() if r['us_median_min_max']['codes'][0] >= r['us_median_min_max']['former'][0]])))
    if not ok:
        sys.exit(1)


if __name__ == '__main__':
    main()
