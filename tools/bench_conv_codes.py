#!/usr/bin/env python3
"""The integer convolution on the stored codes on ResNet-50's distinct 3 x 3 and 1 x 1 layers, the stride-2
ones included, at the given batches, u8 / u8 and pack4 / pack4, two legs timed in one process, alternating call by call:
    int      ops.conv_codes on the codes, the tap table held (ops.conv_codes_tapsums, outside the timed region);
    former   what a holder of codes did without it: ops.dequantize_u8 / dequantize_pack4 of both operands, then
             torch.nn.functional.conv2d in fp32 on channels_last views.
Per leg the median, minimum and maximum time of --steps calls after --warmup (HIP events); for `int` the int8 operation rate
2 M Cout K / t.  A layer whose `int` median is not below the `former` median is listed under not_faster; run the command twice
and count a layer as faster only when its slower `int` median beats the faster `former` median.  Before anything is timed
the two routes' results are compared on every layer (they differ by the fp32 convolution's rounding).  Prints one JSON line; exit
status 1 if that comparison fails.

--requant times the layer that hands CODES to the next one instead, two other legs:
    q        ops.conv_codes_q with ReLU: codes in, codes out, the tap table held;
    chain    the same bytes without it: ops.conv_codes, torch.relu_, ops.quantize_packed_nhwc at a uniform 8 / 4 bits, coloff held.
The two legs' bytes are compared (they are equal) before anything is timed, and not_faster lists the layers whose `q` median is not
below the `chain` median; the rule of two runs is the same.

--residual times the layer that closes a residual block on ResNet-50's four block-closing 1 x 1 layers, with
ReLU, the tables and taps held, two legs again:
    qadd     ops.conv_codes_q(..., residual=): codes and shortcut codes in, codes out, one call;
    five     the same bytes without it: ops.conv_codes, ops.dequantize_packed_nhwc of the shortcut, add_, relu_,
             ops.quantize_packed_nhwc, every buffer held.
The bytes are compared before anything is timed; not_faster and the rule of two runs as above.

    tools/bench_conv_codes.py [--batches 64,1] [--steps 20] [--warmup 5] [--requant | --residual]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (name, H = W, Cin, Cout, kernel, stride); padding = kernel // 2
LAYERS = (
    ('c2_3x3', 56, 64, 64, 3, 1), ('c3_3x3s2', 56, 128, 128, 3, 2), ('c3_3x3', 28, 128, 128, 3, 1), ('c4_3x3s2', 28, 256, 256, 3, 2),
    ('c4_3x3', 14, 256, 256, 3, 1), ('c5_3x3s2', 14, 512, 512, 3, 2), ('c5_3x3', 7, 512, 512, 3, 1),
    ('c2_1x1_64_64', 56, 64, 64, 1, 1), ('c2_1x1_64_256', 56, 64, 256, 1, 1), ('c2_1x1_256_64', 56, 256, 64, 1, 1),
    ('c3_1x1_256_128', 56, 256, 128, 1, 1), ('c3_1x1_128_512', 28, 128, 512, 1, 1), ('c3_1x1_512_128', 28, 512, 128, 1, 1),
    ('c4_1x1_512_256', 28, 512, 256, 1, 1), ('c4_1x1_256_1024', 14, 256, 1024, 1, 1), ('c4_1x1_1024_256', 14, 1024, 256, 1, 1),
    ('c5_1x1_1024_512', 14, 1024, 512, 1, 1), ('c5_1x1_512_2048', 7, 512, 2048, 1, 1), ('c5_1x1_2048_512', 7, 2048, 512, 1, 1),
    ('c3_down_1x1s2', 56, 256, 512, 1, 2), ('c4_down_1x1s2', 28, 512, 1024, 1, 2), ('c5_down_1x1s2', 14, 1024, 2048, 1, 2),
)
# ... and the 1 x 1 layers that close a block: relu(conv(x) + shortcut)
CLOSING = (('c2_1x1_64_256', 56, 64, 256, 1, 1), ('c3_1x1_128_512', 28, 128, 512, 1, 1), ('c4_1x1_256_1024', 14, 256, 1024, 1, 1),
           ('c5_1x1_512_2048', 7, 512, 2048, 1, 1))


def make(fmt, N, H, Cin, Cout, k, stride, dev, gen):
    qmax = 255 if fmt == 'u8' else 15

    def operand(*shape):
        c = torch.randint(0, qmax + 1, shape, generator=gen, dtype=torch.uint8).to(dev)
        return c if fmt == 'u8' else (c[..., 0::2] | (c[..., 1::2] << 4)).contiguous()
    qpx = torch.tensor([[0.05], [qmax / 2 + 0.25], [float(qmax)]], device=dev)
    qpw = torch.stack([torch.linspace(1e-3, 2e-3, Cout), torch.linspace(qmax / 2 - 3, qmax / 2 + 3, Cout), torch.full((Cout,), float(qmax))]).to(dev)
    return dict(fmt=fmt, dims=(N, H, H, Cin), wdims=(Cout, k, k, Cin), stride=stride, pad=k // 2, xq=operand(N, H, H, Cin), wq=operand(Cout, k, k, Cin),
                qpx=qpx, qpw=qpw, bias=torch.linspace(-1, 1, Cout).to(dev))


def dequantize(ops, L):
    """Both operands as fp32 channels_last tensors through the library's dequantizers: the activation one channel, the weight Cout."""
    (N, H, W, Cin), (Cout, KH, KW, _) = L['dims'], L['wdims']
    if L['fmt'] == 'u8':
        x = ops.dequantize_u8(L['xq'].view(1, 1, -1, 1), L['qpx'])
        w = ops.dequantize_u8(L['wq'].view(1, Cout, -1, 1), L['qpw'])
    else:
        x = ops.dequantize_pack4(L['xq'].view(-1), (1, 1, N * H * W * Cin, 1), L['qpx'])
        w = ops.dequantize_pack4(L['wq'].view(-1), (1, Cout, KH * KW * Cin, 1), L['qpw'])
    return x.view(N, H, W, Cin).permute(0, 3, 1, 2), w.view(Cout, KH, KW, Cin).permute(0, 3, 1, 2)


def run_leg(ops, leg, L):
    if leg == 'int':
        return ops.conv_codes(L['xq'], L['wq'], L['qpx'], L['qpw'], bias=L['bias'], stride=L['stride'], padding=L['pad'], x_format=L['fmt'],
                              w_format=L['fmt'], taps=L['taps'], out=L['y'])
    if leg in ('q', 'chain', 'qadd', 'five'):
        kw = dict(bias=L['bias'], stride=L['stride'], padding=L['pad'], x_format=L['fmt'], w_format=L['fmt'], taps=L['taps'])
        if leg == 'q':
            return ops.conv_codes_q(L['xq'], L['wq'], L['qpx'], L['qpw'], L['qpy'], relu=True, y_format=L['fmt'], out=L['yq'], **kw)
        if leg == 'qadd':
            return ops.conv_codes_q(L['xq'], L['wq'], L['qpx'], L['qpw'], L['qpy'], relu=True, y_format=L['fmt'], out=L['yq'], residual=L['rq'],
                                    qpr=L['qpr'], r_format=L['fmt'], **kw)
        y = ops.conv_codes(L['xq'], L['wq'], L['qpx'], L['qpw'], out=L['y'], **kw)
        if leg == 'five':
            y.add_(ops.dequantize_packed_nhwc(L['rq'].view(-1), y.shape, torch.float32, L['qprc'], L['coloff'], out=L['r32']))
        y = torch.relu_(y)
        return ops.quantize_packed_nhwc(y, L['qpc'], L['bits'], out=L['packed'], coloff=L['coloff'])[0]
    x, w = dequantize(ops, L)
    return torch.nn.functional.conv2d(x, w, L['bias'], stride=L['stride'], padding=L['pad'])


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--batches', default='64,1')
    p.add_argument('--steps', type=int, default=20)
    p.add_argument('--warmup', type=int, default=5)
    p.add_argument('--requant', action='store_true')
    p.add_argument('--residual', action='store_true')
    a = p.parse_args()
    LEGS = ('qadd', 'five') if a.residual else ('q', 'chain') if a.requant else ('int', 'former')
    if not torch.cuda.is_available():
        sys.exit('bench_conv_codes.py needs a GPU')
    from cnn_quantization_amd import ops
    dev = torch.device('cuda')
    gen = torch.Generator().manual_seed(1234)
    res, ok = {}, True
    for N in (int(b) for b in a.batches.split(',')):
        for name, H, Cin, Cout, k, stride in (CLOSING if a.residual else LAYERS):
            for fmt in ('u8', 'pack4'):
                L = make(fmt, N, H, Cin, Cout, k, stride, dev, gen)
                L['taps'], L['y'] = ops.conv_codes_tapsums(L['wq'], fmt), None
                if a.requant or a.residual:       # the output table: zero at a non-integer code, the largest output at 1.25 times the top code
                    y, top = run_leg(ops, 'int', L), float(L['qpx'][2, 0])
                    L['y'], L['bits'] = y, 8 if fmt == 'u8' else 4
                    L['qpy'] = torch.tensor([[float(y.max()) / top * 0.8], [0.37], [top]], device=dev)
                    L['qpc'], L['coloff'] = L['qpy'].expand(3, Cout).contiguous(), ops.packed_layout_nhwc(L['bits'], Cout)
                    L['yq'] = torch.empty((N, y.shape[2], y.shape[3], Cout // (1 if fmt == 'u8' else 2)), dtype=torch.uint8, device=dev)
                    L['packed'] = torch.empty(L['yq'].numel(), dtype=torch.uint8, device=dev)
                    if a.residual:  # shortcut codes over the whole range, zero at a non-integer code near its middle, the conv's spread
                        L['rq'] = torch.randint(0, 256, L['yq'].shape, generator=gen, dtype=torch.uint8).to(dev)
                        L['qpr'] = torch.tensor([[2 * float(y.std()) / top], [0.37 + top / 3], [top]], device=dev)
                        L['qprc'], L['r32'] = L['qpr'].expand(3, Cout).contiguous(), torch.empty_like(y)
                    ref = run_leg(ops, LEGS[1], L).clone()
                    same = bool(torch.equal(run_leg(ops, LEGS[0], L).flatten(), ref))
                else:
                    ref = run_leg(ops, 'former', L)
                    L['y'] = torch.empty_like(ref, memory_format=torch.channels_last)
                    same = bool(torch.allclose(run_leg(ops, 'int', L), ref, rtol=1e-3, atol=1e-3 * float(ref.abs().max())))
                ok = ok and same
                del ref
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
                M = L['y'].numel() // Cout
                new, old = LEGS
                res['%s b%d %s' % (name, N, fmt)] = {
                    'us_median_min_max': us, new + '_Top_per_s': round(2.0 * M * Cout * k * k * Cin / us[new][0] / 1e6, 2),
                    new + '_over_' + old: round(us[new][0] / us[old][0], 4), 'results_agree': same}
                del L
                torch.cuda.empty_cache()
    print(json.dumps(dict(workload='convolution on stored codes: ResNet-50 3x3 and 1x1 layers', steps=a.steps, warmup=a.warmup,
                          device=torch.cuda.get_device_name(0), results=res,
                          not_faster=[k for k, r in res.items() if r['us_median_min_max'][LEGS[0]][0] >= r['us_median_min_max'][LEGS[1]][0]])))
    if not ok:
        sys.exit(1)


if __name__ == '__main__':
    main()
