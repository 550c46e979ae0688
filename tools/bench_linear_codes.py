#!/usr/bin/env python3
"""The integer linear layer on the stored codes on the classifier layers of VGG-16 (25088 -> 4096, 4096 -> 4096,
4096 -> 1000) and ResNet-50 (2048 -> 1000) at the given batches, u8 / u8 and pack4 / pack4, three legs timed in one process,
alternating call by call:
    int      ops.linear_codes on the codes, Rw held (ops.linear_codes_rowsums, outside the timed region);
    former   what a holder of codes did without it: ops.dequantize_u8 / dequantize_pack4 of both operands, then
             torch.nn.functional.linear in fp32;
    gemm     that fp32 GEMM alone on operands dequantized beforehand - the comparison for a caller who never stored codes.
Per leg the median, minimum and maximum time of --steps calls after --warmup (HIP events); for `int` the int8 operation rate
2 M N K / t and the bytes the algorithm moves (both code matrices once, y once) over t.  A shape whose `int` minimum is not below
the `former` maximum is listed under not_faster.  Before anything is timed the two routes' results are compared on every shape
(they differ by the fp32 GEMM's rounding).  Prints one JSON line; exit status 1 if that comparison fails.

--requant times the layer that hands CODES to the next one instead, two other legs:
    q        ops.linear_codes_q with ReLU: codes in, codes out, Rw held;
    chain    the same bytes without it: ops.linear_codes, torch.relu_, and ops.quantize_u8 / quantize_pack4 of y seen as one channel
             (a per-tensor table).
The two legs' bytes are compared (they are equal) before anything is timed; not_faster by the same rule.

    tools/bench_linear_codes.py [--batches 512,1] [--steps 20] [--warmup 5] [--requant]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LAYERS = (('vgg16_fc1', 25088, 4096), ('vgg16_fc2', 4096, 4096), ('vgg16_fc3', 4096, 1000), ('resnet50_fc', 2048, 1000))


def make(fmt, M, N, K, dev, gen):
    qmax = 255 if fmt == 'u8' else 15

    def operand(rows):
        c = torch.randint(0, qmax + 1, (rows, K), generator=gen, dtype=torch.uint8).to(dev)
        return c if fmt == 'u8' else (c[:, 0::2] | (c[:, 1::2] << 4)).contiguous()
    qpx = torch.tensor([[0.05], [qmax / 2 + 0.25], [float(qmax)]], device=dev)
    qpw = torch.stack([torch.linspace(1e-3, 2e-3, N), torch.linspace(qmax / 2 - 3, qmax / 2 + 3, N), torch.full((N,), float(qmax))]).to(dev)
    return dict(fmt=fmt, M=M, N=N, K=K, xq=operand(M), wq=operand(N), qpx=qpx, qpw=qpw, bias=torch.linspace(-1, 1, N).to(dev))


def dequantize(ops, L):
    """Both operands as fp32 matrices through the library's dequantizers: the activation one channel, the weight N channels."""
    M, N, K = L['M'], L['N'], L['K']
    if L['fmt'] == 'u8':
        x = ops.dequantize_u8(L['xq'].view(1, 1, M * K, 1), L['qpx'])
        w = ops.dequantize_u8(L['wq'].view(1, N, K, 1), L['qpw'])
    else:
        x = ops.dequantize_pack4(L['xq'].view(-1), (1, 1, M * K, 1), L['qpx'])
        w = ops.dequantize_pack4(L['wq'].view(-1), (1, N, K, 1), L['qpw'])
    return x.view(M, K), w.view(N, K)


def run_leg(ops, leg, L):
    if leg == 'int':
        return ops.linear_codes(L['xq'], L['wq'], L['qpx'], L['qpw'], bias=L['bias'], x_format=L['fmt'], w_format=L['fmt'], rw=L['rw'], out=L['y'])
    if leg in ('q', 'chain'):
        kw = dict(bias=L['bias'], x_format=L['fmt'], w_format=L['fmt'], rw=L['rw'])
        if leg == 'q':
            return ops.linear_codes_q(L['xq'], L['wq'], L['qpx'], L['qpw'], L['qpy'], relu=True, y_format=L['fmt'], out=L['yq'], **kw)
        y = torch.relu_(ops.linear_codes(L['xq'], L['wq'], L['qpx'], L['qpw'], out=L['y'], **kw)).view(1, 1, -1, 1)
        return ops.quantize_u8(y, L['qpy']) if L['fmt'] == 'u8' else ops.quantize_pack4(y, L['qpy'])
    x, w = dequantize(ops, L) if leg == 'former' else (L['xf'], L['wf'])
    return torch.nn.functional.linear(x, w, L['bias'])


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--batches', default='512,1')
    p.add_argument('--steps', type=int, default=20)
    p.add_argument('--warmup', type=int, default=5)
    p.add_argument('--requant', action='store_true')
    a = p.parse_args()
    LEGS = ('q', 'chain') if a.requant else ('int', 'former', 'gemm')
    if not torch.cuda.is_available():
        sys.exit('bench_linear_codes.py needs a GPU')
    from cnn_quantization_amd import ops
    dev = torch.device('cuda')
    gen = torch.Generator().manual_seed(1234)
    res, ok = {}, True
    for M in (int(b) for b in a.batches.split(',')):
        for name, K, N in LAYERS:
            for fmt in ('u8', 'pack4'):
                L = make(fmt, M, N, K, dev, gen)
                L['rw'] = ops.linear_codes_rowsums(L['wq'], fmt)
                L['y'] = torch.empty((M, N), device=dev)
                if a.requant:       # the output table: zero at a non-integer code, the largest output at 1.25 times the top code
                    top = float(L['qpx'][2, 0])
                    L['qpy'] = torch.tensor([[float(run_leg(ops, 'int', L).max()) / top * 0.8], [0.37], [top]], device=dev)
                    L['yq'] = torch.empty((M, N // (1 if fmt == 'u8' else 2)), dtype=torch.uint8, device=dev)
                    same = bool(torch.equal(run_leg(ops, 'q', L).flatten(), run_leg(ops, 'chain', L).flatten()))
                else:
                    L['xf'], L['wf'] = dequantize(ops, L)
                    ref = run_leg(ops, 'gemm', L)
                    same = bool(torch.allclose(run_leg(ops, 'int', L), ref, rtol=1e-3, atol=1e-3 * float(ref.abs().max())))
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
                nbytes = L['xq'].numel() + L['wq'].numel() + 4 * M * N
                if a.requant:
                    res['%s b%d %s' % (name, M, fmt)] = dict(us_median_min_max=us, q_over_chain=round(us['q'][0] / us['chain'][0], 4), results_agree=same)
                    continue
                res['%s b%d %s' % (name, M, fmt)] = dict(
                    us_median_min_max=us, int_Top_per_s=round(2.0 * M * N * K / us['int'][0] / 1e6, 2), int_bytes=nbytes,
                    int_GB_per_s=round(nbytes / us['int'][0] / 1e3, 1), int_over_former=round(us['int'][0] / us['former'][0], 4),
                    int_over_gemm=round(us['int'][0] / us['gemm'][0], 4), results_agree=same)
                del L
                torch.cuda.empty_cache()
    print(json.dumps(dict(workload='linear layer on stored codes: VGG-16 and ResNet-50 classifier layers', steps=a.steps, warmup=a.warmup,
                          device=torch.cuda.get_device_name(0), results=res,
                          not_faster=[k for k, r in res.items() if r['us_median_min_max'][LEGS[0]][1] >= r['us_median_min_max'][LEGS[1]][2]])))
    if not ok:
        sys.exit(1)


if __name__ == '__main__':
    main()
