#!/usr/bin/env python3
"""Config 5 (mid-tread quantization with per-channel bin allocation, -mtq, with and without the entropy of the codes, -me) over
the 13 VGG-16 conv outputs of BASELINE.json's config 5 as dense channels_last tensors, in two routes timed in one process,
alternating step by step:
    native  the channels_last tensor on the NHWC kernels (ops.mid_tread_qdq_nhwc -> cnnq_pc_midtread_nhwc), channels_last result;
    copy    the route without them (CNNQ_NHWC=0, what the quantizer did before): x.contiguous(), then the NCHW pipeline; for
            bf16 / fp16 the upcast in front and the downcast behind, as upcast_fallback does.  The conversion of the NCHW result
            back to channels_last, which a channels_last model pays downstream, is not counted.
One tensor per class of layer (channels x extent) is timed and its time multiplied by the class' layer count; a class whose
tensors do not fit in memory six times over at --batch runs at the largest halved batch that does, and says so.  Per class and
route the median, minimum and maximum of --steps steps after --warmup (HIP events); a class counts as slower native only when
native's minimum exceeds copy's maximum - the tool's own run-to-run spread.  Before a class is timed it is checked against the
contract: no layout copy, and y / the histogram's entropy equal the NCHW kernel's with the table the device reduced, bit for bit.
Prints one JSON line; exit status 1 if that check fails.

    tools/bench_channels_last_midtread.py [--batch 512] [--steps 10] [--warmup 3] [--dtypes float32,bfloat16]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUTES = ('native', 'copy')
TARGET = 4


def same(a, b):
    a, b = a.contiguous(), b.contiguous()
    na, nb = torch.isnan(a), torch.isnan(b)
    if not torch.equal(na, nb):
        return False
    iv = torch.int32 if a.dtype == torch.float32 else torch.int16
    return torch.equal(a.view(iv)[~na], b.view(iv)[~nb])


def activation(shape, dt, seed):
    """A non-negative Laplace-like channels_last activation (fused-ReLU archs: force_positive), made in pieces."""
    g = torch.Generator(device='cuda').manual_seed(seed)
    C = shape[1]
    scale = 0.5 + 2 * torch.rand(1, C, 1, 1, generator=g, device='cuda')
    x = torch.empty(shape, dtype=dt, device='cuda', memory_format=torch.channels_last)
    n = max(1, shape[0] // 16)
    for i in range(0, shape[0], n):
        piece = (min(n, shape[0] - i),) + tuple(shape[1:])
        e = torch.empty(piece, device='cuda').exponential_(generator=g)
        sign = torch.where(torch.rand(piece, device='cuda', generator=g) < 0.5, -1.0, 1.0)
        x[i:i + n] = (e * sign * scale).clamp_(min=0).to(dt)
    return x


def run_route(ops, route, xc, yc, dt, me):
    if route == 'native':
        return ops.mid_tread_qdq_nhwc(xc, TARGET, False, want_entropy=me, out=yc)
    if dt == torch.float32:
        return ops.mid_tread_qdq_nhwc(xc, TARGET, False, want_entropy=me)          # CNNQ_NHWC=0: the counted copy, mid_tread_qdq
    y, e = ops.mid_tread_qdq(xc.float(), TARGET, clip=True, sym=False, want_entropy=me)
    return y.to(dt), e


def contract(ops, L, xc, yc):
    """Half 2 of the contract on this tensor, and that native never copies."""
    import ctypes
    N, C, H, W = xc.shape
    before = ops.LAYOUT_COPIES
    y, ent, parts = ops.mid_tread_qdq_nhwc(xc, TARGET, False, want_entropy=True, out=yc, want_parts=True)
    no_copy = ops.LAYOUT_COPIES == before
    lib, mt = L.load(), parts['mt']
    x32 = xc.contiguous().float()
    ref = torch.empty_like(x32)
    hist = torch.zeros(L.mt_hist_words(C), dtype=torch.int64, device='cuda')
    st = ops._stream(x32)
    L.check(lib.cnnq_pc_midtread_qdq(ops._ptr(x32), ops._ptr(ref), N, C, H * W, ops._ptr(mt), 1, None, ops._ptr(hist), st), 'cnnq_pc_midtread_qdq')
    e_ref = torch.empty(1, dtype=torch.float32, device='cuda')
    L.check(lib.cnnq_midtread_entropy(ops._ptr(hist), ops._ptr(mt), C, xc.numel(), ops._ptr(e_ref), st), 'cnnq_midtread_entropy')
    n = L.MT_HIST_BINS + 2 + 2 * C
    ok = (same(y, ref.to(xc.dtype)) and torch.equal(parts['hist'][:n], hist[:n]) and float(ent) == float(e_ref)
          and int(parts['hist'][:-1].sum()) == xc.numel())
    return bool(ok), bool(no_copy), float(ent)


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--batch', type=int, default=512)
    p.add_argument('--steps', type=int, default=10)
    p.add_argument('--warmup', type=int, default=3)
    p.add_argument('--dtypes', default='float32,bfloat16')
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_channels_last_midtread.py needs a GPU')
    from bench import VGG16_CONV_OUTPUTS
    from cnn_quantization_amd import _lib as L, ops
    res, ok_all = {}, True
    for name in a.dtypes.split(','):
        dt = getattr(torch, name)
        es = torch.empty(0, dtype=dt).element_size()
        classes = {}
        for ci, (C, hw, count) in enumerate(VGG16_CONV_OUTPUTS):
            batch = a.batch
            # xc, yc, the fp32 NCHW copy and its result (and the upcast for the halves), with headroom
            while batch > 1 and 6 * batch * C * hw * hw * 4 > torch.cuda.mem_get_info()[0]:
                batch //= 2
            xc = activation((batch, C, hw, hw), dt, 500 + ci)
            yc = torch.empty_like(xc)
            ops._NHWC = True
            exact, no_copy, ent = contract(ops, L, xc, yc)
            ok_all = ok_all and exact and no_copy
            torch.cuda.empty_cache()
            row = dict(layers=count, batch=batch, elements_per_layer=xc.numel(), contract=exact, native_no_copies=no_copy, entropy=round(ent, 4))
            for me in (False, True):
                def step(route):
                    ops._NHWC = route != 'copy'
                    run_route(ops, route, xc, yc, dt, me)
                for _ in range(a.warmup):
                    for r in ROUTES:
                        step(r)
                torch.cuda.synchronize()
                t = {r: [] for r in ROUTES}
                for _ in range(a.steps):
                    for r in ROUTES:
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        step(r)
                        e1.record()
                        torch.cuda.synchronize()
                        t[r].append(e0.elapsed_time(e1) * 1e3)
                ops.reload_switches()
                m = {r: dict(us_median=round(statistics.median(t[r]), 1), us_min=round(min(t[r]), 1), us_max=round(max(t[r]), 1)) for r in ROUTES}
                m['native']['TB_per_s'] = round(xc.numel() * 4 * es / (m['native']['us_median'] * 1e-6) / 1e12, 3)
                m['native_over_copy'] = round(m['native']['us_median'] / m['copy']['us_median'], 4)
                m['native_slower_than_copy_beyond_spread'] = bool(m['native']['us_min'] > m['copy']['us_max'])
                row['me' if me else 'plain'] = m
            classes['%dx%dx%d' % (C, hw, hw)] = row
            del xc, yc
            torch.cuda.empty_cache()
        tot = {}
        for key in ('plain', 'me'):
            # per image, so that a class that ran at a smaller batch weighs what it should
            ms = {r: sum(c[key][r]['us_median'] * c['layers'] * a.batch / c['batch'] for c in classes.values()) / 1e3 for r in ROUTES}
            tot[key] = dict(native_ms=round(ms['native'], 3), copy_ms=round(ms['copy'], 3), native_over_copy=round(ms['native'] / ms['copy'], 4),
                            classes_native_slower_beyond_spread=[k for k, c in classes.items() if c[key]['native_slower_than_copy_beyond_spread']])
        res[name] = dict(bytes_per_elem_native=4 * es, classes=classes, step_scaled_to_batch=tot)
    print(json.dumps(dict(workload='vgg16 b%d config 5, -mtq [-me] target %d bits (13 conv outputs, one tensor per class)' % (a.batch, TARGET),
                          steps=a.steps, warmup=a.warmup, device=torch.cuda.get_device_name(0), results=res)))
    if not ok_all:
        sys.exit(1)


if __name__ == '__main__':
    main()
