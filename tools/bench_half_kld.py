#!/usr/bin/env python3
"""`-sm collect -kld` (the per-sample KLD threshold, rows = the batch's samples) over the 12 classes of ResNet-50 conv outputs of
bench.py's headline workload as bf16 (or fp16) tensors, contiguous and dense channels_last, one tensor per class, in routes timed
in one process, alternating step by step:
    native          the tensor where it lies (ops.kld_thresholds_half: tensor_row_stats, cnnq_kld_hist_dt, cnnq_kld_search);
    former          the route without the half histogram: the upcast x.float() that upcast_fallback makes - for channels_last
                    with .contiguous(), the transposed copy - then ops.kld_thresholds on the fp32 copy;
    former_as_lies  channels_last only: x.float() keeps the layout and ops.kld_thresholds reads the fp32 copy as it lies (what the
                    per-tensor manager does with a channels_last tensor that arrives through the upcast).
Per class, layout and route the mean step time of --steps steps after --warmup (HIP events) with the minimum and maximum as the
spread, and the same for the whole set weighted by the layers per class.  A class counts as won when native's maximum is below
the minimum of every former route.  Before anything is timed every class is checked: no layout copy and no upcast on the native
route, and out, hist and div bit-equal to the former route's (exit status 1 otherwise).  route_word_native is what
ops._kld_half_native answers for the class: the statistics manager keeps a class with False on the upcast route; this tool times
the native call on every class regardless.
Per class (contiguous) the three launches of the native route are timed one by one, next to the fp32 histogram on the upcast
copy: the row extrema (`rowmm`), the histogram (`hist`), the search; a histogram that takes the same time on 2-byte and on 4-byte
elements is bound by its LDS atomics, not by bytes.  Prints one JSON line.

    tools/bench_half_kld.py [--batch 512] [--steps 10] [--warmup 3] [--dtypes bfloat16,float16]"""
import argparse
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def routes(layout):
    return ('native', 'former') + (('former_as_lies',) if layout == 'channels_last' else ())


def run_route(ops, route, x):
    N = x.shape[0]
    if route == 'native':
        return ops.kld_thresholds_half(x, N, want_parts=True)
    xf = x.float()
    if route == 'former':
        xf = xf.contiguous()
    return ops.kld_thresholds(xf, N, want_parts=True)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def spread(ms):
    return dict(us_mean=round(sum(ms) / len(ms) * 1e3, 1), us_min=round(min(ms) * 1e3, 1), us_max=round(max(ms) * 1e3, 1))


def bit_equal(a, b):
    return all(torch.equal(p.view(torch.int64) if p.dtype == torch.float64 else p, q.view(torch.int64) if q.dtype == torch.float64 else q)
               for p, q in zip(a, b))


def launches(ops, L, x, steps, warmup):
    """The native route's three launches on x and the fp32 histogram on its upcast copy, alternating step by step."""
    lib = L.load()
    N, length = x.shape[0], x.numel() // x.shape[0]
    xf = x.float()
    rowmm = ops.tensor_row_stats(x, N)
    hist = torch.empty((N, L.KLD_BINS), dtype=torch.int32, device=x.device)
    div = torch.empty((N, L.KLD_NCAND), dtype=torch.float64, device=x.device)
    out = torch.empty((N, 3), dtype=torch.float64, device=x.device)
    st = torch.cuda.current_stream().cuda_stream
    dt = ops._HALF_DTYPES[x.dtype]
    legs = dict(
        rowmm=lambda: ops.tensor_row_stats(x, N),
        hist=lambda: L.check(lib.cnnq_kld_hist_dt(x.data_ptr(), dt, N, length, rowmm.data_ptr(), hist.data_ptr(), st), 'cnnq_kld_hist_dt'),
        hist_fp32_copy=lambda: L.check(lib.cnnq_kld_hist(xf.data_ptr(), N, length, rowmm.data_ptr(), hist.data_ptr(), st), 'cnnq_kld_hist'),
        search=lambda: L.check(lib.cnnq_kld_search(hist.data_ptr(), N, rowmm.data_ptr(), div.data_ptr(), out.data_ptr(), st), 'cnnq_kld_search'))
    for _ in range(warmup):
        for f in legs.values():
            f()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(steps):
        for k, f in legs.items():
            ms[k].append(timed(f))
    return {k: spread(v) for k, v in ms.items()}


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--batch', type=int, default=512)
    p.add_argument('--steps', type=int, default=10)
    p.add_argument('--warmup', type=int, default=3)
    p.add_argument('--dtypes', default='bfloat16,float16')
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_half_kld.py needs a GPU')
    import bench
    from cnn_quantization_amd import _lib as L, ops
    iq = importlib.import_module('cnn_quantization_amd.qtypes.int_quantizer')
    dev = torch.device('cuda')
    res = {}
    ok = True
    for name in a.dtypes.split(','):
        dt = getattr(torch, name)
        res[name] = {}
        for layout in ('contiguous', 'channels_last'):
            rts = routes(layout)
            classes = {}
            tot = {r: [0.0] * a.steps for r in rts}
            for k, (C, hw, _, count) in enumerate(bench.RESNET50_CONV_OUTPUTS):
                x = bench.laplace_activation((a.batch, C, hw, hw), 12345 + k, dev).to(dt)
                if layout == 'channels_last':
                    x = x.to(memory_format=torch.channels_last)
                torch.cuda.empty_cache()
                # the contract of this class
                before = (ops.LAYOUT_COPIES, iq.HALF_FALLBACKS)
                got = run_route(ops, 'native', x)
                clean = (ops.LAYOUT_COPIES, iq.HALF_FALLBACKS) == before
                equal = all(bit_equal(got, run_route(ops, r, x)) for r in rts[1:])
                counted = bool((got[1].sum(1) == x.numel() // a.batch).all())
                ok = ok and clean and equal and counted
                del got
                for _ in range(a.warmup):
                    for r in rts:
                        run_route(ops, r, x)
                torch.cuda.synchronize()
                ms = {r: [] for r in rts}
                for _ in range(a.steps):
                    for r in rts:
                        ms[r].append(timed(lambda: run_route(ops, r, x)))
                c = dict(layers=count, elements=x.numel(), contract=bool(clean and equal and counted),
                         route_word_native=bool(ops._kld_half_native(a.batch, x.numel() // a.batch, dt)))
                for r in rts:
                    c[r] = spread(ms[r])
                    for i in range(a.steps):
                        tot[r][i] += ms[r][i] * count
                c['native_wins_beyond_spread'] = all(c['native']['us_max'] < c[r]['us_min'] for r in rts[1:])
                if layout == 'contiguous':
                    c['launches'] = launches(ops, L, x, a.steps, a.warmup)
                classes['%dx%dx%d' % (C, hw, hw)] = c
                del x
                torch.cuda.empty_cache()
            out = {r: dict(ms_mean=round(sum(tot[r]) / a.steps, 4), ms_min=round(min(tot[r]), 4), ms_max=round(max(tot[r]), 4)) for r in rts}
            res[name][layout] = dict(all_53_layers=out,
                                     native_over_former={r: round(out['native']['ms_mean'] / out[r]['ms_mean'], 4) for r in rts[1:]},
                                     native_wins_beyond_spread=all(out['native']['ms_max'] < out[r]['ms_min'] for r in rts[1:]),
                                     classes=classes,
                                     classes_not_won=[k for k, c in classes.items() if not c['native_wins_beyond_spread']])
    print(json.dumps(dict(workload='resnet50 b%d -sm collect -kld on half tensors, rows = samples (12 classes, weighted by their 53 '
                                   'layers)' % a.batch,
                          steps=a.steps, warmup=a.warmup, device=torch.cuda.get_device_name(0), contract=bool(ok), results=res)))
    if not ok:
        sys.exit(1)


if __name__ == '__main__':
    main()
