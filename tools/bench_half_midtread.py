#!/usr/bin/env python3
"""`-c laplace -baa -bata T -mtq [-me]` (config 5) over the 5 classes of VGG-16 and the 12 classes of ResNet-50 conv outputs at batch
512 as contiguous bf16 (or fp16) tensors, one tensor per class, in up to four routes timed in one process, alternating step by step:
    native    ops.mid_tread_qdq_half as the quantizer calls it: the route function's choice;
    chain     the same call with single_launch=0: pass A, pass B, the parameters, the Q/DQ (and the histogram) - 8 B/elem;
    resident  the same call with single_launch=2, where a channel's batch population fits one workgroup's registers: pass A and the
              bin allocation, then one launch that reads x once - 6 B/elem;
    former    the route without them (CNNQ_HALF_MIDTREAD=0): upcast_fallback around ops.mid_tread_qdq - x.float(), the fp32
              pipeline, .to(dtype).
Per class, target, -me and route the mean step time of --steps steps after --warmup (HIP events) with the minimum and maximum as the
spread, and the same for each network weighted by the layers per class.  A route counts as won against another when its maximum is
below the other's minimum.  Before anything is timed every class is checked: no layout copy and no upcast on the native routes, y
equal to cnnq_pc_midtread_qdq on x.float() with the published table, cast back (exit status 1 otherwise); the share of elements that
differ from the former route's result (the statistics are added in another order, so a step size may differ in its last bits) is
reported.  A class whose tensors do not fit the device's memory is run at a smaller batch, which is recorded.  Prints one JSON line.

    tools/bench_half_midtread.py [--batch 512] [--steps 20] [--warmup 3] [--dtypes bfloat16,float16] [--targets 5.3,4]
                                 [--entropy 0,1] [--nets vgg16,resnet50]"""
import argparse
import ctypes
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ALLOW = {'native': None, 'chain': 0, 'resident': 2}


def run_route(ops, iq, route, x, target, me, parts=False):
    if route == 'former':
        return iq.upcast_fallback(lambda t: ops.mid_tread_qdq(t, target, clip=True, sym=True, group=False, want_entropy=me)[0], x)
    return ops.mid_tread_qdq_half(x, target, True, want_entropy=me, single_launch=ALLOW[route], want_parts=parts)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def wins(a, b):
    return a['us_max'] < b['us_min']


def reference(L, ops, x, mt):
    """cnnq_pc_midtread_qdq (clip = 1) on x.float() with the table mt, cast back to x's dtype."""
    N, C, HW = ops.geometry(x)
    xf = x.float()
    y = torch.empty_like(xf)
    L.check(L.load().cnnq_pc_midtread_qdq(xf.data_ptr(), y.data_ptr(), N, C, HW, mt.data_ptr(), 1, None, None, ops._stream(xf)),
            'cnnq_pc_midtread_qdq')
    return y.to(x.dtype)


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--batch', type=int, default=512)
    p.add_argument('--steps', type=int, default=20)
    p.add_argument('--warmup', type=int, default=3)
    p.add_argument('--dtypes', default='bfloat16,float16')
    p.add_argument('--targets', default='5.3,4')
    p.add_argument('--entropy', default='0,1')
    p.add_argument('--nets', default='vgg16,resnet50')
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_half_midtread.py needs a GPU')
    import bench
    from cnn_quantization_amd import _lib as L, ops
    iq = importlib.import_module('cnn_quantization_amd.qtypes.int_quantizer')
    dev = torch.device('cuda')
    nets = {'vgg16': [(C, hw, n) for C, hw, n in bench.VGG16_CONV_OUTPUTS],
            'resnet50': [(C, hw, n) for C, hw, _, n in bench.RESNET50_CONV_OUTPUTS]}
    free = torch.cuda.mem_get_info()[0]
    res = {}
    ok = True
    for name in a.dtypes.split(','):
        dt = getattr(torch, name)
        for net in a.nets.split(','):
            for target in (float(t) for t in a.targets.split(',')):
                for me in (bool(int(e)) for e in a.entropy.split(',')):
                    classes = {}
                    names = ('native', 'chain', 'best', 'former')
                    tot = {r: [0.0] * a.steps for r in names}
                    for k, (C, hw, count) in enumerate(nets[net]):
                        batch = a.batch
                        # x, and on the former route its fp32 copy, the fp32 result and both casts: 2 + 4 + 4 + 2 + 2 B/elem
                        while batch > 1 and batch * C * hw * hw * 16 > free * 0.8:
                            batch //= 2
                        x = bench.laplace_activation((batch, C, hw, hw), 12345 + k, dev).to(dt)
                        torch.cuda.empty_cache()
                        words = {}
                        for allow in (1, 2):
                            word = (ctypes.c_int32 * 4)()
                            L.check(L.load().cnnq_pc_route_midtread_dt(batch, C, hw * hw, ops._HALF_DTYPES[dt], 16, int(me), allow, word),
                                    'cnnq_pc_route_midtread_dt')
                            words[allow] = list(word)
                        routes = ['native', 'chain'] + (['resident'] if words[2][3] == 3 else []) + ['former']
                        # the contract of this class
                        before = (ops.LAYOUT_COPIES, iq.HALF_FALLBACKS)
                        clean, differ = True, {}
                        y0 = None
                        for r in routes[:-1]:
                            y, _, parts = run_route(ops, iq, r, x, target, me, parts=True)
                            clean = clean and bool(torch.equal(y.view(torch.int16), reference(L, ops, x, parts['mt']).view(torch.int16)))
                            if y0 is None:
                                clean = clean and (ops.LAYOUT_COPIES, iq.HALF_FALLBACKS) == before
                                y0 = run_route(ops, iq, 'former', x, target, me)
                                before = (ops.LAYOUT_COPIES, iq.HALF_FALLBACKS)
                            differ[r] = float((y != y0).float().mean())
                            del y, parts
                        clean = clean and (ops.LAYOUT_COPIES, iq.HALF_FALLBACKS) == before
                        ok = ok and clean
                        del y0
                        for _ in range(a.warmup):
                            for r in routes:
                                run_route(ops, iq, r, x, target, me)
                        torch.cuda.synchronize()
                        ms = {r: [] for r in routes}
                        for _ in range(a.steps):
                            for r in routes:
                                ms[r].append(timed(lambda: run_route(ops, iq, r, x, target, me)))
                        c = dict(layers=count, batch=batch, elements=x.numel(), route_words=words[1], route_words_forced=words[2],
                                 contract=bool(clean), share_of_elements_differing_from_former={r: float('%.2e' % v) for r, v in differ.items()})
                        for r in routes:
                            c[r] = dict(us_mean=round(sum(ms[r]) / a.steps * 1e3, 1), us_min=round(min(ms[r]) * 1e3, 1),
                                        us_max=round(max(ms[r]) * 1e3, 1))
                        c['chain_wins_over_former_beyond_spread'] = wins(c['chain'], c['former'])
                        c['former_wins_over_chain_beyond_spread'] = wins(c['former'], c['chain'])
                        best = 'chain'
                        if 'resident' in routes:
                            c['resident_wins_over_chain_beyond_spread'] = wins(c['resident'], c['chain'])
                            c['resident_wins_over_former_beyond_spread'] = wins(c['resident'], c['former'])
                            if c['resident_wins_over_chain_beyond_spread']:
                                best = 'resident'
                        c['best_forced'] = best
                        for i in range(a.steps):
                            for r in names:
                                tot[r][i] += ms[best if r == 'best' else r][i] * count
                        classes['%dx%dx%d' % (C, hw, hw)] = c
                        del x
                        torch.cuda.empty_cache()
                    out = {r: dict(ms_mean=round(sum(tot[r]) / a.steps, 4), ms_min=round(min(tot[r]), 4), ms_max=round(max(tot[r]), 4))
                           for r in tot}
                    key = '%s %s -bata %g%s' % (name, net, target, ' -me' if me else '')
                    print(key, out, file=sys.stderr, flush=True)
                    res[key] = dict(
                        all_layers=out, native_over_former=round(out['native']['ms_mean'] / out['former']['ms_mean'], 4),
                        native_wins_beyond_spread=out['native']['ms_max'] < out['former']['ms_min'], classes=classes,
                        classes_not_won=[k for k, c in classes.items() if not wins(c[c['best_forced']], c['former'])])
    print(json.dumps(dict(workload='vgg16 / resnet50 b%d -c laplace -baa -mtq, on contiguous half tensors (classes weighted by their '
                                   'layers)' % a.batch,
                          steps=a.steps, warmup=a.warmup, device=torch.cuda.get_device_name(0), contract=bool(ok), results=res)))
    if not ok:
        sys.exit(1)


if __name__ == '__main__':
    main()
