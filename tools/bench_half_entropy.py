#!/usr/bin/env python3
"""`-me` with a uniform quantizer - config 2 (`-pcq_a`) and config 3 (`-pcq_a -c laplace`), int4 - over the 12 classes of ResNet-50
conv outputs at batch 512 as contiguous bf16 (or fp16) tensors, one tensor per class, in up to five legs timed in one process,
alternating step by step:
    native    the call the quantizer's route 'half_entropy' makes: ops.act_qdq_per_channel(want_entropy=True) /
              ops.aciq_qdq_half(want_entropy=True), the route function's choice;
    two       config 2 only: the same with single_launch=0 - the statistics launch, then the counting pass (6 B/elem);
    resident  config 2 only, where a channel's batch population fits one workgroup's registers: single_launch=2 - one launch that
              reads x once (4 B/elem);
    upcast    the route without them (CNNQ_HALF_ENTROPY=0, the yardstick): upcast_fallback around the fp32 call - x.float(), the
              fp32 launches with their histogram, .to(dtype);
    plain     native WITHOUT -me (ops.act_qdq_per_channel / ops.aciq_qdq_half as the quantizer calls them): what counting costs.
Every -me leg ends in its own one-workgroup entropy launch (no ops.entropy_batch block around it).
A ROUND is --steps steps of every leg, alternating; a leg's figure for the round is its mean step time (HIP events).  Reported
per class and leg: the mean over --rounds rounds (at least three) and, as the spread, the minimum and maximum over the rounds; the
same for the network, weighted by the layers per class.  A leg counts as won against another when its maximum is below the other's
minimum.  Before anything is timed every class is checked (exit status 1 otherwise): no layout copy and no upcast on the native
legs, config 2's y and entropy equal to the upcast leg's bit for bit, config 3's y equal to the fp32 table-driven pass on the
table it published; the share of config 3's elements that differ from the upcast leg's (the statistics are added in another order)
is reported.  A class whose tensors do not fit the device's memory is run at a smaller batch, which is recorded.  Prints one JSON
line.

    tools/bench_half_entropy.py [--batch 512] [--rounds 3] [--steps 5] [--warmup 3] [--dtypes bfloat16,float16] [--configs 2,3]"""
import argparse
import ctypes
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BITS = 4


def upcast(ops, iq, x, clip):
    """What the quantizer does without the route: the fp32 call on x.float() and the result cast back; (y, entropy)."""
    ent = []

    def fp32(t):
        y, e = ops.act_qdq_per_channel(t, BITS, positive=True, clip=clip, want_entropy=True)
        ent.append(e)
        return y
    return iq.upcast_fallback(fp32, x), ent[0]


def run_leg(ops, iq, leg, config, x, parts=False):
    geo = ops.geometry(x)
    if config == 2:
        if leg == 'upcast':
            return upcast(ops, iq, x, 'no')
        if leg == 'plain':
            return ops.act_qdq_per_channel(x, BITS, positive=True)
        if leg == 'native':
            return ops.act_qdq_per_channel(x, BITS, positive=True, want_entropy=True)
        return ops._minmax_qdq_half_entropy(x, *geo, BITS, True, None, single_launch={'two': 0, 'resident': 2}[leg])
    if leg == 'upcast':
        return upcast(ops, iq, x, 'laplace')
    if leg == 'plain':
        return ops.aciq_qdq_half(x, BITS, positive=True, clip='laplace')
    return ops.aciq_qdq_half(x, BITS, positive=True, clip='laplace', want_entropy=True, want_parts=parts)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def wins(a, b):
    return a['us_max'] < b['us_min']


def same_bits(a, b):
    return a.dtype == b.dtype and bool(torch.equal(a.view(torch.int16), b.view(torch.int16)))


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--batch', type=int, default=512)
    p.add_argument('--rounds', type=int, default=3)
    p.add_argument('--steps', type=int, default=5)
    p.add_argument('--warmup', type=int, default=3)
    p.add_argument('--dtypes', default='bfloat16,float16')
    p.add_argument('--configs', default='2,3')
    a = p.parse_args()
    if a.rounds < 3:
        sys.exit('bench_half_entropy.py: the spread is taken over at least three rounds')
    if not torch.cuda.is_available():
        sys.exit('bench_half_entropy.py needs a GPU')
    import bench
    from cnn_quantization_amd import _lib as L, ops
    iq = importlib.import_module('cnn_quantization_amd.qtypes.int_quantizer')
    dev = torch.device('cuda')
    net = [(C, hw, n) for C, hw, _, n in bench.RESNET50_CONV_OUTPUTS]
    free = torch.cuda.mem_get_info()[0]
    res = {}
    ok = True
    for name in a.dtypes.split(','):
        dt = getattr(torch, name)
        for config in (int(c) for c in a.configs.split(',')):
            classes = {}
            names = ('native', 'best', 'upcast', 'plain')
            tot = {r: [0.0] * a.rounds for r in names}
            for k, (C, hw, count) in enumerate(net):
                batch = a.batch
                # x, and on the upcast leg its fp32 copy, the fp32 result and the cast: 2 + 4 + 4 + 2 B/elem, and the native y
                while batch > 1 and batch * C * hw * hw * 16 > free * 0.8:
                    batch //= 2
                x = bench.laplace_activation((batch, C, hw, hw), 12345 + k, dev).to(dt)
                torch.cuda.empty_cache()
                words = {}
                for allow in (1, 2):
                    word = (ctypes.c_int32 * 4)()
                    L.check(L.load().cnnq_pc_route_qdq_hist_dt(batch, C, hw * hw, ops._HALF_DTYPES[dt], 16, 1 << BITS, allow, word),
                            'cnnq_pc_route_qdq_hist_dt')
                    words[allow] = list(word)
                legs = ['native'] + ((['two'] + (['resident'] if words[2][3] == 1 else [])) if config == 2 else []) + ['upcast', 'plain']
                # the contract of this class
                y0, e0 = run_leg(ops, iq, 'upcast', config, x)
                before = (ops.LAYOUT_COPIES, iq.HALF_FALLBACKS)
                clean, differ = True, None
                for r in legs:
                    if r in ('upcast', 'plain'):
                        continue
                    if config == 2:
                        y, e = run_leg(ops, iq, r, config, x)
                        clean = clean and same_bits(y, y0) and float(e) == float(e0)
                    else:
                        y, e, parts = run_leg(ops, iq, r, config, x, parts=True)
                        hist = torch.zeros(256, dtype=torch.int64, device=dev)
                        yr = ops.pc_qdq(x.float(), *ops.geometry(x), parts['qp'], hist=hist).to(dt)
                        clean = clean and same_bits(y, yr) and float(e) == float(ops.entropy_from_hist(hist))
                        differ = float((y != y0).float().mean())
                        del yr, parts
                    del y
                yp = run_leg(ops, iq, 'plain', config, x)
                clean = clean and (config == 3 or same_bits(yp, y0)) and (ops.LAYOUT_COPIES, iq.HALF_FALLBACKS) == before
                ok = ok and clean
                del y0, yp
                for _ in range(a.warmup):
                    for r in legs:
                        run_leg(ops, iq, r, config, x)
                torch.cuda.synchronize()
                us = {r: [] for r in legs}
                for _ in range(a.rounds):
                    ms = {r: 0.0 for r in legs}
                    for _ in range(a.steps):
                        for r in legs:
                            ms[r] += timed(lambda: run_leg(ops, iq, r, config, x))
                    for r in legs:
                        us[r].append(ms[r] / a.steps * 1e3)
                c = dict(layers=count, batch=batch, elements=x.numel(), route_words=words[1], route_words_forced=words[2], contract=bool(clean))
                if differ is not None:
                    c['share_of_elements_differing_from_upcast'] = float('%.2e' % differ)
                for r in legs:
                    c[r] = dict(us_mean=round(sum(us[r]) / a.rounds, 1), us_min=round(min(us[r]), 1), us_max=round(max(us[r]), 1))
                best = 'native'
                if config == 2:
                    best = 'two'
                    c['two_wins_over_upcast_beyond_spread'] = wins(c['two'], c['upcast'])
                    c['upcast_wins_over_two_beyond_spread'] = wins(c['upcast'], c['two'])
                    if 'resident' in legs:
                        c['resident_wins_over_two_beyond_spread'] = wins(c['resident'], c['two'])
                        c['resident_wins_over_upcast_beyond_spread'] = wins(c['resident'], c['upcast'])
                        if c['resident_wins_over_two_beyond_spread']:
                            best = 'resident'
                else:
                    c['native_wins_over_upcast_beyond_spread'] = wins(c['native'], c['upcast'])
                    c['upcast_wins_over_native_beyond_spread'] = wins(c['upcast'], c['native'])
                c['best_forced'] = best
                c['counting_costs_us'] = round(c['native']['us_mean'] - c['plain']['us_mean'], 1)
                for i in range(a.rounds):
                    for r in names:
                        tot[r][i] += us[best if r == 'best' else r][i] * count / 1e3
                classes['%dx%dx%d' % (C, hw, hw)] = c
                print(name, config, '%dx%dx%d' % (C, hw, hw), {r: c[r] for r in legs}, file=sys.stderr, flush=True)
                del x
                torch.cuda.empty_cache()
            out = {r: dict(ms_mean=round(sum(tot[r]) / a.rounds, 4), ms_min=round(min(tot[r]), 4), ms_max=round(max(tot[r]), 4)) for r in tot}
            key = '%s resnet50 config %d -me' % (name, config)
            print(key, out, file=sys.stderr, flush=True)
            res[key] = dict(all_layers=out, native_over_upcast=round(out['native']['ms_mean'] / out['upcast']['ms_mean'], 4),
                            native_wins_beyond_spread=out['native']['ms_max'] < out['upcast']['ms_min'], classes=classes,
                            classes_not_won=[k for k, c in classes.items() if not wins(c[c['best_forced']], c['upcast'])])
    print(json.dumps(dict(workload='resnet50 b%d int%d -me, configs 2 and 3, on contiguous half tensors (classes weighted by their layers)'
                                   % (a.batch, BITS),
                          rounds=a.rounds, steps=a.steps, warmup=a.warmup, device=torch.cuda.get_device_name(0), contract=bool(ok),
                          results=res)))
    if not ok:
        sys.exit(1)


if __name__ == '__main__':
    main()
