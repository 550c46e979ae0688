#!/usr/bin/env python3
"""Config 2 with the entropy of the codes (-me) over the ResNet-50 conv outputs of bench.py as dense channels_last tensors, in three
legs timed in one process, alternating step by step:
    native  the channels_last tensor on the counting NHWC pass (ops.act_qdq_per_channel(want_entropy=True) ->
            cnnq_pc_minmax_qdq_hist_nhwc and the entropy launch), channels_last result;
    copy    the route without it (CNNQ_NHWC=0, what the quantizer did before): x.contiguous(), then the NCHW pipeline with its
            entropy; for bf16 / fp16 the upcast in front and the downcast behind, as upcast_fallback does.  The conversion of the
            NCHW result back to channels_last, which a channels_last model pays downstream, is not counted;
    plain   native without -me (cnnq_pc_minmax_qdq_nhwc): what the counting costs.
--hist-elems N[,N...] adds one native leg per value with that many elements per counting workgroup (the development knob
CNNQ_CL_HIST_ELEMS: the library must be a -DCNNQ_DEV_KNOBS build, e.g. tools/build_alt.sh knobs -DCNNQ_DEV_KNOBS, loaded through
CNNQ_HIP_LIB; the shipped library ignores the variable, which the tool detects from the route function's workgroup count).
One tensor per class of layer (channels x extent, half-range or not) is timed and its time multiplied by the class' layer count; a
class whose tensors do not fit in memory six times over at --batch runs at the largest halved batch that does, and says so.  Per
class and leg the median, minimum and maximum of --steps steps after --warmup (HIP events); a class counts as slower native only
when native's minimum exceeds copy's maximum - the tool's own run-to-run spread.  Before a class is timed it is checked against the
contract: no layout copy, and y / the entropy equal the NCHW route's bit for bit.  Prints one JSON line; exit status 1 if that check
fails.

    tools/bench_channels_last_entropy.py [--batch 512] [--steps 10] [--warmup 3] [--dtypes float32,bfloat16] [--bits 4]
                                         [--hist-elems 16384,65536,262144]"""
import argparse
import ctypes
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

KNOB = 'CNNQ_CL_HIST_ELEMS'


def same(a, b):
    a, b = a.contiguous(), b.contiguous()
    na, nb = torch.isnan(a), torch.isnan(b)
    if not torch.equal(na, nb):
        return False
    iv = torch.int32 if a.dtype == torch.float32 else torch.int16
    return torch.equal(a.view(iv)[~na], b.view(iv)[~nb])


def activation(shape, dt, positive, seed):
    """A Laplace-like channels_last activation (post-ReLU where the layer is half-range), made in pieces."""
    g = torch.Generator(device='cuda').manual_seed(seed)
    C = shape[1]
    scale = 0.5 + 2 * torch.rand(1, C, 1, 1, generator=g, device='cuda')
    x = torch.empty(shape, dtype=dt, device='cuda', memory_format=torch.channels_last)
    n = max(1, shape[0] // 16)
    for i in range(0, shape[0], n):
        piece = (min(n, shape[0] - i),) + tuple(shape[1:])
        e = torch.empty(piece, device='cuda').exponential_(generator=g)
        sign = torch.where(torch.rand(piece, device='cuda', generator=g) < 0.5, -1.0, 1.0)
        v = e * sign * scale
        x[i:i + n] = (v.clamp_(min=0) if positive else v).to(dt)
    return x


def set_knob(v):
    if v is None:
        os.environ.pop(KNOB, None)
    else:
        os.environ[KNOB] = str(v)


def run_leg(ops, leg, xc, yc, dt, bits, positive):
    if leg == 'plain':
        return ops.act_qdq_per_channel(xc, bits, positive=positive, out=yc)
    if leg != 'copy':
        return ops.act_qdq_per_channel(xc, bits, positive=positive, want_entropy=True, out=yc)
    if dt == torch.float32:
        return ops.act_qdq_per_channel(xc, bits, positive=positive, want_entropy=True)      # CNNQ_NHWC=0: the counted copy
    y, e = ops.act_qdq_per_channel(xc.float(), bits, positive=positive, want_entropy=True)
    return y.to(dt), e


def contract(ops, xc, yc, bits, positive):
    before = ops.LAYOUT_COPIES
    y, ent = ops.act_qdq_per_channel(xc, bits, positive=positive, want_entropy=True, out=yc)
    no_copy = ops.LAYOUT_COPIES == before
    y_ref, e_ref = ops.act_qdq_per_channel(xc.contiguous().float(), bits, positive=positive, want_entropy=True)
    ok = same(y, y_ref.to(xc.dtype)) and float(ent) == float(e_ref)
    return bool(ok), bool(no_copy), float(ent)


def counting_wgs(L, ops, xc):
    out = (ctypes.c_int32 * 4)()
    C = xc.shape[1]
    L.check(L.load().cnnq_pc_route_qdq_hist_nhwc(xc.numel() // C, C, ops._DTYPE_CODES[xc.dtype], 16, 16, out), 'cnnq_pc_route_qdq_hist_nhwc')
    return int(out[1])


def main():
    p = argparse.ArgumentParser()
    p.add_argument('--batch', type=int, default=512)
    p.add_argument('--steps', type=int, default=10)
    p.add_argument('--warmup', type=int, default=3)
    p.add_argument('--dtypes', default='float32,bfloat16')
    p.add_argument('--bits', type=int, default=4)
    p.add_argument('--hist-elems', default='', help='comma-separated elements per counting workgroup to sweep (development build)')
    a = p.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_channels_last_entropy.py needs a GPU')
    from bench import RESNET50_CONV_OUTPUTS
    from cnn_quantization_amd import _lib as L, ops
    sweep = [int(v) for v in a.hist_elems.split(',') if v]
    legs = ['native', 'copy', 'plain'] + ['native@%d' % v for v in sweep]
    res, ok_all, knob_live = {}, True, None
    for name in a.dtypes.split(','):
        dt = getattr(torch, name)
        es = torch.empty(0, dtype=dt).element_size()
        classes = {}
        for ci, (C, hw, positive, count) in enumerate(RESNET50_CONV_OUTPUTS):
            batch = a.batch
            # xc, yc, the fp32 NCHW copy and its result (and the upcast for the halves), with headroom
            while batch > 1 and 6 * batch * C * hw * hw * 4 > torch.cuda.mem_get_info()[0]:
                batch //= 2
            xc = activation((batch, C, hw, hw), dt, positive, 700 + ci)
            yc = torch.empty_like(xc)
            ops._NHWC = True
            set_knob(None)
            exact, no_copy, ent = contract(ops, xc, yc, a.bits, positive)
            ok_all = ok_all and exact and no_copy
            torch.cuda.empty_cache()
            row = dict(layers=count, batch=batch, half_range=bool(positive), elements_per_layer=xc.numel(), contract=exact,
                       native_no_copies=no_copy, entropy=round(ent, 4), counting_workgroups=counting_wgs(L, ops, xc))
            if sweep and knob_live is None:
                set_knob(max(sweep) * 4)
                knob_live = counting_wgs(L, ops, xc) != row['counting_workgroups'] or row['counting_workgroups'] == 1
                set_knob(None)

            def step(leg):
                ops._NHWC = leg != 'copy'
                set_knob(int(leg.split('@')[1]) if '@' in leg else None)
                run_leg(ops, leg, xc, yc, dt, a.bits, positive)
            for _ in range(a.warmup):
                for leg in legs:
                    step(leg)
            torch.cuda.synchronize()
            t = {leg: [] for leg in legs}
            for _ in range(a.steps):
                for leg in legs:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    step(leg)
                    e1.record()
                    torch.cuda.synchronize()
                    t[leg].append(e0.elapsed_time(e1) * 1e3)
            set_knob(None)
            ops.reload_switches()
            for leg in legs:
                row[leg] = dict(us_median=round(statistics.median(t[leg]), 1), us_min=round(min(t[leg]), 1), us_max=round(max(t[leg]), 1))
            # 3 passes over the tensor: the statistics read, the Q/DQ read and write
            row['native']['TB_per_s'] = round(xc.numel() * 3 * es / (row['native']['us_median'] * 1e-6) / 1e12, 3)
            row['native_over_copy'] = round(row['native']['us_median'] / row['copy']['us_median'], 4)
            row['native_over_plain'] = round(row['native']['us_median'] / row['plain']['us_median'], 4)
            row['native_slower_than_copy_beyond_spread'] = bool(row['native']['us_min'] > row['copy']['us_max'])
            classes['%dx%dx%d%s' % (C, hw, hw, '+' if positive else '')] = row
            del xc, yc
            torch.cuda.empty_cache()
        # per image, so that a class that ran at a smaller batch weighs what it should
        ms = {leg: round(sum(c[leg]['us_median'] * c['layers'] * a.batch / c['batch'] for c in classes.values()) / 1e3, 3) for leg in legs}
        res[name] = dict(bytes_per_elem_native=3 * es, classes=classes,
                         step_scaled_to_batch=dict(ms=ms, native_over_copy=round(ms['native'] / ms['copy'], 4),
                                                   native_over_plain=round(ms['native'] / ms['plain'], 4),
                                                   classes_native_slower_beyond_spread=[k for k, c in classes.items()
                                                                                        if c['native_slower_than_copy_beyond_spread']]))
    print(json.dumps(dict(workload='resnet50 b%d config 2 -me, int%d (%d classes of conv output, one tensor per class)'
                                   % (a.batch, a.bits, len(RESNET50_CONV_OUTPUTS)),
                          steps=a.steps, warmup=a.warmup, device=torch.cuda.get_device_name(0), hist_elems_swept=sweep,
                          hist_elems_knob_live=knob_live, results=res)))
    if not ok_all:
        sys.exit(1)


if __name__ == '__main__':
    main()
