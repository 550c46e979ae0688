#!/usr/bin/env python3
"""Cost of collect_err on the ResNet-50 conv outputs at BATCH (default 512), per layer shape and alternating in one process:
(i) the statistics table of a collect step (ops.pc_stats, all seven), (ii) the same plus the three candidates' error columns
(ops.mix_candidates + ops.pc_quant_errors), (iii) the materialising route from existing ops: three ops.pc_qdq plus the torch
reductions of smpc.py:84, 96-98.  Median of REPS (default 7) after one warm-up, device events around each call.  Prints one
markdown table; (ii) - (i) is the price of the feature, (iii) what it would cost without cnnq_pc_qerr.  The last two columns are
whole calls, host side included (ops.pc_quant_errors: one torch.stack and two launches; ops.pc_absdev: one torch.empty and the
k_absdev launch), as bytes of x over the call's time; kernel times come from a kernel trace of this script.
ONLY=C,hw (e.g. ONLY=256,56) restricts the run to one layer shape - short enough to trace."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from bench import RESNET50_CONV_OUTPUTS, laplace_activation  # noqa: E402
from cnn_quantization_amd import _lib as L  # noqa: E402
from cnn_quantization_amd import ops  # noqa: E402


def timed(fns, reps):
    """Median time (ms) of every fn, the fns taking turns inside each repetition."""
    for fn in fns:
        fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts[i].append(a.elapsed_time(b))
    return [sorted(t)[len(t) // 2] for t in ts]


def main():
    batch, reps = int(os.environ.get('BATCH', '512')), int(os.environ.get('REPS', '7'))
    dev = torch.device('cuda')
    print('device: %s, batch %d, median of %d' % (torch.cuda.get_device_name(0), batch, reps))
    print('| C | hw | layers | (i) stats ms | (ii) stats+err ms | (ii)-(i) ms | (iii) materialising ms | pc_quant_errors GB/s of x | pc_absdev GB/s of x |')
    print('|---|---|---|---|---|---|---|---|---|')
    tot = [0., 0., 0.]
    only = os.environ.get('ONLY')
    for (C, hw, half, rep) in RESNET50_CONV_OUTPUTS:
        if only and only != '%d,%d' % (C, hw):
            continue
        x = laplace_activation((batch, C, hw, hw), 3, dev)
        N, HW = batch, hw * hw
        kw = dict(num_bits=4, positive=bool(half), bit_alloc=False)

        def stats():
            return ops.pc_stats(x, N, C, HW, need_b=True, need_kurt=True, need_relu=True)[0]

        def with_err():
            t = stats()
            ql, qg, qp = ops.mix_candidates(t, **kw)
            return ops.pc_quant_errors(x, N, C, HW, (qp, qg, ql), mm=t[[L.STAT_MIN, L.STAT_MAX]])

        table = stats()
        qps = ops.mix_candidates(table, **kw)

        def only_err():
            return ops.pc_quant_errors(x, N, C, HW, qps, mm=table[[L.STAT_MIN, L.STAT_MAX]])

        def materialise():
            xr = x.view(N, C, -1)
            nx = torch.sqrt(torch.sum(torch.sqrt(torch.sum(xr ** 2, dim=-1)), dim=0))
            out = []
            for q in qps:
                y = ops.pc_qdq(x, N, C, HW, q).view(N, C, -1)
                out.append(torch.mean(torch.mean((xr - y) ** 2, dim=-1), dim=0))
                out.append(torch.sum(torch.sum(xr * y, dim=-1), dim=0)
                           / (nx * torch.sqrt(torch.sum(torch.sqrt(torch.sum(y ** 2, dim=-1)), dim=0))))
            return out

        def absdev():
            return ops.pc_absdev(x, N, C, HW, table, want_kurt=True)

        t_i, t_ii, t_iii, t_k, t_a = timed([stats, with_err, materialise, only_err, absdev], reps)
        print('| %d | %d | %d | %.3f | %.3f | %.3f | %.3f | %.0f | %.0f |' % (C, hw, rep, t_i, t_ii, t_ii - t_i, t_iii,
                                                                           x.numel() * 4 / t_k / 1e6, x.numel() * 4 / t_a / 1e6), flush=True)
        for i, t in enumerate((t_i, t_ii, t_iii)):
            tot[i] += t * rep
        del x
    print('| all | | | %.3f | %.3f | %.3f | %.3f | | |' % (tot[0], tot[1], tot[1] - tot[0], tot[2]))


if __name__ == '__main__':
    main()
