"""Host microseconds per call of the ops entry points on tensors so small that the GPU work hides behind the host's: what the
Python layer itself costs (argument checks, cached plans and workspaces, the ctypes call).  One line per leg; the NCHW legs on a
contiguous [2, 8, 4, 4] tensor, the channels_last legs on the same shape in channels_last storage, fp32 and bf16, the half legs on
the same shape in contiguous bf16.  A leg is timed
in BLOCKS blocks of CALLS calls; the fastest block is the figure to compare (the host's own noise only ever adds), the median
says how noisy the run was.

    python tools/host_overhead.py [calls per block, default 500] [blocks, default 9]
"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cnn_quantization_amd import _lib as L, ops  # noqa: E402

CALLS = int(sys.argv[1]) if len(sys.argv) > 1 else 500
BLOCKS = int(sys.argv[2]) if len(sys.argv) > 2 else 9
x = torch.randn(2, 8, 4, 4, device='cuda')
y = torch.empty_like(x)
legs = [('act_qdq_per_channel cfg2', lambda: ops.act_qdq_per_channel(x, 4, out=y)),
        ('act_qdq_per_channel cfg3', lambda: ops.act_qdq_per_channel(x, 4, clip='laplace', bit_alloc=True, out=y)),
        ('torch.empty x4', lambda: [torch.empty((4, 2, 8), device='cuda') for _ in range(4)])]
for dtype, tag in ((torch.float32, 'fp32'), (torch.bfloat16, 'bf16')):
    xc = x.to(dtype).contiguous(memory_format=torch.channels_last)
    qp, _ = ops.pc_params(ops.pc_stats_nhwc(xc, need_b=True)[0], 4, clip='laplace')
    legs += [('nhwc %s act_qdq_per_channel cfg2' % tag, lambda xc=xc: ops.act_qdq_per_channel(xc, 4)),
             ('nhwc %s act_qdq_per_channel cfg2 -me' % tag, lambda xc=xc: ops.act_qdq_per_channel(xc, 4, want_entropy=True)),
             ('nhwc %s aciq_qdq_nhwc' % tag, lambda xc=xc: ops.aciq_qdq_nhwc(xc, 4)),
             ('nhwc %s qdq_bias_corrected_nhwc' % tag, lambda xc=xc, qp=qp: ops.qdq_bias_corrected_nhwc(xc, qp, True)),
             ('nhwc %s mid_tread_qdq_nhwc' % tag, lambda xc=xc: ops.mid_tread_qdq_nhwc(xc, 4., True)),
             ('nhwc %s pc_stats_nhwc' % tag, lambda xc=xc: ops.pc_stats_nhwc(xc, need_b=True)),
             ('nhwc %s minmax_quantize_packed_nhwc' % tag, lambda xc=xc: ops.minmax_quantize_packed_nhwc(xc, 4))]
xh = x.to(torch.bfloat16).contiguous()
qph, _ = ops.pc_params(ops.pc_stats_half(xh, need_b=True)[0], 4, clip='laplace')
legs += [('half bf16 pc_stats_half', lambda: ops.pc_stats_half(xh, need_b=True)),
         ('half bf16 aciq_qdq_half', lambda: ops.aciq_qdq_half(xh, 4)),
         ('half bf16 qdq_bias_corrected_half', lambda: ops.qdq_bias_corrected_half(xh, qph, True)),
         ('half bf16 mid_tread_qdq_half', lambda: ops.mid_tread_qdq_half(xh, 4., True)),
         ('half bf16 act_qdq_per_channel cfg2', lambda: ops.act_qdq_per_channel(xh, 4))]
print('%s, %d blocks of %d calls per leg' % (L.load().cnnq_version().decode(), BLOCKS, CALLS))
for name, fn in legs:
    for _ in range(50):
        fn()
    host = []
    for _ in range(BLOCKS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(CALLS):
            fn()
        host.append((time.perf_counter() - t0) / CALLS * 1e6)
    torch.cuda.synchronize()
    host.sort()
    print('%-48s host %6.1f us per call (median block %.1f)' % (name, host[0], host[BLOCKS // 2]))
assert ops.LAYOUT_COPIES == 0, 'a channels_last leg took the copy route'
