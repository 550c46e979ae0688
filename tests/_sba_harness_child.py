"""One harness run in a process of its own, for tests/test_sba_collect_manager_gpu.py: `python _sba_harness_child.py ARG...` runs
inference_sim with those arguments under spies and prints one JSON line - what reached the statistics manager and how.  The
environment (HOME, CNNQ_SBA_NATIVE) is the caller's: the switches are read once, at import."""
import contextlib
import importlib
import io
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main(argv):
    import torch
    from cnn_quantization_amd import ops
    from cnn_quantization_amd.harness import inference_sim as H
    from cnn_quantization_amd.inference import inference_quantization_manager as iqm
    iq = importlib.import_module('cnn_quantization_amd.qtypes.int_quantizer')
    # the two runs a test compares must see the same activations: MIOpen's deterministic algorithms, and a digest of every spatial
    # activation handed to the statistics manager to prove it
    torch.backends.cudnn.deterministic = True
    torch.backends.cudnn.benchmark = False
    seen = dict(stats=[], extrema=[], pc_stats=0, upcast=[], digest=[])
    route = iqm._route

    def spy_route(layer, out, *a, **kw):
        if isinstance(out, torch.Tensor) and out.dim() == 4 and (out.shape[2] > 1 or out.shape[3] > 1) and out.element_size() == 2:
            seen['digest'].append(int(out.detach().contiguous().view(torch.int16).to(torch.int64).sum()))
        return route(layer, out, *a, **kw)
    iqm._route = spy_route

    def spy(name, key):
        real = getattr(ops, name)

        def fn(x, *a, **kw):
            fb, copies = iq.HALF_FALLBACKS, ops.LAYOUT_COPIES
            out = real(x, *a, **kw)
            seen[key].append([str(x.dtype), ops._layout(x), iq.HALF_FALLBACKS == fb, ops.LAYOUT_COPIES == copies])
            return out
        setattr(ops, name, fn)
    for name in ('pc_stats_half', 'pc_stats_nhwc'):
        spy(name, 'stats')
    for name in ('pc_sample_extrema_half', 'pc_sample_extrema_nhwc'):
        spy(name, 'extrema')
    pc_stats, fallback = ops.pc_stats, iqm.upcast_fallback

    def spy_pc_stats(*a, **kw):
        seen['pc_stats'] += 1
        return pc_stats(*a, **kw)

    def spy_fallback(fn, *a, **kw):
        t = a[0] if a and isinstance(a[0], torch.Tensor) else None
        if getattr(fn, '__name__', '') == 'save_tensor_stats' and t is not None and t.dim() == 4 and (t.shape[2] > 1 or t.shape[3] > 1):
            seen['upcast'].append(list(t.shape))
        return fallback(fn, *a, **kw)
    ops.pc_stats = spy_pc_stats
    iqm.upcast_fallback = spy_fallback
    copies = ops.LAYOUT_COPIES
    with contextlib.redirect_stdout(io.StringIO()):
        res = H.run(H.build_parser().parse_args(argv), quiet=True)
    logits = res.get('logits')
    print(json.dumps(dict(seen, output_finite=bool(res['output_finite']), layout_copies=ops.LAYOUT_COPIES - copies,
                          logits_finite=bool(torch.isfinite(logits.float()).all()) if logits is not None else None)))


if __name__ == '__main__':
    main(sys.argv[1:])
