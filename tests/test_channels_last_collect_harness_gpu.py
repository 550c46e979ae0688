"""The harness end to end on the calibrated recipe with a bf16 channels_last model: ResNet-18 at batch 4,
`--channels-last --dtype bfloat16 -pcq_a -sm collect`, then `-sm use -c laplace -baa` on the file it wrote.  Collect reads every
dense channels_last activation where it lies: none of them is handed to the statistics manager through the half-precision
upcast and none is copied to NCHW; the statistics file loads; the `use` run ends with finite logits and a top-1 class."""
import contextlib
import glob
import importlib
import io
import os
import pickle

import pytest
import torch

pytestmark = pytest.mark.gpu


def test_resnet18_bf16_channels_last_collect_then_use(tmp_path, monkeypatch):
    from cnn_quantization_amd import ops
    from cnn_quantization_amd.harness import inference_sim as H
    from cnn_quantization_amd.inference import inference_quantization_manager as iqm
    from cnn_quantization_amd.utils.misc import Singleton
    iq = importlib.import_module('cnn_quantization_amd.qtypes.int_quantizer')
    monkeypatch.setenv('HOME', str(tmp_path))
    base = ['-a', 'resnet18', '-b', '4', '--image-size', '64', '--qtype', 'int4', '-qw', 'int4', '-pcq_a', '-pcq_w',
            '--channels-last', '--dtype', 'bfloat16']
    native, upcast = [], []
    stats_nhwc, fallback = ops.pc_stats_nhwc, iqm.upcast_fallback

    def spy_stats(x, *a, **kw):
        fb, copies = iq.HALF_FALLBACKS, ops.LAYOUT_COPIES
        out = stats_nhwc(x, *a, **kw)
        native.append((x.dtype, ops._layout(x), iq.HALF_FALLBACKS == fb, ops.LAYOUT_COPIES == copies))
        return out

    def spy_fallback(fn, *a, **kw):
        t = a[0] if a and isinstance(a[0], torch.Tensor) else None
        if getattr(fn, '__name__', '') == 'save_tensor_stats' and t is not None and t.dim() == 4 and ops._layout(t) == 'nhwc':
            upcast.append(tuple(t.shape))
        return fallback(fn, *a, **kw)
    monkeypatch.setattr(ops, 'pc_stats_nhwc', spy_stats)
    monkeypatch.setattr(iqm, 'upcast_fallback', spy_fallback)
    Singleton.reset()
    copies = ops.LAYOUT_COPIES
    with contextlib.redirect_stdout(io.StringIO()):
        assert H.run(H.build_parser().parse_args(base + ['-sm', 'collect']), quiet=True)['output_finite']
    monkeypatch.undo()
    monkeypatch.setenv('HOME', str(tmp_path))
    assert len(native) >= 10, len(native)                                          # the per-channel conv activations
    assert all(c == (torch.bfloat16, 'nhwc', True, True) for c in native), native
    assert not upcast, 'a dense channels_last activation reached the statistics manager through the upcast: %r' % (upcast,)
    assert ops.LAYOUT_COPIES == copies
    # the statistics file loads: per layer a frame of float32 columns, one row per channel
    files = glob.glob(os.path.join(str(tmp_path), 'mxt-sim', 'statistics', 'per_channel', '*', '*_summary.pkl'))
    assert len(files) == 1, files
    with open(files[0], 'rb') as f:
        summary = pickle.load(f)
    assert len(summary) >= 10
    for layer, df in summary.items():
        assert len(df) >= 1 and {'mean_max', 'mean_min', 'mean_std', 'mean_mean', 'mean_b'} <= set(df.columns), layer
        assert all(str(t) == 'float32' for t in df.dtypes), layer
        assert bool((df['mean_std'] >= 0).all()) and bool((df['mean_max'] >= df['mean_min']).all()), layer
    # (`-sm use` also loads the per-tensor file, for the layers that are not quantized per channel: the per-tensor manager's
    # collection is not this route)
    Singleton.reset()
    with contextlib.redirect_stdout(io.StringIO()):
        assert H.run(H.build_parser().parse_args([a for a in base if a != '-pcq_a'] + ['-sm', 'collect']), quiet=True)['output_finite']
    Singleton.reset()
    with contextlib.redirect_stdout(io.StringIO()):
        res = H.run(H.build_parser().parse_args(base + ['-sm', 'use', '-c', 'laplace', '-baa']), quiet=True)
    Singleton.reset()
    assert res['output_finite']
    top1 = res['logits'].float().argmax(dim=1)
    assert top1.shape == (4,) and bool(((top1 >= 0) & (top1 < res['logits'].shape[1])).all())
