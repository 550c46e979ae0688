"""The harness end to end with --channels-last on config 2 with the entropy of the codes (-me, per-channel int4): ResNet-18 on small
images in bf16.  A wrapper around the quantizer records every 4-D dense channels_last activation call: its output is channels_last
in its own dtype, and the call took neither a layout copy nor the half-precision upcast; every logged activation entropy is finite
and within [0, 4] bits.  (Value equality is the op-level tests' job: conv outputs of the two layouts differ in their last bits.)"""
import contextlib
import importlib
import io
import math

import pytest
import torch

pytestmark = pytest.mark.gpu


def test_resnet18_channels_last_config2_me(monkeypatch):
    from cnn_quantization_amd import ops
    from cnn_quantization_amd.harness import inference_sim as H
    iq = importlib.import_module('cnn_quantization_amd.qtypes.int_quantizer')
    argv = ['-a', 'resnet18', '-b', '4', '--image-size', '64', '-pcq_a', '-pcq_w', '--qtype', 'int4', '-qw', 'int4', '-me',
            '--channels-last', '--dtype', 'bfloat16']
    args = H.build_parser().parse_args(argv)
    orig = iq.IntQuantizer.__call__
    calls = []

    def wrapper(self, tensor, *a, **kw):
        nhwc = isinstance(tensor, torch.Tensor) and tensor.dim() == 4 and ops._layout(tensor) == 'nhwc'
        fb, copies = iq.HALF_FALLBACKS, ops.LAYOUT_COPIES
        native = nhwc and self._nhwc_entropy(tensor)
        out = orig(self, tensor, *a, **kw)
        if nhwc:
            calls.append((out.is_contiguous(memory_format=torch.channels_last) and not out.is_contiguous(),
                          iq.HALF_FALLBACKS == fb, ops.LAYOUT_COPIES == copies, out.dtype == tensor.dtype, native))
        return out
    monkeypatch.setattr(iq.IntQuantizer, '__call__', wrapper)
    logged = []
    log_metric = H.MeterLogger.log_metric

    def recorder(self, key, value, step=None, meterId=None, weight=1.):
        logged.append((key, value, meterId))
        return log_metric(self, key, value, step=step, meterId=meterId, weight=weight)
    monkeypatch.setattr(H.MeterLogger, 'log_metric', recorder)
    with contextlib.redirect_stdout(io.StringIO()):
        res = H.run(args, quiet=True)
    assert res['output_finite']
    assert sum(c[4] for c in calls) >= 10, [c[4] for c in calls]                     # the conv outputs take the counting route
    assert all(c[0] for c in calls), 'an activation result is not channels_last'
    assert all(c[1] for c in calls), 'an activation call took the half-precision upcast'
    assert all(c[2] for c in calls), 'an activation call copied its input to NCHW'
    assert all(c[3] for c in calls), 'an activation result changed dtype'
    act = [v for _, v, meter in logged if meter == 'avg.entropy.act']
    assert len(act) >= sum(c[4] for c in calls)
    assert all(math.isfinite(v) and 0.0 <= v <= 4.0 for v in act), act
    ent = res['entropy'].get('avg.entropy.act')
    assert ent is not None and math.isfinite(ent) and 0.0 < ent <= 4.0, res['entropy']
