"""The harness end to end with --channels-last: ResNet-18 on small images, fp32 and bf16, config 2 (-pcq_a) and config 1.  A
wrapper around the quantizer records each activation call: its output is channels_last and equals, bit for bit, the quantizer
on input.contiguous(); no layout copy and no half-precision upcast happen.  (Conv outputs of the two layouts differ in their
last bits, so logits are not compared across layouts.)"""
import contextlib
import io

import pytest
import torch

pytestmark = pytest.mark.gpu


def same(a, b):
    a, b = a.contiguous(), b.contiguous()
    na, nb = torch.isnan(a), torch.isnan(b)
    iv = torch.int32 if a.dtype == torch.float32 else torch.int16
    return a.dtype == b.dtype and torch.equal(na, nb) and torch.equal(a.view(iv)[~na], b.view(iv)[~nb])


@pytest.mark.parametrize('dtype', ['float32', 'bfloat16'])
@pytest.mark.parametrize('pcq', [True, False], ids=['config2', 'config1'])
def test_resnet18_channels_last(monkeypatch, dtype, pcq):
    from cnn_quantization_amd import ops
    from cnn_quantization_amd.harness import inference_sim as H
    import sys
    iq = sys.modules['cnn_quantization_amd.qtypes.int_quantizer']
    argv = ['-a', 'resnet18', '-b', '4', '--image-size', '64', '--qtype', 'int4', '-qw', 'int4', '--dtype', dtype,
            '--channels-last'] + (['-pcq_a', '-pcq_w'] if pcq else [])
    args = H.build_parser().parse_args(argv)
    orig = iq.IntQuantizer.__call__
    calls = []

    def wrapper(self, tensor, *a, **kw):
        out = orig(self, tensor, *a, **kw)
        if isinstance(tensor, torch.Tensor) and ops._layout(tensor) == 'nhwc':
            fb = iq.HALF_FALLBACKS
            ref = orig(self, tensor.contiguous(), *a, **kw)
            calls.append((out.is_contiguous(memory_format=torch.channels_last) and not out.is_contiguous(), same(out, ref),
                          iq.HALF_FALLBACKS == fb))
        return out
    monkeypatch.setattr(iq.IntQuantizer, '__call__', wrapper)
    copies = ops.LAYOUT_COPIES
    with contextlib.redirect_stdout(io.StringIO()):
        res = H.run(args, quiet=True)
    assert res['output_finite']
    assert len(calls) >= 10, len(calls)
    assert all(c[0] for c in calls), 'an activation result is not channels_last'
    assert all(c[1] for c in calls), 'an activation result differs from the NCHW path'
    assert all(c[2] for c in calls), 'an activation call took the half-precision upcast'
    assert ops.LAYOUT_COPIES == copies
