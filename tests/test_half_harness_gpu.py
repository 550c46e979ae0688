"""The harness end to end in bf16 (--dtype bfloat16): ResNet-50 with the two flag sets of test_resnet50_config2_and_3 -
config 2 (native half kernels) and config 3 with bit allocation and weight bias correction (the upcast fallback)."""
import contextlib
import io

import pytest
import torch

pytestmark = pytest.mark.gpu

BASE = ['-a', 'resnet50', '-b', '4', '--image-size', '64', '-pcq_w', '-pcq_a', '--qtype', 'int4', '-qw', 'int4',
        '--dtype', 'bfloat16']


def run(argv):
    from cnn_quantization_amd.harness import inference_sim as H
    args = H.build_parser().parse_args(argv)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        res = H.run(args, quiet=True)
    return res


@pytest.mark.parametrize('extra', [[], ['-c', 'laplace', '-baa', '-baw', '-bcw']], ids=['config2', 'config3'])
def test_resnet50_bf16(extra):
    res = run(BASE + extra)
    convs = [r for r in res['rows'] if r[0].startswith('conv')]
    assert len(convs) == 53
    assert res['output_finite']
    assert res['logits'].dtype == torch.bfloat16


def test_resnet50_bf16_config2_levels_and_no_fallback():
    """Every channel of every quantized conv output takes at most 2^4 values, and no activation of config 2 is upcast."""
    import sys
    from cnn_quantization_amd.harness import inference_sim as H, models
    from cnn_quantization_amd.inference.inference_quantization_manager import QuantizationManagerInference as QM
    from cnn_quantization_amd.utils import model_prep
    from cnn_quantization_amd.utils.misc import Singleton
    iq = sys.modules['cnn_quantization_amd.qtypes.int_quantizer']
    args = H.build_parser().parse_args(BASE)
    Singleton.reset()
    torch.manual_seed(1)
    worst, dtypes = [], set()

    def hook(mod, i, o):
        dtypes.add(o.dtype)
        worst.append(max(torch.unique(o[:, c]).numel() for c in range(o.shape[1])))
    with contextlib.redirect_stdout(io.StringIO()):
        with QM(args, H.get_params(args)) as qm:
            model = models.ResNet50()
            models.mark_before_relu(model)
            model = model.cuda().eval()
            model_prep.absorb_bn(model)
            qm.bn_folding = True
            model = model.to(torch.bfloat16)
            qm.quantize_model(model)                   # -pcq_w weights: the fallback (weights are not config 2)
            before = iq.HALF_FALLBACKS
            for m in model.modules():
                if isinstance(m, torch.nn.Conv2d):
                    m.register_forward_hook(hook)
            with torch.no_grad():
                out = model(torch.randn(4, 3, 64, 64, device='cuda').to(torch.bfloat16))
            assert iq.HALF_FALLBACKS == before
    assert len(worst) == 53 and max(worst) <= 16, worst
    assert dtypes == {torch.bfloat16}
    assert torch.isfinite(out.float()).all()
