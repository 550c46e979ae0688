"""Dynamic ACIQ clipping on contiguous bf16 / fp16 activations through the quantizer and the harness: the
route is opt-in per quantizer object (half_dynamic, which the inference manager sets on the quantizers it builds); a directly
constructed IntQuantizer, CNNQ_HALF_ACIQ=0 and everything outside the predicate keep the route they had."""
import contextlib
import io

import pytest
import torch

from test_channels_last_gpu import same, values
from test_channels_last_bcorr_gpu import iq_mod, mods, quantizer

pytestmark = pytest.mark.gpu


def counted(q, x, **kw):
    """(q(x), the upcasts it counted)."""
    iq = iq_mod()
    fb = iq.HALF_FALLBACKS
    y = q(x, 'act', **kw)
    return y, iq.HALF_FALLBACKS - fb


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'f16'])
def test_quantizer_takes_the_native_route_when_opted_in(dtype, monkeypatch):
    L, ops = mods()
    x = values((8, 32, 14, 14), seed=8).to(dtype).cuda()
    for clipping, ba, prior, half_range in (('laplace', True, 'gaus', False), ('laplace', True, 'laplace', False),
                                            ('gaus', False, 'gaus', True), ('laplace', False, 'gaus', False)):
        q = quantizer(clipping=clipping, bit_alloc_act=ba, bit_alloc_prior=prior)
        q.half_range = half_range
        assert q.half_dynamic is False
        # the default: one counted upcast, the fp32 route's result cast back - as before
        y0, n = counted(q, x)
        assert n == 1 and y0.dtype == dtype and same(y0, q(x.float(), 'act').to(dtype))
        q.half_dynamic = True
        copies = ops.LAYOUT_COPIES
        y, n = counted(q, x)
        assert n == 0 and ops.LAYOUT_COPIES == copies and y.dtype == dtype and y.shape == x.shape and y.is_contiguous()
        assert same(y, ops.aciq_qdq_half(x, 4, positive=half_range, clip=clipping, bit_alloc=ba, prior_is_b=prior != 'gaus',
                                         target=q.bit_alloc_target_act, round_mode=q.bit_alloc_round))
        # __call__'s override pair reaches the predicate and the route
        yo, n = counted(quantizer(clipping='no', bit_alloc_act=ba, bit_alloc_prior=prior), x, override_att=('clipping', clipping))
        assert n == 1
        qo = quantizer(clipping='no', bit_alloc_act=ba, bit_alloc_prior=prior)
        qo.half_dynamic, qo.half_range = True, half_range
        yo, n = counted(qo, x, override_att=('clipping', clipping))
        assert n == 0 and same(yo, y)
        # the switch off: the upcast again
        monkeypatch.setenv('CNNQ_HALF_ACIQ', '0')
        ops.reload_switches()
        try:
            yu, n = counted(q, x)
            assert n == 1 and same(yu, y0)
        finally:
            monkeypatch.delenv('CNNQ_HALF_ACIQ')
            ops.reload_switches()
        # a class of layer the route function sends back: the upcast
        monkeypatch.setattr(ops, '_aciq_half_native', lambda *a: 0)
        yu, n = counted(q, x)
        monkeypatch.undo()
        assert n == 1 and same(yu, y0)


def test_what_stays_on_its_route():
    """mtd_quant, -me, mix, 2std, a pending correction and replicated data (group = False) keep their routes with the opt-in set:
    the same upcast count and the same bits as without it."""
    L, ops = mods()
    x = values((8, 32, 14, 14), seed=8).to(torch.bfloat16).cuda()
    xf = x.float()

    class SM:
        def get_tensor_stat(self, stat_id, name, kind='mean'):
            t = xf.transpose(0, 1).reshape(32, -1)
            if name.startswith('mse_'):
                return {'mse_laplace': 1., 'mse_gaus': 2., 'mse_lowp': 3.}[name]
            return {'min': t.min(1)[0], 'max': t.max(1)[0], 'mean': t.mean(1), 'std': t.std(1),
                    'b': (t - t.mean(1, keepdim=True)).abs().mean(1)}[name].cpu().numpy()

    def both(make, stat_id=None, pending=None, **kw):
        out = []
        for opt in (False, True):
            q = make()
            q.sm = SM
            q.half_dynamic = opt
            q.fuse_bcorr, q.bcorr_fused = pending, False
            out.append(counted(q, x, stat_id=stat_id, **kw))
        (y0, n0), (y1, n1) = out
        assert n0 == n1 and same(y0, y1) and y1.dtype == x.dtype
        return n1

    assert both(lambda: quantizer(mtd_quant=True, bit_alloc_target_act=3)) == 1              # mid-tread
    assert both(lambda: quantizer(measure_entropy=True)) == 1                                # -me
    assert both(lambda: quantizer(clipping='mix'), stat_id='layer0') == 1                    # -c mix
    assert both(lambda: quantizer(clipping='2std')) == 1                                     # <p>std
    assert both(lambda: quantizer(), pending=True) == 1                                      # a pending correction without a table
    assert both(lambda: quantizer(), stat_id='layer0') == 0                                  # calibrated: _half_table's
    assert both(lambda: quantizer(clipping='no', bit_alloc_act=False)) == 0                  # config 2

    def replicated():
        q = quantizer()
        q.group = False
        return q
    assert both(replicated) == 1
    # not 4-D with a spatial extent: the per-tensor tail's own route
    q = quantizer()
    q.half_dynamic = True
    flat = x.reshape(8, -1)
    y, n = counted(q, flat)
    q.half_dynamic = False
    y0, n0 = counted(q, flat)
    assert n == n0 and same(y, y0)


def test_resnet18_bf16_dynamic_config3_through_the_harness(monkeypatch):
    """-c laplace -baa --dtype bfloat16 in the default layout, batch 4, image 64: no 4-D per-channel activation call upcasts, the
    results keep their dtype and the logits are finite bf16; CNNQ_HALF_ACIQ=0 restores the upcast for those calls."""
    _, ops = mods()
    iq = iq_mod()
    from cnn_quantization_amd.harness import inference_sim as H
    from cnn_quantization_amd.utils.misc import Singleton
    orig = iq.IntQuantizer.__call__
    calls = []

    def wrapper(self, tensor, *a, **kw):
        act = (isinstance(tensor, torch.Tensor) and tensor.dtype == torch.bfloat16 and tensor.dim() == 4 and tensor.is_contiguous()
               and (tensor.shape[2] > 1 or tensor.shape[3] > 1) and bool(self.pcq_a) and not self.pcq_w and self.clipping == 'laplace')
        fb, copies = iq.HALF_FALLBACKS, ops.LAYOUT_COPIES
        out = orig(self, tensor, *a, **kw)
        if act:
            calls.append((iq.HALF_FALLBACKS == fb, ops.LAYOUT_COPIES == copies, out.dtype == tensor.dtype, self.half_dynamic))
        return out
    monkeypatch.setattr(iq.IntQuantizer, '__call__', wrapper)
    args = ['-a', 'resnet18', '-b', '4', '--image-size', '64', '--qtype', 'int4', '-qw', 'int4', '-pcq_a', '-pcq_w', '-c', 'laplace',
            '-baa', '--dtype', 'bfloat16']
    Singleton.reset()
    with contextlib.redirect_stdout(io.StringIO()):
        res = H.run(H.build_parser().parse_args(args), quiet=True)
    native = list(calls)
    monkeypatch.setenv('CNNQ_HALF_ACIQ', '0')
    ops.reload_switches()
    try:
        del calls[:]
        Singleton.reset()
        with contextlib.redirect_stdout(io.StringIO()):
            ref = H.run(H.build_parser().parse_args(args), quiet=True)
        former = list(calls)
    finally:
        monkeypatch.delenv('CNNQ_HALF_ACIQ')
        ops.reload_switches()
        Singleton.reset()
    assert len(native) >= 10, len(native)                                          # the per-channel conv activations
    assert all(c[3] for c in native), 'the manager did not opt a quantizer in'
    assert all(c[0] for c in native), 'a per-channel activation call took the half-precision upcast'
    assert all(c[1] for c in native), 'an activation call copied its input'
    assert all(c[2] for c in native), 'an activation result changed dtype'
    assert res['output_finite'] and res['logits'].dtype == torch.bfloat16
    assert len(former) == len(native) and not any(c[0] for c in former)
    assert ref['output_finite'] and ref['logits'].dtype == torch.bfloat16
