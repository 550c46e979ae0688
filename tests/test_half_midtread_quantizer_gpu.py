"""Mid-tread quantization (config 5) on contiguous bf16 / fp16 activations through the quantizer and the harness (DESIGN.md section
28): the route is opt-in per quantizer object (half_midtread, which the inference manager sets on the quantizers it builds); a
directly constructed IntQuantizer, CNNQ_HALF_MIDTREAD=0, a class of layer the route function sends back and everything outside
the route's conditions keep the route they had."""
import contextlib
import io
import math

import pytest
import torch

import _quantizer as Q
from test_channels_last_bcorr_gpu import iq_mod, mods
from test_channels_last_gpu import same, values

pytestmark = pytest.mark.gpu


class Logger:
    def __init__(self):
        self.rows = []

    def log_metric(self, name, value, step=None, meterId=None, weight=None):
        self.rows.append((name, value, meterId, weight))


def quantizer(**kw):
    return Q.quantizer(**dict(dict(clipping='laplace', pcq_act=True, bit_alloc_act=True, bit_alloc_target_act=5.3, mtd_quant=True), **kw))


def counted(q, x, **kw):
    """(q(x), the upcasts it counted, the layout copies it counted)."""
    iq, (_, ops) = iq_mod(), mods()
    fb, copies = iq.HALF_FALLBACKS, ops.LAYOUT_COPIES
    y = q(x, 'act', **kw)
    return y, iq.HALF_FALLBACKS - fb, ops.LAYOUT_COPIES - copies


@pytest.mark.parametrize('me', [False, True], ids=['plain', 'me'])
@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'f16'])
def test_quantizer_takes_the_native_route_when_opted_in(dtype, me, monkeypatch):
    L, ops = mods()
    x = values((8, 32, 14, 14), seed=6).to(dtype).cuda()
    log = Logger()
    q = quantizer(measure_entropy=me, logger=log)
    assert q.half_midtread is False
    # the default: one counted upcast, the fp32 route's result cast back - as before
    y0, n, copies = counted(q, x)
    assert (n, copies) == (1, 0) and y0.dtype == dtype and same(y0, q(x.float(), 'act').to(dtype))
    del log.rows[:]
    q.half_midtread = True
    y, n, copies = counted(q, x)
    assert (n, copies) == (0, 0) and y.dtype == dtype and y.shape == x.shape and y.is_contiguous()
    y_ref, e_ref = ops.mid_tread_qdq_half(x, 5.3, sym=True, want_entropy=me)
    assert same(y, y_ref)
    if me:
        assert len(log.rows) == 1 and log.rows[0][0] == 'act.entropy' and log.rows[0][2] == 'avg.entropy.act'
        assert log.rows[0][1] == float(e_ref) and log.rows[0][3] == x.numel()
    else:
        assert not log.rows
    # the non-negative range
    q.force_positive = True
    xp = values((8, 32, 14, 14), seed=6, positive=True).to(dtype).cuda()
    yp, n, copies = counted(q, xp)
    assert (n, copies) == (0, 0) and same(yp, ops.mid_tread_qdq_half(xp, 5.3, sym=False)[0])
    q.force_positive = False
    # __call__'s override pair reaches the route
    qo = quantizer(mtd_quant=False, measure_entropy=me, logger=Logger())
    yo, n, _ = counted(qo, x, override_att=('mtd_quant', True))
    assert n == 1 and same(yo, y0)
    qo.half_midtread = True
    yo, n, copies = counted(qo, x, override_att=('mtd_quant', True))
    assert (n, copies) == (0, 0) and same(yo, y)
    # the switch off: the upcast again
    monkeypatch.setenv('CNNQ_HALF_MIDTREAD', '0')
    ops.reload_switches()
    try:
        yu, n, _ = counted(q, x)
        assert n == 1 and same(yu, y0)
    finally:
        monkeypatch.delenv('CNNQ_HALF_MIDTREAD')
        ops.reload_switches()
    # a class of layer the route function sends back: the upcast
    monkeypatch.setattr(ops, '_midtread_half_native', lambda *a: 0)
    yu, n, _ = counted(q, x)
    monkeypatch.undo()
    assert n == 1 and same(yu, y0)
    assert counted(q, x)[1] == 0


def test_what_stays_on_its_route():
    """A pending correction, replicated data (group = False), clipping 'no', KLD and a 2-D tensor keep their routes with the opt-in
    set: the same upcast count and the same bits as without it."""
    x = values((8, 32, 14, 14), seed=8).to(torch.bfloat16).cuda()

    def both(make, t=x, **kw):
        out = []
        for opt in (False, True):
            q = make()
            q.half_midtread = opt
            out.append(counted(q, t, **kw))
        (y0, n0, c0), (y1, n1, c1) = out
        assert (n0, c0) == (n1, c1) and same(y0, y1) and y1.dtype == t.dtype
        return n1

    def pending():
        q = quantizer()
        q.fuse_bcorr, q.bcorr_fused = True, False
        return q

    def replicated():
        q = quantizer()
        q.group = False
        return q

    xf = x.float().cpu()
    whole = {'min': xf.min() * 0.8, 'max': xf.max() * 0.9, 'mean': xf.mean(), 'kld_th': xf.abs().max() * 0.6}

    class SM:
        def get_tensor_stat(self, stat_id, name, kind='mean'):
            return whole[name].numpy()

    def kld():
        q = quantizer(kld=True)
        q.sm = SM
        return q
    assert both(pending) == 1
    assert both(replicated) == 1
    assert both(lambda: quantizer(clipping='no')) == 1                   # the per-channel branch at clipping 'no' has no route
    assert both(kld, stat_id='tensor') == 0                              # KLD hands a half tensor to its own kernel
    assert both(lambda: quantizer(), t=x.reshape(8, -1)) == 0            # not 4-D: the per-tensor route over flat storage
    assert both(lambda: quantizer(), t=x.to(memory_format=torch.channels_last)) == 0        # channels_last comes first
    assert both(lambda: quantizer(mtd_quant=False)) == 1                 # -me without mid-tread is not this route's
    # and with it: the native route
    q = quantizer()
    q.half_midtread = True
    assert counted(q, x)[1:] == (0, 0)


def test_vgg16_bf16_config5_through_the_harness(monkeypatch):
    """-c laplace -baa -bata 5.3 -mtq -me --dtype bfloat16 in the default layout, batch 2, image 64: no mid-tread call on a
    contiguous 4-D activation upcasts or copies, the results keep their dtype, the entropy is finite and positive;
    CNNQ_HALF_MIDTREAD=0 restores the upcast for the same calls."""
    _, ops = mods()
    iq = iq_mod()
    from cnn_quantization_amd.harness import inference_sim as H
    from cnn_quantization_amd.utils.misc import Singleton
    orig = iq.IntQuantizer.__call__
    calls = []

    def wrapper(self, tensor, *a, **kw):
        act = (isinstance(tensor, torch.Tensor) and tensor.dtype == torch.bfloat16 and tensor.dim() == 4 and tensor.is_contiguous()
               and (tensor.shape[2] > 1 or tensor.shape[3] > 1) and bool(self.pcq_a) and not self.pcq_w and bool(self.mtd_quant)
               and self.clipping != 'no')
        fb, copies = iq.HALF_FALLBACKS, ops.LAYOUT_COPIES
        out = orig(self, tensor, *a, **kw)
        if act:
            calls.append((iq.HALF_FALLBACKS == fb, ops.LAYOUT_COPIES == copies, out.dtype == tensor.dtype and out.is_contiguous(),
                          self.half_midtread))
        return out
    monkeypatch.setattr(iq.IntQuantizer, '__call__', wrapper)
    args = ['-a', 'vgg16', '-b', '2', '--image-size', '64', '--qtype', 'int4', '-qw', 'int4', '--dtype', 'bfloat16',
            '-pcq_a', '-pcq_w', '-c', 'laplace', '-baa', '-bata', '5.3', '-mtq', '-me']
    Singleton.reset()
    with contextlib.redirect_stdout(io.StringIO()):
        res = H.run(H.build_parser().parse_args(args), quiet=True)
    native = list(calls)
    monkeypatch.setenv('CNNQ_HALF_MIDTREAD', '0')
    ops.reload_switches()
    try:
        del calls[:]
        Singleton.reset()
        with contextlib.redirect_stdout(io.StringIO()):
            ref = H.run(H.build_parser().parse_args(args), quiet=True)
        former = list(calls)
    finally:
        monkeypatch.delenv('CNNQ_HALF_MIDTREAD')
        ops.reload_switches()
        Singleton.reset()
    assert len(native) >= 13, len(native)                                          # the 13 conv outputs on the mid-tread route
    assert all(c[3] for c in native), 'the manager did not opt a quantizer in'
    assert all(c[0] for c in native), 'a mid-tread activation call took the half-precision upcast'
    assert all(c[1] for c in native), 'an activation call copied its input'
    assert all(c[2] for c in native), 'an activation result changed dtype or layout'
    assert res['output_finite'] and res['logits'].dtype == torch.bfloat16
    ent = res['entropy'].get('avg.entropy.act')
    assert ent is not None and math.isfinite(ent) and ent > 0, res['entropy']
    assert len(former) == len(native) and not any(c[0] for c in former)
    assert ref['output_finite'] and ref['logits'].dtype == torch.bfloat16
