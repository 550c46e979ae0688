"""-sm use on contiguous bf16 / fp16 per-channel activations through the quantizer: with a calibration
table (stat_id) the clipping, bit-allocation and bias-correction branches quantize the tensor where it lies - no upcast, no copy -
and everything dynamic, -me, mid-tread, -c mix and replicated data keep the route they had; then the harness end to end."""
import contextlib
import io

import pytest
import torch

from test_channels_last_gpu import same, values
from test_channels_last_bcorr_gpu import iq_mod, mods, quantizer

pytestmark = pytest.mark.gpu
# (clipping, bit allocation, relu first): the four combinations of tests/test_channels_last_bcorr_gpu.py
COMBOS = (('laplace', True, True), ('gaus', False, False), ('no', False, True), ('no', True, False))


def setup(dtype):
    L, ops = mods()
    x = values((8, 32, 14, 14), seed=8).to(dtype).cuda()
    xf = x.float()
    C = 32
    stat = {'min': xf.amin(dim=(0, 2, 3)), 'max': xf.amax(dim=(0, 2, 3)) * 0.9, 'mean': xf.mean(dim=(0, 2, 3)),
            'std': xf.std(dim=(0, 2, 3)), 'b': (xf - xf.mean(dim=(0, 2, 3)).view(1, C, 1, 1)).abs().mean(dim=(0, 2, 3))}

    class SM:
        def get_tensor_stat(self, stat_id, name, kind='mean'):
            return stat[name].cpu().numpy()
    table = torch.zeros((L.NSTAT, C), dtype=torch.float32, device='cuda')
    for k, r in (('min', L.STAT_MIN), ('max', L.STAT_MAX), ('mean', L.STAT_MEAN), ('std', L.STAT_STD), ('b', L.STAT_B)):
        table[r] = stat[k]
    return x, SM, table


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=['bf16', 'f16'])
def test_quantizer_with_a_statistics_table(dtype, monkeypatch):
    L, ops = mods()
    iq = iq_mod()
    x, SM, table = setup(dtype)
    for clipping, ba, relu_first in COMBOS:
        q = quantizer(clipping=clipping, bit_alloc_act=ba)
        q.sm = SM
        q.half_range = relu_first
        qp, _ = ops.pc_params(table, 4, relu_first, clipping, ba, False, None, True)
        # a pending correction: folded in where the tensor lies
        fb, copies = iq.HALF_FALLBACKS, ops.LAYOUT_COPIES
        q.fuse_bcorr, q.bcorr_fused = relu_first, False
        y = q(x, 'act', stat_id='layer0')
        assert q.fuse_bcorr is None and q.bcorr_fused
        assert y.is_contiguous() and y.dtype == dtype and y.shape == x.shape
        assert (iq.HALF_FALLBACKS, ops.LAYOUT_COPIES) == (fb, copies), (clipping, ba)
        assert same(y, ops.qdq_bias_corrected_half(x, qp, relu_first))
        # without one: the table-driven Q/DQ, no correction
        q.bcorr_fused = False
        y0 = q(x, 'act', stat_id='layer0')
        assert y0.dtype == dtype and not q.bcorr_fused and (iq.HALF_FALLBACKS, ops.LAYOUT_COPIES) == (fb, copies), (clipping, ba)
        assert same(y0, ops.pc_qdq(x, 8, 32, 196, qp))
        # the switch off: one counted upcast, the fp32 chain's result cast back
        monkeypatch.setenv('CNNQ_HALF_TABLE', '0')
        ops.reload_switches()
        try:
            for pending in ((False, True) if (clipping != 'no' or ba) else (True,)):    # (plain min/max without a correction is config 2)
                fb = iq.HALF_FALLBACKS
                q.fuse_bcorr, q.bcorr_fused = (relu_first if pending else None), False
                yu = q(x, 'act', stat_id='layer0')
                assert iq.HALF_FALLBACKS == fb + 1 and q.bcorr_fused == pending and yu.dtype == dtype
                q.fuse_bcorr, q.bcorr_fused = (relu_first if pending else None), False
                assert same(yu, q(x.float(), 'act', stat_id='layer0').to(dtype))
        finally:
            monkeypatch.delenv('CNNQ_HALF_TABLE')
            ops.reload_switches()


def test_what_stays_on_the_former_route(monkeypatch):
    L, ops = mods()
    iq = iq_mod()
    x, SM, table = setup(torch.bfloat16)
    mse = {'mse_laplace': 1., 'mse_gaus': 2., 'mse_lowp': 3.}

    class SMX(SM):
        def get_tensor_stat(self, stat_id, name, kind='mean'):
            if name in mse:
                return mse[name]
            return SM.get_tensor_stat(self, stat_id, name, kind)

    def upcasts(q, stat_id='layer0', pending=None, **kw):
        """The counted upcasts of one call, which must equal the fp32 call cast back."""
        q.sm = SMX
        fb = iq.HALF_FALLBACKS
        q.fuse_bcorr, q.bcorr_fused = pending, False
        y = q(x, 'act', stat_id=stat_id, **kw)
        n = iq.HALF_FALLBACKS - fb
        q.fuse_bcorr, q.bcorr_fused = pending, False
        assert y.dtype == x.dtype and same(y, q(x.float(), 'act', stat_id=stat_id, **kw).to(x.dtype))
        return n

    assert upcasts(quantizer(), stat_id=None) == 1                                   # dynamic config 3
    assert upcasts(quantizer(), stat_id=None, pending=True) == 1
    assert upcasts(quantizer(clipping='no'), stat_id=None, pending=True) == 1        # dynamic min/max with a correction
    assert upcasts(quantizer(measure_entropy=True)) == 1                             # -me
    assert upcasts(quantizer(mtd_quant=True, bit_alloc_target_act=3)) == 1           # mid-tread
    assert upcasts(quantizer(clipping='mix')) == 1                                   # -c mix
    assert upcasts(quantizer(), override_att=('clipping', 'mix')) == 1
    q = quantizer()
    q.group = False                                                                  # replicated data
    assert upcasts(q) == 1 and upcasts(q, pending=True) == 1
    assert upcasts(quantizer()) == 0 and upcasts(quantizer(), pending=False) == 0    # ... and what does not


def test_resnet18_calibrated_bias_correction(tmp_path, monkeypatch):
    """The harness end to end on the paper's recipe in the default layout: -sm collect (per channel, then per tensor), then -sm use
    -c laplace -baa -bca --dtype bfloat16.  Every per-channel conv activation call returns its dtype without the upcast and folds
    the correction in; the logits are finite and agree with the same run under CNNQ_HALF_TABLE=0.

    The two runs differ only in the order the correction's sums are added in: a bias differs in its last bits, an activation by one
    bf16 rounding here and there, and further down a few 4-bit codes by one level.  Such a flip moves one input of a sum over at
    least 64 * 9 products by one step, 1 / 15 of its range, so the logits must agree far inside one 4-bit step of their own range:
    |a - b| <= (max - min of the logits) / 15."""
    _, ops = mods()
    iq = iq_mod()
    from cnn_quantization_amd.harness import inference_sim as H
    from cnn_quantization_amd.utils.misc import Singleton
    monkeypatch.setenv('HOME', str(tmp_path))
    base = ['-a', 'resnet18', '-b', '4', '--image-size', '64', '--qtype', 'int4', '-qw', 'int4', '-pcq_a', '-pcq_w']
    for argv in (base + ['-sm', 'collect'], [a for a in base if a != '-pcq_a'] + ['-sm', 'collect']):
        Singleton.reset()
        with contextlib.redirect_stdout(io.StringIO()):
            assert H.run(H.build_parser().parse_args(argv), quiet=True)['output_finite']
    orig = iq.IntQuantizer.__call__
    calls = []

    def wrapper(self, tensor, *a, **kw):
        half = (isinstance(tensor, torch.Tensor) and tensor.dtype == torch.bfloat16 and tensor.dim() == 4 and tensor.is_contiguous()
                and (tensor.shape[2] > 1 or tensor.shape[3] > 1))
        fb, copies, pending = iq.HALF_FALLBACKS, ops.LAYOUT_COPIES, self.fuse_bcorr is not None
        out = orig(self, tensor, *a, **kw)
        if half:
            calls.append((iq.HALF_FALLBACKS == fb, ops.LAYOUT_COPIES == copies, out.dtype == tensor.dtype, self.clipping,
                          bool(self.pcq_a), pending, self.bcorr_fused))
        return out
    monkeypatch.setattr(iq.IntQuantizer, '__call__', wrapper)
    args = base + ['-sm', 'use', '-c', 'laplace', '-baa', '-bca', '--dtype', 'bfloat16']
    Singleton.reset()
    with contextlib.redirect_stdout(io.StringIO()):
        res = H.run(H.build_parser().parse_args(args), quiet=True)
    native = list(calls)
    monkeypatch.setenv('CNNQ_HALF_TABLE', '0')
    ops.reload_switches()
    try:
        del calls[:]
        Singleton.reset()
        with contextlib.redirect_stdout(io.StringIO()):
            ref = H.run(H.build_parser().parse_args(args), quiet=True)
        former = list(calls)
    finally:
        monkeypatch.delenv('CNNQ_HALF_TABLE')
        ops.reload_switches()
        Singleton.reset()
    assert res['output_finite'] and ref['output_finite']
    corrected = [c for c in native if c[3] == 'laplace' and c[4] and c[5]]
    assert len(corrected) >= 10, len(corrected)                                   # the per-channel conv activations
    assert all(c[6] for c in corrected), 'a per-channel activation did not fold the correction in'
    assert all(c[0] for c in corrected), 'a per-channel activation call took the half-precision upcast'
    assert all(c[1] for c in native), 'an activation call copied its input'
    assert all(c[2] for c in native), 'an activation result changed dtype'
    # the switch restores the former route for those calls
    assert [c for c in former if c[3] == 'laplace' and c[4] and c[5]] and not any(c[0] for c in former if c[3] == 'laplace' and c[4] and c[5])
    a, b = res['logits'].float(), ref['logits'].float()
    span = float(b.max() - b.min())
    print('logits: max |native - former| = %.4g, range of the logits %.4g' % (float((a - b).abs().max()), span))
    assert float((a - b).abs().max()) <= span / 15
