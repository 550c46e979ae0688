"""The per-tensor branches of IntQuantizer on half and channels_last tensors: layer-wise ACIQ clipping, -kld
use and per-tensor mid-tread take neither the half-precision upcast nor a layout copy (contract item 4), the result keeps dtype
and layout and is the ops function's; a contiguous fp32 tensor takes the code it took; and the harness end to end."""
import contextlib
import importlib
import io

import pytest
import torch

from test_channels_last_gpu import cl, same
from test_tensor_clip_cpu import quantizer, values

pytestmark = pytest.mark.gpu


def mods():
    from cnn_quantization_amd import _lib as L, ops
    return L, ops, importlib.import_module('cnn_quantization_amd.qtypes.int_quantizer')


def inputs():
    v = values((4, 6, 5, 5), seed=6)
    return [('bf16 nchw', v.bfloat16().cuda()), ('bf16 nhwc', cl(v, torch.bfloat16)), ('f32 nhwc', cl(v, torch.float32)),
            ('f16 nhwc', cl(v, torch.float16)), ('bf16 2d', values((16, 100), seed=7).bfloat16().cuda())]


class Counters:
    """Both counters stay where they were inside the block."""
    def __enter__(self):
        _, ops, iq = mods()
        self.before = (iq.HALF_FALLBACKS, ops.LAYOUT_COPIES)

    def __exit__(self, *exc):
        _, ops, iq = mods()
        if exc[0] is None:
            assert (iq.HALF_FALLBACKS, ops.LAYOUT_COPIES) == self.before, 'an upcast or a layout copy was made'


def kept(x, y):
    assert y.dtype == x.dtype and y.shape == x.shape and y.stride() == x.stride()


def test_layer_wise_clipping_dynamic():
    L, ops, iq = mods()
    q = quantizer(clipping='laplace', pcq_act=False)
    for name, x in inputs():
        with Counters():
            y = q(x, 'act')
            kept(x, y)
            assert same(y, ops.clip_qdq_tensor(x, 4, clip='laplace')), name
            q.force_positive = True
            assert same(q(x, 'act'), ops.clip_qdq_tensor(x, 4, positive=True, clip='laplace')), name
            q.force_positive = False
            assert same(q(x, 'act', override_att=('clipping', 'gaus')), ops.clip_qdq_tensor(x, 4, clip='gaus')), name
            assert same(q(x, 'act', override_att=('clipping', '2std')), ops.clip_qdq_tensor(x, 4, clip='2std')), name
        # and it is the fp32 route's result on the same table
        _, p = ops.clip_qdq_tensor(x, 4, clip='laplace', want_parts=True)
        ref = ops.act_qdq_per_channel(x.float().contiguous(), 4, clip='laplace', whole_tensor=True, stats=p['stats'].contiguous(), group=False)
        assert same(y, ref.view(x.shape).to(x.dtype)), name


def test_layer_wise_clipping_with_a_statistics_table():
    """-sm use through the quantizer: the [NSTAT, 1] table it builds from the statistics manager."""
    L, ops, iq = mods()
    for name, x in inputs():
        xf = x.float()
        rows = {'min': xf.min(), 'max': xf.max(), 'mean': xf.mean(), 'std': xf.std(), 'b': (xf - xf.mean()).abs().mean()}

        class SM:
            def get_tensor_stat(self, stat_id, stat, kind='mean'):
                return rows[stat].cpu().numpy()
        q = quantizer(clipping='laplace', pcq_act=False)
        q.sm = SM
        with Counters():
            y = q(x, 'act', stat_id='layer0')
            yg = q(x, 'act', stat_id='layer0', override_att=('clipping', 'gaus'))
        kept(x, y)
        table = torch.zeros((L.NSTAT, 1), dtype=torch.float32, device='cuda')
        for k, r in (('min', L.STAT_MIN), ('max', L.STAT_MAX), ('mean', L.STAT_MEAN), ('std', L.STAT_STD), ('b', L.STAT_B)):
            table[r] = rows[k]
        assert same(y, ops.clip_qdq_tensor(x, 4, clip='laplace', stats=table)), name
        assert same(yg, ops.clip_qdq_tensor(x, 4, clip='gaus', stats=table)), name
        ref = ops.act_qdq_per_channel(xf.contiguous(), 4, clip='laplace', whole_tensor=True, stats=table, group=False)
        assert same(y, ref.view(x.shape).to(x.dtype)), name


def test_linear_shaped_tensor_under_a_per_channel_quantizer():
    """-pcq_a does not apply to a 2-D activation (activation_linear, VGG-16's FC layers) nor to a 1x1 spatial extent."""
    L, ops, iq = mods()
    q = quantizer(clipping='laplace', pcq_act=True)
    for x in (values((16, 100), seed=7).bfloat16().cuda(), values((8, 32, 1, 1), seed=8).half().cuda()):
        with Counters():
            y = q(x, 'act')
        kept(x, y)
        assert same(y, ops.clip_qdq_tensor(x, 4, clip='laplace'))


def test_kld_on_half_tensors():
    L, ops, iq = mods()
    stats = dict(min=-3.1, max=4.2, kld_th=1.7, mean=0.2)

    class SM:
        def get_tensor_stat(self, stat_id, stat, kind='mean'):
            return stats[stat]
    q = quantizer(clipping='no', kld=True, pcq_act=False)
    q.sm = SM
    for name, x in inputs():
        if x.dtype == torch.float32:
            continue
        with Counters():
            y = q(x, 'act', stat_id='layer0')
        kept(x, y)
        assert same(y, q(x.float(), 'act', stat_id='layer0').to(x.dtype)), name
        q.force_positive = True
        with Counters():
            yp = q(x, 'act', stat_id='layer0')
        assert same(yp, q(x.float(), 'act', stat_id='layer0').to(x.dtype)), name
        q.force_positive = False


def test_per_tensor_mid_tread():
    L, ops, iq = mods()
    q = quantizer(clipping='laplace', mtd_quant=True, pcq_act=False, bit_alloc_target_act=3)
    for name, x in inputs():
        with Counters():
            y = q(x, 'act')
            kept(x, y)
            assert same(y, ops.mid_tread_qdq_tensor(x, 3, sym=True)), name
            q.force_positive = True
            assert same(q(x, 'act'), ops.mid_tread_qdq_tensor(x, 3, sym=False)), name
            q.force_positive = False
        # the fp32 route's pass on the same table
        _, p = ops.mid_tread_qdq_tensor(x, 3, sym=True, want_parts=True)
        xf = x.float().contiguous()
        ref = torch.empty_like(xf)
        L.check(L.load().cnnq_pc_midtread_qdq(xf.data_ptr(), ref.data_ptr(), 1, 1, xf.numel(), p['mt'].data_ptr(), 1, None, None,
                                              ops._stream(xf)), 'cnnq_pc_midtread_qdq')
        assert same(y, ref.view(x.shape).to(x.dtype)), name
    # under -pcq_a a 2-D tensor is per tensor too
    qa = quantizer(clipping='laplace', mtd_quant=True, pcq_act=True, bit_alloc_target_act=3)
    x = values((16, 100), seed=7).bfloat16().cuda()
    with Counters():
        assert same(qa(x, 'act'), ops.mid_tread_qdq_tensor(x, 3, sym=True))


def test_the_routes_that_stay(monkeypatch):
    """A contiguous fp32 tensor and replicated data take the code they took."""
    L, ops, iq = mods()
    seen = []
    orig_pc, orig_mt = ops.act_qdq_per_channel, ops.mid_tread_qdq

    def pc(*a, **kw):
        seen.append(('pc', kw.get('whole_tensor')))
        return orig_pc(*a, **kw)

    def mt(*a, **kw):
        seen.append(('mt', kw.get('whole_tensor')))
        return orig_mt(*a, **kw)
    monkeypatch.setattr(ops, 'act_qdq_per_channel', pc)
    monkeypatch.setattr(ops, 'mid_tread_qdq', mt)
    x = values((4, 6, 5, 5), seed=9).cuda()
    q = quantizer(clipping='laplace', pcq_act=False)
    y = q(x, 'act')
    assert seen == [('pc', True)] and same(y, orig_pc(x, 4, clip='laplace', whole_tensor=True).view(x.shape))
    qm = quantizer(clipping='laplace', mtd_quant=True, pcq_act=False)
    qm(x, 'act')
    assert seen == [('pc', True), ('mt', True)]
    # replicated data (group False): a bf16 tensor upcasts as before
    q.group = False
    fb = iq.HALF_FALLBACKS
    del seen[:]
    yb = q(x.bfloat16(), 'act')
    assert iq.HALF_FALLBACKS == fb + 1 and seen == [('pc', True)] and yb.dtype == torch.bfloat16


def test_resnet18_per_tensor_recipe_channels_last_bf16(monkeypatch):
    """-c laplace without -pcq_a, --dtype bfloat16 --channels-last: no activation call upcasts or copies (the 2-D activation_linear
    shape has its own test above: ResNet-18's only FC layer is the classifier, which does not clip)."""
    L, ops, iq = mods()
    from cnn_quantization_amd.harness import inference_sim as H
    argv = ['-a', 'resnet18', '-b', '4', '--image-size', '64', '--qtype', 'int4', '-qw', 'int4', '--dtype', 'bfloat16',
            '--channels-last', '-c', 'laplace']
    args = H.build_parser().parse_args(argv)
    orig = iq.IntQuantizer.__call__
    calls = []

    def wrapper(self, tensor, *a, **kw):
        fb, copies = iq.HALF_FALLBACKS, ops.LAYOUT_COPIES
        out = orig(self, tensor, *a, **kw)
        if isinstance(tensor, torch.Tensor):
            tag = a[1] if len(a) > 1 else kw.get('tag', '')
            calls.append((tag, self.clipping, tensor.dim(), ops._layout(tensor), iq.HALF_FALLBACKS == fb, ops.LAYOUT_COPIES == copies,
                          out.dtype == tensor.dtype, out.stride() == tensor.stride()))
        return out
    monkeypatch.setattr(iq.IntQuantizer, '__call__', wrapper)
    with contextlib.redirect_stdout(io.StringIO()):
        res = H.run(args, quiet=True)
    assert res['output_finite']
    acts = [c for c in calls if 'activation' in c[0]]
    clipped = [c for c in acts if c[1] == 'laplace']
    assert sum(c[2] == 4 and c[3] == 'nhwc' for c in clipped) >= 10, calls                # conv outputs on the clipping route
    assert all(c[4] for c in acts), 'an activation call took the half-precision upcast'
    assert all(c[5] for c in acts), 'an activation call copied its input'
    assert all(c[6] and c[7] for c in acts), 'an activation result changed dtype or layout'


def test_resnet18_per_tensor_calibrated_recipe_channels_last_bf16(tmp_path, monkeypatch):
    """The per-tensor recipe, `-sm collect` then `-sm use -c laplace`, --dtype bfloat16 --channels-last: under `-sm use` no
    activation call upcasts or copies, and the clipping calls carry a stat_id (the table-driven form)."""
    L, ops, iq = mods()
    from cnn_quantization_amd.harness import inference_sim as H
    from cnn_quantization_amd.utils.misc import Singleton
    monkeypatch.setenv('HOME', str(tmp_path))
    base = ['-a', 'resnet18', '-b', '4', '--image-size', '64', '--qtype', 'int4', '-qw', 'int4', '--dtype', 'bfloat16', '--channels-last']
    Singleton.reset()
    with contextlib.redirect_stdout(io.StringIO()):
        assert H.run(H.build_parser().parse_args(base + ['-sm', 'collect']), quiet=True)['output_finite']
    Singleton.reset()
    orig = iq.IntQuantizer.__call__
    calls = []

    def wrapper(self, tensor, id, tag='', stat_id=None, override_att=None):
        fb, copies = iq.HALF_FALLBACKS, ops.LAYOUT_COPIES
        out = orig(self, tensor, id, tag, stat_id, override_att)
        if isinstance(tensor, torch.Tensor) and 'activation' in tag:
            calls.append((self.clipping, stat_id is not None, tensor.dim(), ops._layout(tensor), iq.HALF_FALLBACKS == fb,
                          ops.LAYOUT_COPIES == copies, out.dtype == tensor.dtype and out.stride() == tensor.stride()))
        return out
    monkeypatch.setattr(iq.IntQuantizer, '__call__', wrapper)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            res = H.run(H.build_parser().parse_args(base + ['-sm', 'use', '-c', 'laplace']), quiet=True)
    finally:
        Singleton.reset()
    assert res['output_finite']
    clipped = [c for c in calls if c[0] == 'laplace' and c[1]]
    assert sum(c[2] == 4 and c[3] == 'nhwc' for c in clipped) >= 10, calls
    assert all(c[4] for c in calls), 'an activation call took the half-precision upcast'
    assert all(c[5] for c in calls), 'an activation call copied its input'
    assert all(c[6] for c in calls), 'an activation result changed dtype or layout'
