"""IntQuantizer's route decision against the truth table recorded before the decision was gathered in one place
(tests/golden/routes.npz, written by tests/golden/make_golden_routes.py): at every point of the recorded grids the ten predicates, the
branch method __call__ reaches and whether it upcasts first answer bit for bit what was recorded, and the predicates that are true
are exactly the ones the point's route name implies.  Nothing is launched."""
import importlib.util
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
spec = importlib.util.spec_from_file_location('make_golden_routes', os.path.join(GOLDEN, 'make_golden_routes.py'))
G = importlib.util.module_from_spec(spec)
spec.loader.exec_module(G)

# route name -> the predicates that view it (the route table of DESIGN.md section 26)
IMPLIES = {None: (), 'kld': ('_flat_kld',), 'flat_clip': ('_flat_clip',), 'flat_midtread': ('_flat_midtread',),
           'nhwc_midtread': ('_nhwc_midtread',), 'nhwc_entropy': ('_nhwc_entropy',), 'half_table': ('_half_table',),
           'half_aciq': ('_half_aciq',), 'half_minmax': ('_half_table', '_half_native'), 'nhwc_aciq': ('_nhwc_aciq', '_half_native'),
           'nhwc_bcorr': ('_nhwc_bcorr', '_half_native'), 'minmax_pc': ('_half_native',), 'minmax_pt': ('_half_native',)}
METHOD = {'kld': 'gemmlowpKldQuantize', 'midtread': 'mid_tread_quantize_activation', 'clip': 'gemmlowpClippingQuantize',
          'midtread_w': 'mid_tread_quantize_weights_per_channel', 'weights': 'gemmlowpQuantizeWeightsPerChannel',
          'midtread_pc': 'mid_tread_quantize_activation_per_channel', 'pc': 'gemmlowpQuantizeActivationPerChannel',
          'minmax': 'gemmlowpMinMaxQuantize'}


def describe(section, q, x, stat_id, override, clip):
    return (section, dict(clipping=q.clipping, num_bits=q.num_bits, bit_alloc_act=q.bit_alloc_act, bit_alloc_prior=q.bit_alloc_prior,
                          pcq_a=q.pcq_a, pcq_w=q.pcq_w, mtd_quant=q.mtd_quant, kld=q.kld, measure_entropy=q.measure_entropy,
                          fuse_bcorr=q.fuse_bcorr, half_dynamic=q.half_dynamic, group=q.group),
            (tuple(x.shape), x.dtype, x.stride(), getattr(x, 'is_cuda', False)), stat_id, override, clip)


def test_routes_answer_as_recorded_and_imply_their_predicates():
    gold = np.load(os.path.join(GOLDEN, 'routes.npz'))
    count = int(gold['count'])
    want_bits = np.unpackbits(gold['bits'])[:count * 11].reshape(count, 11).astype(bool)
    want_branch = gold['branch']
    cls = G.probe_class()
    import sys
    iq = sys.modules[cls.__mro__[1].__module__]
    n, names = 0, set()
    for point in G.points(cls):
        section, q, x, stat_id, override, clip = point
        bits, reached = G.answers(iq, q, x, stat_id, override, clip)
        assert n < count, 'more points than recorded'
        assert bits == want_bits[n].tolist() and reached == want_branch[n], (n, describe(*point), bits, reached,
                                                                             want_bits[n].tolist(), int(want_branch[n]))
        n += 1
        if clip is not None:        # (the predicates were asked about another clipping than the one __call__ dispatches on)
            continue
        att = q._att(override)
        branch = q._branch(att, x)
        route = q._route(branch, x, stat_id, att)
        names.add(route)
        assert G.BRANCHES[reached] == METHOD[branch], describe(*point)
        assert bits[10] == (x.dtype in (torch.bfloat16, torch.float16) and route is None), (describe(*point), route)
        implied = set(IMPLIES[route])
        # the one view of level 2 alone: _nhwc_aciq ignores mtd_quant and kld, as a direct call of gemmlowpClippingQuantize does
        if branch in ('kld', 'midtread') and q._clip_route(x, att('clipping'), None, att) == 'nhwc_aciq':
            implied.add('_nhwc_aciq')
        assert {p for p, b in zip(G.PREDICATES, bits) if b} == implied, (describe(*point), route)
    assert n == count
    assert names == set(IMPLIES)                 # every route name occurs


def test_no_route_is_kept_on_the_object():
    from _quantizer import act, nhwc, quantizer
    q = quantizer(clipping='laplace', pcq_act=True)
    before = dict(vars(q))
    for x in (act(), nhwc()):
        q._route(q._branch(q._att(), x), x, 'id', q._att())
    assert vars(q) == before
