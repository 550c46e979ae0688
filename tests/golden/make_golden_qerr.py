#!/usr/bin/env python3
"""Golden vectors for the per-channel clipping-error columns (statistic_manager_perchannel.py:24-32, 80-100) by RUNNING THE
REFERENCE.  The reference never passes itself the quantized tensors these columns need, so this script does what its code
expects: `tensors_q = {orig, lowp, gaus, laplace}` built with the reference's own IntQuantizer in `-sm use -c mix` mode (the
error columns of the loaded file forced so that every channel picks the wanted candidate), handed to the reference's
save_tensor_stats.  Build container only (needs the reference checkout); output tests/golden/qerr.npz.

Shape [6, 12, 5, 7]: rows of 35 elements, so that the reference's fp32 reductions stay inside the 2e-6 bound of the fp64
restatement (tests/_qerr.py).

    python tests/golden/make_golden_qerr.py
"""
import os
import pickle
import sys
import tempfile
import types

import numpy as np

REF = os.environ.get('CNNQ_REFERENCE', '/root/reference')
OUT = os.path.dirname(os.path.abspath(__file__))
os.environ['HOME'] = tempfile.mkdtemp(prefix='cnnq_golden_qerr_')
sys.path.insert(0, REF)
sys.modules['int_quantization'] = types.ModuleType('int_quantization')

import torch  # noqa: E402
import pytorch_quantizer.quantization.qtypes.int_quantizer  # noqa: E402,F401

iq = sys.modules['pytorch_quantizer.quantization.qtypes.int_quantizer']
from pytorch_quantizer.quantization.inference import statistic_manager_perchannel as smpc  # noqa: E402

SEVEN = ['max', 'min', 'std', 'mean', 'kurtosis', 'b', 'std_pos']
ERR = ['mse_lowp', 'mse_gaus', 'mse_laplace', 'cos_lowp', 'cos_gaus', 'cos_laplace']
# (mse_laplace, mse_gaus, mse_lowp) that make iq.py:310-323 pick the candidate for every channel
FORCE = {'laplace': (1., 2., 3.), 'gaus': (2., 1., 3.), 'lowp': (3., 2., 1.)}


class _Logger:
    def log_metric(self, *a, **k):
        pass


def params(**kw):
    p = dict(clipping='mix', stats_kind='mean', true_zero=False, kld=False, pcq_weights=False, pcq_act=True,
             bit_alloc_act=False, bit_alloc_weight=False, bit_alloc_rmode='round', bit_alloc_prior='gaus',
             bit_alloc_target_act=None, bit_alloc_target_weight=None, bcorr_act=False, bcorr_weight=False,
             vcorr_weight=False, logger=_Logger(), measure_entropy=False, mtd_quant=False)
    p.update(kw)
    return p


def fresh(name, **kw):
    smpc.Singleton._instances.pop(smpc.StatisticManagerPerChannel, None)
    return smpc.StatisticManagerPerChannel(name, **kw)


def main():
    g = torch.Generator().manual_seed(4242)
    shape = (6, 12, 5, 7)
    C = shape[1]
    u = torch.rand(shape, generator=g) - 0.5
    x = (-torch.sign(u) * torch.log1p(-2 * u.abs()) * torch.exp(torch.randn(1, C, 1, 1, generator=g) * 0.7)
         + torch.randn(1, C, 1, 1, generator=g) * 0.3).float()
    d = {'x': x}
    sm = fresh('golden_qerr', load_stats=False, stats=list(SEVEN))
    for _ in range(2):   # the reference's summary needs more than one batch per layer; twice the same: the means are x's own
        sm.save_tensor_stats(x, 'activation', 'conv0_activation')
    sm.__exit__()
    names = []
    for half in (False, True):
        for baa in (False, True):
            tq = {'orig': x}
            for cand, (ml, mg, mp) in FORCE.items():
                sm2 = fresh('golden_qerr', load_stats=True)
                st = sm2.stats['conv0_activation']
                full = lambda v: np.full(C, v, dtype=np.float32)
                st['mean_mse_laplace'], st['mean_mse_gaus'], st['mean_mse_lowp'] = full(ml), full(mg), full(mp)
                if not names and cand == 'laplace':
                    for k in ('min', 'max', 'mean', 'b', 'std'):
                        d['stat_' + k] = np.asarray(st['mean_' + k], dtype=np.float32)
                q = iq.int_quantizer('int4', params(bit_alloc_act=baa))
                q.half_range = half
                tq[cand] = q(x, 'conv0_activation', 'activation', stat_id='conv0_activation').clone()
            sm3 = fresh('golden_qerr_out', load_stats=False, stats=list(SEVEN), collect_err=True)
            sm3.save_tensor_stats(x, 'activation', 'conv0_activation', tensors_q=tq)
            nm = 'half%d_baa%d' % (half, baa)
            names.append(nm)
            for e in ERR:
                d['%s_%s' % (nm, e)] = np.asarray(sm3.stats['conv0_activation'][e], dtype=np.float32)
            for s in SEVEN:
                d['%s_%s' % (nm, s)] = np.asarray(sm3.stats['conv0_activation'][s], dtype=np.float32)
            for cand in FORCE:
                d['%s_q_%s' % (nm, cand)] = tq[cand]
    d['names'] = np.array(names)
    d['stats_names'] = np.array(sm3.stats_names)
    np.savez_compressed(os.path.join(OUT, 'qerr.npz'), **{k: (v.numpy() if isinstance(v, torch.Tensor) else v) for k, v in d.items()})
    print('qerr.npz:', len(d), 'arrays;', names, list(sm3.stats_names))


if __name__ == '__main__':
    main()
