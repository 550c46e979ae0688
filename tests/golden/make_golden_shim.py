#!/usr/bin/env python3
"""INTEGRATION.md section 2, recorded: the REFERENCE's QuantizationManagerInference, imported unmodified with the
sys.modules shims that section shows, builds its tag -> quantizer table out of THIS package's IntQuantizer.  Recorded per
quantizer the factory call (`qtypes.int_quantizer(qtype, qparams[...])`) and every attribute the manager sets on it after
construction, in order; the table (tag -> quantizer), the default quantizer, the ignore list and the reprs.
tests/test_reference_shim_cpu.py replays the record against the package alone.

Needs the reference tree: CNNQ_REFERENCE=<path to the reference checkout> python tests/golden/make_golden_shim.py
Output: tests/golden/shim.npz (strings only)."""
import argparse
import os
import sys
import tempfile
import types

import numpy as np

REF = os.environ['CNNQ_REFERENCE']
OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))
os.environ['HOME'] = tempfile.mkdtemp(prefix='cnnq_golden_shim_')
sys.path.insert(0, ROOT)

import torch.nn as nn  # noqa: E402

from cnn_quantization_amd import int_quantization  # noqa: E402
import cnn_quantization_amd.qtypes.int_quantizer  # noqa: E402,F401
import cnn_quantization_amd.qtypes.dummy_quantizer  # noqa: E402,F401
import cnn_quantization_amd.inference.statistic_manager_perchannel  # noqa: E402,F401
import cnn_quantization_amd.inference.statistic_manager  # noqa: E402,F401

IQ = sys.modules['cnn_quantization_amd.qtypes.int_quantizer']       # qtypes re-exports the factory under this name

# the same flags as tests/test_reference_shim_cpu.py (ARGS, QPARAMS there)
ARGS = dict(arch='resnet50', qtype='int4', qweight='int4', q_off=False, stats_mode='no', stats_folder=None, kld_threshold=False,
            per_channel_quant_act=True, stats_batch_avg=False, bias_corr_act=False, bias_corr_weight=True, var_corr_weight=False,
            measure_stats=False)
QPARAMS = {'int': dict(clipping='laplace', stats_kind='mean', true_zero=False, kld=False, pcq_weights=True, pcq_act=True,
                       bit_alloc_act=True, bit_alloc_weight=True, bit_alloc_rmode='round', bit_alloc_prior='gaus',
                       bit_alloc_target_act=None, bit_alloc_target_weight=None, bcorr_act=False, bcorr_weight=True,
                       vcorr_weight=False, logger=None, measure_entropy=False, mtd_quant=False),
           'qmanager': {'rho_act': None, 'rho_weight': None}}


class Recorded(IQ.IntQuantizer):
    """An IntQuantizer that logs the attributes set on it once the factory has returned it."""
    def __setattr__(self, k, v):
        log = self.__dict__.get('_log')
        if log is not None:
            log.append((k, v))
        object.__setattr__(self, k, v)


made = []
_factory = IQ.int_quantizer


def recording_factory(qtype, quant_params):
    q = _factory(qtype, quant_params)
    q.__class__ = Recorded
    key = next((k for k, v in QPARAMS.items() if v is quant_params), None)
    assert key is not None or quant_params == {}, 'the manager handed the factory a parameter dict of its own'
    q.__dict__['_log'] = []
    made.append((qtype, key or '', q))
    return q


IQ.int_quantizer = recording_factory

# ---- the shims of INTEGRATION.md section 2
sys.modules['int_quantization'] = int_quantization
sys.modules['pytorch_quantizer.quantization.qtypes.int_quantizer'] = sys.modules['cnn_quantization_amd.qtypes.int_quantizer']
sys.modules['pytorch_quantizer.quantization.qtypes.dummy_quantizer'] = sys.modules['cnn_quantization_amd.qtypes.dummy_quantizer']
sys.modules['pytorch_quantizer.quantization.inference.statistic_manager_perchannel'] = \
    sys.modules['cnn_quantization_amd.inference.statistic_manager_perchannel']
sys.modules['pytorch_quantizer.quantization.inference.statistic_manager'] = \
    sys.modules['cnn_quantization_amd.inference.statistic_manager']
tv = types.ModuleType('torchvision')
tv.models = types.ModuleType('torchvision.models')
tv.models.Inception3 = type('Inception3', (nn.Module,), {})
sys.modules['torchvision'] = tv
sys.modules['torchvision.models'] = tv.models
sys.path.insert(0, REF)
from pytorch_quantizer.quantization.inference import inference_quantization_manager as iqm  # noqa: E402


def value_text(v):
    if isinstance(v, type):
        return 'class:' + v.__name__
    assert v is None or isinstance(v, (bool, int, float, str)), (type(v), v)
    return repr(v)


def ref_of(q):
    i = next((i for i, m in enumerate(made) if m[2] is q), None)
    return str(i) if i is not None else 'class:' + type(q).__name__


with iqm.QuantizationManagerInference(argparse.Namespace(**ARGS), QPARAMS) as qm:
    om = qm.op_manager
    logs = []
    for _, _, q in made:
        logs.append(q.__dict__['_log'])
        q.__dict__['_log'] = None
    rec = {
        'args': np.array([repr(sorted(ARGS.items()))]),
        'qparams': np.array([repr(sorted((k, sorted(v.items())) for k, v in QPARAMS.items()))]),
        'made': np.array(['%s|%s' % (qtype, key) for qtype, key, _ in made]),
        'sets': np.array(['%d|%s|%s' % (i, k, value_text(v)) for i, log in enumerate(logs) for k, v in log]),
        'table': np.array(['%s|%s' % (tag, ref_of(q)) for tag, q in om.quantizers.items()]),
        'default': np.array([ref_of(om.quantizer_default)]),
        'ignore_ids': np.array(list(om.ignore_ids) or ['']),
        'reprs': np.array(['%s|%s' % (tag, repr(q)) for tag, q in om.quantizers.items()]),
    }
np.savez(os.path.join(OUT, 'shim.npz'), **rec)
for k, v in rec.items():
    print(k, len(v))
