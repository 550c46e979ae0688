"""INTEGRATION.md section 2, replayed: the REFERENCE's own manager module, imported unmodified with the sys.modules shims
that section shows, builds its tag -> quantizer table out of THIS package's IntQuantizer.  What it does to the quantizers
was recorded once from the reference (tests/golden/make_golden_shim.py -> shim.npz): per quantizer the factory call and
every attribute set after construction, in order, and the table it ended with.  Replayed here against the package alone:
the modules the shims name exist, the factory takes the reference's call, the attribute surface the reference pokes at
after construction exists and behaves (inference_quantization_manager.py:407-476, 549-562), and the reprs equal those the
reference's own quantizers print for the same flags.  The package's own manager builds the same table.  No tensor is
quantized (that needs the GPU)."""
import ast
import importlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the modules INTEGRATION.md section 2 puts in sys.modules in place of the reference's: reference name -> this package's
SHIMS = {
    'int_quantization': 'cnn_quantization_amd.int_quantization',
    'pytorch_quantizer.quantization.qtypes.int_quantizer': 'cnn_quantization_amd.qtypes.int_quantizer',
    'pytorch_quantizer.quantization.qtypes.dummy_quantizer': 'cnn_quantization_amd.qtypes.dummy_quantizer',
    'pytorch_quantizer.quantization.inference.statistic_manager_perchannel': 'cnn_quantization_amd.inference.statistic_manager_perchannel',
    'pytorch_quantizer.quantization.inference.statistic_manager': 'cnn_quantization_amd.inference.statistic_manager',
}
# what the reference takes from each of them (inference_quantization_manager.py imports, qtypes/__init__.py, iq.py:614)
NAMES = {
    'int_quantization': ('float2gemmlowp',),
    'pytorch_quantizer.quantization.qtypes.int_quantizer': ('int_quantizer', 'IntQuantizer'),
    'pytorch_quantizer.quantization.qtypes.dummy_quantizer': ('DummyQuantizer',),
    'pytorch_quantizer.quantization.inference.statistic_manager_perchannel': ('StatisticManagerPerChannel',),
    'pytorch_quantizer.quantization.inference.statistic_manager': ('StatisticManager',),
}

OWN_MANAGER = r'''
import argparse, ast, os, sys, tempfile
os.environ['HOME'] = tempfile.mkdtemp()
sys.path.insert(0, %(root)r)
import numpy as np
from cnn_quantization_amd.inference import inference_quantization_manager as iqm
z = np.load(%(npz)r, allow_pickle=False)
args = dict(ast.literal_eval(str(z['args'][0])))
qp = {k: dict(v) for k, v in ast.literal_eval(str(z['qparams'][0]))}
with iqm.QuantizationManagerInference(argparse.Namespace(**args), qp) as qm:
    om = qm.op_manager
    for tag, q in om.quantizers.items():
        print('TABLE', tag, '|', repr(q))
    print('IGNORE', '|'.join(om.ignore_ids))
'''


def _split(rows, n):
    return [str(r).split('|', n) for r in rows]


def test_reference_manager_builds_its_table_from_our_quantizer(golden, tmp_path, monkeypatch):
    monkeypatch.setenv('HOME', str(tmp_path))
    mods = {}
    for ref_name, ours in SHIMS.items():
        mods[ref_name] = importlib.import_module(ours)
        for n in NAMES[ref_name]:
            assert hasattr(mods[ref_name], n), (ours, n)
    IntQuantizer = mods['pytorch_quantizer.quantization.qtypes.int_quantizer'].IntQuantizer
    factory = mods['pytorch_quantizer.quantization.qtypes.int_quantizer'].int_quantizer
    classes = {'StatisticManager': mods['pytorch_quantizer.quantization.inference.statistic_manager'].StatisticManager,
               'StatisticManagerPerChannel':
                   mods['pytorch_quantizer.quantization.inference.statistic_manager_perchannel'].StatisticManagerPerChannel,
               'DummyQuantizer': mods['pytorch_quantizer.quantization.qtypes.dummy_quantizer'].DummyQuantizer}

    g = golden('shim')
    args = dict(ast.literal_eval(str(g.np('args')[0])))
    qparams = {k: dict(v) for k, v in ast.literal_eval(str(g.np('qparams')[0]))}
    assert args['qtype'] == 'int4' and args['per_channel_quant_act'] and qparams['int']['clipping'] == 'laplace'

    # the reference's factory calls and attribute assignments, in its order
    made = [factory(qtype, qparams[key] if key else {}) for qtype, key in _split(g.np('made'), 1)]
    for i, attr, text in _split(g.np('sets'), 2):
        q = made[int(i)]
        assert hasattr(q, attr) or attr == 'bit_alloc', (i, attr)       # bit_alloc: the reference's manager adds it itself
        setattr(q, attr, classes[text[6:]] if text.startswith('class:') else ast.literal_eval(text))

    def resolve(ref):
        return classes[ref[6:]]() if ref.startswith('class:') else made[int(ref)]
    table = {tag: resolve(ref) for tag, ref in _split(g.np('table'), 1)}
    default = resolve(str(g.np('default')[0]))
    ignore_ids = [str(s) for s in g.np('ignore_ids') if str(s)]

    for tag in ('activation', 'activation_linear', 'activation_pooling', 'activation_classifier', 'weight',
                'weight_classifier', 'ignored'):
        assert type(table[tag]) is IntQuantizer, (tag, type(table[tag]))
    assert type(default) is IntQuantizer and type(table['bias']) is classes['DummyQuantizer']
    assert table['activation'].clipping == 'laplace' and table['activation'].pcq_a and not table['activation'].pcq_w
    assert table['activation_pooling'].num_bits == 8 and table['activation_pooling'].clipping == 'no'
    assert table['activation_linear'].sm is classes['StatisticManager'] and not table['activation_linear'].pcq_a
    assert table['activation'].sm is classes['StatisticManagerPerChannel']
    assert ignore_ids == ['conv0_activation']
    # the replay prints what the package printed inside the reference's manager
    recorded = dict(_split(g.np('reprs'), 1))
    mine = {tag: repr(q) for tag, q in table.items()}
    assert mine == recorded

    # the reprs equal those the reference's own quantizers print for the same flags (golden trace, cfg3)
    ref_reprs = {}
    for line in golden('manager').np('cfg3/trace'):
        tag, _, rep = [t.strip() for t in str(line).split('|')[:3]]
        ref_reprs.setdefault(tag.replace('Quantize', '').strip(), rep)
    for tag in ('activation', 'activation_pooling', 'activation_classifier', 'weight', 'weight_classifier'):
        assert mine[tag] == ref_reprs[tag], (tag, mine[tag], ref_reprs[tag])

    # the package's own manager (a process of its own: it patches torch.nn while open) builds the same table
    npz = os.path.join(ROOT, 'tests', 'golden', 'shim.npz')
    out = subprocess.run([sys.executable, '-c', OWN_MANAGER % dict(root=ROOT, npz=npz)], capture_output=True, text=True,
                         timeout=300)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    own = dict(l[len('TABLE '):].split(' | ', 1) for l in out.stdout.splitlines() if l.startswith('TABLE '))
    assert own == recorded
    assert [l for l in out.stdout.splitlines() if l.startswith('IGNORE ')] == ['IGNORE ' + '|'.join(ignore_ids)]
