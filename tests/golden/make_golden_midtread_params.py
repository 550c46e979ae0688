#!/usr/bin/env python3
"""Golden vectors for the mid-tread bin allocation and clipping multiplier (int_quantizer.py:128-145) by RUNNING THE REFERENCE:
its own get_omega(...).round() and get_alpha_mult(omega, sym) on the guarded std vectors of tests/_midtread_params.py
(GOLDEN_CELLS: C <= 1025, omegas inside the interpolation table), both ranges.  Results only - std, target, omega, alpha.  Build
container only (needs the reference checkout); output tests/golden/midtread_params.npz.

get_alpha_mult doubles the caller's omega in place on the CPU, where .cpu().numpy() aliases; on the GPU, the reference's device,
it does not.  As tests/golden/make_golden.py does, the driver hands it a clone, so the fixture encodes GPU semantics.

    python tests/golden/make_golden_midtread_params.py
"""
import os
import sys
import tempfile
import types
import zipfile

import numpy as np

REF = os.environ.get('CNNQ_REFERENCE', '/root/reference')
OUT = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(OUT)
os.environ['HOME'] = tempfile.mkdtemp(prefix='cnnq_golden_mtp_')
sys.path.insert(0, REF)
sys.modules['int_quantization'] = types.ModuleType('int_quantization')

import torch  # noqa: E402
import pytorch_quantizer.quantization.qtypes.int_quantizer  # noqa: E402,F401

iq = sys.modules['pytorch_quantizer.quantization.qtypes.int_quantizer']

# ---- GPU semantics for get_alpha_mult (defensive clone in the driver) -----------------------
_orig_alpha_mult = iq.IntQuantizer.get_alpha_mult


def _alpha_mult_gpu_semantics(omega, sym=True):
    return _orig_alpha_mult(omega.clone(), sym=sym)


iq.IntQuantizer.get_alpha_mult = staticmethod(_alpha_mult_gpu_semantics)

for p in (TESTS, os.path.dirname(TESTS)):
    if p not in sys.path:
        sys.path.append(p)
import _midtread_params as M  # noqa: E402  (the cell list and the generator of the priors: data, shared with the tests)


def save(path, d):
    """np.savez_compressed with a fixed time stamp on every member, so that the file regenerates byte for byte."""
    with zipfile.ZipFile(path, 'w', zipfile.ZIP_DEFLATED) as z:
        for k, v in d.items():
            info = zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with z.open(info, 'w') as f:
                np.lib.format.write_array(f, np.asanyarray(v), allow_pickle=False)


def main():
    torch.set_num_threads(1)
    d = {}
    names = []
    for C, target in M.GOLDEN_CELLS:
        std = M.guarded_prior(C, M.CELLS[(C, target)])
        tgt = int(target) if float(target) == int(target) else float(target)
        omega = iq.IntQuantizer.get_omega(std, target_bins=(2 ** tgt)).round()
        key = 'c%d_t%s' % (C, str(target).replace('.', 'p'))
        names.append(key)
        d[key + '_std'], d[key + '_target'], d[key + '_omega'] = std.numpy(), np.float64(target), omega.numpy()
        for sym in (True, False):
            assert float(omega.max()) * (1 if sym else 2) <= float(iq.omega_table[-1]), (key, sym)
            d['%s_alpha_sym%d' % (key, sym)] = np.asarray(iq.IntQuantizer.get_alpha_mult(omega, sym=sym), dtype=np.float64)
    d['names'] = np.array(names)
    path = os.path.join(OUT, 'midtread_params.npz')
    save(path, d)
    print('wrote %s (%d arrays, %.1f KB)' % (path, len(d), os.path.getsize(path) / 1024.))


if __name__ == '__main__':
    main()
