#!/usr/bin/env python3
"""Golden vectors for the KLD calibration row on bf16 / fp16 activations, produced by RUNNING THE REFERENCE.

Runs only where the reference is (CNNQ_REFERENCE).  The reference's
pytorch_quantizer/quantization/inference/kld_threshold.py is loaded unmodified by file path, exactly as
make_golden_kld.py loads it, and is handed float64-widened input (see the numpy note there).  The inputs are
make_golden_kld.py's cases except `huge_zero` (17 M elements: a count above 2^24 is the fp32 fixture's ground),
each rounded to nearest-even into bf16 and into fp16, plus
  f16_edges   +-65504 (the largest finite fp16), subnormals of both signs, -0.0 and +0.0 among ordinary values (fp16 only)
  bf16_max    +-bf16's largest finite value, 0x7f7f = 3.3895e38, among ordinary values (bf16 only): every other
              element falls into the zero bin
bf16 keeps 8 bits of mantissa, so its values leave most of the 2001 bins empty: the ground the search sees nowhere else.

Stored (tests/golden/kld_half.npz), per case <name> and dtype <dt> in (bf16, f16): the rounded input as its uint16 bit
patterns (`in_<dt>_<name>`), and the reference's min, max, minimal divergence and threshold on the exactly upconverted
values (`min_`, `max_`, `div_`, `th_`).  Inputs and outputs only.

    python tests/golden/make_golden_kld_half.py
"""
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_kld as base   # noqa: E402  (loads the reference's kld_threshold.py by path: base.kld)

DTYPES = {'bf16': torch.bfloat16, 'f16': torch.float16}


def to_bits(arr, dt):
    """float32 values rounded to nearest-even into dt: the uint16 patterns."""
    return torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float32)).to(dt).view(torch.int16).numpy().view(np.uint16).copy()


def from_bits(bits, dt):
    """The exact float64 values of uint16 patterns of dt."""
    return torch.from_numpy(bits.view(np.int16).copy()).view(dt).double().numpy()


def cases():
    out = {(name, dt): to_bits(arr, DTYPES[dt]) for name, arr in base.cases().items() if name != 'huge_zero' for dt in DTYPES}
    rng = np.random.default_rng(20251021)
    e = base.laplace(rng, 6000, 0.0, 900.0)
    e[:12] = [65504., -65504., 5.9604645e-08, -5.9604645e-08, 6.0975552e-05, -6.0975552e-05, 3.0e-06, -3.0e-06, -0.0, 0.0, 65504., -0.0]
    out[('f16_edges', 'f16')] = to_bits(rng.permutation(e), torch.float16)
    b = base.laplace(rng, 6000, 0.0, 1.0e30)
    bmax = np.array([0x7f7f0000], np.uint32).view(np.float32)[0]
    b[:4] = [bmax, -bmax, bmax, -0.0]
    out[('bf16_max', 'bf16')] = to_bits(rng.permutation(b), torch.bfloat16)
    return out


def main():
    rec = {}
    for (name, dt), bits in cases().items():
        arr = from_bits(bits, DTYPES[dt])
        assert np.isfinite(arr).all(), (name, dt)
        with warnings.catch_warnings():
            warnings.simplefilter('ignore')
            mn, mx, div, th = base.kld._get_optimal_threshold(arr, num_bins=2001, num_quantized_bins=15)
            th15 = base.kld.get_kld_threshold_15bins(arr)
        assert th15 == th
        key = '%s_%s' % (dt, name)
        rec['in_' + key] = bits
        rec['min_' + key] = np.float64(mn)
        rec['max_' + key] = np.float64(mx)
        rec['div_' + key] = np.float64(div)
        rec['th_' + key] = np.float64(th)
        print('%-22s n=%6d  min %.6g max %.6g  min_div %.6g  th %.7g' % (key, arr.size, mn, mx, div, th))
    rec['edge_dtype'] = np.array('float64')
    path = os.path.join(HERE, 'kld_half.npz')
    np.savez_compressed(path, **rec)
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
