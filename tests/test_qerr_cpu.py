"""Clipping-error columns, everything that needs no GPU: the CPU restatement against rows produced by the reference
(tests/golden/qerr.npz, tests/golden/make_golden_qerr.py), and the host logic of the new entry points."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from cnn_quantization_amd import _build
from cnn_quantization_amd import _lib as L
from cnn_quantization_amd.inference import statistic_manager_perchannel as smpc
from cnn_quantization_amd.utils.misc import Singleton

import _qerr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, 'tests', 'golden', 'qerr.npz'))


@pytest.mark.parametrize('name', [str(n) for n in GOLD['names']])
def test_restatement_reproduces_reference_rows(name):
    """Tier (ii) bound for sums, 2e-6 relative: the reference reduces in fp32, the restatement in fp64."""
    half, baa = name[4] == '1', name[-1] == '1'
    x = torch.from_numpy(GOLD['x'])
    stats = {k: GOLD['stat_' + k] for k in ('min', 'max', 'mean', 'b', 'std')}
    rows, qs = _qerr.mix_columns(x, stats, num_bits=4, positive=half, bit_alloc=baa)
    for cand, q in zip(_qerr.CANDS, qs):
        assert np.array_equal(q.numpy(), GOLD['%s_q_%s' % (name, cand)]), cand   # the candidates themselves: bit for bit
    rows = _qerr.host_post(rows)
    for i, en in enumerate(_qerr.NAMES):
        ref = GOLD['%s_%s' % (name, en)]
        print(name, en, 'max rel err %.3g' % _qerr.rel_err(rows[i], ref))
        assert _qerr.close(rows[i], ref, 2e-6), en


def test_names_in_reference_order(tmp_path, monkeypatch):
    monkeypatch.setenv('HOME', str(tmp_path))
    Singleton._instances.pop(smpc.StatisticManagerPerChannel, None)
    try:
        sm = smpc.StatisticManagerPerChannel('qerr_names', load_stats=False, collect_err=True, group=False)
        assert [str(s) for s in GOLD['stats_names']] == sm.stats_names
        assert sm.stats_names[-6:] == list(_qerr.NAMES)
    finally:
        Singleton._instances.pop(smpc.StatisticManagerPerChannel, None)


def test_collect_err_without_settings_raises(tmp_path, monkeypatch):
    monkeypatch.setenv('HOME', str(tmp_path))
    Singleton._instances.pop(smpc.StatisticManagerPerChannel, None)
    try:
        sm = smpc.StatisticManagerPerChannel('qerr_none', load_stats=False, collect_err=True, group=False)
        with pytest.raises(ValueError, match='err_settings'):
            sm.save_tensor_stats(torch.zeros(2, 3, 4, 4), 'activation', 'conv0_activation')
    finally:
        Singleton._instances.pop(smpc.StatisticManagerPerChannel, None)


def _lib():
    _build.build()
    return L.load()


def test_qerr_rejects_bad_arguments_without_a_device():
    lib = _lib()
    one = ctypes.c_void_p(8)      # never dereferenced: every call below is refused on its arguments
    for K in (0, 4, -1):
        assert lib.cnnq_pc_qerr_workspace(4, 8, 16, K) == 0
        assert lib.cnnq_pc_qerr(one, 4, 8, 16, one, K, None, one, one, None) == -1
    for N, C, HW in ((0, 8, 16), (4, 0, 16), (4, 8, 0), (-1, 8, 16)):
        assert lib.cnnq_pc_qerr_workspace(N, C, HW, 3) == 0
        assert lib.cnnq_pc_qerr(one, N, C, HW, one, 3, None, one, one, None) == -1
    for hole in range(4):
        ptrs = [one, one, one, one]
        ptrs[hole] = None
        x, qp, ws, err = ptrs
        assert lib.cnnq_pc_qerr(x, 4, 8, 16, qp, 3, None, ws, err, None) == -1


def test_qerr_workspace_is_the_row_records():
    """fp64 records [N * pieces][1 + 3K][C]; pieces > 1 only where a workgroup owns a slice of a channel (512 loads of 4
    floats, or of 1 where rows are not whole float4s), the larger of the aligned and the unaligned plan."""
    lib = _lib()
    for (N, C, HW) in ((4, 8, 16), (3, 5, 49), (2, 3, 112 * 112), (8, 64, 56 * 56), (1, 7, 33), (2, 2, 1500)):
        pieces = max(-(-HW // 512), 1) if HW > 512 else 1      # the VEC1 plan (unaligned pointer) is the larger one
        for K in (1, 2, 3):
            assert lib.cnnq_pc_qerr_workspace(N, C, HW, K) == N * pieces * C * (1 + 3 * K) * 8, (N, C, HW, K)


def test_header_declares_what_the_library_exports():
    """Every cnnq_* symbol the library exports is declared in the header and bound in _lib.SIGNATURES, the new ones among them."""
    import subprocess
    hdr = open(os.path.join(ROOT, 'include', 'cnnq_hip.h')).read()
    _lib()
    nm = '/opt/rocm/lib/llvm/bin/llvm-nm' if os.path.exists('/opt/rocm/lib/llvm/bin/llvm-nm') else 'nm'   # ROCm ships one
    out = subprocess.run([nm, '-D', '--defined-only', _build.LIB], check=True, capture_output=True, text=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith('cnnq_')}
    assert {'cnnq_pc_qerr_workspace', 'cnnq_pc_qerr'} <= exported
    for name in sorted(exported):
        assert re.search(r'\b%s\s*\(' % name, hdr), name
        assert name in L.SIGNATURES, name
