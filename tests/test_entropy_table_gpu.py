"""The entropy kernels on histograms whose entropy is known in advance (the cases and the conditions on them:
test_entropy_table_cpu.py; the builder and the fp64 reference: tests/_entropy.py).

cnnq_midtread_entropy / _count / _batch (k_mt_entropy, k_mt_entropy_batch) and cnnq_entropy / cnnq_entropy_replicas / _batch /
cnnq_hist_replicas_fold (k_entropy, k_entropy_replicas, k_hist_replicas_fold) get the words uploaded as they are.  Every entropy is
held to |H - H64| <= 2e-5 * max(1, H64) - the tier of test_entropy_batch_gpu.py against the reference's golden entropies; the CPU
file shows the float32 arithmetic itself stays four hundred times inside it, and that every mistake it knows moves a case by fifty
tiers - a table uniform over 2^k bins to |H - k| <= 1e-6, and everything that is integer work or the same arithmetic twice to
equality of bits.  Every test prints what it measured (-s).  Needs an MI355X: `pytest -m gpu`."""
import ctypes

import numpy as np
import pytest
import torch

import _entropy as E
import test_entropy_table_cpu as T
from cnn_quantization_amd import _lib, ops

pytestmark = pytest.mark.gpu
EINVAL = -1
SENTINEL = -7.25


def bits(t):
    return t.detach().cpu().numpy().view(np.int32).copy()


def result(n=1):
    return torch.full((n,), SENTINEL, dtype=torch.float32, device='cuda')


_UP = {}


def uploaded(name):
    """(words, mt) of a mid-tread case on the device, built once"""
    if name not in _UP:
        d, spread = T.MT_CASES[name]
        _UP[name] = (torch.from_numpy(E.mt_words(d, spread)).cuda(), torch.from_numpy(E.mt_table(d)).cuda())
    return _UP[name]


def mt_entropy(name):
    d, _ = T.MT_CASES[name]
    h, mt = uploaded(name)
    out = result()
    _lib.check(_lib.load().cnnq_midtread_entropy(ops._ptr(h), ops._ptr(mt), d.C, d.total, ops._ptr(out), ops._stream(h)),
               'cnnq_midtread_entropy')
    return out


@pytest.mark.parametrize('name', T.MT_NAMES)
def test_midtread_entropy(name):
    d, spread = T.MT_CASES[name]
    h, mt = uploaded(name)
    h64 = T.mt_reference(name)
    a, b = mt_entropy(name), mt_entropy(name)
    cnt = torch.tensor([d.total // d.C, -1.], dtype=torch.float64, device='cuda')
    c = result()
    _lib.check(_lib.load().cnnq_midtread_entropy_count(ops._ptr(h), ops._ptr(mt), d.C, ops._ptr(cnt), ops._ptr(c), ops._stream(h)),
               'cnnq_midtread_entropy_count')
    got = float(a)
    print('%-26s C %4d  H64 %.9f  H %.9f  |H - H64| %.3g  tier %.3g' % (name, d.C, h64, got, abs(got - h64), E.tier(h64)))
    assert np.isfinite(got) and abs(got - h64) <= E.tier(h64)
    if h64 == 0.:
        assert got == 0.                                          # 0.0 (or -0.0), not NaN
    assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), bits(c))
    assert np.array_equal(h.cpu().numpy(), E.mt_words(d, spread))                    # const: the words are as uploaded


# sixteen tensors of one launch: every C of the case list (2049 and 3000 take the global-memory scan), both flag states, wide counts
BATCH = ['C1', 'C31', 'C33_cross', 'C512', 'C2048_three_cmax', 'C2049_cross', 'C3000', 'clear_C31', 'clear_single_bin',
         'window_lowest', 'window_highest', 'window_past_the_table', 'two_symbols_2p33', 'window_and_clamp_2p33', 'clear_single_clamp',
         'wide_counts_2p40']


def mt_batch(names, C=None, total=None, n=None, out=None):
    n = len(names) if n is None else n
    m = max(len(names), 1)
    ups = [uploaded(x) for x in names]
    hp = (ctypes.c_void_p * m)(*[h.data_ptr() for h, _ in ups])
    mp = (ctypes.c_void_p * m)(*[t.data_ptr() for _, t in ups])
    cs = (ctypes.c_int64 * m)(*(C or [T.MT_CASES[x][0].C for x in names]))
    ts = (ctypes.c_int64 * m)(*(total or [T.MT_CASES[x][0].total for x in names]))
    out = result(20) if out is None else out
    rc = _lib.load().cnnq_midtread_entropy_batch(n, hp, mp, cs, ts, ops._ptr(out), ops._stream(out))
    return rc, out


def test_midtread_entropy_batch():
    assert len(BATCH) == 16 and {T.MT_CASES[x][0].C for x in BATCH} >= {1, 2, 3, 4, 31, 33, 512, 2048, 2049, 3000}
    single = np.concatenate([bits(mt_entropy(x)) for x in BATCH])
    rc, out = mt_batch(BATCH)
    assert rc == 0
    assert np.array_equal(bits(out[:16]), single)
    assert (out[16:] == SENTINEL).all()
    for x in ('C2049_cross', 'C33'):
        rc, out = mt_batch([x])
        assert rc == 0 and np.array_equal(bits(out[:1]), bits(mt_entropy(x))) and (out[1:] == SENTINEL).all()


def test_midtread_entropy_batch_refuses_bad_arguments_before_launching():
    names = BATCH + ['C33']
    Cs = [T.MT_CASES[x][0].C for x in BATCH]
    tot = [T.MT_CASES[x][0].total for x in BATCH]
    out = result(20)
    assert mt_batch(BATCH, n=0, out=out)[0] == EINVAL
    assert mt_batch(names, out=out)[0] == EINVAL                                     # n = 17
    assert mt_batch(BATCH, C=Cs[:5] + [0] + Cs[6:], out=out)[0] == EINVAL
    assert mt_batch(BATCH, total=tot[:15] + [0], out=out)[0] == EINVAL
    assert mt_batch(BATCH[:1], total=[0], out=out)[0] == EINVAL
    torch.cuda.synchronize()
    assert (out == SENTINEL).all()                                                    # nothing ran


def test_the_placement_over_the_replicas_does_not_change_a_bit():
    a, b, c = (bits(mt_entropy(x)) for x in T.PLACEMENTS)
    assert np.array_equal(a, b) and np.array_equal(a, c)


def test_window_form_and_global_form_agree_within_the_tier():
    hs = []
    for d in T.window_and_global_forms():
        h, mt, out = torch.from_numpy(E.mt_words(d)).cuda(), torch.from_numpy(E.mt_table(d)).cuda(), result()
        _lib.check(_lib.load().cnnq_midtread_entropy(ops._ptr(h), ops._ptr(mt), d.C, d.total, ops._ptr(out), ops._stream(h)),
                   'cnnq_midtread_entropy')
        h64 = E.entropy64(E.symbols(d), d.total)
        hs.append(float(out))
        assert abs(hs[-1] - h64) <= E.tier(h64)
    print('window form %.9f, global form %.9f' % tuple(hs))
    assert abs(hs[0] - hs[1]) <= E.tier(h64)


# ------------------------------------------------------------------------------------------ the uniform quantizers' tables
def check_uniform(name, got, counts):
    h64 = T.table_reference(counts)
    print('%-22s H64 %.9f  H %.9f  |H - H64| %.3g' % (name, h64, got, abs(got - h64)))
    assert np.isfinite(got) and abs(got - h64) <= E.tier(h64)
    if name.startswith('pow2_'):
        assert abs(got - float(name.split('_')[1])) <= T.POW2_TOL
    if not counts:
        assert got == 0.


@pytest.mark.parametrize('name', T.PLAIN_NAMES)
def test_entropy_of_a_plain_table(name):
    counts, nbins = T.PLAIN_CASES[name]
    words = E.plain_table(counts, nbins)
    h = torch.from_numpy(words).cuda()
    a, b = result(), result()
    for o in (a, b):
        _lib.check(_lib.load().cnnq_entropy(ops._ptr(h), nbins, ops._ptr(o), ops._stream(h)), 'cnnq_entropy')
    check_uniform(name, float(a), counts)
    assert np.array_equal(bits(a), bits(b)) and np.array_equal(h.cpu().numpy(), words)


@pytest.mark.parametrize('name', T.REPLICA_NAMES)
def test_entropy_of_replica_tables(name):
    counts, spread = T.REPLICA_CASES[name]
    lib = _lib.load()
    assert lib.cnnq_hist_replica_bytes() == E.XREP * E.XBINS * 8
    h = torch.from_numpy(E.replica_tables(counts, spread)).cuda()
    out = result()
    _lib.check(lib.cnnq_entropy_replicas(ops._ptr(h), ops._ptr(out), ops._stream(h)), 'cnnq_entropy_replicas')
    check_uniform(name, float(out), counts)
    assert int(h.abs().sum()) == 0                                                    # left zero for the next launch


def test_entropy_replicas_batch():
    lib = _lib.load()
    names = T.REPLICA_NAMES
    n = len(names)
    tables = np.stack([E.replica_tables(*T.REPLICA_CASES[x]) for x in names] + [np.full((E.XREP, E.XBINS), 0x0123456789abcdef, np.int64)])
    h = torch.from_numpy(tables).cuda()
    out = result(n + 1)
    _lib.check(lib.cnnq_entropy_replicas_batch(ops._ptr(h), n, ops._ptr(out), ops._stream(h)), 'cnnq_entropy_replicas_batch')
    for i, x in enumerate(names):
        check_uniform(x, float(out[i]), T.REPLICA_CASES[x][0])
        one, t1 = result(), torch.from_numpy(tables[i]).cuda()
        _lib.check(lib.cnnq_entropy_replicas(ops._ptr(t1), ops._ptr(one), ops._stream(t1)), 'cnnq_entropy_replicas')
        assert np.array_equal(bits(one), bits(out[i:i + 1])), x
    assert int(h[:n].abs().sum()) == 0
    assert np.array_equal(h[n].cpu().numpy(), tables[n])                              # the set behind them is not touched
    assert float(out[n]) == SENTINEL
    assert lib.cnnq_entropy_replicas_batch(ops._ptr(h), 0, ops._ptr(out), ops._stream(h)) == EINVAL


def test_the_spreading_over_the_replicas_does_not_change_a_bit():
    for live in (16, 256):
        got = []
        for how in ('one', 'even', 'random'):
            counts, spread = T.REPLICA_CASES['ramp_%d_%s' % (live, how)]
            h, out = torch.from_numpy(E.replica_tables(counts, spread)).cuda(), result()
            _lib.check(_lib.load().cnnq_entropy_replicas(ops._ptr(h), ops._ptr(out), ops._stream(h)), 'cnnq_entropy_replicas')
            got.append(bits(out))
        assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2])


@pytest.mark.parametrize('name', ['ramp_16_random', 'ramp_256_one', 'mixed_wide_counts', 'two_bins_2p33_even', 'empty'])
def test_fold_adds_the_exact_totals_to_a_table_that_was_not_zero(name):
    counts, spread = T.REPLICA_CASES[name]
    before = (np.arange(E.XBINS, dtype=np.int64) * 1000003 + 17) % 99991 + (np.arange(E.XBINS, dtype=np.int64) % 3 == 0) * (1 << 35)
    rep = torch.from_numpy(E.replica_tables(counts, spread)).cuda()
    hist = torch.from_numpy(before).cuda()
    _lib.check(_lib.load().cnnq_hist_replicas_fold(ops._ptr(rep), ops._ptr(hist), ops._stream(rep)), 'cnnq_hist_replicas_fold')
    assert np.array_equal(hist.cpu().numpy(), before + E.plain_table(counts, E.XBINS))
    assert int(rep.abs().sum()) == 0
