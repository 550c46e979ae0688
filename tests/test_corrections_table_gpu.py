"""The fp32 NCHW correction chains (csrc/cnnq_corrections.hip.h) against tests/_corrections.py: k_bcorr_sums, k_bcorr_bias,
k_bcorr_apply, k_qdq_bias (-bca) and k_weight_correct (-bcw), DESIGN.md section 15a.

The contract, as the channels_last and bf16 / fp16 routes have it (sections 15 and 24), which compare with this chain:
  1. the per-channel sums within 2e-6 of sum |term| of float64 - and EQUAL to it on the dyadic inputs, whose every partial sum is
     exact in every load shape and fold (A: every plan class of K.CLASSES, asserted through cnnq_plan_describe); the count exact;
  2. given the sums, the bias bit for bit (B: hand-built records), and given a bias, y bit for bit (C: hand-built bias and y,
     both walks, every misalignment);
  3. given the tables, the corrected weights bit for bit (D: hand-built tables).
The only tolerances in this file are that tier and the one of tests/test_stats_single_gpu.py for the statistics the weight
correction derives itself.  Each test prints the worst ratio it saw."""
import ctypes

import numpy as np
import pytest
import torch

import _corrections as K
from conftest import bits_equal

pytestmark = pytest.mark.gpu
F = np.float32
SMALL = [c for c in K.CLASSES if int(np.prod(c[0])) <= K.BIG]
GUARD = -777.


def mods():
    from cnn_quantization_amd import _lib as L, ops
    return L, ops


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(a, off=0):
    """the array on the device, its base pointer `off` elements past a 16-byte boundary"""
    a = torch.from_numpy(np.ascontiguousarray(a))
    base = torch.empty(a.numel() + 4, dtype=a.dtype, device='cuda')
    assert base.data_ptr() % 16 == 0
    view = base[off:off + a.numel()].view(a.shape)
    view.copy_(a)
    return view


def host(t):
    return t.detach().cpu().numpy()


def describe(N, C, HW, aligned, fine):
    L, _ = mods()
    out = (ctypes.c_int32 * 12)()
    assert L.load().cnnq_plan_describe(N, C, HW, int(aligned), fine, out) == 0
    return dict(zip(K.PLAN_WORDS, list(out)))


def al16(*ts):
    return all(t.data_ptr() % 16 == 0 for t in ts)


def assert_class(case, aligned):
    (N, C, H, W), off, want = case
    got = describe(N, C, H * W, aligned, 0)
    assert aligned == (off == 0) and {k: got[k] for k in want} == want, (K.class_id(case), got)
    return got


def merge(part3, G, C, want_sums=True, want_bias=True):
    """cnnq_pc_bcorr_bias on device records -> (sums [3, C] float64 or None, bias [C] or None) on the host"""
    L, _ = mods()
    sums = torch.full((3, C), GUARD, dtype=torch.float64, device='cuda') if want_sums else None
    bias = torch.full((C,), GUARD, dtype=torch.float32, device='cuda') if want_bias else None
    rc = L.load().cnnq_pc_bcorr_bias(part3.data_ptr(), G, C, sums.data_ptr() if want_sums else None,
                                     bias.data_ptr() if want_bias else None, stream())
    assert rc == 0, rc
    return (host(sums) if want_sums else None), (host(bias) if want_bias else None)


def sums_records(x, y, qp, relu_first):
    """cnnq_pc_bcorr_sums (y given) or cnnq_pc_qdq_bcorr_sums (qp given) -> part3[G][3][C] on the device.  The records are
    pre-filled with NaN and followed by a guard record: one that is not written, or written twice as far, shows."""
    L, _ = mods()
    lib = L.load()
    N, C, H, W = x.shape
    G = lib.cnnq_pc_groups(N, C, H * W, int(al16(x) if y is None else al16(x, y)))
    assert G > 0
    buf = torch.full((G + 1, 3, C), float('nan'), dtype=torch.float64, device='cuda')
    buf[G] = GUARD
    if y is None:
        rc = lib.cnnq_pc_qdq_bcorr_sums(x.data_ptr(), N, C, H * W, qp.data_ptr(), int(relu_first), buf.data_ptr(), stream())
    else:
        rc = lib.cnnq_pc_bcorr_sums(x.data_ptr(), y.data_ptr(), N, C, H * W, int(relu_first), buf.data_ptr(), stream())
    assert rc == 0, rc
    assert bool((buf[G] == GUARD).all()), 'a record was written past part3[G]'
    return buf[:G], G


def worst_ratio(dev_sum, ref, mag):
    with np.errstate(all='ignore'):
        r = np.abs(dev_sum - ref) / np.where(mag > 0, mag, 1.)
    return float(np.nanmax(r)) if r.size else 0.


def gaussian_case(shape, seed, relu_first, off=0):
    """x on the device at `off`, the 4-bit min/max table of its own statistics, q = pc_qdq(x) on the device (aligned) and host"""
    _, ops = mods()
    N, C, H, W = shape
    x = K.gaussian(shape, seed)
    xa = dev(x)
    stats, _ = ops.pc_stats(xa, N, C, H * W)
    qp, _ = ops.pc_params(stats, 4, bool(relu_first), 'no', False)
    qd = ops.pc_qdq(xa, N, C, H * W, qp)
    return x, (xa if off == 0 else dev(x, off)), qp, qd, host(qd)


# ------------------------------------------------------------------------------------------ A: the sums records
@pytest.mark.parametrize('case', K.CLASSES, ids=K.class_id)
def test_sums_dyadic_equal_float64(case):
    """every partial sum the kernel can form of the dyadic inputs is exact: sums == float64, no tolerance"""
    _, ops = mods()
    shape, off, _ = case
    N, C, H, W = shape
    plan = assert_class(case, off == 0)
    x, qp = K.dyadic(shape, seed=C + H)
    y2, _ = K.dyadic(shape, seed=C + H + 1000)
    xd, yd, qpd = dev(x, off), dev(y2, off), dev(qp)
    q = host(ops.pc_qdq(dev(x), N, C, H * W, qpd))
    assert K.same(q, K.qdq32(x, qp))
    for relu_first in (0, 1):
        for name, second, args in (('x/y', y2, (xd, yd, None)), ('fused', q, (xd, None, qpd))):
            ref, _ = K.sums64(x, second, relu_first)
            part3, G = sums_records(*args, relu_first)
            assert G == plan['G'] == plan['S'] * plan['nb']
            sums, bias = merge(part3, G, C)
            records = host(part3)
            assert not np.isnan(records).any(), 'a record was not written'
            for row, what in enumerate(('sum x', 'sum q', 'count')):
                assert np.array_equal(sums[row], ref[row]), (name, what, relu_first, K.where_differ(sums[row], ref[row]))
                assert np.array_equal(records[:, row].sum(0), ref[row]), (name, what, relu_first, 'records')
            assert bits_equal(bias, K.bias32(ref))
            again, _ = sums_records(*args, relu_first)
            assert K.same(host(again), records)
            if C > 1:
                assert sums[2][C - 1] == 0                                  # the all-negative channel divides by 1e-8f


@pytest.mark.parametrize('case', K.CLASSES, ids=K.class_id)
def test_sums_gaussian_within_the_tier(case):
    """|sum - float64| <= 2e-6 * sum |term|, the count exact; with y = pc_qdq(x) the fused form's
    records are the x/y form's, bit for bit"""
    shape, off, _ = case
    N, C, H, W = shape
    assert_class(case, off == 0)
    for relu_first in (0, 1):
        x, xd, qp, qd, q = gaussian_case(shape, 7 + C + relu_first, relu_first, off)
        yd = qd if off == 0 else dev(q, off)
        ref, mag = K.sums64(x, q, relu_first)
        records = {}
        for name, args in (('x/y', (xd, yd, None)), ('fused', (xd, None, qp))):
            part3, G = sums_records(*args, relu_first)
            sums, bias = merge(part3, G, C)
            records[name] = host(part3)
            ratios = [worst_ratio(sums[r], ref[r], mag[r]) for r in (0, 1)]
            print('%s %s relu=%d: worst |sum - fp64| / sum|term|: x %.3g, q %.3g' % (K.class_id(case), name, relu_first, *ratios))
            for r in (0, 1):
                assert (np.abs(sums[r] - ref[r]) <= K.RTOL_SUMS * mag[r]).all(), (name, r, relu_first)
            assert np.array_equal(sums[2], ref[2]), (name, relu_first)
            assert bits_equal(bias, K.bias32(sums))
            again, _ = sums_records(*args, relu_first)
            assert K.same(host(again), records[name])
        assert K.same(records['x/y'], records['fused'])


# ------------------------------------------------------------------------------------------ B: the merge
@pytest.mark.parametrize('C', K.MERGE_C)
@pytest.mark.parametrize('G', K.MERGE_G)
def test_merge_of_hand_built_records(G, C):
    part, named = K.merge_records(G, C, rot=G)
    ref = part.sum(0)                                       # integers: exact in any order
    part3 = dev(part)
    sums, bias = merge(part3, G, C)
    assert K.same(sums, ref), K.where_differ(sums, ref)
    want = K.bias32(ref)
    assert K.same(bias, want), [(ch, named.get(ch), bias[ch], want[ch]) for ch in range(C) if not K.same(bias[ch:ch + 1], want[ch:ch + 1])]
    only_sums, none = merge(part3, G, C, want_bias=False)
    none2, only_bias = merge(part3, G, C, want_sums=False)
    assert none is None and none2 is None and K.same(only_sums, sums) and K.same(only_bias, bias)
    for ch, name in named.items():
        if name == 'equal_sums':
            assert bias[ch] == 0 and not np.signbit(bias[ch])
        if name == 'nan_record':
            assert np.isnan(bias[ch]) and np.isnan(sums[0, ch])
        if name == 'two_roundings':
            assert bias[ch] == 0


def test_merge_refuses_bad_arguments():
    L, _ = mods()
    lib = L.load()
    part3 = dev(np.ones((2, 3, 4)))
    out = torch.zeros(4, dtype=torch.float32, device='cuda')
    assert lib.cnnq_pc_bcorr_bias(part3.data_ptr(), 2, 4, None, None, stream()) == -1
    assert lib.cnnq_pc_bcorr_bias(None, 2, 4, None, out.data_ptr(), stream()) == -1
    assert lib.cnnq_pc_bcorr_bias(part3.data_ptr(), 0, 4, None, out.data_ptr(), stream()) == -1
    assert lib.cnnq_pc_bcorr_bias(part3.data_ptr(), 2, 0, None, out.data_ptr(), stream()) == -1
    assert float(out.abs().sum()) == 0


# ------------------------------------------------------------------------------------------ C: the two output passes
def assert_fine_plan(case, aligned):
    """the short-workgroup geometry of the table-driven passes: the class's load shape, rows of about 14 KB per workgroup"""
    (N, C, H, W), _, want = case
    HW = H * W
    coarse, fine = describe(N, C, HW, aligned, 0), describe(N, C, HW, aligned, 1)
    for k in ('vec', 'A', 'J', 'mode', 'nb', 'w', 'k', 'ncb'):
        assert fine[k] == coarse[k], (k, fine, coarse)
    if aligned == (case[1] == 0):
        assert {k: fine[k] for k in want if k != 'S'} == {k: v for k, v in want.items() if k != 'S'}
    row_bytes = (fine['w'] if fine['mode'] == 1 else fine['k'] * HW // fine['vec']) * fine['vec'] * 4
    rows = max(1, (14336 + row_bytes // 2) // row_bytes)
    assert fine['S'] == -(-N // rows), (fine, rows)
    return fine


@pytest.mark.parametrize('case', SMALL, ids=K.class_id)
def test_apply_in_place_on_hand_built_y(case):
    L, _ = mods()
    shape, off0, _ = case
    N, C, H, W = shape
    y0 = K.hand_y(shape, seed=3 + C)
    for rot in (0, 3, 5):
        bias = K.hand_bias(C, rot)
        want = K.apply32(y0, bias)
        bd = dev(bias)
        for off in sorted({0, 1, off0}):
            assert_fine_plan(case, off == 0)
            yd = dev(y0, off)
            assert L.load().cnnq_pc_bcorr_apply(yd.data_ptr(), N, C, H * W, bd.data_ptr(), stream()) == 0
            got = host(yd)
            assert K.same(got, want), (K.class_id(case), rot, off, K.where_differ(got, want))


@pytest.mark.parametrize('case', SMALL, ids=K.class_id)
def test_fused_quantize_and_correct_given_a_bias(case):
    """cnnq_pc_qdq_bcorr == apply32(pc_qdq(x), bias) bit for bit: both walks, x and y at every 4-byte misalignment"""
    L, ops = mods()
    lib = L.load()
    shape, _, _ = case
    N, C, H, W = shape
    assert_fine_plan(case, True)
    assert_fine_plan(case, False)
    xdy, qpdy = K.dyadic(shape, seed=C + W)
    xg, _, qpg, _, qg = gaussian_case(shape, 11 + C, 0)
    tables = (('dyadic', xdy, dev(qpdy), host(ops.pc_qdq(dev(xdy), N, C, H * W, dev(qpdy)))), ('gaussian', xg, qpg, qg))
    for i, (name, x, qp, q) in enumerate(tables):
        bias = K.hand_bias(C, rot=2 * i + C % 3)
        want = K.apply32(q, bias)
        bd = dev(bias)
        xs = [dev(x, o) for o in range(4)]
        for ox in range(4):
            for oy in range(4):
                for reverse in (0, 1):
                    yd = dev(np.full(shape, GUARD, dtype=F), oy)
                    rc = lib.cnnq_pc_qdq_bcorr(xs[ox].data_ptr(), yd.data_ptr(), N, C, H * W, qp.data_ptr(), bd.data_ptr(), reverse, stream())
                    assert rc == 0, rc
                    got = host(yd)
                    assert K.same(got, want), (K.class_id(case), name, ox, oy, reverse, K.where_differ(got, want))


@pytest.mark.parametrize('case', SMALL, ids=K.class_id)
def test_end_to_end_ops(case):
    """ops.qdq_bias_corrected and ops.act_bias_correction_: the sums in the tier, then bias and y bit for bit"""
    _, ops = mods()
    shape, off, _ = case
    N, C, H, W = shape
    for relu_first in (0, 1):
        x, xd, qp, qd, q = gaussian_case(shape, 23 + C + relu_first, relu_first, off)
        ref, mag = K.sums64(x, q, relu_first)
        y, parts = ops.qdq_bias_corrected(xd, N, C, H * W, qp, bool(relu_first), want_parts=True)
        sums, bias = host(parts['sums']), host(parts['bias'])
        print('%s relu=%d: worst |sum - fp64| / sum|term|: x %.3g, q %.3g' % (K.class_id(case), relu_first,
                                                                              worst_ratio(sums[0], ref[0], mag[0]), worst_ratio(sums[1], ref[1], mag[1])))
        for r in (0, 1):
            assert (np.abs(sums[r] - ref[r]) <= K.RTOL_SUMS * mag[r]).all(), (r, relu_first)
        assert np.array_equal(sums[2], ref[2])
        assert bits_equal(bias, K.bias32(sums))
        want = K.apply32(q, bias)
        assert K.same(host(y), want), K.where_differ(host(y), want)
        # the two-step form returns no parts: its records, merged again, are its bias
        yq = qd.clone() if off == 0 else dev(q, off)
        part3, G = sums_records(xd, yq, None, relu_first)
        sums2, bias2 = merge(part3, G, C)
        out = ops.act_bias_correction_(xd, yq, bool(relu_first))
        assert out is yq
        for r in (0, 1):
            assert (np.abs(sums2[r] - ref[r]) <= K.RTOL_SUMS * mag[r]).all(), (r, relu_first)
        assert np.array_equal(sums2[2], ref[2]) and bits_equal(bias2, K.bias32(sums2))
        want2 = K.apply32(q, bias2)
        assert K.same(host(out), want2), K.where_differ(host(out), want2)


# ------------------------------------------------------------------------------------------ D: the weight correction
def weight_correct(wq, tw, tq, vc, bc):
    L, _ = mods()
    C, HW = wq.shape
    out = dev(wq)
    rc = L.load().cnnq_pc_weight_correct(out.data_ptr(), C, HW, tw.data_ptr(), tq.data_ptr(), int(vc), int(bc), stream())
    assert rc == 0, rc
    return host(out)


@pytest.mark.parametrize('C,HW', K.WEIGHT_CASES)
def test_weight_correction_on_hand_built_tables(C, HW):
    wq, mean_w, std_w, mean_q, std_q = K.weight_case(C, HW, seed=C + HW)
    tw, tq = dev(K.stat_table(C, mean_w, std_w)), dev(K.stat_table(C, mean_q, std_q))
    assert K.same(weight_correct(wq, tw, tq, 0, 0), wq)
    for vc, bc in ((1, 0), (0, 1), (1, 1)):
        want = K.weight32(wq, mean_w, std_w, mean_q, std_q, vc, bc)
        got = weight_correct(wq, tw, tq, vc, bc)
        assert K.same(got, want), (vc, bc, K.where_differ(got, want))


def test_weight_correction_return_codes():
    L, _ = mods()
    lib = L.load()
    wq = dev(np.full((4, 4), 1.5, dtype=F))
    t = dev(K.stat_table(4, np.ones(4), np.ones(4)))
    EINVAL, ERANGE = -1, -2
    assert lib.cnnq_pc_weight_correct(wq.data_ptr(), 65536, 1, t.data_ptr(), t.data_ptr(), 1, 1, stream()) == ERANGE
    assert lib.cnnq_pc_weight_correct(wq.data_ptr(), 4, 4, None, t.data_ptr(), 1, 1, stream()) == EINVAL
    assert lib.cnnq_pc_weight_correct(wq.data_ptr(), 4, 4, t.data_ptr(), None, 1, 1, stream()) == EINVAL
    assert lib.cnnq_pc_weight_correct(None, 4, 4, t.data_ptr(), t.data_ptr(), 1, 1, stream()) == EINVAL
    assert lib.cnnq_pc_weight_correct(wq.data_ptr(), 4, 0, t.data_ptr(), t.data_ptr(), 1, 1, stream()) == EINVAL
    assert bool((wq == 1.5).all())                          # nothing was enqueued


@pytest.mark.parametrize('wshape', [(16, 8, 3, 3), (10, 64), (24, 3, 7, 7), (300, 5, 1, 1)])
def test_weight_correction_end_to_end(wshape):
    """ops.weight_correction: the statistics it derives are in the tier of test_stats_single_gpu.py, and the output is weight32
    of those very tables, bit for bit"""
    L, ops = mods()
    from oracle import quant_oracle as O
    gen = torch.Generator().manual_seed(21)
    w = torch.randn(wshape, generator=gen) * 0.05 + 0.01
    wq = O.weights_per_channel_qdq(w, 4)
    C = wshape[0]
    HW = w.numel() // C
    wd, qd = w.cuda(), wq.cuda()
    tables = []
    for t, td in ((w, wd), (wq, qd)):
        st, _ = ops.pc_stats(td, 1, C, HW, local_only=True)
        st = host(st)
        t64 = t.view(C, -1).double()
        for row, ref in ((L.STAT_MEAN, t64.mean(1).numpy()), (L.STAT_STD, t64.std(1).numpy())):
            with np.errstate(all='ignore'):
                print('%s row %d: worst relative error %.3g' % (wshape, row, float(np.max(np.abs(st[row] - ref) / np.maximum(np.abs(ref), 1e-30)))))
        np.testing.assert_allclose(st[L.STAT_MEAN].astype(np.float64), t64.mean(1).numpy(), rtol=2e-6, atol=1e-7)
        np.testing.assert_allclose(st[L.STAT_STD].astype(np.float64), t64.std(1).numpy(), rtol=2e-6)
        tables.append(st)
    (sw, sq), q2 = tables, wq.view(C, -1).numpy()
    for vc, bc in ((0, 1), (1, 0), (1, 1)):
        out = host(ops.weight_correction(wd, qd, vcorr=bool(vc), bcorr=bool(bc)))
        want = K.weight32(q2, sw[L.STAT_MEAN], sw[L.STAT_STD], sq[L.STAT_MEAN], sq[L.STAT_STD], vc, bc).reshape(wshape)
        assert K.same(out, want), (vc, bc, K.where_differ(out, want))
    assert ops.weight_correction(wd, qd) is qd
