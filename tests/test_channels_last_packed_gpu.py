"""Integer codes as the stored format of dense channels_last activations on the GPU: the packed bytes
against the numpy restatement (tests/_packed_nhwc.py) of the EXISTING code's codes, the round trip against the existing
channels_last Q/DQ, configs 2 and 3 in one call, non-finite values, determinism; no layout copy and no upcast anywhere.

The reference is never the code under test: codes come from ops.pc_qdq(x.contiguous().float(), ..., want_codes=True) (the fp32
NCHW kernel), floats from ops.pc_qdq on the channels_last tensor (k_cl_qdq)."""
import importlib

import numpy as np
import pytest
import torch

import _packed_nhwc as PK
from test_channels_last_gpu import DTYPES, IDS, cl, is_cl, same, values

pytestmark = pytest.mark.gpu
F32, BF16, F16 = DTYPES

# (4,64,14,14): several workgroups; (2,20,7,7): 80-bit rows at 4 bits, padding; (3,6,5,9): W = 2; (2,5,5,9): odd C, W = 1;
# (1,8,1,3): R = 3 rows, fewer than a step; (2,300,4,4); (2,1028,3,3) fp32 and (2,2056,3,3) bf16: two column blocks that share a dword
GRID = [(s, d) for s in [(4, 64, 14, 14), (2, 20, 7, 7), (3, 6, 5, 9), (2, 5, 5, 9), (1, 8, 1, 3), (2, 300, 4, 4)] for d in DTYPES]
GRID += [((2, 1028, 3, 3), F32), ((2, 2056, 3, 3), BF16)]
GRID_IDS = ['%s-%s' % ('x'.join(map(str, s)), IDS[DTYPES.index(d)]) for s, d in GRID]
TABLES = ['all4', 'all8', 'all0', 'ramp', 'ramp4']


def mods():
    from cnn_quantization_amd import _lib as L, ops
    return L, ops


def iq_mod():
    return importlib.import_module('cnn_quantization_amd.qtypes.int_quantizer')


@pytest.fixture(autouse=True)
def no_copy_no_upcast():
    """No call of this file transposes a channels_last tensor or upcasts a half-precision one."""
    _, ops = mods()
    copies, ups = ops.LAYOUT_COPIES, iq_mod().HALF_FALLBACKS
    yield
    assert ops.LAYOUT_COPIES == copies and iq_mod().HALF_FALLBACKS == ups


def widths(name, C):
    ar = np.arange(C)
    return {'all4': np.full(C, 4), 'all8': np.full(C, 8), 'all0': np.zeros(C, dtype=np.int64), 'ramp': ar % 9, 'ramp4': (ar + 4) % 9}[name]


def rows(t):
    """an NCHW-shaped tensor -> numpy [R, C] in the row order of the channels_last storage"""
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1]).cpu().numpy()


def ref_codes(x, qp):
    """The existing fp32 NCHW kernel's codes of x, [R, C]."""
    _, ops = mods()
    N, C, H, W = x.shape
    _, codes = ops.pc_qdq(x.contiguous().float(), N, C, H * W, qp, want_codes=True)
    return rows(codes).astype(np.int64)


def ref_floats(x, qp):
    """The existing channels_last Q/DQ (k_cl_qdq) on the tensor itself."""
    _, ops = mods()
    N, C, H, W = x.shape
    y = ops.pc_qdq(x, N, C, H * W, qp)
    assert is_cl(y) and y.dtype == x.dtype
    return y


_CASES = {}


def case(shape, dtype, offset, table):
    """x, its table and the reference's codes and floats: computed once, shared by the tests, never written again."""
    key = (shape, dtype, offset, table)
    if key not in _CASES:
        L, ops = mods()
        C = shape[1]
        x = cl(values(shape, seed=sum(shape)), dtype, offset)
        bkey = (shape, dtype, offset, 'qp')
        if bkey not in _CASES:
            _, parts = ops.act_qdq_per_channel(x.contiguous().float(), 4, want_parts=True)
            _CASES[bkey] = parts['qp']
        bits = widths(table, C)
        qp = _CASES[bkey].clone()
        qp[L.QP_QMAX] = torch.from_numpy(2.0 ** bits - 1.0).float().cuda()
        _CASES[key] = dict(x=x, qp=qp, bits=bits, codes=ref_codes(x, qp), y=ref_floats(x, qp))
    return _CASES[key]


def pack_into_canary(x, qp, bits, **kw):
    """quantize_packed_nhwc into a 0xFF buffer 64 bytes longer than the capacity -> (the whole buffer as bytes, coloff, buffer)."""
    _, ops = mods()
    buf = torch.full((ops.packed_capacity_nhwc(x.shape) + 64,), 0xFF, dtype=torch.uint8, device='cuda')
    out, coloff = ops.quantize_packed_nhwc(x, qp, bits, out=buf, **kw)
    assert out is buf
    return buf.cpu().numpy().tobytes(), coloff, buf


def check_bytes(raw, coloff, bits, codes):
    R, C = codes.shape
    assert coloff.dtype == torch.int32 and coloff.cpu().tolist() == PK.coloff(bits).tolist()
    want = PK.pack(codes, bits)
    used = R * PK.rowbytes(bits)
    assert len(want) == used
    assert raw[:used] == want, 'packed bytes differ from the restatement (first at %d of %d)' % (
        next(i for i in range(used) if raw[i] != want[i]), used)
    assert raw[used:] == b'\xff' * (len(raw) - used), 'a byte beyond R * rowbytes was written'


def bits_args(table, bits):
    """The forms a width table is handed over in: the device table, and for a uniform one also the integer."""
    forms = [torch.from_numpy(bits.astype(np.float32)).cuda()]
    if table.startswith('all'):
        forms.append(int(bits[0]))
    return forms


@pytest.mark.parametrize('shape,dtype', GRID, ids=GRID_IDS)
def test_bytes_equal_the_restatement(shape, dtype):
    for offset in (0, 1):
        for table in TABLES:
            c = case(shape, dtype, offset, table)
            for arg in bits_args(table, c['bits']):
                raw, coloff, _ = pack_into_canary(c['x'], c['qp'], arg)
                check_bytes(raw, coloff, c['bits'], c['codes'])


@pytest.mark.parametrize('shape,dtype', GRID, ids=GRID_IDS)
def test_round_trip_equals_the_channels_last_qdq(shape, dtype):
    _, ops = mods()
    for offset in (0, 1):
        for table in TABLES:
            c = case(shape, dtype, offset, table)
            for arg in bits_args(table, c['bits']):
                packed, coloff = ops.quantize_packed_nhwc(c['x'], c['qp'], arg)
                if isinstance(arg, int):
                    assert packed.numel() == c['codes'].shape[0] * PK.rowbytes(c['bits'])          # sized exactly on the host
                else:
                    assert packed.numel() == ops.packed_capacity_nhwc(shape)
                y = ops.dequantize_packed_nhwc(packed, shape, dtype, c['qp'], coloff)
                assert y.dtype == dtype and tuple(y.shape) == shape and y.is_contiguous(memory_format=torch.channels_last)
                assert is_cl(y)
                assert torch.equal(y, c['y']) and same(y, c['y']), (shape, dtype, offset, table)
    # into the caller's tensor, at the odd element offset
    c = case(shape, dtype, 0, 'ramp')
    packed, coloff = ops.quantize_packed_nhwc(c['x'], c['qp'], bits_args('ramp', c['bits'])[0])
    out = cl(torch.zeros(shape), dtype, 1)
    assert ops.dequantize_packed_nhwc(packed, shape, dtype, c['qp'], coloff, out=out) is out
    assert same(out, c['y'])


def edge_tensor(dtype):
    """[2, 8, 4, 8]: per channel the rounding ties of the code ((k + 0.5) * scale) and values a few ulps around them, zeros,
    denormals; channel 7 holds |x| = 2^80 and channel 6 one 3e38, outside qdq_fast_domain (fp16: inf, outside as well)."""
    L, _ = mods()
    C = 8
    sc = torch.tensor([0.25, 0.1, 0.3, 1.0, 0.0123, 2.0, 0.7, 0.5])
    zp = torch.tensor([0., 3., 7., 8., 15., 0., 5., 6.])
    qp = torch.zeros(L.NQP, C)
    qp[L.QP_SCALE], qp[L.QP_ZP], qp[L.QP_QMAX] = sc, zp, 15.
    k = torch.arange(64, dtype=torch.float32).reshape(2, 1, 4, 8)
    tie = ((k % 16) + 0.5 - zp.reshape(1, C, 1, 1)) * sc.reshape(1, C, 1, 1)
    x = tie.clone()
    for n, ulps in ((1, 1), (2, -1), (3, 3)):                         # a few ulps of fp32 around the tie
        sel = (k.expand_as(x) // 16) == n
        moved = (tie.view(torch.int32) + ulps).view(torch.float32)
        x = torch.where(sel, moved, x)
    x[0, :, 0, 0] = 0.
    x[0, :, 0, 1] = -0.
    x[0, :, 0, 2] = 1e-40                                             # an fp32 denormal
    x[0, :, 0, 3] = -1e-42
    x[0, 7, 1, 0] = 2.0 ** 80
    x[1, 7, 2, 3] = -(2.0 ** 80)
    x[1, 6, 0, 0] = 3e38                                              # x / scale overflows: the divide-free quotient would be NaN
    xd = cl(x, dtype)
    xf = xd.contiguous().float()
    mm = torch.stack([xf.amin(dim=(0, 2, 3)), xf.amax(dim=(0, 2, 3))]).contiguous()
    return xd, qp.cuda(), mm


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_extrema_do_not_change_the_bytes(dtype):
    x, qp, mm = edge_tensor(dtype)
    bits = np.full(8, 4)
    codes = ref_codes(x, qp)
    for arg in (4, torch.full((8,), 4.).cuda()):
        plain, coloff, _ = pack_into_canary(x, qp, arg)
        fast, _, _ = pack_into_canary(x, qp, arg, mm=mm)
        assert plain == fast
        check_bytes(fast, coloff, bits, codes)
    assert not (mm.abs() <= 2.0 ** 70).all()                          # one channel is outside the divide-free domain


@pytest.mark.parametrize('shape,dtype', [((2, 20, 7, 7), F32), ((3, 6, 5, 9), BF16), ((2, 1028, 3, 3), F32), ((2, 2056, 3, 3), BF16)],
                         ids=['f32', 'bf16-w2', 'f32-blocks', 'bf16-blocks'])
def test_a_code_wider_than_its_channel_never_touches_a_neighbour(shape, dtype):
    """qmax[c] > 2^bits[c] - 1 is the caller's error: that channel's codes lose their high bits, every other bit of the row is
    what it would be without them."""
    L, ops = mods()
    for offset in (0, 1):
        for table in ('ramp', 'ramp4', 'all0'):
            c = case(shape, dtype, offset, table)
            qp = c['qp'].clone()
            qp[L.QP_QMAX] = 255.
            wide = ref_codes(c['x'], qp)
            assert (wide > 2 ** c['bits'] - 1).any()
            raw, coloff, _ = pack_into_canary(c['x'], qp, bits_args(table, c['bits'])[0])
            check_bytes(raw, coloff, c['bits'], wide & (2 ** c['bits'] - 1))


@pytest.mark.parametrize('shape', [(4, 64, 14, 14), (2, 20, 7, 7)], ids=['4x64x14x14', '2x20x7x7'])
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_config2_in_one_call(shape, dtype):
    L, ops = mods()
    N, C, H, W = shape
    for positive in (False, True):
        x = cl(values(shape, seed=3, positive=positive), dtype)
        for nb in (4, 8):
            _, parts = ops.act_qdq_per_channel(x.contiguous().float(), nb, positive=positive, want_parts=True)
            buf = torch.full((N * H * W * PK.rowbytes([nb] * C) + 64,), 0xFF, dtype=torch.uint8, device='cuda')
            packed, got = ops.minmax_quantize_packed_nhwc(x, nb, positive=positive, out=buf)
            assert packed is buf and sorted(got) == ['coloff', 'mm', 'qp']
            assert same(got['qp'], parts['qp'])
            assert same(got['mm'], torch.stack([parts['stats'][L.STAT_MIN], parts['stats'][L.STAT_MAX]]))
            check_bytes(buf.cpu().numpy().tobytes(), got['coloff'], np.full(C, nb), ref_codes(x, parts['qp']))
            exact, got2 = ops.minmax_quantize_packed_nhwc(x, nb, positive=positive)
            assert exact.numel() == N * H * W * PK.rowbytes([nb] * C) and torch.equal(exact, buf[:exact.numel()])
            y = ops.dequantize_packed_nhwc(exact, shape, dtype, got2['qp'], got2['coloff'])
            assert is_cl(y) and same(y, ops.act_qdq_per_channel(x, nb, positive=positive))


@pytest.mark.parametrize('shape', [(8, 64, 28, 28), (2, 64, 7, 7)], ids=['8x64x28x28', '2x64x7x7'])     # the two summation regimes
@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_config3_in_one_call(shape, dtype):
    L, ops = mods()
    N, C, H, W = shape
    R = N * H * W
    x = cl(values(shape, seed=11), dtype)
    y_ref, parts = ops.aciq_qdq_nhwc(x, 4, bit_alloc=True, want_parts=True)
    x2 = cl(values(shape, seed=11), dtype)                             # a fresh allocation, as x: the same piece width
    packed, got = ops.aciq_quantize_packed_nhwc(x2, 4, bit_alloc=True)
    assert sorted(got) == ['coloff', 'diag', 'qp', 'stats']
    for k in ('stats', 'qp', 'diag'):
        assert same(got[k], parts[k]), k
    assert packed.numel() == ops.packed_capacity_nhwc(shape)
    bits = got['diag'][L.DIAG_BITS].cpu().numpy().astype(np.int64)
    assert coloff_list(got['coloff']) == PK.coloff(bits).tolist()
    used = R * PK.rowbytes(bits)
    assert packed.cpu().numpy().tobytes()[:used] == PK.pack(ref_codes(x, parts['qp']), bits)
    assert used / (R * C) <= bits.mean() / 8 + 4 / C
    y = ops.dequantize_packed_nhwc(packed, shape, dtype, got['qp'], got['coloff'])
    assert is_cl(y) and same(y, y_ref)
    # without bit allocation: the uniform width, the buffer exact
    y_ref, parts = ops.aciq_qdq_nhwc(x, 4, want_parts=True)
    packed, got = ops.aciq_quantize_packed_nhwc(x2, 4)
    assert packed.numel() == R * PK.rowbytes([4] * C) and same(got['qp'], parts['qp'])
    assert packed.cpu().numpy().tobytes() == PK.pack(ref_codes(x, parts['qp']), np.full(C, 4))
    assert same(ops.dequantize_packed_nhwc(packed, shape, dtype, got['qp'], got['coloff']), y_ref)


def coloff_list(t):
    return t.cpu().tolist()


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS)
def test_non_finite_values(dtype):
    L, ops = mods()
    shape = (2, 8, 3, 3)
    C = 8
    clean = values(shape, seed=5)
    _, parts = ops.act_qdq_per_channel(cl(clean, dtype).contiguous().float(), 4, want_parts=True)
    qp = parts['qp']
    bits = np.full(C, 4)
    spots = {(0, 1, 0, 0): float('nan'), (1, 3, 1, 1): float('inf'), (0, 5, 2, 2): float('-inf')}
    dirty = clean.clone()
    for at, v in spots.items():
        dirty[at] = v
    xc, xd = cl(clean, dtype), cl(dirty, dtype)
    want = ref_codes(xc, qp).reshape(2, 3, 3, C)
    zp, sc, qm = (qp[r].cpu() for r in (L.QP_ZP, L.QP_SCALE, L.QP_QMAX))
    y_want = ref_floats(xc, qp).clone()
    for (n, c, h, w), v in spots.items():
        code = qm[c] if v == float('inf') else torch.tensor(0.)       # NaN -> code 0, +Inf -> qmax, -Inf -> 0
        want[n, h, w, c] = int(code)
        y_want[n, c, h, w] = ((code - zp[c]) * sc[c]).to(dtype)
    raw, coloff, buf = pack_into_canary(xd, qp, 4)
    check_bytes(raw, coloff, bits, want.reshape(-1, C))
    y = ops.dequantize_packed_nhwc(buf, shape, dtype, qp, coloff)
    assert not torch.isnan(y).any() and same(y, y_want)
    # a channel whose zero point is NaN decodes to NaN everywhere and disturbs no neighbour
    qn = qp.clone()
    qn[L.QP_ZP, 2] = float('nan')
    raw_n, coloff, buf = pack_into_canary(xc, qn, 4)
    got = PK.unpack(raw_n[:18 * PK.rowbytes(bits)], bits, 18, C)
    keep = [c for c in range(C) if c != 2]
    assert (got[:, keep] == ref_codes(xc, qp)[:, keep]).all()
    assert raw_n[18 * PK.rowbytes(bits):] == b'\xff' * (len(raw_n) - 18 * PK.rowbytes(bits))
    y = ops.dequantize_packed_nhwc(buf, shape, dtype, qn, coloff)
    assert torch.isnan(y[:, 2]).all() and not torch.isnan(y[:, keep]).any()
    assert same(y[:, keep], ref_floats(xc, qp)[:, keep])


@pytest.mark.parametrize('shape,dtype', [((4, 64, 14, 14), BF16), ((2, 1028, 3, 3), F32), ((2, 5, 5, 9), F16)], ids=['bf16', 'f32-blocks', 'f16-odd'])
def test_two_runs_write_the_same_bytes(shape, dtype):
    c = case(shape, dtype, 0, 'ramp')
    arg = bits_args('ramp', c['bits'])[0]
    a, _, _ = pack_into_canary(c['x'], c['qp'], arg)
    b, _, _ = pack_into_canary(c['x'], c['qp'], arg)
    assert a == b


def test_refusals_make_no_copy():
    L, ops = mods()
    c = case((2, 20, 7, 7), F32, 0, 'all4')
    x = c['x']
    for bad in (x.contiguous(), x[:, ::2], x.double(), x.cpu()):
        with pytest.raises(L.CnnqError):
            ops.quantize_packed_nhwc(bad, c['qp'], 4)
        with pytest.raises(L.CnnqError):
            ops.minmax_quantize_packed_nhwc(bad, 4)
        with pytest.raises(L.CnnqError):
            ops.aciq_quantize_packed_nhwc(bad, 4, bit_alloc=True)
    with pytest.raises(L.CnnqError):
        ops.quantize_packed_nhwc(x, c['qp'][:, :10].contiguous(), 4)
    with pytest.raises(L.CnnqError):
        ops.quantize_packed_nhwc(x, c['qp'], 4, out=torch.empty(8, dtype=torch.uint8, device='cuda'))
