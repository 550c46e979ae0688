"""Config 2's scale and zero point on hand-built extrema at every site that writes the arithmetic out:
k_minmax_params on uploaded records, the gathered prologue of k_qdq, and every tensor route - the three-launch chain, k_mmq_group
/ k_mmq_flat, the resident kernel, the single launch, the bf16 / fp16 kernels, the channels_last front and the two packed fronts -
on tensors whose per-channel extrema are the table of tests/_minmax_params.py.

Every comparison is M.same_bits against M.params_ref / M.qdq_ref: NaN in the same places, every other word bit for bit.  There is
no tolerance in this file.  test_minmax_params_cpu.py pins the restatement to the oracle and proves the table has teeth."""
import ctypes

import numpy as np
import pytest
import torch

import _minmax_params as M
import _packed_nhwc as PK

pytestmark = pytest.mark.gpu
F32 = np.float32
SENT, PAD = 77.0625, 64             # (no parameter or extremum of the table equals the sentinel)


def mods():
    from cnn_quantization_amd import _lib as L, ops
    return L, ops


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().float().cpu().numpy()


def check(got, want, where):
    assert M.same_bits(got, want), (where, M.first_diff(got, want))


class Placed:
    """a float32 output of `shape` as a view inside a sentinel-filled buffer: PAD guard words in front and behind"""

    def __init__(self, shape):
        self.shape, self.n = shape, int(np.prod(shape))
        self.buf = torch.full((self.n + 2 * PAD,), SENT, dtype=torch.float32, device='cuda')

    def ptr(self):
        return self.buf[PAD:].data_ptr()

    def take(self, what):
        b = self.buf.cpu().numpy()
        assert (b[:PAD] == SENT).all() and (b[PAD + self.n:] == SENT).all(), 'guard words around %s' % what
        return b[PAD:PAD + self.n].reshape(self.shape).copy()


# ------------------------------------------------------------------------------------------ (a) the parameter kernel on records
ZEROS = [('neg_zero_min', F32(-0.0), F32(1.0)), ('pos_zero_min', F32(0.0), F32(1.0)), ('neg_zero_max', F32(-1.0), F32(-0.0)),
         ('pos_zero_max', F32(-1.0), F32(0.0))]
GRID_G, GRID_C = [1, 3, 64, 65, 300], [1, 3, 4, 5, 257]


def inner(a, b):
    """two values strictly inside (a, b), a quarter of the way in from either end; the value itself for a constant channel"""
    lo, hi = (a if np.isfinite(a) else F32(-1000)), (b if np.isfinite(b) else F32(1000))
    if lo == hi:
        return lo, hi
    inlo, inhi = (F32(np.float64(lo) + f * (np.float64(hi) - np.float64(lo))) for f in (0.25, 0.75))
    assert lo < inlo <= inhi < hi, (a, b)
    return inlo, inhi


def records(G, C, rot):
    """pmm [G][2][C] whose channel c merges to row (c + rot) of the named channels: the true minimum in one group, the true maximum
    in another (G > 1), both rotating with c; every other group holds values strictly inside the range - or the same value, for a
    constant channel.  A NaN channel holds its NaN in one group only - first, middle or last - as a workgroup that saw one reports it:
    in both rows.  -> (pmm, mn [C], mx [C])"""
    rows = M.all_named() + ZEROS
    pmm = np.empty((G, 2, C), dtype=F32)
    mn, mx = np.empty(C, dtype=F32), np.empty(C, dtype=F32)
    for c in range(C):
        _, a, b = rows[(c + rot) % len(rows)]
        mn[c], mx[c] = a, b
        ga = (c + rot) % G
        gb = (ga + 1 + c % max(G - 1, 1)) % G
        if a != a:
            pmm[:, 0, c], pmm[:, 1, c] = -0.5, 0.5
            pmm[(0, G // 2, G - 1)[c % 3], :, c] = np.nan
            continue
        pmm[:, 0, c], pmm[:, 1, c] = inner(a, b)
        pmm[ga, 0, c] = a
        pmm[gb, 1, c] = b
    return pmm, mn, mx


@pytest.mark.parametrize('C', GRID_C)
@pytest.mark.parametrize('G', GRID_G)
def test_parameter_kernel_on_hand_built_records(G, C):
    L, _ = mods()
    lib = L.load()
    for rot in (0, 11, 23, 37):
        pmm, mn, mx = records(G, C, rot + G)
        pmm_d = dev(pmm)
        out = Placed((2, C))
        assert lib.cnnq_pc_minmax_reduce(pmm_d.data_ptr(), G, C, out.ptr(), stream()) == 0
        red = out.take('the reduced extrema')
        check(red[0], mn, (G, C, rot, 'min'))
        check(red[1], mx, (G, C, rot, 'max'))
        for bits in (2, 4, 8, 16, 32):
            for positive in (0, 1):
                qp = Placed((L.NQP, C))
                assert lib.cnnq_pc_minmax_params(pmm_d.data_ptr(), G, C, bits, positive, qp.ptr(), stream()) == 0
                got = qp.take('qp')
                sc, zp, qm = M.params_ref(mn, mx, bits, bool(positive))
                where = (G, C, rot, bits, positive)
                check(got[L.QP_SCALE], sc, where + ('scale',))
                check(got[L.QP_ZP], zp, where + ('zp',))
                assert (got[L.QP_QMAX] == qm).all() and (bits != 32 or qm == 2.0 ** 32), where


# ------------------------------------------------------------------------------------------ the tensors of (b) and (c)
# the smallest shapes of test_group_gpu.SHAPES that reach each tiling -> (mode, A) cnnq_pc_group_describe must report: straddling
# float4s; whole channels; whole channels in column blocks and two batch splits; flat tiles; row pieces of one channel (8 MB); short
# rows, many channels, twice
SHAPES = {(3, 8, 7, 7): (2, 4), (2, 8, 14, 14): (2, 1), (5, 3, 28, 28): (2, 1), (9, 4, 56, 56): (3, 1), (1030, 1, 32, 64): (1, 1),
          (4, 260, 1, 4): (2, 1), (1, 1100, 2, 2): (2, 1)}
_CASES = {}


def table_windows(shape, mode, which, dtype=torch.float32):
    """the windows of a table over a shape's channels.  which: 'fast' - the fast table alone; 'mixed' - both, interleaved (a
    one-channel shape does not repeat the fast ones)"""
    fast, _ = M.split(mode, dtype)
    rows = fast if which == 'fast' else M.mixed(mode, dtype)
    return M.windows(rows, shape[1], {r[0] for r in fast} if which == 'mixed' else ())


def cases(shape, mode, which, dtype=torch.float32):
    """[(names, x on the CPU, mn, mx, (scale, zp, qmax), y, codes)] for the windows of a table over a shape: built once, never
    changed (the 8 MB shape, which one test reads, is not kept)."""
    key = (shape, mode, which, dtype)
    if key not in _CASES:
        out = []
        for k, win in enumerate(table_windows(shape, mode, which, dtype)):
            x, mn, mx = M.window_tensor(shape, win, 1000 * mode[0] + 31 * k + shape[1] + int(mode[1]), dtype)
            p = M.params_ref(mn, mx, *mode)
            y, q = M.qdq_ref(x.float().numpy(), *p)
            if dtype != torch.float32:
                y = torch.from_numpy(y).to(dtype).float().numpy()
            out.append(([w[0] for w in win], x, mn, mx, p, y, q))
        if x.numel() > 1 << 18:
            return out
        _CASES[key] = out
    return _CASES[key]


def describe(shape):
    L, _ = mods()
    out = (ctypes.c_int32 * 8)()
    rc = L.load().cnnq_pc_group_describe(shape[0], shape[1], shape[2] * shape[3], out)
    return rc, dict(zip(('A', 'K', 'mode', 'S', 'ncb', 'Gs', 'groups', 'wgs'), list(out)))


def test_shapes_cover_every_tiling_and_every_named_channel_passes_each():
    """a planner change must not silently un-test a mode, and the windows must carry every name through every mode"""
    seen = {}
    for shape, want in SHAPES.items():
        rc, d = describe(shape)
        assert rc == 0 and (d['mode'], d['A']) == want, (shape, d)
        assert shape[0] * shape[1] * shape[2] * shape[3] * 4 <= 1030 * 32 * 64 * 4
        for mode in M.MODES:
            for which in ('fast', 'mixed'):
                for win in table_windows(shape, mode, which):
                    seen.setdefault((d['mode'], mode), set()).update(w[0] for w in win)
    assert {k[0] for k in seen} == {1, 2, 3} and {v[1] for v in SHAPES.values()} == {1, 4}
    for (gm, mode), names in seen.items():
        assert names == {r[0] for r in M.table(mode)}, (gm, mode)


def check_parts(parts, mn, mx, p, where):
    L, _ = mods()
    qp, stats = host(parts['qp']), host(parts['stats'])
    check(qp[L.QP_SCALE], p[0], where + ('scale',))
    check(qp[L.QP_ZP], p[1], where + ('zp',))
    assert (qp[L.QP_QMAX] == p[2]).all(), where
    check(stats[L.STAT_MIN], mn, where + ('min',))
    check(stats[L.STAT_MAX], mx, where + ('max',))


def check_codes(codes, q, where):
    """integer codes against the restatement's wherever it has one (a NaN has no code)"""
    has = ~np.isnan(q)
    assert np.array_equal(np.asarray(codes)[has].astype(np.int64), q[has].astype(np.int64)), where


# ------------------------------------------------------------------------------------------ (b) the gathered form
@pytest.mark.parametrize('W', [1, 2, 8])
@pytest.mark.parametrize('shape', [(3, 8, 7, 7), (2, 8, 14, 14), (4, 260, 1, 4)], ids=str)
def test_gathered_records(shape, W):
    L, ops = mods()
    lib = L.load()
    N, C, HW = shape[0], shape[1], shape[2] * shape[3]
    for mode in M.MODES:
        for names, x, mn, mx, p, y_ref, _ in cases(shape, mode, 'mixed'):
            rec = np.empty((W, 2, C), dtype=F32)
            for c in range(C):                       # the tensor's own extrema in one rank's record each, the others inside
                a, b = mn[c], mx[c]
                if a != a:
                    rec[:, 0, c], rec[:, 1, c] = -0.5, 0.5
                    rec[(0, W // 2, W - 1)[c % 3], :, c] = np.nan
                    continue
                rec[:, 0, c], rec[:, 1, c] = inner(a, b)
                rec[c % W, 0, c] = a
                rec[(c + 1 + c // W) % W, 1, c] = b
            xd, rec_d = x.cuda(), dev(rec)
            y = torch.empty_like(xd)
            qp = Placed((L.NQP, C))
            L.check(lib.cnnq_pc_gathered_qdq(xd.data_ptr(), y.data_ptr(), N, C, HW, rec_d.data_ptr(), W, mode[0], int(mode[1]), qp.ptr(),
                                             stream()), 'cnnq_pc_gathered_qdq')
            where = (shape, W, mode, names[:8])
            got = qp.take('qp')
            check(got[L.QP_SCALE], p[0], where + ('scale',))
            check(got[L.QP_ZP], p[1], where + ('zp',))
            assert (got[L.QP_QMAX] == p[2]).all(), where
            check(host(y), y_ref, where + ('y',))


# ------------------------------------------------------------------------------------------ (c) every tensor route
RAN = {}


def ran(route, shape):
    RAN.setdefault(route, set()).add(shape)


def run_f32_routes(shape, mode, which):
    L, ops = mods()
    bits, positive = mode
    N, C, HW = shape[0], shape[1], shape[2] * shape[3]
    byte_codes = bits <= 8
    for names, x, mn, mx, p, y_ref, q_ref in cases(shape, mode, which):
        where = (shape, mode, which, names[:8])
        xd = x.cuda()
        # the three-launch chain: k_minmax -> k_minmax_params -> k_qdq
        res = ops.minmax_qdq_fused(xd, N, C, HW, bits, positive, want_codes=byte_codes, want_parts=True, chain=True)
        check(host(res[0]), y_ref, where + ('chain y',))
        check_parts(res[-1], mn, mx, p, where + ('chain',))
        if byte_codes:
            check_codes(res[1].cpu().numpy(), q_ref, where + ('chain codes',))
        ran('chain', shape)
        # k_mmq_group / k_mmq_flat: the exchange, the forced recompute, the IEEE divide
        by_flag = {}
        for flags in (0, 1, 2):
            y, parts = ops.minmax_qdq_group(xd, N, C, HW, bits, positive, want_parts=True, flags=flags)
            by_flag[flags] = host(y)
            check(by_flag[flags], y_ref, where + ('group y', flags))
            check_parts(parts, mn, mx, p, where + ('group', flags))
        if which == 'fast':                          # the whole observable content of the fast-domain decision
            assert by_flag[0].tobytes() == by_flag[2].tobytes() == by_flag[1].tobytes(), where
        ran('group', shape)
        res = ops.minmax_qdq_resident(xd, N, C, HW, bits, positive, want_parts=True)
        if res is not None:
            check(host(res[0]), y_ref, where + ('resident y',))
            check_parts(res[1], mn, mx, p, where + ('resident',))
            ran('resident', shape)
        res = ops.minmax_qdq_single(xd, N, C, HW, bits, positive, want_codes=byte_codes, want_parts=True)
        if res is not None:
            check(host(res[0]), y_ref, where + ('single y',))
            check_parts(res[-1], mn, mx, p, where + ('single',))
            if byte_codes:
                check_codes(res[1].cpu().numpy(), q_ref, where + ('single codes',))
            ran('single', shape)
        # the channels_last front on the same values: [R][C] rows
        y, qp, mm = nhwc(xd.permute(0, 2, 3, 1).contiguous(), N * HW, C, bits, positive)
        check(host(y.view(N, shape[2], shape[3], C).permute(0, 3, 1, 2)), y_ref, where + ('nhwc y',))
        check_parts(dict(qp=qp, stats=mm), mn, mx, p, where + ('nhwc',))
        ran('nhwc f32', shape)
    ops.group_status(xd, clear=True)                 # (the forced recompute reports itself in the sticky word)


def nhwc(rows, R, C, bits, positive):
    """cnnq_pc_minmax_qdq_nhwc on buffers of the test's own: (y [R][C], qp, mm as the two first rows of a stats table)"""
    L, ops = mods()
    lib = L.load()
    dt = ops._DTYPE_CODES[rows.dtype]
    ws = torch.empty(max(lib.cnnq_pc_nhwc_workspace(R, C, dt) // 4, 1), dtype=torch.float32, device='cuda')
    qp = torch.empty((L.NQP, C), dtype=torch.float32, device='cuda')
    mm = torch.empty((2, C), dtype=torch.float32, device='cuda')
    y = torch.empty_like(rows)
    L.check(lib.cnnq_pc_minmax_qdq_nhwc(rows.data_ptr(), y.data_ptr(), dt, R, C, bits, int(positive), ws.data_ptr(), qp.data_ptr(),
                                        mm.data_ptr(), stream()), 'cnnq_pc_minmax_qdq_nhwc')
    return y, qp, mm


@pytest.mark.parametrize('which', ['fast', 'mixed'])
@pytest.mark.parametrize('mode', M.MODES, ids=str)
@pytest.mark.parametrize('shape', list(SHAPES), ids=str)
def test_fp32_routes(shape, mode, which):
    run_f32_routes(shape, mode, which)
    assert {'chain', 'group', 'nhwc f32'} <= {r for r, s in RAN.items() if shape in s}


def test_the_optional_single_launches_ran_somewhere():
    """minmax_qdq_resident and minmax_qdq_single answer None where the shape has no such kernel: not everywhere"""
    for shape in ((2, 8, 14, 14), (3, 8, 7, 7)):
        run_f32_routes(shape, (4, False), 'fast')
    assert RAN.get('resident') and RAN.get('single'), RAN


def auto_dt(x, bits, positive):
    """cnnq_pc_minmax_qdq_auto_dt on a workspace of the test's own: (y, qp, mm)"""
    L, ops = mods()
    lib = L.load()
    N, C, HW = ops.geometry(x)
    ws = torch.empty(lib.cnnq_pc_minmax_qdq_workspace(N, C, HW) // 4, dtype=torch.float32, device='cuda')
    y = torch.empty_like(x)
    L.check(lib.cnnq_pc_minmax_qdq_auto_dt(x.data_ptr(), y.data_ptr(), ops._DTYPE_CODES[x.dtype], N, C, HW, bits, int(positive),
                                           ws.data_ptr(), None, 0, 1, stream()), 'cnnq_pc_minmax_qdq_auto_dt')
    return y, ws[:L.NQP * C].view(L.NQP, C), ws[L.NQP * C:(L.NQP + 2) * C].view(2, C)


def half_codes(packed, rowoff, shape):
    """the 4-bit codes [N, C, HW] of the contiguous packed format: row (n, c) a little-endian nibble stream at n * rowoff[C] + rowoff[c]"""
    N, C, HW = shape[0], shape[1], shape[2] * shape[3]
    ro = rowoff.cpu().numpy().astype(np.int64)
    raw = packed.cpu().numpy()
    out = np.empty((N, C, HW), dtype=np.int64)
    for n in range(N):
        for c in range(C):
            b = raw[n * ro[C] + ro[c]: n * ro[C] + ro[c] + (HW + 1) // 2].astype(np.int64)
            out[n, c] = np.stack([b & 15, b >> 4], axis=1).reshape(-1)[:HW]
    return out


@pytest.mark.parametrize('which', ['fast', 'mixed'])
@pytest.mark.parametrize('dtype', ['bf16', 'f16'])
@pytest.mark.parametrize('mode', M.MODES, ids=str)
@pytest.mark.parametrize('shape', list(SHAPES), ids=str)
def test_half_and_channels_last_routes(shape, mode, dtype, which):
    """h_params (k_h_whole and k_h_qdq) and the channels_last front on the bf16 / fp16 sub-tables; at 4 bits also the two packed
    fronts, whose decoded codes are the restatement's"""
    L, ops = mods()
    dt = M.DTYPES[dtype]
    bits, positive = mode
    N, C, H, W = shape
    HW = H * W
    for names, x, mn, mx, p, y_ref, q_ref in cases(shape, mode, which, dt):
        where = (shape, mode, dtype, which, names[:8])
        xd = x.cuda()
        y, qp, mm = auto_dt(xd, bits, positive)
        check(host(y), y_ref, where + ('auto_dt y',))
        check_parts(dict(qp=qp, stats=mm), mn, mx, p, where + ('auto_dt',))
        rows = xd.permute(0, 2, 3, 1).contiguous()
        y, qp, mm = nhwc(rows, N * HW, C, bits, positive)
        check(host(y.view(N, H, W, C).permute(0, 3, 1, 2)), y_ref, where + ('nhwc y',))
        check_parts(dict(qp=qp, stats=mm), mn, mx, p, where + ('nhwc',))
        if bits != 4:
            continue
        packed, rowoff, qp = ops.minmax_quantize_packed_half(xd, 4, positive)
        check(host(qp)[:2], np.stack([p[0], p[1]]), where + ('packed half qp',))
        check_codes(half_codes(packed, rowoff, shape).reshape(shape), q_ref, where + ('packed half codes',))
        check(host(ops.dequantize_packed_half(packed, shape, dt, qp, 4, rowoff)), y_ref, where + ('packed half y',))
        xcl = xd.contiguous(memory_format=torch.channels_last)
        if ops._layout(xcl) != 'nhwc':               # C == 1 or H * W == 1: dense in both layouts, the wrapper takes the other one
            continue
        packed, got = ops.minmax_quantize_packed_nhwc(xcl, 4, positive)
        check_parts(dict(qp=got['qp'], stats=got['mm']), mn, mx, p, where + ('packed nhwc',))
        codes = PK.unpack(packed.cpu().numpy().tobytes(), np.full(C, 4), N * HW, C).reshape(N, H, W, C).transpose(0, 3, 1, 2)
        check_codes(codes, q_ref, where + ('packed nhwc codes',))
        yd = ops.dequantize_packed_nhwc(packed, shape, dt, got['qp'], got['coloff'])
        check(host(yd.contiguous()), y_ref, where + ('packed nhwc y',))


def test_packed_fronts_fp32_channels_last():
    """ops.minmax_quantize_packed_nhwc on float32 storage, the whole 4-bit tables"""
    L, ops = mods()
    for shape in ((3, 8, 7, 7), (2, 8, 14, 14), (5, 3, 28, 28)):
        N, C, H, W = shape
        for mode in ((4, False), (4, True)):
            for which in ('fast', 'mixed'):
                for names, x, mn, mx, p, y_ref, q_ref in cases(shape, mode, which):
                    where = (shape, mode, which, names)
                    xcl = x.cuda().contiguous(memory_format=torch.channels_last)
                    packed, got = ops.minmax_quantize_packed_nhwc(xcl, 4, mode[1])
                    check_parts(dict(qp=got['qp'], stats=got['mm']), mn, mx, p, where)
                    codes = PK.unpack(packed.cpu().numpy().tobytes(), np.full(C, 4), N * H * W, C).reshape(N, H, W, C).transpose(0, 3, 1, 2)
                    check_codes(codes, q_ref, where)
                    yd = ops.dequantize_packed_nhwc(packed, shape, torch.float32, got['qp'], got['coloff'])
                    check(host(yd.contiguous()), y_ref, where + ('y',))


# ------------------------------------------------------------------------------------------ (d) a table handed in with zp = -0
def test_table_with_negative_zero_zero_point():
    """-sm use: statistics from other data.  The table of neg_zero_zp (scale 1, zp -0) on an x that holds -0.0, negative denormals
    and small negatives - values the channel that made the table never held.  The table-driven kernels (k_qdq, k_h_qdq without
    partials) run the IEEE divide only; what the divide-free form does with zp = -0 is what a tensor can show whose own extrema
    give it, and there every element is positive: flags 0 and 2 of the group launch on such a tensor, the same bytes."""
    L, ops = mods()
    lib = L.load()
    a, b = dict((n, (lo, hi)) for n, lo, hi in M.table((4, False)))['neg_zero_zp']
    sc, zp, qm = M.params_ref([a], [b], 4, False)
    assert np.signbit(zp[0]) and zp[0] == 0
    for shape in ((3, 8, 7, 7), (2, 8, 14, 14), (5, 3, 28, 28)):
        N, C, HW = shape[0], shape[1], shape[2] * shape[3]
        rng = np.random.default_rng(C + HW)
        x = rng.uniform(-0.75, 15.5, size=(N, C, HW)).astype(F32)
        x[:, :, 0::5] = -0.0
        x[:, :, 1::5] = -(2.0 ** -140)
        x[:, :, 2::5] = -(2.0 ** -20)
        x[:, :, 3::7] = 0.0
        x[:, :, 4::11] = 0.5                                   # a tie: 0.5 + -0 rounds to even, 0
        x = x.reshape(shape)
        qp = np.stack([np.full(C, sc[0]), np.full(C, zp[0]), np.full(C, qm)]).astype(F32)
        qp_d = dev(qp)
        assert np.signbit(qp_d.cpu().numpy()[L.QP_ZP]).all()
        y_ref, q_ref = M.qdq_ref(x, qp[0], qp[1], qm)
        assert not np.signbit(y_ref[x == 0]).any() and (q_ref[x <= 0] == 0).all()
        xd = dev(x)
        y, codes = ops.pc_qdq(xd, N, C, HW, qp_d, want_codes=True)
        check(host(y), y_ref, (shape, 'pc_qdq y'))
        check_codes(codes.cpu().numpy(), q_ref, (shape, 'pc_qdq codes'))
        for name, dt in (('bf16', torch.bfloat16), ('f16', torch.float16)):
            xh = torch.from_numpy(x).to(dt)
            yh_ref, _ = M.qdq_ref(xh.float().numpy(), qp[0], qp[1], qm)
            yh = torch.empty_like(xh, device='cuda')
            xh_d = xh.cuda()
            L.check(lib.cnnq_pc_qdq_dt(xh_d.data_ptr(), yh.data_ptr(), ops._DTYPE_CODES[dt], N, C, HW, qp_d.data_ptr(), None, None, 0,
                                       stream()), 'cnnq_pc_qdq_dt')
            check(host(yh), torch.from_numpy(yh_ref).to(dt).float().numpy(), (shape, name))
        # the divide-free form meets zp = -0 only behind extrema of its own
        xt, mn, mx = M.window_tensor(shape, [('neg_zero_zp', a, b)] * C, 5)
        y_ref, _ = M.qdq_ref(xt.numpy(), *M.params_ref(mn, mx, 4, False))
        ys = {}
        for flags in (0, 2):
            yt, parts = ops.minmax_qdq_group(xt.cuda(), N, C, HW, 4, False, want_parts=True, flags=flags)
            assert np.signbit(host(parts['qp'])[L.QP_ZP]).all(), (shape, flags)
            ys[flags] = host(yt)
            check(ys[flags], y_ref, (shape, 'group', flags))
        assert ys[0].tobytes() == ys[2].tobytes()
