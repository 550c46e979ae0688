"""What the tests of the per-sample extrema (`-sm collect -sba`) share: the two launch plans restated in Python
(cnnq_sample_extrema.hip.h: h_se_seg / h_se_steps for contiguous bf16 / fp16, cl_se_slabs / cl_geo_se for channels_last), who owns what
under them, the GPU tests' case lists with the branch each case is there for, and the maker of their inputs."""
import numpy as np
import torch

TPB = 256
SE_HW = 8                   # elements of a 16-byte load of a bf16 / fp16 row
H_SE_PPL = 4
H_MM_ELEMS = 16384
CL_SE_ELEMS = 16384
CL_SE_MAX_WGS = 1024


def cdiv(a, b):
    return -(-a // b)


# ---- contiguous bf16 / fp16: rows of HW elements back to back
def seg(HW):
    nv = cdiv(HW, SE_HW)
    s = 1
    while s < 8 and s < nv:
        s *= 2
    while s < 64 and s * H_SE_PPL < nv:
        s *= 2
    return s


def half_plan(N, C, HW):
    """(seg, rows per workgroup, workgroups): the first three words of cnnq_pc_route_sample_extrema_dt."""
    rows, sg = N * C, seg(HW)
    nseg = TPB // sg
    steps = max(1, min(H_MM_ELEMS // (nseg * HW), cdiv(rows, nseg)))
    return sg, steps * nseg, cdiv(rows, steps * nseg)


def half_native(N, C, HW):
    """The "native" word: the classes that did not win against the former route stay there (h_sample_extrema_native)."""
    return int(not (HW % 8 != 0 and N * HW >= H_MM_ELEMS and N * C * HW < 1 << 25))


def half_owned(N, C, HW, sg, rpw, grid):
    """How often each of the N * C rows is owned: workgroup b, step k, segment s take row b * rpw + k * (TPB / seg) + s."""
    rows, nseg = N * C, TPB // sg
    assert rpw % nseg == 0
    r = (np.arange(grid, dtype=np.int64)[:, None, None] * rpw + np.arange(rpw // nseg, dtype=np.int64)[None, :, None] * nseg
         + np.arange(nseg, dtype=np.int64)[None, None, :]).ravel()
    return np.bincount(r[r < rows], minlength=rows)


def row_walk(addr, HW):
    """(head, whole loads, tail start) of a row at byte address addr: the elements in front of the first 16-byte boundary, the
    16-byte loads, where the single elements behind them begin."""
    head = min(((16 - addr % 16) % 16) // 2, HW)
    nv = (HW - head) // SE_HW
    return head, nv, head + nv * SE_HW


# ---- channels_last: [N][HW][C]
def piece(C, esize, align):
    w = 16 // esize
    while w > 1:
        if C % w == 0 and align % (w * esize) == 0:
            return w
        w //= 2
    return 1


def slabs(N, HW, C, esize):
    colw = min(C, TPB * (16 // esize))
    S = min(cdiv(HW, cdiv(CL_SE_ELEMS, colw)), CL_SE_MAX_WGS // N)
    return max(S, 1)


def nhwc_geo(N, HW, C, w, esize):
    """dict(P, CP, RS, nb, S, rpw): cl_geo_se."""
    P = C // w
    CP = min(P, TPB)
    RS = TPB // CP
    S = slabs(N, HW, C, esize)
    return dict(P=P, CP=CP, RS=RS, nb=cdiv(P, CP), S=S, rpw=cdiv(cdiv(HW, S), RS) * RS)


def nhwc_owned(HW, g, lanes=False):
    """How often each (hw-row, channel piece) of ONE sample is owned by the S * nb workgroups of that sample.  lanes: lane by lane
    as cl_lane places them (small shapes); else by the workgroup's row and piece ranges."""
    seen = np.zeros((HW, g['P']), dtype=np.int32)
    assert g['RS'] * g['CP'] <= TPB
    for s in range(g['S']):
        r0, r1 = s * g['rpw'], min((s + 1) * g['rpw'], HW)
        for b in range(g['nb']):
            if not lanes:
                seen[r0:max(r0, r1), b * g['CP']:min((b + 1) * g['CP'], g['P'])] += 1
                continue
            for t in range(TPB):
                lr, lp = divmod(t, g['CP'])
                p = b * g['CP'] + lp
                if lr < g['RS'] and p < g['P']:
                    seen[r0 + lr:max(r0 + lr, r1):g['RS'], p] += 1
    return seen


# ---- the GPU tests' cases: (shape, element offset of the view into a larger buffer, what the case is there for)
HALF_CASES = [((2, 3, 7, 7), 0, 'odd HW, 2-byte aligned rows'),
              ((3, 5, 1, 2), 0, 'the shortest row the manager sends'),
              ((2, 4, 14, 14), 0, 'rows alternate between 16-byte and 8-byte alignment'),
              ((2, 2, 56, 56), 0, 'several steps per segment'),
              ((1, 2, 225, 223), 0, 'a long odd row'),
              ((64, 520, 2, 2), 0, 'many more rows than segments, a partly filled last workgroup'),
              ((2, 3, 3, 4), 0, 'seg 2'),
              ((2, 3, 5, 5), 0, 'seg 4'),
              ((2, 2, 17, 19), 0, 'seg 16'),
              ((2, 2, 28, 28), 0, 'seg 32'),
              ((2, 4, 14, 14), 1, 'a view one element into a larger buffer: a 2-byte aligned base')]
NHWC_CASES = [((2, 3, 7, 7), 0, 'odd C: single elements'),
              ((3, 5, 1, 2), 0, 'the shortest row the manager sends'),
              ((2, 67, 5, 3), 0, 'C not a multiple of the piece'),
              ((2, 1030, 2, 2), 0, 'several channel blocks'),
              ((1, 8, 56, 56), 0, 'S > 1: partial pairs and the fold'),
              ((2, 16, 9, 5), 0, 'the widest piece, several row-lanes per piece'),
              ((2, 16, 9, 5), 1, 'a view at a storage offset')]


def make_input(shape, dtype, nhwc, offset, first_max, seed=0):
    """A CPU tensor of `shape` (logical NCHW; nhwc: dense channels_last, else contiguous), a view `offset` elements into a larger
    buffer.  Normal values scaled per (n, c) row r = n * C + c; every row's maximum planted at its first element and its minimum at
    its last (first_max) or the other way round, with magnitudes that grow (or shrink) with r so that the element next to a row's
    end in memory - the adjacent row's planted extremum; for channels_last the previous / next sample and the neighbouring channels
    - has the LARGER magnitude of that sign: a mask that is off by one shows.  Rows 1..4, where the tensor has them: a NaN in the
    middle, +inf, -inf, a constant row."""
    N, C, H, W = shape
    HW, rows = H * W, N * C
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(rows, HW, generator=gen) * (0.5 + torch.arange(rows, dtype=torch.float32) / rows)[:, None]
    x = x.clamp(-7, 7)
    up = 16 + 16 * torch.arange(rows, dtype=torch.float32) / rows          # grows with r
    down = 32 - 16 * torch.arange(rows, dtype=torch.float32) / rows        # shrinks with r
    if first_max:
        x[:, 0], x[:, -1] = up, -down        # behind a row: the next row's larger maximum; in front: the previous row's lower minimum
    else:
        x[:, 0], x[:, -1] = -up, down
    mid = HW // 2
    for r, v in ((1, float('nan')), (2, float('inf')), (3, float('-inf'))):
        if r < rows:
            x[r, mid] = v
    if rows > 4:
        x[4] = 1.25
    x = x.view(N, C, H, W).to(dtype)
    buf = torch.zeros(x.numel() + 8, dtype=dtype)
    if nhwc:
        buf[offset:offset + x.numel()] = x.permute(0, 2, 3, 1).reshape(-1)
        return buf[offset:offset + x.numel()].view(N, H, W, C).permute(0, 3, 1, 2)
    buf[offset:offset + x.numel()] = x.reshape(-1)
    return buf[offset:offset + x.numel()].view(N, C, H, W)


def to_device(x):
    """The same view of a device copy of x's whole buffer: a view at an element offset keeps its offset, and so its alignment."""
    whole = torch.empty(0, dtype=x.dtype).set_(x.untyped_storage())
    return torch.as_strided(whole.cuda(), x.shape, x.stride(), x.storage_offset())


def reference(x):
    """[2, N * C] float32: the rows' minima and maxima of the exactly upconverted tensor, by torch where x lies."""
    N, C = x.shape[0], x.shape[1]
    f = x.float().reshape(N, C, -1)
    return torch.stack([f.amin(-1).reshape(-1), f.amax(-1).reshape(-1)])


def same_values(a, b):
    """Equal as values, NaN positions equal (the sign of a zero is not pinned)."""
    return bool((torch.isnan(a) == torch.isnan(b)).all() and (a[~torch.isnan(a)] == b[~torch.isnan(b)]).all())
