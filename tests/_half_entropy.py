"""What tests/test_half_entropy_cpu.py and tests/test_half_entropy_gpu.py share: the shapes that reach each
branch of the counting pass over contiguous bf16 / fp16 activations, the benchmark's classes of layer, and the route function
cnnq_pc_route_qdq_hist_dt restated in Python."""
from _half_aciq import WHOLE_CAP, whole_fits  # noqa: F401
from _half_collect import H_MM_ELEMS, piece
from _half_midtread import CLASSES, RESNET50, VGG16  # noqa: F401

H_QDQ_ELEMS = 8192                 # csrc/cnnq_half.hip.h: elements per workgroup of the element-wise pass

# (shape, storage offset in elements) -> (W, batch splits S of the counting launch, column splits of config 2's statistics launch,
# the resident form fits): the smallest shapes that reach each branch
CASES = [((2, 3, 4, 4), 0, (8, 1, 1, True)),             # W = 8, one piece per row and lanes to spare
         ((3, 5, 8, 8), 0, (8, 1, 1, True)),             # W = 8
         ((3, 5, 14, 14), 0, (4, 1, 1, True)),           # W = 4
         ((3, 5, 3, 6), 0, (2, 1, 1, True)),             # W = 2
         ((4, 8, 7, 7), 0, (1, 1, 1, False)),            # W = 1: the two launches only
         ((3, 5, 8, 8), 1, (1, 1, 1, False)),            # the W = 8 shape at an odd element offset: W = 1
         ((48, 4, 14, 14), 0, (4, 2, 1, True)),          # short rows, two batch splits
         ((5, 6, 80, 80), 0, (8, 4, 1, True)),           # long rows at the short tile: four uneven batch splits (1, 1, 1, 2 samples)
         ((1, 4, 224, 224), 0, (8, 1, 4, True)),         # N = 1, long rows: column splits of the statistics launch
         ((3, 70, 8, 8), 0, (8, 1, 1, True)),            # 70 workgroups: replica tables are shared (W = 8)
         ((4, 520, 7, 7), 0, (1, 1, 1, False)),          # ... and at W = 1
         ((8, 32, 14, 14), 0, (4, 1, 1, True)),          # the resident form's ordinary case
         ((128, 2, 32, 32), 0, (8, 16, 1, True)),        # a population of exactly 131072: the last that fits
         ((129, 2, 32, 32), 0, (8, 17, 1, False))]       # the first that does not: the two launches whatever the caller allows
IDS = ['%s+%d' % ('x'.join(map(str, s)), o) for s, o, _ in CASES]
# the long tile: 700 channels x 3 splits of 32768 elements are more than 2048 workgroups (one case, it is 46 M elements)
LONG_TILE = ((84, 700, 28, 28), 0, (8, 3, 1, True))


def h_splits(N, C, HW, per, smax):
    """h_splits (csrc/cnnq_half.hip.h): ~per elements per workgroup, at most N and smax parts, the grid C * S below 2^31."""
    s = max(1, min(-(-N * HW // per), N, smax))
    while s > 1 and C * s >= 1 << 31:
        s -= 1
    return s


def hist_elems(N, C, HW):
    """h_mt_hist_elems, which the counting pass shares with the mid-tread pass that counts: four of the element-wise pass' tiles
    on long rows where that leaves more than 2048 workgroups."""
    if HW <= 196:
        return H_QDQ_ELEMS
    return H_QDQ_ELEMS if C * h_splits(N, C, HW, 4 * H_QDQ_ELEMS, N) <= 2048 else 4 * H_QDQ_ELEMS


def hist_splits(N, C, HW):
    return h_splits(N, C, HW, hist_elems(N, C, HW), N)


def mm_col_splits(N, C, HW, W, G):
    """Column splits of config 2's statistics launch (h_geo_mm); G: the fp32 plan's record count (cnnq_pc_groups, the larger of
    the two alignments')."""
    total = h_splits(N * HW, C, 1, H_MM_ELEMS, G)
    bs = min(total, N)
    return min(total // bs, HW // W)


def whole_wins(N, C, HW, nbins):
    """h_ent_whole_wins: the classes where the resident form measured faster than the two launches: 256
    channels at a population of 100352 per channel or more."""
    return C == 256 and N * HW >= 100352


def native(N, C, HW, nbins):
    """h_ent_native: the classes that measured faster native than through the upcast: all but rows of an
    odd length - single elements whatever the alignment - with a population of 6272 per channel or more."""
    return not (HW % 2 == 1 and N * HW >= 6272)


def route(N, C, HW, align, allow, nbins, G):
    """out[4] of cnnq_pc_route_qdq_hist_dt for a bf16 / fp16 tensor."""
    W = piece(HW, align)
    if allow and whole_fits(N, HW, W) and (allow > 1 or whole_wins(N, C, HW, nbins)):
        r = 1
    else:
        r = 2 if native(N, C, HW, nbins) else 0
    return W, hist_splits(N, C, HW), mm_col_splits(N, C, HW, W, G), r
