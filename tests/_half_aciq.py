"""What tests/test_half_aciq_cpu.py and tests/test_half_aciq_gpu.py share: the shapes that reach each branch
of cnnq_pc_aciq_qdq_dt and its route rule restated in Python."""
from _half_collect import piece, splits

WHOLE_CAP = 1024 * 128            # csrc/cnnq_half.hip.h, h_whole_cap: the elements a 1024-lane workgroup keeps in registers

# (shape, storage offset in elements) -> (W, batch splits S, column splits, the resident form fits): the smallest shapes that
# reach each branch
CASES = [((8, 12, 28, 28), 0, (8, 1, 1, True)),          # W = 8, resident
         ((3, 10, 14, 14), 0, (4, 1, 1, True)),          # W = 4
         ((3, 6, 7, 14), 0, (2, 1, 1, True)),            # W = 2; a partial last step of the resident walk
         ((2, 64, 7, 7), 0, (1, 1, 1, False)),           # W = 1: the chain only
         ((8, 12, 28, 28), 1, (1, 1, 1, False)),         # the W = 8 shape at an odd element offset: W = 1
         ((5, 6, 80, 80), 0, (8, 2, 1, True)),           # two uneven batch splits (2 and 3 samples)
         ((1, 4, 224, 224), 0, (8, 1, 4, True)),         # column splits of the rows
         ((32, 2, 64, 64), 0, (8, 8, 1, True)),          # a population of exactly 131072: the last that fits
         ((33, 2, 64, 64), 0, (8, 9, 1, False))]         # the first that does not: the chain whatever the caller allows
IDS = ['%s+%d' % ('x'.join(map(str, s)), o) for s, o, _ in CASES]


def whole_fits(N, HW, W):
    """k_h_aciq_whole holds the channel: packed pieces (W >= 2) of at most WHOLE_CAP elements."""
    return W >= 2 and N * HW <= WHOLE_CAP


def whole_wins(N, C, HW, ba):
    """h_aciq_whole_wins: the classes where the resident form measured faster than the chain: at least 128
    channels and - a population of 65536 per channel on - at most 512 with bit allocation, 1024 without; from 25088 on, 256
    channels, without bit allocation also up to 512."""
    pop = N * HW
    if C < 128:
        return False
    if pop >= 65536:
        return C <= (512 if ba else 1024)
    return pop >= 25088 and 256 <= C <= (256 if ba else 512)


def native(N, C, HW):
    """h_aciq_native: the classes that measured faster native than through the upcast: all but rows of an
    odd length - single elements whatever the alignment - with a population of 6272 per channel or more."""
    return not (HW % 2 == 1 and N * HW >= 6272)


def route(N, C, HW, align, allow, ba=False, prior_is_b=False):
    """out[4] of cnnq_pc_route_aciq_dt for a bf16 / fp16 tensor; ba: bit allocation in effect."""
    W = piece(HW, align)
    S, cs = splits(N, C, HW)
    if allow and not (ba and prior_is_b) and whole_fits(N, HW, W) and (allow > 1 or whole_wins(N, C, HW, ba)):
        r = 3 if ba else 1
    else:
        r = 2 if native(N, C, HW) else 0
    return W, S, cs, r
