"""What tests/test_half_bcorr_cpu.py and tests/test_half_bcorr_gpu.py share: the shapes that reach each
branch of cnnq_pc_qdq_bcorr_dt and its route rule restated in Python."""
from _half_collect import piece, splits

WHOLE_CAP = 1024 * 128            # csrc/cnnq_half.hip.h, h_whole_cap: the elements a 1024-lane workgroup keeps in registers

# (shape, storage offset in elements) -> (W, batch splits S, column splits, the single launch fits)
CASES = [((2, 3, 8, 8), 0, (8, 1, 1, True)),            # W = 8
         ((4, 16, 14, 14), 0, (4, 1, 1, True)),         # W = 4
         ((3, 5, 5, 10), 0, (2, 1, 1, True)),           # W = 2; a partial last step of the resident walk (75 pairs, 1024 lanes)
         ((3, 5, 7, 7), 0, (1, 1, 1, False)),           # W = 1: two passes only
         ((2, 3, 8, 8), 1, (1, 1, 1, False)),           # the W = 8 shape at an odd element offset: W = 1
         ((2, 3, 8, 8), 4, (4, 1, 1, True)),            # ... at 8 bytes: W = 4
         ((40, 3, 28, 28), 0, (8, 2, 1, True)),         # S > 1
         ((1, 2, 128, 256), 0, (8, 1, 2, True)),        # column splits of the rows
         ((64, 1, 32, 64), 0, (8, 8, 1, True)),         # exactly the resident capacity; C = 1
         ((65, 1, 32, 64), 0, (8, 9, 1, False)),        # one sample beyond it: the route function says 2
         ((5, 1, 6, 6), 0, (4, 1, 1, True))]            # a single channel
IDS = ['%s+%d' % ('x'.join(map(str, s)), o) for s, o, _ in CASES]


def whole_fits(N, HW, W):
    """k_h_bcorr_whole holds the channel: packed pieces (W >= 2) of at most WHOLE_CAP elements."""
    return W >= 2 and N * HW <= WHOLE_CAP


def whole_wins(N, C, HW):
    """h_bcorr_whole_wins: the classes where the single launch measured faster than the two passes:
    exactly one full round of workgroups on the device's 256 compute units, a population of at least 32768 per channel."""
    return C == 256 and N * HW >= 32768


def native(N, C, HW):
    """h_bcorr_native: the classes that measured faster native than through the upcast: all of them."""
    return True


def route(N, C, HW, align, allow):
    """out[4] of cnnq_pc_route_qdq_bcorr_dt for a bf16 / fp16 tensor."""
    W = piece(HW, align)
    S, cs = splits(N, C, HW)
    if allow and whole_fits(N, HW, W) and (allow > 1 or whole_wins(N, C, HW)):
        r = 1
    else:
        r = 2 if native(N, C, HW) else 0
    return W, S, cs, r
