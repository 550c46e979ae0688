"""What tests/test_half_midtread_cpu.py and tests/test_half_midtread_gpu.py share: the shapes that reach each
branch of cnnq_pc_midtread_dt (tests/_half_aciq.py: CASES), the benchmark's classes of layer, and the route rule restated in Python."""
from _half_aciq import CASES, IDS, WHOLE_CAP, whole_fits  # noqa: F401
from _half_collect import piece, splits

# the conv outputs of VGG-16 and ResNet-50 at batch 512 (tools/bench_half_midtread.py): (C, H) of [512, C, H, H]
VGG16 = [(64, 224), (128, 112), (256, 56), (512, 28), (512, 14)]
RESNET50 = [(64, 112), (64, 56), (256, 56), (128, 56), (128, 28), (512, 28), (256, 28), (256, 14), (1024, 14), (512, 14), (512, 7), (2048, 7)]
CLASSES = [(512, C, H * H) for C, H in VGG16 + RESNET50]


def whole_wins(N, C, HW, hist):
    """h_mt_whole_wins: the classes where the resident form measured faster than the chain: 256 channels at
    a population of 100352 per channel or more."""
    return C == 256 and N * HW >= 100352


def native(N, C, HW, hist):
    """h_mt_native: the classes that measured faster native than through the upcast: all but rows of an odd
    length - single elements whatever the alignment - with a population of 6272 per channel or more."""
    return not (HW % 2 == 1 and N * HW >= 6272)


def route(N, C, HW, align, allow, hist=False):
    """out[4] of cnnq_pc_route_midtread_dt for a bf16 / fp16 tensor."""
    W = piece(HW, align)
    S, cs = splits(N, C, HW)
    if allow and whole_fits(N, HW, W) and (allow > 1 or whole_wins(N, C, HW, hist)):
        r = 3
    else:
        r = 2 if native(N, C, HW, hist) else 0
    return W, S, cs, r
