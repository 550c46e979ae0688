"""The per-sample channel extrema of `-sm collect -sba` (smpc.py:72-78) on the device: ops.pc_sample_extrema_half
on contiguous bf16 / fp16 and ops.pc_sample_extrema_nhwc on dense channels_last fp32 / bf16 / fp16 against torch on the same tensor -
x.float().view(N, C, -1).amin(-1) / .amax(-1) - as values, NaN positions equal, and two runs on one input the same bytes.  The shapes
are the smallest that reach each branch of the two plans (tests/test_sba_collect_cpu.py checks on the CPU that they do); the inputs
plant every row's extrema at its first and last element next to larger ones of the adjacent rows, and hold a NaN, a +inf, a -inf and a
constant row (tests/_sample_extrema.py)."""
import pytest
import torch

import _sample_extrema as SE

pytestmark = pytest.mark.gpu
HALF = [torch.bfloat16, torch.float16]


def check(op, x_cpu):
    from cnn_quantization_amd import _lib as L, ops
    assert (L.STAT_MIN, L.STAT_MAX) == (0, 1)
    x = SE.to_device(x_cpu)
    assert x.stride() == x_cpu.stride() and x.data_ptr() % 16 == (x_cpu.storage_offset() * x.element_size()) % 16
    copies = ops.LAYOUT_COPIES
    ext = op(x)
    again = op(x)
    want = SE.reference(x)
    N, C = x.shape[0], x.shape[1]
    assert ext.shape == (2, N * C) and ext.dtype == torch.float32 and ext.is_contiguous() and ops.LAYOUT_COPIES == copies
    assert SE.same_values(ext, want), (tuple(x.shape), (ext != want).nonzero()[:8].tolist())
    assert torch.equal(ext.view(torch.int32), again.view(torch.int32))            # run after run the same bits
    rows = N * C
    if rows > 1:
        assert bool(torch.isnan(ext[:, 1]).all())                                 # a NaN in the row: both entries
    if rows > 3:
        assert ext[1, 2] == float('inf') and ext[0, 3] == float('-inf')
    if rows > 4:
        assert ext[0, 4] == 1.25 and ext[1, 4] == 1.25
    return ext


@pytest.mark.parametrize('first_max', [True, False])
@pytest.mark.parametrize('dtype', HALF)
@pytest.mark.parametrize('case', SE.HALF_CASES, ids=lambda c: '%dx%dx%dx%d+%d' % (c[0] + (c[1],)))
def test_contiguous_half(case, dtype, first_max):
    from cnn_quantization_amd import ops
    shape, offset, _ = case
    x = SE.make_input(shape, dtype, False, offset, first_max)
    assert x.is_contiguous() and x.storage_offset() == offset
    check(ops.pc_sample_extrema_half, x)


@pytest.mark.parametrize('first_max', [True, False])
@pytest.mark.parametrize('dtype', [torch.float32] + HALF)
@pytest.mark.parametrize('case', SE.NHWC_CASES, ids=lambda c: '%dx%dx%dx%d+%d' % (c[0] + (c[1],)))
def test_channels_last(case, dtype, first_max):
    from cnn_quantization_amd import ops
    shape, offset, _ = case
    x = SE.make_input(shape, dtype, True, offset, first_max)
    assert ops._layout(x) == 'nhwc' and x.storage_offset() == offset
    check(ops.pc_sample_extrema_nhwc, x)


def test_the_table_is_what_the_row_statistics_give():
    """The second yardstick: ops.tensor_row_stats on the [N * C, HW] view answers the same [2, rows] table."""
    from cnn_quantization_amd import ops
    x = SE.make_input((2, 4, 14, 14), torch.bfloat16, False, 0, True).cuda()
    assert SE.same_values(ops.pc_sample_extrema_half(x), ops.tensor_row_stats(x, 8))
