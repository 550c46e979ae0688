"""What the CPU tests of IntQuantizer's routing share: the constructor's full parameter dict, one factory, a CPU tensor that says it is
on the device, and the two tensor makers."""
import torch

PARAMS = dict(clipping='no', pcq_weights=False, pcq_act=False, bit_alloc_act=False, bit_alloc_weight=False, bcorr_act=False,
              bcorr_weight=False, vcorr_weight=False, bit_alloc_rmode='round', bit_alloc_prior='gaus', bit_alloc_target_act=None,
              bit_alloc_target_weight=None, measure_entropy=False, logger=None, mtd_quant=False)


def quantizer(bits=4, **kw):
    """IntQuantizer(bits, PARAMS updated by kw); a test file with other defaults passes them through its own one-line wrapper."""
    from cnn_quantization_amd.qtypes.int_quantizer import IntQuantizer
    return IntQuantizer(bits, dict(PARAMS, **kw))


class FakeCuda(torch.Tensor):
    """A CPU tensor that says it lives on the device: the predicates read shape, strides, dtype and this flag only."""
    @staticmethod
    def __new__(cls, t):
        return torch.Tensor._make_subclass(cls, t)

    @property
    def is_cuda(self):
        return True


def act(dtype=torch.bfloat16, shape=(2, 8, 4, 4)):
    """A contiguous activation on the "device"."""
    return FakeCuda(torch.zeros(shape, dtype=dtype))


def nhwc(dtype=torch.bfloat16, shape=(2, 8, 4, 4)):
    """A dense channels_last activation on the "device"."""
    return FakeCuda(torch.zeros(shape, dtype=dtype).to(memory_format=torch.channels_last))
