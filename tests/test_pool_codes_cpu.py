"""The host side of cnnq_max_pool_codes / cnnq_avg_pool_codes / cnnq_avg_pool_codes_q without a device: what is
refused before anything is enqueued, with which error, and the tile and load path the route gives ResNet-50's stem pool."""
import ctypes

import pytest

from test_conv_codes_cpu import EINVAL, ERANGE, P, PACK4, U8

MAXG = dict(N=1, H=8, W=8, C=16, KH=3, KW=3, sh=2, sw=2, ph=1, pw=1)
AVGG = dict(N=2, H=7, W=7, C=16)


def arr(base, kw):
    v = dict(base, **{k: kw[k] for k in kw if k in base}).values()
    return (ctypes.c_int64 * len(base))(*v)


@pytest.mark.parametrize('kw,rc', [
    (dict(fmt=2), EINVAL), (dict(fmt=-1), EINVAL),                                          # a format outside cnnq_code_format
    (dict(KH=0), EINVAL), (dict(sw=0), EINVAL), (dict(N=0), EINVAL),                        # a size or stride below 1
    (dict(ph=-1), EINVAL), (dict(ph=2), EINVAL), (dict(KW=2, pw=2), EINVAL),                # padding negative / above half the kernel
    (dict(H=2, KH=6, ph=1), EINVAL),                                                        # no output pixel
    (dict(C=18), EINVAL), (dict(C=20, fmt=PACK4), EINVAL),                                  # C % 4, C % 8
    (dict(xq=None), EINVAL), (dict(y=None), EINVAL), (dict(xq=P + 2), EINVAL), (dict(y=P + 1), EINVAL),
    (dict(H=1 << 31), ERANGE), (dict(sh=1 << 31), ERANGE),                                  # an extent of 2^31
    (dict(N=1 << 20, H=64, W=64), ERANGE),                                                  # 2^32 input pixels
    (dict(N=1 << 30, H=1, W=1, KH=2, KW=2, sh=1, sw=1, ph=1, pw=1), ERANGE),                # 2^30 input pixels, 2^32 output pixels
    (dict(H=400, W=400, KH=120, KW=120, ph=0, pw=0), ERANGE),                               # a window beyond the LDS
], ids=str)
def test_max_pool_refused_before_the_device(kw, rc):
    from cnn_quantization_amd import _lib as L
    lib, g, fmt = L.load(), arr(MAXG, kw), kw.get('fmt', U8)
    assert lib.cnnq_max_pool_codes(kw.get('xq', P), fmt, kw.get('y', P + 4096), g, None) == rc
    if not {'xq', 'y'} & set(kw):       # a refused geometry has no route
        assert lib.cnnq_max_pool_codes_route(g, fmt, 16, (ctypes.c_int32 * 6)()) == rc


def test_max_pool_route_answers_without_a_device():
    """ResNet-50's stem pool: tiles of 8 x 8 output pixels x the 64 (u8) / 32 (pack4) channel bytes, 16-byte pieces on aligned bases."""
    from cnn_quantization_amd import _lib as L
    lib, out = L.load(), (ctypes.c_int32 * 6)()
    g = arr(MAXG, dict(N=64, H=112, W=112, C=64))
    for fmt, nbytes in ((U8, 64), (PACK4, 32)):
        assert lib.cnnq_max_pool_codes_route(g, fmt, 16, out) == 0 and list(out) == [8, 8, nbytes, 1, 56, 56]
        assert lib.cnnq_max_pool_codes_route(g, fmt, 4, out) == 0 and list(out) == [8, 8, nbytes, 0, 56, 56]
    assert lib.cnnq_max_pool_codes_route(arr(MAXG, dict(C=24)), U8, 16, out) == 0 and list(out) == [4, 4, 24, 0, 4, 4]     # 24 bytes a pixel
    big = arr(MAXG, dict(H=64, W=64, C=64, KH=31, KW=31, ph=15, pw=15))      # a 31 x 31 window: the tile and the slab shrink to the LDS
    assert lib.cnnq_max_pool_codes_route(big, U8, 16, out) == 0 and list(out) == [1, 1, 32, 1, 32, 32]
    assert lib.cnnq_max_pool_codes_route(g, U8, 3, out) == EINVAL and lib.cnnq_max_pool_codes_route(g, U8, 16, None) == EINVAL


@pytest.mark.parametrize('kw,rc', [
    (dict(fx=2), EINVAL), (dict(fy=-1), EINVAL), (dict(W=0), EINVAL), (dict(C=18), EINVAL), (dict(C=20, fx=PACK4), EINVAL),
    (dict(C=20, fy=PACK4), EINVAL),                                                         # the output's own divisibility
    (dict(Cx=3), EINVAL), (dict(Cy=3), EINVAL), (dict(N=4, Cx=2), EINVAL),
    (dict(xq=None), EINVAL), (dict(y=None), EINVAL), (dict(qpx=None), EINVAL), (dict(qpy=None), EINVAL),
    (dict(xq=P + 2), EINVAL), (dict(y=P + 4), EINVAL), (dict(qpx=P + 2), EINVAL), (dict(qpy=P + 1), EINVAL),
    (dict(C=1 << 31), ERANGE), (dict(H=1 << 12, W=1 << 11), ERANGE),                        # an extent of 2^31; H W = 2^23
    (dict(N=1 << 12, H=1 << 10, W=1 << 9), ERANGE),                                         # 2^31 pixels
], ids=str)
def test_avg_pool_refused_before_the_device(kw, rc):
    """y = P + 4 is 4-byte aligned: refused by the fp32 entry (16 bytes for its float4 stores), a fine address for codes."""
    from cnn_quantization_amd import _lib as L
    lib, g = L.load(), arr(AVGG, kw)
    xq, y, qpx, qpy = (kw.get(k, P) for k in ('xq', 'y', 'qpx', 'qpy'))
    if not {'fy', 'Cy', 'qpy'} & set(kw):
        assert lib.cnnq_avg_pool_codes(xq, kw.get('fx', U8), y, g, qpx, kw.get('Cx', 1), None) == rc
    if kw.get('y', P) != P + 4:
        assert lib.cnnq_avg_pool_codes_q(xq, kw.get('fx', U8), y, kw.get('fy', U8), g, qpx, kw.get('Cx', 1), qpy, kw.get('Cy', 1), None) == rc
