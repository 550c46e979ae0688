"""The host side of cnnq_dwconv_codes / cnnq_dwconv_codes_q without a device: what is refused before anything
is enqueued, with which error, and the tile, slab and load path the route gives MobileNetV2's depthwise layers."""
import ctypes

import pytest

from test_conv_codes_cpu import EINVAL, ERANGE, P, PACK4, U8

GEO = dict(N=1, H=8, W=8, C=16, KH=3, KW=3, sh=1, sw=1, ph=1, pw=1)


def geometry(kw):
    return (ctypes.c_int64 * 10)(*dict(GEO, **{k: kw[k] for k in kw if k in GEO}).values())


@pytest.mark.parametrize('kw,rc', [
    (dict(fx=2), EINVAL), (dict(fw=-1), EINVAL), (dict(fy=2), EINVAL),                      # a format outside cnnq_code_format
    (dict(KH=0), EINVAL), (dict(sw=0), EINVAL), (dict(N=0), EINVAL), (dict(pw=-1), EINVAL),  # a size or stride below 1, negative padding
    (dict(KH=11, ph=1), EINVAL), (dict(KW=9, pw=0), EINVAL),                                # no output pixel
    (dict(C=18), EINVAL), (dict(C=20, fx=PACK4), EINVAL), (dict(C=20, fw=PACK4), EINVAL), (dict(C=20, fy=PACK4), EINVAL),
    (dict(Cx=2), EINVAL), (dict(Cy=3), EINVAL), (dict(N=4, Cx=2), EINVAL),
    (dict(xq=None), EINVAL), (dict(wq=None), EINVAL), (dict(y=None), EINVAL), (dict(qpx=None), EINVAL), (dict(qpw=None), EINVAL),
    (dict(qpy=None), EINVAL), (dict(xq=P + 2), EINVAL), (dict(wq=P + 1), EINVAL), (dict(y=P + 2), EINVAL), (dict(bias=P + 2), EINVAL),
    (dict(qpy=P + 1), EINVAL),
    (dict(KH=9, KW=8, H=16, W=16), ERANGE),                                                 # 72 taps
    (dict(H=1 << 31), ERANGE), (dict(sh=1 << 31), ERANGE),                                  # an extent of 2^31
    (dict(N=1 << 12, H=64, W=64, C=128), ERANGE),                                           # N OH OW C = 2^31
    (dict(N=1 << 20, H=64, W=64), ERANGE),                                                  # 2^32 pixels
], ids=str)
def test_refused_before_the_device(kw, rc):
    from cnn_quantization_amd import _lib as L
    lib, g = L.load(), geometry(kw)
    xq, wq, y, qpx, qpw, qpy = (kw.get(k, P) for k in ('xq', 'wq', 'y', 'qpx', 'qpw', 'qpy'))
    fx, fw, bias = kw.get('fx', U8), kw.get('fw', U8), kw.get('bias')
    if not {'fy', 'Cy', 'qpy'} & set(kw):
        assert lib.cnnq_dwconv_codes(xq, fx, wq, fw, y, g, qpx, kw.get('Cx', 1), qpw, bias, None) == rc
    assert lib.cnnq_dwconv_codes_q(xq, fx, wq, fw, y, kw.get('fy', U8), g, qpx, kw.get('Cx', 1), qpw, bias, qpy, kw.get('Cy', 1), 1, None) == rc
    if not set(kw) - set(GEO) - {'fx', 'fw'}:        # a refused geometry has no route
        assert lib.cnnq_dwconv_codes_route(g, fx, fw, 16, (ctypes.c_int32 * 6)()) == rc


def test_a_window_of_64_taps_always_has_a_tile():
    """With KH KW <= 64 the patch of ONE output pixel is at most 64 pixels x a slab of two dwords, far inside the 32 KB patch: the plan
    shrinks the tile to that pixel before it would refuse (CNNQ_ERANGE for a window beyond the LDS is unreachable behind the tap limit)."""
    from cnn_quantization_amd import _lib as L
    out = (ctypes.c_int32 * 6)()
    g = geometry(dict(H=64, W=1 << 22, KH=64, KW=1, ph=0, pw=0, sw=1 << 20))      # a stride of 2^20: no two pixels share a patch
    assert L.load().cnnq_dwconv_codes_route(g, U8, U8, 16, out) == 0 and list(out) == [1, 1, 16, 1, 1, 4]


@pytest.mark.parametrize('geo,u8,pack4', [
    # MobileNetV2's distinct depthwise layers at batch 64: {tile rows, columns, slab bytes of xq, 16-byte path, OH, OW}
    (dict(N=64, H=112, W=112, C=32), [8, 16, 32, 1, 112, 112], [8, 16, 16, 1, 112, 112]),
    (dict(N=64, H=112, W=112, C=96, sh=2, sw=2), [8, 8, 64, 1, 56, 56], [8, 8, 32, 1, 56, 56]),       # 17 x 33 x 16 dwords: the tile shrinks
    (dict(N=64, H=56, W=56, C=144), [8, 16, 64, 1, 56, 56], [8, 16, 32, 0, 56, 56]),                  # 72 pack4 bytes a pixel: dwords
    (dict(N=64, H=56, W=56, C=144, sh=2, sw=2), [8, 8, 64, 1, 28, 28], [8, 8, 32, 0, 28, 28]),
    (dict(N=64, H=28, W=28, C=192), [8, 16, 64, 1, 28, 28], [8, 16, 32, 1, 28, 28]),
    (dict(N=64, H=28, W=28, C=192, sh=2, sw=2), [8, 14, 32, 1, 14, 14], [8, 14, 16, 1, 14, 14]),       # 384 workgroups: half slabs
    (dict(N=64, H=14, W=14, C=384), [8, 14, 64, 1, 14, 14], [8, 14, 32, 1, 14, 14]),
    (dict(N=64, H=14, W=14, C=576), [8, 14, 64, 1, 14, 14], [8, 14, 32, 1, 14, 14]),
    (dict(N=64, H=14, W=14, C=576, sh=2, sw=2), [7, 7, 64, 1, 7, 7], [7, 7, 32, 1, 7, 7]),
    (dict(N=64, H=7, W=7, C=960), [7, 7, 64, 1, 7, 7], [7, 7, 32, 1, 7, 7]),
    (dict(N=1, H=7, W=7, C=960), [7, 7, 32, 1, 7, 7], [7, 7, 16, 1, 7, 7]),                            # batch 1: 30 half slabs
    (dict(N=1, H=112, W=112, C=96, sh=2, sw=2), [8, 16, 32, 1, 56, 56], [8, 16, 16, 1, 56, 56]),
], ids=str)
def test_route_of_mobilenetv2_layers(geo, u8, pack4):
    from cnn_quantization_amd import _lib as L
    lib, out, g = L.load(), (ctypes.c_int32 * 6)(), geometry(geo)
    assert lib.cnnq_dwconv_codes_route(g, U8, U8, 16, out) == 0 and list(out) == u8
    assert lib.cnnq_dwconv_codes_route(g, PACK4, U8, 16, out) == 0 and list(out) == pack4
    assert lib.cnnq_dwconv_codes_route(g, U8, PACK4, 4, out) == 0 and list(out) == u8[:3] + [0] + u8[4:]      # bases of 4 bytes: dwords
    assert lib.cnnq_dwconv_codes_route(g, U8, U8, 3, out) == EINVAL and lib.cnnq_dwconv_codes_route(g, U8, U8, 16, None) == EINVAL
