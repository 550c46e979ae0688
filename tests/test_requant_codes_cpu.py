"""The host side of cnnq_linear_codes_q / cnnq_conv_codes_q without a device: what is refused before anything
is enqueued - everything the fp32 entries refuse, and the output's own format, divisibility, table and alignment - that the workspace
is the fp32 entries', and the route of one ResNet 3 x 3 layer and one classifier layer."""
import ctypes

import pytest

from test_conv_codes_cpu import EINVAL, ERANGE, GEO, P, PACK4, U8, geometry


def conv(lib, xq=P, fx=U8, wq=P, fw=U8, y=P, fy=U8, qpx=P, Cx=1, qpw=P, bias=None, qpy=P, Cy=1, relu=1, taps=None, splits=0, ws=P, ws_bytes=None, **geo):
    g = geometry(**geo)
    if ws_bytes is None:
        ws_bytes = lib.cnnq_conv_codes_q_workspace(g, fx, fw, fy, int(taps is not None), splits)
    return lib.cnnq_conv_codes_q(xq, fx, wq, fw, y, fy, g, qpx, Cx, qpw, bias, qpy, Cy, relu, taps, splits, ws, ws_bytes, None)


def linear(lib, xq=P, fx=U8, wq=P, fw=U8, y=P, fy=U8, M=8, N=16, K=64, qpx=P, Cx=1, qpw=P, bias=None, qpy=P, Cy=1, relu=1, rw=None, splits=0, ws=P, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.cnnq_linear_codes_q_workspace(M, N, K, fx, fw, fy, splits)
    return lib.cnnq_linear_codes_q(xq, fx, wq, fw, y, fy, M, N, K, qpx, Cx, qpw, bias, qpy, Cy, relu, rw, splits, ws, ws_bytes, None)


SHARED = [(dict(fx=2), EINVAL), (dict(fw=-1), EINVAL), (dict(splits=65), EINVAL), (dict(xq=P + 2), EINVAL), (dict(wq=None), EINVAL),
          (dict(qpx=None), EINVAL), (dict(qpw=P + 1), EINVAL), (dict(ws=P + 8), EINVAL), (dict(ws_bytes=15), EINVAL), (dict(Cx=3), EINVAL),
          # the output's own
          (dict(fy=2), EINVAL), (dict(fy=-1), EINVAL), (dict(Cy=3), EINVAL), (dict(qpy=None), EINVAL), (dict(qpy=P + 2), EINVAL),
          (dict(y=None), EINVAL), (dict(y=P + 2), EINVAL)]


@pytest.mark.parametrize('kw,rc', SHARED + [
    (dict(C=18), EINVAL), (dict(C=16384), ERANGE), (dict(KH=11, ph=1), EINVAL), (dict(sh=0), EINVAL), (dict(taps=P + 2), EINVAL),
    (dict(Cout=18), EINVAL), (dict(Cout=20, fy=PACK4), EINVAL),                                   # rows of whole dwords of codes
], ids=str)
def test_conv_refused_before_the_device(kw, rc):
    from cnn_quantization_amd import _lib as L
    assert conv(L.load(), **kw) == rc


@pytest.mark.parametrize('kw,rc', SHARED + [
    (dict(K=66), EINVAL), (dict(K=68, fw=PACK4), EINVAL), (dict(K=131072), ERANGE), (dict(M=0), EINVAL), (dict(rw=P + 2), EINVAL),
    (dict(N=18), EINVAL), (dict(N=20, fy=PACK4), EINVAL),
], ids=str)
def test_linear_refused_before_the_device(kw, rc):
    from cnn_quantization_amd import _lib as L
    assert linear(L.load(), **kw) == rc


def test_workspace_is_the_fp32_entries():
    from cnn_quantization_amd import _lib as L
    lib = L.load()
    g = geometry(N=2, H=7, W=5, C=32, Cout=40, KH=3, KW=3, sh=2, sw=2, ph=1, pw=1)
    for fy in (U8, PACK4):
        for held in (0, 1):
            for s in (0, 1, 3):
                want = lib.cnnq_conv_codes_workspace(g, U8, PACK4, held, s)
                assert want > 0 and lib.cnnq_conv_codes_q_workspace(g, U8, PACK4, fy, held, s) == want
        for s in (0, 1, 3):
            want = lib.cnnq_linear_codes_workspace(130, 264, 320, PACK4, U8, s)
            assert want > 0 and lib.cnnq_linear_codes_q_workspace(130, 264, 320, PACK4, U8, fy, s) == want
    assert lib.cnnq_conv_codes_q_workspace(geometry(Cout=20), U8, U8, PACK4, 0, 0) == 0 and lib.cnnq_conv_codes_q_workspace(g, U8, U8, 2, 0, 0) == 0
    assert lib.cnnq_linear_codes_q_workspace(8, 18, 64, U8, U8, U8, 0) == 0 and lib.cnnq_linear_codes_q_workspace(8, 16, 64, U8, U8, 2, 0) == 0


def test_routes():
    """The fp32 route's words and one more: 16-byte stores of the codes where the output rows are whole 16-byte pieces on such a base."""
    from cnn_quantization_amd import _lib as L
    lib = L.load()
    res = geometry(N=64, H=56, W=56, C=64, Cout=64)                      # ResNet 3 x 3, batch 64
    fp32, out = (ctypes.c_int32 * 6)(), (ctypes.c_int32 * 7)()
    assert lib.cnnq_conv_codes_route(res, U8, U8, 0, 16, fp32) == 0
    for fy, align, wide in ((U8, 16, 1), (PACK4, 16, 1), (U8, 4, 0)):   # 64 u8 / 32 pack4 bytes per pixel
        assert lib.cnnq_conv_codes_q_route(res, U8, U8, fy, 0, align, out) == 0 and list(out) == list(fp32)[:3] + [int(align == 16)] + [56, 56, wide]
    assert lib.cnnq_conv_codes_q_route(geometry(N=64, H=56, W=56, C=64, Cout=40), U8, U8, PACK4, 0, 16, out) == 0 and out[6] == 0   # 20 bytes per pixel
    assert lib.cnnq_conv_codes_q_route(geometry(Cout=20), U8, U8, PACK4, 0, 16, out) == EINVAL
    fp32, out = (ctypes.c_int32 * 4)(), (ctypes.c_int32 * 5)()
    assert lib.cnnq_linear_codes_route(512, 1000, 2048, U8, U8, 0, 16, fp32) == 0       # the classifier, batch 512
    assert lib.cnnq_linear_codes_q_route(512, 1000, 2048, U8, U8, U8, 0, 16, out) == 0 and list(out) == list(fp32) + [0]    # 1000 % 16 != 0
    assert lib.cnnq_linear_codes_q_route(512, 1000, 2048, U8, U8, PACK4, 0, 16, out) == 0 and list(out) == list(fp32) + [0]
    assert lib.cnnq_linear_codes_q_route(512, 1024, 2048, U8, U8, PACK4, 0, 16, out) == 0 and out[4] == 1
    assert lib.cnnq_linear_codes_q_route(512, 1001, 2048, U8, U8, U8, 0, 16, out) == EINVAL
