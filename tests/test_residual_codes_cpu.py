"""cnnq_conv_codes_q_add's host side, no device: the refusals, cnnq_conv_codes_q's workspace, the route's word."""
import ctypes

import pytest

from test_conv_codes_cpu import EINVAL, P, PACK4, U8, geometry


def call(lib, y=P, fy=U8, rq=P + 64, fr=U8, qpr=P, Cr=1, Cx=1, splits=0, **geo):
    g = geometry(**geo)
    ws_bytes = lib.cnnq_conv_codes_q_add_workspace(g, U8, U8, fy, fr, 0, splits)
    return lib.cnnq_conv_codes_q_add(P, U8, P, U8, y, fy, g, P, Cx, P, None, P, 1, 1, rq, fr, qpr, Cr, None, splits, P, ws_bytes, None)


@pytest.mark.parametrize('kw', [
    dict(fr=2), dict(fr=-1), dict(Cout=20, fr=PACK4), dict(Cr=3), dict(N=4, Cr=2), dict(rq=None), dict(rq=P + 2), dict(qpr=None),
    dict(qpr=P + 2), dict(rq=P, fr=PACK4),                                                  # the output itself in another format
    dict(fy=2), dict(y=None), dict(splits=65), dict(C=18),                                  # what cnnq_conv_codes_q refuses
], ids=str)
def test_refused_before_the_device(kw):
    from cnn_quantization_amd import _lib as L
    assert call(L.load(), **kw) == EINVAL


def test_workspace_and_route():
    from cnn_quantization_amd import _lib as L
    lib = L.load()
    g = geometry(N=2, H=7, W=5, C=32, Cout=40, KH=3, KW=3, sh=2, sw=2, ph=1, pw=1)
    for fr in (U8, PACK4):
        for held, s in ((0, 0), (1, 1), (0, 3)):
            want = lib.cnnq_conv_codes_q_workspace(g, U8, PACK4, U8, held, s)
            assert want > 0 and lib.cnnq_conv_codes_q_add_workspace(g, U8, PACK4, U8, fr, held, s) == want
    assert lib.cnnq_conv_codes_q_add_workspace(geometry(Cout=20), U8, U8, U8, PACK4, 0, 0) == 0 and lib.cnnq_conv_codes_q_add_workspace(g, U8, U8, U8, 2, 0, 0) == 0
    res = geometry(N=64, H=56, W=56, C=64, Cout=256, KH=1, KW=1, ph=0, pw=0)                # ResNet-50's first block-closing layer
    q, out = (ctypes.c_int32 * 7)(), (ctypes.c_int32 * 8)()
    assert lib.cnnq_conv_codes_q_route(res, U8, U8, PACK4, 0, 16, q) == 0
    for fr, align, wide in ((U8, 16, 1), (PACK4, 16, 1), (U8, 4, 0)):
        assert lib.cnnq_conv_codes_q_add_route(res, U8, U8, PACK4, fr, 0, align, out) == 0 and list(out) == list(q)[:3] + [int(align == 16)] + list(q)[4:6] + [int(align == 16), wide]
    assert lib.cnnq_conv_codes_q_add_route(geometry(Cout=48), U8, U8, U8, PACK4, 0, 16, out) == 0 and out[6:8] == [1, 0]   # 48, 24 bytes per pixel
    assert lib.cnnq_conv_codes_q_add_route(geometry(Cout=48), U8, U8, PACK4, U8, 0, 16, out) == 0 and out[6:8] == [0, 1]
    assert lib.cnnq_conv_codes_q_add_route(geometry(Cout=20), U8, U8, U8, PACK4, 0, 16, out) == EINVAL
