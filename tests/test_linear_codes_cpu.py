"""The host side of cnnq_linear_codes without a device: what is refused before anything is enqueued, how the
workspace grows with the splits, and which tile and split the plan gives the classifier layers of VGG-16 and ResNet-50."""
import ctypes

import pytest

EINVAL, ERANGE = -1, -2
U8, PACK4 = 0, 1
P = 0x10000          # a well-aligned address that is never dereferenced: every call below is refused before a launch


def call(lib, xq=P, fx=U8, wq=P, fw=U8, y=P, M=16, N=16, K=64, qpx=P, Cx=1, qpw=P, bias=None, rw=None, splits=0, ws=P, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = lib.cnnq_linear_codes_workspace(M, N, K, fx, fw, splits)
    return lib.cnnq_linear_codes(xq, fx, wq, fw, y, M, N, K, qpx, Cx, qpw, bias, rw, splits, ws, ws_bytes, None)


@pytest.mark.parametrize('kw,rc', [
    (dict(fx=2), EINVAL), (dict(fw=-1), EINVAL),                            # a format outside cnnq_code_format
    (dict(K=66), EINVAL), (dict(K=68, fw=PACK4), EINVAL), (dict(K=68, fx=PACK4), EINVAL),   # K % 4, K % 8 with pack4
    (dict(K=131072), ERANGE), (dict(M=1 << 16, N=1 << 15), ERANGE),
    (dict(xq=P + 2), EINVAL), (dict(wq=P + 1), EINVAL), (dict(ws=P + 8), EINVAL), (dict(rw=P + 2), EINVAL),
    (dict(xq=None), EINVAL), (dict(wq=None), EINVAL), (dict(y=None), EINVAL), (dict(qpx=None), EINVAL), (dict(qpw=None), EINVAL),
    (dict(ws=None), EINVAL), (dict(ws_bytes=127), EINVAL), (dict(splits=2, ws_bytes=128), EINVAL),
    (dict(Cx=2), EINVAL), (dict(M=0), EINVAL), (dict(splits=65), EINVAL), (dict(splits=-1), EINVAL),
], ids=str)
def test_refused_before_the_device(kw, rc):
    from cnn_quantization_amd import _lib as L
    lib = L.load()
    assert call(lib, **kw) == rc
    geo = {k: kw[k] for k in ('M', 'N', 'K', 'fx', 'fw', 'splits') if k in kw}
    if geo and 'ws_bytes' not in kw:          # a refused geometry sizes no workspace and has no route
        g = dict(dict(M=16, N=16, K=64, fx=U8, fw=U8, splits=0), **geo)
        assert lib.cnnq_linear_codes_workspace(g['M'], g['N'], g['K'], g['fx'], g['fw'], g['splits']) == 0
        out = (ctypes.c_int32 * 4)()
        assert lib.cnnq_linear_codes_route(g['M'], g['N'], g['K'], g['fx'], g['fw'], g['splits'], 16, out) == rc
    assert lib.cnnq_linear_codes_rowsums(P, 2, 4, 64, P, None) == EINVAL and lib.cnnq_linear_codes_rowsums(P, PACK4, 4, 68, P, None) == EINVAL


def test_workspace_grows_with_the_splits():
    """int32 Rx[M] and Rw[N], each rounded up to 16 bytes, and - more than one split - splits int32 copies of y."""
    from cnn_quantization_amd import _lib as L
    lib = L.load()
    M, N, K = 33, 48, 1024
    base = 144 + 192
    assert lib.cnnq_linear_codes_workspace(M, N, K, U8, PACK4, 1) == base
    for s in (2, 3, 64):
        assert lib.cnnq_linear_codes_workspace(M, N, K, U8, PACK4, s) == base + 4 * s * M * N


@pytest.mark.parametrize('M,N,K,want', [
    (512, 4096, 25088, [128, 128, 2, 1]), (512, 4096, 4096, [128, 128, 2, 1]), (512, 1000, 4096, [64, 64, 2, 1]),   # VGG-16
    (512, 1000, 2048, [64, 64, 2, 1]),                                                                          # ResNet-50
    (1, 4096, 25088, [16, 128, 32, 1]), (1, 1000, 2048, [16, 128, 8, 1]),                                          # batch 1
])
def test_route_of_the_classifier_layers(M, N, K, want):
    from cnn_quantization_amd import _lib as L
    lib = L.load()
    out = (ctypes.c_int32 * 4)()
    for fmt in (U8, PACK4):
        assert lib.cnnq_linear_codes_route(M, N, K, fmt, fmt, 0, 16, out) == 0 and list(out) == want
        assert lib.cnnq_linear_codes_workspace(M, N, K, fmt, fmt, 0) == lib.cnnq_linear_codes_workspace(M, N, K, fmt, fmt, want[2])
    assert lib.cnnq_linear_codes_route(M, N, K, U8, U8, 0, 4, out) == 0 and out[3] == 0      # bases of 4 bytes: the dword path
