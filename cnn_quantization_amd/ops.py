"""Tensor-level wrappers over the C ABI (include/cnnq_hip.h): device pointers, sizes and the
current HIP stream go straight to libcnnq_hip.so.  torch supplies memory and streams only.

No function here synchronises with the host; none has a CPU path - CPU tensors are rejected
and a missing library raises (cnn_quantization_amd._lib.load)."""
import ctypes
import os

import torch

from . import _lib as L
from . import distributed as D


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


# the raw handle of the current stream of a device: torch keeps a direct accessor (the one its own compiled code
# uses); torch.cuda.current_stream() builds a Stream object per call, ~1.5 us, three times per hot call before
_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None) or (
    lambda index: torch.cuda.current_stream(index).cuda_stream)


def _stream(t):
    return ctypes.c_void_p(_raw_stream(t.device.index))


def _dev(x, what='tensor', dtypes=(torch.float32,), keep_nhwc=False):
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise L.CnnqError('%s must be a CUDA/HIP tensor (there is no CPU path)' % what)
    if x.dtype not in dtypes:
        raise L.CnnqError('%s must be %s, got %s' % (what, ' or '.join(str(d).replace('torch.', '') for d in dtypes), x.dtype))
    if x.device.index != torch.cuda.current_device():
        # kernels are enqueued in the calling thread's current device context (one process per GPU is the
        # deployment model; in-process multi-GPU callers must enter torch.cuda.device(x.device) first)
        raise L.CnnqError('%s is on %s but the current device is cuda:%d' % (what, x.device, torch.cuda.current_device()))
    if x.requires_grad:
        x = x.detach()
    if x.is_contiguous():
        return x
    if _layout(x) == 'nhwc':
        if keep_nhwc and _NHWC:
            return x
        global LAYOUT_COPIES
        LAYOUT_COPIES += 1
    return x.contiguous()


# dense channels_last activations: configs 1 and 2 run on the storage as it is and return a result of the
# input's layout.  Every copy _dev makes of such a tensor is counted here, so that tests can prove those paths never copy.
LAYOUT_COPIES = 0


def _layout(x):
    """'nchw': dense in the default layout (also every tensor dense in both, C == 1 or H*W == 1); 'nhwc': a dense channels_last
    4-D tensor that is not; 'copy': anything else.  Shape and strides only, so CPU tensors work too."""
    if x.is_contiguous():
        return 'nchw'
    if x.dim() == 4 and x.is_contiguous(memory_format=torch.channels_last):
        return 'nhwc'
    return 'copy'


def _is_nhwc(x):
    """A tensor _dev_act_layout let through is either contiguous or dense channels_last."""
    return not x.is_contiguous()


def _sharded(group):
    """x is this rank's shard of the batch (a 1-rank group too under CNNQ_FORCE_EXCHANGE=1, which times the exchange on one GPU)."""
    return group is not False and (D.world_size(group) > 1 or D.forced_exchange())


# activations of another element type (include/cnnq_hip.h, cnnq_dtype): the entry points of configs 1 and 2 that take them
_HALF_DTYPES = {torch.bfloat16: L.DTYPE_BF16, torch.float16: L.DTYPE_F16}
_DTYPE_CODES = {torch.float32: L.DTYPE_F32, **_HALF_DTYPES}
_ACT_DTYPES = (torch.float32, torch.bfloat16, torch.float16)


def _dev_act(x, what='tensor'):
    """_dev for the activation paths that have bf16 / fp16 kernels."""
    return _dev(x, what, _ACT_DTYPES)


def _dev_act_layout(x, what='tensor'):
    """_dev_act for the paths that have channels_last kernels: a dense channels_last tensor passes as it is (CNNQ_NHWC=0: copied)."""
    return _dev(x, what, _ACT_DTYPES, keep_nhwc=True)


def _half_only(what, reason):
    """The error of a half-precision call that has no native kernel: the caller upcasts (qtypes/int_quantizer.py)."""
    raise L.CnnqError('%s: no bfloat16 / float16 kernel for %s (compute on x.float())' % (what, reason))


# switches, read ONCE at import (not per hot call); reload_switches() re-reads them after the environment changed (tests, tools)
def reload_switches():
    global _RESIDENT, _SINGLE_CODES, _DIRECT_RCCL, _PT_FUSED, _XRANK_ON, _ACIQ_SINGLE, _NHWC, _HALF_TABLE, _HALF_ACIQ, _HALF_MIDTREAD, _HALF_ENTROPY
    global _SBA_NATIVE
    _SBA_NATIVE = os.environ.get('CNNQ_SBA_NATIVE', '1') != '0'        # 0: -sm collect -sba per channel takes the former route, upcast and copy (A/B)
    _HALF_ENTROPY = os.environ.get('CNNQ_HALF_ENTROPY', '1') != '0'    # 0: -me on contiguous half activations takes the upcast route (A/B)
    _HALF_MIDTREAD = os.environ.get('CNNQ_HALF_MIDTREAD', '1') != '0'  # 0: mid-tread on contiguous half activations takes the upcast route (A/B)
    _HALF_ACIQ = os.environ.get('CNNQ_HALF_ACIQ', '1') != '0'          # 0: dynamic ACIQ on contiguous half activations takes the upcast route (A/B)
    _HALF_TABLE = os.environ.get('CNNQ_HALF_TABLE', '1') != '0'        # 0: calibrated per-channel half activations take the upcast route (A/B)
    _NHWC = os.environ.get('CNNQ_NHWC', '1') != '0'                    # 0: channels_last tensors take the NCHW copy route (A/B)
    _ACIQ_SINGLE = os.environ.get('CNNQ_ACIQ_SINGLE', '1') != '0'      # 0: the ACIQ path always takes the five-launch chain (A/B)
    _XRANK_ON = D.xrank_mode() != '0'                                  # opt-in (CNNQ_XRANK=1 / auto, D.set_xrank_mode): sharded config 2 exchanges INSIDE the single launch
    _PT_FUSED = os.environ.get('CNNQ_PT_FUSED', '0') == '1'           # 1: config 1 in one launch (slower: see ops.minmax_qdq_per_tensor)
    _RESIDENT = os.environ.get('CNNQ_RESIDENT', '1') != '0'            # 0: never take a single-launch kernel
    _SINGLE_CODES = os.environ.get('CNNQ_SINGLE_CODES', '1') != '0'    # 0: codes / entropy requests take the chain
    _DIRECT_RCCL = os.environ.get('CNNQ_DIRECT_RCCL', '1')
    _XPLAN.clear()


_XPLAN = {}     # per (group, device, stream, geometry): what the multi-GPU hot call needs, looked up once
reload_switches()

_SCRATCH = {}
_WS_BYTES = {}


def release_plans():
    """Drop the cached multi-GPU exchange plans (they hold process groups and direct RCCL communicators): called by
    rccl.close_all(), so that no plan outlives its communicator."""
    _XPLAN.clear()


def release_workspaces():
    """Give back every cached buffer: scratch tensors, the replica histograms and the fine-grained exchange
    workspaces of all streams (cnnq_group_ws_free).  Synchronises the device first; later calls re-allocate."""
    torch.cuda.synchronize()
    release_plans()
    _SCRATCH.clear()
    _HIST_REP.clear()
    _ENT_TABLES.clear()
    lib = L.load()
    for ws in list(_GROUP_WS.values()) + [w for pool in _GROUP_POOL.values() for w in pool]:
        lib.cnnq_group_ws_free(ws)
    _GROUP_WS.clear()
    _GROUP_POOL.clear()


def _scratch(x, tag, nbytes, st=None):
    """A per-(device, stream, tag) scratch buffer (uint8, at least nbytes), grown on demand and never returned
    to callers: launches on one stream are ordered, so consecutive calls may share it.  Saves the 2-4
    torch.empty calls (8-15 us of host time) the small layers would otherwise pay per call."""
    key = (x.device.index, _raw_stream(x.device.index) if st is None else st, tag)
    buf = _SCRATCH.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=x.device)
        # inside a stream capture the buffer comes from the graph's private pool: hand it out WITHOUT caching it (a cached
        # one would later serve eager calls from memory that belongs to the graph); the pool keeps the block for the
        # graph's replays and reuses it in capture order
        if not torch.cuda.is_current_stream_capturing():
            _SCRATCH[key] = buf
    return buf


def _out_like(x, out):
    """The result buffer: a new tensor like x, or the caller's - which must match x exactly."""
    if out is None:
        return torch.empty_like(x)          # a dense channels_last x: a channels_last y (preserve_format)
    if not (isinstance(out, torch.Tensor) and out.is_cuda and out.dtype == x.dtype and out.shape == x.shape
            and out.device == x.device and (out.is_contiguous() if x.is_contiguous() else _layout(out) == 'nhwc')):
        raise L.CnnqError('out must be a %s %s tensor on %s shaped like the input'
                          % ('contiguous' if x.is_contiguous() else 'dense channels_last', str(x.dtype).replace('torch.', ''),
                             x.device))
    nbytes = x.numel() * x.element_size()
    if out.data_ptr() < x.data_ptr() + nbytes and x.data_ptr() < out.data_ptr() + nbytes:
        # the kernels declare x and y __restrict__, and a single-launch workgroup whose bounded wait expires recomputes
        # its channels' extrema by re-reading x after other members may have stored y (include/cnnq_hip.h: x != y).
        # Byte ranges, not storages: two views of one arena that do not overlap are fine.
        raise L.CnnqError('out must not overlap the input (in-place quantization is not supported)')
    return out


def geometry(x, per_channel_dim=1):
    """(N, C, HW) of a tensor addressed as x[N][C][HW].  4-D activations: channel dim 1.
    per_channel_dim=0 (weights [OFM, ...], iq.py:455): N = 1, C = OFM."""
    if per_channel_dim == 0:
        return 1, x.shape[0], x.numel() // x.shape[0]
    n, c = x.shape[0], x.shape[1]
    return n, c, x.numel() // (n * c)


# ------------------------------------------------------------------------------------- launch plumbing
def _supported(rc, what):
    """False on CNNQ_ENOTSUP (no single-launch kernel for this shape: the caller takes another route); other errors raise."""
    if rc != L.ENOTSUP:
        L.check(rc, what)
    return rc != L.ENOTSUP


def _gws_args(gws):
    return gws, (GROUP_WS_BYTES if gws is not None else 0)


def _groups(N, C, HW, aligned=None):
    """The chain's partial-record count for x's alignment, or (None) the larger of both, so that G records serve either."""
    lib = L.load()
    if aligned is None:
        G = max(lib.cnnq_pc_groups(N, C, HW, 1), lib.cnnq_pc_groups(N, C, HW, 0))
    else:
        G = lib.cnnq_pc_groups(N, C, HW, int(aligned))
    if G <= 0:
        L.check(G, 'cnnq_pc_groups(%d,%d,%d)' % (N, C, HW))
    return G


_WS_FN = {  # kind: (workspace function of a storage form's one-call entry points, geometry words it takes in front of the dtype code)
    'pt_clip': ('cnnq_pt_clip_workspace', 1), 'rows': ('cnnq_rows_stats_workspace', 2),
    'nhwc': ('cnnq_pc_nhwc_workspace', 2), 'aciq_nhwc': ('cnnq_pc_aciq_nhwc_workspace', 2),
    'bcorr_nhwc': ('cnnq_pc_qdq_bcorr_nhwc_workspace', 2), 'stats_nhwc': ('cnnq_pc_stats_nhwc_workspace', 2),
    'stats_half': ('cnnq_pc_stats_dt_workspace', 3), 'bcorr_half': ('cnnq_pc_qdq_bcorr_dt_workspace', 3),
    'aciq_half': ('cnnq_pc_aciq_dt_workspace', 3), 'midtread_half': ('cnnq_pc_midtread_dt_workspace', 3)}


def _ws_bytes(kind, N, C, HW, arg=0):
    """Workspace bytes of a one-call entry point, asked once and rounded up to 16 so that tables may follow in one scratch buffer.
    arg: x is 16-byte aligned ('stats', 'aciq'), else the dtype code - of the kinds of _WS_FN, which take the first 1 (N = elements),
    2 (N = rows, C = their length or the channels) or 3 (N, C, HW) of the geometry words.  0 from the library: no plan for the
    geometry."""
    key = (kind, N, C, HW, arg)
    nbytes = _WS_BYTES.get(key)
    if nbytes is None:
        lib = L.load()
        if kind in _WS_FN:
            fn, words = _WS_FN[kind]
            args = (N, C, HW)[:words] + (arg,)
            nbytes = getattr(lib, fn)(*args)
            if nbytes == 0 and words < 3:
                raise L.CnnqError('%s(%s): bad arguments' % (fn, ', '.join('%d' % a for a in args)))
            if nbytes == 0:
                L.check(min(lib.cnnq_pc_groups(N, C, HW, 0), -1), '%s(%d,%d,%d,%d)' % ((fn,) + args))
        elif kind == 'aciq':
            nbytes = lib.cnnq_pc_aciq_workspace(N, C, HW, arg)
        else:
            nbytes = lib.cnnq_pc_minmax_qdq_workspace(N, C, HW) if kind == 'cfg2' else lib.cnnq_pc_stats_workspace(N, C, HW, arg)
            if nbytes == 0:
                L.check(min(lib.cnnq_pc_groups(N, C, HW, 1), -1), 'cnnq_pc_groups(%d,%d,%d)' % (N, C, HW))
        nbytes = _WS_BYTES[key] = (nbytes + 15) // 16 * 16
    return nbytes


def _result(y, codes=None, entropy=None, parts=None):
    res = tuple(v for v in (y, codes, entropy, parts) if v is not None)
    return res if len(res) > 1 else y


def _mt_result(y, entropy, codes=None, parts=None):
    return (y, entropy) + tuple(v for v in (codes, parts) if v is not None)


def _minmax_parts(mm, qp, g=None):
    """Config 2's parts from the {min, max} rows mm, or (the chain) from the first g records of the partial extrema mm."""
    if g is not None:
        mm = (mm[:g, 0].min(dim=0)[0], mm[:g, 1].max(dim=0)[0])
    stats = torch.zeros((L.NSTAT, qp.shape[1]), dtype=torch.float32, device=qp.device)
    stats[L.STAT_MIN] = mm[0]
    stats[L.STAT_MAX] = mm[1]
    return dict(stats=stats, qp=qp, diag=None)


# ------------------------------------------------------------------------------------- statistics
def pc_moments(x, N, C, HW, want_relu=False):
    """Pass A partial records [G, NMOM, C] (float64)."""
    lib = L.load()
    G = _groups(N, C, HW, x.data_ptr() % 16 == 0)
    part = torch.empty((G, L.NMOM, C), dtype=torch.float64, device=x.device)
    L.check(lib.cnnq_pc_moments(_ptr(x), N, C, HW, int(want_relu), _ptr(part), _stream(x)), 'cnnq_pc_moments')
    return part


def pc_combine(part, has_relu=False, stats=None, want_mom=True):
    """Merge [G, NMOM, C] records -> (mom [NMOM, C] f64, stats [NSTAT, C] f32)."""
    lib = L.load()
    G, _, C = part.shape
    mom = torch.empty((L.NMOM, C), dtype=torch.float64, device=part.device) if want_mom else None
    if stats is None:
        stats = torch.zeros((L.NSTAT, C), dtype=torch.float32, device=part.device)
    L.check(lib.cnnq_pc_combine(_ptr(part), G, C, int(has_relu), _ptr(mom), _ptr(stats), _stream(part)),
            'cnnq_pc_combine')
    return mom, stats


def pc_absdev(x, N, C, HW, stats, want_kurt=False):
    lib = L.load()
    G = _groups(N, C, HW, x.data_ptr() % 16 == 0)
    part2 = torch.empty((G, L.NDEV, C), dtype=torch.float64, device=x.device)
    L.check(lib.cnnq_pc_absdev(_ptr(x), N, C, HW, _ptr(stats), int(want_kurt), _ptr(part2), _stream(x)),
            'cnnq_pc_absdev')
    return part2


def pc_combine_dev(part2, mom, stats=None, want_kurt=False, want_sums=False):
    lib = L.load()
    G, _, C = part2.shape
    dev = torch.empty((L.NDEV, C), dtype=torch.float64, device=part2.device) if want_sums else None
    L.check(lib.cnnq_pc_combine_dev(_ptr(part2), G, C, _ptr(mom), int(want_kurt), _ptr(dev), _ptr(stats),
                                    _stream(part2)), 'cnnq_pc_combine_dev')
    return dev


def pc_stats(x, N, C, HW, need_b=False, need_kurt=False, need_relu=False, group=None, local_only=False):
    """Per-channel statistics table [NSTAT, C] of x[N][C][HW] (rows MIN, MAX, MEAN, STD always;
    B / KURT / STD_POS on request) plus the merged moment record [NMOM, C].

    With a process group of world size > 1 the tensor is this rank's batch shard: the fp64
    moment records are all-gathered (<= 7*C*8 bytes per rank, latency-bound on xGMI) and merged
    in rank order on every rank, so all ranks hold the statistics of the GLOBAL batch."""
    x = _dev(x, 'x')
    sharded = not local_only and _sharded(group)
    if sharded and _ACIQ_SINGLE and _RESIDENT:
        # the batch is sharded and the group has a (verified) in-launch exchange: the table of the GLOBAL batch from one read of
        # this rank's shard (cnnq_pc_stats_xrank; round 6) - every rank takes this route or none does
        res = _pc_stats_xrank(x, N, C, HW, need_b, need_kurt, need_relu, group)
        if res is not None:
            return res
    if not sharded:
        # one C call, one cached workspace (cnnq_pc_stats_auto)
        lib = L.load()
        nbytes = _ws_bytes('stats', N, C, HW, int(x.data_ptr() % 16 == 0))
        stats = torch.empty((L.NSTAT, C), dtype=torch.float32, device=x.device)
        mom = torch.empty((L.NMOM, C), dtype=torch.float64, device=x.device)
        st = _raw_stream(x.device.index)
        gws = _group_workspace(x, st) if (_ACIQ_SINGLE and _RESIDENT) else None
        # one launch that reads x once where the shape has a flat plan (cnnq_pc_stats_single), else the three-launch chain
        L.check(lib.cnnq_pc_stats_auto(_ptr(x), N, C, HW, int(bool(need_b)), int(bool(need_kurt)), int(bool(need_relu)),
                                       _ptr(_scratch(x, 'stats', nbytes, st)), *_gws_args(gws), _ptr(mom), _ptr(stats), st),
                'cnnq_pc_stats')
        return stats, mom
    # the collective route (ranks sharing a GPU, CNNQ_XRANK=0, after a recovery; also a 1-rank group under CNNQ_FORCE_EXCHANGE=1,
    # which times the real collectives on one GPU): the chain's passes with an all_gather of the fp64 records behind each
    mom_local, _ = pc_combine(pc_moments(x, N, C, HW, need_relu), need_relu)
    mom, stats = pc_combine(D.all_gather_records(mom_local, group), need_relu)
    if need_b or need_kurt:
        dev_local = pc_combine_dev(pc_absdev(x, N, C, HW, stats, need_kurt), mom, None, need_kurt, want_sums=True)
        pc_combine_dev(D.all_gather_records(dev_local, group), mom, stats, need_kurt)
    return stats, mom


# ------------------------------------------------------------------------------------- the native front
# what the entry points on the two native storage forms - dense channels_last (*_nhwc) and contiguous
# bf16 / fp16 (*_half) - share on the host.  An admission (_admit_nhwc, _admit_half) hands back a site:
#     (layout, geo, C, dtype code, raw stream)
# geo, the geometry words the layout's C calls take, is splatted into them: (R, C) or (N, C, HW).  layout is one of the two
# tables below: what differs between the storage forms, written once.  Every operation is one body of (site, its own arguments)
# - _pc_stats_native, _aciq_qdq_native, _qdq_bias_corrected_native, _mid_tread_qdq_native, _qdq_native - behind two public
# wrappers that keep what is their layout's own: the argument checks, the fallback of a channels_last tensor that does not run
# native, single_launch, and where the counting pass of a want_entropy call counts (_nhwc_hist_slot may send the tensor to the
# copy route, _half_hist_slot raises).  One Python call more per entry than a body written into its wrapper, and no more: the
# bodies keep their pointer arithmetic inline, a helper per call costs more host time than it saves lines
# (profiles/host_overhead_nhwc.md, profiles/host_overhead_native.md).
# The config-2 pair stays apart (_minmax_qdq_nhwc against _minmax_qdq_half / _minmax_qdq_half_entropy): their workspaces are
# laid out differently, and the half one runs the C code float32 runs.
_NHWC_LAYOUT = {    # operation: (C function [, its counting or table-driven form], the _ws_bytes / _scratch kind)
    'stats': ('cnnq_pc_stats_nhwc', 'stats_nhwc'),
    'aciq': ('cnnq_pc_aciq_qdq_nhwc', 'cnnq_pc_aciq_qdq_hist_nhwc', 'aciq_nhwc'),
    'bcorr': ('cnnq_pc_qdq_bcorr_nhwc', 'bcorr_nhwc'),
    'midtread': ('cnnq_pc_midtread_nhwc', 'cnnq_pc_midtread_qdq_nhwc', 'aciq_nhwc'),
    'qdq': ('cnnq_pc_qdq_nhwc', (), 'cnnq_pc_qdq_hist_nhwc'),       # (the words between qp and the stream of the plain form)
    'ws_pad': (1,),     # _ws_bytes is keyed by (N, C, HW): the HW of the kinds that take rows
    'single': False}    # whether the calls of 'aciq', 'bcorr' and 'midtread' end in an allow_single_launch word
_HALF_LAYOUT = {
    'stats': ('cnnq_pc_stats_dt', 'stats_half'),
    'aciq': ('cnnq_pc_aciq_qdq_dt', 'cnnq_pc_aciq_qdq_hist_dt', 'aciq_half'),
    'bcorr': ('cnnq_pc_qdq_bcorr_dt', 'bcorr_half'),
    'midtread': ('cnnq_pc_midtread_dt', 'cnnq_pc_midtread_qdq_dt', 'midtread_half'),
    'qdq': ('cnnq_pc_qdq_dt', (None, None, 0), 'cnnq_pc_qdq_hist_dt'),
    'ws_pad': (),
    'single': True}


def _route_word(cache, key, cast, fn, geo, dtype, extra=(), words=4, word=3):
    """cast(word `word` of the `words` the route function `fn` reports) for a class of layer - a function of its geometry words geo
    and the dtype alone - asked once per `key` with alignment 16 (extra: fn's arguments behind align_bytes) and kept in `cache`."""
    v = cache.get(key)
    if v is None:
        out = (ctypes.c_int32 * words)()
        L.check(getattr(L.load(), fn)(*geo, _DTYPE_CODES.get(dtype, -1), 16, *extra, out), fn)
        v = cache[key] = cast(out[word])
    return v


_NHWC_ROUTES = {    # kind: (route function, its arguments behind align_bytes, words of out, the word that says "native")
    'stats': ('cnnq_pc_route_stats_nhwc', (), 4, 3),
    'hist': ('cnnq_pc_route_qdq_hist_nhwc', (256,), 4, 3),
    'midtread': ('cnnq_pc_route_midtread_nhwc', (0,), 6, 5)}
_NHWC_NATIVE = {}


def _nhwc_native(kind, R, C, dtype):
    """Whether this class of layer runs on the channels_last kernels of `kind`: the "native" word of its route function's report
    (0: a class that measured slower native than copied is sent back to the copy route there; a function of R, C and the dtype
    alone), asked once per (kind, R, C, dtype).  'stats' is kept under its own name: _stats_nhwc_native.  (On the hot path of
    _admit_nhwc: a class that has asked costs no further call.)"""
    if kind == 'stats':
        return _stats_nhwc_native(R, C, dtype)
    v = _NHWC_NATIVE.get((kind, R, C, dtype))
    return v if v is not None else _route_word(_NHWC_NATIVE, (kind, R, C, dtype), bool, _NHWC_ROUTES[kind][0], (R, C), dtype,
                                               *_NHWC_ROUTES[kind][1:])


_STATS_NHWC_NATIVE = {}


def _stats_nhwc_native(R, C, dtype):
    """The 'stats' answer under the name, and with the cache, that the statistics manager (collects_native_nhwc) and the tests
    of the collect family use: they patch the function and empty the cache by name."""
    v = _STATS_NHWC_NATIVE.get((R, C, dtype))
    return v if v is not None else _route_word(_STATS_NHWC_NATIVE, (R, C, dtype), bool, _NHWC_ROUTES['stats'][0], (R, C), dtype)


def _admit_nhwc(x, what, route=None, half_reason=None, dev_first=False):
    """(x, site) - x as a channels_last entry point takes it, and its site, geo = (R = N*H*W, C), when x runs native: a dense
    channels_last 4-D CUDA tensor of fp32 / bf16 / fp16 with CNNQ_NHWC on and - route - a class of layer the route function keeps.
    Otherwise the site is None and x the contiguous copy _dev makes and counts, for the caller's fallback.  Two orders, chosen by
    the caller:
      dev_first=False: the 4-D check, the decision, then - half_reason: the fallback is float32 only - the error of a half tensor
        before anything is copied or counted, then _dev;
      dev_first=True: _dev's checks and its copy, then the 4-D check; no route, no half error (the caller raises its own)."""
    if dev_first:
        x = _dev(x, 'x', _ACT_DTYPES, keep_nhwc=True)
        if x.dim() != 4:
            _not_4d(x, what)
        native = not x.is_contiguous()
    else:
        tensor = isinstance(x, torch.Tensor)
        if tensor and x.dim() != 4:
            _not_4d(x, what)
        native = (tensor and x.is_cuda and _NHWC and _layout(x) == 'nhwc' and x.dtype in _ACT_DTYPES
                  and (route is None or _nhwc_native(route, x.numel() // x.shape[1], x.shape[1], x.dtype)))
        if not native and half_reason is not None and tensor and x.dtype in _HALF_DTYPES:
            _half_only(what, half_reason)
        x = _dev(x, 'x', _ACT_DTYPES, keep_nhwc=native)
    if not native:
        return x, None
    C = x.shape[1]
    return x, (_NHWC_LAYOUT, (x.numel() // C, C), C, _DTYPE_CODES[x.dtype], _raw_stream(x.device.index))


def _not_4d(x, what):
    raise L.CnnqError('%s: x must be a 4-D activation, got %d dimensions' % (what, x.dim()))


def _is_table(t, dtype, shape, device):
    """A contiguous `dtype` table of `shape` on `device`: what the C side reads through a bare pointer."""
    return (isinstance(t, torch.Tensor) and t.is_cuda and t.device == device and t.dtype == dtype and t.is_contiguous()
            and tuple(t.shape) == tuple(shape))


def _pc_stats_native(site, x, need_b, need_kurt, need_relu):
    """The -sm collect table of a tensor on its site in one host call with one cached workspace (cnnq_pc_stats_nhwc /
    cnnq_pc_stats_dt): pass A, the merge, pass B when b or the kurtosis is asked for, its merge.  (stats [NSTAT, C] f32, mom
    [NMOM, C] f64) as pc_stats; rows nobody asked for are zero (B comes with pass B: need_b or need_kurt, as in pc_stats).  One
    GPU: the statistics are this tensor's."""
    layout, geo, C, dt, st = site
    fn, kind = layout['stats']
    stats = torch.empty((L.NSTAT, C), dtype=torch.float32, device=x.device)
    mom = torch.empty((L.NMOM, C), dtype=torch.float64, device=x.device)
    ws = _scratch(x, kind, _ws_bytes(kind, *geo, *layout['ws_pad'], dt), st)
    rc = getattr(L.load(), fn)(x.data_ptr(), dt, *geo, int(bool(need_b)), int(bool(need_kurt)), int(bool(need_relu)),
                               ws.data_ptr(), mom.data_ptr(), stats.data_ptr(), st)
    if rc:
        L.check(rc, fn)
    return stats, mom


def pc_stats_nhwc(x, need_b=False, need_kurt=False, need_relu=False):
    """pc_stats of a dense channels_last activation of fp32 / bf16 / fp16, on the storage as it is (-sm
    collect, smpc.py:45-79): _pc_stats_native over slabs of rows, 8 B/elem in fp32 and 4 in bf16 / fp16 for the full table.  A
    tensor that is not dense channels_last (or CNNQ_NHWC=0, or a class of layer the route function sends back: copied, counted)
    takes pc_stats, which is float32 only - a half tensor raises before anything is copied."""
    x, site = _admit_nhwc(x, 'pc_stats_nhwc', 'stats', 'the statistics of a tensor that does not take the channels_last kernels')
    if site is None:
        N, C, HW = geometry(x)
        return pc_stats(x, N, C, HW, need_b, need_kurt, need_relu, group=False)
    return _pc_stats_native(site, x, need_b, need_kurt, need_relu)


def _admit_half(x, what, f32_name):
    """(x, site) of a non-empty contiguous 4-D bf16 / fp16 tensor on the current device, as the *_half entry points take it, geo =
    (N, C, HW); anything else raises (f32_name: the function float32 takes): nothing is copied or upcast, so there is no fallback
    and the site is never None."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise L.CnnqError('%s: x must be a CUDA/HIP tensor (there is no CPU path)' % what)
    if x.dtype not in _HALF_DTYPES:
        raise L.CnnqError('%s: x must be bfloat16 or float16, got %s (float32 takes %s)' % (what, x.dtype, f32_name))
    if x.dim() != 4:
        _not_4d(x, what)
    if not x.is_contiguous() or x.numel() == 0:
        raise L.CnnqError('%s: x must be a non-empty contiguous tensor (no copy is made here)' % what)
    if x.device.index != torch.cuda.current_device():
        raise L.CnnqError('%s: x is on %s but the current device is cuda:%d' % (what, x.device, torch.cuda.current_device()))
    if x.requires_grad:
        x = x.detach()
    N, C, HW = geometry(x)
    return x, (_HALF_LAYOUT, (N, C, HW), C, _HALF_DTYPES[x.dtype], _raw_stream(x.device.index))


_STATS_HALF_NATIVE = {}


def _stats_half_native(N, C, HW, dtype):
    """Whether this class of layer collects its statistics on the contiguous bf16 / fp16 kernels: the "native" word of
    cnnq_pc_route_stats_dt's report (0: a class that measured slower native than through the upcast is sent back there).  The
    statistics manager (collects_native_half) and the tests patch the function and empty the cache by name."""
    return _route_word(_STATS_HALF_NATIVE, (N, C, HW, dtype), bool, 'cnnq_pc_route_stats_dt', (N, C, HW), dtype)


def pc_stats_half(x, need_b=False, need_kurt=False, need_relu=False):
    """pc_stats of a contiguous 4-D bf16 / fp16 activation, on the storage as it is (-sm collect,
    smpc.py:45-79): _pc_stats_native over (channel, batch split) workgroups, 4 B/elem for the full table.  Anything else - a CPU
    tensor, float32, not 4-D, not contiguous - raises: nothing is copied or upcast here."""
    x, site = _admit_half(x, 'pc_stats_half', 'pc_stats')
    return _pc_stats_native(site, x, need_b, need_kurt, need_relu)


_SAMPLE_EXTREMA_HALF_NATIVE = {}
_SAMPLE_EXTREMA_NHWC_NATIVE = {}


def _sample_extrema_half_native(N, C, HW, dtype):
    """Whether this class of layer takes its per-sample extrema (-sba) on the contiguous bf16 / fp16 kernel: the "native" word of
    cnnq_pc_route_sample_extrema_dt's report (0: a class that did not measure faster than the former route is sent back there).
    The statistics manager (collect_route with native_batch_avg) and the tests patch the function and empty the cache by name."""
    return _route_word(_SAMPLE_EXTREMA_HALF_NATIVE, (N, C, HW, dtype), bool, 'cnnq_pc_route_sample_extrema_dt', (N, C, HW), dtype)


def _sample_extrema_nhwc_native(N, HW, C, dtype):
    """The same for the channels_last kernel: the "native" word of cnnq_pc_route_sample_extrema_nhwc's report."""
    return _route_word(_SAMPLE_EXTREMA_NHWC_NATIVE, (N, HW, C, dtype), bool, 'cnnq_pc_route_sample_extrema_nhwc', (N, HW, C), dtype)


def pc_sample_extrema_half(x):
    """The per-sample channel extrema of a contiguous 4-D bf16 / fp16 activation, on the storage as it lies (DESIGN.md section 33;
    -sm collect -sba, smpc.py:72-78; cnnq_pc_sample_extrema_dt): the float32 device table [2, N * C], sample-major, row STAT_MIN the
    minima and row STAT_MAX the maxima of x.float() - what tensor_row_stats returns and statistic_manager.batch_extrema_sums
    reads.  One read of x, 2 B/elem, one launch, no workspace.  Anything else - a CPU tensor, float32, not 4-D, not contiguous -
    raises: nothing is copied or upcast here."""
    x, (_, geo, C, dt, st) = _admit_half(x, 'pc_sample_extrema_half', 'tensor_row_stats')
    ext = torch.empty((2, geo[0] * C), dtype=torch.float32, device=x.device)
    rc = L.load().cnnq_pc_sample_extrema_dt(x.data_ptr(), dt, *geo, ext.data_ptr(), st)
    if rc:
        L.check(rc, 'cnnq_pc_sample_extrema_dt')
    return ext


def pc_sample_extrema_nhwc(x):
    """The per-sample channel extrema of a dense channels_last activation of fp32 / bf16 / fp16, on the storage as it lies
    (-sm collect -sba, smpc.py:72-78; cnnq_pc_sample_extrema_nhwc): the float32 device table [2, N * C] of
    pc_sample_extrema_half.  One read of x, 4 B/elem in fp32 and 2 in bf16 / fp16; one launch, or - small batches of large images
    - two with a cached workspace of partial pairs.  A tensor that is not dense channels_last (or CNNQ_NHWC=0: copied, counted)
    takes tensor_row_stats on its (n, c) rows, which is float32 only here - a half tensor raises before anything is copied."""
    x, site = _admit_nhwc(x, 'pc_sample_extrema_nhwc', None, 'the per-sample extrema of a tensor that does not take the channels_last kernels')
    N, C = x.shape[0], x.shape[1]
    if site is None:
        return tensor_row_stats(x, N * C)
    _, (R, _), _, dt, st = site
    HW = R // N
    lib = L.load()
    key = ('sample_extrema_nhwc', N, HW, C, dt)
    nbytes = _WS_BYTES.get(key)
    if nbytes is None:
        out = (ctypes.c_int32 * 4)()
        L.check(lib.cnnq_pc_route_sample_extrema_nhwc(N, HW, C, dt, 16, out), 'cnnq_pc_route_sample_extrema_nhwc')   # (0 bytes is a plan too)
        nbytes = _WS_BYTES[key] = lib.cnnq_pc_sample_extrema_nhwc_workspace(N, HW, C, dt)
    ws = _scratch(x, 'sample_extrema', nbytes, st).data_ptr() if nbytes else None
    ext = torch.empty((2, N * C), dtype=torch.float32, device=x.device)
    rc = lib.cnnq_pc_sample_extrema_nhwc(x.data_ptr(), dt, N, HW, C, ws, ext.data_ptr(), st)
    if rc:
        L.check(rc, 'cnnq_pc_sample_extrema_nhwc')
    return ext


def _xrank_plan(kind, x, N, C, HW, group, xr=None):
    """(exchange, group, scratch, group workspace arguments, stream) of the sharded one-call routes, looked up once; None: the group has no
    (verified) in-launch exchange whose windows fit C channels - a test of the group and the layer, never of this rank's shard,
    so all ranks decide alike.  The plan keeps `group` alive, so its id stays its own.  Not cached: under a stream capture (the
    scratch would belong to the graph's pool) or with an exchange `xr` the caller forces (XRankExchange.verify)."""
    st = _raw_stream(x.device.index)
    key = (kind, id(group), x.device.index, st, N, C, HW, kind != 'cfg2' and x.data_ptr() % 16 == 0)
    plan = _XPLAN.get(key) if xr is None else None
    if plan is None:
        cache = xr is None and not torch.cuda.is_current_stream_capturing()
        if xr is None and _XRANK_ON:
            xr = D.xrank_exchange(group)
        plan = False
        if xr is not None and xr.fits(C, 1 if kind == 'cfg2' else 8):
            nbytes = _ws_bytes(kind, N, C, HW, int(key[-1]))
            if kind == 'aciq':          # the tables that nobody outside the call reads live behind the workspace
                nbytes += (L.NSTAT + L.NQP + L.NDIAG) * C * 4 + L.NMOM * C * 8
            plan = (xr, group, _scratch(x, kind, nbytes, st), _gws_args(_group_workspace(x, st)), st)
        if cache:
            _XPLAN[key] = plan
    return plan or None


def _pc_stats_xrank(x, N, C, HW, need_b, need_kurt, need_relu, group, flags=0, _xrank=None):
    """Config 4 of a batch shard in ONE host call and - where the shard has a flat-tile plan - one launch and one read of x
    (cnnq_pc_stats_xrank: k_stats_flat with the cross-rank stage; otherwise the chain's two passes with their records made global
    through the same window slots).  No collective.  Returns (stats, mom) of the GLOBAL batch, or None when the group has no
    in-launch exchange.  _xrank: an XRankExchange to use instead of the group's (its verify())."""
    plan = _xrank_plan('stats', x, N, C, HW, group, _xrank)
    if plan is None:
        return None
    xr, _, ws, gws, st = plan
    stats = torch.empty((L.NSTAT, C), dtype=torch.float32, device=x.device)
    mom = torch.empty((L.NMOM, C), dtype=torch.float64, device=x.device)
    rc = L.load().cnnq_pc_stats_xrank(x.data_ptr(), N, C, HW, 1 if need_b else 0, 1 if need_kurt else 0, 1 if need_relu else 0, ws.data_ptr(),
                                 *gws, mom.data_ptr(), stats.data_ptr(), ctypes.byref(xr.ctx(st)), int(flags), st)
    if rc:
        L.check(rc, 'cnnq_pc_stats_xrank')
    return stats, mom


def _aciq_qdq_xrank(x, N, C, HW, cfg, group, want_parts, out, flags=0):
    """Config 3 of a batch shard (Laplace clipping, optional bit allocation on the 'gaus' prior) in ONE host call
    (cnnq_pc_aciq_fused_xrank; round 6): pass A, its record made global through the exchange windows, (bit allocation), ONE launch
    for pass B + the ranks' sums of |x - mean| + parameters + Q/DQ - the four launches of one GPU, 12 bytes per element, no
    collective, where the chain moves 16 around two.  Returns y [, parts], or None when the group has no in-launch exchange (the
    caller takes the chain)."""
    plan = _xrank_plan('aciq', x, N, C, HW, group)
    if plan is None:
        return None
    xr, _, ws, gws, st = plan
    y = _out_like(x, out)
    if want_parts:
        tabs = torch.empty((L.NSTAT + L.NQP + L.NDIAG, C), dtype=torch.float32, device=x.device)
        mom = torch.empty((L.NMOM, C), dtype=torch.float64, device=x.device)
        tp, mp = tabs.data_ptr(), mom.data_ptr()
    else:                       # nobody outside the call reads the tables: they live behind the workspace
        mp = ws.data_ptr() + _ws_bytes('aciq', N, C, HW, int(x.data_ptr() % 16 == 0))
        tp = mp + L.NMOM * C * 8
    sp, qp, dp = tp, tp + L.NSTAT * C * 4, tp + (L.NSTAT + L.NQP) * C * 4
    rc = L.load().cnnq_pc_aciq_fused_xrank(x.data_ptr(), y.data_ptr(), N, C, HW, ctypes.byref(cfg), ws.data_ptr(), *gws, sp, mp, qp,
                                      dp, ctypes.byref(xr.ctx(st)), int(flags), st)
    if rc:
        L.check(rc, 'cnnq_pc_aciq_fused_xrank')
    if want_parts:
        return y, dict(stats=tabs[:L.NSTAT], qp=tabs[L.NSTAT:L.NSTAT + L.NQP], diag=tabs[L.NSTAT + L.NQP:], mom=mom)
    return y


def _mid_tread_qdq_xrank(x, N, C, HW, target, sym, tabs_mt, group, want_entropy, want_parts, flags=0):
    """Config 5 of a batch shard: as _aciq_qdq_xrank with the bin allocation and MODE 1 of the fused kernels
    (cnnq_pc_midtread_fused_xrank); the ranks' code counts are summed before the entropy (the one collective left: an integer
    all-reduce of the count table).  Returns what mid_tread_qdq returns, or None when the group has no in-launch exchange."""
    plan = _xrank_plan('aciq', x, N, C, HW, group)
    if plan is None:
        return None
    xr, _, ws, gws, st = plan
    y = torch.empty_like(x)
    tabs = torch.empty((L.NSTAT + L.NMT, C), dtype=torch.float32, device=x.device)
    stats, mt = tabs[:L.NSTAT], tabs[L.NSTAT:]
    mom = torch.empty((L.NMOM, C), dtype=torch.float64, device=x.device)
    hist = torch.empty(L.mt_hist_words(C), dtype=torch.int64, device=x.device) if want_entropy else None     # zeroed by the call
    rc = L.load().cnnq_pc_midtread_fused_xrank(x.data_ptr(), y.data_ptr(), N, C, HW, float(target), int(bool(sym)), tabs_mt.data_ptr(),
                                          tabs_mt.shape[1], ws.data_ptr(), *gws, stats.data_ptr(), mom.data_ptr(), mt.data_ptr(),
                                          _ptr(hist), ctypes.byref(xr.ctx(st)), int(flags), st)
    if rc:
        L.check(rc, 'cnnq_pc_midtread_fused_xrank')
    entropy = _mt_entropy(x, hist, mt, C, st, group, mom) if want_entropy else None
    return _mt_result(y, entropy, parts=dict(stats=stats, mt=mt, hist=hist, mom=mom) if want_parts else None)


def pc_stats_single(x, N, C, HW, need_b=False, need_kurt=False, need_relu=False, flags=8):
    """The statistics table and the merged moment record from ONE launch that reads x once (cnnq_pc_stats_single), or None
    when the shape has no flat-tile plan.  flags: bit 3 (default here) also takes channels of more than 256 tiles, which
    ops.pc_stats leaves to the chain; bit 0 forces the recompute path (tests)."""
    lib = L.load()
    x = _dev(x, 'x')
    st = _raw_stream(x.device.index)
    gws = _group_workspace(x, st)
    if gws is None:
        return None
    stats = torch.empty((L.NSTAT, C), dtype=torch.float32, device=x.device)
    mom = torch.empty((L.NMOM, C), dtype=torch.float64, device=x.device)
    rc = lib.cnnq_pc_stats_single(_ptr(x), N, C, HW, int(bool(need_b)), int(bool(need_kurt)), int(bool(need_relu)), gws,
                                  GROUP_WS_BYTES, _ptr(mom), _ptr(stats), int(flags), st)
    if not _supported(rc, 'cnnq_pc_stats_single'):
        return None
    return stats, mom


# ------------------------------------------------------------------------------------- parameters
CLIP_CODES = {'no': 0, 'laplace': 1, 'gaus': 2}


def _params_cfg(num_bits, positive, clip, bit_alloc, prior_is_b, target, round_mode, direct_range):
    cfg = L.ParamsCfg()
    cfg.num_bits = int(num_bits)
    cfg.positive = int(bool(positive))
    if clip in CLIP_CODES:
        if clip != 'no' and int(num_bits) > 8:
            # iq.py:14-41: alpha_laplace / alpha_gaus have keys 0..8 only (the reference raises KeyError)
            raise L.CnnqError('%s clipping is tabulated for at most 8 bits, got %d' % (clip, int(num_bits)))
        cfg.clip, cfg.pstd = CLIP_CODES[clip], 0.
    elif 'std' in clip:
        cfg.clip, cfg.pstd = 3, float(clip.replace('std', ''))
    elif clip == 'mix':
        # iq.py:310-323 picks per channel between three clipping values from error columns of a statistics file: that is
        # act_qdq_mix (three parameter tables merged per channel), not one configuration of this kernel
        raise L.CnnqError("clipping 'mix' goes through ops.act_qdq_mix (it needs the mse_* columns of a statistics file)")
    else:
        raise L.CnnqError('unsupported clipping %r' % (clip,))
    cfg.bit_alloc = int(bool(bit_alloc))
    cfg.prior_is_b = int(bool(prior_is_b))
    cfg.target = float(num_bits if target is None else target)
    cfg.round_mode = int(bool(round_mode))
    cfg.direct_range = int(bool(direct_range))
    return cfg


def pc_params(stats, num_bits, positive=False, clip='no', bit_alloc=False, prior_is_b=False, target=None,
              round_mode=True, direct_range=False):
    """stats [NSTAT, C] -> (qp [NQP, C], diag [NDIAG, C]); see cnnq_pc_params."""
    lib = L.load()
    C = stats.shape[1]
    cfg = _params_cfg(num_bits, positive, clip, bit_alloc, prior_is_b, target, round_mode, direct_range)
    qp = torch.empty((L.NQP, C), dtype=torch.float32, device=stats.device)
    diag = torch.empty((L.NDIAG, C), dtype=torch.float32, device=stats.device)
    L.check(lib.cnnq_pc_params(_ptr(stats), C, ctypes.byref(cfg), _ptr(qp), _ptr(diag), _stream(stats)),
            'cnnq_pc_params')
    return qp, diag


def mix_candidates(stats, num_bits, positive=False, bit_alloc=False, prior_is_b=False, target=None, round_mode=True,
                   whole_tensor=False):
    """The three parameter tables `-c mix` chooses between per channel (iq.py:310-323), from one statistics table
    [NSTAT, C]: (qp_l, qp_g, qp_p) - Laplace clipping, Gaussian clipping, the min/max half range (max - min) / 2.  Two
    cnnq_pc_params launches; the min/max candidate in a few [C]-sized fp32 torch ops that repeat that kernel's arithmetic
    (iq.py:284-300, 351, 443, 559-572).  Shared by act_qdq_mix (the consumer) and the per-channel statistics manager's
    collect_err (the producer of the error columns), so both speak about the same three quantizations."""
    kw = dict(positive=positive, bit_alloc=bit_alloc, prior_is_b=prior_is_b, target=target, round_mode=round_mode,
              direct_range=whole_tensor)
    qp_l, dg_l = pc_params(stats, num_bits, clip='laplace', **kw)
    qp_g, _ = pc_params(stats, num_bits, clip='gaus', **kw)
    mn, mx, mean = stats[L.STAT_MIN], stats[L.STAT_MAX], stats[L.STAT_MEAN]
    alpha = (mx - mn) / 2
    if positive:
        rng, off = torch.clamp_min(mean, 0.) + alpha, torch.zeros_like(alpha)
    else:
        rng, off = 2 * alpha, torch.maximum(mn, mean - alpha)
    delta = rng if whole_tensor else (off + rng) - off
    if bit_alloc and num_bits <= 4:
        qmax = torch.exp2(dg_l[L.DIAG_BITS]) - 1.
        scale = torch.where(qmax > 0, delta / qmax, torch.zeros_like(delta))
    else:
        qmax = torch.full_like(delta, float(2 ** int(num_bits) - 1))
        scale = delta / qmax
    scale = torch.where(scale < 1e-8, torch.full_like(scale, 1e-8), scale)
    zp = torch.round(0. - off / scale)
    return qp_l, qp_g, torch.stack([scale, zp, qmax])


def pc_quant_errors(x, N, C, HW, qps, mm=None):
    """Error columns [2K, C] (float32, on the device) of K = 1..3 candidate parameter tables `qps` (each [NQP, C]) on
    x[N][C][HW]: rows mse_0..K-1 (smpc.py:84), then cos_0..K-1 (smpc.py:96-98) - see cnnq_pc_qerr.  One read of x, no
    quantized tensor is materialised.  mm [2, C] (optional): x's exact channel extrema (rows min, max), which let the kernel
    take the divide-free quotient; the result does not depend on it.  float32 dense NCHW only."""
    lib = L.load()
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float32 or not x.is_contiguous():
        raise L.CnnqError('pc_quant_errors: x must be a contiguous float32 CUDA/HIP tensor (upcast / copy first)')
    x = _dev(x, 'x')
    qps = list(qps)
    K = len(qps)
    if not 1 <= K <= 3:
        raise L.CnnqError('pc_quant_errors: 1..3 candidate tables, got %d' % K)
    for q in qps:
        if not (isinstance(q, torch.Tensor) and q.device == x.device and q.dtype == torch.float32 and tuple(q.shape) == (L.NQP, C)):
            raise L.CnnqError('pc_quant_errors: every table must be a float32 [%d, %d] tensor on %s' % (L.NQP, C, x.device))
    if x.numel() != N * C * HW:
        raise L.CnnqError('pc_quant_errors: x has %d elements, N*C*HW = %d' % (x.numel(), N * C * HW))
    qp = torch.stack(qps).contiguous()
    if mm is not None:
        mm = mm.to(device=x.device, dtype=torch.float32).contiguous()
        if tuple(mm.shape) != (2, C):
            raise L.CnnqError('pc_quant_errors: mm must be [2, %d]' % C)
    key = ('qerr', N, C, HW, K)
    nbytes = _WS_BYTES.get(key)
    if nbytes is None:
        nbytes = lib.cnnq_pc_qerr_workspace(N, C, HW, K)
        if nbytes == 0:
            raise L.CnnqError('cnnq_pc_qerr_workspace(%d, %d, %d, %d): no plan for these sizes' % (N, C, HW, K))
        _WS_BYTES[key] = nbytes
    st = _raw_stream(x.device.index)
    err = torch.empty((2 * K, C), dtype=torch.float32, device=x.device)
    L.check(lib.cnnq_pc_qerr(_ptr(x), N, C, HW, _ptr(qp), K, _ptr(mm), _ptr(_scratch(x, 'qerr', nbytes, st)), _ptr(err), st),
            'cnnq_pc_qerr')
    return err


_QERR_NHWC_NATIVE = {}


def _qerr_nhwc_native(N, HW, C, dtype):
    """Whether this class of layer measures its error columns on the channels_last kernel: the "native" word of
    cnnq_pc_route_qerr_nhwc's report (0: a class that measured slower native than through the copy is sent back there).  The
    statistics manager (collect_route with native_err) and the tests patch the function and empty the cache by name."""
    return _route_word(_QERR_NHWC_NATIVE, (N, HW, C, dtype), bool, 'cnnq_pc_route_qerr_nhwc', (N, HW, C), dtype)


def pc_quant_errors_nhwc(x, qps, mm=None):
    """pc_quant_errors of a dense channels_last 4-D activation of fp32 / bf16 / fp16, on the storage as it lies (DESIGN.md section
    30; cnnq_pc_qerr_nhwc): [2K, C] float32, the columns of x.float() - one read of x, 4 B/elem in fp32 and 2 in bf16 / fp16, no
    quantized tensor.  qps, mm: as pc_quant_errors (the result does not depend on mm).  Anything else - a CPU tensor, another dtype,
    not 4-D, contiguous, not dense - raises: nothing is copied or upcast here."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise L.CnnqError('pc_quant_errors_nhwc: x must be a CUDA/HIP tensor (there is no CPU path)')
    if x.dtype not in _ACT_DTYPES:
        raise L.CnnqError('pc_quant_errors_nhwc: x must be float32, bfloat16 or float16, got %s' % x.dtype)
    if x.dim() != 4:
        _not_4d(x, 'pc_quant_errors_nhwc')
    if _layout(x) != 'nhwc' or x.numel() == 0:
        raise L.CnnqError('pc_quant_errors_nhwc: x must be a non-empty dense channels_last tensor that is not contiguous (no copy '
                          'is made here; pc_quant_errors takes contiguous float32)')
    if x.device.index != torch.cuda.current_device():
        raise L.CnnqError('pc_quant_errors_nhwc: x is on %s but the current device is cuda:%d' % (x.device, torch.cuda.current_device()))
    if x.requires_grad:
        x = x.detach()
    N, C = x.shape[0], x.shape[1]
    return _quant_errors_native('pc_quant_errors_nhwc', 'cnnq_pc_qerr_nhwc', x, (N, x.numel() // (N * C), C), C, _DTYPE_CODES[x.dtype],
                                _raw_stream(x.device.index), qps, mm)


def _quant_errors_native(what, fn, x, geo, C, dt, st, qps, mm):
    """The error columns [2K, C] of an admitted tensor on its native storage in one host call with one cached workspace (fn:
    cnnq_pc_qerr_nhwc with geo = (N, HW, C), cnnq_pc_qerr_dt with geo = (N, C, HW)): the table and mm checks, the row records, the
    kernel and the fold."""
    lib = L.load()
    qps = list(qps)
    K = len(qps)
    if not 1 <= K <= 3:
        raise L.CnnqError('%s: 1..3 candidate tables, got %d' % (what, K))
    for q in qps:
        if not (isinstance(q, torch.Tensor) and q.device == x.device and q.dtype == torch.float32 and tuple(q.shape) == (L.NQP, C)):
            raise L.CnnqError('%s: every table must be a float32 [%d, %d] tensor on %s' % (what, L.NQP, C, x.device))
    qp = torch.stack(qps).contiguous()
    if mm is not None:
        mm = mm.to(device=x.device, dtype=torch.float32).contiguous()
        if tuple(mm.shape) != (2, C):
            raise L.CnnqError('%s: mm must be [2, %d]' % (what, C))
    key = (fn, *geo, K, dt)
    nbytes = _WS_BYTES.get(key)
    if nbytes is None:
        nbytes = getattr(lib, fn + '_workspace')(*geo, K, dt)
        if nbytes == 0:
            raise L.CnnqError('%s_workspace(%d, %d, %d, %d): no plan for these sizes' % (fn, *geo, K))
        _WS_BYTES[key] = nbytes
    err = torch.empty((2 * K, C), dtype=torch.float32, device=x.device)
    L.check(getattr(lib, fn)(_ptr(x), dt, *geo, _ptr(qp), K, _ptr(mm), _ptr(_scratch(x, 'qerr', nbytes, st)), _ptr(err), st), fn)
    return err


_QERR_HALF_NATIVE = {}


def _qerr_half_native(N, C, HW, dtype):
    """Whether this class of layer measures its error columns on the contiguous bf16 / fp16 kernel: the "native" word of
    cnnq_pc_route_qerr_dt's report (0: a class that measured slower native than through the upcast is sent back there).  The
    statistics manager (collect_route with native_err_half) and the tests patch the function and empty the cache by name."""
    return _route_word(_QERR_HALF_NATIVE, (N, C, HW, dtype), bool, 'cnnq_pc_route_qerr_dt', (N, C, HW), dtype)


def pc_quant_errors_half(x, qps, mm=None):
    """pc_quant_errors of a contiguous 4-D bf16 / fp16 activation, on the storage as it lies (DESIGN.md section 31;
    cnnq_pc_qerr_dt): [2K, C] float32, the columns of x.float() - one read of x, 2 B/elem, no quantized tensor.  qps, mm: as
    pc_quant_errors (the result does not depend on mm).  Anything else - a CPU tensor, float32, not 4-D, not contiguous - raises:
    nothing is copied or upcast here."""
    x, (_, geo, C, dt, st) = _admit_half(x, 'pc_quant_errors_half', 'pc_quant_errors')
    return _quant_errors_native('pc_quant_errors_half', 'cnnq_pc_qerr_dt', x, geo, C, dt, st, qps, mm)


def act_qdq_mix(x, num_bits, stats, mse, positive=False, bit_alloc=False, prior_is_b=False, target=None, round_mode=True,
                whole_tensor=False, want_codes=False, want_entropy=False, out=None):
    """clip_type == 'mix' of the `-sm use` route (iq.py:310-323 + 327-359): per channel the Gaussian clipping value where
    mse_gaus < mse_laplace, else the Laplace one, and the min/max half range (max - min) / 2 where mse_lowp < mse_gaus;
    comparisons with NaN are False, so a file whose error columns are NaN - all the reference's own collection writes -
    gives plain Laplace clipping.  stats [NSTAT, C]: the file's mean_{min, max, mean, b, std} rows; mse [3, C]: rows
    laplace, gaus, lowp.  Everything downstream of the clipping value is per channel and elementwise, so the three
    candidates' parameter tables (mix_candidates) are merged per channel, then one fused Q/DQ.  Per channel without codes or
    entropy x is admitted as pc_qdq admits it - a dense channels_last tensor of fp32 / bf16 / fp16 or a contiguous bf16 / fp16
    one is quantized where it lies, and y keeps its dtype and layout; every other combination takes a
    contiguous float32 x."""
    x = _dev(x, 'x') if (whole_tensor or want_codes or want_entropy) else _dev_act_layout(x, 'x')
    N, C, HW = (1, 1, x.numel()) if whole_tensor else geometry(x)
    stats = stats.to(device=x.device, dtype=torch.float32)
    mse = torch.as_tensor(mse, dtype=torch.float32, device=x.device).view(3, C)
    qp_l, qp_g, qp_p = mix_candidates(stats, num_bits, positive, bit_alloc, prior_is_b, target, round_mode, whole_tensor=whole_tensor)
    pick_g = (mse[1] < mse[0]).view(1, C)
    pick_p = (mse[2] < mse[1]).view(1, C)
    qp = torch.where(pick_p, qp_p, torch.where(pick_g, qp_g, qp_l)).contiguous()
    hist = torch.zeros(256, dtype=torch.int64, device=x.device) if want_entropy else None
    res = pc_qdq(x, N, C, HW, qp, want_codes=want_codes, out=out, hist=hist)
    if want_entropy:
        res = (res + (entropy_from_hist(hist),)) if want_codes else (res, entropy_from_hist(hist))
    return res


# ------------------------------------------------------------------------------------- Q/DQ
def pc_qdq(x, N, C, HW, qp, want_codes=False, out=None, hist=None, reverse=False):
    """y = dequant(quant(x)) with per-channel parameters; optionally the uint8 codes; `hist`
    (optional zeroed int64[256] tensor) receives the code histogram; reverse: descending addresses."""
    lib = L.load()
    x = _dev_act(x, 'x') if (want_codes or hist is not None) else _dev_act_layout(x, 'x')
    if _is_nhwc(x):
        return _pc_qdq_nhwc(x, qp, out)
    if x.dtype != torch.float32 and (want_codes or hist is not None):
        _half_only('pc_qdq', 'codes / the code histogram')
    y = _out_like(x, out)
    if x.dtype != torch.float32:
        L.check(lib.cnnq_pc_qdq_dt(_ptr(x), _ptr(y), _HALF_DTYPES[x.dtype], N, C, HW, _ptr(qp), None, None, 0, _stream(x)),
                'cnnq_pc_qdq_dt')
        return y
    codes = torch.empty(x.shape, dtype=torch.uint8, device=x.device) if want_codes else None
    L.check(lib.cnnq_pc_qdq(_ptr(x), _ptr(y), N, C, HW, _ptr(qp), _ptr(codes), _ptr(hist), int(bool(reverse)),
                            _stream(x)), 'cnnq_pc_qdq')
    return (y, codes) if want_codes else y


def _qdq_native(site, x, qp, out, nbins=0, slot=None):
    """pc_qdq of a tensor on its site with the table qp (cnnq_pc_qdq_nhwc / cnnq_pc_qdq_dt: the IEEE divide); y has x's layout and
    dtype.  slot (the replica tables of _nhwc_hist_slot / _half_hist_slot, on the site's stream): the pass also counts its codes
    into them, nbins bins (cnnq_pc_qdq_hist_nhwc / cnnq_pc_qdq_hist_dt): (y, entropy)."""
    layout, geo, C, dt, st = site
    fn, mid, fn_hist = layout['qdq']
    y = _out_like(x, out)
    if slot is None:
        rc = getattr(L.load(), fn)(x.data_ptr(), y.data_ptr(), dt, *geo, qp.data_ptr(), *mid, st)
        if rc:
            L.check(rc, fn)
        return y
    rc = getattr(L.load(), fn_hist)(x.data_ptr(), y.data_ptr(), dt, *geo, qp.data_ptr(), int(nbins), slot[0].data_ptr(), st)
    if rc:
        L.check(rc, fn_hist)
    return y, _replica_entropy(x, slot[0], slot[1], st)


def _pc_qdq_nhwc(x, qp, out, nbins=0, slot=None, st=None):
    """_qdq_native on a dense channels_last x that came through _dev_act_layout (st: the stream of the slot's tables)."""
    C = x.shape[1]
    return _qdq_native((_NHWC_LAYOUT, (x.numel() // C, C), C, _DTYPE_CODES[x.dtype], _raw_stream(x.device.index) if st is None else st),
                       x, qp, out, nbins, slot)


def _minmax_qdq_nhwc(x, num_bits, positive, out, slot=None, st=None):
    """Config 2 on a dense channels_last x on one GPU (cnnq_pc_minmax_qdq_nhwc: statistics partials over slabs of rows, the
    parameters, the channel extrema, the Q/DQ); one cached workspace, which also holds the parameter table.  y has x's layout.
    slot, st: as _pc_qdq_nhwc, 2^num_bits bins (cnnq_pc_minmax_qdq_hist_nhwc): (y, entropy)."""
    lib = L.load()
    C = x.shape[1]
    R = x.numel() // C
    dt = _DTYPE_CODES[x.dtype]
    nbytes = _ws_bytes('nhwc', R, C, 1, dt)
    y = _out_like(x, out)
    if slot is None:
        st = _raw_stream(x.device.index)
    ws = _scratch(x, 'nhwc', nbytes + L.NQP * C * 4, st).data_ptr()
    if slot is None:
        rc = lib.cnnq_pc_minmax_qdq_nhwc(x.data_ptr(), y.data_ptr(), dt, R, C, int(num_bits), 1 if positive else 0, ws, ws + nbytes,
                                         None, st)
        if rc:
            L.check(rc, 'cnnq_pc_minmax_qdq_nhwc')
        return y
    rc = lib.cnnq_pc_minmax_qdq_hist_nhwc(x.data_ptr(), y.data_ptr(), dt, R, C, int(num_bits), 1 if positive else 0, ws, ws + nbytes,
                                          None, slot[0].data_ptr(), st)
    if rc:
        L.check(rc, 'cnnq_pc_minmax_qdq_hist_nhwc')
    return y, _replica_entropy(x, slot[0], slot[1], st)


def _hist_bins(num_bits, use_ba):
    """The bins a counting channels_last pass keeps (nbins of cnnq_pc_qdq_hist_nhwc): 2^num_bits where the parameters come from
    num_bits alone - every channel's qmax is 2^num_bits - 1 - and 256 under bit allocation, whose per-channel qmax is decided on
    the device."""
    return 256 if use_ba else 1 << int(num_bits)


def _nhwc_hist_slot(x, what, st):
    """Where the counting pass of a dense channels_last x counts, as _entropy_slot gives it: (x, (tables, result or None)).  A class
    of layer the route function sends back ('hist', asked with 256 bins), and a call that can have no replica table (first use
    under a stream capture), take the copy route instead: (x.contiguous() - counted, as _dev counts it - , None); that route is
    float32 only, so a half tensor raises before anything is copied."""
    C = x.shape[1]
    slot = _entropy_slot(x, st) if _nhwc_native('hist', x.numel() // C, C, x.dtype) else (None, None)
    if slot[0] is not None:
        return x, slot
    if x.dtype != torch.float32:
        _half_only(what, 'the entropy of a tensor that does not take the channels_last kernels')
    global LAYOUT_COPIES
    LAYOUT_COPIES += 1
    return x.contiguous(), None


_GROUP_WS = {}
GROUP_WS_BYTES = 18 << 20


_GROUP_POOL = {}
GROUP_POOL_SIZE = 4


def _group_workspace(x, st=None):
    """The exchange workspace of the group single launch (cnnq_pc_minmax_qdq_group): fine-grained device memory
    from cnnq_group_ws_alloc, zeroed ONCE, one per (device, stream) - launches on one stream are ordered, so they
    share it; the kernel re-arms its counters.  Allocation synchronises the device, which a stream capture does
    not survive: the first call on a device allocates a small pool, later streams (a capture stream included)
    take from it; with the pool empty under capture there is no workspace (None: the caller takes the chain).
    Returns the raw device pointer (a ctypes.c_void_p)."""
    dev = x.device.index
    key = (dev, _raw_stream(dev) if st is None else st)
    ws = _GROUP_WS.get(key)
    if ws is not None:
        return ws
    pool = _GROUP_POOL.setdefault(dev, [])
    if not pool:
        if torch.cuda.is_current_stream_capturing():
            return None
        lib = L.load()
        for _ in range(GROUP_POOL_SIZE):
            w = ctypes.c_void_p()
            L.check(lib.cnnq_group_ws_alloc(GROUP_WS_BYTES, ctypes.byref(w)), 'cnnq_group_ws_alloc')
            pool.append(w)
    ws = _GROUP_WS[key] = pool.pop()
    return ws


GROUP_WAIT_EXPIRED, GROUP_TEST_HOOK = 1, 2


def group_status(x, clear=None):
    """Status word of this stream's group workspace (synchronises).  Bit 0 (GROUP_WAIT_EXPIRED): a bounded wait of the
    in-launch exchange ran out and its workgroup recomputed the extrema from x - results are unaffected, but the
    launch was slow (a group's members were not co-resident: another kernel held the CUs).  Bit 1 (GROUP_TEST_HOOK):
    the recompute path was forced by the test flag.  The word is sticky on the device, and while bit 0 is up every later
    wait is bounded by 0.5 ms instead of 20 ms (csrc/cnnq_group.hip.h): reading it ACKNOWLEDGES it - a non-zero word is
    zeroed after the read unless clear=False - so one transient expiry (a profiler attaching, a co-tenant's kernel) does
    not leave the short bound in force for the rest of the process.  clear=True zeroes unconditionally."""
    ws = _GROUP_WS.get((x.device.index, _raw_stream(x.device.index)))
    if ws is None:
        return 0
    v = ctypes.c_uint32()
    lib = L.load()
    L.check(lib.cnnq_group_ws_status(ws, ctypes.byref(v)), 'cnnq_group_ws_status')
    if clear or (clear is None and v.value != 0):
        L.check(lib.cnnq_group_ws_status_clear(ws), 'cnnq_group_ws_status_clear')
    return int(v.value)


def minmax_qdq_group(x, N, C, HW, num_bits, positive=False, out=None, want_parts=False, flags=0):
    """Config 2 in ONE launch and ONE read of x for tensors whose channels span several workgroups
    (cnnq_pc_minmax_qdq_group).  Returns None when the shape is not supported (the caller takes the chain)."""
    lib = L.load()
    x = _dev(x, 'x')
    nbytes = lib.cnnq_pc_group_workspace(N, C, HW)
    if nbytes == 0 or nbytes > GROUP_WS_BYTES:
        return None
    gws = _group_workspace(x)
    if gws is None:
        return None
    y = _out_like(x, out)
    qp = torch.empty((L.NQP + 2, C), dtype=torch.float32, device=x.device)
    rc = lib.cnnq_pc_minmax_qdq_group(_ptr(x), _ptr(y), N, C, HW, int(num_bits), int(bool(positive)),
                                      gws, _ptr(qp), _ptr(qp[L.NQP:]) if want_parts else None,
                                      int(flags), _stream(x))
    if not _supported(rc, 'cnnq_pc_minmax_qdq_group'):
        return None
    return (y, _minmax_parts(qp[L.NQP:], qp[:L.NQP])) if want_parts else y


def minmax_qdq_resident(x, N, C, HW, num_bits, positive=False, out=None, want_parts=False):
    """Config 2 in ONE launch and ONE read of x (cnnq_pc_minmax_qdq_resident): the bits of the three-launch chain
    at 8 instead of 12 bytes per element.  Returns None when the shape has no resident kernel (a channel's batch
    population does not fit a workgroup's registers, unaligned pointers, H*W % 4 != 0 without a straddling
    layout) - the caller then takes the chain."""
    lib = L.load()
    x = _dev(x, 'x')
    y = _out_like(x, out)
    qp = torch.empty((L.NQP + 2, C), dtype=torch.float32, device=x.device)     # parameters + {min, max} rows
    rc = lib.cnnq_pc_minmax_qdq_resident(_ptr(x), _ptr(y), N, C, HW, int(num_bits), int(bool(positive)), _ptr(qp),
                                         _ptr(qp[L.NQP:]) if want_parts else None, _stream(x))
    if not _supported(rc, 'cnnq_pc_minmax_qdq_resident'):
        return None
    return (y, _minmax_parts(qp[L.NQP:], qp[:L.NQP])) if want_parts else y


_HIST_REP = {}


def _hist_replicas(x, st):
    """The replica histogram of the single-launch kernels (cnnq_hist_replica_bytes), one per (device, stream), zeroed
    ONCE: cnnq_entropy_replicas leaves it zero."""
    key = (x.device.index, st)
    t = _HIST_REP.get(key)
    if t is None:
        if torch.cuda.is_current_stream_capturing():
            # first use under a stream capture: the zero fill would only be RECORDED and the block would belong to the
            # graph's pool - an eager call on this stream later would count into a table that was never zeroed.  The
            # caller takes the chain for this call instead (its histogram is a per-call buffer).
            return None
        t = _HIST_REP[key] = torch.zeros(L.load().cnnq_hist_replica_bytes() // 8, dtype=torch.int64, device=x.device)
    return t


_ENT_BATCH = None
_ENT_TABLES = {}        # per (device, stream): ENT_BATCH_CAP sets of replica tables, zeroed once (the batch kernel leaves them zero)
ENT_BATCH_CAP = 64


class entropy_batch:
    """`with ops.entropy_batch(): ...` - the entropies of the codes (want_entropy=True: -me, iq.py:445,179,217) of every tensor
    quantized inside the block are computed by ONE launch at its end instead of a dependent one-workgroup launch behind every
    tensor (8-25 us each: 0.76 ms of the 9.5 ms ResNet-50 b512 step with -me in round 5).  Nothing consumes an entropy
    mid-forward - the reference logs it - so the 0-dim tensors the calls hand out are only filled when the block ends (or at
    flush()); reading one earlier gives whatever the buffer held.  Each tensor counts into its own set of replica tables (128 KB;
    64 sets per stream).  One stream per block; not for use under a stream capture on its first use (the tables are zero-filled
    once) - the calls then take the per-tensor launch."""

    def __init__(self):
        self.n, self.out, self.tables, self.st, self.key, self.mt, self.pending = 0, None, None, None, None, [], []

    def after(self, fn):
        """run fn() once the entropies of the block are there (IntQuantizer's logger calls: float(entropy) is a host read)"""
        self.pending.append(fn)

    def __enter__(self):
        global _ENT_BATCH
        self._outer, _ENT_BATCH = _ENT_BATCH, self
        return self

    def __exit__(self, *exc):
        global _ENT_BATCH
        _ENT_BATCH = self._outer
        if exc[0] is None:
            self.flush()
        else:
            self._abandon()
        return False

    def _abandon(self):
        """The block raised: nothing is launched and no callback runs.  The table sets the block counted into are not zero, so
        the stream's cache entry goes - the next block allocates zeroed ones (the allocator hands the old block out again on the
        same stream only, behind the launches that still count into it)."""
        if self.n:
            _ENT_TABLES.pop(self.key, None)
        self.n, self.out, self.tables, self.mt, self.pending = 0, None, None, [], []

    def slot(self, x, st):
        """(replica tables of this tensor, the 0-dim result) or None when no table set can be had (first use under a capture)"""
        if self.st is not None and st != self.st:
            raise L.CnnqError('entropy_batch: one stream per block')
        if self.tables is None:             # (not `self.st is None`: add_midtread sets the stream too)
            key = (x.device.index, st)
            tables = _ENT_TABLES.get(key)
            if tables is None:
                if torch.cuda.is_current_stream_capturing():
                    return None
                words = L.load().cnnq_hist_replica_bytes() // 8
                tables = _ENT_TABLES[key] = torch.zeros((ENT_BATCH_CAP, words), dtype=torch.int64, device=x.device)
            self.st, self.tables, self.key = st, tables, key
        if self.n == ENT_BATCH_CAP:
            self.flush()
        if self.out is None:
            self.out = torch.empty(ENT_BATCH_CAP, dtype=torch.float32, device=x.device)
        i = self.n
        self.n += 1
        return self.tables[i], self.out[i]

    def add_midtread(self, hist, mt, C, total, device):
        """the mid-tread path's histogram of one tensor (cnnq_midtread_entropy's arguments); returns the 0-dim result"""
        st = _raw_stream(device.index)
        if self.st is None:
            self.st = st
        elif st != self.st:
            raise L.CnnqError('entropy_batch: one stream per block')
        if len(self.mt) == 16:
            self._flush_midtread()
        if not self.mt:
            self.mt_out = torch.empty(16, dtype=torch.float32, device=device)
        self.mt.append((hist, mt, int(C), int(total)))      # (the references keep the tables alive until the launch)
        return self.mt_out[len(self.mt) - 1]

    def _flush_midtread(self):
        n = len(self.mt)
        if n:
            hp = (ctypes.c_void_p * n)(*[h.data_ptr() for h, _, _, _ in self.mt])
            mp = (ctypes.c_void_p * n)(*[m.data_ptr() for _, m, _, _ in self.mt])
            cs = (ctypes.c_int64 * n)(*[c for _, _, c, _ in self.mt])
            ts = (ctypes.c_int64 * n)(*[t for _, _, _, t in self.mt])
            L.check(L.load().cnnq_midtread_entropy_batch(n, hp, mp, cs, ts, self.mt_out.data_ptr(), self.st), 'cnnq_midtread_entropy_batch')
            self.mt = []

    def flush(self):
        if self.n:
            L.check(L.load().cnnq_entropy_replicas_batch(self.tables.data_ptr(), self.n, self.out.data_ptr(), self.st),
                    'cnnq_entropy_replicas_batch')
            self.n, self.out = 0, None          # (the views handed out keep the old result buffer alive)
        self._flush_midtread()
        pending, self.pending = self.pending, []
        for fn in pending:
            fn()


def _entropy_slot(x, st):
    """Where a want_entropy launch counts: (tables, result or None).  Inside an entropy_batch block its next table set and the
    result it will fill at the end; else the stream's shared replica tables (None: no result yet - the caller launches
    cnnq_entropy_replicas behind its tensor)."""
    if _ENT_BATCH is not None:
        s = _ENT_BATCH.slot(x, st)
        if s is not None:
            return s
    return _hist_replicas(x, st), None


def _replica_entropy(x, hist, ent_batched, st):
    """The entropy of a single launch's replica tables: the entropy_batch result (filled at the block's end), else one launch."""
    if ent_batched is not None:
        return ent_batched
    ent = torch.empty(1, dtype=torch.float32, device=x.device)
    L.check(L.load().cnnq_entropy_replicas(_ptr(hist), _ptr(ent), st), 'cnnq_entropy_replicas')
    return ent[0]


def minmax_qdq_single(x, N, C, HW, num_bits, positive=False, want_codes=False, want_entropy=False, out=None,
                      want_parts=False):
    """Config 2 in ONE launch also when the codes and / or the entropy of the codes are wanted
    (cnnq_pc_minmax_qdq_single; the entropy is one more tiny launch).  Returns None when the shape has no
    single-launch kernel or the codes do not fit a byte (the caller takes the chain)."""
    if num_bits > 8 and (want_codes or want_entropy):
        return None
    lib = L.load()
    x = _dev(x, 'x')
    st = _raw_stream(x.device.index)
    gws = _group_workspace(x, st)
    y = _out_like(x, out)
    qp = torch.empty((L.NQP + 2, C), dtype=torch.float32, device=x.device)
    codes = torch.empty(x.shape, dtype=torch.uint8, device=x.device) if want_codes else None
    hist, ent_batched = _entropy_slot(x, st) if want_entropy else (None, None)
    if want_entropy and hist is None:
        return None
    rc = lib.cnnq_pc_minmax_qdq_single(_ptr(x), _ptr(y), N, C, HW, int(num_bits), int(bool(positive)), *_gws_args(gws),
                                       _ptr(qp), _ptr(qp[L.NQP:]), _ptr(codes), _ptr(hist), None, st)
    if not _supported(rc, 'cnnq_pc_minmax_qdq_single'):
        return None
    return _result(y, codes, _replica_entropy(x, hist, ent_batched, st) if want_entropy else None,
                   _minmax_parts(qp[L.NQP:], qp[:L.NQP]) if want_parts else None)


def aciq_qdq_single(x, N, C, HW, num_bits, positive=False, bit_alloc=False, target=None, round_mode=True, want_codes=False,
                    want_entropy=False, want_parts=False, out=None, flags=0):
    """Config 3 (Laplace clipping, dynamic statistics, optional bit allocation on the 'gaus' prior) with pass B, the
    parameters and the Q/DQ in ONE launch and one read of x (cnnq_pc_aciq_qdq_single: pass A, merge, bit allocation, the
    single launch).  Returns y [, codes] [, entropy] [, parts], or None when the shape has no single-launch plan (the
    caller takes the chain)."""
    lib = L.load()
    x = _dev(x, 'x')
    st = _raw_stream(x.device.index)
    gws = _group_workspace(x, st)
    if gws is None:
        return None
    hist, ent_batched = _entropy_slot(x, st) if want_entropy else (None, None)
    if want_entropy and hist is None:
        return None
    cfg = _params_cfg(num_bits, positive, 'laplace', bit_alloc, False, target, round_mode, False)
    nbytes = _ws_bytes('aciq', N, C, HW, int(x.data_ptr() % 16 == 0))
    ws = _scratch(x, 'aciq', nbytes + (L.NQP + L.NDIAG) * C * 4, st)
    y = _out_like(x, out)
    tabs = torch.empty((L.NSTAT + L.NQP + L.NDIAG, C), dtype=torch.float32, device=x.device)
    stats, qp, diag = tabs[:L.NSTAT], tabs[L.NSTAT:L.NSTAT + L.NQP], tabs[L.NSTAT + L.NQP:]
    codes = torch.empty(x.shape, dtype=torch.uint8, device=x.device) if want_codes else None
    rc = lib.cnnq_pc_aciq_qdq_single(_ptr(x), _ptr(y), N, C, HW, ctypes.byref(cfg), ws.data_ptr(), gws, GROUP_WS_BYTES, _ptr(stats),
                                     _ptr(qp), _ptr(diag), _ptr(codes), _ptr(hist), int(flags), st)
    if not _supported(rc, 'cnnq_pc_aciq_qdq_single'):
        return None
    return _result(y, codes, _replica_entropy(x, hist, ent_batched, st) if want_entropy else None,
                   dict(stats=stats, qp=qp, diag=diag) if want_parts else None)


def minmax_quantize_pack4(x, num_bits=4, positive=False, out=None):
    """Dynamic per-channel min/max quantization of x [N, C, H, W] straight to the STORED format: two 4-bit codes per
    byte instead of the dequantized floats, in one launch and one read of x (4.5 bytes per element).
    Returns (packed uint8 [numel / 2], qp [NQP, C]); dequantize_pack4(packed, x.shape, qp) gives back exactly what
    act_qdq_per_channel(x, num_bits) returns.  None when the shape has no single-launch kernel."""
    lib = L.load()
    x = _dev(x, 'x')
    if num_bits > 4 or x.numel() % 2:
        raise L.CnnqError('packed 4-bit storage needs num_bits <= 4 and an even number of elements')
    N, C, HW = geometry(x)
    st = _raw_stream(x.device.index)
    gws = _group_workspace(x, st)
    packed = torch.empty(x.numel() // 2, dtype=torch.uint8, device=x.device) if out is None else out
    if out is not None and not (out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.numel() >= x.numel() // 2):
        raise L.CnnqError('out must be a contiguous uint8 device buffer of numel / 2 bytes')
    qp = torch.empty((L.NQP, C), dtype=torch.float32, device=x.device)
    rc = lib.cnnq_pc_minmax_qdq_single(_ptr(x), None, N, C, HW, int(num_bits), int(bool(positive)), *_gws_args(gws), _ptr(qp),
                                       None, None, None, _ptr(packed), st)
    if not _supported(rc, 'cnnq_pc_minmax_qdq_single'):
        return None
    return packed, qp


def minmax_qdq_fused(x, N, C, HW, num_bits, positive=False, want_codes=False, want_entropy=False, out=None,
                     want_parts=False, group=None, _checked=False, chain=False, _xrank=None):
    """Config 2 (iq.py:409-451, 557-603): dynamic per-channel min/max -> scale / zero point -> Q/DQ; no host sync.
    Three routes, one function each:

    * one GPU (_minmax_qdq_local): a single launch that reads x once where the shape has one, else the three-launch
      chain (k_minmax -> k_minmax_params -> k_qdq);
    * the batch sharded over the ranks of `group`, x this rank's shard (world size > 1, or CNNQ_FORCE_EXCHANGE=1 on a
      1-rank group): the collective route (_minmax_qdq_collective, default: statistics launch -> all_gather of the local
      extrema [2, C] -> parameters + Q/DQ launch), or - opt-in, D.xrank_mode - the exchange inside the single launch
      (_minmax_qdq_xrank).  Extrema are exact, so every rank gets the bits of one GPU holding the whole batch.

    chain=True forces the three-launch chain where a single-launch kernel would otherwise run: the reference form the
    single-launch kernels are tested against.  _xrank: an XRankExchange to use (its verify()), False: never.  group=False:
    replicated data, the one-GPU route."""
    if not _checked:
        nhwc = not (want_codes or want_entropy or want_parts or chain or _xrank) and not _sharded(group)
        x = _dev_act_layout(x, 'x') if nhwc else _dev_act(x, 'x')
    if _is_nhwc(x):
        # a dense channels_last x: plain config 2 on one GPU, on the storage as it is
        return _minmax_qdq_nhwc(x, num_bits, positive, out)
    if x.dtype != torch.float32:
        return _minmax_qdq_half(x, N, C, HW, num_bits, positive, want_codes, want_entropy, out, want_parts, group)
    # group=False: replicated data (weights) - never exchanged, whatever process group the job runs in: an exchange would give
    # the same bits for one needless collective per layer, and a wait that expired there would leave NaN WEIGHTS behind,
    # outside any forward a checkpoint redoes
    if not _sharded(group):
        return _minmax_qdq_local(x, N, C, HW, num_bits, positive, want_codes, want_entropy, out, want_parts, chain)
    resident = _RESIDENT and not chain
    if _xrank is not False and (_xrank is not None or _XRANK_ON) and not ((want_codes or want_entropy) and num_bits > 8):
        res = _minmax_qdq_xrank(x, N, C, HW, num_bits, positive, want_codes, want_entropy, out, want_parts, group, resident, _xrank)
        if res is not None:
            return res
    return _minmax_qdq_collective(x, N, C, HW, num_bits, positive, want_codes, want_entropy, out, want_parts, group,
                                  D.world_size(group), resident)


def _minmax_qdq_half(x, N, C, HW, num_bits, positive, want_codes, want_entropy, out, want_parts, group):
    """Config 2 on a bf16 / fp16 tensor on one GPU (cnnq_pc_minmax_qdq_auto_dt: one launch when a channel fits a workgroup,
    else exact extrema of the 2-byte elements then the Q/DQ; the result rounded back into the input type).  want_entropy (codes
    that fit a byte): _minmax_qdq_half_entropy.  Codes, the parts, wider codes' entropy and the sharded exchange have no half
    kernels: the quantizer computes those on x.float()."""
    if want_codes or want_parts or (want_entropy and num_bits > 8):
        _half_only('minmax_qdq_fused', "codes / parts / the entropy of codes wider than a byte")
    if _sharded(group):
        _half_only('minmax_qdq_fused', 'the sharded exchange')
    if want_entropy:
        return _minmax_qdq_half_entropy(x, N, C, HW, num_bits, positive, out)
    lib = L.load()
    nbytes = _ws_bytes('cfg2', N, C, HW)
    y = _out_like(x, out)
    st = _raw_stream(x.device.index)
    rc = lib.cnnq_pc_minmax_qdq_auto_dt(x.data_ptr(), y.data_ptr(), _HALF_DTYPES[x.dtype], N, C, HW, int(num_bits),
                                        1 if positive else 0, _scratch(x, 'cfg2', nbytes, st).data_ptr(), None, 0,
                                        1 if _RESIDENT else 0, st)
    if rc:
        L.check(rc, 'cnnq_pc_minmax_qdq_auto_dt')
    return y


_ENTROPY_HALF_NATIVE = {}


def _entropy_half_native(N, C, HW, dtype, nbins=256):
    """The route word of cnnq_pc_route_qdq_hist_dt's report for this class of contiguous bf16 / fp16 layer:
    1 - config 2 with the entropy of its codes in one launch, 2 - the statistics launch and the counting pass, 0 - a class that
    measured slower native than through the upcast and is sent back there.  The quantizer (_pc_route, _clip_route) and the tests
    patch the function and empty the cache by name."""
    return _route_word(_ENTROPY_HALF_NATIVE.setdefault(int(nbins), {}), (N, C, HW, dtype), int, 'cnnq_pc_route_qdq_hist_dt',
                       (N, C, HW), dtype, (int(nbins), 1))


def _half_hist_slot(x, what, st):
    """The replica tables a counting pass over a contiguous bf16 / fp16 x counts into, as _entropy_slot gives them: (tables, result
    or None).  There is no other route for a half tensor here, so a call that can have no table - first use under a stream
    capture - raises, and names the remedy."""
    slot = _entropy_slot(x, st)
    if slot[0] is None:
        raise L.CnnqError('%s: no replica table for the code histogram on this stream yet, and none can be made under a stream '
                          'capture: make one eager want_entropy call on the stream first' % what)
    return slot


def _minmax_qdq_half_entropy(x, N, C, HW, num_bits, positive, out, single_launch=None):
    """Config 2 with the entropy of its codes on a contiguous bf16 / fp16 tensor on one GPU (cnnq_pc_minmax_qdq_hist_dt, DESIGN.md
    section 29): one launch that keeps a channel in registers where the route function says so, else the exact extrema of the 2-byte
    elements and the counting Q/DQ pass; 2^num_bits bins.  (y, entropy); inside an entropy_batch block the entropy is filled by
    the block's one launch.  single_launch: None - the route function's choice; 0 - the two launches; 2 - the resident form
    wherever the channel fits (tests, A/B)."""
    lib = L.load()
    nbytes = _ws_bytes('cfg2', N, C, HW)
    y = _out_like(x, out)
    st = _raw_stream(x.device.index)
    hist, ent_batched = _half_hist_slot(x, 'act_qdq_per_channel', st)
    ws = _scratch(x, 'cfg2', nbytes, st).data_ptr()
    allow = (1 if _RESIDENT else 0) if single_launch is None else int(single_launch)
    rc = lib.cnnq_pc_minmax_qdq_hist_dt(x.data_ptr(), y.data_ptr(), _HALF_DTYPES[x.dtype], N, C, HW, int(num_bits),
                                        1 if positive else 0, ws, ws, ws + L.NQP * C * 4, hist.data_ptr(), allow, st)
    if rc:
        L.check(rc, 'cnnq_pc_minmax_qdq_hist_dt')
    return y, _replica_entropy(x, hist, ent_batched, st)


def _pc_qdq_half_entropy(x, N, C, HW, qp, nbins, out):
    """_qdq_native on a contiguous bf16 / fp16 x that came through _dev_act, the codes counted in nbins bins: (y, entropy)."""
    st = _raw_stream(x.device.index)
    return _qdq_native((_HALF_LAYOUT, (N, C, HW), C, _HALF_DTYPES[x.dtype], st), x, qp, out, nbins, _half_hist_slot(x, 'pc_qdq', st))


_LOCAL_PLAN = {}    # per (N, C, HW): (workspace bytes, whether the one-GPU hot call hands the C side the group workspace)


def _minmax_qdq_local(x, N, C, HW, num_bits, positive, want_codes, want_entropy, out, want_parts, chain):
    """Config 2 on one GPU."""
    lib = L.load()
    resident = _RESIDENT and not chain
    if not (want_codes or want_entropy or want_parts):
        # the hot call: one C entry point, one cached workspace, no torch allocation besides the result
        plan = _LOCAL_PLAN.get((N, C, HW))
        if plan is None:
            nbytes = _ws_bytes('cfg2', N, C, HW)
            d = (ctypes.c_int32 * 8)()
            # the group workspace is needed when there is no whole-channel kernel, or one with too few workgroups
            # to fill the chip (RES_MIN_WGS in csrc/cnnq_plan.hip.h: the C side routes, this only decides whether
            # to hand it the workspace)
            wants_group = ((lib.cnnq_pc_resident_describe(N, C, HW, d) != 0 or d[6] < 192)
                           and 0 < lib.cnnq_pc_group_workspace(N, C, HW) <= GROUP_WS_BYTES)
            plan = _LOCAL_PLAN[(N, C, HW)] = (nbytes, wants_group)
        nbytes, wants_group = plan
        y = _out_like(x, out)
        st = _raw_stream(x.device.index)          # looked up once: workspace keys and the launch stream
        gws = _group_workspace(x, st) if (resident and wants_group) else None
        rc = lib.cnnq_pc_minmax_qdq_auto(x.data_ptr(), y.data_ptr(), N, C, HW, int(num_bits), 1 if positive else 0,
                                         _scratch(x, 'cfg2', nbytes, st).data_ptr(), *_gws_args(gws), 1 if resident else 0, st)
        if rc:
            L.check(rc, 'cnnq_pc_minmax_qdq_auto')
        return y
    if resident and not want_codes and not want_entropy:
        res = minmax_qdq_resident(x, N, C, HW, num_bits, positive, out=out, want_parts=want_parts)
        if res is None:
            res = minmax_qdq_group(x, N, C, HW, num_bits, positive, out=out, want_parts=want_parts)
        if res is not None:
            return res
    if resident and _SINGLE_CODES:
        # codes / entropy out of the single launch too (round 3): no chain, no memset
        res = minmax_qdq_single(x, N, C, HW, num_bits, positive, want_codes, want_entropy, out=out, want_parts=want_parts)
        if res is not None:
            return res
    y, pmm, qp, codes, hist = _chain_buffers(x, N, C, HW, out, want_codes, want_entropy)
    L.check(lib.cnnq_pc_minmax_qdq(_ptr(x), _ptr(y), N, C, HW, int(num_bits), int(bool(positive)), _ptr(pmm),
                                   _ptr(qp), _ptr(codes), _ptr(hist), _stream(x)), 'cnnq_pc_minmax_qdq')
    entropy = entropy_from_hist(hist) if want_entropy else None
    parts = _minmax_parts(pmm, qp, lib.cnnq_pc_groups(N, C, HW, int(x.data_ptr() % 16 == 0))) if want_parts else None
    return _result(y, codes, entropy, parts)


def _chain_buffers(x, N, C, HW, out, want_codes, want_entropy):
    y = _out_like(x, out)
    G = _groups(N, C, HW)
    pmm = torch.empty((G, 2, C), dtype=torch.float32, device=x.device)
    qp = torch.empty((L.NQP, C), dtype=torch.float32, device=x.device)
    codes = torch.empty(x.shape, dtype=torch.uint8, device=x.device) if want_codes else None
    hist = torch.zeros(256, dtype=torch.int64, device=x.device) if want_entropy else None
    return y, pmm, qp, codes, hist


def _minmax_qdq_xrank(x, N, C, HW, num_bits, positive, want_codes, want_entropy, out, want_parts, group, resident, _xrank):
    """Config 2 of a batch shard with the cross-rank exchange INSIDE the single launch (csrc/cnnq_xrank.hip.h; opt-in,
    verified against the collective at first use): x is read once; every rank takes this route or none does.  Also with
    the codes / the entropy of the codes / the parameters wanted (the ranks' code counts are summed afterwards).  None: this
    group has no (verified) in-launch exchange - the caller takes the collective."""
    plan = _xrank_plan('cfg2', x, N, C, HW, group, _xrank)      # D.disable_xrank / release_plans() drop the plans
    hist_rep = _hist_replicas(x, plan[4]) if (want_entropy and plan is not None) else None
    if plan is None or (want_entropy and hist_rep is None):
        return None
    xr, _, ws, gws, st = plan
    y = _out_like(x, out)
    codes = torch.empty(x.shape, dtype=torch.uint8, device=x.device) if want_codes else None
    xr.minmax_qdq(x, y, N, C, HW, num_bits, positive, ws.data_ptr(), *(gws if resident else _gws_args(None)), st, codes=codes,
                  hist_rep=hist_rep)
    if not (want_codes or want_entropy or want_parts):
        return y
    entropy = parts = None
    if want_entropy:
        hist = torch.zeros(256, dtype=torch.int64, device=x.device)
        L.check(L.load().cnnq_hist_replicas_fold(_ptr(hist_rep), _ptr(hist), st), 'cnnq_hist_replicas_fold')
        D.all_reduce_sum_(hist, group)                       # the global batch's code counts
        entropy = entropy_from_hist(hist)
    if want_parts:
        tab = ws[:4 * (L.NQP + 2) * C].view(torch.float32).view(L.NQP + 2, C).clone()    # qp rows, then the global {min, max}
        parts = _minmax_parts(tab[L.NQP:], tab[:L.NQP])
    return _result(y, codes, entropy, parts)


def _minmax_qdq_collective(x, N, C, HW, num_bits, positive, want_codes, want_entropy, out, want_parts, group, world, resident):
    """Config 2 of a batch shard around a collective: local extrema (one launch) -> all_gather of [2, C] (ncclAllGather
    enqueued directly on the compute stream, rccl.py; torch.distributed on gloo rigs) -> parameters from the W gathered
    records + Q/DQ (one launch).  x is read twice (12 bytes per element); host-side skew between the ranks is harmless."""
    lib = L.load()
    if not (want_codes or want_entropy or want_parts):
        # the hot call: two C calls and the collective, all in cached workspaces
        st = _raw_stream(x.device.index)
        key = (id(group), x.device.index, st, N, C, HW, world, _DIRECT_RCCL)
        plan = _XPLAN.get(key)
        if plan is None:
            # everything that does not change from call to call: workspace slices, the gathered buffer, the direct
            # RCCL communicator (created collectively at first use).  The plan keeps `group` alive, so its id stays its
            # own, and its scratch buffers too (a later, larger tensor may make _scratch hand out new ones).
            ws = _scratch(x, 'cfg2', _ws_bytes('cfg2', N, C, HW), st)
            gbuf = _scratch(x, 'gath', 8 * C * world, st)
            from . import rccl
            dc = rccl.direct_comm(group)
            plan = _XPLAN[key] = dict(
                group=group, ws=ws, gbuf=gbuf, base=ws.data_ptr(), dc=dc,
                local=ws[12 * C:20 * C].view(torch.float32).view(2, C),            # the mm[2][C] slot of the workspace
                gathered=gbuf[:8 * C * world].view(torch.float32).view(world, 2, C))
        base = plan['base']
        y = _out_like(x, out)
        gws = _group_workspace(x, st) if resident else None      # one launch for the local extrema when the plan allows
        rc = lib.cnnq_pc_minmax_local_auto(x.data_ptr(), N, C, HW, base + 20 * C, *_gws_args(gws), base + 12 * C, st)
        if rc:
            L.check(rc, 'cnnq_pc_minmax_local_auto')
        dc = plan['dc']
        gathered = plan['gathered']
        if dc is not None:
            dc.all_gather_raw(base + 12 * C, gathered.data_ptr(), 8 * C, st)
        else:
            gathered = D.all_gather_records(plan['local'], group, out=gathered)
        rc = lib.cnnq_pc_gathered_qdq(x.data_ptr(), y.data_ptr(), N, C, HW, gathered.data_ptr(), world, int(num_bits),
                                      1 if positive else 0, base, st)
        if rc:
            L.check(rc, 'cnnq_pc_gathered_qdq')
        return y
    y, pmm, qp, codes, hist = _chain_buffers(x, N, C, HW, out, want_codes, want_entropy)
    g_used = lib.cnnq_pc_groups(N, C, HW, int(x.data_ptr() % 16 == 0))
    L.check(lib.cnnq_pc_minmax(_ptr(x), N, C, HW, _ptr(pmm), _stream(x)), 'cnnq_pc_minmax')
    local = torch.empty((2, C), dtype=torch.float32, device=x.device)
    L.check(lib.cnnq_pc_minmax_reduce(_ptr(pmm), g_used, C, _ptr(local), _stream(x)), 'cnnq_pc_minmax_reduce')
    pmm = D.all_gather_records(local, group)                     # [W, 2, C]
    L.check(lib.cnnq_pc_minmax_params(_ptr(pmm), world, C, int(num_bits), int(bool(positive)), _ptr(qp),
                                      _stream(x)), 'cnnq_pc_minmax_params')
    L.check(lib.cnnq_pc_qdq(_ptr(x), _ptr(y), N, C, HW, _ptr(qp), _ptr(codes), _ptr(hist), 1, _stream(x)),
            'cnnq_pc_qdq')
    if want_entropy:
        D.all_reduce_sum_(hist, group)
    return _result(y, codes, entropy_from_hist(hist) if want_entropy else None,
                   _minmax_parts(pmm, qp, world) if want_parts else None)


def _slice_ptr(t, c0, HW):
    return ctypes.c_void_p(t.data_ptr() + 4 * c0 * HW)


def _slice_aligned(t, c0, HW, stride):
    return int((t.data_ptr() + 4 * c0 * HW) % 16 == 0 and stride % 4 == 0)


def minmax_qdq_channel_slice(x, c0, c1, num_bits, positive=False, out=None):
    """Config 2 on the channel slice x[:, c0:c1] of a contiguous NCHW tensor, read and written in place of
    the parent (no slice copy): e.g. the branches of a concatenated output, each with its own quantizer
    settings.  Returns `out` (default: a new tensor shaped like x; only the slice is written)."""
    lib = L.load()
    x = _dev(x, 'x')
    N, C, HW = geometry(x)
    if not 0 <= c0 < c1 <= C:
        raise L.CnnqError('bad channel slice [%d, %d) of %d' % (c0, c1, C))
    y = _out_like(x, out)
    Cs, stride = c1 - c0, C * HW
    G = _groups(N, Cs, HW, _slice_aligned(x, c0, HW, stride))
    pmm = torch.empty((G, 2, Cs), dtype=torch.float32, device=x.device)
    qp = torch.empty((L.NQP, Cs), dtype=torch.float32, device=x.device)
    st = _stream(x)
    L.check(lib.cnnq_pc_minmax_strided(_slice_ptr(x, c0, HW), N, Cs, HW, stride, _ptr(pmm), st), 'cnnq_pc_minmax_strided')
    L.check(lib.cnnq_pc_minmax_params(_ptr(pmm), G, Cs, int(num_bits), int(bool(positive)), _ptr(qp), st),
            'cnnq_pc_minmax_params')
    L.check(lib.cnnq_pc_qdq_strided(_slice_ptr(x, c0, HW), _slice_ptr(y, c0, HW), N, Cs, HW, stride, _ptr(qp), None,
                                    None, 1, st), 'cnnq_pc_qdq_strided')
    return y


def quantize_pack4(x, qp):
    """x [N, C, H, W] + parameter table -> packed int4 codes (uint8, numel/2 bytes, two codes per byte)."""
    lib = L.load()
    x = _dev(x, 'x')
    N, C, HW = geometry(x)
    packed = torch.empty(x.numel() // 2, dtype=torch.uint8, device=x.device)
    L.check(lib.cnnq_pc_quantize_pack4(_ptr(x), _ptr(packed), N, C, HW, _ptr(qp), _stream(x)), 'cnnq_pc_quantize_pack4')
    return packed


def dequantize_pack4(packed, shape, qp):
    """Inverse of quantize_pack4: the dequantized fp32 tensor (bit-identical to pc_qdq's output)."""
    lib = L.load()
    y = torch.empty(shape, dtype=torch.float32, device=packed.device)
    N, C, HW = geometry(y)
    L.check(lib.cnnq_pc_dequantize_pack4(_ptr(packed), _ptr(y), N, C, HW, _ptr(qp), _stream(y)),
            'cnnq_pc_dequantize_pack4')
    return y


def quantize_u8(x, qp):
    """x [N, C, H, W] + parameter table -> uint8 codes (one byte each, numel bytes): the stored format for
    quantizations of up to 8 bits."""
    lib = L.load()
    x = _dev(x, 'x')
    N, C, HW = geometry(x)
    codes = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    L.check(lib.cnnq_pc_quantize_u8(_ptr(x), _ptr(codes), N, C, HW, _ptr(qp), _stream(x)), 'cnnq_pc_quantize_u8')
    return codes


def dequantize_u8(codes, qp):
    """Inverse of quantize_u8: the dequantized fp32 tensor (bit-identical to pc_qdq's output)."""
    lib = L.load()
    y = torch.empty(codes.shape, dtype=torch.float32, device=codes.device)
    N, C, HW = geometry(y)
    L.check(lib.cnnq_pc_dequantize_u8(_ptr(codes), _ptr(y), N, C, HW, _ptr(qp), _stream(y)), 'cnnq_pc_dequantize_u8')
    return y


def packed_capacity(shape):
    """Worst-case bytes of the packed format for an activation of this shape (every channel at 8 bits)."""
    N, C = shape[0], shape[1]
    HW = 1
    for d in shape[2:]:
        HW *= d
    return N * C * ((HW * 8 + 31) // 32 * 4)


def packed_layout(bits, HW):
    """rowoff int32 [C + 1] of the packed format for per-channel widths `bits` and H*W elements per row
    (cnnq_pc_packed_layout): row (n, c) starts at byte n * rowoff[C] + rowoff[c].  A function of the parameters only - with
    a fixed bit allocation it is computed once and handed to quantize_packed / dequantize_packed."""
    lib = L.load()
    bits = bits.contiguous()
    C = bits.numel()
    rowoff = torch.empty(C + 1, dtype=torch.int32, device=bits.device)
    L.check(lib.cnnq_pc_packed_layout(_ptr(bits), C, int(HW), _ptr(rowoff), _stream(bits)), 'cnnq_pc_packed_layout')
    return rowoff


def quantize_packed(x, qp, bits, out=None, form=0, rowoff=None):
    """x [N, C, H, W] + parameter table + per-channel bit widths (diag[DIAG_BITS] of pc_params with bit
    allocation) -> (packed uint8 [N * bytes_per_sample], rowoff int32 [C + 1]): bits[c] bits per code, i.e.
    sum(bits)/8 bytes per spatial position (cnnq_pc_quantize_packed).  Sizing the buffer exactly takes one host
    read of rowoff[C]; with `out` (a uint8 buffer of at least packed_capacity(x.shape) bytes) nothing synchronises
    and the whole buffer is returned (the used prefix is N * rowoff[C] bytes).  form: 0 = the library's choice, 1 = the
    general kernel, 2 = the lean kernel (cnnq_pc_quantize_packed_form); every form writes the same bytes.  rowoff: the
    layout of packed_layout(bits, H * W) when the caller already has it (one launch less)."""
    lib = L.load()
    x = _dev(x, 'x')
    N, C, HW = geometry(x)
    bits = bits.contiguous()
    if rowoff is None:
        rowoff = torch.empty(C + 1, dtype=torch.int32, device=x.device)
        L.check(lib.cnnq_pc_packed_layout(_ptr(bits), C, HW, _ptr(rowoff), _stream(x)), 'cnnq_pc_packed_layout')
    elif not (rowoff.is_cuda and rowoff.dtype == torch.int32 and rowoff.is_contiguous() and rowoff.numel() == C + 1):
        raise L.CnnqError('rowoff must be the int32 device tensor [C + 1] of packed_layout(bits, H * W)')
    if out is not None:
        if not (out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.numel() >= packed_capacity(x.shape)):
            raise L.CnnqError('out must be a contiguous uint8 device buffer of at least packed_capacity(x.shape) bytes')
        packed, plane = out, None
    else:
        plane = int(rowoff[C].item())
        packed = torch.empty(max(N * plane, 4), dtype=torch.uint8, device=x.device)
    L.check(lib.cnnq_pc_quantize_packed_form(_ptr(x), _ptr(packed), N, C, HW, _ptr(qp), _ptr(bits), _ptr(rowoff), int(form),
                                             _stream(x)), 'cnnq_pc_quantize_packed')
    return (packed if plane is None else packed[:N * plane]), rowoff


def dequantize_packed(packed, shape, qp, bits, rowoff, out=None, form=0):
    """Inverse of quantize_packed: the dequantized fp32 tensor (bit-identical to pc_qdq's output).  form as in
    quantize_packed (cnnq_pc_dequantize_packed_form)."""
    lib = L.load()
    y = torch.empty(shape, dtype=torch.float32, device=packed.device) if out is None else out
    if out is not None and not (out.is_cuda and out.dtype == torch.float32 and out.is_contiguous()
                                and tuple(out.shape) == tuple(shape)):
        raise L.CnnqError('out must be a contiguous float32 device tensor of the given shape')
    N, C, HW = geometry(y)
    L.check(lib.cnnq_pc_dequantize_packed_form(_ptr(packed), _ptr(y), N, C, HW, _ptr(qp), _ptr(bits.contiguous()),
                                               _ptr(rowoff), int(form), _stream(y)), 'cnnq_pc_dequantize_packed')
    return y


# ------------------------------------------------------------------------------------- stored codes on channels_last storage
# the packed format of a dense channels_last activation of fp32 / bf16 / fp16 - row r of [R = N*H*W][C] is
# one little-endian bit stream, channel c at bits [coloff[c], coloff[c] + bits[c]), padded to whole dwords.  These functions take
# the storage as it is or raise: no copy, no upcast (LAYOUT_COPIES never moves here).
def _packed_x(x, what):
    """x as the packed channels_last entry points take it: a dense channels_last 4-D fp32 / bf16 / fp16 tensor on the current device."""
    if not isinstance(x, torch.Tensor):
        raise L.CnnqError('%s: x must be a tensor' % what)
    if x.dtype not in _ACT_DTYPES:
        raise L.CnnqError('%s: x must be float32, bfloat16 or float16, got %s' % (what, x.dtype))
    if x.dim() != 4 or _layout(x) != 'nhwc':             # shape and strides only
        raise L.CnnqError('%s: x must be a dense channels_last 4-D activation (no copy is made here)' % what)
    if not x.is_cuda:
        raise L.CnnqError('%s: x must be a CUDA/HIP tensor (there is no CPU path)' % what)
    if x.device.index != torch.cuda.current_device():
        raise L.CnnqError('%s: x is on %s but the current device is cuda:%d' % (what, x.device, torch.cuda.current_device()))
    return x.detach() if x.requires_grad else x


def _packed_table(t, what, dtype, shape, device):
    if not _is_table(t, dtype, shape, device):
        raise L.CnnqError('%s must be a contiguous %s device tensor of shape %s' % (what, str(dtype).replace('torch.', ''), list(shape)))
    return t


def _packed_rowbytes(bits, C):
    return (int(bits) * C + 31) // 32 * 4


def _packed_buffer(out, nbytes, device, what):
    """The code buffer and what the caller gets back: a new one, cut to exactly nbytes, or the caller's (returned whole) - uint8,
    contiguous, 4-byte aligned, at least nbytes long."""
    if out is None:
        buf = torch.empty(max(nbytes, 4), dtype=torch.uint8, device=device)      # never empty: the C side refuses a null pointer
        return buf, buf[:nbytes]
    if not (isinstance(out, torch.Tensor) and out.is_cuda and out.device == device and out.dtype == torch.uint8 and out.is_contiguous()
            and out.numel() >= max(nbytes, 1) and out.data_ptr() % 4 == 0):
        raise L.CnnqError('%s: out must be a contiguous, 4-byte aligned uint8 device buffer of at least %d bytes' % (what, nbytes))
    return out, out


def _uniform_width(bits, what):
    if isinstance(bits, bool) or not isinstance(bits, int):
        return None
    if not 0 <= bits <= 8:
        raise L.CnnqError('%s: a uniform width must be in 0..8, got %d' % (what, bits))
    return bits


def packed_capacity_nhwc(shape):
    """Worst-case bytes of the channels_last packed format for an activation of this shape (every channel at 8 bits):
    cnnq_pc_packed_nhwc_capacity, R * 4 * ceil(8 * C / 32)."""
    C = int(shape[1])
    R = 1
    for d in tuple(shape[:1]) + tuple(shape[2:]):
        R *= int(d)
    return R * ((8 * C + 31) // 32 * 4)


def packed_layout_nhwc(bits, C, device=None):
    """coloff int32 [C + 1] of the channels_last packed format (cnnq_pc_packed_layout_nhwc): the exclusive prefix sum of the
    per-channel widths `bits` (a float32 device table of C entries, e.g. diag[DIAG_BITS]) or of one integer width 0..8 for every
    channel.  A function of the widths only: computed once, it serves every quantize / dequantize call with them."""
    lib = L.load()
    C = int(C)
    uni = _uniform_width(bits, 'packed_layout_nhwc')
    if uni is None:
        device = bits.device if isinstance(bits, torch.Tensor) else None
        bits = _packed_table(bits, 'bits', torch.float32, (C,), device)
    elif device is None:
        device = torch.device('cuda', torch.cuda.current_device())
    coloff = torch.empty(C + 1, dtype=torch.int32, device=device)
    L.check(lib.cnnq_pc_packed_layout_nhwc(None if uni is not None else _ptr(bits), uni or 0, C, _ptr(coloff), _stream(coloff)),
            'cnnq_pc_packed_layout_nhwc')
    return coloff


def quantize_packed_nhwc(x, qp, bits, mm=None, out=None, coloff=None):
    """A dense channels_last x + parameter table qp [NQP, C] + widths -> (packed uint8, coloff int32 [C + 1])
    (cnnq_pc_quantize_packed_nhwc, one launch on the storage as it is).  bits: an integer 0..8 for every channel - the buffer is
    sized exactly on the host, R * 4 * ceil(bits * C / 32) bytes - or a float32 device table [C] (diag[DIAG_BITS]): a buffer of
    packed_capacity_nhwc(x.shape) bytes comes back, of which R * 4 * ceil(coloff[C] / 32) are used, and nothing synchronises.
    mm: the channels' exact extrema [2, C] (config 2's), or None; the bytes do not depend on it.  out: the caller's buffer, returned
    whole.  coloff: packed_layout_nhwc(bits, C) when the caller already has it (one launch less)."""
    lib = L.load()
    x = _packed_x(x, 'quantize_packed_nhwc')
    C = x.shape[1]
    R = x.numel() // C
    qp = _packed_table(qp, 'qp', torch.float32, (L.NQP, C), x.device)
    if mm is not None:
        mm = _packed_table(mm, 'mm', torch.float32, (2, C), x.device)
    uni = _uniform_width(bits, 'quantize_packed_nhwc')
    if coloff is None:
        coloff = packed_layout_nhwc(bits, C, x.device)
    else:
        coloff = _packed_table(coloff, 'coloff', torch.int32, (C + 1,), x.device)
    nbytes = R * _packed_rowbytes(uni, C) if uni is not None else packed_capacity_nhwc(x.shape)
    buf, packed = _packed_buffer(out, nbytes, x.device, 'quantize_packed_nhwc')
    L.check(lib.cnnq_pc_quantize_packed_nhwc(_ptr(x), _DTYPE_CODES[x.dtype], R, C, _ptr(qp), _ptr(mm), _ptr(coloff),
                                             _ptr(buf), _stream(x)), 'cnnq_pc_quantize_packed_nhwc')
    return packed, coloff


def dequantize_packed_nhwc(packed, shape, dtype, qp, coloff, out=None):
    """Inverse of quantize_packed_nhwc (cnnq_pc_dequantize_packed_nhwc): a dense channels_last tensor of `shape` and `dtype`
    (float32 / bfloat16 / float16) holding (code - zp) * scale - pc_qdq's result on the channels_last x with the same qp, bit for bit
    (a NaN element of a channel with finite parameters, stored as code 0, excepted)."""
    lib = L.load()
    if not isinstance(packed, torch.Tensor) or not packed.is_cuda:
        raise L.CnnqError('dequantize_packed_nhwc: packed must be a CUDA/HIP tensor (there is no CPU path)')
    if dtype not in _ACT_DTYPES:
        raise L.CnnqError('dequantize_packed_nhwc: dtype must be float32, bfloat16 or float16, got %s' % (dtype,))
    shape = tuple(int(d) for d in shape)
    if len(shape) != 4:
        raise L.CnnqError('dequantize_packed_nhwc: shape must be that of a 4-D activation')
    if not (packed.dtype == torch.uint8 and packed.is_contiguous() and packed.data_ptr() % 4 == 0):
        raise L.CnnqError('dequantize_packed_nhwc: packed must be a contiguous, 4-byte aligned uint8 buffer')
    if packed.device.index != torch.cuda.current_device():
        raise L.CnnqError('dequantize_packed_nhwc: packed is on %s but the current device is cuda:%d' % (packed.device, torch.cuda.current_device()))
    C = shape[1]
    qp = _packed_table(qp, 'qp', torch.float32, (L.NQP, C), packed.device)
    coloff = _packed_table(coloff, 'coloff', torch.int32, (C + 1,), packed.device)
    if out is None:
        y = torch.empty(shape, dtype=dtype, device=packed.device, memory_format=torch.channels_last)
    else:
        y = out
        if not (isinstance(y, torch.Tensor) and y.is_cuda and y.device == packed.device and y.dtype == dtype and tuple(y.shape) == shape
                and y.is_contiguous(memory_format=torch.channels_last)):
            raise L.CnnqError('dequantize_packed_nhwc: out must be a dense channels_last %s tensor of the given shape' % str(dtype).replace('torch.', ''))
    R = y.numel() // C
    # an empty buffer (every width 0) has no address; nothing is read through the pointer then
    L.check(lib.cnnq_pc_dequantize_packed_nhwc(ctypes.c_void_p(packed.data_ptr() or y.data_ptr()), _ptr(y), _DTYPE_CODES[dtype], R, C,
                                               _ptr(qp), _ptr(coloff), _stream(y)), 'cnnq_pc_dequantize_packed_nhwc')
    return y


def minmax_quantize_packed_nhwc(x, num_bits=4, positive=False, out=None):
    """Config 2 straight into the stored format (cnnq_pc_minmax_quantize_packed_nhwc): per-channel min / max of a dense
    channels_last x, the parameter table, the uniform num_bits (1..8) layout and the packed codes, one host call ->
    (packed uint8 [R * 4 * ceil(num_bits * C / 32)], dict(qp, mm, coloff))."""
    lib = L.load()
    x = _packed_x(x, 'minmax_quantize_packed_nhwc')
    if not 1 <= int(num_bits) <= 8:
        raise L.CnnqError('minmax_quantize_packed_nhwc: num_bits must be in 1..8, got %r' % (num_bits,))
    C = x.shape[1]
    R = x.numel() // C
    dt = _DTYPE_CODES[x.dtype]
    st = _raw_stream(x.device.index)
    ws = _scratch(x, 'nhwc', _ws_bytes('nhwc', R, C, 1, dt), st).data_ptr()
    qp = torch.empty(L.NQP, C, dtype=torch.float32, device=x.device)
    mm = torch.empty(2, C, dtype=torch.float32, device=x.device)
    coloff = torch.empty(C + 1, dtype=torch.int32, device=x.device)
    buf, packed = _packed_buffer(out, R * _packed_rowbytes(num_bits, C), x.device, 'minmax_quantize_packed_nhwc')
    rc = lib.cnnq_pc_minmax_quantize_packed_nhwc(x.data_ptr(), dt, R, C, int(num_bits), 1 if positive else 0, ws, qp.data_ptr(),
                                                 mm.data_ptr(), coloff.data_ptr(), buf.data_ptr(), st)
    if rc:
        L.check(rc, 'cnnq_pc_minmax_quantize_packed_nhwc')
    return packed, dict(qp=qp, mm=mm, coloff=coloff)


def aciq_quantize_packed_nhwc(x, num_bits, positive=False, clip='laplace', bit_alloc=False, prior_is_b=False, target=None,
                              round_mode=True, out=None):
    """Config 3 straight into the stored format (cnnq_pc_aciq_quantize_packed_nhwc): aciq_qdq_nhwc's statistics and parameters of a
    dense channels_last x, then the packed codes instead of y, one host call -> (packed uint8, dict(stats, qp, diag, coloff)).  With
    bit allocation the widths are diag[DIAG_BITS] - a buffer of packed_capacity_nhwc(x.shape) bytes comes back, of which
    R * 4 * ceil(coloff[C] / 32) are used, and nothing synchronises; without it the width is num_bits (<= 8) and the buffer exact."""
    if clip not in ('laplace', 'gaus'):
        raise L.CnnqError("aciq_quantize_packed_nhwc: clip must be 'laplace' or 'gaus', got %r" % (clip,))
    lib = L.load()
    x = _packed_x(x, 'aciq_quantize_packed_nhwc')
    if not 1 <= int(num_bits) <= 8:
        raise L.CnnqError('aciq_quantize_packed_nhwc: num_bits must be in 1..8, got %r' % (num_bits,))
    use_ba = bool(bit_alloc) and num_bits <= 4
    C = x.shape[1]
    R = x.numel() // C
    dt = _DTYPE_CODES[x.dtype]
    st = _raw_stream(x.device.index)
    cfg = _params_cfg(num_bits, positive, clip, use_ba, prior_is_b, target, round_mode, False)
    ws = _scratch(x, 'aciq_nhwc', _ws_bytes('aciq_nhwc', R, C, 1, dt), st).data_ptr()
    tabs = torch.empty(L.NSTAT + L.NQP + L.NDIAG, C, dtype=torch.float32, device=x.device)
    coloff = torch.empty(C + 1, dtype=torch.int32, device=x.device)
    nbytes = packed_capacity_nhwc(x.shape) if use_ba else R * _packed_rowbytes(num_bits, C)
    buf, packed = _packed_buffer(out, nbytes, x.device, 'aciq_quantize_packed_nhwc')
    tp = tabs.data_ptr()
    rc = lib.cnnq_pc_aciq_quantize_packed_nhwc(x.data_ptr(), dt, R, C, ctypes.byref(cfg), ws, tp, tp + L.NSTAT * C * 4,
                                               tp + (L.NSTAT + L.NQP) * C * 4, coloff.data_ptr(), buf.data_ptr(), st)
    if rc:
        L.check(rc, 'cnnq_pc_aciq_quantize_packed_nhwc')
    return packed, dict(stats=tabs[:L.NSTAT], qp=tabs[L.NSTAT:L.NSTAT + L.NQP], diag=tabs[L.NSTAT + L.NQP:], coloff=coloff)


def entropy_from_hist(hist):
    """Shannon entropy (bits) of an int64 histogram tensor -> 0-dim float32 tensor on the device."""
    lib = L.load()
    out = torch.empty(1, dtype=torch.float32, device=hist.device)
    L.check(lib.cnnq_entropy(_ptr(hist), hist.numel(), _ptr(out), _stream(hist)), 'cnnq_entropy')
    return out[0]


def pt_setup(device, num_bits, range_offset=None, stats=None, rows=0, rows_mode=0, zero_min=False,
             int_exp=False, enforce_true_zero=True):
    """Per-tensor parameters ptp[8] on the device from host scalars or from per-row stats."""
    lib = L.load()
    ptp = torch.empty(8, dtype=torch.float32, device=device)
    ro = None
    if range_offset is not None:
        ro = (ctypes.c_float * 2)(float(range_offset[0]), float(range_offset[1]))
    stride = stats.shape[1] if stats is not None else 0
    L.check(lib.cnnq_pt_setup(ro, _ptr(stats), stride, int(rows), int(rows_mode), int(bool(zero_min)),
                              int(num_bits), int(bool(int_exp)), int(bool(enforce_true_zero)), _ptr(ptp),
                              _stream(ptp)), 'cnnq_pt_setup')
    return ptp


def pt_qdq(x, ptp, noise=None, out=None):
    lib = L.load()
    # element by element: a dense channels_last x is quantized in its storage order, y has its layout (the noise of
    # stochastic rounding is indexed in NCHW order: that route keeps the copy)
    x = _dev_act(x, 'x') if noise is not None else _dev_act_layout(x, 'x')
    y = _out_like(x, out)
    if noise is not None:
        noise = _dev(noise, 'noise')
    if x.numel() == 0:
        return y
    if x.dtype != torch.float32:
        L.check(lib.cnnq_pt_qdq_dt(_ptr(x), _ptr(y), _HALF_DTYPES[x.dtype], x.numel(), _ptr(ptp), _ptr(noise), _stream(x)),
                'cnnq_pt_qdq_dt')
        return y
    L.check(lib.cnnq_pt_qdq(_ptr(x), _ptr(y), x.numel(), _ptr(ptp), _ptr(noise), _stream(x)), 'cnnq_pt_qdq')
    return y


# ------------------------------------------------------------------------------------- pipelines
def act_qdq_per_channel(x, num_bits, positive=False, clip='no', bit_alloc=False, prior_is_b=False, target=None,
                        round_mode=True, per_channel_dim=1, group=None, want_codes=False, want_parts=False,
                        stats=None, want_entropy=False, whole_tensor=False, out=None, bcorr=None):
    """The dynamic per-channel hot path end to end: statistics (one or two coalesced reads of
    x) -> parameters (one workgroup) -> fused Q/DQ (one read, one write).  Covers iq.py:409-451
    (clip='no'), iq.py:327-352 (ACIQ) and, with per_channel_dim=0, the weights of iq.py:453-476;
    whole_tensor=True treats the tensor as ONE channel (per-tensor clipping, iq.py:353-357).
    `stats` (optional [NSTAT, C] table, e.g. from a calibration file) replaces the dynamic
    statistics.  group=False: never exchange (replicated data such as weights).
    bcorr (None, or the relu-first flag): also apply the activation bias correction of iqm.py:180-196,
    fused into the passes where the parameter table is at hand (qdq_bias_corrected).
    Returns y [, codes] [, entropy (0-dim device tensor)] [, parts].  No host synchronisation."""
    use_ba = bool(bit_alloc) and num_bits <= 4 and not whole_tensor
    # config 2, dynamic on one GPU or from a statistics table, keeps a dense channels_last x as it is - also
    # with the entropy of its codes when they fit a byte (section 17; a sharded batch sums the ranks' counts: the NCHW route)
    nhwc = (per_channel_dim == 1 and not whole_tensor and clip == 'no' and not use_ba and bcorr is None
            and not (want_codes or want_parts) and (stats is not None or not _sharded(group))
            and not (want_entropy and (num_bits > 8 or _sharded(group))))
    x = _dev_act_layout(x, 'x') if nhwc else _dev_act(x, 'x')
    N, C, HW = (1, 1, x.numel()) if whole_tensor else geometry(x, per_channel_dim)
    if _is_nhwc(x) and want_entropy:
        st = _raw_stream(x.device.index)
        x, slot = _nhwc_hist_slot(x, 'act_qdq_per_channel', st)
        if slot is not None:
            if stats is None:
                return _minmax_qdq_nhwc(x, num_bits, positive, out, slot, st)
            qp, _ = pc_params(stats, num_bits, positive, clip, use_ba, prior_is_b, target, round_mode)
            return _pc_qdq_nhwc(x, qp, out, _hist_bins(num_bits, use_ba), slot, st)
    if _is_nhwc(x):
        if stats is None:
            return _minmax_qdq_nhwc(x, num_bits, positive, out)
        qp, _ = pc_params(stats, num_bits, positive, clip, use_ba, prior_is_b, target, round_mode)
        return _pc_qdq_nhwc(x, qp, out)
    if x.dtype != torch.float32:
        # bf16 / fp16: config 2, dynamic or from a statistics table - min/max parameters, no clipping, no bit allocation; with the
        # entropy of its codes where they fit a byte, on one GPU
        if (clip != 'no' or use_ba or whole_tensor or per_channel_dim != 1 or bcorr is not None or want_codes or want_parts
                or (want_entropy and (num_bits > 8 or _sharded(group)))):
            _half_only('act_qdq_per_channel', 'clipping / bit allocation / whole-tensor / weights / bias correction / codes')
        if stats is None:
            return minmax_qdq_fused(x, N, C, HW, num_bits, positive, want_entropy=want_entropy, out=out, group=group, _checked=True)
        qp, _ = pc_params(stats, num_bits, positive, clip, use_ba, prior_is_b, target, round_mode, direct_range=whole_tensor)
        if want_entropy:
            return _pc_qdq_half_entropy(x, N, C, HW, qp, _hist_bins(num_bits, use_ba), out)
        return pc_qdq(x, N, C, HW, qp, out=out)
    if bcorr is not None and (want_codes or want_entropy or want_parts or whole_tensor or per_channel_dim != 1):
        raise L.CnnqError('bcorr combines only with the plain per-channel activation Q/DQ')
    if stats is None and clip == 'no' and not use_ba and not whole_tensor:
        res = minmax_qdq_fused(x, N, C, HW, num_bits, positive, want_codes, want_entropy, out=out,
                               want_parts=want_parts, group=group, _checked=True)
        if bcorr is not None:
            res = act_bias_correction_(x, res, bool(bcorr), group=None if group is False else group)
        return res
    # Laplace clipping with dynamic statistics on one GPU: pass B, the parameters and the Q/DQ in ONE launch that reads
    # x once (cnnq_pc_aciq_qdq_single: 12 instead of 16 bytes per element) when the shape has a single-launch plan
    exchanging = _sharded(group)
    single = (_ACIQ_SINGLE and _RESIDENT and stats is None and bcorr is None and clip == 'laplace'
              and not whole_tensor and not (use_ba and prior_is_b) and num_bits <= 8)
    if single and exchanging and not (want_codes or want_entropy):
        # sharded: the ranks' sums meet inside the single launch; None: no in-launch exchange for this group - the chain
        cfg = _params_cfg(num_bits, positive, clip, use_ba, prior_is_b, target, round_mode, whole_tensor)
        res = _aciq_qdq_xrank(x, N, C, HW, cfg, group, want_parts, out)
        if res is not None:
            return res
    single = single and not exchanging
    if (stats is None and not exchanging and bcorr is None and not (want_codes or want_entropy or want_parts)):
        # one host call for the whole pipeline (cnnq_pc_aciq_qdq_auto: four launches through the single-launch kernel,
        # else the five of the chain), one cached workspace (statistics partials, then the parameter and diagnostic
        # tables, which nobody outside the call reads)
        lib = L.load()
        cfg = _params_cfg(num_bits, positive, clip, use_ba, prior_is_b, target, round_mode, whole_tensor)
        y = _out_like(x, out)
        nbytes = _ws_bytes('aciq', N, C, HW, int(x.data_ptr() % 16 == 0))
        st = _raw_stream(x.device.index)
        base = _scratch(x, 'aciq', nbytes + (L.NQP + L.NDIAG) * C * 4, st).data_ptr()
        qd = base + nbytes
        gws = _group_workspace(x, st) if single else None
        if gws is not None:
            rc = lib.cnnq_pc_aciq_qdq_auto(x.data_ptr(), y.data_ptr(), N, C, HW, ctypes.byref(cfg), base, gws, GROUP_WS_BYTES, qd,
                                           qd + L.NQP * C * 4, st)
        else:
            rc = lib.cnnq_pc_aciq_qdq(x.data_ptr(), y.data_ptr(), N, C, HW, ctypes.byref(cfg), base, qd, qd + L.NQP * C * 4, st)
        if rc:
            L.check(rc, 'cnnq_pc_aciq_qdq')
        return y
    if single:
        res = aciq_qdq_single(x, N, C, HW, num_bits, positive, use_ba, target, round_mode, want_codes, want_entropy, want_parts,
                              out=out)
        if res is not None:
            return res
    if stats is None:
        need_b = (clip == 'laplace') or (use_ba and prior_is_b)
        stats, _ = pc_stats(x, N, C, HW, need_b=need_b, group=None if group is False else group,
                            local_only=group is False)
    qp, diag = pc_params(stats, num_bits, positive, clip, use_ba, prior_is_b, target, round_mode,
                         direct_range=whole_tensor)
    if bcorr is not None:
        return qdq_bias_corrected(x, N, C, HW, qp, bool(bcorr), group=None if group is False else group, out=out)
    hist = torch.zeros(256, dtype=torch.int64, device=x.device) if want_entropy else None
    y = pc_qdq(x, N, C, HW, qp, want_codes, out=out, hist=hist)
    y, codes = y if want_codes else (y, None)
    entropy = None
    if want_entropy:
        if group is not False and D.world_size(group) > 1:
            D.all_reduce_sum_(hist, group)
        entropy = entropy_from_hist(hist)
    return _result(y, codes, entropy, dict(stats=stats, qp=qp, diag=diag) if want_parts else None)


def _aciq_qdq_native(site, x, what, num_bits, positive, clip, bit_alloc, prior_is_b, target, round_mode, stats, out, want_parts, slot,
                     allow=1):
    """Config 3 (iq.py:327-352 -> 409-451: ACIQ clipping 'laplace' / 'gaus', optionally bit allocation) of a tensor on its site:
    the statistics, the parameters and the Q/DQ in one host call with one cached workspace (cnnq_pc_aciq_qdq_nhwc /
    cnnq_pc_aciq_qdq_dt; allow: the allow_single_launch word of a layout that takes one) - or, with `stats` (a float32 [NSTAT, C]
    device table, -sm use), pc_params and the table-driven Q/DQ.  y has x's layout and dtype; want_parts: (y, dict(stats, qp,
    diag)).  One GPU: the statistics are this tensor's.  slot (the replica tables of a want_entropy call): the Q/DQ pass counts its
    codes into them (cnnq_pc_aciq_qdq_hist_*, or cnnq_pc_qdq_hist_* with `stats`) and the entropy follows y as
    act_qdq_per_channel returns it - y, entropy [, parts]; inside an entropy_batch block it is filled by the block's one launch."""
    layout, geo, C, dt, st = site
    use_ba = bool(bit_alloc) and num_bits <= 4
    if stats is not None:
        if not _is_table(stats, torch.float32, (L.NSTAT, C), x.device):
            raise L.CnnqError('%s: stats must be a contiguous float32 [%d, %d] device table' % (what, L.NSTAT, C))
        qp, diag = pc_params(stats, num_bits, positive, clip, use_ba, prior_is_b, target, round_mode)
        parts = dict(stats=stats, qp=qp, diag=diag) if want_parts else None
        if slot is None:
            return _result(_qdq_native(site, x, qp, out), parts=parts)
        y, entropy = _qdq_native(site, x, qp, out, _hist_bins(num_bits, use_ba), slot)
        return _result(y, entropy=entropy, parts=parts)
    fn, fn_hist, kind = layout['aciq']
    cfg = _params_cfg(num_bits, positive, clip, use_ba, prior_is_b, target, round_mode, False)
    nbytes = _ws_bytes(kind, *geo, *layout['ws_pad'], dt)
    y = _out_like(x, out)
    if want_parts:
        tabs = torch.empty(L.NSTAT + L.NQP + L.NDIAG, C, dtype=torch.float32, device=x.device)
        ws, tp = _scratch(x, kind, nbytes, st).data_ptr(), tabs.data_ptr()
        parts = dict(stats=tabs[:L.NSTAT], qp=tabs[L.NSTAT:L.NSTAT + L.NQP], diag=tabs[L.NSTAT + L.NQP:])
    else:
        # the tables nobody outside the call reads follow the records in the cached workspace
        ws = _scratch(x, kind, nbytes + (L.NSTAT + L.NQP + L.NDIAG) * C * 4, st).data_ptr()
        tp, parts = ws + nbytes, None
    if slot is not None:
        rc = getattr(L.load(), fn_hist)(x.data_ptr(), y.data_ptr(), dt, *geo, ctypes.byref(cfg), ws, tp, tp + L.NSTAT * C * 4,
                                        tp + (L.NSTAT + L.NQP) * C * 4, slot[0].data_ptr(), st)
    else:
        rc = getattr(L.load(), fn)(x.data_ptr(), y.data_ptr(), dt, *geo, ctypes.byref(cfg), ws, tp, tp + L.NSTAT * C * 4,
                                   tp + (L.NSTAT + L.NQP) * C * 4, *((allow,) if layout['single'] else ()), st)
    if rc:
        L.check(rc, fn)
    return _result(y, entropy=_replica_entropy(x, slot[0], slot[1], st) if slot is not None else None, parts=parts)


def aciq_qdq_nhwc(x, num_bits, positive=False, clip='laplace', bit_alloc=False, prior_is_b=False, target=None, round_mode=True,
                  stats=None, out=None, want_parts=False, want_entropy=False):
    """_aciq_qdq_native on a dense channels_last activation of fp32 / bf16 / fp16, on the storage as it is:
    the statistics over slabs of rows.  A tensor that is not dense channels_last (or CNNQ_NHWC=0: copied, counted) takes
    act_qdq_per_channel, `stats` as it is.  want_entropy: who takes the counted copy instead of counting
    native: _nhwc_hist_slot."""
    if clip not in ('laplace', 'gaus'):
        raise L.CnnqError("aciq_qdq_nhwc: clip must be 'laplace' or 'gaus', got %r" % (clip,))
    if want_entropy and num_bits > 8:
        raise L.CnnqError('aciq_qdq_nhwc: the ACIQ factor tables end at 8 bits')
    x, site = _admit_nhwc(x, 'aciq_qdq_nhwc', dev_first=True)
    slot = None
    if want_entropy and site is not None:
        x, slot = _nhwc_hist_slot(x, 'aciq_qdq_nhwc', site[4])
        if slot is None:
            site = None
    if site is None:
        return act_qdq_per_channel(x, num_bits, positive, clip, bit_alloc, prior_is_b, target, round_mode, group=False,
                                   want_parts=want_parts, stats=stats, out=out, want_entropy=want_entropy)
    return _aciq_qdq_native(site, x, 'aciq_qdq_nhwc', num_bits, positive, clip, bit_alloc, prior_is_b, target, round_mode, stats, out,
                            want_parts, slot)


_ACIQ_HALF_NATIVE = {}


def _aciq_half_native(N, C, HW, dtype, bit_alloc=False, prior_is_b=False):
    """The route word of cnnq_pc_route_aciq_dt's report for this class of contiguous bf16 / fp16 layer and bit allocation
    (bit_alloc: in effect, i.e. at 4 bits or fewer): 1 - dynamic ACIQ in one launch, 3 - pass A and the bit allocation in front of
    it, 2 - the chain, 0 - a class that measured slower native than through the upcast and is sent back there.  The quantizer
    (_half_aciq) and the tests patch the function and empty the cache by name."""
    cfg = _params_cfg(4, False, 'laplace', bit_alloc, prior_is_b, None, True, False)
    cache = _ACIQ_HALF_NATIVE.setdefault((bool(bit_alloc), bool(prior_is_b)), {})
    return _route_word(cache, (N, C, HW, dtype), int, 'cnnq_pc_route_aciq_dt', (N, C, HW), dtype, (ctypes.byref(cfg), 1))


def aciq_qdq_half(x, num_bits, positive=False, clip='laplace', bit_alloc=False, prior_is_b=False, target=None, round_mode=True,
                  stats=None, out=None, want_parts=False, single_launch=None, want_entropy=False):
    """_aciq_qdq_native on a contiguous 4-D bf16 / fp16 activation, on the storage as it is: the statistics,
    the parameters and the Q/DQ in one launch where a channel's batch population fits one workgroup's registers (behind pass A and
    the bit allocation with -baa), else the chain of cnnq_pc_stats_dt, cnnq_pc_params and cnnq_pc_qdq_dt.  single_launch: None -
    the route function's choice; 0 - the chain; 2 - the resident form wherever the channel fits (the chain elsewhere), for tests
    and A/B.  Anything else - a CPU tensor, float32, not 4-D, not contiguous - raises: nothing is copied or upcast here.
    want_entropy: the counting pass is the chain's, whatever single_launch says."""
    what = 'aciq_qdq_half'
    if clip not in ('laplace', 'gaus'):
        raise L.CnnqError("%s: clip must be 'laplace' or 'gaus', got %r" % (what, clip))
    if want_entropy and num_bits > 8:
        raise L.CnnqError('%s: the ACIQ factor tables end at 8 bits' % what)
    x, site = _admit_half(x, what, 'act_qdq_per_channel')
    if stats is None and single_launch not in (None, 0, 1, 2):
        raise L.CnnqError('%s: single_launch must be None, 0, 1 or 2, got %r' % (what, single_launch))
    # (the counting pass of a table-driven call reports a missing replica table under pc_qdq's name)
    slot = _half_hist_slot(x, what if stats is None else 'pc_qdq', site[4]) if want_entropy else None
    return _aciq_qdq_native(site, x, what, num_bits, positive, clip, bit_alloc, prior_is_b, target, round_mode, stats, out, want_parts,
                            slot, 1 if single_launch is None or stats is not None else int(single_launch))


def weight_correction(w, w_q, vcorr=False, bcorr=False):
    """Per-output-channel variance / mean correction of quantized weights (iqm.py:374-391).
    Returns a new tensor; weights are replicated across ranks, so no exchange."""
    if not (vcorr or bcorr):
        return w_q
    lib = L.load()
    w = _dev(w, 'w')
    out = _dev(w_q, 'w_q').clone()
    C, HW = w.shape[0], w.numel() // w.shape[0]
    st_w, _ = pc_stats(w, 1, C, HW, local_only=True)
    st_q, _ = pc_stats(out, 1, C, HW, local_only=True)
    L.check(lib.cnnq_pc_weight_correct(_ptr(out), C, HW, _ptr(st_w), _ptr(st_q), int(bool(vcorr)), int(bool(bcorr)),
                                       _stream(out)), 'cnnq_pc_weight_correct')
    return out.view(w_q.shape)


def act_bias_correction_(out, out_q, relu_first, group=None):
    """Activation bias correction (iqm.py:180-196), IN PLACE on out_q; `out` is the unquantized
    activation.  With world size > 1 the per-channel sums are exchanged so the bias is global."""
    lib = L.load()
    x = _dev(out, 'out')
    if not (isinstance(out_q, torch.Tensor) and out_q.is_cuda and out_q.is_contiguous() and out_q.dtype == torch.float32):
        raise L.CnnqError('out_q must be a contiguous float32 device tensor')
    N, C, HW = geometry(x)
    G = _groups(N, C, HW, x.data_ptr() % 16 == 0 and out_q.data_ptr() % 16 == 0)
    part3 = torch.empty((G, 3, C), dtype=torch.float64, device=x.device)
    L.check(lib.cnnq_pc_bcorr_sums(_ptr(x), _ptr(out_q), N, C, HW, int(bool(relu_first)), _ptr(part3), _stream(x)),
            'cnnq_pc_bcorr_sums')
    bias = _bcorr_bias(x, part3, group)
    L.check(lib.cnnq_pc_bcorr_apply(_ptr(out_q), N, C, HW, _ptr(bias), _stream(x)), 'cnnq_pc_bcorr_apply')
    return out_q


def qdq_bias_corrected(x, N, C, HW, qp, relu_first, group=None, out=None, want_parts=False):
    """Q/DQ with the parameter table qp followed by the activation bias correction, without ever
    storing the uncorrected tensor: one read-only pass over x for the per-channel sums (the quantized
    value is recomputed on the fly) and one fused quantize+correct pass - 12 B/elem instead of 24, the
    same floats as pc_qdq + act_bias_correction_.  want_parts: (y, dict(sums [3, C] float64, bias [C]))."""
    lib = L.load()
    x = _dev(x, 'x')
    y = _out_like(x, out)
    G = _groups(N, C, HW, x.data_ptr() % 16 == 0)
    part3 = torch.empty((G, 3, C), dtype=torch.float64, device=x.device)
    L.check(lib.cnnq_pc_qdq_bcorr_sums(_ptr(x), N, C, HW, _ptr(qp), int(bool(relu_first)), _ptr(part3), _stream(x)),
            'cnnq_pc_qdq_bcorr_sums')
    sums = torch.empty((3, C), dtype=torch.float64, device=x.device) if want_parts else None
    bias = _bcorr_bias(x, part3, group, sums)
    L.check(lib.cnnq_pc_qdq_bcorr(_ptr(x), _ptr(y), N, C, HW, _ptr(qp), _ptr(bias), 1, _stream(x)), 'cnnq_pc_qdq_bcorr')
    return _result(y, parts=dict(sums=sums, bias=bias) if want_parts else None)


def _qdq_bias_corrected_native(site, x, what, qp, relu_first, out, want_parts, allow=1):
    """qdq_bias_corrected of a tensor on its site in one host call with one cached workspace (cnnq_pc_qdq_bcorr_nhwc /
    cnnq_pc_qdq_bcorr_dt; allow: the allow_single_launch word of a layout that takes one): the per-channel sums, the bias, the
    fused quantize + correct pass.  qp: a float32 [NQP, C] device table.  y has x's layout and dtype; want_parts: (y, dict(sums
    [3, C] float64 = {sum x', sum q, count(x' > 0)}, bias [C])).  One GPU: the sums are this tensor's."""
    layout, geo, C, dt, st = site
    if not _is_table(qp, torch.float32, (L.NQP, C), x.device):
        raise L.CnnqError('%s: qp must be a contiguous float32 [%d, %d] device table' % (what, L.NQP, C))
    fn, kind = layout['bcorr']
    nbytes = _ws_bytes(kind, *geo, *layout['ws_pad'], dt)
    y = _out_like(x, out)
    ws, sp, bp, parts = _bcorr_buffers(x, kind, nbytes, C, want_parts, st)
    rc = getattr(L.load(), fn)(x.data_ptr(), y.data_ptr(), dt, *geo, qp.data_ptr(), int(bool(relu_first)), ws, sp, bp,
                               *((allow,) if layout['single'] else ()), st)
    if rc:
        L.check(rc, fn)
    return _result(y, parts=parts)


def qdq_bias_corrected_nhwc(x, qp, relu_first, out=None, want_parts=False):
    """_qdq_bias_corrected_native on a dense channels_last activation of fp32 / bf16 / fp16, on the storage as it is (DESIGN.md
    section 15): the sums over slabs of rows, 12 B/elem in fp32, 6 in bf16 / fp16.  A tensor that is not dense channels_last (or
    CNNQ_NHWC=0: copied, counted) takes qdq_bias_corrected, which is float32 only."""
    x, site = _admit_nhwc(x, 'qdq_bias_corrected_nhwc', dev_first=True)
    if site is None:
        if x.dtype != torch.float32:
            _half_only('qdq_bias_corrected_nhwc', 'the bias correction of a tensor that is not dense channels_last')
        N, C, HW = geometry(x)
        return qdq_bias_corrected(x, N, C, HW, qp, relu_first, out=out, want_parts=want_parts)
    return _qdq_bias_corrected_native(site, x, 'qdq_bias_corrected_nhwc', qp, relu_first, out, want_parts)


_TABLE_HALF_NATIVE = {}


def _table_half_native(N, C, HW, dtype):
    """The route word of cnnq_pc_route_qdq_bcorr_dt's report for this class of contiguous bf16 / fp16 layer: 1 - the table-driven
    Q/DQ with the bias correction in one launch, 2 - in two passes, 0 - a class that measured slower native than through the upcast
    and is sent back there.  The quantizer (_half_table) and the tests patch the function and empty the cache by name."""
    return _route_word(_TABLE_HALF_NATIVE, (N, C, HW, dtype), int, 'cnnq_pc_route_qdq_bcorr_dt', (N, C, HW), dtype, (1,))


def qdq_bias_corrected_half(x, qp, relu_first, out=None, want_parts=False, single_launch=None):
    """_qdq_bias_corrected_native on a contiguous 4-D bf16 / fp16 activation, on the storage as it is (-sm
    use with -bca): the sums over (channel, batch split) workgroups and the fused pass, 6 B/elem; or all three steps in one launch,
    4 B/elem, where a channel's batch population fits one workgroup's registers.  single_launch: None - the route function's
    choice; True / False - the single launch (raises where the channel does not fit) / the two passes, for tests and A/B.
    Anything else - a CPU tensor, float32, not 4-D, not contiguous - raises: nothing is copied or upcast here."""
    what = 'qdq_bias_corrected_half'
    x, site = _admit_half(x, what, 'qdq_bias_corrected')
    if single_launch:
        out = _out_like(x, out)              # (the forced form asks its route at the alignment the pair has)
        route = (ctypes.c_int32 * 4)()
        bits = x.data_ptr() | out.data_ptr() | 16
        align = bits & -bits                 # the alignment x and y share, 16 at most
        L.check(L.load().cnnq_pc_route_qdq_bcorr_dt(*site[1], site[3], align, 2, route), 'cnnq_pc_route_qdq_bcorr_dt')
        if route[3] != 1:
            raise L.CnnqError('%s: no single launch for [%d, %d, %d] at piece width %d' % ((what,) + site[1] + (route[0],)))
    return _qdq_bias_corrected_native(site, x, what, qp, relu_first, out, want_parts,
                                      1 if single_launch is None else (2 if single_launch else 0))


def _bcorr_buffers(x, tag, nbytes, C, want_parts, st):
    """(workspace, sums, bias, parts) of a one-call bias correction: the pointers its C call takes and what the caller returns as
    parts.  want_parts: sums [3, C] float64 and bias [C] are fresh tensors beside the cached workspace of nbytes; else nobody
    outside the call reads the bias, which follows the records in the cached workspace, and no sums are published."""
    if want_parts:
        sums = torch.empty((3, C), dtype=torch.float64, device=x.device)
        bias = torch.empty(C, dtype=torch.float32, device=x.device)
        return _scratch(x, tag, nbytes, st).data_ptr(), sums.data_ptr(), bias.data_ptr(), dict(sums=sums, bias=bias)
    ws = _scratch(x, tag, nbytes + C * 4, st).data_ptr()
    return ws, None, ws + nbytes, None


def _bcorr_bias(x, part3, group, sums_out=None):
    """The correction's bias from the [G, 3, C] partial sums; with world size > 1 those of the global batch (an all_gather).
    sums_out (optional [3, C] float64) receives the merged sums the bias was made from."""
    lib = L.load()
    G, _, C = part3.shape
    bias = torch.empty(C, dtype=torch.float32, device=x.device)
    if D.world_size(group) > 1:
        sums = torch.empty((3, C), dtype=torch.float64, device=x.device)
        L.check(lib.cnnq_pc_bcorr_bias(_ptr(part3), G, C, _ptr(sums), None, _stream(x)), 'cnnq_pc_bcorr_bias')
        part3 = D.all_gather_records(sums, group)
        G = part3.shape[0]
    L.check(lib.cnnq_pc_bcorr_bias(_ptr(part3), G, C, _ptr(sums_out), _ptr(bias), _stream(x)), 'cnnq_pc_bcorr_bias')
    return bias


_MT_TABLES = {}


def _midtread_tables(device):
    """The (omega, alpha) interpolation tables of iq.py:41-51 as a device fp64 [2, 101] tensor."""
    key = str(device)
    if key not in _MT_TABLES:
        from .qtypes._midtread_tables import ALPHA_TABLE, OMEGA_TABLE
        _MT_TABLES[key] = torch.tensor([OMEGA_TABLE, ALPHA_TABLE], dtype=torch.float64, device=device)
    return _MT_TABLES[key]


def mid_tread_qdq(x, target, clip, sym, per_channel_dim=1, whole_tensor=False, group=None, want_entropy=False,
                  want_codes=False, want_parts=False):
    """Mid-tread quantization with per-channel bin allocation (iq.py:147-225): statistics ->
    cnnq_pc_midtread_params -> cnnq_pc_midtread_qdq (+ histogram -> entropy).  Returns
    (y, entropy or None [, codes] [, parts])."""
    lib = L.load()
    x = _dev(x, 'x')
    N, C, HW = (1, 1, x.numel()) if whole_tensor else geometry(x, per_channel_dim)
    grp = None if group is False else group
    tabs = _midtread_tables(x.device)
    single = _ACIQ_SINGLE and _RESIDENT and clip and not whole_tensor and per_channel_dim == 1 and not want_codes
    exchanging = _sharded(group)
    if single and exchanging:
        # sharded: pass A through the collective, the ranks' sums of |x - mean| inside the single launch
        res = _mid_tread_qdq_xrank(x, N, C, HW, target, sym, tabs, grp, want_entropy, want_parts)
        if res is not None:
            return res
    if single and not exchanging:
        # pass B, the step sizes / clamp bounds and the quantization in ONE launch that reads x once
        # (cnnq_pc_midtread_qdq_single: 12 instead of 16 bytes per element) when the shape has a single-launch plan
        res = mid_tread_qdq_single(x, N, C, HW, target, sym, tabs, want_entropy, want_parts)
        if res is not None:
            return res
    stats, mom = pc_stats(x, N, C, HW, need_b=bool(clip), group=grp, local_only=group is False)
    mt = torch.empty((L.NMT, C), dtype=torch.float32, device=x.device)
    L.check(lib.cnnq_pc_midtread_params(_ptr(stats), C, float(target), int(bool(clip)), int(bool(sym)), _ptr(tabs),
                                        tabs.shape[1], _ptr(mt), _stream(x)), 'cnnq_pc_midtread_params')
    y = torch.empty_like(x)
    codes = torch.empty_like(x) if want_codes else None
    hist = torch.zeros(L.mt_hist_words(C), dtype=torch.int64, device=x.device) if want_entropy else None
    L.check(lib.cnnq_pc_midtread_qdq(_ptr(x), _ptr(y), N, C, HW, _ptr(mt), int(bool(clip)), _ptr(codes), _ptr(hist),
                                     _stream(x)), 'cnnq_pc_midtread_qdq')
    multi = want_entropy and group is not False and D.world_size(grp) > 1      # (a 1-rank forced exchange issues no collective)
    entropy = _mt_entropy(x, hist, mt, C, _raw_stream(x.device.index), grp, mom if multi else None) if want_entropy else None
    return _mt_result(y, entropy, codes, dict(stats=stats, mt=mt, hist=hist) if want_parts else None)


def mid_tread_qdq_single(x, N, C, HW, target, sym, tabs, want_entropy=False, want_parts=False, flags=0):
    """Config 5 with clipping in four launches (cnnq_pc_midtread_qdq_single) + the entropy kernel.  Returns what mid_tread_qdq
    returns, or None when the shape has no single-launch plan."""
    lib = L.load()
    st = _raw_stream(x.device.index)
    gws = _group_workspace(x, st)
    if gws is None:
        return None
    nbytes = _ws_bytes('aciq', N, C, HW, int(x.data_ptr() % 16 == 0))
    ws = _scratch(x, 'aciq', nbytes + (L.NQP + L.NDIAG) * C * 4, st)
    y = torch.empty_like(x)
    tabs_out = torch.empty((L.NSTAT + L.NMT, C), dtype=torch.float32, device=x.device)
    stats, mt = tabs_out[:L.NSTAT], tabs_out[L.NSTAT:]
    hist = torch.empty(L.mt_hist_words(C), dtype=torch.int64, device=x.device) if want_entropy else None     # zeroed by the call
    rc = lib.cnnq_pc_midtread_qdq_single(_ptr(x), _ptr(y), N, C, HW, float(target), int(bool(sym)), _ptr(tabs), tabs.shape[1],
                                         ws.data_ptr(), gws, GROUP_WS_BYTES, _ptr(stats), _ptr(mt), _ptr(hist), int(flags), st)
    if not _supported(rc, 'cnnq_pc_midtread_qdq_single'):
        return None
    return _mt_result(y, _mt_entropy_here(x, hist, mt, C, st) if want_entropy else None,
                      parts=dict(stats=stats, mt=mt, hist=hist) if want_parts else None)


def _mid_tread_qdq_native(site, x, what, target, sym, want_entropy, stats, out, want_parts, allow=1):
    """Config 5 with clipping (iq.py:170-225: mid-tread quantization with per-channel bin allocation; want_entropy: the entropy of
    the codes, -me) of a tensor on its site: the statistics, the step sizes and clamp bounds and the Q/DQ with the code histogram
    in one host call with one cached workspace (cnnq_pc_midtread_nhwc / cnnq_pc_midtread_dt; allow: the allow_single_launch word
    of a layout that takes one) - or, with `stats` (a float32 [NSTAT, C] device table), cnnq_pc_midtread_params on that table and
    the table-driven pass.  y has x's layout and dtype.  Returns what mid_tread_qdq returns: (y, entropy or None [, dict(stats,
    mt, hist)]); inside an entropy_batch block the entropy is filled by the block's one launch.  One GPU: the statistics are this
    tensor's."""
    layout, geo, C, dt, st = site
    fn, fn_table, kind = layout['midtread']
    lib = L.load()
    tabs = _midtread_tables(x.device)
    if stats is not None and not _is_table(stats, torch.float32, (L.NSTAT, C), x.device):
        raise L.CnnqError('%s: stats must be a contiguous float32 [%d, %d] device table' % (what, L.NSTAT, C))
    y = _out_like(x, out)
    if stats is not None:
        mt = torch.empty((L.NMT, C), dtype=torch.float32, device=x.device)
        L.check(lib.cnnq_pc_midtread_params(_ptr(stats), C, float(target), 1, int(bool(sym)), _ptr(tabs), tabs.shape[1], _ptr(mt), st),
                'cnnq_pc_midtread_params')
        hist = torch.zeros(L.mt_hist_words(C), dtype=torch.int64, device=x.device) if want_entropy else None
        rc = getattr(lib, fn_table)(x.data_ptr(), y.data_ptr(), dt, *geo, _ptr(mt), _ptr(hist), st)
        if rc:
            L.check(rc, fn_table)
    else:
        nbytes = _ws_bytes(kind, *geo, *layout['ws_pad'], dt)
        hist = torch.empty(L.mt_hist_words(C), dtype=torch.int64, device=x.device) if want_entropy else None     # zeroed by the call
        if want_parts or want_entropy:
            # (the entropy launch reads mt behind the call - at the end of the block inside an entropy_batch)
            out_tabs = torch.empty((L.NSTAT + L.NMT, C), dtype=torch.float32, device=x.device)
            stats, mt = out_tabs[:L.NSTAT], out_tabs[L.NSTAT:]
            ws, tp = _scratch(x, kind, nbytes, st).data_ptr(), out_tabs.data_ptr()
        else:
            # the tables nobody outside the call reads follow the records in the cached workspace
            ws = _scratch(x, kind, nbytes + (L.NSTAT + L.NMT) * C * 4, st).data_ptr()
            tp = ws + nbytes
            mt = None
        rc = getattr(lib, fn)(x.data_ptr(), y.data_ptr(), dt, *geo, float(target), int(bool(sym)), _ptr(tabs), tabs.shape[1],
                              ws, tp, tp + L.NSTAT * C * 4, _ptr(hist), *((allow,) if layout['single'] else ()), st)
        if rc:
            L.check(rc, fn)
    return _mt_result(y, _mt_entropy_here(x, hist, mt, C, st) if want_entropy else None,
                      parts=dict(stats=stats, mt=mt, hist=hist) if want_parts else None)


def mid_tread_qdq_nhwc(x, target, sym, want_entropy=False, stats=None, out=None, want_parts=False):
    """_mid_tread_qdq_native on a dense channels_last activation of fp32 / bf16 / fp16, on the storage as it is (DESIGN.md section
    16): the statistics over slabs of rows, 16 B/elem in fp32, 8 in bf16 / fp16.  A tensor that is not dense channels_last (or
    CNNQ_NHWC=0, or a class of layer the route function sends back: copied, counted) takes mid_tread_qdq, which is float32 only -
    a half tensor raises before anything is copied - and knows neither `stats` nor `out`."""
    x, site = _admit_nhwc(x, 'mid_tread_qdq_nhwc', 'midtread',
                          'the mid-tread quantization of a tensor that does not take the channels_last kernels')
    if site is None:
        if stats is not None or out is not None:
            raise L.CnnqError('mid_tread_qdq_nhwc: stats= and out= need a dense channels_last tensor')
        return mid_tread_qdq(x, target, clip=True, sym=sym, group=False, want_entropy=want_entropy, want_parts=want_parts)
    return _mid_tread_qdq_native(site, x, 'mid_tread_qdq_nhwc', target, sym, want_entropy, stats, out, want_parts)


_MIDTREAD_HALF_NATIVE = {}


def _midtread_half_native(N, C, HW, dtype, hist=False):
    """The route word of cnnq_pc_route_midtread_dt's report for this class of contiguous bf16 / fp16 layer, with (hist) or without
    the code histogram: 3 - pass A and the bin allocation in front of the resident launch, 2 - the chain, 0 - a class that measured
    slower native than through the upcast and is sent back there.  The quantizer (_midtread_route) and the tests patch the function
    and empty the cache by name."""
    return _route_word(_MIDTREAD_HALF_NATIVE.setdefault(bool(hist), {}), (N, C, HW, dtype), int, 'cnnq_pc_route_midtread_dt',
                       (N, C, HW), dtype, (int(bool(hist)), 1))


def mid_tread_qdq_half(x, target, sym, want_entropy=False, stats=None, out=None, want_parts=False, single_launch=None):
    """_mid_tread_qdq_native on a contiguous 4-D bf16 / fp16 activation, on the storage as it is: pass A, the
    bin allocation and one launch that keeps a channel in registers for b, the step size, the clamp bounds and the Q/DQ with the
    code histogram where the channel's batch population fits, else the chain of cnnq_pc_stats_dt, cnnq_pc_midtread_params and
    cnnq_pc_midtread_qdq_dt.  8 B/elem as a chain, 6 resident.  single_launch: None - the route function's choice; 0 - the chain;
    2 - the resident form wherever the channel fits (the chain elsewhere), for tests and A/B.  Anything else - a CPU tensor,
    float32, not 4-D, not contiguous - raises: nothing is copied or upcast here."""
    what = 'mid_tread_qdq_half'
    x, site = _admit_half(x, what, 'mid_tread_qdq')
    if stats is None and single_launch not in (None, 0, 1, 2):
        raise L.CnnqError('%s: single_launch must be None, 0, 1 or 2, got %r' % (what, single_launch))
    return _mid_tread_qdq_native(site, x, what, target, sym, want_entropy, stats, out, want_parts,
                                 1 if single_launch is None or stats is not None else int(single_launch))


def _mt_entropy_here(x, hist, mt, C, st):
    """The entropy of this GPU's mid-tread code histogram of x: inside an entropy_batch block one launch for the whole block, at its
    end; else one launch behind the tensor."""
    if _ENT_BATCH is not None:
        return _ENT_BATCH.add_midtread(hist, mt, C, x.numel(), x.device)
    return _mt_entropy(x, hist, mt, C, st)


def _mt_entropy(x, hist, mt, C, st, group=None, mom=None):
    """The entropy of a mid-tread code histogram of x.  With the merged moment record `mom` x is a batch shard: the ranks'
    counts are summed over `group` first, and the element count is the global batch's (shards may differ by a sample)."""
    lib = L.load()
    ent = torch.empty(1, dtype=torch.float32, device=x.device)
    if mom is not None:
        D.all_reduce_sum_(hist, group)
        rc = lib.cnnq_midtread_entropy_count(_ptr(hist), _ptr(mt), C, mom[L.MOM_COUNT].data_ptr(), _ptr(ent), st)
    else:
        rc = lib.cnnq_midtread_entropy(_ptr(hist), _ptr(mt), C, x.numel(), _ptr(ent), st)
    L.check(rc, 'cnnq_midtread_entropy')
    return ent[0]


def tensor_stats(x, rows=1, need_dev=True):
    """The statistics of x viewed as [rows, numel / rows], rows contiguous and back to back - rows = 1: the whole tensor, the
    per-tensor calibration table of statistic_manager.py:55-96; rows = N: the samples - for fp32 / bf16 / fp16 on the storage as
    it lies: cnnq_rows_stats - pass A, the merge, and with need_dev pass B and its merge - one host call,
    one cached workspace, 8 B/elem in fp32 and 4 in bf16 / fp16 for the full table.  Returns (stats [NSTAT, rows] f32, mom
    [NMOM, rows] f64); rows B and KURT are zero without need_dev, the rectified sums are always there.  Taken as it is: a
    contiguous tensor, and - the sums and extrema of a sample do not depend on its elements' order - a dense channels_last 4-D
    tensor with rows in (1, N).  Anything else is copied by _dev_act, counted.  One GPU: the statistics are this tensor's."""
    rows = int(rows)
    keep = isinstance(x, torch.Tensor) and x.dim() == 4 and rows in (1, x.shape[0])
    x = _dev_act_layout(x, 'x') if keep else _dev_act(x, 'x')
    n = x.numel()
    if rows < 1 or n == 0 or n % rows:
        raise L.CnnqError('tensor_stats: %d elements do not make %d rows' % (n, rows))
    length = n // rows
    dt = _DTYPE_CODES[x.dtype]
    st = _raw_stream(x.device.index)
    stats = torch.empty((L.NSTAT, rows), dtype=torch.float32, device=x.device)
    mom = torch.empty((L.NMOM, rows), dtype=torch.float64, device=x.device)
    ws = _scratch(x, 'rows', _ws_bytes('rows', rows, length, 1, dt), st)
    rc = L.load().cnnq_rows_stats(x.data_ptr(), dt, rows, length, int(bool(need_dev)), ws.data_ptr(), mom.data_ptr(), stats.data_ptr(), st)
    if rc:
        L.check(rc, 'cnnq_rows_stats')
    return stats, mom


def _flat_x(x, what):
    """x as the per-tensor entry points take it: an fp32 / bf16 / fp16 tensor on the current device whose storage is its elements
    back to back - contiguous, or 4-D and dense channels_last.  Anything else raises: no copy is made here."""
    if not isinstance(x, torch.Tensor):
        raise L.CnnqError('%s: x must be a tensor' % what)
    if x.dtype not in _ACT_DTYPES:
        raise L.CnnqError('%s: x must be float32, bfloat16 or float16, got %s' % (what, x.dtype))
    if _layout(x) == 'copy' or x.numel() == 0:             # shape and strides only
        raise L.CnnqError('%s: x must be a non-empty contiguous or dense channels_last tensor (no copy is made here)' % what)
    if not x.is_cuda:
        raise L.CnnqError('%s: x must be a CUDA/HIP tensor (there is no CPU path)' % what)
    if x.device.index != torch.cuda.current_device():
        raise L.CnnqError('%s: x is on %s but the current device is cuda:%d' % (what, x.device, torch.cuda.current_device()))
    return x.detach() if x.requires_grad else x


def clip_qdq_tensor(x, num_bits, positive=False, clip='laplace', stats=None, out=None, want_parts=False):
    """Per-tensor clipping (iq.py:353-357: ACIQ layer-wise - 'laplace', 'gaus' or '<p>std' with scalar statistics, delta the range
    itself, no bit allocation) of an fp32 / bf16 / fp16 tensor on the storage as it lies: the result does
    not depend on the elements' order, so a contiguous tensor and a dense channels_last 4-D one are read as they are - no upcast,
    no layout copy; anything else raises.  Dynamic: cnnq_pt_clip_qdq - the whole-tensor statistics of tensor_stats, the
    parameters, the flat Q/DQ - one host call, one cached workspace.  With `stats` ([NSTAT, 1], -sm use): pc_params on that
    table and cnnq_flat_qdq.  y has x's dtype, shape and strides; want_parts: (y, dict(stats, qp, diag)).  One GPU: the
    statistics are this tensor's."""
    x = _flat_x(x, 'clip_qdq_tensor')
    cfg = _params_cfg(num_bits, positive, clip, False, False, None, True, True)
    if cfg.clip == 0:
        raise L.CnnqError("clip_qdq_tensor: clip must be 'laplace', 'gaus' or '<p>std', got %r" % (clip,))
    if stats is not None and not _is_table(stats, torch.float32, (L.NSTAT, 1), x.device):
        raise L.CnnqError('clip_qdq_tensor: stats must be a contiguous float32 [%d, 1] device table' % L.NSTAT)
    y = _out_like(x, out)
    lib = L.load()
    n, dt, st = x.numel(), _DTYPE_CODES[x.dtype], _raw_stream(x.device.index)
    if stats is not None:
        qp, diag = pc_params(stats, num_bits, positive, clip, direct_range=True)
        rc = lib.cnnq_flat_qdq(x.data_ptr(), y.data_ptr(), dt, n, qp.data_ptr(), st)
        if rc:
            L.check(rc, 'cnnq_flat_qdq')
        return _result(y, parts=dict(stats=stats, qp=qp, diag=diag) if want_parts else None)
    nbytes = _ws_bytes('pt_clip', n, 1, 1, dt)
    if want_parts:
        tabs = torch.empty(L.NSTAT + L.NQP + L.NDIAG, 1, dtype=torch.float32, device=x.device)
        ws, tp = _scratch(x, 'pt_clip', nbytes, st).data_ptr(), tabs.data_ptr()
    else:
        # the tables nobody outside the call reads follow the records in the cached workspace
        ws = _scratch(x, 'pt_clip', nbytes + (L.NSTAT + L.NQP + L.NDIAG) * 4, st).data_ptr()
        tp = ws + nbytes
    rc = lib.cnnq_pt_clip_qdq(x.data_ptr(), y.data_ptr(), dt, n, ctypes.byref(cfg), ws, tp, tp + L.NSTAT * 4, tp + (L.NSTAT + L.NQP) * 4, st)
    if rc:
        L.check(rc, 'cnnq_pt_clip_qdq')
    return _result(y, parts=dict(stats=tabs[:L.NSTAT], qp=tabs[L.NSTAT:L.NSTAT + L.NQP], diag=tabs[L.NSTAT + L.NQP:]) if want_parts else None)


def mid_tread_qdq_tensor(x, target, sym, out=None, want_parts=False):
    """Per-tensor mid-tread quantization with clipping (iq.py:158-168 without -pcq_a: the whole tensor is one channel) of an fp32 /
    bf16 / fp16 tensor on the storage as it lies, taken and refused as clip_qdq_tensor takes and refuses:
    cnnq_pt_midtread - the whole-tensor statistics, step size and clamp bounds, the flat pass - one host call, one cached
    workspace.  No entropy: the per-tensor branch discards it.  y has x's dtype, shape and strides; want_parts: (y, dict(stats, mt))."""
    x = _flat_x(x, 'mid_tread_qdq_tensor')
    y = _out_like(x, out)
    n, dt, st = x.numel(), _DTYPE_CODES[x.dtype], _raw_stream(x.device.index)
    tabs = _midtread_tables(x.device)
    nbytes = _ws_bytes('pt_clip', n, 1, 1, dt)
    if want_parts:
        out_tabs = torch.empty(L.NSTAT + L.NMT, 1, dtype=torch.float32, device=x.device)
        ws, tp = _scratch(x, 'pt_clip', nbytes, st).data_ptr(), out_tabs.data_ptr()
    else:
        ws = _scratch(x, 'pt_clip', nbytes + (L.NSTAT + L.NMT) * 4, st).data_ptr()
        tp = ws + nbytes
    rc = L.load().cnnq_pt_midtread(x.data_ptr(), y.data_ptr(), dt, n, float(target), int(bool(sym)), _ptr(tabs), tabs.shape[1], ws, tp,
                                   tp + L.NSTAT * 4, st)
    if rc:
        L.check(rc, 'cnnq_pt_midtread')
    return _result(y, parts=dict(stats=out_tabs[:L.NSTAT], mt=out_tabs[L.NSTAT:]) if want_parts else None)


def tensor_row_stats(x, rows):
    """Per-row MIN/MAX (and friends) of x viewed as [rows, numel/rows]: the per-sample statistics
    of iq.py:510-517 (rows = batch) - the per-channel kernels with N = 1, C = rows."""
    lib = L.load()
    # each sample of a dense channels_last tensor is one contiguous block of C*H*W elements: rows = samples (or 1) read the
    # storage as it is
    per_sample = isinstance(x, torch.Tensor) and x.dim() == 4 and rows in (1, x.shape[0])
    x = _dev_act_layout(x, 'x') if per_sample else _dev_act(x, 'x')
    hw = x.numel() // rows
    half = x.dtype != torch.float32
    G = _groups(1, rows, hw, None if half else x.data_ptr() % 16 == 0)
    pmm = torch.empty((G, 2, rows), dtype=torch.float32, device=x.device)
    # rows MIN (0) and MAX (1) of a stats table with stride `rows`: what cnnq_pt_setup reads
    table = torch.empty((2, rows), dtype=torch.float32, device=x.device)
    if half:
        L.check(lib.cnnq_pc_minmax_local_dt(_ptr(x), _HALF_DTYPES[x.dtype], 1, rows, hw, _ptr(pmm), _ptr(table), _stream(x)),
                'cnnq_pc_minmax_local_dt')
    else:
        L.check(lib.cnnq_pc_minmax(_ptr(x), 1, rows, hw, _ptr(pmm), _stream(x)), 'cnnq_pc_minmax')
        L.check(lib.cnnq_pc_minmax_reduce(_ptr(pmm), G, rows, _ptr(table), _stream(x)), 'cnnq_pc_minmax_reduce')
    return table


def minmax_qdq_per_tensor(x, num_bits, avg_over_batch, zero_min=False, int_exp=False, enforce_true_zero=True,
                          group=None, fused=None):
    """iq.py:361-379 + 605-614 with dynamic statistics: per-sample min/max, their batch mean
    (or the whole-tensor min/max), then the GEMMLOWP kernel - all on the device, four launches.
    fused=True (default: CNNQ_PT_FUSED=1) takes the ONE-launch form on a single GPU (cnnq_pt_minmax_qdq_fused): the same
    bits, but measured SLOWER than the chain - 70 against 54 us on the [32,64,112,112] tensor of BASELINE config 1: its
    second sweep is not served by the Infinity Cache once 103 MB of y are written next to it - so
    it is opt-in.  A dense channels_last x is read as it is (its samples are contiguous blocks too); y has its layout."""
    x = _dev_act_layout(x, 'x')
    rows = x.shape[0] if x.dim() > 1 else 1
    if (_PT_FUSED if fused is None else fused) and D.world_size(group) == 1 and x.numel() > 0 and x.dtype == torch.float32:
        # one launch (k_pt_fused): two sweeps with a tile count in between, the second served by the Infinity Cache
        st = _raw_stream(x.device.index)
        gws = _group_workspace(x, st)
        if gws is not None:
            y = torch.empty_like(x)
            rc = L.load().cnnq_pt_minmax_qdq_fused(x.data_ptr(), y.data_ptr(), x.numel(), rows, 0 if avg_over_batch else 1,
                                                   int(bool(zero_min)), int(num_bits), int(bool(int_exp)),
                                                   int(bool(enforce_true_zero)), gws, GROUP_WS_BYTES, None, st)
            if _supported(rc, 'cnnq_pt_minmax_qdq_fused'):
                return y
    stats = tensor_row_stats(x, rows)
    if D.world_size(group) > 1:
        stats = D.merge_row_minmax(stats, rows, avg_over_batch, group)
        rows = stats.shape[1]
    ptp = pt_setup(x.device, num_bits, stats=stats, rows=rows, rows_mode=0 if avg_over_batch else 1,
                   zero_min=zero_min, int_exp=int_exp, enforce_true_zero=enforce_true_zero)
    return pt_qdq(x, ptp)


def kld_thresholds(x, rows=None, want_parts=False):
    """`-kld` calibration (inference/kld_threshold.py:6-84 per sample, statistic_manager.py:80-82):
    x viewed as [rows, numel/rows] (rows = batch samples) -> float64 tensor [rows, 3] =
    {optimal clipping threshold, its KL divergence, candidate index}; the `kld_th` statistic of
    the batch is out[:, 0].max().  want_parts adds (hist [rows, 2001] int32, div [rows, 994]).  float32 only."""
    lib = L.load()
    if rows is None and isinstance(x, torch.Tensor):
        rows = x.shape[0] if x.dim() > 1 else 1
    # the histogram of a sample (or of the whole tensor) does not depend on the order of its elements, and a sample of a dense
    # channels_last tensor is one contiguous block: rows = samples (or 1) read the storage as it is, the copy route's bits
    x = _dev(x, 'x', keep_nhwc=isinstance(x, torch.Tensor) and x.dim() == 4 and rows is not None and int(rows) in (1, x.shape[0]))
    rows = int(rows)
    length = x.numel() // rows
    rowmm = tensor_row_stats(x, rows)
    hist = torch.empty((rows, L.KLD_BINS), dtype=torch.int32, device=x.device)
    div = torch.empty((rows, L.KLD_NCAND), dtype=torch.float64, device=x.device)
    out = torch.empty((rows, 3), dtype=torch.float64, device=x.device)
    L.check(lib.cnnq_kld_hist(_ptr(x), rows, length, _ptr(rowmm), _ptr(hist), _stream(x)), 'cnnq_kld_hist')
    L.check(lib.cnnq_kld_search(_ptr(hist), rows, _ptr(rowmm), _ptr(div), _ptr(out), _stream(x)), 'cnnq_kld_search')
    if want_parts:
        return out, hist, div
    return out


_KLD_HALF_NATIVE = {}


def _kld_half_native(rows, length, dtype):
    """Whether this class of tensor - rows samples of `length` elements - collects its KLD threshold on the bf16 / fp16 histogram
    (kld_thresholds_half) or stays on the upcast route: the last question of the per-tensor manager's collect_route.  Host only,
    a function of the shape and the dtype, cached; the tests patch the function and empty the cache by name.
    The yardstick is tools/bench_half_kld.py (MI355X, ResNet-50 conv outputs at batch 512, the routes alternating step by step,
    us per call, mean (min-max) of ten steps; profiles/half_kld.md has every figure): the search takes 4.86 ms at 512 rows whatever
    the rows hold, and the two smallest classes did not win beyond its spread in any of the four runs - [512,256,14,14] bf16
    4912.6 (4896.2-4928.0) against 4940.5 (4917.3-4954.9), [512,512,7,7] 4900.6 (4882.6-4929.6) against 4913.9 (4900.7-4928.1) -
    while [512,128,28,28], [512,512,14,14] and [512,2048,7,7] (2^25.6 elements) and everything larger did.  So 512 rows or more
    of fewer than 2^25 elements in all stay on the upcast route; fewer rows were not measured and stay native."""
    key = (rows, length, dtype)
    v = _KLD_HALF_NATIVE.get(key)
    if v is None:
        v = _KLD_HALF_NATIVE[key] = not (rows >= 512 and rows * length < (1 << 25))
    return v


def kld_thresholds_half(x, rows=None, want_parts=False):
    """kld_thresholds of a bf16 / fp16 tensor on the storage as it lies (-sm collect -kld): x viewed as
    [rows, numel/rows] (rows None: its samples) -> kld_thresholds' result, float64 [rows, 3], with want_parts (out, hist, div) -
    bit for bit what kld_thresholds gives on x.float(): the upconversion is exact, so the histogram is that copy's, count for
    count, and the search sees nothing else.  tensor_row_stats (cnnq_pc_minmax_local_dt), cnnq_kld_hist_dt, cnnq_kld_search:
    two reads of x at 2 B/elem.  Taken: a non-empty tensor on the current device that is contiguous, or 4-D dense channels_last
    with rows in (1, N) - a sample is one contiguous block, and a histogram does not depend on the order of its elements.
    Anything else - a CPU tensor, float32 (kld_thresholds takes it), an empty or non-dense tensor, channels_last with other rows
    or with CNNQ_NHWC=0, rows that do not divide the elements - raises: nothing is copied or upcast here."""
    what = 'kld_thresholds_half'
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise L.CnnqError('%s: x must be a CUDA/HIP tensor (there is no CPU path)' % what)
    if x.dtype not in _HALF_DTYPES:
        raise L.CnnqError('%s: x must be bfloat16 or float16, got %s (float32 takes kld_thresholds)' % (what, x.dtype))
    if rows is None:
        rows = x.shape[0] if x.dim() > 1 else 1
    rows = int(rows)
    layout = _layout(x)
    if layout == 'copy' or x.numel() == 0:
        raise L.CnnqError('%s: x must be a non-empty contiguous or dense channels_last tensor (no copy is made here)' % what)
    if layout == 'nhwc' and not (_NHWC and rows in (1, x.shape[0])):
        raise L.CnnqError('%s: a channels_last tensor is read as it lies for rows = 1 or its samples, with the channels_last '
                          'switch on (no copy is made here); got rows = %d' % (what, rows))
    if x.device.index != torch.cuda.current_device():
        raise L.CnnqError('%s: x is on %s but the current device is cuda:%d' % (what, x.device, torch.cuda.current_device()))
    if rows < 1 or x.numel() % rows:
        raise L.CnnqError('%s: %d elements do not make %d rows' % (what, x.numel(), rows))
    if x.requires_grad:
        x = x.detach()
    lib = L.load()
    length = x.numel() // rows
    rowmm = tensor_row_stats(x, rows)
    hist = torch.empty((rows, L.KLD_BINS), dtype=torch.int32, device=x.device)
    div = torch.empty((rows, L.KLD_NCAND), dtype=torch.float64, device=x.device)
    out = torch.empty((rows, 3), dtype=torch.float64, device=x.device)
    L.check(lib.cnnq_kld_hist_dt(_ptr(x), _HALF_DTYPES[x.dtype], rows, length, _ptr(rowmm), _ptr(hist), _stream(x)), 'cnnq_kld_hist_dt')
    L.check(lib.cnnq_kld_search(_ptr(hist), rows, _ptr(rowmm), _ptr(div), _ptr(out), _stream(x)), 'cnnq_kld_search')
    if want_parts:
        return out, hist, div
    return out


def row_sumsq_native(x, rows=None):
    """Whether row_sumsq reads x where it lies: a bf16 / fp16 device tensor, or a dense channels_last float32 one (with the
    channels_last switch on) whose rows are its samples (rows None: they are).  Shape, strides and dtype only."""
    return (isinstance(x, torch.Tensor) and x.is_cuda and x.dim() > 0 and
            (x.dtype in _HALF_DTYPES or (x.dtype == torch.float32 and _NHWC and _layout(x) == 'nhwc' and rows in (None, x.shape[0]))))


def row_sumsq(x, rows=None):
    """Per-sample sum of squares, the runtime distance measure of distance_stats.py:22-33
    (`torch.sum(t**2, dim=-1)` on [N, -1]): the moments kernel with N = 1, C = rows (fp64 sums) for a contiguous float32
    tensor; a bf16 / fp16 tensor, and a dense channels_last one with rows = its samples, take tensor_stats where they lie."""
    if row_sumsq_native(x, rows):
        # bf16 / fp16, and the samples of a dense channels_last tensor: the flat-row kernels on the storage as it lies
        return tensor_stats(x, int(rows if rows is not None else x.shape[0]), need_dev=False)[1][L.MOM_SUMSQ].to(torch.float32)
    x = _dev(x, 'x')
    rows = int(rows if rows is not None else x.shape[0])
    _, mom = pc_stats(x, 1, rows, x.numel() // rows, local_only=True)
    return mom[L.MOM_SUMSQ].to(torch.float32)
