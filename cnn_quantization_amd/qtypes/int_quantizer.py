"""`IntQuantizer` - the op surface of the reference's quantizer
(pytorch_quantizer/quantization/qtypes/int_quantizer.py:56-632, "iq.py" below) re-hosted on the
MI355X kernels: same constructor keys, same `__call__(tensor, id, tag, stat_id, override_att)`,
same externally mutated attributes and the same dispatch order, so the reference's manager and
`inference_sim.py` drive it unchanged.  What differs is below the surface: every branch is a
handful of launches into libcnnq_hip.so (statistics -> parameters -> fused Q/DQ on native NCHW)
with no transposed copies, no elementwise temporaries and no host synchronisation.

Only the arithmetic lives on the device; there is no CPU path (CPU tensors raise)."""
import math
from functools import partial

import numpy as np
import torch

from .. import _lib as L
from .. import distributed as D
from .. import ops

# bf16 / fp16 activations.  A tensor whose route (IntQuantizer._route) has a name is quantized where it lies.
# Every other path that meets a half tensor goes through upcast_fallback, the ONE place that upcasts: it computes on x.float() and
# returns .to(x.dtype), and counts the call (HALF_FALLBACKS) so that tests can prove the native routes never arrive there.
HALF_DTYPES = (torch.bfloat16, torch.float16)
HALF_FALLBACKS = 0


def upcast_fallback(fn, *args, cast_back=True, **kw):
    """fn(*args, **kw) with every bf16 / fp16 tensor argument upcast to float32; a tensor result is cast back to the dtype
    of the first half argument (cast_back=False: returned as computed).  Without a half argument: fn(*args, **kw), uncounted."""
    global HALF_FALLBACKS
    dt = next((a.dtype for a in args if isinstance(a, torch.Tensor) and a.dtype in HALF_DTYPES), None)
    if dt is None:
        return fn(*args, **kw)
    HALF_FALLBACKS += 1
    res = fn(*[a.float() if isinstance(a, torch.Tensor) and a.dtype in HALF_DTYPES else a for a in args], **kw)
    if cast_back and isinstance(res, torch.Tensor) and res.is_floating_point():
        return res.to(dt)
    return res


def _is_pc_act(t):
    """iq.py:110,160,333: 4-D with a spatial extent."""
    return len(t.shape) > 3 and (t.shape[2] > 1 or t.shape[3] > 1)


def _dense_nhwc(t):
    """A dense channels_last 4-D tensor that is not contiguous - what ops._layout calls 'nhwc'; a contiguous tensor never asks ops -
    with the channels_last switch on.  Shape and strides only."""
    return t.dim() == 4 and not t.is_contiguous() and t.is_contiguous(memory_format=torch.channels_last) and ops._NHWC


def _storage(t):
    """The storage class of the per-channel routes: 'nhwc' - dense channels_last with the switch on, 'half' - a contiguous non-empty
    4-D bf16 / fp16 tensor on the device, None - neither.  The costly fact: a route asks it once, after its attributes."""
    return 'nhwc' if _dense_nhwc(t) else 'half' if (getattr(t, 'is_cuda', False) and t.dtype in HALF_DTYPES and t.dim() == 4
                                                    and t.is_contiguous() and t.numel() > 0) else None


def _to_f32_vec(v, C):
    a = np.asarray(v, dtype=np.float32).reshape(-1)
    if a.size == 1 and C > 1:
        a = np.repeat(a, C)
    return torch.from_numpy(np.ascontiguousarray(a))


# the rows of the calibration table every ACIQ clipping reads (per channel, per tensor and -c mix)
ACIQ_ROWS = {L.STAT_MIN: ('min', 'mean'), L.STAT_MAX: ('max', 'mean'), L.STAT_MEAN: ('mean', 'mean'), L.STAT_B: ('b', 'mean'),
             L.STAT_STD: ('std', 'mean')}
# the routes _half_native answers for: configs 1 and 2, config 3 on channels_last, a correction folded in on channels_last
HALF_NATIVE_ROUTES = frozenset(('minmax_pt', 'minmax_pc', 'half_minmax', 'nhwc_aciq', 'nhwc_bcorr'))


class IntQuantizer:
    def __init__(self, size, params):
        # iq.py:57-90
        self.num_bits = size
        self.stochastic = False
        self.int_exp = False
        self.enforce_true_zero = True
        self.clipping = params['clipping'] if 'clipping' in params else 'no'
        self.stats_kind = params['stats_kind'] if 'stats_kind' in params else 'mean'
        self.kld = params['kld'] if 'kld' in params else False
        self.pcq_w = params['pcq_weights']
        self.pcq_a = params['pcq_act']
        self.bit_alloc_act = params['bit_alloc_act']
        self.bit_alloc_weight = params['bit_alloc_weight']
        self.bcorr_act = params['bcorr_act']
        self.bcorr_weight = params['bcorr_weight']
        self.vcorr_weight = params['vcorr_weight']
        self.bit_alloc_round = params['bit_alloc_rmode'] == 'round'
        self.bit_alloc_prior = params['bit_alloc_prior']
        self.bit_alloc_target_act = params['bit_alloc_target_act'] if params['bit_alloc_target_act'] is not None \
            else self.num_bits
        self.bit_alloc_target_weight = params['bit_alloc_target_weight'] \
            if params['bit_alloc_target_weight'] is not None else self.num_bits
        self.measure_entropy = params['measure_entropy']
        self.logger = params['logger']
        self.mtd_quant = params['mtd_quant']
        # the statistics managers are looked up lazily: `self.sm` is a class the manager may replace
        from ..inference.statistic_manager import StatisticManager
        from ..inference.statistic_manager_perchannel import StatisticManagerPerChannel
        self.sm = StatisticManagerPerChannel if params['pcq_act'] else StatisticManager
        self.force_positive = False
        self.half_range = False
        # process group over which dynamic statistics are made global (None = default group if
        # torch.distributed is initialised, single process otherwise); see distributed.py
        self.group = None
        self._table_cache = {}
        # activation bias correction hand-off (iqm.py:180-196): a layer that wants its output corrected sets
        # fuse_bcorr to the relu-first flag before the call; a per-channel path that folds the correction
        # into its own passes resets it to None and raises bcorr_fused, otherwise the layer corrects after
        self.fuse_bcorr = None
        self.bcorr_fused = False
        # the route 'half_aciq' (dynamic ACIQ on a contiguous bf16 / fp16 activation) is opt-in per object:
        # the inference manager sets this on the quantizers it builds; one constructed directly keeps the upcast route
        self.half_dynamic = False
        # the route 'half_midtread' (mid-tread on a contiguous bf16 / fp16 activation): opt-in per object in
        # the same way, and for the same reason
        self.half_midtread = False
        # the route 'half_entropy' (-me with a uniform quantizer on a contiguous bf16 / fp16 activation):
        # opt-in per object in the same way, and for the same reason
        self.half_entropy = False
        # the route 'mix' (-sm use -c mix on a dense channels_last or contiguous bf16 / fp16 activation):
        # opt-in per object in the same way, and for the same reason
        self.native_mix = False

    # ------------------------------------------------------------------ dispatch, iq.py:92-122
    def __call__(self, tensor, id, tag="", stat_id=None, override_att=None):
        att = self._att(override_att)
        branch = self._branch(att, tensor)
        if (isinstance(tensor, torch.Tensor) and tensor.dtype in HALF_DTYPES
                and self._route(branch, tensor, stat_id, att) is None):
            return upcast_fallback(self.__call__, tensor, id, tag, stat_id, override_att)
        if override_att is not None:
            orig_att = getattr(self, override_att[0])
            setattr(self, override_att[0], override_att[1])
        try:
            return BRANCH_CALLS[branch](self, tensor, id, tag, stat_id)
        finally:
            if override_att is not None:
                setattr(self, override_att[0], orig_att)

    def _att(self, override_att=None):
        """The attribute lookup the route decision reads through: __call__'s override_att pair wins over the attribute."""
        return partial(getattr, self) if override_att is None else \
            lambda k: override_att[1] if override_att[0] == k else getattr(self, k)

    def _one_gpu(self):
        """Replicated data excluded (group is not False), a batch that is not sharded, no forced exchange."""
        return self.group is not False and D.world_size(self.group) == 1 and not D.forced_exchange()

    # The route decision (table: DESIGN.md section 26).  Level 1, _branch: the branch method __call__ hands the tensor to.  Level 2,
    # one function per branch: the name of the native route its method takes, None - its fp32 code, which a half tensor reaches
    # through the upcast.  Shape, strides and attributes (att: the lookup of _att) only; nothing stored; before _take_bcorr.
    def _branch(self, att, tensor):
        """iq.py:92-122's ladder."""
        if att('kld'):
            return 'kld'
        if att('clipping') != 'no':
            return 'midtread' if att('mtd_quant') else 'clip'
        if att('pcq_w'):
            return 'midtread_w' if att('mtd_quant') else 'weights'
        if att('pcq_a') and _is_pc_act(tensor):
            return 'midtread_pc' if att('mtd_quant') else 'pc'
        return 'minmax'

    def _route(self, branch, tensor, stat_id, att):
        """Level 2 of the branch __call__ takes."""
        if branch == 'clip':
            return self._clip_route(tensor, att('clipping'), stat_id, att)
        if branch == 'pc':
            return self._pc_route(tensor, stat_id, att)
        if branch in ('midtread', 'midtread_pc'):
            return self._midtread_route(tensor, att)
        if branch == 'kld':
            return self._kld_route(tensor)
        return 'minmax_pt' if branch == 'minmax' else None          # config 1 has half and channels_last kernels; weights: none

    def _facts(self, tensor, att):
        """What the routes of a branch share, computed once: whether the per-channel activation code applies, one GPU's own data,
        bit allocation in effect, a bias correction pending.  (The storage class, _storage, comes after them: it costs the most.)"""
        return (bool(att('pcq_a')) and _is_pc_act(tensor), self._one_gpu(), bool(att('bit_alloc_act')) and att('num_bits') <= 4,
                self.fuse_bcorr is not None)

    def _flat_tensor(self, tensor):
        """What the per-tensor routes over flat storage take: on the device and either bf16 / fp16, contiguous
        or dense channels_last, or fp32 dense channels_last; not empty."""
        if not getattr(tensor, 'is_cuda', False) or tensor.numel() == 0:
            return False
        if tensor.dtype in HALF_DTYPES:
            return tensor.is_contiguous() or _dense_nhwc(tensor)
        return tensor.dtype == torch.float32 and _dense_nhwc(tensor)

    def _kld_route(self, tensor):
        """gemmlowpKldQuantize: __gemmlowpQuantize__ hands a half tensor, contiguous or dense channels_last, to ops.pt_qdq's half
        kernel as it is.  The name routes nothing; it keeps __call__ from upcasting."""
        return 'kld' if (getattr(tensor, 'is_cuda', False) and tensor.dtype in HALF_DTYPES
                         and (tensor.is_contiguous() or _dense_nhwc(tensor))) else None

    def _clip_route(self, tensor, clip_type, stat_id, att):
        """gemmlowpClippingQuantize.  Per channel, Laplace or Gaussian clipping without -me: a pending correction folded in on
        channels_last, the calibration table on a contiguous half tensor (both need stat_id), ACIQ on channels_last, dynamic ACIQ
        on a contiguous half tensor (opt-in: half_dynamic).  With -me: 'half_entropy' on a contiguous half tensor, dynamic or
        from the table (opt-in: half_entropy).  Per tensor, also '<p>std': the flat route.  'mix': per channel from the statistics
        file, without -me or a pending correction, on either storage class (opt-in: native_mix)."""
        pc, one_gpu, use_ba, pending = self._facts(tensor, att)
        if not one_gpu:
            return None
        # a mid-tread or KLD object comes here by a direct call only, and only channels_last ACIQ serves it
        direct = att('mtd_quant') or att('kld')
        if not pc:
            clips = clip_type in ('laplace', 'gaus') or (isinstance(clip_type, str) and clip_type.endswith('std'))
            return 'flat_clip' if clips and not direct and self._flat_tensor(tensor) else None
        if clip_type == 'mix':
            # -c mix from the statistics file: ops.act_qdq_mix merges the candidates' tables and ends in ops.pc_qdq, which has
            # kernels for both storage classes (opt-in: native_mix).  The name routes nothing; it keeps __call__ from upcasting.
            return 'mix' if (stat_id is not None and not att('measure_entropy') and not pending and self.native_mix
                             and _storage(tensor) is not None) else None
        if clip_type not in ('laplace', 'gaus'):
            return None
        if att('measure_entropy'):
            # -me: the chain with the counting pass last, dynamic or from the table (opt-in: half_entropy)
            return 'half_entropy' if not pending and not direct and self._half_entropy(tensor, att, use_ba) else None
        storage = _storage(tensor)
        if stat_id is not None and not direct:
            if pending and storage == 'nhwc':
                return 'nhwc_bcorr'
            if storage == 'half' and ops._HALF_TABLE and ops._table_half_native(*ops.geometry(tensor), tensor.dtype) != 0:
                return 'half_table'
        if pending:
            return None
        if storage == 'nhwc':
            return 'nhwc_aciq'
        if (storage == 'half' and stat_id is None and self.half_dynamic and not direct and ops._HALF_ACIQ
                and ops._aciq_half_native(*ops.geometry(tensor), tensor.dtype, use_ba,
                                          use_ba and att('bit_alloc_prior') != 'gaus') != 0):
            return 'half_aciq'
        return None

    def _pc_route(self, tensor, stat_id, att):
        """gemmlowpQuantizeActivationPerChannel.  From the calibration table (stat_id) without -me: a pending correction folded in
        on channels_last; on a contiguous half tensor the table route under bit allocation or a pending correction, else
        'half_minmax' (ops.act_qdq_per_channel's own half route).  Then -me on channels_last byte codes or on a contiguous half
        tensor (opt-in: half_entropy), and config 2's kernels."""
        pc, one_gpu, use_ba, pending = self._facts(tensor, att)
        if not (pc and one_gpu) or att('mtd_quant') or att('kld') or att('pcq_w'):          # (by a direct call only)
            return None
        entropy = att('measure_entropy')
        if stat_id is not None and not entropy:
            storage = _storage(tensor)
            if pending and storage == 'nhwc':
                return 'nhwc_bcorr'
            if storage == 'half' and ops._HALF_TABLE and ops._table_half_native(*ops.geometry(tensor), tensor.dtype) != 0:
                return 'half_table' if use_ba or pending else 'half_minmax'
        if use_ba or pending:
            return None
        if entropy:
            if att('num_bits') <= 8 and _dense_nhwc(tensor):
                return 'nhwc_entropy'
            return 'half_entropy' if self._half_entropy(tensor, att, False) else None
        return 'minmax_pc'

    def _half_entropy(self, tensor, att, use_ba):
        """What the two 'half_entropy' routes share behind their own conditions: codes that fit a byte, the object's flag, the
        switch, a contiguous half tensor and a class of layer the route function keeps native (256 bins under bit allocation)."""
        bits = att('num_bits')
        return bool(bits <= 8 and self.half_entropy and ops._HALF_ENTROPY and _storage(tensor) == 'half'
                    and ops._entropy_half_native(*ops.geometry(tensor), tensor.dtype, 256 if use_ba else 1 << bits) != 0)

    def _midtread_route(self, tensor, att):
        """The two mid_tread_quantize_activation methods: with clipping (the per-channel one is also __call__'s branch at clipping
        'no', which has no route) and no KLD, per channel with no correction pending on channels_last or on a contiguous half tensor
        (opt-in: half_midtread), per tensor on flat storage."""
        pc, one_gpu, _, pending = self._facts(tensor, att)
        if not (att('mtd_quant') and one_gpu) or att('clipping') == 'no' or att('kld'):
            return None
        if pc:
            if pending:
                return None
            if _dense_nhwc(tensor):
                return 'nhwc_midtread'
            if (self.half_midtread and ops._HALF_MIDTREAD and _storage(tensor) == 'half'
                    and ops._midtread_half_native(*ops.geometry(tensor), tensor.dtype, bool(att('measure_entropy'))) != 0):
                return 'half_midtread'
            return None
        return 'flat_midtread' if self._flat_tensor(tensor) else None

    # The predicates of the routes, as tests, tools and DESIGN.md know them: each is a view of the decision above.  _asked is the route
    # __call__ would decide; _nhwc_aciq alone asks level 2 only, so it ignores mtd_quant and kld as gemmlowpClippingQuantize does.
    def _asked(self, tensor, stat_id=None, att=None, clip_type=None):
        """The route of __call__(tensor, stat_id=stat_id) under the lookup att, with clip_type (if given) as the clipping."""
        get = att or self._att()
        att = get if clip_type is None else lambda k: clip_type if k == 'clipping' else get(k)
        return self._route(self._branch(att, tensor), tensor, stat_id, att)

    def _half_native(self, tensor, override_att=None, stat_id=None):
        return self._asked(tensor, stat_id, self._att(override_att)) in HALF_NATIVE_ROUTES

    def _nhwc_aciq(self, tensor, clip_type, att=None):
        return self._clip_route(tensor, clip_type, None, att or self._att()) == 'nhwc_aciq'

    def _nhwc_bcorr(self, tensor, clip_type, stat_id, att=None):
        return self._asked(tensor, stat_id, att, clip_type) == 'nhwc_bcorr'

    def _nhwc_midtread(self, tensor, att=None):
        return self._asked(tensor, None, att) == 'nhwc_midtread'

    def _nhwc_entropy(self, tensor, att=None):
        return self._asked(tensor, None, att) == 'nhwc_entropy'

    def _flat_clip(self, tensor, att=None):
        return self._asked(tensor, None, att) == 'flat_clip'

    def _flat_midtread(self, tensor, att=None):
        return self._asked(tensor, None, att) == 'flat_midtread'

    def _flat_kld(self, tensor, att=None):
        return self._asked(tensor, None, att) == 'kld'

    def _half_table(self, tensor, clip_type, stat_id, att=None):
        return self._asked(tensor, stat_id, att, clip_type) in ('half_table', 'half_minmax')

    def _half_aciq(self, tensor, clip_type, stat_id, att=None):
        return self._asked(tensor, stat_id, att, clip_type) == 'half_aciq'

    def __repr__(self):
        # iq.py:124-126, printed by the manager in verbose mode
        return 'IntQuantizer - [bits: {}, clipping: {}, bit_alloc_act: {}, bit_alloc_weight: {}, bit_alloc_round: {}, pcq_w: {}, pcq_a: {}, bcorr_act: {}, bcorr_weight: {}, vcorr_weight: {}, kind: {}]'\
            .format(self.num_bits, self.clipping, self.bit_alloc_act, self.bit_alloc_weight, self.bit_alloc_round,
                    self.pcq_w, self.pcq_a, self.bcorr_act, self.bcorr_weight, self.vcorr_weight, self.stats_kind)

    # ------------------------------------------------------------------ helpers
    @property
    def _positive(self):
        return bool(self.force_positive or self.half_range)

    def _stats_table(self, stat_id, C, device, rows):
        """Device table [NSTAT, C] filled from the calibration file for `stat_id`
        (`rows`: {STAT row: (stat name, kind)}); uploaded once per (stat_id, rows, device)."""
        key = (stat_id, tuple(sorted(rows.items())), str(device), id(self.sm))
        tab = self._table_cache.get(key)
        if tab is None:
            host = torch.zeros((L.NSTAT, C), dtype=torch.float32)
            for row, (stat, kind) in rows.items():
                host[row] = _to_f32_vec(self.sm().get_tensor_stat(stat_id, stat, kind=kind), C)
            tab = host.to(device)
            self._table_cache[key] = tab
        return tab

    def _table_params(self, table, clip_type):
        """The quantization parameters of the calibration table."""
        return ops.pc_params(table, self.num_bits, self._positive, clip_type, bool(self.bit_alloc_act) and self.num_bits <= 4,
                             self.bit_alloc_prior != 'gaus', self.bit_alloc_target_act, self.bit_alloc_round)[0]

    def _table_half(self, tensor, table, clip_type):
        """The 'half_table' route: Q/DQ from the table's parameters - with a pending correction folded in - where the tensor lies."""
        qp = self._table_params(table, clip_type)
        if self.fuse_bcorr is not None:
            return ops.qdq_bias_corrected_half(tensor, qp, bool(self._take_bcorr()))
        return ops.pc_qdq(tensor, *ops.geometry(tensor), qp)

    def _act_qdq(self, tensor, id, clip_type, table):
        """ops.act_qdq_per_channel on a per-channel activation - dynamic statistics or `table`, a pending correction folded in -
        with the entropy of its codes logged where it is measured."""
        out = ops.act_qdq_per_channel(tensor, self.num_bits, positive=self._positive, clip=clip_type,
                                      bit_alloc=self.bit_alloc_act, prior_is_b=self.bit_alloc_prior != 'gaus',
                                      target=self.bit_alloc_target_act, round_mode=self.bit_alloc_round,
                                      group=self.group, stats=table, want_entropy=self.measure_entropy,
                                      bcorr=self._take_bcorr())
        if self.measure_entropy:
            out, entropy = out
            self._log_entropy(id, entropy, 'avg.entropy.act', out.numel())
        return out.view(tensor.shape)

    def _take_bcorr(self):
        """The pending bias-correction request, if this call can fold it in (no entropy measurement)."""
        if self.fuse_bcorr is None or self.measure_entropy:
            return None
        flag, self.fuse_bcorr, self.bcorr_fused = self.fuse_bcorr, None, True
        return flag

    def _log_entropy(self, id, entropy, meter, weight):
        if entropy is not None and self.logger is not None:
            def log(e=entropy):
                self.logger.log_metric(id + '.entropy', float(e), step='auto', meterId=meter, weight=weight)
            eb = getattr(ops, '_ENT_BATCH', None)
            if eb is not None:
                # inside an ops.entropy_batch block (the harness wraps a forward in one): the value exists when the block's one
                # entropy launch has run - the logger is called then, in the order of the layers, as int_quantizer.py:153,179,445
                eb.after(log)
            else:
                log()

    # ------------------------------------------------------------------ per-channel activations
    def gemmlowpQuantizeActivationPerChannel(self, tensor, id, tag="", stat_id=None, min_=None, max_=None):
        """iq.py:409-451.  Dynamic statistics: one fused pipeline on the device.  With `stat_id`
        the statistics come from the calibration file (iq.py:414,421,433)."""
        if min_ is not None or max_ is not None:
            raise NotImplementedError('explicit min_/max_ are an internal hand-off of the reference '
                                      '(iq.py:352); use gemmlowpClippingQuantize')
        route = table = None
        if stat_id is not None:                                   # (the routes that change the call need the table)
            route = self._pc_route(tensor, stat_id, self._att())
            prior_b = self.bit_alloc_prior != 'gaus'
            rows = {L.STAT_MAX: ('max', self.stats_kind)}
            if not self._positive:
                rows[L.STAT_MIN] = ('min', self.stats_kind)
            if bool(self.bit_alloc_act) and self.num_bits <= 4:
                rows[L.STAT_B if prior_b else L.STAT_STD] = ('b' if prior_b else 'std', 'mean')
            table = self._stats_table(stat_id, tensor.shape[1], tensor.device, rows)
        if route == 'nhwc_bcorr':
            return ops.qdq_bias_corrected_nhwc(tensor, self._table_params(table, 'no'), bool(self._take_bcorr()))
        if route == 'half_table':
            return self._table_half(tensor, table, 'no')
        return self._act_qdq(tensor, id, 'no', table)            # 'half_minmax', 'nhwc_entropy', 'half_entropy', 'minmax_pc': its own routes

    def gemmlowpClippingQuantize(self, tensor, id, tag="", stat_id=None, clip_type='laplace'):
        """iq.py:327-359: ACIQ clipping (laplace / gaus / <p>std), per channel when -pcq_a applies,
        otherwise per tensor with scalar statistics."""
        if clip_type == 'mix':
            return self._clipping_mix(tensor, id, stat_id, self.bit_alloc_prior != 'gaus')
        route = self._clip_route(tensor, clip_type, stat_id, self._att())
        # per tensor (iq.py:353-357) the whole tensor is ONE channel; bit allocation does not apply (iq.py:236 requires per_channel)
        # and delta is the range itself
        pc = route != 'flat_clip' and (route is not None or (self.pcq_a and _is_pc_act(tensor)))    # (every other route is per channel)
        table = None if stat_id is None else self._stats_table(stat_id, tensor.shape[1] if pc else 1, tensor.device, ACIQ_ROWS)
        if route == 'nhwc_bcorr':
            return ops.qdq_bias_corrected_nhwc(tensor, self._table_params(table, clip_type), bool(self._take_bcorr()))
        if route == 'half_table':
            return self._table_half(tensor, table, clip_type)
        if route in ('nhwc_aciq', 'half_aciq'):
            # a dense channels_last activation, or a contiguous bf16 / fp16 one with dynamic statistics: quantized where it lies
            kw = dict(positive=self._positive, clip=clip_type, bit_alloc=self.bit_alloc_act, prior_is_b=self.bit_alloc_prior != 'gaus',
                      target=self.bit_alloc_target_act, round_mode=self.bit_alloc_round)
            if route == 'half_aciq':
                return ops.aciq_qdq_half(tensor, self.num_bits, **kw)
            return ops.aciq_qdq_nhwc(tensor, self.num_bits, stats=table, **kw)
        if route == 'half_entropy':
            # a contiguous bf16 / fp16 activation with -me: the chain where it lies, its last pass counting the codes
            out, entropy = ops.aciq_qdq_half(tensor, self.num_bits, positive=self._positive, clip=clip_type, bit_alloc=self.bit_alloc_act,
                                             prior_is_b=self.bit_alloc_prior != 'gaus', target=self.bit_alloc_target_act,
                                             round_mode=self.bit_alloc_round, stats=table, want_entropy=True)
            self._log_entropy(id, entropy, 'avg.entropy.act', out.numel())
            return out
        if route == 'flat_clip':
            # half or dense channels_last: quantized where it lies, the result keeps dtype and layout
            return ops.clip_qdq_tensor(tensor, self.num_bits, positive=self._positive, clip=clip_type, stats=table)
        if pc:
            return self._act_qdq(tensor, id, clip_type, table)
        out = ops.act_qdq_per_channel(tensor, self.num_bits, positive=self._positive, clip=clip_type,
                                      bit_alloc=False, group=self.group, stats=table, whole_tensor=True)
        return out.view(tensor.shape)

    def _clipping_mix(self, tensor, id, stat_id, prior_b):
        """iq.py:310-323: `-c mix` picks the clipping value per channel from the mse_laplace / mse_gaus / mse_lowp columns of
        the statistics file (`-sm use` only: the reference looks them up by stat_id unconditionally).  A column the file
        does not have counts as NaN - every comparison False, i.e. Laplace clipping, which is also what the files the
        reference itself writes (NaN error columns) amount to."""
        if stat_id is None:
            raise ValueError("clipping 'mix' needs a statistics file (-sm use): int_quantizer.py:311-313 reads mse_* by stat_id")
        pc = self.pcq_a and _is_pc_act(tensor)
        C = tensor.shape[1] if pc else 1
        table = self._stats_table(stat_id, C, tensor.device, ACIQ_ROWS)
        mse = torch.full((3, C), float('nan'), dtype=torch.float32)
        for r, name in enumerate(('mse_laplace', 'mse_gaus', 'mse_lowp')):
            try:
                v = self.sm().get_tensor_stat(stat_id, name, 'mean')
            except KeyError:
                v = None
            if v is not None:
                mse[r] = _to_f32_vec(v, C)
        out = ops.act_qdq_mix(tensor, self.num_bits, table, mse, positive=self._positive,
                              bit_alloc=self.bit_alloc_act and pc, prior_is_b=prior_b, target=self.bit_alloc_target_act,
                              round_mode=self.bit_alloc_round, whole_tensor=not pc, want_entropy=self.measure_entropy and pc)
        if self.measure_entropy and pc:
            out, entropy = out
            self._log_entropy(id, entropy, 'avg.entropy.act', out.numel())
        return out.view(tensor.shape)

    # ------------------------------------------------------------------ weights
    def gemmlowpQuantizeWeightsPerChannel(self, tensor, id, min_=None, max_=None):
        """iq.py:453-476: rows of [OFM, IFM*K*K]; weights are replicated, never sharded."""
        out = ops.act_qdq_per_channel(tensor, self.num_bits, positive=False, clip='no',
                                      bit_alloc=self.bit_alloc_weight, prior_is_b=False,
                                      target=self.bit_alloc_target_weight, round_mode=self.bit_alloc_round,
                                      per_channel_dim=0, group=False, want_entropy=self.measure_entropy)
        if self.measure_entropy:
            out, entropy = out
            self._log_entropy(id, entropy, 'avg.entropy.weight', out.numel())
        return out.view(tensor.shape)

    # ------------------------------------------------------------------ per-tensor paths
    def gemmlowpMinMaxQuantize(self, tensor, tag="", stat_id=None):
        """iq.py:361-379."""
        if stat_id is not None:
            kmin, kmax = ('mean', 'mean') if self.stats_kind == 'mean' else ('min', 'max')
            min_ = self.sm().get_tensor_stat(stat_id, 'min', kmin)
            max_ = self.sm().get_tensor_stat(stat_id, 'max', kmax)
            if self._positive:
                min_ = 0
            return self.__gemmlowpQuantize__(tensor, max_ - min_, min_)
        avg = ('activation' in tag and 'classifier' not in tag)
        return ops.minmax_qdq_per_tensor(tensor, self.num_bits, avg_over_batch=avg, zero_min=self._positive,
                                         int_exp=self.int_exp, enforce_true_zero=self.enforce_true_zero,
                                         group=self.group).view(tensor.shape)

    def gemmlowpKldQuantize(self, tensor, tag="", stat_id=None):
        """iq.py:478-486: KLD threshold from the (per-tensor) calibration file as the clipping value."""
        min_ = self.sm().get_tensor_stat(stat_id, 'min', 'mean')
        max_ = self.sm().get_tensor_stat(stat_id, 'max', 'mean')
        kld_th = self.sm().get_tensor_stat(stat_id, 'kld_th', 'mean')
        mean = self.sm().get_tensor_stat(stat_id, 'mean', 'mean')
        range_, offset = self.alpha2DeltaOffset(kld_th, max_, min_, mean)
        return self.__gemmlowpQuantize__(tensor, range_, offset)

    def alpha2DeltaOffset(self, alpha, max_value, min_value, mean, clip2max=False):
        """iq.py:284-300 for host scalars / numpy vectors (stats-file driven callers); the
        per-channel device version lives in cnnq_pc_params."""
        alpha, max_value, min_value, mean = (np.asarray(v.cpu() if isinstance(v, torch.Tensor) else v)
                                             for v in (alpha, max_value, min_value, mean))
        if self._positive:
            delta = np.maximum(mean, 0) + alpha
            if clip2max:
                delta = np.minimum(delta, max_value)
            offset = 0
        else:
            delta = 2 * alpha
            if clip2max:
                delta = np.minimum(delta, max_value - min_value)
            offset = np.maximum(min_value, mean - alpha)
        return delta, offset

    def __gemmlowpQuantize__(self, tensor, delta, offset):
        """iq.py:605-614: scalar range/offset -> the per-tensor GEMMLOWP kernel."""
        from .. import int_quantization
        delta, offset = float(delta), float(offset)
        preserve_zero = self.enforce_true_zero and (offset + delta) > 0 and offset < 0
        # the pass is element by element: a dense channels_last tensor goes as it is, and the result keeps its layout
        x = tensor if ops._layout(tensor) == 'nhwc' else tensor.contiguous()
        return int_quantization.float2gemmlowp(x, delta, offset, self.num_bits, self.int_exp, preserve_zero, None)

    # ------------------------------------------------------------------ mid-tread (config 5)
    def mid_tread_quantize_weights_per_channel(self, tensor, id):
        """iq.py:147-156."""
        out, entropy = ops.mid_tread_qdq(tensor, self.bit_alloc_target_weight, clip=False, sym=True,
                                         per_channel_dim=0, group=False, want_entropy=self.measure_entropy)
        self._log_entropy(id, entropy, 'avg.entropy.weight', out.numel())
        return out.view(tensor.shape)

    def mid_tread_quantize_activation(self, tensor, id):
        """iq.py:158-168."""
        if self.pcq_a and _is_pc_act(tensor):
            return self.mid_tread_quantize_activation_per_channel(tensor, id)
        if self._midtread_route(tensor, self._att()) == 'flat_midtread':
            return ops.mid_tread_qdq_tensor(tensor, self.bit_alloc_target_act, sym=not self._positive)
        out, _ = ops.mid_tread_qdq(tensor, self.bit_alloc_target_act, clip=True, sym=not self._positive,
                                   whole_tensor=True, group=self.group, want_entropy=self.measure_entropy)
        return out.view(tensor.shape)

    def mid_tread_quantize_activation_per_channel(self, tensor, id):
        """iq.py:170-183."""
        route = self._midtread_route(tensor, self._att())
        if route == 'nhwc_midtread':
            # a dense channels_last activation: quantized where it lies, the result keeps layout and dtype
            out, entropy = ops.mid_tread_qdq_nhwc(tensor, self.bit_alloc_target_act, sym=not self._positive,
                                                  want_entropy=self.measure_entropy)
        elif route == 'half_midtread':
            # a contiguous bf16 / fp16 activation: quantized where it lies, the result keeps the dtype
            out, entropy = ops.mid_tread_qdq_half(tensor, self.bit_alloc_target_act, sym=not self._positive,
                                                  want_entropy=self.measure_entropy)
        else:
            out, entropy = ops.mid_tread_qdq(tensor, self.bit_alloc_target_act, clip=True, sym=not self._positive,
                                             group=self.group, want_entropy=self.measure_entropy)
            out = out.view(tensor.shape)
        self._log_entropy(id, entropy, 'avg.entropy.act', tensor.numel())
        return out


# how iq.py:92-122 calls the branch method of each of _branch's answers
BRANCH_CALLS = {
    'kld': lambda q, t, id, tag, stat_id: q.gemmlowpKldQuantize(t, tag, stat_id=stat_id),
    'midtread': lambda q, t, id, tag, stat_id: q.mid_tread_quantize_activation(t, id),
    'clip': lambda q, t, id, tag, stat_id: q.gemmlowpClippingQuantize(t, id, tag, stat_id=stat_id, clip_type=q.clipping),
    'midtread_w': lambda q, t, id, tag, stat_id: q.mid_tread_quantize_weights_per_channel(t, id),
    'weights': lambda q, t, id, tag, stat_id: q.gemmlowpQuantizeWeightsPerChannel(t, id),
    'midtread_pc': lambda q, t, id, tag, stat_id: q.mid_tread_quantize_activation_per_channel(t, id),
    'pc': lambda q, t, id, tag, stat_id: q.gemmlowpQuantizeActivationPerChannel(t, id, tag, stat_id=stat_id),
    'minmax': lambda q, t, id, tag, stat_id: q.gemmlowpMinMaxQuantize(t, tag, stat_id=stat_id)}


def int_quantizer(qtype, quant_params):
    """iq.py:626-632: 'int4' -> IntQuantizer(4, params); bare 'int' -> 32 bits."""
    if len(qtype) > len('int'):
        size = int(qtype[len('int'):])
    else:
        size = 32
    return IntQuantizer(size, quant_params)


__all__ = ['IntQuantizer', 'int_quantizer', 'math', 'upcast_fallback', 'HALF_DTYPES']
