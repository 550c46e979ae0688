"""`IntQuantizer` - the op surface of the reference's quantizer
(pytorch_quantizer/quantization/qtypes/int_quantizer.py:56-632, "iq.py" below) re-hosted on the
MI355X kernels: same constructor keys, same `__call__(tensor, id, tag, stat_id, override_att)`,
same externally mutated attributes and the same dispatch order, so the reference's manager and
`inference_sim.py` drive it unchanged.  What differs is below the surface: every branch is a
handful of launches into libcnnq_hip.so (statistics -> parameters -> fused Q/DQ on native NCHW)
with no transposed copies, no elementwise temporaries and no host synchronisation.

Only the arithmetic lives on the device; there is no CPU path (CPU tensors raise)."""
import math

import numpy as np
import torch

from .. import _lib as L
from .. import distributed as D
from .. import ops

# bf16 / fp16 activations.  Configs 1 and 2 (per-tensor and per-channel min/max, dynamic or from a statistics file) run on
# their half-precision kernels.  Every other path that meets a half tensor goes through upcast_fallback, the ONE place that
# upcasts: it computes on x.float() and returns .to(x.dtype), and counts the call (HALF_FALLBACKS) so that tests can prove
# configs 1 and 2 never arrive there.
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


def _to_f32_vec(v, C):
    a = np.asarray(v, dtype=np.float32).reshape(-1)
    if a.size == 1 and C > 1:
        a = np.repeat(a, C)
    return torch.from_numpy(np.ascontiguousarray(a))


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
        # dynamic ACIQ clipping of a contiguous bf16 / fp16 activation where it lies (_half_aciq): opt-in
        # per quantizer object - the inference manager sets it on the quantizers it builds; one constructed directly keeps the
        # upcast route
        self.half_dynamic = False

    # ------------------------------------------------------------------ dispatch, iq.py:92-122
    def __call__(self, tensor, id, tag="", stat_id=None, override_att=None):
        if (isinstance(tensor, torch.Tensor) and tensor.dtype in HALF_DTYPES
                and not self._half_native(tensor, override_att, stat_id)
                and not self._half_table(tensor, self._att(override_att)('clipping'), stat_id, self._att(override_att))
                and not self._half_aciq(tensor, self._att(override_att)('clipping'), stat_id, self._att(override_att))
                and not self._nhwc_midtread(tensor, self._att(override_att))
                and not self._nhwc_entropy(tensor, self._att(override_att)) and not self._flat_clip(tensor, self._att(override_att))
                and not self._flat_midtread(tensor, self._att(override_att)) and not self._flat_kld(tensor, self._att(override_att))):
            return upcast_fallback(self.__call__, tensor, id, tag, stat_id, override_att)
        if override_att is not None:
            orig_att = getattr(self, override_att[0])
            setattr(self, override_att[0], override_att[1])
        try:
            if self.kld:
                res = self.gemmlowpKldQuantize(tensor, tag, stat_id=stat_id)
            elif self.clipping != 'no':
                if self.mtd_quant:
                    res = self.mid_tread_quantize_activation(tensor, id)
                else:
                    res = self.gemmlowpClippingQuantize(tensor, id, tag, stat_id=stat_id, clip_type=self.clipping)
            elif self.pcq_w:
                if self.mtd_quant:
                    res = self.mid_tread_quantize_weights_per_channel(tensor, id)
                else:
                    res = self.gemmlowpQuantizeWeightsPerChannel(tensor, id)
            elif self.pcq_a and _is_pc_act(tensor):
                if self.mtd_quant:
                    res = self.mid_tread_quantize_activation_per_channel(tensor, id)
                else:
                    res = self.gemmlowpQuantizeActivationPerChannel(tensor, id, tag, stat_id=stat_id)
            else:
                res = self.gemmlowpMinMaxQuantize(tensor, tag, stat_id=stat_id)
        finally:
            if override_att is not None:
                setattr(self, override_att[0], orig_att)
        return res

    def _att(self, override_att=None):
        """The attribute lookup the dispatch predicates share: __call__'s override_att pair wins over the attribute."""
        return lambda k: override_att[1] if override_att is not None and override_att[0] == k else getattr(self, k)

    def _one_gpu(self):
        """Replicated data excluded (group is not False), a batch that is not sharded, no forced exchange."""
        return self.group is not False and D.world_size(self.group) == 1 and not D.forced_exchange()

    def _half_native(self, tensor, override_att=None, stat_id=None):
        """Whether a bf16 / fp16 tensor takes a path with half kernels: config 2 (gemmlowpQuantizeActivationPerChannel without
        clipping, bit allocation, entropy, a bias correction to fold in or a sharded batch), config 1 (gemmlowpMinMaxQuantize),
        config 3 on a dense channels_last tensor (_nhwc_aciq: gemmlowpClippingQuantize's native route), or - stat_id given - a
        pending bias correction on a dense channels_last tensor (_nhwc_bcorr).  Config 5 on a dense channels_last tensor has half
        kernels too, but is asked separately (_nhwc_midtread): the answers given here for mtd_quant are pinned by tests."""
        att = self._att(override_att)
        if att('kld'):
            return False
        if self._nhwc_bcorr(tensor, att('clipping'), stat_id, att):
            return True
        if att('clipping') != 'no':
            return not att('mtd_quant') and self._nhwc_aciq(tensor, att('clipping'), att)
        if att('pcq_w'):
            return False
        if att('pcq_a') and _is_pc_act(tensor):
            return (not att('mtd_quant') and not att('measure_entropy') and self.fuse_bcorr is None
                    and not (att('bit_alloc_act') and att('num_bits') <= 4) and self._one_gpu())
        return True

    # The four channels_last routes.  Each wants a dense channels_last tensor (_dense_nhwc) on the per-channel activation branch and
    # one GPU's own data (_one_gpu), and reads shape, strides and attributes only; att: the lookup of _att.  _nhwc_midtread and
    # _nhwc_entropy are kept apart from _half_native, which goes on answering False for mtd_quant and measure_entropy: the tests
    # of the earlier channels_last routes pin those answers, so __call__ asks all three before it upcasts.
    def _nhwc_aciq(self, tensor, clip_type, att=None):
        """gemmlowpClippingQuantize runs on the storage as it is (ops.aciq_qdq_nhwc): Laplace or Gaussian
        clipping, no entropy measurement, no bias correction to fold in."""
        att = att or (lambda k: getattr(self, k))
        return (bool(att('pcq_a')) and _is_pc_act(tensor) and clip_type in ('laplace', 'gaus') and _dense_nhwc(tensor)
                and not att('measure_entropy') and self.fuse_bcorr is None and self._one_gpu())

    def _nhwc_bcorr(self, tensor, clip_type, stat_id, att=None):
        """The per-channel activation branches (min/max, Laplace or Gaussian clipping) fold a pending bias correction in on the
        storage as it is (ops.qdq_bias_corrected_nhwc): calibrated statistics (stat_id: the product requests
        the correction only under -sm use, so only the table-driven form exists; without it False), a pending fuse_bcorr, no
        entropy measurement."""
        att = att or (lambda k: getattr(self, k))
        return (stat_id is not None and self.fuse_bcorr is not None and bool(att('pcq_a')) and _is_pc_act(tensor)
                and clip_type in ('no', 'laplace', 'gaus') and not (clip_type == 'no' and att('pcq_w')) and _dense_nhwc(tensor)
                and not att('mtd_quant') and not att('kld') and not att('measure_entropy') and self._one_gpu())

    def _nhwc_midtread(self, tensor, att=None):
        """mid_tread_quantize_activation_per_channel runs on the storage as it is (ops.mid_tread_qdq_nhwc):
        mid-tread quantization with clipping, no KLD, no bias correction to fold in; the entropy measurement may be on or off."""
        get = att or self._att()
        return (bool(get('mtd_quant')) and get('clipping') != 'no' and not get('kld')
                and bool(get('pcq_a')) and _is_pc_act(tensor) and _dense_nhwc(tensor)
                and self.fuse_bcorr is None and self._one_gpu())

    def _nhwc_entropy(self, tensor, att=None):
        """gemmlowpQuantizeActivationPerChannel measures the entropy of its codes on the storage as it is (ops.act_qdq_per_channel's
        counting route): measure_entropy without clipping - no KLD, no weight branch in front of it, no
        mid-tread, no bit allocation in effect, codes that fit a byte - and no bias correction pending (with -me the layer
        corrects afterwards); dynamic or with stat_id.  Config 3 with -me is one predicate away (ops.aciq_qdq_nhwc takes
        want_entropy) and stays on the copy route, as its tests pin it."""
        get = att or self._att()
        return (bool(get('measure_entropy')) and bool(get('pcq_a')) and _is_pc_act(tensor)
                and get('clipping') == 'no' and not get('pcq_w') and not get('mtd_quant') and not get('kld')
                and not (get('bit_alloc_act') and get('num_bits') <= 4) and get('num_bits') <= 8 and _dense_nhwc(tensor)
                and self.fuse_bcorr is None and self._one_gpu())

    # The three per-tensor routes over flat storage.  One parameter set serves the whole tensor, so the element
    # order does not matter: a contiguous bf16 / fp16 tensor and a dense channels_last tensor of any of the three dtypes are
    # quantized where they lie.  A contiguous fp32 tensor keeps ops.act_qdq_per_channel(whole_tensor=True) / ops.mid_tread_qdq: its
    # dynamic statistics differ from the flat rows' in the last bits.  Kept apart from _half_native for the reason above: tests pin it.
    def _flat_tensor(self, tensor):
        """On the device and either bf16 / fp16, contiguous or dense channels_last, or fp32 dense channels_last; not empty."""
        if not getattr(tensor, 'is_cuda', False) or tensor.numel() == 0:
            return False
        if tensor.dtype in HALF_DTYPES:
            return tensor.is_contiguous() or _dense_nhwc(tensor)
        return tensor.dtype == torch.float32 and _dense_nhwc(tensor)

    def _flat_clip(self, tensor, att=None):
        """The per-tensor tail of gemmlowpClippingQuantize runs on ops.clip_qdq_tensor: the clipping branch where -pcq_a does not
        apply, 'laplace', 'gaus' or '<p>std' (not 'mix': its candidates come from error columns), no mid-tread, no KLD, one GPU."""
        get = att or self._att()
        clip = get('clipping')
        return (not get('kld') and not get('mtd_quant') and not (get('pcq_a') and _is_pc_act(tensor))
                and (clip in ('laplace', 'gaus') or (isinstance(clip, str) and clip.endswith('std')))
                and self._one_gpu() and self._flat_tensor(tensor))

    def _flat_midtread(self, tensor, att=None):
        """mid_tread_quantize_activation without -pcq_a runs on ops.mid_tread_qdq_tensor."""
        get = att or self._att()
        return (not get('kld') and bool(get('mtd_quant')) and get('clipping') != 'no' and not (get('pcq_a') and _is_pc_act(tensor))
                and self._one_gpu() and self._flat_tensor(tensor))

    def _flat_kld(self, tensor, att=None):
        """gemmlowpKldQuantize needs no upcast: __gemmlowpQuantize__ hands a half tensor, contiguous or dense channels_last, to
        ops.pt_qdq's half kernel as it is.  Nothing is routed by this: it only keeps __call__ from upcasting."""
        get = att or self._att()
        return (bool(get('kld')) and getattr(tensor, 'is_cuda', False) and tensor.dtype in HALF_DTYPES
                and (tensor.is_contiguous() or _dense_nhwc(tensor)))

    def _half_table(self, tensor, clip_type, stat_id, att=None):
        """The per-channel activation branches quantize a contiguous bf16 / fp16 tensor from the calibration table where it lies
        (DESIGN.md section 24): stat_id given (everything dynamic keeps its route), min/max, Laplace or Gaussian clipping, with or
        without bit allocation and a pending bias correction (ops.qdq_bias_corrected_half, else ops.pc_qdq), no mid-tread, KLD or
        entropy measurement, one GPU's own data, the switch CNNQ_HALF_TABLE on and a class of layer the route function keeps
        native.  Kept apart from _half_native, whose answers are pinned by tests; shape, strides and attributes only."""
        att = att or (lambda k: getattr(self, k))
        if not (stat_id is not None and getattr(tensor, 'is_cuda', False) and tensor.dtype in HALF_DTYPES and tensor.dim() == 4
                and tensor.is_contiguous() and tensor.numel() > 0):
            return False
        if not (bool(att('pcq_a')) and _is_pc_act(tensor) and clip_type in ('no', 'laplace', 'gaus')
                and not (clip_type == 'no' and att('pcq_w')) and not att('mtd_quant') and not att('kld')
                and not att('measure_entropy') and self._one_gpu() and ops._HALF_TABLE):
            return False
        N, C, HW = ops.geometry(tensor)
        return ops._table_half_native(N, C, HW, tensor.dtype) != 0

    def _half_aciq(self, tensor, clip_type, stat_id, att=None):
        """gemmlowpClippingQuantize quantizes a contiguous bf16 / fp16 tensor with DYNAMIC statistics where it lies
        (ops.aciq_qdq_half): half_dynamic set on this object, no stat_id (calibrated statistics are
        _half_table's), Laplace or Gaussian clipping with or without bit allocation, no mid-tread, KLD or entropy measurement, no
        bias correction to fold in, one GPU's own data, the switch CNNQ_HALF_ACIQ on and a class of layer the route function keeps
        native.  Kept apart from _half_native, whose answers are pinned by tests; shape, strides and attributes only."""
        att = att or (lambda k: getattr(self, k))
        if not (self.half_dynamic and stat_id is None and getattr(tensor, 'is_cuda', False) and tensor.dtype in HALF_DTYPES
                and tensor.dim() == 4 and tensor.is_contiguous() and tensor.numel() > 0):
            return False
        if not (bool(att('pcq_a')) and _is_pc_act(tensor) and clip_type in ('laplace', 'gaus') and not att('mtd_quant')
                and not att('kld') and not att('measure_entropy') and self.fuse_bcorr is None and self._one_gpu()
                and ops._HALF_ACIQ):
            return False
        N, C, HW = ops.geometry(tensor)
        use_ba = bool(att('bit_alloc_act')) and att('num_bits') <= 4
        return ops._aciq_half_native(N, C, HW, tensor.dtype, use_ba, use_ba and att('bit_alloc_prior') != 'gaus') != 0

    def _table_half(self, tensor, table, clip_type, prior_b):
        """The _half_table route: the parameters of the calibration table, then Q/DQ - with a pending correction folded in - where
        the tensor lies."""
        use_ba = bool(self.bit_alloc_act) and self.num_bits <= 4
        qp, _ = ops.pc_params(table, self.num_bits, self._positive, clip_type, use_ba, prior_b, self.bit_alloc_target_act,
                              self.bit_alloc_round)
        if self.fuse_bcorr is not None:
            return ops.qdq_bias_corrected_half(tensor, qp, bool(self._take_bcorr()))
        N, C, HW = ops.geometry(tensor)
        return ops.pc_qdq(tensor, N, C, HW, qp)

    def _bcorr_nhwc(self, tensor, table, clip_type, prior_b):
        """The _nhwc_bcorr route: the parameters of the calibration table, then Q/DQ and correction where the tensor lies."""
        use_ba = bool(self.bit_alloc_act) and self.num_bits <= 4
        qp, _ = ops.pc_params(table, self.num_bits, self._positive, clip_type, use_ba, prior_b, self.bit_alloc_target_act,
                              self.bit_alloc_round)
        return ops.qdq_bias_corrected_nhwc(tensor, qp, bool(self._take_bcorr()))

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
        prior_b = self.bit_alloc_prior != 'gaus'
        use_ba = bool(self.bit_alloc_act) and self.num_bits <= 4
        table = None
        if stat_id is not None:
            C = tensor.shape[1]
            rows = {L.STAT_MAX: ('max', self.stats_kind)}
            if not self._positive:
                rows[L.STAT_MIN] = ('min', self.stats_kind)
            if use_ba:
                rows[L.STAT_B if prior_b else L.STAT_STD] = ('b' if prior_b else 'std', 'mean')
            table = self._stats_table(stat_id, C, tensor.device, rows)
            if self._nhwc_bcorr(tensor, 'no', stat_id):
                return self._bcorr_nhwc(tensor, table, 'no', prior_b)
            if (use_ba or self.fuse_bcorr is not None) and self._half_table(tensor, 'no', stat_id):
                # (plain min/max from the table without a correction: act_qdq_per_channel's own half route below)
                return self._table_half(tensor, table, 'no', prior_b)
        out = ops.act_qdq_per_channel(tensor, self.num_bits, positive=self._positive, clip='no',
                                      bit_alloc=self.bit_alloc_act, prior_is_b=prior_b,
                                      target=self.bit_alloc_target_act, round_mode=self.bit_alloc_round,
                                      group=self.group, stats=table, want_entropy=self.measure_entropy,
                                      bcorr=self._take_bcorr())
        if self.measure_entropy:
            out, entropy = out
            self._log_entropy(id, entropy, 'avg.entropy.act', out.numel())
        return out.view(tensor.shape)

    def gemmlowpClippingQuantize(self, tensor, id, tag="", stat_id=None, clip_type='laplace'):
        """iq.py:327-359: ACIQ clipping (laplace / gaus / <p>std), per channel when -pcq_a applies,
        otherwise per tensor with scalar statistics."""
        prior_b = self.bit_alloc_prior != 'gaus'
        if clip_type == 'mix':
            return self._clipping_mix(tensor, id, stat_id, prior_b)
        if self.pcq_a and _is_pc_act(tensor):
            table = None
            if stat_id is not None:
                C = tensor.shape[1]
                rows = {L.STAT_MIN: ('min', 'mean'), L.STAT_MAX: ('max', 'mean'), L.STAT_MEAN: ('mean', 'mean'),
                        L.STAT_B: ('b', 'mean'), L.STAT_STD: ('std', 'mean')}
                table = self._stats_table(stat_id, C, tensor.device, rows)
                if self._nhwc_bcorr(tensor, clip_type, stat_id):
                    return self._bcorr_nhwc(tensor, table, clip_type, prior_b)
                if self._half_table(tensor, clip_type, stat_id):
                    return self._table_half(tensor, table, clip_type, prior_b)
            if self._nhwc_aciq(tensor, clip_type):
                # a dense channels_last activation: quantized where it lies, the result keeps layout and dtype
                return ops.aciq_qdq_nhwc(tensor, self.num_bits, positive=self._positive, clip=clip_type,
                                         bit_alloc=self.bit_alloc_act, prior_is_b=prior_b, target=self.bit_alloc_target_act,
                                         round_mode=self.bit_alloc_round, stats=table)
            if self._half_aciq(tensor, clip_type, stat_id):
                # a contiguous bf16 / fp16 activation, dynamic statistics: quantized where it lies, the result keeps the dtype
                return ops.aciq_qdq_half(tensor, self.num_bits, positive=self._positive, clip=clip_type,
                                         bit_alloc=self.bit_alloc_act, prior_is_b=prior_b, target=self.bit_alloc_target_act,
                                         round_mode=self.bit_alloc_round)
            out = ops.act_qdq_per_channel(tensor, self.num_bits, positive=self._positive, clip=clip_type,
                                          bit_alloc=self.bit_alloc_act, prior_is_b=prior_b,
                                          target=self.bit_alloc_target_act, round_mode=self.bit_alloc_round,
                                          group=self.group, stats=table, want_entropy=self.measure_entropy,
                                          bcorr=self._take_bcorr())
            if self.measure_entropy:
                out, entropy = out
                self._log_entropy(id, entropy, 'avg.entropy.act', out.numel())
            return out.view(tensor.shape)
        # per-tensor branch (iq.py:353-357): the whole tensor is ONE channel; bit allocation does not
        # apply (iq.py:236 requires per_channel) and delta is the range itself
        table = None
        if stat_id is not None:
            rows = {L.STAT_MIN: ('min', 'mean'), L.STAT_MAX: ('max', 'mean'), L.STAT_MEAN: ('mean', 'mean'),
                    L.STAT_B: ('b', 'mean'), L.STAT_STD: ('std', 'mean')}
            table = self._stats_table(stat_id, 1, tensor.device, rows)
        if self._flat_clip(tensor, self._att(('clipping', clip_type))):
            # half or dense channels_last: quantized where it lies, the result keeps dtype and layout
            return ops.clip_qdq_tensor(tensor, self.num_bits, positive=self._positive, clip=clip_type, stats=table)
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
        rows = {L.STAT_MIN: ('min', 'mean'), L.STAT_MAX: ('max', 'mean'), L.STAT_MEAN: ('mean', 'mean'),
                L.STAT_B: ('b', 'mean'), L.STAT_STD: ('std', 'mean')}
        table = self._stats_table(stat_id, C, tensor.device, rows)
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
        if self._flat_midtread(tensor):
            return ops.mid_tread_qdq_tensor(tensor, self.bit_alloc_target_act, sym=not self._positive)
        out, _ = ops.mid_tread_qdq(tensor, self.bit_alloc_target_act, clip=True, sym=not self._positive,
                                   whole_tensor=True, group=self.group, want_entropy=self.measure_entropy)
        return out.view(tensor.shape)

    def mid_tread_quantize_activation_per_channel(self, tensor, id):
        """iq.py:170-183."""
        if self._nhwc_midtread(tensor):
            # a dense channels_last activation: quantized where it lies, the result keeps layout and dtype
            out, entropy = ops.mid_tread_qdq_nhwc(tensor, self.bit_alloc_target_act, sym=not self._positive,
                                                  want_entropy=self.measure_entropy)
        else:
            out, entropy = ops.mid_tread_qdq(tensor, self.bit_alloc_target_act, clip=True, sym=not self._positive,
                                             group=self.group, want_entropy=self.measure_entropy)
            out = out.view(tensor.shape)
        self._log_entropy(id, entropy, 'avg.entropy.act', tensor.numel())
        return out


def int_quantizer(qtype, quant_params):
    """iq.py:626-632: 'int4' -> IntQuantizer(4, params); bare 'int' -> 32 bits."""
    if len(qtype) > len('int'):
        size = int(qtype[len('int'):])
    else:
        size = 32
    return IntQuantizer(size, quant_params)


__all__ = ['IntQuantizer', 'int_quantizer', 'math', 'upcast_fallback', 'HALF_DTYPES']
