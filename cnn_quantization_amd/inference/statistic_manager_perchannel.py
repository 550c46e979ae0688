"""Per-channel calibration statistics: `-sm collect` computes them, `-sm use` serves them.
Mirror of pytorch_quantizer/quantization/inference/statistic_manager_perchannel.py ("smpc.py"):
same constructor, `save_tensor_stats`, `get_tensor_stat`, `__exit__` and the SAME on-disk format
(`~/mxt-sim/statistics/per_channel/<name>/<name>_statistics_perchannel_summary.pkl`: a pickled
dict layer-id -> DataFrame with float32 columns {min,mean,max}_<stat>, one row per channel), so
files written by either implementation are interchangeable.

The seven statistics of one batch come from two coalesced passes over the activation on the
device (cnnq_pc_moments + cnnq_pc_absdev) and ONE device->host copy of a [7, C] table, instead
of a transposed copy, nine full-tensor reductions and seven synchronising copies
(smpc.py:51-79,112).
collect_route decides once per tensor how it is taken: 'nhwc' - a dense channels_last activation of fp32 /
bf16 / fp16 is read where it lies (ops.pc_stats_nhwc, DESIGN.md section 18: no layout copy, no upcast); 'half' - a contiguous
bf16 / fp16 activation is read in its own dtype (ops.pc_stats_half); None - every other tensor takes the
NCHW kernels on a contiguous float32 copy.  collects_native_nhwc and collects_native_half are its boolean views.
With collect_err the answer is None unless the manager opted in (native_err, which the inference manager sets): then a channels_last
activation answers 'nhwc' and its error columns come from the same storage too (ops.pc_quant_errors_nhwc);
with native_err_half on top (the inference manager sets both) a contiguous bf16 / fp16 activation answers 'half' and its error
columns are measured in its own dtype (ops.pc_quant_errors_half).
With batch_avg (-sba: a channel's max / min is the mean over the batch of the per-sample extrema, smpc.py:72-78) the answer is None
unless the manager opted in (native_batch_avg, which the inference manager sets) and collect_err is off: then both routes take the
(n, c) extrema from one more read of the same storage (ops.pc_sample_extrema_nhwc / ops.pc_sample_extrema_half).

`collect_err=True` adds the six clipping-error columns the reference declares (smpc.py:24-32: mse_lowp, mse_gaus,
mse_laplace, cos_lowp, cos_gaus, cos_laplace; formulas smpc.py:80-100) - the columns `-sm use -c mix` (iq.py:310-323)
compares per channel.  The reference never fills them (nothing passes it the quantized tensors, so its files hold NaN
there); here every batch measures exactly the three quantizations `-c mix` chooses between: the candidates are built from
the batch's own table (ops.mix_candidates) and their errors come from one more read of the activation
(ops.pc_quant_errors: no quantized tensor is materialised), recorded through the same single device->host copy.  What
the candidates need besides the table - bit width, half range, the bit-allocation settings - belongs to the layer's
activation quantizer: `err_settings`, see save_tensor_stats.  A caller-supplied `tensors_q` stays ignored; a batch
sharded over ranks is not supported with collect_err."""
import os
import pickle
import shutil

import numpy as np
import pandas as pd
import torch

from .. import _lib as L
from .. import distributed as D
from .. import ops
from ..utils.misc import Singleton
from .statistic_manager import Collector, base_dir, batch_extrema_sums, checkpointed, summary_columns

SAVE_FULL_STATS = False
_ROW = {'max': L.STAT_MAX, 'min': L.STAT_MIN, 'std': L.STAT_STD, 'mean': L.STAT_MEAN,
        'kurtosis': L.STAT_KURT, 'b': L.STAT_B, 'std_pos': L.STAT_STD_POS}


ERR_NAMES = ('mse_lowp', 'mse_gaus', 'mse_laplace', 'cos_lowp', 'cos_gaus', 'cos_laplace')


def collect_route(manager, tensor, force_global_min_max=False):
    """How save_tensor_stats takes this tensor: 'nhwc' - on its channels_last storage (ops.pc_stats_nhwc),
    'half' - contiguous, in its own dtype (ops.pc_stats_half) - or None: ops.pc_stats on a contiguous float32 copy.  Each fact
    once, in this order: the manager - no error columns (with native_err: 'nhwc' measures them too, 'half' with native_err_half as well), the extrema
    of the whole batch (batch_avg off, or the caller forces them - or, with native_batch_avg, ops._SBA_NATIVE on and no error columns, the
    per-sample extrema of ops.pc_sample_extrema_*, whose route word is asked after the others); the storage class - 'nhwc': dense channels_last and not contiguous, a dtype the kernels have, the channels_last switch
    on; 'half': a contiguous non-empty 4-D bf16 / fp16 CUDA activation with a spatial extent; the group - one process, no forced
    exchange; last the class's route function.  Shape, strides and attributes only: nothing touches the device."""
    err = manager.collect_err
    sba = manager.batch_avg and not force_global_min_max
    if (err and not getattr(manager, 'native_err', False)) \
            or (sba and (err or not getattr(manager, 'native_batch_avg', False) or not ops._SBA_NATIVE)) \
            or not isinstance(tensor, torch.Tensor):
        return None
    if tensor.dtype in ops._ACT_DTYPES and ops._NHWC and ops._layout(tensor) == 'nhwc':
        route = 'nhwc'
    elif err and not getattr(manager, 'native_err_half', False):
        return None
    elif (tensor.is_cuda and tensor.dtype in ops._HALF_DTYPES and tensor.dim() == 4 and tensor.numel() > 0 and tensor.is_contiguous()
            and (tensor.shape[2] > 1 or tensor.shape[3] > 1)):
        route = 'half'
    else:
        return None
    if D.world_size(manager.group) > 1 or D.forced_exchange():
        return None
    if route == 'nhwc':
        N, C = tensor.shape[0], tensor.shape[1]
        native = ops._stats_nhwc_native(tensor.numel() // C, C, tensor.dtype)
        if native and err:
            native = ops._qerr_nhwc_native(N, tensor.numel() // (N * C), C, tensor.dtype)
        if native and sba:
            native = ops._sample_extrema_nhwc_native(N, tensor.numel() // (N * C), C, tensor.dtype)
    else:
        native = ops._stats_half_native(*ops.geometry(tensor), tensor.dtype)
        if native and err:
            native = ops._qerr_half_native(*ops.geometry(tensor), tensor.dtype)
        if native and sba:
            native = ops._sample_extrema_half_native(*ops.geometry(tensor), tensor.dtype)
    return route if native else None


def collects_native_nhwc(manager, tensor, force_global_min_max=False):
    """Whether collect_route answers 'nhwc'."""
    return collect_route(manager, tensor, force_global_min_max) == 'nhwc'


def collects_native_half(manager, tensor, force_global_min_max=False):
    """Whether collect_route answers 'half'."""
    return collect_route(manager, tensor, force_global_min_max) == 'half'


class StatisticManagerPerChannel(Collector, metaclass=Singleton):
    collect_route = collect_route       # the face inference_quantization_manager._route asks

    def __init__(self, folder, load_stats, stats=('max', 'min', 'std', 'mean', 'kurtosis', 'b', 'std_pos'),
                 batch_avg=False, collect_err=False, group=None, err_settings=None, native_err=False,
                 native_err_half=False, native_batch_avg=False):
        self.name = folder
        self.folder = os.path.join(base_dir(), 'statistics/per_channel', folder)
        self.stats_names = list(stats)
        if collect_err:
            if D.world_size(group) > 1:
                raise NotImplementedError('collect_err with a batch sharded over ranks (the row records are local to a sample)')
            self.stats_names += [n for n in ERR_NAMES if n not in self.stats_names]   # smpc.py:24-32, in that order
        self.collect_err = collect_err
        # the route 'nhwc' with collect_err: opt-in per object; the inference manager opts in
        self.native_err = native_err
        # the route 'half' with collect_err: opt-in per object on top of native_err
        self.native_err_half = native_err_half
        # batch_avg on the routes 'nhwc' and 'half' (DESIGN.md section 33): opt-in per object; the inference manager opts in
        self.native_batch_avg = native_batch_avg
        # what the three candidates need besides the table: a dict {num_bits, positive, bit_alloc, prior_is_b, target,
        # round_mode} (the arguments of ops.mix_candidates) or a callable (tag, half_range) -> such a dict
        self.err_settings = err_settings
        self.batch_avg = batch_avg
        self.group = group
        self.save_stats = not load_stats
        if load_stats:
            stats_file = os.path.join(self.folder, '%s_statistics_perchannel_summary.pkl' % self.name)
            assert os.path.exists(stats_file), stats_file
            with open(stats_file, 'rb') as f:
                self.stats = pickle.load(f)
        else:
            self.stats = {}

    def save_tensor_stats(self, tensor, tag, id, tensors_q={}, force_global_min_max=False, half_range=False,
                          err_settings=None, *, route=None):
        """smpc.py:45-125.  half_range / err_settings matter with collect_err only: err_settings (a dict, see __init__)
        overrides the manager's own for this call; a callable provider is asked with (tag, half_range).  route: collect_route's
        answer, from a caller that has asked already (None: ask here)."""
        # FC and 1x1-spatial outputs are not per-channel quantized (smpc.py:47-48)
        if len(tensor.shape) < 3 or (tensor.shape[2] == 1 and tensor.shape[3] == 1):
            return
        need = dict(need_b='b' in self.stats_names or self.collect_err, need_kurt='kurtosis' in self.stats_names,
                    need_relu='std_pos' in self.stats_names)
        route = route or collect_route(self, tensor, force_global_min_max)
        if route:
            # the table from the channels_last storage as it lies, or from the tensor in its own dtype (23)
            table, _ = (ops.pc_stats_nhwc if route == 'nhwc' else ops.pc_stats_half)(tensor.detach(), **need)
            if self.batch_avg and not force_global_min_max:
                # mean over the batch of the per-sample extrema (smpc.py:72,78), the (n, c) extrema from one more read of the storage
                # (DESIGN.md section 33); the fp64 sums and the division are the expressions of the fp32 branch below: the same bits
                rows = (ops.pc_sample_extrema_nhwc if route == 'nhwc' else ops.pc_sample_extrema_half)(tensor.detach())
                smax, smin, cnt = batch_extrema_sums(rows, tensor.shape[0], self.group)
                table[L.STAT_MAX] = (smax / cnt).float()
                table[L.STAT_MIN] = (smin / cnt).float()
            if self.collect_err:
                # the same three candidates as below, measured on the channels_last storage or on the
                # contiguous tensor in its own dtype (31); the table's min / max rows are x's exact extrema (no batch_avg on
                # these routes)
                qp_l, qp_g, qp_p = ops.mix_candidates(table, **self._err_settings(tag, half_range, err_settings))
                errors = ops.pc_quant_errors_nhwc if route == 'nhwc' else ops.pc_quant_errors_half
                err = errors(tensor.detach(), (qp_p, qp_g, qp_l), mm=table[[L.STAT_MIN, L.STAT_MAX]])
                table = torch.cat([table, err])
            return self._record(id, table)
        N, C = tensor.shape[0], tensor.shape[1]
        HW = tensor.numel() // (N * C)
        x = tensor.detach().contiguous()
        settings = self._err_settings(tag, half_range, err_settings) if self.collect_err else None
        table, _ = checkpointed(lambda: ops.pc_stats(x, N, C, HW, group=self.group, **need), self.group)
        batch_mean = self.batch_avg and not force_global_min_max
        if batch_mean:
            # mean over the batch of the per-sample extrema (smpc.py:72,78): rows = (n, c) pairs, fp64 sums divided per channel
            # on the device
            rows, _ = ops.pc_stats(x, 1, N * C, HW, local_only=True)
            smax, smin, cnt = batch_extrema_sums(rows, N, self.group)
            table = table.clone()
            table[L.STAT_MAX] = (smax / cnt).float()
            table[L.STAT_MIN] = (smin / cnt).float()
        if self.collect_err:
            # the three quantizations `-sm use -c mix` chooses between, from THIS batch's table; rows in ERR_NAMES' order.
            # The table's min / max rows are x's exact extrema unless batch_avg replaced them.
            qp_l, qp_g, qp_p = ops.mix_candidates(table, **settings)
            err = ops.pc_quant_errors(x, N, C, HW, (qp_p, qp_g, qp_l),
                                      mm=None if batch_mean else table[[L.STAT_MIN, L.STAT_MAX]])
            table = torch.cat([table, err])
        self._record(id, table)

    def _record(self, id, table):
        host = table.cpu().numpy()          # the only synchronisation of this call
        layer = self.stats.setdefault(id, {})
        for sn in self.stats_names:
            st = host[_ROW[sn] if sn in _ROW or not self.collect_err else L.NSTAT + ERR_NAMES.index(sn)].copy()
            if sn.startswith('cos'):
                st = np.nan_to_num(st)      # smpc.py:113-115
                st[st == 0] = 1.
            layer[sn] = st if sn not in layer else np.vstack([layer[sn], st])

    def _err_settings(self, tag, half_range, given):
        s = given if given is not None else self.err_settings
        if callable(s):
            s = s(tag, half_range)
        if s is None:
            raise ValueError('collect_err needs the settings of the activation quantizer whose candidates it measures: pass '
                             'err_settings (dict(num_bits=..., positive=..., bit_alloc=..., prior_is_b=..., target=..., '
                             'round_mode=...) or a callable (tag, half_range) -> dict) to the manager or to save_tensor_stats')
        return dict(s)

    def get_tensor_stat(self, id, stat, kind='mean'):
        if self.stats is not None:
            return self.stats[id]['%s_%s' % (kind, stat)]
        return None

    def _write(self):
        if os.path.exists(self.folder):
            shutil.rmtree(self.folder)
        os.makedirs(self.folder)
        if SAVE_FULL_STATS:
            with open(os.path.join(self.folder, 'statistics_perchannel.pkl'), 'wb') as f:
                pickle.dump(self.stats, f)
        self._save_summary()

    def _save_summary(self):
        """min / mean / max over the collected batches per channel (smpc.py:152-174)."""
        columns = summary_columns(self.stats_names)
        summary = {}
        for layer in self.stats:
            df = pd.DataFrame(columns=columns)
            for s in self.stats_names:
                if s in self.stats[layer]:
                    t = self.stats[layer][s]
                    many = len(t.shape) > 1
                    df['min_%s' % s] = t.min(axis=0) if many else [t.min(axis=0)]
                    df['mean_%s' % s] = t.mean(axis=0) if many else [t.mean(axis=0)]
                    df['max_%s' % s] = t.max(axis=0) if many else [t.max(axis=0)]
            summary[layer] = df
        with open(os.path.join(self.folder, '%s_statistics_perchannel_summary.pkl' % self.name), 'wb') as f:
            pickle.dump(summary, f)
