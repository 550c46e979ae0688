"""Per-tensor calibration statistics (CSV), mirror of
pytorch_quantizer/quantization/inference/statistic_manager.py: same API and file layout
(`~/mxt-sim/statistics/<name>/<name>_summary.csv`, columns {min,mean,max}_<stat> indexed by layer
id).  Serves the per-tensor quantizers (pooling, classifier, linear) in `-sm use` mode.

The scalar statistics of a batch are one pass of the device kernels over the tensor viewed as a
single channel; a bf16 / fp16 tensor and a dense channels_last one are read where they lie, in their
own dtype (collect_route answers 'flat': ops.tensor_stats).  `kld_threshold=True` adds the `kld_th` column (statistic_manager.py:80-82: the
maximum over the batch's samples of the KLD-optimal clipping threshold) from the device
histogram + search kernels (ops.kld_thresholds; with `native_kld=True` a bf16 / fp16 tensor that collect_route takes stays where it
lies there too: ops.kld_thresholds_half, the same bits).  The error columns (mse_*/cos_*,
statistic_manager.py:22-30) exist in the reference's files but no caller ever passes the quantized
tensors they need (`tensors_q`), so they always hold NaN there; `collect_err=True` reproduces
those columns, a non-empty `tensors_q` is rejected.  What this manager and the per-channel one share is defined here, once."""
import os
import shutil
from pathlib import Path

import numpy as np
import pandas as pd
import torch

from .. import _lib as L
from .. import distributed as D
from .. import ops
from ..utils.misc import Singleton, sorted_nicely


def base_dir():
    return os.path.join(str(Path.home()), 'mxt-sim')


def collect_route(manager, tensor, force_global_min_max=False):
    """How save_tensor_stats takes this tensor: 'flat' - on its storage as it lies (ops.tensor_stats: no
    layout copy, no upcast): a CUDA tensor of fp32 / bf16 / fp16 that is contiguous and not float32, or dense channels_last with
    the channels_last switch on; one process and no forced exchange; and not a half tensor when the KLD threshold is collected,
    unless the manager opted in with `native_kld` (ops.kld_thresholds_half: DESIGN.md section 32) and the route word
    ops._kld_half_native, asked last, keeps the class native - or None: a contiguous float32 tensor and every sharded run take the
    code they took.
    Shape, strides, dtype and attributes only: nothing touches the device.  No class of tensor measured slower native than
    through the copy (profiles/tensor_collect.md), so no route function is asked but the KLD one (profiles/half_kld.md)."""
    if not (isinstance(tensor, torch.Tensor) and tensor.is_cuda and tensor.dtype in ops._ACT_DTYPES and tensor.numel() > 0):
        return None
    half = tensor.dtype != torch.float32
    layout = ops._layout(tensor)
    if not ((layout == 'nchw' and half) or (layout == 'nhwc' and ops._NHWC)):
        return None
    if D.world_size(manager.group) != 1 or D.forced_exchange():
        return None
    if manager.kld_threshold and half:
        if not getattr(manager, 'native_kld', False):
            return None
        rows = tensor.shape[0] if tensor.dim() > 1 else 1       # save_tensor_stats' rows
        return 'flat' if ops._kld_half_native(rows, tensor.numel() // rows, tensor.dtype) else None
    return 'flat'


def collects_native_flat(manager, tensor):
    """Whether collect_route answers 'flat'."""
    return collect_route(manager, tensor) == 'flat'


# ---- what the per-tensor and the per-channel manager share
def checkpointed(launch, group):
    """launch()'s result; in a sharded run, after a wait of the in-launch exchange expired on some rank (the table is NaN there and
    the group is on the collective now): launch()'s result again, before anything of it is recorded."""
    out = launch()
    if D.world_size(group) > 1 and not D.xrank_checkpoint(group):
        out = launch()
    return out


def batch_extrema_sums(rows, N, group):
    """For the mean over the batch of the per-sample extrema, from the per-sample table `rows` ([.., N * C], sample-major): a
    float64 device record [3, C] - the samples' maxima summed, their minima summed, the sample count.  With several ranks the sums
    and counts travel: every rank holds those of the GLOBAL batch.  The caller divides (per channel on the device, per tensor on
    the host)."""
    smax = rows[L.STAT_MAX].view(N, -1).double().sum(dim=0)
    smin = rows[L.STAT_MIN].view(N, -1).double().sum(dim=0)
    rec = torch.stack([smax, smin, torch.full_like(smax, float(N))])
    if D.world_size(group) > 1:
        rec = D.all_gather_records(rec, group).sum(dim=0)
    return rec


def summary_columns(names):
    return ['%s_%s' % (kind, c) for c in names for kind in ('min', 'mean', 'max')]


class Collector:
    """The way out of both managers: every rank holds the same (global) statistics, so rank 0 writes, the others wait for the files."""

    def __exit__(self, *args):
        if not self.save_stats:
            return
        world = D.world_size(self.group)
        if world == 1 or D.rank(self.group) == 0:
            self._write()
        if world > 1:
            torch.distributed.barrier(group=self.group)


class StatisticManager(Collector, metaclass=Singleton):
    collect_route = collect_route       # the face inference_quantization_manager._route asks

    def __init__(self, folder, load_stats, stats=('max', 'min', 'std', 'mean', 'kurtosis', 'mean_abs', 'b', 'dim'),
                 batch_avg=False, kld_threshold=False, collect_err=False, group=None, native_kld=False):
        self.name = folder
        self.group = group          # process group of a batch-sharded run (None: the default group, if any)
        self.folder = os.path.join(base_dir(), 'statistics', folder)
        self.stats_names = list(stats)
        self.collect_err = collect_err
        if collect_err:
            self.stats_names += ['mse_lowp', 'mse_gaus', 'mse_laplace', 'cos_lowp', 'cos_gaus', 'cos_laplace']
        self.kld_threshold = kld_threshold
        self.native_kld = native_kld    # opt-in: the histogram of a bf16 / fp16 tensor on its storage (collect_route)
        if kld_threshold:
            self.stats_names.append('kld_th')
        self.batch_avg = batch_avg
        self.stats = {}
        self.metadata = {}
        self.save_stats = not load_stats
        if load_stats:
            stats_file = os.path.join(self.folder, '%s_summary.csv' % self.name)
            assert os.path.exists(stats_file), stats_file
            self.stats_df = pd.read_csv(stats_file, index_col=0)
        else:
            self.stats_df = None

    def save_tensor_stats(self, tensor, tag, id, tensors_q={}, force_global_min_max=False, *, route=None):
        """route: collect_route's answer, from a caller that has asked already (None: ask here)."""
        if len(tensors_q) > 0:
            raise NotImplementedError('error columns from quantized tensors: no caller in the reference')
        native = (route or collect_route(self, tensor)) == 'flat'
        x = tensor.detach() if native else tensor.detach().contiguous()
        n = x.numel()
        # with several ranks x is this rank's batch shard: the moment records travel (ops.pc_stats), every rank
        # holds the statistics of the GLOBAL batch
        world = D.world_size(self.group)
        if native:
            # bf16 / fp16 and dense channels_last tensors, one process: the flat-row kernels on the storage as it lies
            table, mom = ops.tensor_stats(x, 1)
        else:
            table, mom = checkpointed(lambda: ops.pc_stats(x, 1, 1, n, need_b=True, need_kurt=True, need_relu=True,
                                                           group=self.group), self.group)
        host = table.cpu().numpy()[:, 0]
        m = mom.cpu().numpy()[:, 0]
        total = m[L.MOM_COUNT]      # elements of the global batch (== n on one rank)
        vals = {'max': host[L.STAT_MAX], 'min': host[L.STAT_MIN], 'std': host[L.STAT_STD],
                'mean': host[L.STAT_MEAN], 'kurtosis': host[L.STAT_KURT], 'b': host[L.STAT_B],
                'mean_abs': np.float32((2. * m[L.MOM_SUM_RELU] - m[L.MOM_SUM]) / total), 'dim': int(total)}
        if self.batch_avg and not force_global_min_max and x.dim() > 1:
            if native:      # the exact per-sample extrema, rows MIN / MAX: native in the three dtypes and both layouts
                rows = ops.tensor_row_stats(x, x.shape[0])
            else:
                rows, _ = ops.pc_stats(x, 1, x.shape[0], n // x.shape[0], local_only=True)
            r = batch_extrema_sums(rows, x.shape[0], self.group).cpu().numpy()[:, 0]
            vals['max'] = np.float32(r[0] / r[2])
            vals['min'] = np.float32(r[1] / r[2])
        for s in self.stats_names:
            if s.startswith('mse_') or s.startswith('cos_'):
                vals[s] = np.nan
        if self.kld_threshold:
            # a half tensor arrives here natively only through native_kld (collect_route); its threshold is the upcast copy's
            kld = ops.kld_thresholds_half if native and x.dtype != torch.float32 else ops.kld_thresholds
            th = kld(x, x.shape[0] if x.dim() > 1 else 1)[:, 0].max().view(1, 1)
            if world > 1:           # the maximum over the samples of every rank
                th = D.all_gather_records(th, self.group).max().view(1, 1)
            vals['kld_th'] = float(th.item())
        row = np.array([[vals[s] for s in self.stats_names]], dtype=np.float64)
        if id in self.stats:
            self.stats[id] = np.concatenate([self.stats[id], row])
        else:
            self.stats[id] = row
            self.metadata[id] = tag

    def get_tensor_stat(self, id, stat, kind='mean'):
        if self.stats_df is not None:
            return self.stats_df.loc[id, '%s_%s' % (kind, stat)]
        return None

    def get_tensor_stats(self, id, kind=None):
        kind = kind or {}
        if self.stats_df is None:
            return (None,) * 6
        return tuple(self.stats_df.loc[id, '%s_%s' % (kind.get(s, 'mean'), s)]
                     for s in ('min', 'max', 'mean', 'std', 'mean_abs', 'b'))

    def _write(self):
        if os.path.exists(self.folder):
            shutil.rmtree(self.folder)
        os.makedirs(self.folder)
        frames = {}
        for s_id in self.stats:
            df = pd.DataFrame(columns=self.stats_names, data=self.stats[s_id])
            df.to_csv(os.path.join(self.folder, '%s.csv' % s_id), index=False)
            frames[s_id] = df
        summary = pd.DataFrame(columns=['internal_name'] + summary_columns(self.stats_names))
        for s_id in sorted_nicely(frames.keys()):
            summary.loc[s_id, 'internal_name'] = self.metadata[s_id]
            for c in self.stats_names:
                summary.loc[s_id, 'min_%s' % c] = frames[s_id][c].min()
                summary.loc[s_id, 'mean_%s' % c] = frames[s_id][c].mean()
                summary.loc[s_id, 'max_%s' % c] = frames[s_id][c].max()
            summary.loc[s_id, 'dim'] = frames[s_id]['dim'][0]
        summary.to_csv(os.path.join(self.folder, '%s_summary.csv' % self.name), index=True)
