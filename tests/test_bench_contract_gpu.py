"""The driver's bench.py contract on a small batch: exactly ONE JSON line on stdout with the agreed keys; a plain run with
the headline alone and the outputs of its last step (--dump-outputs); with --full the roofline and cpu_baseline objects,
internally consistent numbers, every other_configs entry verified - and `--gpus 2` started as
a PLAIN process (the form of the driver's N = 1 command) starts its own two ranks (VERDICT r2 missing #4; here both
ranks share the one GPU over gloo).  Needs an MI355X: `pytest -m gpu`."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((64, 112, 1), (256, 56, 4), (128, 56, 1), (512, 28, 5), (64, 56, 6), (256, 28, 1), (1024, 14, 7), (128, 28, 7),
          (512, 14, 1), (2048, 7, 4), (256, 14, 11), (512, 7, 5))


def run_bench(*extra, env=None):
    e = dict(os.environ)
    e.pop('WORLD_SIZE', None), e.pop('RANK', None), e.pop('LOCAL_RANK', None)
    e.update(env or {})
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + list(extra), capture_output=True, text=True,
                       timeout=900, cwd=ROOT, env=e)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def test_json_line_contract():
    d = run_bench('--gpus', '1', '--steps', '2', '--warmup', '1', '--batch', '8', '--full')
    for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling',
              'vs_baseline', 'dtype', 'data', 'config', 'roofline', 'cpu_baseline', 'verified', 'group_status',
              'other_configs', 'ms_per_step_by_rank', 'rccl_ranks', 'box', 'sustained'):
        assert k in d, k
    assert d['n_gpus'] == 1 and d['steps'] == 2 and d['warmup'] == 1
    assert d['higher_is_better'] is True and d['vs_baseline'] is None and d['verified'] is True
    assert d['group_status'] == 0 and d['rccl_ranks'] == 0
    sus = d['sustained']
    assert sus['steps'] >= 2 and sus['seconds'] > 0 and abs(sus['ms_per_step'] - sus['seconds'] * 1e3 / sus['steps']) < 1e-9
    assert abs(sus['value'] * sus['ms_per_step'] * 1e-3 - sum(c * hw * hw * n for (c, hw, n) in SHAPES) * 8) < 1.
    assert d['unit'] == 'elements/s' and d['dtype'] == 'f32' and d['data'] == 'synthetic'
    assert 'workload' in d['config'] and 'model' not in d['config']
    elems = sum(c * hw * hw * n for (c, hw, n) in SHAPES) * 8
    assert abs(d['value'] * d['ms_per_step'] * 1e-3 - elems) / elems < 1e-6       # value = elements / step time
    r = d['roofline']
    assert r['bound'] == 'hbm' and r['unit'] == 'GB/s' and r['peak'] == 8000.0
    assert abs(r['frac'] - r['achieved'] / r['peak']) < 1e-9 and 0 < r['frac'] < 1
    assert abs(r['achieved'] - r['bytes_per_launch'] / (r['avg_launch_ms'] * 1e-3) / 1e9) / r['achieved'] < 1e-6
    c = d['cpu_baseline']
    assert c['kind'] == 'port' and c['unit'] == 'elements/s' and c['cores'] >= 1 and c['value'] > 0 and c['sample']
    oc = d['other_configs']
    for k in ('config1', 'config2_entropy', 'config2_packed_single_launch', 'config3', 'config3_packed_storage',
              'config3_packed_load', 'config4', 'config5'):
        assert oc[k]['verified'] is True, k
        ro = oc[k]['roofline']
        assert ro['bound'] == 'hbm' and oc[k]['value'] > 0
        # round 6: `frac` is ACHIEVED bandwidth - the bytes the launches move - and never above the peak; the
        # SURVEY accounting of earlier rounds sits beside it under its own name
        assert 0 < ro['frac'] <= 1 and abs(ro['frac'] - ro['achieved'] / ro['peak']) < 1e-12, k
        assert abs(ro['achieved'] - oc[k]['value'] * ro['bytes_moved_per_element'] / 1e9) / ro['achieved'] < 1e-9, k
        assert ro['bytes_moved_per_element'] <= ro['survey_bytes_per_element'] and ro['frac'] <= ro['frac_survey_accounting'] + 1e-12, k
    assert oc['config3']['roofline']['bytes_moved_per_element'] == 12 and oc['config5']['roofline']['bytes_moved_per_element'] == 12
    assert 0 < d['path_frac_hbm_peak'] <= 1 and d['path_bytes_moved_per_element'] == 8
    assert abs(d['path_frac_hbm_peak'] - d['value'] * 8 / 1e9 / 8000.) < 1e-9 and d['path_equiv_12B'] > d['path_frac_hbm_peak']


def test_plain_line_and_dumped_outputs(tmp_path):
    """A plain run (no --full) times exactly --steps steps and prints the headline without what --full adds; --dump-outputs
    writes the outputs of the last timed step: float32, inside 64 MB, the same in two runs, and the same values the product
    entry point gives for the workload's inputs in this process."""
    import numpy as np
    import torch
    import bench
    from cnn_quantization_amd import ops
    elems = sum(c * hw * hw * n for (c, hw, n) in SHAPES) * 8
    dirs = {3: tmp_path / 'run3', 2: tmp_path / 'run2'}
    for k, out in dirs.items():
        d = run_bench('--gpus', '1', '--steps', str(k), '--warmup', '1', '--batch', '8', '--dump-outputs', str(out))
        assert d['steps'] == k and d['warmup'] == 1 and d['full'] is False and d['n_gpus'] == 1
        assert d['unit'] == 'elements/s' and d['dtype'] == 'f32' and d['higher_is_better'] is True and d['metric']
        assert d['ms_per_step'] > 0 and abs(d['value'] * d['ms_per_step'] * 1e-3 - elems) / elems < 1e-6
        assert d['group_status'] == 0
        for key in ('verified', 'sustained', 'roofline', 'roofline_other_kernels', 'other_configs', 'cpu_baseline'):
            assert key not in d, key
    layers = bench.build_workload(8, torch.device('cuda'))
    names = ['y_%02d.npy' % i for i in range(len(layers))]
    assert sorted(os.listdir(dirs[3])) == names and sorted(os.listdir(dirs[2])) == names
    for L in layers:
        ops.act_qdq_per_channel(L['x'], 4, positive=L['half'], out=L['y'])
    bench.dump_outputs(layers, str(tmp_path / 'here'))
    total = 0
    for i, n in enumerate(names):
        a, b, c = (np.load(str(p / n)) for p in (dirs[3], dirs[2], tmp_path / 'here'))
        assert a.dtype == np.float32 and a.ndim == 1 and a.size == min(layers[i]['y'].numel(), bench.DUMP_SAMPLE), n
        assert a.tobytes() == b.tobytes() and a.tobytes() == c.tobytes(), n
        total += a.nbytes
    assert total <= 64 << 20


def test_shard_legs_of_configs_3_4_5():
    """Round 6: `bench.py --batch 64 --force-exchange` (and --gpus N) carries BASELINE configs 3 / 4 / 5 at the shard in
    other_configs, with the bytes they move; with the in-launch exchange in force (CNNQ_XRANK=1 on the forced 1-rank group) they
    run the sharded single-launch kernels, with the collective the chain."""
    d = run_bench('--gpus', '1', '--batch', '16', '--steps', '2', '--warmup', '1', '--force-exchange', '--no-cpu-baseline', '--full',
                  env={'CNNQ_XRANK': '1'})
    oc = d['other_configs']
    assert d['verified'] is True and 'in-launch exchange' in d['config']['exchange']
    for k, moved in (('config3', 12), ('config5', 12)):
        assert oc[k]['verified'] is True and oc[k]['roofline']['bytes_moved_per_element'] == moved and 'in-launch' in oc[k]['exchange'], k
    assert oc['config4']['verified'] is True and 4 <= oc['config4']['roofline']['bytes_moved_per_element'] <= 8
    assert d['path_bytes_moved_per_element'] == 8
    d = run_bench('--gpus', '1', '--batch', '16', '--steps', '2', '--warmup', '1', '--force-exchange', '--no-cpu-baseline', '--full',
                  env={'CNNQ_XRANK': '0'})
    oc = d['other_configs']
    for k, moved in (('config3', 16), ('config4', 8), ('config5', 16)):
        assert oc[k]['verified'] is True and oc[k]['roofline']['bytes_moved_per_element'] == moved and 'all_gather' in oc[k]['exchange'], k
    assert d['path_bytes_moved_per_element'] == 12
    # two ranks sharing the GPU over gloo (the collective route): every rank takes part in the legs, rank 0 prints them
    d = run_bench('--gpus', '2', '--batch', '16', '--steps', '2', '--warmup', '1', '--no-cpu-baseline', '--full',
                  env={'CNNQ_BENCH_BACKEND': 'gloo'})
    oc = d['other_configs']
    assert all(oc[k]['verified'] is True for k in ('config3', 'config4', 'config5'))


def test_plain_process_starts_its_own_ranks():
    d = run_bench('--gpus', '2', '--batch', '64', '--steps', '3', '--warmup', '1', '--no-cpu-baseline', '--no-other-configs', '--full',
                  env={'CNNQ_BENCH_BACKEND': 'gloo'})
    assert d['n_gpus'] == 2 and d['scaling'] == 'strong' and d['verified'] is True
    assert d['config']['per_gpu_batch'] == 32 and d['config']['global_batch'] == 64
    assert len(d['ms_per_step_by_rank']) == 2 and all(t > 0 for t in d['ms_per_step_by_rank'])
    assert abs(max(d['ms_per_step_by_rank']) - d['ms_per_step']) / d['ms_per_step'] < 0.5
    elems = sum(c * hw * hw * n for (c, hw, n) in SHAPES) * 64
    assert abs(d['value'] * d['ms_per_step'] * 1e-3 - elems) / elems < 1e-6       # whole-job elements over the max time


def test_eight_ranks_on_one_gpu():
    """The driver's N = 8 form (one batch of 64 sharded eight ways), all ranks on the one GPU over gloo: exit 0, one line,
    eight per-rank times, the job's elements over the slowest rank's time, outputs verified on every rank."""
    d = run_bench('--gpus', '8', '--batch', '64', '--steps', '2', '--warmup', '1', '--no-cpu-baseline', '--no-other-configs', '--full',
                  env={'CNNQ_BENCH_BACKEND': 'gloo'})
    assert d['n_gpus'] == 8 and d['scaling'] == 'strong' and d['verified'] is True
    assert d['config']['per_gpu_batch'] == 8 and d['config']['global_batch'] == 64
    assert len(d['ms_per_step_by_rank']) == 8 and all(t > 0 for t in d['ms_per_step_by_rank'])
    elems = sum(c * hw * hw * n for (c, hw, n) in SHAPES) * 64
    assert abs(d['value'] * d['ms_per_step'] * 1e-3 - elems) / elems < 1e-6
    assert d['box'].startswith('gpu-')


def test_in_launch_exchange_falls_back_to_the_collective():
    """CNNQ_XRANK=1 with two ranks on the one GPU: the job starts through the in-launch exchange.  Two processes on one GPU
    cannot count on their launches running together at these sizes, so a wait for the peer may really expire - and with the
    test hook one is reported for sure: every rank then drops to the collective together, the job is timed again and the line
    is verified.  The default (auto) never starts the in-launch exchange between ranks that share a GPU."""
    env = {'CNNQ_BENCH_BACKEND': 'gloo', 'CNNQ_XRANK': '1', 'CNNQ_XRANK_TIMEOUT_MS': '1000'}
    d = run_bench('--gpus', '2', '--batch', '16', '--steps', '3', '--warmup', '1', '--no-cpu-baseline', '--full', env=env)
    assert all(d['other_configs'][k]['verified'] is True for k in ('config3', 'config4', 'config5'))     # whichever exchange they ended on
    assert d['verified'] is True and d['xrank'] is not None and d['xrank']['used'] == (not d['xrank']['fell_back'])
    assert ('in-launch exchange' in d['config']['exchange']) == d['xrank']['used']
    d = run_bench('--gpus', '2', '--batch', '16', '--steps', '3', '--warmup', '1', '--no-cpu-baseline', '--full',
                  env=dict(env, CNNQ_XRANK_TEST_FAIL_AT='70'))
    assert d['verified'] is True and d['xrank'] == {'used': False, 'healthy': False, 'fell_back': True}
    assert 'in-launch exchange' not in d['config']['exchange']      # the records move by all_gather (or, with CNNQ_XRANK=1, by peer stores)
    d = run_bench('--gpus', '2', '--batch', '16', '--steps', '2', '--warmup', '1', '--no-cpu-baseline', '--full',
                  env={'CNNQ_BENCH_BACKEND': 'gloo'})
    assert d['verified'] is True and d['xrank'] is None and 'all_gather' in d['config']['exchange']
    # auto, with the one-GPU rig declared eligible: both exchanges are probed (untimed), the timed steps take the faster one
    # that stayed healthy - whichever that is here, the line is verified and says what was measured
    d = run_bench('--gpus', '2', '--batch', '16', '--steps', '2', '--warmup', '1', '--no-cpu-baseline', '--full',
                  env={'CNNQ_BENCH_BACKEND': 'gloo', 'CNNQ_XRANK_SHARED_OK': '1', 'CNNQ_XRANK_TIMEOUT_MS': '1000'})
    assert d['verified'] is True and d['xrank'] is not None
    assert d['xrank']['probe_ms_collective'] > 0 and d['xrank']['probe_ms_in_launch'] > 0
    assert ('in-launch exchange' in d['config']['exchange']) == d['xrank']['used']



@pytest.mark.parametrize('xrank', ['0', '1'])
def test_graph_replay_of_the_sharded_step(xrank):
    """--graph with the exchange in the captured step: the multi-GPU launch sequence of a 64-sample shard on a
    1-rank RCCL group, through the collective route (ncclAllGather captured on the compute stream) and through the in-launch
    exchange (device-side sequence word), replayed from a HIP graph; outputs verified after the replays."""
    d = run_bench('--batch', '64', '--steps', '4', '--warmup', '2', '--no-cpu-baseline', '--no-other-configs', '--force-exchange',
                  '--graph', '--full', '--sustained-secs', '0.2', env={'CNNQ_XRANK': xrank})
    assert d['verified'] is True and d['group_status'] == 0
    assert d['config']['launch'] == 'hip graph replay'
    assert ('in-launch exchange' in d['config']['exchange']) == (xrank == '1')
    assert d['sustained']['steps'] >= 4
