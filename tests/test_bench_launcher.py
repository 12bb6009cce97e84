"""CPU rehearsal of bench.py's multi-rank launch (`python bench.py --gpus N`): the parent spawns N children, rank 0
prints ONE JSON line with n_gpus = N, the barrier + max-over-ranks timing and the ragged index gather run over gloo.
No kernels run here (--dry-run); the GPU box runs the same plumbing over RCCL.  Also --dump-outputs: its size limit on
the CPU, and on the GPU that two runs with the same arguments write the same outputs."""
import json
import os
import subprocess
import sys

import pytest

from conftest import ROOT

BENCH = os.path.join(ROOT, 'bench.py')


def run(args, env=None, timeout=240):
    e = dict(os.environ)
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_PORT'):
        e.pop(k, None)
    e.update(env or {})
    return subprocess.run([sys.executable, BENCH] + args, capture_output=True, text=True, env=e, timeout=timeout)


def json_lines(stdout):
    return [json.loads(ln) for ln in stdout.splitlines() if ln.startswith('{')]


def test_gpus_2_spawns_two_ranks_and_prints_one_line():
    p = run(['--gpus', '2', '--steps', '4', '--warmup', '1', '--dry-run', '--rows', '5'])
    assert p.returncode == 0, p.stderr[-2000:]
    lines = json_lines(p.stdout)
    assert len(lines) == 1
    out = lines[0]
    assert out['n_gpus'] == 2 and out['steps'] == 4 and out['warmup'] == 1 and out['scaling'] == 'weak'
    assert out['extras']['index_gather_ms'] is not None          # the ragged gather ran across both ranks
    assert out['config']['rows_per_gpu'] == 5
    assert abs(out['value'] - 2 * 5 * 4 / (out['ms_per_step'] * 4e-3)) / out['value'] < 1e-3   # whole-job aggregate


def test_single_rank_needs_no_process_group():
    p = run(['--steps', '2', '--warmup', '0', '--dry-run'])
    assert p.returncode == 0, p.stderr[-2000:]
    out = json_lines(p.stdout)[0]
    assert out['n_gpus'] == 1 and out['extras']['index_gather_ms'] is None


def test_gpus_flag_must_agree_with_world_size():
    """Launched by torch.distributed.run the ranks come from the environment; a mismatch fails loudly instead of
    reporting a wrong n_gpus."""
    p = run(['--gpus', '2', '--steps', '1', '--dry-run'], env={'RANK': '0', 'LOCAL_RANK': '0', 'WORLD_SIZE': '1'})
    assert p.returncode != 0
    assert 'WORLD_SIZE=1' in (p.stderr + p.stdout)


def test_failed_rank_gives_nonzero_exit():
    p = run(['--gpus', '2', '--steps', '1', '--dry-run', '--config', 'bogus'])
    assert p.returncode != 0


def test_one_dead_rank_ends_the_run_quickly(tmp_path):
    """Rank 1 dies before the rendezvous (STOF_TEST_FAIL_RANK): rank 0 would wait in init_process_group until the
    process-group timeout; the launcher polls every child, ends the survivors and reports the dead rank."""
    import time
    t0 = time.monotonic()
    p = run(['--gpus', '2', '--steps', '1', '--dry-run'], env={'STOF_TEST_FAIL_RANK': '1', 'STOF_BENCH_LOGDIR': str(tmp_path)},
            timeout=120)
    took = time.monotonic() - t0
    assert p.returncode != 0
    assert took < 30, f'launcher took {took:.1f} s to notice a dead rank'
    assert '(1, 3)' in p.stderr and 'STOF_TEST_FAIL_RANK' in p.stderr         # which rank, which code, its stderr tail
    assert json_lines(p.stdout) == []


def test_watchdog_ends_a_hung_run(tmp_path):
    p = run(['--gpus', '2', '--steps', '1', '--dry-run'], env={'STOF_TEST_HANG_RANK': '1', 'STOF_BENCH_TIMEOUT': '8',
                                                                'STOF_BENCH_LOGDIR': str(tmp_path)}, timeout=120)
    assert p.returncode != 0 and 'watchdog' in p.stderr


def test_line_proves_the_ranks_that_took_part(tmp_path):
    p = run(['--gpus', '2', '--steps', '2', '--warmup', '0', '--dry-run'], env={'STOF_BENCH_LOGDIR': str(tmp_path)})
    assert p.returncode == 0, p.stderr[-2000:]
    ranks = json_lines(p.stdout)[0]['ranks']
    assert ranks['ranks_seen'] == 2 and [r['rank'] for r in ranks['devices']] == [0, 1]
    assert ranks['physical_gpus'] == 0 and 'gloo' in ranks['collective_backend']      # a CPU dry run says so in the record


def test_steps_must_be_positive():
    p = run(['--steps', '0', '--dry-run'])
    assert p.returncode != 0 and '--steps' in p.stderr


def test_dump_outputs_keeps_to_the_size_limit_with_a_fixed_sample(tmp_path):
    """--dump-outputs: arrays over the limit are cut to the same seeded rows; dtypes are float32 / float64 only."""
    import numpy as np
    import torch
    import bench
    g = torch.Generator().manual_seed(0)
    arrays = {'maps': torch.randn(1000, 1, 50, generator=g), 'counts': torch.randint(0, 9, (1000,), generator=g, dtype=torch.int32),
              'loss': torch.tensor(0.25, dtype=torch.float64)}
    limit = 60_000
    for d in ('a', 'b'):
        bench.dump_outputs(str(tmp_path / d), arrays, limit=limit)
    files = sorted(os.listdir(tmp_path / 'a'))
    assert files == ['counts.npy', 'counts_rows.npy', 'loss.npy', 'maps.npy', 'maps_rows.npy']
    assert sum(os.path.getsize(tmp_path / 'a' / f) for f in files) <= limit
    for f in files:
        a, b = np.load(tmp_path / 'a' / f), np.load(tmp_path / 'b' / f)
        assert a.dtype in (np.float32, np.float64) and np.array_equal(a, b)
    rows = np.load(tmp_path / 'a' / 'maps_rows.npy').astype(np.int64)
    assert np.array_equal(rows, np.load(tmp_path / 'a' / 'counts_rows.npy')) and np.all(np.diff(rows) > 0)
    assert np.array_equal(np.load(tmp_path / 'a' / 'maps.npy'), arrays['maps'].numpy()[rows])
    assert np.array_equal(np.load(tmp_path / 'a' / 'counts.npy'), arrays['counts'].numpy()[rows].astype(np.float64))
    assert float(np.load(tmp_path / 'a' / 'loss.npy')) == 0.25
    bench.dump_outputs(str(tmp_path / 'c'), arrays)                  # under the default limit: everything, no row files
    assert sorted(os.listdir(tmp_path / 'c')) == ['counts.npy', 'loss.npy', 'maps.npy']
    assert np.array_equal(np.load(tmp_path / 'c' / 'maps.npy'), arrays['maps'].numpy())


@pytest.mark.gpu
@pytest.mark.parametrize('config,rows', [('C2', '64'), ('C4', '1024'), ('C5', '8')])
def test_dump_outputs_of_two_runs_are_identical(tmp_path, config, rows):
    """Same arguments, same inputs: two runs of the timed path write the same outputs, and --steps is the timed step count."""
    import numpy as np
    recs = []
    for d in ('a', 'b'):
        p = run(['--config', config, '--rows', rows, '--steps', '3', '--warmup', '1', '--no-cpu-baseline', '--no-fp32-extra',
                 '--dump-outputs', str(tmp_path / d)], env={'STOF_BENCH_LOGDIR': str(tmp_path)}, timeout=400)
        assert p.returncode == 0, p.stderr[-2000:]
        recs.append(json_lines(p.stdout)[-1])
    assert all(r['steps'] == 3 and r['ms_per_step'] > 0 for r in recs)
    files = sorted(os.listdir(tmp_path / 'a'))
    assert files == sorted(os.listdir(tmp_path / 'b'))
    assert files == (['loss.npy', 'pred.npy', 'weights.npy'] if config == 'C5' else
                     ['maps.npy', 'onset_counts.npy', 'onset_indices.npy'] if config == 'C4' else ['maps.npy'])
    for f in files:
        a, b = np.load(tmp_path / 'a' / f), np.load(tmp_path / 'b' / f)
        assert a.dtype in (np.float32, np.float64) and a.size > 0, f
        if f == 'loss.npy':        # float64 partial sums of the blocks are added atomically, in the order the blocks finish
            assert np.allclose(a, b, rtol=1e-12, atol=0), (a, b)
        else:
            assert np.array_equal(a, b), f


@pytest.mark.gpu
def test_plain_run_prints_the_headline_and_full_adds_the_rest(tmp_path):
    """A plain run times its steps and prints the line; --full adds, after the same timed steps, the CPU baseline with its
    parity check, the pickers, the fused onsets and the exact-fp32 mode."""
    recs = {}
    for mode in ('plain', 'full'):
        p = run(['--rows', '64', '--steps', '2', '--warmup', '1', '--cpu-sample-rows', '8'] + (['--full'] if mode == 'full' else []),
                env={'STOF_BENCH_LOGDIR': str(tmp_path)}, timeout=400)
        assert p.returncode == 0, p.stderr[-2000:]
        recs[mode] = json_lines(p.stdout)[-1]
    plain, full = recs['plain'], recs['full']
    for k in ('metric', 'unit', 'higher_is_better', 'dtype', 'steps', 'warmup', 'config'):
        assert plain[k] == full[k], k
    assert plain['value'] > 0 and plain['ms_per_step'] > 0 and plain['kernels_ms']['body_sweep'] > 0
    assert 'cpu_baseline' not in plain and set(plain['extras']) == {'auto_mode_fp32_rerun_taken'}
    assert full['cpu_baseline']['parity_on_sample']['rows'] == 8
    assert {'picker_argmax_ms', 'fused_argmax_onsets', 'fp32_exact_mode', 'index_gather_ms'} <= set(full['extras'])


def test_under_torch_distributed_run_like_the_driver(tmp_path):
    """The driver's N > 1 launch line: torch.distributed.run provides RANK / WORLD_SIZE / MASTER_*."""
    import socket
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    e = dict(os.environ, STOF_BENCH_LOGDIR=str(tmp_path))
    for k in ('RANK', 'LOCAL_RANK', 'WORLD_SIZE', 'MASTER_PORT'):
        e.pop(k, None)
    p = subprocess.run([sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', '--nproc-per-node', '2', '--master-addr',
                        '127.0.0.1', '--master-port', str(port), BENCH, '--gpus', '2', '--steps', '2', '--warmup', '1',
                        '--dry-run'], capture_output=True, text=True, env=e, timeout=240)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = json_lines(p.stdout)
    assert len(lines) == 1 and lines[0]['n_gpus'] == 2 and lines[0]['ranks']['ranks_seen'] == 2
