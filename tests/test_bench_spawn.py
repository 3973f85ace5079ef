"""bench.py --gpus N really means N ranks: the spawn command carries N, a node
with fewer devices fails loudly instead of reporting a 1-GPU number, and a WORLD_SIZE that disagrees
with --gpus is an error."""
import os
import subprocess
import sys
import types

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_spawn_command_builds_n_workers():
    import bench
    args = types.SimpleNamespace(gpus=8)
    cmd = bench.spawn_command(args, ['--gpus', '8', '--steps', '20', '--warmup', '5'])
    assert cmd[1:3] == ['-m', 'torch.distributed.run']
    assert cmd[cmd.index('--nproc-per-node') + 1] == '8'
    assert cmd[cmd.index('--master-addr') + 1] == '127.0.0.1'
    assert cmd[-6:] == ['--gpus', '8', '--steps', '20', '--warmup', '5']
    assert os.path.basename(cmd[cmd.index('--master-port') + 2]) == 'bench.py'


def _run(extra_env, *argv):
    env = dict(os.environ)
    for k in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK'):
        env.pop(k, None)
    env.update(extra_env)
    return subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + list(argv), env=env,
                          capture_output=True, text=True, timeout=300)


def test_more_gpus_than_devices_fails_loudly():
    import torch
    n = torch.cuda.device_count()
    p = _run({}, '--gpus', str(n + 2))
    assert p.returncode != 0
    assert 'needs %d devices' % (n + 2) in p.stderr


def test_world_size_must_agree_with_gpus():
    p = _run({'WORLD_SIZE': '4', 'RANK': '0', 'LOCAL_RANK': '0'}, '--gpus', '2')
    assert p.returncode != 0
    assert 'WORLD_SIZE=4' in p.stderr


def test_stdout_carries_only_the_result_line():
    """The driver parses ONE JSON line from stdout; RCCL prints its version banner to stdout when a
    communicator is created (under torch.distributed.run).  bench.own_stdout() points file descriptor 1 at
    stderr and keeps the original for emit_line()."""
    import subprocess
    code = ("import os, sys; sys.path.insert(0, %r); import bench; bench.own_stdout(); "
            "print('library noise'); os.write(1, b'raw noise on fd 1\\n'); bench.emit_line('{\"value\": 1}')"
            % os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    r = subprocess.run([sys.executable, '-c', code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout == '{"value": 1}\n'
    assert 'library noise' in r.stderr and 'raw noise on fd 1' in r.stderr


def test_full_is_opt_in():
    """`--full` (every measurement and check beside the headline) is off unless asked for; `--plain` names the
    default and cannot be combined with it."""
    import bench
    assert not bench.parse(['--gpus', '1', '--steps', '20', '--warmup', '5']).full
    assert bench.parse(['--gpus', '1', '--steps', '20', '--warmup', '5', '--full']).full
    with pytest.raises(SystemExit):
        bench.parse(['--full', '--plain'])


# what only a --full run reports
FULL_ONLY = ('parity_check', 'single_batch', 'config3', 'eos_retire', 'bf16x3', 'roofline', 'roofline_attention',
             'kernels', 'gpu_us_per_step', 'config4', 'config5', 'cpu_baseline')


@pytest.mark.gpu
def test_plain_run_reports_the_headline_alone(tmp_path):
    """A run without --full: the headline figures of exactly --steps timed passes and the --dump-outputs
    arrays, nothing of what --full adds."""
    import json
    import numpy as np
    p = _run({}, '--gpus', '1', '--steps', '4', '--warmup', '2', '--dump-outputs', str(tmp_path))
    assert p.returncode == 0, p.stderr[-4000:]
    lines = p.stdout.splitlines()
    assert len(lines) == 1, p.stdout
    line = json.loads(lines[0])
    assert line['unit'] == 'questions/sec' and line['higher_is_better'] is True and line['dtype'] == 'f32'
    assert line['steps'] == 4 and line['warmup'] == 2 and line['n_gpus'] == 1
    assert line['value'] > 0 and line['ms_per_step'] > 0
    assert line['metric'].startswith('questions/sec (forward) on CLEVR')
    for k in FULL_ONLY:
        assert k not in line, k
    rows = line['config']['rows_per_launch']
    sc = np.load(str(tmp_path / 'scores.npy'))
    assert sc.dtype == np.float32 and sc.shape[0] == 2 * rows and np.isfinite(sc).all()


def test_result_line_fits_a_short_stdout_tail():
    """The full report of a --full run (profiles/r06_bench_steps20.json, 22 KB) goes to stderr; the stdout line
    keeps the headline, `config`, `parity_check`, `roofline`, `cpu_baseline` and the figures of every sub-report
    in a few KB."""
    import json
    import bench
    with open(os.path.join(ROOT, 'profiles', 'r06_bench_steps20.json')) as f:
        full = json.load(f)
    line = bench.result_line(full)
    assert len(json.dumps(line)) <= 6000
    for k in ('metric', 'value', 'unit', 'steps', 'ms_per_step', 'config', 'parity_check', 'roofline', 'cpu_baseline'):
        assert line[k] == full[k], k
    assert line['config4']['value'] == full['config4']['value']
    assert line['config5']['passes']['value'] == full['config5']['passes']['value']
    assert line['roofline_attention']['byte_weighted'] == full['roofline_attention']['byte_weighted']
    assert 'kernels' not in line


def _fake_pipe(S, rows, T, C, passes_per_worker):
    """PassPipeline's worker records as dump_outputs reads them: bucket (next - 1) % 2 holds the last pass"""
    import torch
    workers = []
    for si in range(S):
        buckets = []
        for j in range(2):
            b = types.SimpleNamespace()
            b.scores = torch.full((rows, C), 10.0 * si + j)
            b.tokens = torch.full((T, rows), si * 2 + j, dtype=torch.int32)
            b.validity = torch.ones(rows, dtype=torch.int32)
            buckets.append(b)
        workers.append({'buckets': buckets, 'next': passes_per_worker[si]})
    return types.SimpleNamespace(S=S, workers=workers)


def test_dump_outputs_writes_the_last_pass_of_every_worker(tmp_path):
    import numpy as np
    import bench
    pipe = _fake_pipe(2, 8, 5, 3, [4, 3])            # 7 timed passes: worker 0 ends on bucket 1, worker 1 on 0
    names = bench.dump_outputs(str(tmp_path), pipe, 7)
    assert names == ['scores', 'tokens', 'validity']
    sc, tk, va = (np.load(str(tmp_path / (n + '.npy'))) for n in names)
    assert sc.dtype == tk.dtype == va.dtype == np.float32
    assert sc.shape == (16, 3) and tk.shape == (5, 16) and va.shape == (16,)
    assert (sc[:8] == 1.0).all() and (sc[8:] == 10.0).all()
    assert (tk[:, :8] == 1).all() and (tk[:, 8:] == 2).all()
    # one timed pass: only worker 0 ran one
    names = bench.dump_outputs(str(tmp_path / 'one'), _fake_pipe(2, 8, 5, 3, [1, 0]), 1)
    assert np.load(str(tmp_path / 'one' / 'scores.npy')).shape == (8, 3)


def test_dump_outputs_samples_rows_past_the_limit(tmp_path, monkeypatch):
    import numpy as np
    import bench
    monkeypatch.setattr(bench, 'DUMP_LIMIT_BYTES', 4096)
    pipe = _fake_pipe(1, 256, 5, 3, [1])             # 256 rows x 36 B > 4 KB
    names = bench.dump_outputs(str(tmp_path / 'a'), pipe, 1)
    assert names == ['rows', 'scores', 'tokens', 'validity']
    total = sum(np.load(str(tmp_path / 'a' / (n + '.npy'))).nbytes for n in names)
    assert total <= 4096
    rows = np.load(str(tmp_path / 'a' / 'rows.npy'))
    assert rows.dtype == np.float64 and (np.diff(rows) > 0).all()
    bench.dump_outputs(str(tmp_path / 'b'), pipe, 1)  # the sample is fixed
    assert np.array_equal(rows, np.load(str(tmp_path / 'b' / 'rows.npy')))
