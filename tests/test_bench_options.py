"""bench.py's plain run and its options: --steps / --warmup / --full / --dump-outputs (parsing and the
output writer need no GPU; one short plain run on the GPU checks the line and the files)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT

sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_plain_run_is_lean_by_default():
    args = bench.parse_args(['--gpus', '1', '--steps', '5', '--warmup', '2'])
    assert (args.steps, args.warmup, args.full, args.dump_outputs) == (5, 2, False, None)
    args = bench.parse_args(['--full', '--dump-outputs', 'out'])
    assert args.full and args.dump_outputs == 'out'


@pytest.mark.parametrize('argv', [['--steps', '0'], ['--warmup', '-1']])
def test_step_counts_are_checked(argv):
    with pytest.raises(SystemExit):
        bench.parse_args(argv)


def test_dump_outputs_writes_logs_and_parameters(tmp_path):
    torch.manual_seed(0)
    model = torch.nn.Module()
    model.small = torch.nn.Linear(3, 4)
    model.big = torch.nn.Parameter(torch.randn(bench.DUMP_MAX_BYTES // 16 + 7))   # > DUMP_MAX_BYTES / 4
    model.register_buffer('fp64', torch.arange(5, dtype=torch.float64))
    model.register_buffer('count', torch.zeros(2, dtype=torch.int64))
    logs = [{'train_loss': [1.0, 2.0], 'test_loss': [3.0, 4.0]},
            {'train_loss': [5.0, 6.0], 'test_loss': [7.0, 8.0]}]
    names = bench.dump_outputs(str(tmp_path / 'a'), logs, model)
    assert names == ['param.big', 'param.fp64', 'param.small.bias', 'param.small.weight',
                     'test_loss', 'train_loss']
    load = lambda d, n: np.load(str(tmp_path / d / (n + '.npy')))      # noqa: E731
    assert load('a', 'test_loss').dtype == np.float64
    np.testing.assert_array_equal(load('a', 'test_loss'), [[3.0, 4.0], [7.0, 8.0]])
    np.testing.assert_array_equal(load('a', 'param.small.weight'), model.small.weight.detach().numpy())
    assert load('a', 'param.small.weight').dtype == np.float32
    assert load('a', 'param.fp64').dtype == np.float64
    big = load('a', 'param.big')
    assert big.shape == (bench.DUMP_SAMPLE,)
    assert np.isin(big, model.big.detach().numpy()).all()
    total = sum(os.path.getsize(str(tmp_path / 'a' / (n + '.npy'))) for n in names)
    assert total <= bench.DUMP_MAX_BYTES
    # the sample is fixed: a second dump of the same tensors is the same file
    bench.dump_outputs(str(tmp_path / 'b'), logs, model)
    np.testing.assert_array_equal(load('b', 'param.big'), big)


@pytest.mark.gpu
def test_plain_bench_run_prints_the_headline_and_dumps_the_last_fit(tmp_path):
    out = tmp_path / 'dump'
    r = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '2',
                        '--warmup', '1', '--pairs', '2000', '--dump-outputs', str(out)],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-4000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line['metric'] == 'summary_vectors_per_sec_in_fit' and line['unit'] == 'pairs/s'
    assert line['higher_is_better'] is True and line['dtype'] == 'f32'
    assert line['steps'] == 2 and line['warmup'] == 1
    assert line['ms_per_step'] > 0
    assert abs(line['value'] - 2000 * 2 / (line['ms_per_step'] * 2e-3)) <= 1e-6 * line['value']
    assert not {'roofline', 'nll_match', 'cpu_baseline', 'per_config', 'scaled_batch_mode'} & set(line)
    test_loss = np.load(str(out / 'test_loss.npy'))
    assert test_loss.shape == (2, 6) and np.isfinite(test_loss).all()
    # the files are the last timed fit's: its mean final held-out NLL is the line's
    assert test_loss[:, -1].mean() == pytest.approx(line['heldout_nll_last_step_mean'], rel=1e-12)
    params = [f for f in os.listdir(str(out)) if f.startswith('param.')]
    assert params and all(np.isfinite(np.load(str(out / f))).all() for f in params)
