"""`bench.py --dump-outputs DIR`: the arrays the last timed step computed, written as DIR/<name>.npy so that two builds can be
compared output by output.  The size cap and the format are checked on the CPU (`dump_outputs` is host code); the end-to-end runs
of bench.py need the GPU."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_dump_writes_float32_and_keeps_float64(tmp_path):
    arrays = {'a': torch.arange(12, dtype=torch.float32).view(4, 3), 'b': np.linspace(0, 1, 5), 'c': torch.tensor(2.5, dtype=torch.float16)}
    files = bench.dump_outputs(str(tmp_path / 'd'), arrays)
    assert sorted(os.path.basename(f) for f in files) == ['a.npy', 'b.npy', 'c.npy']
    a, b, c = (np.load(tmp_path / 'd' / f'{n}.npy') for n in 'abc')
    assert a.dtype == np.float32 and a.shape == (4, 3) and np.array_equal(a, arrays['a'].numpy())
    assert b.dtype == np.float64 and np.array_equal(b, arrays['b'])
    assert c.dtype == np.float32 and c.shape == () and float(c) == 2.5


def test_dump_over_the_limit_is_a_fixed_sample(tmp_path):
    big = {'x': torch.arange(21000, dtype=torch.float32).view(3000, 7), 'y': -torch.arange(1, 501, dtype=torch.float32)}      # value = flat index
    limit = 4000
    for d in ('p', 'q'):
        bench.dump_outputs(str(tmp_path / d), big, limit=limit)
    x, y = np.load(tmp_path / 'p' / 'x.npy'), np.load(tmp_path / 'p' / 'y.npy')
    assert x.nbytes + y.nbytes <= limit and x.size > 0 and y.size > 0
    # same fraction of every array, elements taken in their flat order, the same sample in every run
    assert abs(x.size / big['x'].numel() - y.size / big['y'].numel()) < 0.01
    assert np.all(np.diff(x) > 0) and np.all(np.diff(-y) > 0)
    assert np.array_equal(x, np.load(tmp_path / 'q' / 'x.npy')) and np.array_equal(y, np.load(tmp_path / 'q' / 'y.npy'))


def _bench(args, out_dir):
    env = {k: v for k, v in os.environ.items() if not k.startswith('KPD_')}      # bench.py refuses KPD_* switches
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--no-cpu-baseline', '--no-secondary',
                        '--dump-outputs', str(out_dir)] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
    assert p.returncode == 0 and len(lines) == 1, (p.stdout[-2000:], p.stderr[-2000:])
    return json.loads(lines[0])


@pytest.mark.gpu
def test_sampling_dump_is_the_last_step_and_repeats(cuda, tmp_path):
    args = ['--steps', '3', '--warmup', '1', '--repeats', '2', '--batch', '4']
    line = _bench(args, tmp_path / 'a')
    assert line['steps'] == 3 and line['ms_per_step'] > 0
    _bench(args, tmp_path / 'b')
    names = sorted(os.listdir(tmp_path / 'a'))
    assert names == ['kp_x.npy', 'lig_h.npy', 'lig_x.npy'] and sorted(os.listdir(tmp_path / 'b')) == names
    lig_x, lig_h, kp_x = (np.load(tmp_path / 'a' / n) for n in ('lig_x.npy', 'lig_h.npy', 'kp_x.npy'))
    assert lig_x.dtype == np.float32 and lig_x.shape == (4 * 25, 3) and lig_h.shape == (4 * 25, 10) and kp_x.shape[1] == 3
    assert all(np.isfinite(a).all() for a in (lig_x, lig_h, kp_x))
    # the same arguments give the same inputs (weights, batch, noise) and the path is bit-stable across processes
    for n in names:
        assert np.array_equal(np.load(tmp_path / 'a' / n), np.load(tmp_path / 'b' / n)), n


@pytest.mark.gpu
def test_training_dump_holds_the_loss_and_updated_parameters(cuda, tmp_path):
    line = _bench(['--workload', 'egnn_train', '--steps', '2', '--warmup', '1', '--repeats', '1', '--batch', '2'], tmp_path / 'd')
    full = json.load(open(os.path.join(ROOT, line['full_record'])))
    loss = np.load(tmp_path / 'd' / 'loss_l2.npy')
    assert loss.shape == () and float(loss) == pytest.approx(full['final_l2'], rel=1e-6)
    params = np.load(tmp_path / 'd' / 'parameters.npy')
    model = bench.build_model('cpu', 'egnn_train')
    assert params.dtype == np.float32 and params.size == sum(p.numel() for p in model.parameters())
    assert np.isfinite(params).all()
    # Adam moved the parameters away from their seeded initial values
    init = torch.cat([p.detach().reshape(-1) for p in model.parameters()]).numpy()
    assert not np.array_equal(params, init)
