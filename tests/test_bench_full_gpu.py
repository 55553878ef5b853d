"""A plain `bench.py` run times the contract steps and prints the line, nothing else; `--full` adds the legs that take runs of their own
(the CPU baseline with its parity check of the measured path, the secondary workloads, the end-to-end runs)."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTRAS = ('cpu_baseline', 'parity_vs_oracle', 'gpu_over_cpu', 'secondary', 'end_to_end', 'ligands_per_min', 'c1_gpu_s_100_steps')


def _line(args):
    env = {k: v for k, v in os.environ.items() if not k.startswith('KPD_')}      # bench.py refuses KPD_* switches
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--steps', '2', '--warmup', '1', '--repeats', '1',
                        '--batch', '4'] + args, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
    assert p.returncode == 0 and len(lines) == 1, (p.stdout[-2000:], p.stderr[-2000:])
    return json.loads(lines[0])


def test_plain_run_measures_only_the_contract_steps(cuda):
    line = _line(['--n-rec', '60', '--n-lig', '9'])
    assert line['metric'] == 'denoising steps/sec' and line['unit'] == 'steps/s' and line['higher_is_better'] is True
    assert line['dtype'] == 'f32' and line['steps'] == 2 and line['warmup'] == 1
    assert line['value'] > 0 and line['ms_per_step'] > 0 and line['roofline']['frac'] > 0
    for k in EXTRAS:
        assert k not in line, k


def test_full_run_adds_the_cpu_baseline_and_its_parity_check(cuda):
    line = _line(['--full', '--no-secondary'])
    cb = line['cpu_baseline']
    assert cb['kind'] == 'port' and cb['value'] > 0 and set(cb['cases']) == {'B1', 'B8'} and cb['c1_total_s_100_steps'] > 0
    h, x, tol = line['parity_vs_oracle']
    assert h < tol and x < tol and line['gpu_over_cpu'] > 0
    assert 'secondary' not in line and 'end_to_end' not in line
