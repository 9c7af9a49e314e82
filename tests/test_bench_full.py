"""bench.py without and with --full: a plain run prints the line of its own timed steps and nothing that takes runs of its
own; --full adds the CPU baselines and the other measurements beside the line."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step', 'steps', 'warmup', 'roofline', 'config')


def _line(*args):
    res = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1'] + list(args),
                         cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert res.returncode == 0, res.stderr.decode()[-3000:]
    lines = [ln for ln in res.stdout.decode().splitlines() if ln.startswith('{')]
    assert len(lines) == 1, res.stdout.decode()[-2000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_leaves_the_extras_to_full():
    plain = _line('--workload', 'tiny', '--steps', '2', '--warmup', '1')
    assert all(key in plain for key in HEADLINE) and plain['steps'] == 2 and plain['warmup'] == 1 and plain['value'] > 0
    assert 'cpu_baseline' not in plain and 'secondary' not in plain
    full = _line('--full', '--workload', 'tiny', '--steps', '2', '--warmup', '1')
    assert all(key in full for key in HEADLINE) and full['metric'] == plain['metric'] and full['unit'] == plain['unit']
    cpu = full['cpu_baseline']
    assert cpu['value'] > 0 and cpu['numpy_loop']['value'] > 0 and cpu['hogwild']['value'] > 0
    # FISM: the sequential device pass is a run of its own as well
    plain = _line('--workload', 'fism', '--steps', '1', '--warmup', '0')
    assert 'sequential_device_pass_draws_per_s' not in plain['config'] and plain['cpu_baseline'] is None
    full = _line('--full', '--workload', 'fism', '--steps', '1', '--warmup', '0', '--no-cpu-baseline')
    assert full['config']['sequential_device_pass_draws_per_s'] > 0 and full['cpu_baseline'] is None
