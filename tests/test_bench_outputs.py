"""bench.py's own contract: a plain run prints the headline line only (the extras are behind
--full), --steps sets the number of timed steps, and --dump-outputs writes what the last timed
step computed -- the same arrays from run to run with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from hip_util import rel_l2

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 10071          # parameters of the demo model
FULL_ONLY = ('kernel_ms', 'roofline', 'hbm_roofline', 'step_flops', 'b100_ms', 'b200_ms',
             'autograd_route_ms', 'autograd_route_b100_ms', 'c5_b50_ms', 'config5', 'cpu_baseline')


def _run(args, timeout=600):
    env = {k: v for k, v in os.environ.items()
           if k not in ('WORLD_SIZE', 'RANK', 'LOCAL_RANK', 'NJODE_BENCH_SHARE_GPU')}
    return subprocess.run([sys.executable, os.path.join(REPO, 'bench.py')] + args, env=env, cwd=REPO,
                          stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=timeout)


def test_bench_offers_full_and_dump_outputs():
    p = _run(['--help'], timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    assert '--full' in p.stdout and '--dump-outputs' in p.stdout


def _plain(tmp_path, tag, steps):
    out = tmp_path / tag
    p = _run(['--gpus', '1', '--steps', str(steps), '--warmup', '1', '--dump-outputs', str(out)])
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith('{')]
    assert len(lines) == 1, p.stdout[-2000:]
    return json.loads(lines[0]), {n: np.load(out / (n + '.npy')) for n in ('loss', 'grad', 'params')}


@pytest.mark.gpu
def test_plain_bench_is_the_headline_and_dumps_its_last_step(tmp_path):
    line, got = _plain(tmp_path, 'a', 3)
    for key in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
        assert key in line, key
    assert line['steps'] == 3 and line['unit'] == 'paths/s' and line['dtype'] == 'f32'
    assert line['value'] == pytest.approx(20000 / (line['ms_per_step'] * 1e-3), rel=1e-3)
    assert not [k for k in FULL_ONLY if k in line]
    assert got['loss'].dtype == np.float64 and got['loss'].shape == (1,)
    assert float(got['loss'][0]) == pytest.approx(line['final_loss'], rel=1e-7)
    for name in ('grad', 'params'):
        assert got[name].dtype == np.float32 and got[name].shape == (P,)
        assert np.isfinite(got[name]).all() and np.abs(got[name]).max() > 0
    # same arguments, same inputs: the same outputs (up to fp32 summation order)
    _, again = _plain(tmp_path, 'b', 3)
    assert float(again['loss'][0]) == pytest.approx(float(got['loss'][0]), rel=1e-6)
    for name in ('grad', 'params'):
        assert rel_l2(again[name], got[name]) < 1e-6, name
    # --steps is the number of timed steps: one more step moves the parameters
    _, longer = _plain(tmp_path, 'c', 4)
    assert not np.array_equal(longer['params'], got['params'])
