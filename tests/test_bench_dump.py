"""bench.py --dump-outputs: the helpers on the host (CPU), and the flag on every kind of timed path (GPU) -- the files hold what
the last timed step computed, within 64 MB, and --steps sets the number of timed epochs."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    sys.path.insert(0, ROOT)
    import bench
    return bench


def test_dump_rows_is_a_fixed_sample_within_the_budget():
    bench = _bench()
    assert np.array_equal(bench.dump_rows(1000, 512), np.arange(1000))         # fits: every row
    a, b = bench.dump_rows(1000000, 512), bench.dump_rows(1000000, 512)
    assert np.array_equal(a, b) and len(a) == (16 << 20) // 512
    assert (np.diff(a) > 0).all() and a[0] >= 0 and a[-1] < 1000000


def test_dump_outputs_writes_float_arrays_and_keeps_the_limit(tmp_path):
    bench = _bench()
    ids = np.arange(12, dtype=np.int32).reshape(3, 4)
    sc = np.linspace(0, 1, 12, dtype=np.float32).reshape(3, 4)
    bench.dump_outputs(str(tmp_path / 'd'), {'ids': ids, 'scores': sc})
    got_ids, got_sc = np.load(tmp_path / 'd' / 'ids.npy'), np.load(tmp_path / 'd' / 'scores.npy')
    assert got_ids.dtype == np.float64 and np.array_equal(got_ids, ids)
    assert got_sc.dtype == np.float32 and np.array_equal(got_sc, sc)
    with pytest.raises(SystemExit):
        bench.dump_outputs(str(tmp_path / 'big'), {'x': np.zeros((65 << 20) // 4, np.float32)})
    assert not os.path.exists(tmp_path / 'big')


def _run(tmp_path, name, *args):
    out = tmp_path / name
    res = subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py'), '--gpus', '1', '--no-cpu-baseline', '--dump-outputs', str(out)] + list(args),
                         cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    assert res.returncode == 0, res.stderr.decode()[-3000:]
    lines = [ln for ln in res.stdout.decode().splitlines() if ln.startswith('{')]
    assert len(lines) == 1, res.stdout.decode()[-2000:]
    arrays = {os.path.basename(f)[:-4]: np.load(f) for f in glob.glob(str(out / '*.npy'))}
    assert arrays and all(a.dtype in (np.float32, np.float64) for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    return json.loads(lines[0]), arrays


@pytest.mark.gpu
def test_bench_dumps_what_the_timed_steps_computed(tmp_path):
    # BPR epochs (tiny: factors small enough to be dumped whole): the sums of the last epoch belong to the dumped factors
    one, _ = _run(tmp_path, 'tiny1', '--workload', 'tiny', '--steps', '1', '--warmup', '1')
    out, a = _run(tmp_path, 'tiny3', '--workload', 'tiny', '--steps', '3', '--warmup', '1')
    assert out['steps'] == 3 and out['ms_per_step'] > 0
    assert out['roofline']['launches_timed'] == 3 * one['roofline']['launches_timed']        # --steps sets the timed epochs
    m, n = 20000, 5000
    assert a['P_rows'].shape == (m, 128) and a['Q_rows'].shape == (n, 128) and np.array_equal(a['P_row_index'], np.arange(m))
    nll, sp, sq = a['epoch_sums']
    E = m * 20
    assert abs(nll / E - out['config']['final_nll_per_triplet']) <= 1e-12 * abs(nll / E)
    assert abs(np.sum(a['P_rows'].astype(np.float64) ** 2) - sp) <= 1e-5 * sp
    assert abs(np.sum(a['Q_rows'].astype(np.float64) ** 2) - sq) <= 1e-5 * sq
    # top-N scan of every user: ids are item numbers, scores non-increasing along a list
    out, a = _run(tmp_path, 'c5small', '--workload', 'c5small', '--steps', '1', '--warmup', '0')
    assert out['steps'] == 1 and out['ms_per_step'] > 0
    assert a['topn_ids'].shape == (65536, 20) and a['topn_scores'].shape == (65536, 20)
    assert np.array_equal(a['user_index'], np.arange(65536))
    assert (a['topn_ids'] >= 0).all() and (a['topn_ids'] < 200000).all() and (np.diff(a['topn_scores'], axis=1) <= 0).all()
    # FISM rounds: the model and the sums of the last timed epoch
    out, a = _run(tmp_path, 'fism', '--workload', 'fism', '--steps', '1', '--warmup', '0')
    assert out['steps'] == 1 and out['ms_per_step'] > 0
    assert a['P_rows'].dtype == np.float64 and a['P_rows'].shape == (20000, 64) and a['Bi_rows'].shape == (20000,)
    half, sP, sQ, sB = a['fism_sums']
    assert abs(half - out['config']['final_half_sq_error']) <= 1e-12 * abs(half)
    assert abs(np.sum(a['P_rows'] ** 2) - sP) <= 1e-9 * sP and abs(np.sum(a['Q_rows'].astype(np.float64) ** 2) - sQ) <= 1e-5 * sQ
    assert abs(np.dot(a['Bi_rows'], a['Bi_rows']) - sB) <= 1e-9 * sB
