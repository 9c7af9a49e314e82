#!/usr/bin/env python3
"""ExpoMF half-sweeps and the mu update: one JSON line per shape.

Median device time (HIP events inside yue_expo_half_sweep / yue_expo_update_mu, options expo_last_ns / expo_last_gram_ns)
over --iters timed iterations after one warm-up iteration, on the NowPlaying shape (1,744 x 16,864, k = 20) and on C2
(100,000 x 50,000, 50 events per user) at k = 64 and 128; seeded 0.01 * randn factors, mu = 0.01.  Flop model per half-sweep:
rows * columns * (k(k+1) + 2k) for the dense Gram and the scores, plus k^3/3 per solved row; the achieved rate is given
as a fraction of the 157.3 TFLOP/s fp32-matrix figure of AMD's MI355X specification (labelled spec: not measured here).
The reference's CPU time per row at C2, k = 64 is in tests/golden/g13_expomf_c2rows.json (measured when the fixture was made).
    python tools/expomf_bench.py [--iters 3] [--shapes nowplaying,c2k64,c2k128]
For the kernel split run it under ``rocprofv3 --kernel-trace --stats -- python tools/expomf_bench.py --shapes c2k64 --iters 1``.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

SPEC_FP32_MATRIX_TFLOPS = 157.3
SHAPES = {'nowplaying': (1744, 16864, 40, 20), 'c2k64': (100000, 50000, 50, 64), 'c2k128': (100000, 50000, 50, 128)}


def run(dev, name, iters):
    from helpers.numpy_wrmf import pairs_from_events
    from yue_amd import synth
    m, n, d, k = SHAPES[name]
    data = synth.make_arrays(m, n, d)
    ev_u = np.repeat(np.arange(m, dtype=np.int32), np.diff(data['ev_ptr']))
    um, im = pairs_from_events(ev_u, data['ev_i'], m, n)
    rs = np.random.RandomState(20260013)
    theta = (0.01 * rs.randn(m, k)).astype(np.float32)
    beta = (0.01 * rs.randn(n, k)).astype(np.float32)
    dev.set_factors(theta, beta)
    dev.expo_set_pairs(*(um + im))
    dev.expo_set_mu(np.full(n, 0.01, np.float32))
    t = {'user': [], 'item': [], 'user_gram': [], 'item_gram': [], 'mu': []}
    for it in range(1 + iters):
        for side, key in ((0, 'user'), (1, 'item')):
            dev.expo_half_sweep(side, 1e-5, 1.0, side == 0 or m == n)
            if it:
                t[key].append(dev.get_option('expo_last_ns') * 1e-6)
                t[key + '_gram'].append(dev.get_option('expo_last_gram_ns') * 1e-6)
        dev.expo_update_mu(1.0, 99.0, 1.0)
        if it:
            t['mu'].append(dev.get_option('expo_last_ns') * 1e-6)
    med = {key: float(np.median(v)) for key, v in t.items()}
    flop_half = float(m) * n * (k * (k + 1) + 2 * k)
    flop_iter = 2 * flop_half + (m + n) * k ** 3 / 3.0 + 2.0 * m * n * k
    ms_iter = med['user'] + med['item'] + med['mu']
    return {'workload': 'expomf_' + name, 'users': m, 'items': n, 'k': k, 'pairs': int(um[0][-1]), 'iters_timed': iters,
            'ms_user_half': round(med['user'], 3), 'ms_item_half': round(med['item'], 3), 'ms_mu_update': round(med['mu'], 3),
            'ms_gram_user': round(med['user_gram'], 3), 'ms_gram_item': round(med['item_gram'], 3), 'ms_per_iter': round(ms_iter, 3),
            'flop_per_iter_model': flop_iter, 'fp32_tflops': round(flop_iter / (ms_iter * 1e-3) / 1e12, 3),
            'fraction_of_fp32_matrix_spec': round(flop_iter / (ms_iter * 1e-3) / 1e12 / SPEC_FP32_MATRIX_TFLOPS, 4),
            'fp32_matrix_spec_tflops': SPEC_FP32_MATRIX_TFLOPS}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=3)
    ap.add_argument('--shapes', default='nowplaying,c2k64,c2k128')
    args = ap.parse_args()
    from yue_amd._shim import Device
    dev = Device(0, raise_errors=True)
    for name in args.shapes.split(','):
        print(json.dumps(run(dev, name, args.iters)), flush=True)
    dev.close()


if __name__ == '__main__':
    main()
