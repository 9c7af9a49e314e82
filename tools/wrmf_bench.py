#!/usr/bin/env python3
"""WRMF half-sweeps at C3 (1M users x 200K items, d = 50, k = 128): one JSON line.

Median device time per iteration and per half-sweep (HIP events inside yue_wrmf_half_sweep, options wrmf_last_ns /
wrmf_last_long_ns) over --iters timed iterations after one warm-up iteration; pairs; the flop model from shapes
(Gram updates nnz * k(k+1)/2 per side, Cholesky k^3/6 per row, 2 flop per multiply-add); achieved fp64 TFLOP/s and the
fraction of the 78.6 TFLOP/s fp64 figure of AMD's MI355X specification (labelled spec: not measured here); the time of
the long-row chunks.  CPU baselines: the reference's per-row statements (recommender/cf/WRMF.py:37-56 / :63-75, restated)
timed on sampled users and items and extrapolated to a whole iteration, and the contract oracle's per-row rate.
    python tools/wrmf_bench.py [--iters 5] [--cpu-users 20] [--cpu-items 4]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

SPEC_FP64_TFLOPS = 78.6


def reference_row(F, FtF, ids, cnt, reg, n_fixed):
    """One row of the reference's half-sweep, its statements at its dtypes (dense over all n_fixed rows of F)."""
    from scipy.sparse import coo_matrix
    H = np.ones(n_fixed)
    P_u = np.zeros(n_fixed)
    H[ids] += 10 * cnt
    P_u[ids] = 1
    C_u = coo_matrix((10 * cnt, (ids, ids)), shape=(n_fixed, n_fixed))
    A = (FtF + np.dot(F.T, C_u.dot(F)) + reg * np.eye(F.shape[1]))
    return np.dot(np.linalg.inv(A), (F.T * H).dot(P_u))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--users', type=int, default=1000000)
    ap.add_argument('--items', type=int, default=200000)
    ap.add_argument('--d', type=int, default=50)
    ap.add_argument('--k', type=int, default=128)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--cpu-users', type=int, default=20)
    ap.add_argument('--cpu-items', type=int, default=4)
    ap.add_argument('--no-cpu', action='store_true')
    args = ap.parse_args()
    from helpers.numpy_wrmf import gram_fp32, pairs_from_events, wrmf_half_sweep_contract
    from yue_amd import synth
    from yue_amd._shim import Device
    m, n, k = args.users, args.items, args.k
    data = synth.make_arrays(m, n, args.d)
    P0, Q0 = synth.init_factors(m, n, k)
    X0, Y0 = P0 * 10, Q0 * 10
    ev_u = np.repeat(np.arange(m, dtype=np.int32), np.diff(data['ev_ptr']))
    (up, ui, uc), (ip, iu, ic) = pairs_from_events(ev_u, data['ev_i'], m, n)
    nnz = int(up[-1])
    dev = Device(0, raise_errors=True)
    dev.set_factors(X0, Y0)
    t0 = time.time()
    dev.wrmf_set_pairs(up, ui, uc, ip, iu, ic)
    set_pairs_s = time.time() - t0
    times = {'user': [], 'item': [], 'user_long': [], 'item_long': []}
    for it in range(1 + args.iters):
        for side, name in ((0, 'user'), (1, 'item')):
            dev.wrmf_half_sweep(side, 10.0, 1.0)
            if it > 0:
                times[name].append(dev.get_option('wrmf_last_ns') * 1e-6)
                times[name + '_long'].append(dev.get_option('wrmf_last_long_ns') * 1e-6)
    per_iter = [a + b for a, b in zip(times['user'], times['item'])]
    ms = float(np.median(per_iter))
    gram_ma = 2.0 * nnz * k * (k + 1) / 2
    chol_ma = (m + n) * k ** 3 / 6.0
    flop = 2.0 * (gram_ma + chol_ma)
    out = {'workload': 'wrmf_c3', 'users': m, 'items': n, 'k': k, 'pairs': nnz, 'iters_timed': args.iters,
           'ms_per_iter': round(ms, 3), 'ms_user_half': round(float(np.median(times['user'])), 3), 'ms_item_half': round(float(np.median(times['item'])), 3),
           'ms_long_rows_user': round(float(np.median(times['user_long'])), 3), 'ms_long_rows_item': round(float(np.median(times['item_long'])), 3),
           'long_rows_item': dev.get_option('wrmf_long_rows_item'), 'long_pairs_threshold': dev.get_option('wrmf_long_pairs'),
           'flop_per_iter_model': flop, 'fp64_tflops': round(flop / (ms * 1e-3) / 1e12, 3),
           'fraction_of_fp64_spec': round(flop / (ms * 1e-3) / 1e12 / SPEC_FP64_TFLOPS, 4), 'fp64_spec_tflops': SPEC_FP64_TFLOPS,
           'set_pairs_s': round(set_pairs_s, 2)}
    X, Y = dev.get_factors()
    dev.close()
    if not args.no_cpu:
        rng = np.random.RandomState(1)
        users = rng.choice(m, args.cpu_users, replace=False)
        items = rng.choice(n, args.cpu_items, replace=False)
        YtY = Y.T.dot(Y)
        t0 = time.time()
        for u in users:
            reference_row(Y, YtY, ui[up[u]:up[u + 1]], uc[up[u]:up[u + 1]], 1.0, n)
        t_user = (time.time() - t0) / len(users)
        XtX = X.T.dot(X)
        t0 = time.time()
        for i in items:
            reference_row(X, XtX, iu[ip[i]:ip[i + 1]], ic[ip[i]:ip[i + 1]], 1.0, m)
        t_item = (time.time() - t0) / len(items)
        out['cpu_reference_form_s_per_iter_extrapolated'] = round(t_user * m + t_item * n, 1)
        out['cpu_reference_form_sampled'] = {'users': len(users), 's_per_user': round(t_user, 4), 'items': len(items), 's_per_item': round(t_item, 4)}
        rows = rng.choice(m, 2000, replace=False)
        G = gram_fp32(Y)
        t0 = time.time()
        wrmf_half_sweep_contract(Y, up, ui, uc, 1.0, rows=rows, G=G)
        out['cpu_contract_oracle_user_rows_per_s'] = round(len(rows) / (time.time() - t0), 1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
