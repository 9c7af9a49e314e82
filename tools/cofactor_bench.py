#!/usr/bin/env python3
"""CoFactor on a synthetic log: one JSON line.

Device time of the co-occurrence build (HIP events inside yue_cof_cooccur, option cof_last_ns), host time of the SPPMI, and
the median over --iters timed iterations (after one warm-up iteration) of the user half-sweep (wrmf_last_ns) and the item
sweep (cof_last_ns), with the part of the item sweep spent in levels of fewer than 256 rows (cof_last_small_ns), cof_levels and
cof_cooccur_nnz.
    python tools/cofactor_bench.py [--users 1000 --items 1000 --d 20 --k 20 --filter 2] [--iters 5]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--users', type=int, default=1000)
    ap.add_argument('--items', type=int, default=1000)
    ap.add_argument('--d', type=int, default=20)
    ap.add_argument('--k', type=int, default=20)
    ap.add_argument('--filter', type=int, default=2)
    ap.add_argument('--neg', type=int, default=1)
    ap.add_argument('--gamma', type=float, default=1.0)
    ap.add_argument('--reg', type=float, default=1.0)
    ap.add_argument('--iters', type=int, default=5)
    args = ap.parse_args()
    from helpers.numpy_wrmf import pairs_from_events
    from yue_amd import synth
    from yue_amd._shim import Device
    from yue_amd.recommender.advanced.CoFactor import sppmi_from_counts
    m, n, k = args.users, args.items, args.k
    data = synth.make_arrays(m, n, args.d)
    P0, Q0 = synth.init_factors(m, n, k)
    ev_u = np.repeat(np.arange(m, dtype=np.int32), np.diff(data['ev_ptr']))
    um, im = pairs_from_events(ev_u, data['ev_i'], m, n)
    rs = np.random.RandomState(1)
    dev = Device(0, raise_errors=True)
    dev.set_option('cof_level_timing', 1)
    dev.set_factors(P0 * 10, Q0 * 10)
    dev.wrmf_set_pairs(*(um + im))
    co = dev.cof_cooccur(args.filter)
    cooccur_ms = dev.get_option('cof_last_ns') * 1e-6
    t0 = time.time()
    sp = sppmi_from_counts(co[0], co[1], co[2], args.neg)
    sppmi_s = time.time() - t0
    dev.cof_set_sppmi(*sp)
    dev.cof_set_state(rs.rand(n, k) / 10, rs.rand(n) / 10, rs.rand(n) / 10)
    user, item, small = [], [], []
    for it in range(1 + args.iters):
        dev.wrmf_half_sweep(0, 10.0, args.reg)
        u_ms = dev.get_option('wrmf_last_ns') * 1e-6
        dev.cof_item_sweep(10.0, args.reg, args.gamma)
        if it > 0:
            user.append(u_ms)
            item.append(dev.get_option('cof_last_ns') * 1e-6)
            small.append(dev.get_option('cof_last_small_ns') * 1e-6)
    out = {'workload': 'cofactor', 'users': m, 'items': n, 'k': k, 'pairs': int(um[0][-1]), 'filter': args.filter, 'iters_timed': args.iters,
           'cooccur_ms': round(cooccur_ms, 3), 'cof_cooccur_nnz': dev.get_option('cof_cooccur_nnz'), 'sppmi_host_s': round(sppmi_s, 3),
           'sppmi_nnz': int(sp[0][-1]), 'cof_levels': dev.get_option('cof_levels'),
           'ms_user_half': round(float(np.median(user)), 3), 'ms_item_sweep': round(float(np.median(item)), 3),
           'ms_per_iter': round(float(np.median(user) + np.median(item)), 3),
           'ms_item_sweep_small_levels': round(float(np.median(small)), 3),
           'small_level_share': round(float(np.median(small) / np.median(item)), 3)}
    dev.close()
    print(json.dumps(out))


if __name__ == '__main__':
    main()
