#!/usr/bin/env python3
"""APR on one MI355X: device ms per minibatch step, split into the coefficient launches, the parameter-gradient rows, the
perturbation rows (gradient and normalisation) and adam (between HIP events), for a phase-1 and for an adversarial step; the wall
time of a whole call through the shim; the host time of the reference's sampler (next_batch as written, :95-111, on ids); and
yue_adam_step (float atomics) beside the phase-1 step on the same triplets.  Batch 512 events x 3 negatives
(T = 1536), k = 64, on a config-2-shaped log (100,000 x 50,000 users x items, 50 events per user) and a config-3-shaped one
(1,000,000 x 200,000, 50 events per user; also at its own k = 128) from yue_amd.synth.  One JSON line per run.

The yardstick is derived, not measured: TF-1 applies Adam to every row, so a step reads the variable, both moments and the gradient
buffer and writes three of them for U and V: about (m + n) k 4 B x 6.  Reported: the measured device step time and its ratio to that
floor at 8 TB/s, the phase that dominates, and the longest list of terms one wave added with that wave's share of the step (the
rows launch is bounded below by its longest wave: its whole time is charged to that wave, an upper bound of the share).

    python tools/apr_bench.py [--logs c2,c3,c3k128] [--steps 5] [--batch 512]      (YUE_LIB=path of another build of the library)
"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from yue_amd import _shim                      # noqa: E402
from yue_amd import synth                      # noqa: E402
from yue_amd._shim import Device               # noqa: E402
if os.environ.get('YUE_LIB'):
    _shim.LIB_PATH = os.environ['YUE_LIB']

LOGS = {'c2': (100000, 50000, 50, 64), 'c3': (1000000, 200000, 50, 64), 'c3k128': (1000000, 200000, 50, 128), 'tiny': (2000, 500, 20, 64)}
PEAK, NEG, LR, REG, EPS, REG_A = 8e12, 3, 0.003, 0.002, 0.5, 2.0
PHASES = ('coef', 'rows', 'norm', 'adam')


def next_batch(ev_u, ev_i, listened, n, batch):
    """The reference's loop on ids: the batch's events by np.random.randint, then NEG rejection-sampled negatives per event."""
    u_idx, i_idx, j_idx = [], [], []
    for idx in np.random.randint(len(ev_u), size=batch):
        user = int(ev_u[idx])
        mine = listened[user]
        for _ in range(NEG):
            item_j = random.randint(0, n - 1)
            while item_j in mine:
                item_j = random.randint(0, n - 1)
            u_idx.append(user); i_idx.append(int(ev_i[idx])); j_idx.append(item_j)
    return u_idx, i_idx, j_idx


def median(rows):
    return {p: float(np.median([r[q] for r in rows])) / 1e6 for q, p in enumerate(PHASES)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--logs', default='c2,c3,c3k128')
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--batch', type=int, default=512)
    args = ap.parse_args()
    dev = Device(0, raise_errors=True)
    for name in args.logs.split(','):
        m, n, d, k = LOGS[name]
        data = synth.make_arrays(m, n, d, seed=17)
        ev_u = np.repeat(np.arange(m, dtype=np.int32), np.diff(data['ev_ptr']))
        ev_i = data['ev_i']
        indptr, indices = data['indptr'], data['indices']

        class Listened(dict):                                        # a user's item set, built when the sampler first meets the user
            def __missing__(self, u):
                self[u] = set(indices[indptr[u]:indptr[u + 1]].tolist())
                return self[u]
        listened = Listened()
        rs = np.random.RandomState(3)
        U, V = (0.005 * rs.standard_normal((m, k))).astype(np.float32), (0.005 * rs.standard_normal((n, k))).astype(np.float32)
        dev.set_factors(U, V)
        dev.adam_reset()
        dev.apr_reset()
        np.random.seed(5); random.seed(5)
        pre, adv, atom, wall_pre, wall_adv, wall_atom, host, longest = [], [], [], [], [], [], [], []
        step = 0
        for t in range(args.steps + 1):                              # the first step of each kind allocates: not counted
            t0 = time.perf_counter()
            u, i, j = next_batch(ev_u, ev_i, listened, n, args.batch)
            t1 = time.perf_counter()
            step += 1
            dev.apr_pre_step(u, i, j, LR, REG, step)
            t2 = time.perf_counter()
            times, rows = dev.apr_times(), dev.get_option('apr_last_longest_row')
            step += 1
            dev.set_kernel_timing(0)
            t3 = time.perf_counter()
            dev.adam_step(u, i, j, LR, REG, step)                    # the same triplets through k_mb_grad's float atomics
            t4 = time.perf_counter()
            if t > 0:
                host.append((t1 - t0) * 1e3); wall_pre.append((t2 - t1) * 1e3); wall_atom.append((t4 - t3) * 1e3); pre.append(times); longest.append(rows)
        for t in range(args.steps + 1):
            u, i, j = next_batch(ev_u, ev_i, listened, n, args.batch)
            step += 1
            t1 = time.perf_counter()
            loss = dev.apr_adv_step(u, i, j, LR, EPS, REG_A, step)
            t2 = time.perf_counter()
            if t > 0:
                wall_adv.append((t2 - t1) * 1e3); adv.append(dev.apr_times())
        med_pre, med_adv = median(pre), median(adv)
        floor_bytes = (m + n) * k * 4 * 6
        floor_ms = floor_bytes / PEAK * 1e3
        total_pre, total_adv = float(sum(med_pre.values())), float(sum(med_adv.values()))
        row = {'log': name, 'm': m, 'n': n, 'k': k, 'batch': args.batch, 'T': NEG * args.batch, 'loss_adv': loss,
               'ms_device_pre': med_pre, 'ms_step_device_pre': total_pre, 'ms_device_adv': med_adv, 'ms_step_device_adv': total_adv,
               'ms_step_wall_pre': float(np.median(wall_pre)), 'ms_step_wall_adv': float(np.median(wall_adv)),
               'ms_step_wall_adam_step_atomics': float(np.median(wall_atom)), 'ms_host_sampler': float(np.median(host)),
               'floor_bytes_derived': floor_bytes, 'floor_ms_at_8TBs_derived': floor_ms, 'pre_ratio_to_floor': total_pre / floor_ms,
               'adv_ratio_to_floor': total_adv / floor_ms, 'dominant_phase_pre': max(med_pre, key=med_pre.get), 'dominant_phase_adv': max(med_adv, key=med_adv.get),
               'longest_row': int(max(longest)), 'longest_wave_share_of_pre_step_at_most': med_pre['rows'] / total_pre}
        print(json.dumps(row), flush=True)
    dev.close()


if __name__ == '__main__':
    main()
