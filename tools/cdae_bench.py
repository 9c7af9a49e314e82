#!/usr/bin/env python3
"""CDAE on one MI355X: device ms per minibatch step, split into encode, decode (with the sums of squares), regroup and adam
(between HIP events), the wall time of a whole yue_cdae_step call through the shim, and the host time of the reference's sampler
(next_batch as written, :76-98, on ids), at batch 256 and h = 128 on a config-2-shaped log (100,000 x 50,000 users x items, 50
events per user) and a config-3-shaped one (1,000,000 x 200,000, 50 events per user) from yue_amd.synth.  One JSON line per log.

The yardstick is derived, not measured: TF-1 applies Adam to every row of every variable, so a step reads the variable and both
moments and writes all three for U, W and W': (m + 2 n) h 4 B x 6, about 4.3 GB on config 3.  Everything else (about 10^5 sampled
entries) is small beside it.  Reported: the measured device step time and its ratio to that floor at 8 TB/s, and the phase that
dominates.  There is no earlier implementation to compare against.

    python tools/cdae_bench.py [--logs c2,c3] [--steps 5] [--batch 256] [--hub 1024]      (YUE_LIB=path of another build of the library)
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

LOGS = {'c2': (100000, 50000, 50), 'c3': (1000000, 200000, 50), 'tiny': (2000, 500, 20)}
H, PEAK, CO, NEG, STDDEV = 128, 8e12, 0.1, 5, 0.05
PHASES = ('encode', 'decode', 'regroup', 'adam')


def user_csr(data, m, n):
    """(ptr, items ascending, counts) of the distinct pairs, from the events (ev_ptr / ev_i)."""
    ev_u = np.repeat(np.arange(m, dtype=np.int64), np.diff(data['ev_ptr']))
    uniq, cnt = np.unique(ev_u * n + data['ev_i'], return_counts=True)
    ptr = np.concatenate([[0], np.cumsum(np.bincount(uniq // n, minlength=m))]).astype(np.int64)
    return ptr, (uniq % n).astype(np.int32), cnt.astype(np.int32)


def next_batch(ptr, items, user_list, item_list, batch):
    """The reference's loop on ids: one choice per slot, then NEG choices per item of the user; the sample is a set."""
    users, sets = [], []
    for _ in range(batch):
        u = random.choice(user_list)
        mine = items[ptr[u]:ptr[u + 1]].tolist()
        sample = set(mine)
        for _ in range(NEG * len(mine)):
            sample.add(random.choice(item_list))
        users.append(u)
        sets.append(sample)
    sptr = np.zeros(batch + 1, np.int64)
    sptr[1:] = np.cumsum([len(s) for s in sets])
    return users, sptr, np.array([i for s in sets for i in sorted(s)], np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--logs', default='c2,c3')
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--hub', type=int, default=1024)
    args = ap.parse_args()
    dev = Device(0, raise_errors=True)
    dev.set_option('cdae_hub', args.hub)
    for name in args.logs.split(','):
        m, n, d = LOGS[name]
        data = synth.make_arrays(m, n, d, seed=17)
        ptr, items, cnt = user_csr(data, m, n)
        rs = np.random.RandomState(3)
        lim = np.sqrt(6.0 / (m + H))
        U = rs.uniform(-lim, lim, size=(m, H)).astype(np.float32)
        W, Wd = (STDDEV * rs.standard_normal((n, H))).astype(np.float32), (STDDEV * rs.standard_normal((H, n))).astype(np.float32)
        b, bd = (STDDEV * rs.standard_normal(H)).astype(np.float32), (STDDEV * rs.standard_normal(n)).astype(np.float32)
        dev.cdae_set_data(m, n, ptr, items, cnt)
        dev.cdae_set_params(U, W, Wd, b, bd)
        random.seed(5)
        user_list, item_list = list(range(m)), list(range(n))
        ms = {p: [] for p in PHASES}
        wall, host, entries, sat = [], [], [], 0
        for t in range(1, args.steps + 2):                           # the first step allocates: not counted
            t0 = time.perf_counter()
            users, sptr, sitems = next_batch(ptr, items, user_list, item_list, args.batch)
            t1 = time.perf_counter()
            loss, s = dev.cdae_step(users, sptr, sitems, CO, 2, 0.001, 0.1, t)
            t2 = time.perf_counter()
            sat += s
            if t > 1:
                host.append((t1 - t0) * 1e3); wall.append((t2 - t1) * 1e3); entries.append(int(sptr[-1]))
                for p, ns in zip(PHASES, dev.cdae_times()):
                    ms[p].append(ns / 1e6)
        med = {p: float(np.median(v)) for p, v in ms.items()}
        total = float(sum(med.values()))
        floor_bytes = (m + 2 * n) * H * 4 * 6
        floor_ms = floor_bytes / PEAK * 1e3
        hubs = dev.get_option('cdae_last_hubs')
        t0 = time.perf_counter()
        dev.cdae_load_factors()
        load_ms = (time.perf_counter() - t0) * 1e3
        row = {'log': name, 'm': m, 'n': n, 'h': H, 'pairs': int(ptr[-1]), 'batch': args.batch, 'sampled_entries': int(np.median(entries)),
               'hubs': hubs, 'saturated_steps': sat, 'loss': loss, 'ms_device': med, 'ms_step_device': total,
               'ms_step_wall': float(np.median(wall)), 'ms_host_sampler': float(np.median(host)), 'floor_bytes': floor_bytes, 'floor_ms_at_8TBs': floor_ms,
               'ratio_to_floor': total / floor_ms, 'adam_ratio_to_floor': med['adam'] / floor_ms, 'dominant_phase': max(med, key=med.get),
               'ms_load_factors_wall': load_ms}
        print(json.dumps(row), flush=True)
    dev.close()


if __name__ == '__main__':
    main()
