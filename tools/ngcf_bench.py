#!/usr/bin/env python3
"""NGCF on one MI355X: device ms per minibatch step, split into gather (the three forward products), dense (the three layer
kernels), minibatch, backward (layer kernels and the three transposed products), wgrad and Adam (between HIP events: kernels
only), the wall time of a whole yue_ngcf_step call through the shim, and the forward gather's share of the 8 TB/s roofline by
algorithmic bytes, on a config-2-shaped graph (100,000 x 50,000 users x items, 50 events per user) and a config-3-shaped one
(1,000,000 x 200,000, 50 events per user) from yue_amd.synth, both at k = 64 (3 layers: width 256, the limit).  The graphs have
m > n, so they are built with ``-graph symmetric``; weights are the reference's c (c + 1) / sqrt(d_u) / sqrt(d_t).
The yardstick is LightGCN's step on the same pairs at the same k: its device ms and the ratio.
One JSON line per graph.

Algorithmic bytes of one forward product: every entry gathers a k-float row and reads its (index, weight) = nnz (4 k + 8);
every row reads its two pointers' share and writes k floats = N (4 k + 8).

    python tools/ngcf_bench.py [--graphs c2,c3] [--steps 5] [--batch 2048] [--hub 1024]      (YUE_LIB=path of another build of the library)
"""
import argparse
import json
import os
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

GRAPHS = {'c2': (100000, 50000, 50), 'c3': (1000000, 200000, 50), 'tiny': (2000, 500, 20)}
K, LAYERS, PEAK = 64, 3, 8e12
PHASES = ('gather', 'dense', 'batch', 'backward', 'wgrad', 'adam')


def pairs(data, m, n):
    """Unique (user, item) pairs ascending with their event counts, from the events (ev_ptr / ev_i)."""
    ev_u = np.repeat(np.arange(m, dtype=np.int64), np.diff(data['ev_ptr']))
    uniq, cnt = np.unique(ev_u * n + data['ev_i'], return_counts=True)
    return uniq // n, uniq % n, cnt.astype(np.float64), np.diff(data['ev_ptr']).astype(np.float64), np.bincount(data['ev_i'], minlength=n).astype(np.float64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--graphs', default='c2,c3')
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--batch', type=int, default=2048)
    ap.add_argument('--hub', type=int, default=1024)
    args = ap.parse_args()
    dev = Device(0, raise_errors=True)
    dev.set_option('ngcf_hub', args.hub)
    dev.set_option('lgcn_hub', args.hub)
    for name in args.graphs.split(','):
        m, n, d = GRAPHS[name]
        data = synth.make_arrays(m, n, d, seed=17)
        pu, pt, cnt, du, dt = pairs(data, m, n)
        w = (cnt * (cnt + 1) / np.sqrt(du[pu]) / np.sqrt(np.maximum(dt[pt], 1))).astype(np.float32)
        o = np.argsort(pt, kind='stable')                            # by item, users ascending within an item
        u_ptr = np.concatenate([[0], np.cumsum(np.bincount(pu, minlength=m))]).astype(np.int64)
        i_ptr = np.concatenate([[0], np.cumsum(np.bincount(pt, minlength=n))]).astype(np.int64)
        ptr = np.concatenate([u_ptr, u_ptr[-1] + i_ptr[1:]])
        col = np.concatenate([m + pt, pu[o]]).astype(np.int32)
        ww = np.concatenate([w, w[o]])
        nnz, N = len(col), m + n
        rs = np.random.RandomState(3)
        U = (0.005 * rs.standard_normal((m, K))).astype(np.float32)
        V = (0.005 * rs.standard_normal((n, K))).astype(np.float32)
        lim = np.sqrt(6.0 / (2 * K))
        W = rs.uniform(-lim, lim, size=(LAYERS, 2, K, K)).astype(np.float32)
        batches = [(rs.randint(0, m, args.batch), rs.randint(0, n, args.batch), rs.randint(0, n, args.batch)) for _ in range(args.steps + 1)]
        dev.set_factors(U, V)
        dev.ngcf_set_graph(m, n, ptr, col, ww)
        dev.ngcf_set_weights(W)
        dev.adam_reset()
        ms = {p: [] for p in PHASES}
        wall = []
        for t, (u, i, j) in enumerate(batches, 1):                   # the first step allocates: not counted
            t0 = time.perf_counter()
            dev.ngcf_step(LAYERS, True, 0.9, 2, u, i, j, 0.003, 0.001, t)
            if t > 1:
                wall.append((time.perf_counter() - t0) * 1e3)
                for p in PHASES:
                    ms[p].append(dev.get_option('ngcf_last_%s_ns' % p) / 1e6)
        med = {p: float(np.median(v)) for p, v in ms.items()}
        hubs, parts = dev.get_option('ngcf_last_hubs'), dev.get_option('ngcf_last_parts')
        # the yardstick: LightGCN's step on the same pairs
        dev.set_factors(U, V)
        dev.lgcn_set_graph(m, n, u_ptr, pt.astype(np.int32), w, i_ptr, pu[o].astype(np.int32), w[o])
        dev.adam_reset()
        lg = []
        for t, (u, i, j) in enumerate(batches, 1):
            dev.lgcn_step(LAYERS, u, i, j, 0.003, 0.001, t)
            if t > 1:
                lg.append(sum(dev.get_option('lgcn_last_%s_ns' % p) for p in ('forward', 'batch', 'backward', 'adam')) / 1e6)
        gather_bytes = LAYERS * (nnz * (4 * K + 8) + N * (4 * K + 8))
        total = float(sum(med.values()))
        row = {'graph': name, 'm': m, 'n': n, 'k': K, 'nnz': nnz, 'max_degree': int(np.diff(ptr).max()), 'hubs': hubs, 'parts': parts,
               'batch': args.batch, 'ms_device': med, 'ms_step_device': total, 'ms_step_wall': float(np.median(wall)),
               'gather_roofline': gather_bytes / (med['gather'] * 1e-3) / PEAK, 'ms_lightgcn_step_device': float(np.median(lg)),
               'ratio_to_lightgcn': total / float(np.median(lg))}
        print(json.dumps(row), flush=True)
    dev.close()


if __name__ == '__main__':
    main()
