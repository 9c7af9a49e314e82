#!/usr/bin/env python3
"""LightGCN on one MI355X: device ms per minibatch step, split into forward (3 products), minibatch, backward (3 products) and
Adam (between HIP events: kernels only), the wall time of a whole yue_lgcn_step call through the shim (with the host's sort of
the batch's entries, the uploads and the loss read-back), and the propagation's share of the 8 TB/s roofline by algorithmic
bytes, on a config-2-shaped graph (100,000 x 50,000 users x items, 50 events per user, k 64) and a config-3-shaped one
(1,000,000 x 200,000, 50 events per user, k 128) from yue_amd.synth.
Weights are the squared event counts, as the reference's graph has them.  One JSON line per graph.

Algorithmic bytes of one product: every entry gathers a k-float row and reads its (index, weight) = nnz (4 k + 8); every row
reads its two pointers' share and writes k floats (forward: also reads and writes the running sum F) = N (4 k [+ 8 k] + 8).

    python tools/lightgcn_bench.py [--graphs c2,c3] [--steps 5] [--batch 2048] [--hub 1024]      (YUE_LIB=path of another build of the library)
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

GRAPHS = {'c2': (100000, 50000, 50, 64), 'c3': (1000000, 200000, 50, 128), 'tiny': (2000, 500, 20, 64)}
PEAK = 8e12


def graph_lists(data, m, n):
    """Both sides' lists with weight count^2 from the events (ev_ptr / ev_i) and the sorted-unique lists (indptr / indices)."""
    u_ptr, u_items = data['indptr'], data['indices']
    ev_u = np.repeat(np.arange(m, dtype=np.int64), np.diff(data['ev_ptr']))
    key = ev_u * n + data['ev_i']
    uniq, cnt = np.unique(key, return_counts=True)                 # ascending (user, item): the order of indices
    assert len(uniq) == len(u_items)
    w = (cnt * cnt).astype(np.float32)
    pu = (uniq // n).astype(np.int32)
    o = np.argsort(u_items, kind='stable')                           # by item, users ascending within an item
    i_ptr = np.concatenate([[0], np.cumsum(np.bincount(u_items, minlength=n))]).astype(np.int64)
    return u_ptr, u_items, w, i_ptr, pu[o], w[o]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--graphs', default='c2,c3')
    ap.add_argument('--steps', type=int, default=5)
    ap.add_argument('--batch', type=int, default=2048)
    ap.add_argument('--hub', type=int, default=1024)
    args = ap.parse_args()
    dev = Device(0, raise_errors=True)
    dev.set_option('lgcn_hub', args.hub)
    for name in args.graphs.split(','):
        m, n, d, k = GRAPHS[name]
        data = synth.make_arrays(m, n, d, seed=17)
        lists = graph_lists(data, m, n)
        nnz, N = 2 * len(lists[1]), m + n
        rs = np.random.RandomState(3)
        U = (0.005 * rs.standard_normal((m, k))).astype(np.float32)
        V = (0.005 * rs.standard_normal((n, k))).astype(np.float32)
        dev.set_factors(U, V)
        dev.lgcn_set_graph(m, n, *lists)
        dev.adam_reset()
        ms = {p: [] for p in ('forward', 'batch', 'backward', 'adam')}
        wall = []
        for t in range(1, args.steps + 2):                           # the first step allocates: not counted
            u, i, j = rs.randint(0, m, args.batch), rs.randint(0, n, args.batch), rs.randint(0, n, args.batch)
            t0 = time.perf_counter()
            dev.lgcn_step(3, u, i, j, 0.002, 0.001, t)                # returns after the step's last kernel
            if t > 1:
                wall.append((time.perf_counter() - t0) * 1e3)
                for p in ms:
                    ms[p].append(dev.get_option('lgcn_last_%s_ns' % p) / 1e6)
        med = {p: float(np.median(v)) for p, v in ms.items()}
        fwd_bytes = 3 * (nnz * (4 * k + 8) + N * (12 * k + 8))
        bwd_bytes = 3 * (nnz * (4 * k + 8) + N * (4 * k + 8))        # three gathers (two with J fused, the final one); the gather-free J_L launch is not counted
        row = {'graph': name, 'm': m, 'n': n, 'k': k, 'nnz': nnz, 'max_degree': int(max(np.diff(lists[0]).max(), np.diff(lists[3]).max())),
               'hubs': dev.get_option('lgcn_last_hubs'), 'parts': dev.get_option('lgcn_last_parts'), 'batch': args.batch,
               'ms_device': med, 'ms_step_device': float(sum(med.values())), 'ms_step_wall': float(np.median(wall)),
               'forward_roofline': fwd_bytes / (med['forward'] * 1e-3) / PEAK, 'backward_roofline': bwd_bytes / (med['backward'] * 1e-3) / PEAK}
        print(json.dumps(row), flush=True)
    dev.close()


if __name__ == '__main__':
    main()
