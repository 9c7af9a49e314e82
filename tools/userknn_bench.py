#!/usr/bin/env python3
"""UserKNN on one MI355X: neighbour kernel and top-N ranking of all users, per shape, against the NumPy oracle.

Per shape (yue_amd.synth.make_arrays; K = 20, N = 20, all users): the neighbour kernel's device time and its rate in
counter increments per second (sum over items of deg^2), the posting-list byte floor 4 * sum deg^2 at 8 TB/s, the top-N
device time, a CPU baseline (the oracle, tests/helpers/numpy_userknn.py, on a slice of users, extrapolated to all users;
one process, its core count stated), and a parity check of sampled users against the oracle.  One JSON line per shape.

    python tools/userknn_bench.py [--shapes nowplaying,c2,c3] [--out FILE]
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

from helpers import numpy_userknn as ok        # noqa: E402
from yue_amd import synth                      # noqa: E402
from yue_amd._shim import Device               # noqa: E402

SHAPES = {'nowplaying': (1744, 16864, 640), 'c2': (100000, 50000, 50), 'c3': (1000000, 200000, 50)}


def run(dev, name, K=20, N=20, cpu_users=100, parity_users=200):
    m, n, d = SHAPES[name]
    data = synth.make_arrays(m, n, d)
    (up, ui, uc), (ip, iu) = ok.pairs_from_events(data['ev_ptr'], data['ev_i'], n)
    deg = np.diff(ip).astype(np.float64)
    work = float((deg * deg).sum())
    dev.knn_set_pairs(m, n, up, ui, uc, ip, iu)
    dev.knn_neighbors(K)                                               # warm-up
    nbr, inter, uni = dev.knn_neighbors(K)
    nb_ms = dev.get_option('knn_last_ns') / 1e6
    users = np.arange(m, dtype=np.int32)
    dev.knn_topn(users[:min(m, 4096)], N)                             # warm-up
    ids, scores, lens = dev.knn_topn(users, N)
    top_ms = dev.get_option('knn_last_ns') / 1e6
    rng = np.random.RandomState(7)
    sample = np.sort(rng.choice(m, min(parity_users, m), replace=False))
    on, oi, oU = ok.neighbors(up, ui, ip, iu, K, sample)
    ok_nb = bool(np.array_equal(nbr[sample], on) and np.array_equal(inter[sample], oi) and np.array_equal(uni[sample], oU))
    ok_top = True
    for t, u in enumerate(sample):
        it, sc = ok.topn(up, ui, uc, u, on[t], oi[t], oU[t], n, N)
        ok_top &= bool(lens[u] == len(it) and np.array_equal(ids[u, :lens[u]], it) and np.array_equal(scores[u, :lens[u]], sc))
    slice_users = sample[:cpu_users]
    t0 = time.perf_counter()
    cn, ci, cU = ok.neighbors(up, ui, ip, iu, K, slice_users)
    for t, u in enumerate(slice_users):
        ok.topn(up, ui, uc, u, cn[t], ci[t], cU[t], n, N)
    cpu_s = (time.perf_counter() - t0) * m / len(slice_users)
    return {'shape': name, 'm': m, 'n': n, 'd': d, 'K': K, 'N': N, 'nnz': int(up[-1]), 'sum_deg2': work,
            'max_item_degree': int(deg.max()), 'neighbors_ms': nb_ms, 'increments_per_s': work / (nb_ms / 1e3),
            'byte_floor_ms': 4 * work / 8e12 * 1e3, 'topn_all_users_ms': top_ms, 'chunked_users': dev.get_option('knn_last_chunked_users'),
            'cpu_oracle_s_extrapolated': cpu_s, 'cpu_oracle_users_timed': len(slice_users), 'cpu_cores_used': 1,
            'parity_users': len(sample), 'parity_neighbors': ok_nb, 'parity_topn': ok_top}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='nowplaying,c2,c3')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dev = Device(0, raise_errors=True)
    rows = []
    for name in args.shapes.split(','):
        row = run(dev, name)
        print(json.dumps(row), flush=True)
        rows.append(row)
    if args.out:
        json.dump(rows, open(args.out, 'w'), indent=1)
    dev.close()
    sys.exit(0 if all(r['parity_neighbors'] and r['parity_topn'] for r in rows) else 1)


if __name__ == '__main__':
    main()
