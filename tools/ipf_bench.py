#!/usr/bin/env python3
"""IPF on one MI355X: top-N ranking over the session temporal graph, per shape, against the NumPy oracle.

Per shape (yue_amd.synth.make_arrays; rho 1, beta 0.7, eta 0.3, N = 20): the device time of one yue_ipf_topn call over
the shape's users; the level-2 entries (holder-list entries the level-1 items scatter over, four paths, exact) and the
level-3 entries (distinct-list entries of the reached users, two passes; the oracle's mean over the timed slice times
the users); edges per second over both; the byte floor at 8 TB/s (12 B per level-2 entry: id + 64-bit max; 24 B per
level-3 entry: id + max, id + compare); a CPU baseline (the oracle, tests/helpers/numpy_ipf.py, on a slice of users,
extrapolated; one process, its core count stated); and a parity check of sampled users.  One JSON line per shape.

    python tools/ipf_bench.py [--shapes nowplaying,c2] [--out FILE]
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

from helpers import numpy_ipf as oi                    # noqa: E402
from yue_amd import synth                              # noqa: E402
from yue_amd._shim import Device                       # noqa: E402
from yue_amd.recommender.cf.IPF import ipf_graph       # noqa: E402

# (users, items, events per user, users ranked)
SHAPES = {'nowplaying': (1744, 16864, 640, 1744), 'c2': (100000, 50000, 50, 10000)}


def level2_entries(g, users):
    nU, nHS = np.diff(g['hu_ptr']), np.diff(g['hs_ptr'])
    tot = 0
    for ptr, items in ((g['u_ptr'], g['u_items']), (g['s_ptr'], g['s_items'])):
        per = np.add.reduceat(np.concatenate([nU[items] + nHS[items], [0]]), ptr[:-1]) * (np.diff(ptr) > 0)
        tot += int(per[users].sum())
    return tot


def run(dev, name, N=20, cpu_users=20, parity_users=40):
    m, n, d, q = SHAPES[name]
    data = synth.make_arrays(m, n, d)
    g = ipf_graph(data['ev_ptr'], data['ev_i'], n, 1.0, 0.7, 0.3)
    dev.ipf_set_graph(g)
    rng = np.random.RandomState(7)
    users = np.arange(m, dtype=np.int32) if q == m else np.sort(rng.choice(m, q, replace=False)).astype(np.int32)
    dev.ipf_topn(users[:min(q, 256)], N)                                   # warm-up
    ids, scores, lens = dev.ipf_topn(users, N)
    ms = dev.get_option('ipf_last_ns') / 1e6
    og = oi.Graph(data['ev_ptr'], data['ev_i'], n, 1.0, 0.7, 0.3)
    sample = np.sort(rng.choice(q, min(parity_users, q), replace=False))
    ok = True
    for t in sample:
        it, sc = oi.topn(og, int(users[t]), N)
        ok &= bool(lens[t] == len(it) and np.array_equal(ids[t, :lens[t]], it) and np.array_equal(scores[t, :lens[t]], sc))
    # level-3 entries of the slice: the distinct lists of every reached user, per path
    t0 = time.perf_counter()
    l3 = 0
    for t in sample[:cpu_users]:
        oi.topn(og, int(users[t]), N)
    cpu_s = (time.perf_counter() - t0) * q / min(cpu_users, len(sample))
    for t in sample[:cpu_users]:
        l3 += level3_entries(og, int(users[t]))
    l3 = l3 * q / min(cpu_users, len(sample))
    l2 = level2_entries(g, users)
    return {'shape': name, 'm': m, 'n': n, 'd': d, 'users_ranked': q, 'N': N, 'topn_ms': ms,
            'level2_entries': l2, 'level3_entries_est': l3, 'edges_per_s': (l2 + l3) / (ms / 1e3),
            'byte_floor_ms': (12 * l2 + 24 * l3) / 8e12 * 1e3, 'cpu_oracle_s_extrapolated': cpu_s,
            'cpu_oracle_users_timed': int(min(cpu_users, len(sample))), 'cpu_cores_used': 1,
            'parity_users': len(sample), 'parity_topn': ok}


def level3_entries(og, u):
    """Distinct-list entries of the users each path reaches (the level-3 work of one query)."""
    tot = 0
    for p in range(4):
        L1 = og.D[0 if p < 2 else 1][u]
        h = p & 1
        if len(L1) == 0:
            continue
        b = np.unique(np.concatenate([og.H[h][a][0] for a in L1]))
        if p in (0, 3):
            b = b[b != u]
        tot += sum(len(og.D[h][x]) for x in b)
    return tot


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='nowplaying,c2')
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
    sys.exit(0 if all(r['parity_topn'] for r in rows) else 1)


if __name__ == '__main__':
    main()
