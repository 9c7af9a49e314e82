#!/usr/bin/env python3
"""CUNE's user-network stage on one MI355X: device time of each stage (pairs upload + prefix, walks, embedding, friends)
on a synthetic log at two sizes, C1-like (1000 x 1000, 20 events) and config 2 (100K users x 50K items, 50 events), with
CUNE.conf's options (T 20, L 10, dim 20, window 5, K 50, 10 epochs).  One JSON line per shape.  Friends are all-pairs
(network users squared): --friends-cap limits the shape they are timed on.

    python tools/cune_net_bench.py [--shapes c1,c2] [--epochs 10] [--friends-cap 20000] [--out FILE]
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

from helpers import numpy_cune_net as cn       # noqa: E402
from yue_amd import synth                      # noqa: E402
from yue_amd._shim import Device               # noqa: E402

SHAPES = {'c1': (1000, 1000, 20), 'c2': (100000, 50000, 50)}


def run(dev, name, epochs, friends_cap, T=20, L=10, dim=20, window=5, K=50, seed=1):
    m, n, d = SHAPES[name]
    data = synth.make_arrays(m, n, d)
    ev_u = np.repeat(np.arange(m), np.diff(data['ev_ptr']))
    (up, ui), (ip, iu) = cn.pairs_from_events(ev_u, data['ev_i'], m, n)
    t0 = time.perf_counter()
    dev.cnet_set_pairs(m, n, up, ui, ip, iu)
    pairs_s = time.perf_counter() - t0
    walks = dev.cnet_walks(T, L, seed)
    walks_ms = dev.get_option('cnet_last_ns') / 1e6
    row = {'shape': name, 'm': m, 'n': n, 'd': d, 'nnz': int(up[-1]), 'T': T, 'L': L, 'dim': dim, 'window': window, 'K': K,
           'epochs': epochs, 'walks': int(len(walks)), 'set_pairs_wall_s': pairs_s, 'walks_ms': walks_ms}
    if m <= 2000:                                                      # the contract, where it is quick
        row['walks_equal_contract'] = bool(np.array_equal(walks, cn.walks(cn.Net(up, ui, ip, iu), T, L, seed)))
    dev.cnet_embed(dim, window, epochs, seed)
    row['embed_ms'] = dev.get_option('cnet_last_ns') / 1e6
    row['embed_words_per_s'] = len(walks) * L * epochs / (row['embed_ms'] / 1e3)
    if m <= friends_cap:
        dev.cnet_friends(K)
        row['friends_ms'] = dev.get_option('cnet_last_ns') / 1e6
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--shapes', default='c1,c2')
    ap.add_argument('--epochs', type=int, default=10)
    ap.add_argument('--friends-cap', type=int, default=20000)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    dev = Device(0, raise_errors=True)
    rows = []
    for name in args.shapes.split(','):
        row = run(dev, name, args.epochs, args.friends_cap)
        print(json.dumps(row), flush=True)
        rows.append(row)
    if args.out:
        json.dump(rows, open(args.out, 'w'), indent=1)
    dev.close()


if __name__ == '__main__':
    main()
