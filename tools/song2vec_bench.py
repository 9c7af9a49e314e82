#!/usr/bin/env python3
"""Song2vec on one MI355X, on the C1-size golden log (tests/golden/g16_song2vec_c1_k20: 1000 x 1000, 16 training events per
user, k 20, K 10): levels of both schedules, the share of steps in levels of fewer than 256 steps, device time per iteration
under s2v_schedule 1 (levels) and 0 (one wave walks all steps), embedding and similar-tracks time from cnet_last_ns -- next to
the reference's own seconds recorded in the golden.  One JSON line.

    python tools/song2vec_bench.py [--iters 3] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from helpers import numpy_song2vec as ns       # noqa: E402
from test_song2vec_golden import load          # noqa: E402
from yue_amd._shim import Device               # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    z, st, meta, ev_ptr, ev_i, steps, pairs, h = load('c1_k20')
    m, n, k, K = int(z['m']), int(z['n']), int(z['k']), int(z['K'])
    dev = Device(0, raise_errors=True)
    users, sents = ns.sentences(ev_ptr, ev_i)
    ptr = np.concatenate([[0], np.cumsum([len(s) for s in sents])]).astype(np.int64)
    dev.cnet_set_sentences(n, ptr, np.concatenate(sents))
    dev.cnet_embed(k, 5, 10, 1)
    row = {'m': m, 'n': n, 'k': k, 'K': K, 'steps': int(len(steps[0])), 'pairs': int(len(pairs[0])), 'words': int(ptr[-1]),
           'embed_ms': dev.get_option('cnet_last_ns') / 1e6}
    dev.cnet_friends(K)
    row['friends_ms'] = dev.get_option('cnet_last_ns') / 1e6
    lv_s, lv_p = ns.levels(steps[0], steps[1]), ns.levels(pairs[0], pairs[1], shared=True)
    small = lambda lv: float(np.isin(lv, np.flatnonzero(np.bincount(lv) < 256)).mean())      # noqa: E731
    row.update({'levels_steps': int(lv_s.max()) + 1, 'levels_pairs': int(lv_p.max()) + 1,
                'share_steps_in_small_levels': small(lv_s), 'share_pairs_in_small_levels': small(lv_p)})
    for schedule in (1, 0):
        dev.set_option('s2v_schedule', schedule)
        X, Y, Bu, Bi = ns.init_from_seed(int(z['seed']), m, n, k)
        dev.set_factors(X, Y)
        dev.s2v_set_state(Bu, Bi)
        dev.s2v_set_steps(*steps)
        dev.s2v_set_pairs(*pairs)
        ms = []
        for _ in range(args.iters):
            dev.s2v_epoch(h['lRate'], h['regU'], h['regI'], h['regB'], h['alpha'], 0.0)
            ms.append(dev.get_option('s2v_last_ns') / 1e6)
        row['iteration_ms_schedule_%d' % schedule] = ms
    row['reference_seconds'] = meta['reference_seconds']
    print(json.dumps(row), flush=True)
    if args.out:
        json.dump(row, open(args.out, 'w'), indent=1)
    dev.close()


if __name__ == '__main__':
    main()
