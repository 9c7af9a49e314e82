#!/usr/bin/env python3
"""Generate tests/golden/g20_cdae_* from the CDAE contract tests/helpers/numpy_cdae.py.

The reference (recommender/advanced/CDAE.py) cannot be executed here: it needs TensorFlow.  These goldens therefore pin the
CONTRACT, not TensorFlow: a later change to the contract's formulas, its mask or its sampler shows up as a changed loss, checksum or
batch.  Per case (tests/helpers/cdae_cases.py): the fp64 loss, the float32 loss, a checksum (sum and sum of absolute values) of hid,
of the sampled logits and of each of the five fp64 gradients, the number of kept input entries, and the case's d32 figures.  Beside
them a fixed log with its seed, and the users and sample sets the contract's sampler (:76-98 restated on ids) draws from it.
"""
import json
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'tests'))

from helpers import cdae_cases as cc                            # noqa: E402
from helpers import numpy_cdae as cd                            # noqa: E402

GOLDEN = os.path.join(os.path.dirname(HERE), 'tests', 'golden')
GOLDEN_CASES = ('h33', 'twice', 'low', 'keep01')


def checksum(a):
    a = np.asarray(a, np.float64)
    return [float(a.sum()), float(np.abs(a).sum())]


def case_record(name):
    c = cc.build(name)
    out = {'name': name, 'seed': c['seed'], 'loss': c['loss'], 'loss32': c['loss32'], 'kept': int(sum(int(f.sum()) for f in c['fw']['flags'])),
           'entries': int(c['sptr'][-1]), 'hid': checksum(c['fw']['hid']), 'logit': checksum(c['fw']['logit']), 'd32': c['d32']}
    for k in cd.NAMES:
        out['g' + k] = checksum(c['g'][k])
    return out


def sampler_record(seed=20260020, m=9, n=14, E=60, batch_size=6, neg=5, sampler_seed=7):
    rng = np.random.RandomState(seed)
    ev_u = [int(m * rng.rand() ** 1.5) for _ in range(E)]
    ev_t = [int(n * rng.rand() ** 2) for _ in range(E)]
    # ids by first appearance in the log, as the data layer assigns them
    uid, tid = {}, {}
    ev_u = [uid.setdefault(u, len(uid)) for u in ev_u]
    ev_t = [tid.setdefault(t, len(tid)) for t in ev_t]
    data = cd.user_csr(ev_u, ev_t, len(uid))
    random.seed(sampler_seed)
    batches = []
    for _ in range(2):
        users, sets = cd.next_batch(list(range(len(uid))), list(range(len(tid))), data, batch_size, neg, random)
        batches.append([users, [sorted(s) for s in sets]])
    mine = {}
    for u, t in zip(ev_u, ev_t):
        mine.setdefault(u, set()).add(t)
    assert all(mine[u] <= set(s) for users, sets in batches for u, s in zip(users, sets))
    assert any(len(s) < 6 * len(mine[u]) for users, sets in batches for u, s in zip(users, sets))        # a negative repeats or is a positive
    assert len(set(zip(ev_u, ev_t))) < len(ev_u)
    return {'m': len(uid), 'n': len(tid), 'ev_u': ev_u, 'ev_t': ev_t, 'batch_size': batch_size, 'neg': neg, 'sampler_seed': sampler_seed, 'batches': batches}


if __name__ == '__main__':
    for name in GOLDEN_CASES:
        rec = case_record(name)
        json.dump(rec, open(os.path.join(GOLDEN, 'g20_cdae_%s.json' % name), 'w'), separators=(',', ':'))
        print(name, 'loss', rec['loss'], 'kept', rec['kept'], 'entries', rec['entries'])
    rec = sampler_record()
    json.dump(rec, open(os.path.join(GOLDEN, 'g20_cdae_sampler.json'), 'w'), separators=(',', ':'))
    print('sampler', rec['m'], rec['n'], [len(b[0]) for b in rec['batches']])
