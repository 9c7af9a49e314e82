#!/usr/bin/env python3
"""Generate tests/golden/g21_apr_* from the APR contract tests/helpers/numpy_apr.py.

The reference (recommender/advanced/APR.py) cannot be executed here: it needs TensorFlow.  These goldens therefore pin the CONTRACT,
not TensorFlow: a later change to the contract's formulas, its update rule or its sampler shows up as a changed loss, checksum or
batch.  Per case (tests/helpers/apr_cases.py): the two fp64 losses, a checksum (sum and sum of absolute values) of the parameter
gradients of both forms, of the raw perturbation gradients and of the new perturbation, the same of the factors after three phase-1
and three adversarial fp64 steps with the six losses, and the case's d32 figures.  Beside them a fixed log with its seeds, and the
triplets the contract's sampler (:95-111 restated on ids) draws from it.
"""
import json
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'tests'))

from helpers import apr_cases as ac                             # noqa: E402
from helpers import numpy_apr as ap                             # noqa: E402

GOLDEN = os.path.join(os.path.dirname(HERE), 'tests', 'golden')
GOLDEN_CASES = ('base', 'k50', 'k64', 'ieqj')
LR = 0.002


def checksum(a):
    a = np.asarray(a, np.float64)
    return [float(a.sum()), float(np.abs(a).sum())]


def trained(c):
    """(U, V, losses) of the fp64 contract over the case's six step batches."""
    return ap.train(c['U'], c['V'], ac.step_batches(c), 3, LR, ac.REG, c['eps'], c['regA'], np.float64)


def case_record(name):
    c = ac.build(name)
    out = {'name': name, 'seed': c['seed'], 'T': int(len(c['u'])), 'd32': c['d32']}
    for q in ac.QUANTITIES:
        out[q] = c['want'][q] if q.startswith('loss') else checksum(c['want'][q])
    U, V, losses = trained(c)
    out.update(U6=checksum(U), V6=checksum(V), losses6=losses)
    return out


def sampler_record(seed=20260021, m=9, n=14, E=60, batch_size=6, neg=3, np_seed=5, sampler_seed=7):
    rng = np.random.RandomState(seed)
    ev_u = [int(m * rng.rand() ** 1.5) for _ in range(E)]
    ev_t = [int(n * rng.rand() ** 2) for _ in range(E)]
    # ids by first appearance in the log, as the data layer assigns them
    uid, tid = {}, {}
    ev_u = [uid.setdefault(u, len(uid)) for u in ev_u]
    ev_t = [tid.setdefault(t, len(tid)) for t in ev_t]
    listened = {}
    for u, t in zip(ev_u, ev_t):
        listened.setdefault(u, set()).add(t)
    np_rng = np.random.RandomState(np_seed)
    random.seed(sampler_seed)
    batches = [[list(map(int, x)) for x in ap.next_batch(ev_u, ev_t, listened, len(tid), batch_size, neg, np_rng, random)] for _ in range(2)]
    assert all(len(b[0]) == neg * batch_size and all(j not in listened[u] for u, j in zip(b[0], b[2])) for b in batches)
    return {'m': len(uid), 'n': len(tid), 'ev_u': ev_u, 'ev_t': ev_t, 'batch_size': batch_size, 'neg': neg, 'np_seed': np_seed, 'sampler_seed': sampler_seed,
            'batches': batches}


if __name__ == '__main__':
    for name in GOLDEN_CASES:
        rec = case_record(name)
        json.dump(rec, open(os.path.join(GOLDEN, 'g21_apr_%s.json' % name), 'w'), separators=(',', ':'))
        print(name, 'loss_pre', rec['loss_pre'], 'loss_adv', rec['loss_adv'], 'losses', rec['losses6'])
    rec = sampler_record()
    json.dump(rec, open(os.path.join(GOLDEN, 'g21_apr_sampler.json'), 'w'), separators=(',', ':'))
    print('sampler', rec['m'], rec['n'], [len(b[0]) for b in rec['batches']])
