#!/usr/bin/env python3
"""Generate tests/golden/g18_ngcf_* by running the plain-Python parts of the REFERENCE's own NGCF class
(recommender/advanced/NGCF.py): the graph's index / value lists (:62-71) and the sampler next_batch (:16-41).

Only runs where the reference tree exists (tools/make_goldens.py is imported, which puts it on sys.path).  Nothing from the
reference is copied: the fixtures are inputs (a small seeded log with repeated pairs, seeds, batch_size) and what the class
computes from them.

How the class is loaded: ``tensorflow`` is a module object whose functions return an inert value that can be added to itself,
except that SparseTensor records its ``indices`` and ``values`` and split returns a pair; ``base.DeepRecommender`` (missing from
the reference) is a module object whose class provides what recommender/cf/BPR.py:93-101 shows such a base must: m, n, k,
train_size, batch_size, U, V, u_idx, v_idx.  The data object is the small class below (trainingData, userRecord, trackRecord as
lists of records, getId by first appearance).
Log a has m <= n, repeated pairs and a user id >= some track ids; log b has a user id >= n, so that its recorded indices show the
out-of-range row that the plugin refuses.  The tool asserts that the CPU contract (tests/helpers/numpy_ngcf.py) reproduces lists
and batches before it writes.
"""
import json
import os
import random
import sys
import types
from collections import defaultdict

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'tests'))

import make_goldens as mg                                       # noqa: E402,F401  (puts the reference on sys.path)
from helpers import numpy_ngcf as ng                            # noqa: E402

SEED = 20260018
GOLDEN = os.path.join(os.path.dirname(HERE), 'tests', 'golden')
RECORDED = {}


class Inert(object):
    """What every stand-in function returns: it adds to itself and can be called."""
    def __add__(self, other):
        return self

    def __call__(self, *a, **k):
        return self


class SparseTensor(Inert):
    def __init__(self, indices, values, dense_shape):
        RECORDED['indices'], RECORDED['values'], RECORDED['dense_shape'] = indices, values, dense_shape


def install_stand_ins():
    tf = types.ModuleType('tensorflow')
    inert = lambda *a, **k: Inert()                             # noqa: E731
    for name in ('concat', 'sparse_tensor_dense_matmul', 'matmul', 'reduce_sum', 'placeholder', 'multiply', 'set_random_seed', 'cast', 'Variable',
                 'cond'):
        setattr(tf, name, inert)
    tf.split = lambda *a, **k: (Inert(), Inert())
    tf.SparseTensor = SparseTensor
    tf.int32, tf.bool = 'int32', 'bool'
    tf.nn = types.SimpleNamespace(l2_normalize=inert, embedding_lookup=inert, leaky_relu=inert, dropout=inert)
    tf.contrib = types.SimpleNamespace(layers=types.SimpleNamespace(xavier_initializer=inert))
    sys.modules['tensorflow'] = tf

    class DeepRecommender(object):
        def __init__(self, conf, trainingSet=None, testSet=None, fold='[1]'):
            self.config, self.data = conf, trainingSet

        def initModel(self):
            self.m, self.n = len(self.data.id2name['user']), len(self.data.id2name['track'])
            self.k = int(self.config['num.factors'])
            self.train_size = len(self.data.trainingData)
            self.batch_size = int(self.config['batch_size'])
            self.U = self.V = self.u_idx = self.v_idx = Inert()

    mod = types.ModuleType('base.DeepRecommender')
    mod.DeepRecommender = DeepRecommender
    import base                                                 # the reference's package
    sys.modules['base.DeepRecommender'] = mod
    base.DeepRecommender = mod


class Data(object):
    def __init__(self, events):
        self.trainingData = [{'user': u, 'track': t} for u, t in events]
        self.name2id, self.id2name = {'user': {}, 'track': {}}, {'user': {}, 'track': {}}
        self.userRecord, self.trackRecord = defaultdict(list), defaultdict(list)
        for e in self.trainingData:
            for kind in ('user', 'track'):
                if e[kind] not in self.name2id[kind]:
                    self.name2id[kind][e[kind]] = len(self.name2id[kind])
                    self.id2name[kind][self.name2id[kind][e[kind]]] = e[kind]
            self.userRecord[e['user']].append(e)
            self.trackRecord[e['track']].append(e)

    def getId(self, obj, t):
        return self.name2id[t][obj]


def events_for(seed, m, n, E):
    """A log in which popular pairs repeat (not adjacent), every user occurs and min(m, n) tracks at least."""
    rng = np.random.RandomState(seed)
    ev = [('u%d' % int(m * rng.rand() ** 1.5), 't%d' % int(n * rng.rand() ** 2)) for _ in range(E)]
    ev += [('u%d' % u, 't%d' % (u % n)) for u in range(m)]
    return ev


def case(tag, m, n, E, batch_size, sampler_seed):
    import recommender.advanced.NGCF as ref
    data = Data(events_for(SEED + len(tag) + ord(tag[0]), m, n, E))
    rec = ref.NGCF({'batch_size': str(batch_size), 'num.factors': '8'}, data)
    rec.initModel()
    random.seed(sampler_seed)
    batches = [[list(map(int, x)) for x in b] for b in rec.next_batch()]
    ev_u = [data.getId(e['user'], 'user') for e in data.trainingData]
    ev_t = [data.getId(e['track'], 'track') for e in data.trainingData]
    keys = [data.getId(t, 'track') for t in data.trackRecord.keys()]
    out = {'m': rec.m, 'n': rec.n, 'batch_size': batch_size, 'sampler_seed': sampler_seed, 'layers': rec.n_layers, 'ev_u': ev_u, 'ev_t': ev_t,
           'track_keys': keys, 'indices': [list(map(int, x)) for x in RECORDED['indices']], 'values': [float(v) for v in RECORDED['values']],
           'dense_shape': list(map(int, RECORDED['dense_shape'])), 'batches': batches}
    # the contract reproduces both before anything is written
    g = ng.graph_from_events(ev_u, ev_t, rec.m, rec.n, 'written')
    assert g['indices'] == out['indices'] and g['values'] == out['values']
    random.seed(sampler_seed)
    assert [list(b) for b in ng.next_batch(ev_u, ev_t, keys, batch_size, random)] == batches
    mine = defaultdict(set)
    for u, t in zip(ev_u, ev_t):
        mine[u].add(t)
    hits = sum(j in mine[u] for b in batches for u, j in zip(b[0], b[2]))
    assert hits > 0 and len(set(zip(ev_u, ev_t))) < len(ev_u) and len(batches[-1][0]) < batch_size
    out['out_of_range_rows'] = g['out_of_range']
    assert bool(g['out_of_range']) == (max(ev_u) >= rec.n)
    json.dump(out, open(os.path.join(GOLDEN, 'g18_ngcf_%s.json' % tag), 'w'), separators=(',', ':'))
    print(tag, 'm', rec.m, 'n', rec.n, 'events', len(ev_u), 'batches', [len(b[0]) for b in batches], 'negatives the user listened to', hits,
          'rows out of range', g['out_of_range'])


if __name__ == '__main__':
    install_stand_ins()
    case('a', 12, 30, 100, 32, 7)
    case('b', 40, 25, 300, 128, 11)
