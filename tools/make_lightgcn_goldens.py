#!/usr/bin/env python3
"""Generate tests/golden/g17_lightgcn_* by running the plain-Python parts of the REFERENCE's own LightGCN class
(recommender/advanced/LightGCN.py): the graph's index / value lists (:29-32) and the sampler next_batch_pairwise (:56-79).

Only runs where the reference tree exists (tools/make_goldens.py is imported, which puts it on sys.path).  Nothing from the
reference is copied: the fixtures are inputs (a small seeded log with repeated pairs, seeds, batch_size) and what the class
computes from them.

How the class is loaded: ``tensorflow`` is a module object whose functions return None, except that SparseTensor records its
``indices`` and ``values`` and split returns a pair; ``base.DeepRecommender`` (missing from the reference) is a module object
whose class provides what recommender/cf/BPR.py:93-101 shows such a base must: m, n, train_size, batch_size, U, V, u_idx,
v_idx.  The data object is the small class below (trainingData, getId, id2name / name2id by first appearance).
The tool asserts that the CPU contract (tests/helpers/numpy_lightgcn.py) reproduces lists and batches before it writes.
"""
import json
import os
import random
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'tests'))

import make_goldens as mg                                       # noqa: E402,F401  (puts the reference on sys.path)
from helpers import numpy_lightgcn as nl                        # noqa: E402

SEED = 20260017
GOLDEN = os.path.join(os.path.dirname(HERE), 'tests', 'golden')
RECORDED = {}


class SparseTensor(object):
    def __init__(self, indices, values, dense_shape):
        RECORDED['indices'], RECORDED['values'], RECORDED['dense_shape'] = indices, values, dense_shape


def install_stand_ins():
    tf = types.ModuleType('tensorflow')
    nothing = lambda *a, **k: None                              # noqa: E731
    for name in ('concat', 'sparse_tensor_dense_matmul', 'reduce_sum', 'placeholder', 'multiply', 'set_random_seed'):
        setattr(tf, name, nothing)
    tf.split = lambda *a, **k: (None, None)
    tf.SparseTensor = SparseTensor
    tf.int32 = 'int32'
    tf.nn = types.SimpleNamespace(l2_normalize=nothing, embedding_lookup=nothing)
    sys.modules['tensorflow'] = tf

    class DeepRecommender(object):
        def __init__(self, conf, trainingSet=None, testSet=None, fold='[1]'):
            self.config, self.data = conf, trainingSet

        def initModel(self):
            self.m, self.n = len(self.data.id2name['user']), len(self.data.id2name['track'])
            self.train_size = len(self.data.trainingData)
            self.batch_size = int(self.config['batch_size'])
            self.U = self.V = self.u_idx = self.v_idx = None

    mod = types.ModuleType('base.DeepRecommender')
    mod.DeepRecommender = DeepRecommender
    import base                                                 # the reference's package
    sys.modules['base.DeepRecommender'] = mod
    base.DeepRecommender = mod


class Data(object):
    def __init__(self, events):
        self.trainingData = [{'user': u, 'track': t} for u, t in events]
        self.name2id, self.id2name = {'user': {}, 'track': {}}, {'user': {}, 'track': {}}
        for e in self.trainingData:
            for kind in ('user', 'track'):
                if e[kind] not in self.name2id[kind]:
                    self.name2id[kind][e[kind]] = len(self.name2id[kind])
                    self.id2name[kind][self.name2id[kind][e[kind]]] = e[kind]

    def getId(self, obj, t):
        return self.name2id[t][obj]


def events_for(seed, m, n, E):
    """A log in which popular pairs repeat: the same (user, track) up to several times, not adjacent."""
    rng = np.random.RandomState(seed)
    ev = [('u%d' % int(m * rng.rand() ** 1.5), 't%d' % int(n * rng.rand() ** 2)) for _ in range(E)]
    ev += [('u%d' % u, 't%d' % u) for u in range(m)]           # every user and at least m tracks occur
    return ev


def case(tag, m, n, E, batch_size, sampler_seed):
    import recommender.advanced.LightGCN as lg
    data = Data(events_for(SEED + len(tag), m, n, E))
    rec = lg.LightGCN({'batch_size': str(batch_size)}, data)
    rec.initModel()
    random.seed(sampler_seed)
    batches = [[list(map(int, x)) for x in b] for b in rec.next_batch_pairwise()]
    ev_u = [data.getId(e['user'], 'user') for e in data.trainingData]
    ev_i = [data.getId(e['track'], 'track') for e in data.trainingData]
    out = {'m': rec.m, 'n': rec.n, 'batch_size': batch_size, 'sampler_seed': sampler_seed, 'negatives': rec.negativeCount, 'layers': rec.n_layers,
           'ev_u': ev_u, 'ev_i': ev_i, 'indices': [list(map(int, x)) for x in RECORDED['indices']], 'values': [float(v) for v in RECORDED['values']],
           'dense_shape': list(map(int, RECORDED['dense_shape'])), 'batches': batches}
    # the contract reproduces both before anything is written
    g = nl.graph_from_events(ev_u, ev_i, rec.m, rec.n)
    assert g['indices'] == out['indices'] and g['values'] == out['values']
    listened = {}
    for u, i in zip(ev_u, ev_i):
        listened.setdefault(u, set()).add(i)
    random.seed(sampler_seed)
    assert [list(b) for b in nl.next_batch_pairwise(ev_u, ev_i, listened, rec.n, batch_size, rec.negativeCount, random)] == batches
    assert max(out['values']) > 1 and len(batches[-1][0]) < batch_size and all(len(b[0]) == len(b[2]) for b in batches)
    json.dump(out, open(os.path.join(GOLDEN, 'g17_lightgcn_%s.json' % tag), 'w'), separators=(',', ':'))
    print(tag, 'm', rec.m, 'n', rec.n, 'events', len(ev_u), 'batches', [len(b[0]) for b in batches], 'max count', max(out['values']))


if __name__ == '__main__':
    install_stand_ins()
    case('a', 12, 30, 100, 32, 7)
    case('b', 40, 25, 300, 128, 11)
