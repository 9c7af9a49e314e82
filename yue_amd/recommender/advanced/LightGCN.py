#coding:utf8
"""LightGCN (embeddings propagated over the user-item graph, pairwise loss, Adam) behind the reference's plugin hooks.

Replaces the TensorFlow-1 graph of the reference's recommender/advanced/LightGCN.py with the device calls yue_lgcn_*
(include/yue_hip.h).  PARITY UNPINNED: TensorFlow cannot be installed here and the reference's
base/DeepRecommender.py is missing; what that class must provide is taken from the one TF set-up the reference holds
(recommender/cf/BPR.py:93-101).  What is kept:
  set-up      U [m,k], V [n,k] = truncated_normal(stddev 0.005), U drawn first; ``batch_size`` from the config key   (BPR.py:93-98)
  graph       every training event adds (u, m + i) and (m + i, u) with the pair's event count c; repeated indices are
              summed by the matmul, so a pair weighs c * c; no degree normalisation                                   (:20-34)
  layers      3; E_l = A E_{l-1} unnormalised, F = E_0 + sum_l l2_normalize(E_l)                                       (:36-45)
  batches     events in order in slices of batch_size, the last one short; 5 negatives per event by random.randint with
              rejection, of which the LAST is kept: one triplet per event                                             (:56-79)
  loss        -sum log sigmoid(y) + regU * (the three l2_loss terms), Adam(lRate); printed as
              ``training: <iter> batch <n> loss: <l>``                                                                (:83-100)
  predict     F_items . F_u after one final propagation, through the base class's scoring path                        (:54, 102-106)
The reference's branch for users outside the training set names undefined variables and cannot run; such users get what
the base class does for them.  ``lightgcn.hip=-layers L -neg N`` overrides the two constants; ``bpr.hip=-gpu N`` selects the
device as for BPR.  Data comes from the text log: the sampler walks ``data.trainingData``, which the reference's Record assigns
before a ``-byTime`` split, so under ``-byTime`` the graph and the batches hold every event of the log (kept).
"""
import random

import numpy as np

from ...base.IterativeRecommender import IterativeRecommender
from ...data.arrays import ArrayRecord
from ...tool.config import LineConfig
from ..cf.BPR import _truncated_normal


class LightGCN(IterativeRecommender):

    def __init__(self, conf, trainingSet=None, testSet=None, fold='[1]'):
        super(LightGCN, self).__init__(conf, trainingSet, testSet, fold)

    def readConfiguration(self):
        super(LightGCN, self).readConfiguration()
        self.batch_size = int(self.config['batch_size'])
        self.n_layers, self.negativeCount = 3, 5
        if self.config.contains('lightgcn.hip'):
            given = LineConfig(self.config['lightgcn.hip'])
            if given.contains('-layers'):
                self.n_layers = int(given['-layers'])
            if given.contains('-neg'):
                self.negativeCount = int(given['-neg'])
        if self.n_layers < 1 or self.negativeCount < 1 or self.batch_size < 1:
            print('LightGCN: -layers, -neg and batch_size must be at least 1')
            exit(-1)

    def initModel(self):
        if isinstance(self.data, ArrayRecord):
            print('LightGCN samples from the text log\'s training events; array-native data is not supported')
            exit(-1)
        super(LightGCN, self).initModel()
        self.m = self.data.getSize('user')
        self.n = self.data.getSize(self.recType)
        self.train_size = len(self.data.trainingData)
        self.U = _truncated_normal((self.m, self.k), 0.005)
        self.V = _truncated_normal((self.n, self.k), 0.005)
        rt = self.recType
        self.userListen = {}
        for entry in self.data.trainingData:                         # :20-24
            row = self.userListen.setdefault(entry['user'], {})
            row[entry[rt]] = row.get(entry[rt], 0) + 1
        print('training...')

    def _graph(self):
        """Sorted unique (user, item) pairs of both sides with the weight c * c."""
        d, rt = self.data, self.recType
        pu, pi, w = [], [], []
        for user, row in self.userListen.items():
            for item, c in row.items():
                pu.append(d.getId(user, 'user')); pi.append(d.getId(item, rt)); w.append(float(c) * float(c))
        pu, pi, w = np.asarray(pu, np.int64), np.asarray(pi, np.int64), np.asarray(w, np.float32)
        a, b = np.lexsort((pi, pu)), np.lexsort((pu, pi))
        u_ptr = np.concatenate([[0], np.cumsum(np.bincount(pu, minlength=self.m))]).astype(np.int64)
        i_ptr = np.concatenate([[0], np.cumsum(np.bincount(pi, minlength=self.n))]).astype(np.int64)
        return u_ptr, pi[a].astype(np.int32), w[a], i_ptr, pu[b].astype(np.int32), w[b]

    def next_batch_pairwise(self):
        d, rt, train = self.data, self.recType, self.data.trainingData
        names = d.id2name[rt]
        batch_id = 0
        while batch_id < self.train_size:
            end = min(batch_id + self.batch_size, self.train_size)
            u_idx, i_idx, j_idx = [], [], []
            for idx in range(batch_id, end):
                user = train[idx]['user']
                mine = self.userListen[user]
                for _ in range(self.negativeCount):
                    item_j = random.randint(0, self.n - 1)
                    while names[item_j] in mine:
                        item_j = random.randint(0, self.n - 1)
                u_idx.append(d.getId(user, 'user'))
                i_idx.append(d.getId(train[idx][rt], rt))
                j_idx.append(item_j)                                 # the appends sit outside the loop over negatives (:75-77)
            batch_id = end
            yield u_idx, i_idx, j_idx

    def buildModel(self):
        dev = self._device()
        dev.set_factors(self.U, self.V)
        dev.lgcn_set_graph(self.m, self.n, *self._graph())
        dev.adam_reset()
        step = 0
        for iteration in range(self.maxIter):
            for n, batch in enumerate(self.next_batch_pairwise()):
                user_idx, i_idx, j_idx = batch
                step += 1
                l = dev.lgcn_step(self.n_layers, user_idx, i_idx, j_idx, self.lRate, self.regU, step)
                self.loss = l
                print('training:', iteration + 1, 'batch', n, 'loss:', l)
        self.U, self.V = dev.get_factors()
        F = dev.lgcn_propagate(self.n_layers)                        # the final propagation: what self.test reads (:54)
        self.P, self.Q = np.ascontiguousarray(F[:self.m]), np.ascontiguousarray(F[self.m:])
        self._sync_factors_to_device()                               # the scoring path ranks with P = F_users, Q = F_items

    # ---- model file -----------------------------------------------------------------------
    def saveModel(self):
        out = self.output['-dir'] if hasattr(self, 'output') else './'
        np.savez(out + self.config['recommender'] + self.foldInfo + '-factors.npz', P=self.P, Q=self.Q, U=self.U, V=self.V)

    def loadModel(self):
        out = self.output['-dir'] if hasattr(self, 'output') else './'
        with np.load(out + self.config['recommender'] + self.foldInfo + '-factors.npz', allow_pickle=False) as z:
            self.P, self.Q, self.U, self.V = z['P'], z['Q'], z['U'], z['V']
        self._device_factors_current = False
