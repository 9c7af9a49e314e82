#coding:utf8
"""NGCF (graph convolution with two k x k weights per layer, bi-interaction term, message dropout; pairwise loss, Adam) behind
the reference's plugin hooks.

Replaces the TensorFlow-1 graph of the reference's recommender/advanced/NGCF.py with the device calls yue_ngcf_*
(include/yue_hip.h).  PARITY UNPINNED: TensorFlow cannot be installed here and the reference's
base/DeepRecommender.py is missing; what that class must provide is taken from recommender/cf/BPR.py:93-101.  What is kept:
  set-up      U [m,k], V [n,k] = truncated_normal(stddev 0.005), U drawn first; then the six weights W_l_1, W_l_2 [k,k], Xavier
              uniform U(-sqrt(6 / 2k), +sqrt(6 / 2k)), drawn with NumPy in the order W_0_1, W_0_2, W_1_1, ...             (:77-88)
  counts      userListen[u][t] starts at 1 on first sight and is then incremented: a pair with c events holds c + 1      (:48-54)
  graph       every training event adds (u, m + t) and (m + u, t) -- the second block is not the transpose -- with the value
              (c + 1) / sqrt(len(userRecord[u])) / sqrt(len(trackRecord[t])) (0 where a length is 0); repeated indices are
              summed by the matmul, so a pair weighs c (c + 1) / sqrt(d_u) / sqrt(d_t), formed in Python doubles and rounded
              once to float32 (TensorFlow's c sequential float32 additions may differ in the last bits)                  (:62-73)
  layers      3; S = A E, Z = (S + E) W_1 + (E o S) W_2, leaky ReLU 0.2, dropout keep 0.9 in training, the dropped unnormalised
              rows carried on, F = [E_0 | l2_normalize(E_1) | ...]                                                       (:90-113)
  batches     events in order in slices of batch_size, the last one short; one negative per event by random.choice over
              list(trackRecord.keys()); the rejection test compares a track name with record dicts and is never true, so
              negatives are never rejected                                                                              (:16-41)
  loss        -sum log sigmoid(y) + regU * (the three l2_loss terms), Adam(lRate) on U, V and the weights; printed as
              ``training: <iter> batch <n> loss: <l>``                                                                  (:124-141)
  predict     F_items . F_u after one propagation without dropout, through the base class's scoring path                 (:120, 143-149)
As written, "item row" m + x of the graph gathers the tracks of the USER whose id is x, and a user id >= n names a row >= m + n,
which TensorFlow's CPU kernel refuses with a bounds error.  ``ngcf.hip=-graph written`` (the default) keeps the blocks as
written and stops with a message on such a log; ``-graph symmetric`` puts (m + t, u) in the second block, the formula of :64's
comment.  TensorFlow's dropout stream cannot be reproduced: the mask is the device's counter hash of (seed, step, layer, row,
column), seed from ``-seed`` (default 2, the reference's set_random_seed).  ``ngcf.hip=-layers L -keep P`` override the two
constants; (L + 1) k must not exceed 256, the widest factors the ranking scan takes.  ``bpr.hip=-gpu N`` selects the device.
"""
import math
import random

import numpy as np

from ...base.IterativeRecommender import IterativeRecommender
from ...data.arrays import ArrayRecord
from ...tool.config import LineConfig
from ..cf.BPR import _truncated_normal

MAX_WIDTH = 256


class NGCF(IterativeRecommender):

    def __init__(self, conf, trainingSet=None, testSet=None, fold='[1]'):
        super(NGCF, self).__init__(conf, trainingSet, testSet, fold)

    def readConfiguration(self):
        super(NGCF, self).readConfiguration()
        self.batch_size = int(self.config['batch_size'])
        self.n_layers, self.keep_prob, self.graph_form, self.mask_seed = 3, 0.9, 'written', 2
        if self.config.contains('ngcf.hip'):
            given = LineConfig(self.config['ngcf.hip'])
            if given.contains('-layers'):
                self.n_layers = int(given['-layers'])
            if given.contains('-keep'):
                self.keep_prob = float(given['-keep'])
            if given.contains('-graph'):
                self.graph_form = given['-graph']
            if given.contains('-seed'):
                self.mask_seed = int(given['-seed'])
        if self.n_layers < 1 or self.batch_size < 1 or not 0.0 < self.keep_prob <= 1.0:
            print('NGCF: -layers and batch_size must be at least 1, -keep in (0, 1]')
            exit(-1)
        if self.graph_form not in ('written', 'symmetric'):
            print('NGCF: -graph must be written or symmetric')
            exit(-1)
        if (self.n_layers + 1) * self.k > MAX_WIDTH:
            print('NGCF: (layers + 1) * num.factors = %d, but the ranking scan takes factors of width %d at the most'
                  % ((self.n_layers + 1) * self.k, MAX_WIDTH))
            exit(-1)

    def initModel(self):
        if isinstance(self.data, ArrayRecord):
            print('NGCF samples from the text log\'s training events; array-native data is not supported')
            exit(-1)
        super(NGCF, self).initModel()
        self.m = self.data.getSize('user')
        self.n = self.data.getSize(self.recType)
        self.train_size = len(self.data.trainingData)
        self.U = _truncated_normal((self.m, self.k), 0.005)
        self.V = _truncated_normal((self.n, self.k), 0.005)
        lim = math.sqrt(6.0 / (2 * self.k))
        self.W = np.random.uniform(-lim, lim, size=(self.n_layers, 2, self.k, self.k)).astype(np.float32)
        rt = self.recType
        self.userListen = {}
        for entry in self.data.trainingData:                         # :48-54
            row = self.userListen.setdefault(entry['user'], {})
            if entry[rt] not in row:
                row[entry[rt]] = 1
            row[entry[rt]] += 1
        self._graph_csr = self._graph()
        print('training...')

    def _graph(self):
        """(ptr, col, w) of the (m + n)-row graph: both blocks, columns ascending within a row."""
        d, rt, m, n = self.data, self.recType, self.m, self.n
        pu, pt, w = [], [], []
        for user, row in self.userListen.items():
            du = len(d.userRecord[user])
            for item, held in row.items():
                dt = len(d.trackRecord[item])                        # (a lookup that adds the key, as the reference's does, :67)
                c = held - 1
                value = 0.0 if du == 0 or dt == 0 else float(held) / math.sqrt(du) / math.sqrt(dt)
                pu.append(d.getId(user, 'user')); pt.append(d.getId(item, rt)); w.append(c * value)
        pu, pt, w = np.asarray(pu, np.int64), np.asarray(pt, np.int64), np.asarray(w, np.float64).astype(np.float32)
        if self.graph_form == 'written':
            if len(pu) and pu.max() >= n:
                print('NGCF: the graph as the reference writes it puts user %d\'s tracks in row m + %d, and the log has %d tracks only: '
                      'TensorFlow refuses such an index with a bounds error.  ngcf.hip=-graph symmetric builds the graph of the '
                      'reference\'s comment instead' % (int(pu.max()), int(pu.max()), n))
                exit(-1)
            rows, cols = np.concatenate([pu, m + pu]), np.concatenate([m + pt, pt])
        else:
            rows, cols = np.concatenate([pu, m + pt]), np.concatenate([m + pt, pu])
        ww = np.concatenate([w, w])
        o = np.lexsort((cols, rows))
        ptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=m + n))]).astype(np.int64)
        return ptr, cols[o].astype(np.int32), ww[o]

    def next_batch(self):
        d, rt, train = self.data, self.recType, self.data.trainingData
        batch_id = 0
        while batch_id < self.train_size:
            end = min(batch_id + self.batch_size, self.train_size)
            u_idx, i_idx, j_idx = [], [], []
            item_list = list(d.trackRecord.keys())                   # rebuilt per batch (:31)
            for idx in range(batch_id, end):
                u_idx.append(d.getId(train[idx]['user'], 'user'))
                i_idx.append(d.getId(train[idx][rt], rt))
                j_idx.append(d.getId(random.choice(item_list), rt))  # never rejected (:36-38)
            batch_id = end
            yield u_idx, i_idx, j_idx

    def buildModel(self):
        dev = self._device()
        dev.set_factors(self.U, self.V)
        dev.ngcf_set_graph(self.m, self.n, *self._graph_csr)
        dev.ngcf_set_weights(self.W)
        dev.adam_reset()
        step = 0
        for iteration in range(self.maxIter):
            for n, batch in enumerate(self.next_batch()):
                user_idx, i_idx, j_idx = batch
                step += 1
                l = dev.ngcf_step(self.n_layers, True, self.keep_prob, self.mask_seed, user_idx, i_idx, j_idx, self.lRate, self.regU, step)
                self.loss = l
                print('training:', iteration + 1, 'batch', n, 'loss:', l)
        self.U, self.V = dev.get_factors()
        self.W = dev.ngcf_get_weights()
        F = dev.ngcf_propagate(self.n_layers)                        # without dropout: what self.test reads (:120, :147)
        self.P, self.Q = np.ascontiguousarray(F[:self.m]), np.ascontiguousarray(F[self.m:])
        self._sync_factors_to_device()                               # the scoring path ranks with P = F_users, Q = F_items

    # ---- model file -----------------------------------------------------------------------
    def saveModel(self):
        out = self.output['-dir'] if hasattr(self, 'output') else './'
        np.savez(out + self.config['recommender'] + self.foldInfo + '-factors.npz', P=self.P, Q=self.Q, U=self.U, V=self.V, W=self.W)

    def loadModel(self):
        out = self.output['-dir'] if hasattr(self, 'output') else './'
        with np.load(out + self.config['recommender'] + self.foldInfo + '-factors.npz', allow_pickle=False) as z:
            self.P, self.Q, self.U, self.V, self.W = z['P'], z['Q'], z['U'], z['V'], z['W']
        self._device_factors_current = False
