#coding:utf8
"""APR (Adversarial Personalized Ranking: BPR's live minibatch path plus a loss at perturbed embeddings) behind the reference's
plugin hooks.

Replaces the TensorFlow-1 graph of the reference's recommender/advanced/APR.py with the device calls yue_apr_*
(include/yue_apr.h).  PARITY UNPINNED: TensorFlow cannot be installed here and the reference's
base/DeepRecommender is not importable; what that class must provide is taken from the one TF set-up the reference holds
(recommender/cf/BPR.py:93-101).  What is kept (line numbers are APR.py's):
  set-up      U [m,k], V [n,k] = truncated_normal(stddev 0.005), U drawn first; ``batch_size`` from the config key; regU from
              ``reg.lambda``; ``APR=-eps E -regA A -advEpoch N``; 3 negatives per event                                   (:17-23)
  batches     batch_size events by np.random.randint over data.trainingData, then per event 3 negatives by random.randint,
              drawn again while the track is one the user has in userRecord; one triplet per negative                     (:95-111)
  phase 1     num.max.iter steps of Adam(lRate) on sum softplus(-x) + regU (2 l2_loss(U_e) + l2_loss(V_e)): the user rows are
              regularised twice, the negative rows never, regU serves all terms                                       (:61-67, 120-127)
  phase 2     -advEpoch steps: the perturbation becomes eps * l2_normalize of the batch's gradient with respect to it, taken at
              the previous perturbation; then one Adam step on sum softplus(-x) + regA sum softplus(-x_adv), without an l2 term,
              by the SAME optimizer (``optimizer_adv`` is never used): moments and step count run on                  (:49-58, 69-76, 129-137)
  per step    ``iteration: <e> loss: <l>`` (e starts over at 0 in phase 2), the factors copied to P and Q, ranking_performance()
  ranking     the base class's predict on P and Q: ``predictForRanking`` is never called and names attributes APR never sets
``apr.hip=-neg N`` overrides the 3 negatives; ``bpr.hip=-gpu N`` selects the device as for BPR.  Data comes from the text log: the
sampler walks ``data.trainingData``, which the reference's Record assigns before a ``-byTime`` split, so under ``-byTime`` the
batches hold every event of the log (kept) while the rejection sees the training side only.
"""
import random

import numpy as np

from ...base.IterativeRecommender import IterativeRecommender
from ...data.arrays import ArrayRecord
from ...tool.config import LineConfig
from ..cf.BPR import _truncated_normal


class APR(IterativeRecommender):

    def __init__(self, conf, trainingSet=None, testSet=None, fold='[1]'):
        super(APR, self).__init__(conf, trainingSet, testSet, fold)

    def readConfiguration(self):
        super(APR, self).readConfiguration()
        self.batch_size = int(self.config['batch_size'])
        args = LineConfig(self.config['APR'])
        try:
            self.eps = float(args['-eps'])
            self.regAdv = float(args['-regA'])
            self.advEpoch = int(args['-advEpoch'])
        except ValueError:                                           # (the line parser reads a leading minus as the next option)
            print('APR: -eps, -regA and -advEpoch each need a number that is not negative')
            exit(-1)
        self.negativeCount = 3
        if self.config.contains('apr.hip'):
            given = LineConfig(self.config['apr.hip'])
            if given.contains('-neg'):
                self.negativeCount = int(given['-neg'])
        if self.batch_size < 1 or self.negativeCount < 1 or self.advEpoch < 0:
            print('APR: batch_size and -neg must be at least 1, -advEpoch at least 0')
            exit(-1)
        if not self.eps >= 0 or not self.regAdv >= 0:
            print('APR: -eps and -regA must not be negative')
            exit(-1)

    def initModel(self):
        if isinstance(self.data, ArrayRecord):
            print('APR samples from the text log\'s training events; array-native data is not supported')
            exit(-1)
        super(APR, self).initModel()
        self.m = self.data.getSize('user')
        self.n = self.data.getSize(self.recType)
        self.train_size = len(self.data.trainingData)
        self.U = _truncated_normal((self.m, self.k), 0.005)
        self.V = _truncated_normal((self.n, self.k), 0.005)
        rt = self.recType
        self.userListen = {}
        for user in self.data.userRecord:                            # :81-86 (the counts are never read)
            row = self.userListen.setdefault(user, {})
            for item in self.data.userRecord[user]:
                row[item[rt]] = row.get(item[rt], 1) + 1
        print('training...')

    def next_batch(self):
        d, rt, train = self.data, self.recType, self.data.trainingData
        names = d.id2name[rt]
        batch_idx = np.random.randint(self.train_size, size=self.batch_size)
        user_idx, item_idx, neg_item_idx = [], [], []
        for idx in batch_idx:
            user = train[idx]['user']
            mine = self.userListen.get(user, ())
            for _ in range(self.negativeCount):
                item_j = random.randint(0, self.n - 1)
                while names[item_j] in mine:
                    item_j = random.randint(0, self.n - 1)
                user_idx.append(d.getId(user, 'user'))
                item_idx.append(d.getId(train[idx][rt], rt))
                neg_item_idx.append(item_j)
        return user_idx, item_idx, neg_item_idx

    def _after_step(self, epoch, loss):
        print('iteration:', epoch, 'loss:', loss)
        self.loss = loss
        self.dev.get_factors(self.P, self.Q)                         # :125-126
        self._device_factors_current = True
        self.ranking_performance()

    def buildModel(self):
        print('training...')
        self.P, self.Q = self.U.copy(), self.V.copy()
        self._sync_factors_to_device()
        dev = self.dev
        dev.adam_reset()
        dev.apr_reset()
        step = 0
        for epoch in range(self.maxIter):
            user_idx, item_idx, neg_item_idx = self.next_batch()
            step += 1
            self._after_step(epoch, dev.apr_pre_step(user_idx, item_idx, neg_item_idx, self.lRate, self.regU, step))
        for epoch in range(self.advEpoch):                           # the optimizer of phase 1 goes on: step = maxIter + epoch + 1
            user_idx, item_idx, neg_item_idx = self.next_batch()
            step += 1
            self._after_step(epoch, dev.apr_adv_step(user_idx, item_idx, neg_item_idx, self.lRate, self.eps, self.regAdv, step))
        self.U, self.V = self.P, self.Q
