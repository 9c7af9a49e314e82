#coding:utf8
"""CDAE (collaborative denoising autoencoder: a user's corrupted listening row through one hidden layer with a per-user input
node, evaluated on sampled outputs; Adam) behind the reference's plugin hooks.

Replaces the TensorFlow-1 graph of the reference's recommender/advanced/CDAE.py with the device calls yue_cdae_*
(include/yue_hip.h).  PARITY UNPINNED: TensorFlow cannot be installed here.  What is kept:
  options     ``CDAE=-batch_size B -co p -nh H``; -nh is read and then overwritten, n_hidden = 128              (:16-21, :26)
  set-up      U [m,h] Xavier uniform with limit sqrt(6 / (m + h)); encoder W [n,h], decoder W' [h,n], biases b [h], b' [n] normal with
              stddev 1; drawn with NumPy in creation order U, W, W', b, b'                                       (:31-48)
  counts      userListen[uid][tid] starts at 1 and later events increment it: the pair's event count             (:50-57)
  input       a row of X holds those counts, not 0 / 1                                                            (:67-74)
  batch       B users by random.choice(userList), with replacement; per slot `sample` is 1 at the user's items and at
              5 len(items) draws of random.choice(itemList); the rejection test compares a track name with a list of record
              dicts and is never true, so a negative may be a positive or repeat; the order of the random calls   (:76-98)
  mask        an input entry is KEPT with probability -co (np.random.binomial(1, co)): the shipped 0.1 keeps a tenth (:124)
  forward     hid = sigmoid((X o mask) W + b + U[u]); dec = sigmoid(hid W' + b'); y_pred = max(1e-6, sample o dec);
              y_true = sample o X o mask                                                                   (:59-65, :101-107)
  loss        mean over [B, n] of the cross entropy + regU (l2_loss of W, W', b, b' and of the gathered rows of U: a user drawn
              twice counts twice); AdamOptimizer(lRate) on all five variables, dense on every row of U too       (:109-117)
  loop        num.max.iter minibatch steps, each printing ``<fold> Epoch: %04d loss= %.9f``; ``Optimization Finished!`` (:123-131)
Three things do not work as written:
  prediction  predictForRanking (:134-141) is never called (evalRanking calls predict), names self.v_idx, which does not exist,
              and leaves the mask placeholder unfed: as shipped the reference ranks with the base class's random P, Q.  Built here
              is what is meant: hid(u) from the uncorrupted row (a mask of ones), scores hid(u) . W'[:, i] + b'[i], as the factors
              P[u] = [hid(u) | 1], Q[i] = [W'[:, i] | b'[i]] of width h + 1 through the base class's scoring path.  The sigmoid is
              left off: it is monotone, so every comparison of the scan is the same except where two sigmoids round to one float.
  saturation  at stddev 1 the decoder's logits have a standard deviation near 7 and about 1 % of the outputs round to 1.0f:
              log(1 - y_pred) = -inf, and TensorFlow's first gradients are NaN.  The formula is kept; the device counts such
              outputs, reports the loss as inf and leaves parameters and moments untouched; this class prints the loss line
              and stops with a message.  ``cdae.hip=-stddev S`` (default 1.0, as written) draws W, W', b, b' at another stddev.
  streams     TensorFlow's and NumPy's random streams: the mask is the device's counter hash of (seed, step, slot, item), the same
              function on host and device, seed from ``cdae.hip=-seed`` (default 2, the reference's set_random_seed); two slots
              that hold the same user get different masks.
``cdae.hip=-nh H`` (1 <= H <= 128) is this project's override of n_hidden, ``-neg`` the negatives per positive (default 5).
``bpr.hip=-gpu N`` selects the device.
"""
import math
import random

import numpy as np

from ...base.IterativeRecommender import IterativeRecommender
from ...data.arrays import ArrayRecord
from ...tool.config import LineConfig

MAX_HIDDEN = 128


class CDAE(IterativeRecommender):

    def __init__(self, conf, trainingSet=None, testSet=None, fold='[1]'):
        super(CDAE, self).__init__(conf, trainingSet, testSet, fold)

    def readConfiguration(self):
        super(CDAE, self).readConfiguration()
        eps = LineConfig(self.config['CDAE'])
        self.corruption_level = float(eps['-co'])
        self.n_hidden = int(eps['-nh'])
        self.batch_size = int(eps['-batch_size'])
        self.n_hidden = 128                                          # :26 overwrites what -nh gave
        self.stddev, self.mask_seed, self.negative_sp = 1.0, 2, 5
        if self.config.contains('cdae.hip'):
            given = LineConfig(self.config['cdae.hip'])
            if given.contains('-nh'):
                self.n_hidden = int(given['-nh'])
            if given.contains('-stddev'):
                self.stddev = float(given['-stddev'])
            if given.contains('-seed'):
                self.mask_seed = int(given['-seed'])
            if given.contains('-neg'):
                self.negative_sp = int(given['-neg'])
        if not 1 <= self.n_hidden <= MAX_HIDDEN:
            print('CDAE: cdae.hip=-nh must be 1 .. %d (the ranking scan takes factors of width h + 1 <= 256; the kernels hold a row in two registers per lane)' % MAX_HIDDEN)
            exit(-1)
        if self.batch_size < 1 or not 0.0 < self.corruption_level <= 1.0 or not self.stddev > 0.0 or self.negative_sp < 0:
            print('CDAE: -batch_size must be at least 1, -co in (0, 1] (the share of input entries KEPT), -stddev above 0, -neg at least 0')
            exit(-1)

    def initModel(self):
        if isinstance(self.data, ArrayRecord):
            print('CDAE samples from the text log\'s training events; array-native data is not supported')
            exit(-1)
        super(CDAE, self).initModel()
        rt = self.recType
        self.num_items = self.n = self.data.getSize(rt)
        self.num_users = self.m = self.data.getSize('user')
        m, n, h = self.m, self.n, self.n_hidden
        lim = math.sqrt(6.0 / (m + h))                               # tf.contrib.layers.xavier_initializer: uniform
        self.U = np.random.uniform(-lim, lim, size=(m, h)).astype(np.float32)
        self.W = np.random.normal(0.0, self.stddev, size=(n, h)).astype(np.float32)
        self.Wd = np.random.normal(0.0, self.stddev, size=(h, n)).astype(np.float32)
        self.b = np.random.normal(0.0, self.stddev, size=h).astype(np.float32)
        self.bd = np.random.normal(0.0, self.stddev, size=n).astype(np.float32)
        self.userListen = {}
        for item in self.data.trainingData:                          # :50-57
            uid = self.data.getId(item['user'], 'user')
            tid = self.data.getId(item[rt], rt)
            row = self.userListen.setdefault(uid, {})
            if tid not in row:
                row[tid] = 1
            else:
                row[tid] += 1
        self._user_csr = self._csr()
        print('training...')

    def _csr(self):
        """(ptr, items ascending, counts) of userListen."""
        ptr = np.zeros(self.m + 1, np.int64)
        items, counts = [], []
        for uid in range(self.m):
            row = self.userListen.get(uid, {})
            for tid in sorted(row):
                items.append(tid); counts.append(row[tid])
            ptr[uid + 1] = len(items)
        return ptr, np.asarray(items, np.int32).reshape(-1), np.asarray(counts, np.int32).reshape(-1)

    def next_batch(self):
        """(uids, sample sets) as written (:76-98), without the dense rows: the device reads the counts from the user CSR."""
        rt = self.recType
        uids, samples = [], []
        userList = list(self.data.name2id['user'].keys())
        itemList = list(self.data.name2id[rt].keys())
        for n in range(self.batch_size):
            user = random.choice(userList)
            uid = self.data.name2id['user'][user]
            uids.append(uid)
            ratedItems = self.userListen.get(uid, {}).keys()
            sample = set(ratedItems)
            for i in range(self.negative_sp * len(ratedItems)):
                ng = random.choice(itemList)                         # never rejected (:93)
                sample.add(self.data.name2id[rt][ng])
            samples.append(sample)
        return uids, samples

    def buildModel(self):
        dev = self._device()
        dev.cdae_set_data(self.m, self.n, *self._user_csr)
        dev.cdae_set_params(self.U, self.W, self.Wd, self.b, self.bd)
        for epoch in range(self.maxIter):
            users, samples = self.next_batch()
            sptr = np.zeros(len(samples) + 1, np.int64)
            sptr[1:] = np.cumsum([len(s) for s in samples])
            sitems = np.array([i for s in samples for i in sorted(s)], np.int32).reshape(-1)
            loss, saturated = dev.cdae_step(users, sptr, sitems, self.corruption_level, self.mask_seed, self.lRate, self.regU, epoch + 1)
            self.loss = loss
            print(self.foldInfo, "Epoch:", '%04d' % (epoch + 1), "loss=", "{:.9f}".format(loss))
            if saturated:
                print('CDAE: %d sampled outputs round to 1.0f at step %d, so that log(1 - y_pred) = -inf: the loss is inf and TensorFlow\'s '
                      'gradients would be NaN.  Nothing was updated.  A smaller initial stddev keeps the outputs away from 1: '
                      'cdae.hip=-stddev 0.25 (the reference draws at 1.0), or a smaller learnRate' % (saturated, epoch + 1))
                exit(-1)
        print("Optimization Finished!")
        got = dev.cdae_get_params()
        self.U, self.W, self.Wd, self.b, self.bd = got['U'], got['W'], got['Wd'], got['b'], got['bd']
        # what predictForRanking means (:134-141): P[u] = [hid(u) | 1] from the uncorrupted row, Q[i] = [W'[:, i] | b'[i]], on the device
        dev.cdae_load_factors()
        arrays = self.data.to_arrays(self.recType)
        dev.set_interactions(arrays['indptr'], arrays['indices'], arrays['ev_ptr'], arrays['ev_i'])
        self._arrays = arrays
        self._device_factors_current = True
        self.P, self.Q = dev.get_factors()

    # ---- model file -----------------------------------------------------------------------
    def saveModel(self):
        out = self.output['-dir'] if hasattr(self, 'output') else './'
        np.savez(out + self.config['recommender'] + self.foldInfo + '-factors.npz', P=self.P, Q=self.Q, U=self.U, W=self.W, Wd=self.Wd, b=self.b, bd=self.bd)

    def loadModel(self):
        out = self.output['-dir'] if hasattr(self, 'output') else './'
        with np.load(out + self.config['recommender'] + self.foldInfo + '-factors.npz', allow_pickle=False) as z:
            self.P, self.Q, self.U, self.W, self.Wd, self.b, self.bd = z['P'], z['Q'], z['U'], z['W'], z['Wd'], z['b'], z['bd']
        self._device_factors_current = False
