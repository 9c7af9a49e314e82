#coding:utf8
"""CoFactor (Liang, Altosaar, Charlin and Blei: "Factorization Meets the Item Embedding") behind the reference's plugin hooks.

Replaces the set intersections of the reference's recommender/advanced/CoFactor.py initModel and the per-row NumPy solves of its
buildModel with the device calls yue_cof_* and yue_wrmf_half_sweep (include/yue_hip.h).  What is kept:
  options     ``CoFactor=-k <neg> -gamma <regR> -filter <f>``, neg clamped to >= 1                                   (:13-20)
  counts      r_ui = training events of (user, item): the pairs of WRMF
  co-occur.   items with at least f training EVENTS take part; count = common users; a pair is kept when count > f   (:46-66)
  SPPMI       freq = row sums, D = their sum, val = max(log(count * D / (freq_i * freq_j)) - log(neg), 0), only val > 0,
              divided by the largest -- on the host in the reference's double arithmetic, from the device's integer counts,
              so the values are the reference's bit for bit                                                          (:68-91)
  set-up      X = P * 10, Y = Q * 10 (float32), then w = rand(n) / 10, c = rand(n) / 10, G = rand(n, k) / 10 from np.random in
              this order, float64: a seeded run starts from the reference's state                                     (:97-101)
  user sweep  WRMF's (alpha = 10, regU) with its loss, printed as ``iteration: i loss: x``                            (:107-125)
  item sweep  items in id order, each reading the current rows of its contexts; regU on the item side too (the quirk of
              WRMF); run on the device level by level with the sequential sweep's result                              (:127-168)
  loop        exactly num.max.iter iterations, no convergence test
  zero rows   users / items without training pairs end with an exact zero row
Deviations: the reference's class cannot run as shipped (initModel reads self.n and self.m, which nothing sets): this plugin
sets them itself.  Its evalRanking calls predict(), which the class does not override, so the shipped lists come from the
untrained P and Q; the model's own ranking formula is predictForRanking = Y . X[u], and that is what ranks here: X and Y are the
context's factors, so predict / evalRanking / ranking_performance use the base class's scan unchanged.  The reference keys its
co-occurrence by track: any other ``-target`` is refused.  ``bpr.hip=-gpu N`` selects the device as for BPR.
"""
import math

import numpy as np

from ...base.IterativeRecommender import IterativeRecommender
from ...tool.config import LineConfig
from ..cf.WRMF import ALPHA, wrmf_pairs


def sppmi_from_counts(ptr, idx, cnt, neg):
    """The SPPMI CSR (ptr, idx, val float64) of a symmetric co-occurrence CSR, operation by operation as CoFactor.py:68-91 on
    doubles: count * D, freq_i * freq_j, their quotient, log, minus log(neg); the positive values divided by the largest."""
    n = len(ptr) - 1
    rows = np.repeat(np.arange(n), np.diff(ptr))
    freq = np.zeros(n, np.float64)
    np.add.at(freq, rows, cnt.astype(np.float64))               # integer-valued doubles: exact in any order
    D = float(freq.sum())
    if len(idx) == 0:
        return np.zeros(n + 1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.float64)
    # math.log entry by entry: NumPy's vectorised log differs from it in the last bit for some arguments
    ratio = cnt.astype(np.float64) * D / (freq[rows] * freq[idx])
    val = np.fromiter((math.log(x) for x in ratio.tolist()), np.float64, len(ratio)) - math.log(neg)
    keep = val > 0
    out_ptr = np.zeros(n + 1, np.int64)
    np.add.at(out_ptr, rows[keep] + 1, 1)
    val = val[keep]
    return np.cumsum(out_ptr), idx[keep].astype(np.int32), (val / val.max() if len(val) else val)


class CoFactor(IterativeRecommender):

    def __init__(self, conf, trainingSet=None, testSet=None, fold='[1]'):
        super(CoFactor, self).__init__(conf, trainingSet, testSet, fold)

    def readConfiguration(self):
        super(CoFactor, self).readConfiguration()
        options = LineConfig(self.config['CoFactor'])
        self.negCount = max(1, int(options['-k']))
        self.regR = float(options['-gamma'])
        self.filter = int(options['-filter'])
        if self.recType != 'track':
            print('CoFactor counts co-occurrence over tracks: evaluation.setup must use -target track (got -target %s)' % self.recType)
            exit(-1)

    def printAlgorConfig(self):
        super(CoFactor, self).printAlgorConfig()
        print('Specified Arguments of', self.config['recommender'] + ':')
        print('k: %d' % self.negCount)
        print('regR: %.5f' % self.regR)
        print('filter: %d' % self.filter)
        print('=' * 80)

    # ---- device state ---------------------------------------------------------------------
    def _sync_factors_to_device(self):
        """The context's factors are X and Y (the scan ranks with Y.X[u], CoFactor.py:176-179)."""
        dev = self._device()
        dev.set_factors(self.X, self.Y)
        arrays = self.data.to_arrays(self.recType)
        dev.set_interactions(arrays['indptr'], arrays['indices'], arrays['ev_ptr'], arrays['ev_i'])
        self._arrays = arrays
        self._device_factors_current = True

    def initModel(self):
        super(CoFactor, self).initModel()
        self.m = self.num_users = self.data.getSize('user')
        self.n = self.num_items = self.data.getSize(self.recType)
        self.X = self.P * 10
        self.Y = self.Q * 10
        print('Constructing SPPMI matrix...')
        self._sync_factors_to_device()
        user_major, item_major = wrmf_pairs(self._arrays['ev_ptr'], self._arrays['ev_i'], self.n)
        self.dev.wrmf_set_pairs(*(user_major + item_major))
        self.cooccur = self.dev.cof_cooccur(self.filter)
        self.SPPMI = sppmi_from_counts(self.cooccur[0], self.cooccur[1], self.cooccur[2], self.negCount)

    def buildModel(self):
        dev = self.dev
        self.X = self.P * 10
        self.Y = self.Q * 10
        self.w = np.random.rand(self.n) / 10
        self.c = np.random.rand(self.n) / 10
        self.G = np.random.rand(self.n, self.k) / 10
        dev.set_factors(self.X, self.Y)
        dev.cof_set_sppmi(*self.SPPMI)
        dev.cof_set_state(self.G, self.w, self.c)
        print('training...')
        iteration = 0
        while iteration < self.maxIter:
            self.loss = dev.wrmf_half_sweep(0, ALPHA, self.regU)
            dev.cof_item_sweep(ALPHA, self.regU, self.regR)      # regU on the item side too (CoFactor.py:163)
            iteration += 1
            print('iteration:', iteration, 'loss:', self.loss)
        dev.get_factors(self.X, self.Y)                          # state contract: trained factors back on the host
        self.G, self.w, self.c = dev.cof_get_state()
        self._device_factors_current = True

    # ---- model file -----------------------------------------------------------------------
    def saveModel(self):
        out = self.output['-dir'] if hasattr(self, 'output') else './'
        np.savez(out + self.config['recommender'] + self.foldInfo + '-factors.npz', X=self.X, Y=self.Y, G=self.G, w=self.w, c=self.c)

    def loadModel(self):
        out = self.output['-dir'] if hasattr(self, 'output') else './'
        with np.load(out + self.config['recommender'] + self.foldInfo + '-factors.npz', allow_pickle=False) as z:
            self.X, self.Y, self.G, self.w, self.c = z['X'], z['Y'], z['G'], z['w'], z['c']
        self._device_factors_current = False
