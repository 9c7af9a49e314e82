#coding:utf8
"""WRMF (Hu, Koren and Volinsky: implicit-feedback matrix factorisation, alternating least squares) behind the
reference's plugin hooks.

Replaces the per-user / per-item NumPy solves of the reference's recommender/cf/WRMF.py:24-76 with the device
half-sweeps yue_wrmf_* (include/yue_hip.h, DESIGN.md section "WRMF").  What is kept from the reference:
  initModel   the base class's P, Q (same random stream), then X = P*10, Y = Q*10, both float32            (:17-22)
  counts      r_ui = training events of (user, item); confidence alpha*r with alpha = 10, b weight 1 + 10*r    (:25-30, :50-53)
  user sweep  X[u] from Y over every user id; item sweep Y[i] from the new X, with regU on BOTH sides (a quirk of
              the reference, :74, kept)
  loss        sum over the distinct pairs of (1 - x_u.y_i)^2 from X[u] before its update, user sweep only (:46-47),
              printed as ``iteration: i loss: x``; no convergence test, exactly num.max.iter iterations (:78-81)
  zero rows   users / items without training pairs (test-only names) end with an exact zero row
The device keeps X and Y in the context's factor buffers, so predict / evalRanking / ranking_performance rank with the
base class's scan unchanged.  ``bpr.hip=-gpu N`` selects the device as for BPR.
"""
import numpy as np

from ...base.IterativeRecommender import IterativeRecommender

ALPHA = 10.0        # WRMF.py:50 (val = 10*r_ui), :53 (H += 10*r_ui)


def wrmf_pairs(ev_ptr, ev_i, n):
    """Distinct (user, item) pairs with their event counts, both ways: user-major (items ascending) and item-major
    (users ascending, a stable sort of the user-major list) -- the arguments of yue_wrmf_set_pairs."""
    m = len(ev_ptr) - 1
    ev_u = np.repeat(np.arange(m, dtype=np.int64), np.diff(ev_ptr))
    keys, counts = np.unique(ev_u * n + np.asarray(ev_i, np.int64), return_counts=True)
    users = (keys // n).astype(np.int32)
    items = (keys % n).astype(np.int32)
    counts = counts.astype(np.int32)
    u_ptr = np.zeros(m + 1, np.int64)
    np.add.at(u_ptr, users.astype(np.int64) + 1, 1)
    order = np.argsort(items, kind='stable')
    i_ptr = np.zeros(n + 1, np.int64)
    np.add.at(i_ptr, items.astype(np.int64) + 1, 1)
    return (np.cumsum(u_ptr), items, counts), (np.cumsum(i_ptr), users[order], counts[order])


class WRMF(IterativeRecommender):

    def __init__(self, conf, trainingSet=None, testSet=None, fold='[1]'):
        super(WRMF, self).__init__(conf, trainingSet, testSet, fold)

    def initModel(self):
        super(WRMF, self).initModel()
        self.X = self.P * 10
        self.Y = self.Q * 10
        self.m = self.data.getSize('user')
        self.n = self.data.getSize(self.recType)

    # ---- device state ---------------------------------------------------------------------
    def _sync_factors_to_device(self):
        """The context's factors are X and Y (the scan ranks with Y.X[u], WRMF.py:83-86)."""
        dev = self._device()
        dev.set_factors(self.X, self.Y)
        arrays = self.data.to_arrays(self.recType)
        dev.set_interactions(arrays['indptr'], arrays['indices'], arrays['ev_ptr'], arrays['ev_i'])
        self._arrays = arrays
        self._device_factors_current = True

    def buildModel(self):
        self._sync_factors_to_device()
        dev = self.dev
        arrays = self._arrays
        user_major, item_major = wrmf_pairs(arrays['ev_ptr'], arrays['ev_i'], self.data.getSize(self.recType))
        dev.wrmf_set_pairs(*(user_major + item_major))
        print('training...')
        iteration = 0
        while iteration < self.maxIter:
            self.loss = dev.wrmf_half_sweep(0, ALPHA, self.regU)
            dev.wrmf_half_sweep(1, ALPHA, self.regU)             # regU on the item side too (WRMF.py:74)
            iteration += 1
            print('iteration:', iteration, 'loss:', self.loss)
        dev.get_factors(self.X, self.Y)                          # state contract: trained factors back on the host
        self._device_factors_current = True

    # ---- model file -----------------------------------------------------------------------
    def saveModel(self):
        out = self.output['-dir'] if hasattr(self, 'output') else './'
        np.savez(out + self.config['recommender'] + self.foldInfo + '-factors.npz', X=self.X, Y=self.Y)

    def loadModel(self):
        out = self.output['-dir'] if hasattr(self, 'output') else './'
        with np.load(out + self.config['recommender'] + self.foldInfo + '-factors.npz', allow_pickle=False) as z:
            self.X, self.Y = z['X'], z['Y']
        self._device_factors_current = False
