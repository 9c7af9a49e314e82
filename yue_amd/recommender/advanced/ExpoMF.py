#coding:utf8
"""ExpoMF (Liang, Charlin, McInerney and Blei: "Modeling User Exposure in Recommendation") behind the reference's plugin hooks.

Replaces the batched NumPy posterior and the per-row dense solves of the reference's recommender/advanced/ExpoMF.py with the
device calls yue_expo_* (include/yue_hip.h, DESIGN.md section "ExpoMF").  What is kept from the reference:
  initModel   the base class's P, Q are drawn first (they advance the random stream and are otherwise unused), then
              theta = 0.01 * randn(m, k), beta = 0.01 * randn(n, k) as float32, mu = 0.01 per item; the hyper-parameters are the
              literals of the reference (lam_theta = lam_beta = 1e-5, lam_y = 1, a = 1, b = 99); reg.lambda and learnRate of the
              configuration are not read by the model
  counts      r_ui = training events of (user, item) (the reference's CSR sums duplicates)
  iteration   every theta[u] from beta (the old theta[u] gives the posterior), every beta[i] from the new theta, then
              mu from the new theta, beta and the old mu; exactly num.max.iter iterations, no loss, no convergence test
  quirk       the reference tells the item half-sweep from the user one by mu.size == X.shape[0]: with as many users as
              items the item side indexes mu by the column (a user id).  Kept: mu_per_column = (m == n) on the item side
  zero rows   users / items without training pairs end with an exact zero row
  printed     ``training...``, ``ITERATION #i``, ``update factors...``, ``\tUpdating exposure prior...`` and the old mu
Deviations: the reference's class cannot run as shipped (initModel reads self.m and self.n, which only its deep-learning
base class sets): this plugin sets them itself.  Its evalRanking calls predict(), which the class does not override, so the
shipped lists come from the untrained P and Q; the model's own ranking formula is predictForRanking = beta . theta[u], and
that is what ranks here: theta and beta are the context's factors, so predict / evalRanking / ranking_performance use the
base class's scan unchanged.  ``bpr.hip=-gpu N`` selects the device as for BPR.
"""
import numpy as np

from ...base.IterativeRecommender import IterativeRecommender
from ..cf.WRMF import wrmf_pairs


class ExpoMF(IterativeRecommender):

    def __init__(self, conf, trainingSet=None, testSet=None, fold='[1]'):
        super(ExpoMF, self).__init__(conf, trainingSet, testSet, fold)

    def initModel(self):
        super(ExpoMF, self).initModel()
        self.m = self.data.getSize('user')
        self.n = self.data.getSize(self.recType)
        self.lam_theta = 1e-5
        self.lam_beta = 1e-5
        self.lam_y = 1.0
        self.init_mu = 0.01
        self.a = 1.0
        self.b = 99.0
        self.init_std = 0.01
        self.theta = self.init_std * np.random.randn(self.m, self.k).astype(np.float32)
        self.beta = self.init_std * np.random.randn(self.n, self.k).astype(np.float32)
        self.mu = self.init_mu * np.ones(self.n, dtype=np.float32)

    # ---- device state ---------------------------------------------------------------------
    def _sync_factors_to_device(self):
        """The context's factors are theta and beta (the scan ranks with beta.theta[u])."""
        dev = self._device()
        dev.set_factors(self.theta, self.beta)
        arrays = self.data.to_arrays(self.recType)
        dev.set_interactions(arrays['indptr'], arrays['indices'], arrays['ev_ptr'], arrays['ev_i'])
        self._arrays = arrays
        self._device_factors_current = True

    def buildModel(self):
        self._sync_factors_to_device()
        dev = self.dev
        user_major, item_major = wrmf_pairs(self._arrays['ev_ptr'], self._arrays['ev_i'], self.n)
        dev.expo_set_pairs(*(user_major + item_major))
        dev.expo_set_mu(self.mu)
        print('training...')
        for i in range(self.maxIter):
            print('ITERATION #%d' % i)
            print('update factors...')
            dev.expo_half_sweep(0, self.lam_theta / self.lam_y, self.lam_y, True)
            dev.expo_half_sweep(1, self.lam_beta / self.lam_y, self.lam_y, self.m == self.n)
            print('\tUpdating exposure prior...')
            print(self.mu)
            dev.expo_update_mu(self.a, self.b, self.lam_y)
            self.mu = dev.expo_get_mu()
        dev.get_factors(self.theta, self.beta)                   # state contract: trained factors back on the host
        self._device_factors_current = True

    # ---- model file -----------------------------------------------------------------------
    def saveModel(self):
        out = self.output['-dir'] if hasattr(self, 'output') else './'
        np.savez(out + self.config['recommender'] + self.foldInfo + '-factors.npz', theta=self.theta, beta=self.beta, mu=self.mu)

    def loadModel(self):
        out = self.output['-dir'] if hasattr(self, 'output') else './'
        with np.load(out + self.config['recommender'] + self.foldInfo + '-factors.npz', allow_pickle=False) as z:
            self.theta, self.beta, self.mu = z['theta'], z['beta'], z['mu']
        self._device_factors_current = False
