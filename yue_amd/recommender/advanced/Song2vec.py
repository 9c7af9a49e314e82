#coding:utf8
"""Song2vec (track embedding from play lists, similar tracks, biased matrix factorisation with a similarity regulariser) behind
the reference's plugin hooks.

Replaces gensim's Word2Vec, the Python cosine loop and the NumPy SGD loop of the reference's recommender/advanced/Song2vec.py
with the device calls yue_cnet_set_sentences / yue_cnet_embed / yue_cnet_friends and yue_s2v_* (include/yue_hip.h, DESIGN.md
section 19).  What is kept:
  options     ``Song2vec=-alpha <a> -k <K>``; regB from ``reg.lambda -b``                                            (:28-32)
  set-up      X = P * 10, Y = Q * 10 (float32), then Bu = rand(m) / 10, Bi = rand(n) / 10 (float64) in this order        (:19-26)
  sentences   only users with MORE than 10 training events take part; a sentence is the user's tracks in record order,
              repeats included; T = rand(n_track, k) is drawn first, as the reference draws it                         (:35-46)
  similar     for every track of a sentence the K others with the largest cosine (0 on a zero norm)                   (:53-68)
  counts      the number of events per (trained user, item), items in first-listen order                              (:70-75)
  iteration   exactly num.max.iter times, no convergence test: the rating pass with the stale bu, then the pair pass;
              loss = squared errors + regB (Bu.Bu + Bi.Bi) + X.X + Y.Y without regU / regI, printed as
              ``iteration: i loss: x``                                                                                (:162-192)
  predict     Y . X[u] + globalMean + Bu[u]; globalMean is 0 as in the reference (it is computed before a record is read)
The embedding comes from one of:
  * ``Song2vec=... -emb hip [-seed N]`` (the default: gensim is absent in this build): gensim's documented CBOW with the library's
    own counter-based stream, sentences cut into segments (parity with gensim's output unpinned);
  * ``Song2vec=... -emb FILE.npy``: an [n_track][k] table in track-id order;
  * a ``T`` attribute set beforehand ([n_track][k]).
Deviations: the reference iterates a set of track names, so the order of its (track, similar track) pairs and of tied cosines
depends on the hash seed; here tracks are visited in ascending id and ties go to the smaller id.  An attribute ``pairOrder``
(t1 ids, t2 ids) set beforehand overrides the order (sims are looked up in the device's lists).  The reference reads
item['track'] whatever -target says: any other ``-target`` is refused.  ``bpr.hip=-gpu N`` selects the device as for BPR.
"""
import numpy as np

from ...base.IterativeRecommender import IterativeRecommender
from ...tool.config import LineConfig

MIN_EVENTS = 10
WINDOW, EPOCHS = 5, 10                                          # Word2Vec(..., window=5, min_count=0, iter=10), :47


class Song2vec(IterativeRecommender):

    def __init__(self, conf, trainingSet=None, testSet=None, fold='[1]'):
        super(Song2vec, self).__init__(conf, trainingSet, testSet, fold)

    def readConfiguration(self):
        super(Song2vec, self).readConfiguration()
        options = LineConfig(self.config['Song2vec'])
        self.alpha = float(options['-alpha'])
        self.topK = int(options['-k'])
        self.embSource = options['-emb'] if options.contains('-emb') else 'hip'
        self.embSeed = int(options['-seed']) if options.contains('-seed') else 1
        if self.recType != 'track':
            print('Song2vec embeds tracks: evaluation.setup must use -target track (got -target %s)' % self.recType)
            exit(-1)

    def printAlgorConfig(self):
        super(Song2vec, self).printAlgorConfig()
        print('Specified Arguments of', self.config['recommender'] + ':')
        print('alpha: %.5f' % self.alpha)
        print('k: %d' % self.topK)
        print('=' * 80)

    def _sync_factors_to_device(self):
        """The context's factors are X and Y (the scan ranks with Y.X[u]; the constant globalMean + Bu[u] moves no list)."""
        dev = self._device()
        dev.set_factors(self.X, self.Y)
        arrays = self.data.to_arrays(self.recType)
        dev.set_interactions(arrays['indptr'], arrays['indices'], arrays['ev_ptr'], arrays['ev_i'])
        self._arrays = arrays
        self._device_factors_current = True

    def initModel(self):
        super(Song2vec, self).initModel()
        self.X = self.P * 10
        self.Y = self.Q * 10
        self.m = self.data.getSize('user')
        self.n = self.data.getSize(self.recType)
        self.Bu = np.random.rand(self.m) / 10                   # bias value of user
        self.Bi = np.random.rand(self.n) / 10                   # bias value of item

    def _embedding(self, dev, ev_ptr, ev_i, users):
        """T [n][k] float32 with rows for the tracks of the sentences, uploaded as the embedding of yue_cnet_friends."""
        n = self.n
        listen = np.unique(np.concatenate([ev_i[ev_ptr[u]:ev_ptr[u + 1]] for u in users])).astype(np.int32) if users else np.zeros(0, np.int32)
        if hasattr(self, 'T') or self.embSource != 'hip':
            T = np.asarray(self.T if hasattr(self, 'T') else np.load(self.embSource), np.float32)
            if T.shape != (n, self.k):
                print('Song2vec: the embedding table must be [%d][%d] in track-id order (got %s)' % (n, self.k, 'x'.join(str(x) for x in T.shape)))
                exit(-1)
            dev.cnet_set_embedding(T, listen)
            return T, listen
        ptr = np.concatenate([[0], np.cumsum([ev_ptr[u + 1] - ev_ptr[u] for u in users])]).astype(np.int64)
        ids = np.concatenate([ev_i[ev_ptr[u]:ev_ptr[u + 1]] for u in users]).astype(np.int32)
        dev.cnet_set_sentences(n, ptr, ids)
        T = dev.cnet_embed(self.k, WINDOW, EPOCHS, self.embSeed)
        self.embed_ns = dev.get_option('cnet_last_ns')
        return T, listen

    def buildModel(self):
        d, rt = self.data, self.recType
        rand_T = np.random.rand(d.getSize('track'), self.k)      # :35, drawn first; its rows are replaced below where a track has one
        self._sync_factors_to_device()
        dev = self.dev
        ev_ptr, ev_i = self._arrays['ev_ptr'], self._arrays['ev_i']
        users = [u for u in range(self.m) if ev_ptr[u + 1] - ev_ptr[u] > MIN_EVENTS]
        su, si, sc = [], [], []
        for u in users:                                         # userListen, :70-75
            row = {}
            for i in ev_i[ev_ptr[u]:ev_ptr[u + 1]]:
                row[int(i)] = row.get(int(i), 0) + 1
            su += [u] * len(row); si += list(row.keys()); sc += list(row.values())
        t1, t2, sim = np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float64)
        self.topKSim = {}
        if users:
            T, listen = self._embedding(dev, ev_ptr, ev_i, users)
            self.T = rand_T
            self.T[listen] = T[listen]
            print('song embedding generated.')
            print('Constructing similarity matrix...')
            ids, sims = dev.cnet_friends(self.topK)
            self.friends_ns = dev.get_option('cnet_last_ns')
            names = d.id2name['track']
            for a in listen:
                self.topKSim[names[int(a)]] = [(names[int(b)], float(s)) for b, s in zip(ids[a], sims[a]) if b >= 0]
            if hasattr(self, 'pairOrder'):
                t1, t2 = (np.asarray(x, np.int32) for x in self.pairOrder)
                at = {(int(a), int(b)): float(s) for a in listen for b, s in zip(ids[a], sims[a]) if b >= 0}
                sim = np.array([at[(int(a), int(b))] for a, b in zip(t1, t2)], np.float64)
            else:
                keep = ids[listen] >= 0
                t1 = np.repeat(listen, keep.sum(axis=1)).astype(np.int32)
                t2, sim = ids[listen][keep], sims[listen][keep]
        else:
            self.T = rand_T
            print('song embedding generated.')
            print('Constructing similarity matrix...')
        dev.s2v_set_state(self.Bu, self.Bi)
        dev.s2v_set_steps(su, si, sc)
        dev.s2v_set_pairs(t1, t2, sim)
        print('training...')
        iteration = 0
        self.epoch_ns = []
        while iteration < self.maxIter:
            self.loss = 0
            e1, e2 = dev.s2v_epoch(self.lRate, self.regU, self.regI, self.regB, self.alpha, d.globalMean)
            self.epoch_ns.append(dev.get_option('s2v_last_ns'))
            for e in e1:
                self.loss += e
            for e in e2.astype(np.float32):                     # float32 squares meet the float64 sum (:187)
                self.loss += e
            dev.get_factors(self.X, self.Y)
            self.Bu, self.Bi = dev.s2v_get_state()
            self.loss += self.regB * (self.Bu * self.Bu).sum() + self.regB * (self.Bi * self.Bi).sum() + (self.X * self.X).sum() + (self.Y * self.Y).sum()
            iteration += 1
            print('iteration:', iteration, 'loss:', self.loss)
        self._device_factors_current = True

    def predict(self, u):
        'invoked to rank all the items for the user'
        scores = super(Song2vec, self).predict(u)
        return scores + self.data.globalMean + self.Bu[self.data.getId(u, 'user')]

    # ---- model file -----------------------------------------------------------------------
    def saveModel(self):
        out = self.output['-dir'] if hasattr(self, 'output') else './'
        np.savez(out + self.config['recommender'] + self.foldInfo + '-factors.npz', X=self.X, Y=self.Y, Bu=self.Bu, Bi=self.Bi)

    def loadModel(self):
        out = self.output['-dir'] if hasattr(self, 'output') else './'
        with np.load(out + self.config['recommender'] + self.foldInfo + '-factors.npz', allow_pickle=False) as z:
            self.X, self.Y, self.Bu, self.Bi = z['X'], z['Y'], z['Bu'], z['Bi']
        self._device_factors_current = False
