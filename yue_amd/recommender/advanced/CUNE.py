#coding:utf8
"""CUNE's training loop (collaborative user network embedding, two-level BPR) behind the reference's plugin hooks.

Replaces the NumPy SGD loop of the reference's recommender/advanced/CUNE.py:120-178 with the device function
yue_cune_steps (include/yue_hip.h): per (user, positive item) three steps, each either the two-level step with a
friends' item k and a sampled negative j or, for a user without friends' items, the plain (i over j) step.  Draws are
made on the host exactly as the reference makes them (``choice`` over the friends' items / the item names, rejection of
listened items through ``data.listened``), so a seeded ``random`` gives the reference's stream; the loss is added up as
the reference adds it (the regulariser once per user, :175 -- the running loss is a float32 from then on).

The friends' item sets (the product of CUNE.py:34-118: collaborative user network, random walks, Word2Vec user embedding,
cosine top-K friends) come from one of:
  * ``CUNE=... -net hip [-seed N]``: the user-network stage on the device (yue_cnet_*).  gensim is
    absent in this build, so the embedding follows gensim's documented algorithm with the library's own counter-based
    stream (parity with gensim's output unpinned); network, walks, friends and the sets follow the reference.
  * ``CUNE=... -friends FILE`` (one line per user: ``user:friend,friend,...``; a user's friends' items are the items its
    friends listened to and the user did not, CUNE.py:112-114);
  * an ``IPositiveSet`` attribute set on the instance beforehand.
Without any of them every user takes the plain branch.
"""
from collections import defaultdict
from math import isnan
from random import choice

import numpy as np

from ...base.IterativeRecommender import IterativeRecommender
from ...tool.config import LineConfig


class CUNE(IterativeRecommender):

    def __init__(self, conf, trainingSet=None, testSet=None, fold='[1]'):
        super(CUNE, self).__init__(conf, trainingSet, testSet, fold)

    def readConfiguration(self):
        super(CUNE, self).readConfiguration()
        options = LineConfig(self.config['CUNE'])
        self.walkCount = int(options['-T'])
        self.walkLength = int(options['-L'])
        self.walkDim = int(options['-l'])
        self.winSize = int(options['-w'])
        self.topK = int(options['-k'])
        self.s = float(options['-s'])
        self.epoch = int(options['-ep'])
        self.friendsFile = options['-friends'] if options.contains('-friends') else ''
        self.netMode = options['-net'] if options.contains('-net') else ''
        self.netSeed = int(options['-seed']) if options.contains('-seed') else 1
        if self.netMode not in ('', 'hip'):
            print('CUNE: -net takes the value hip.')
            exit(-1)

    def _item_sets(self):
        self.PositiveSet = defaultdict(list)                    # CUNE.py:107-113
        for user in self.data.userRecord:
            for event in self.data.userRecord[user]:
                self.PositiveSet[user].append(event[self.recType])
        if hasattr(self, 'IPositiveSet'):
            return
        self.IPositiveSet = defaultdict(list)
        if not self.friendsFile and self.netMode == 'hip':
            self._user_network()
            return
        if not self.friendsFile:
            print('CUNE: no -friends file: the user-network stage (gensim) is not part of this build; every user takes the plain step.')
            return
        for line in open(self.friendsFile):
            if ':' not in line:
                continue
            user, friends = line.strip().split(':', 1)
            for friend in [f for f in friends.split(',') if f]:
                if user in self.PositiveSet and friend in self.PositiveSet:      # :115-117
                    self.IPositiveSet[user] += list(set(self.PositiveSet[friend]).difference(self.PositiveSet[user]))

    def _user_network(self):
        """CUNE.py:34-114 with the four device stages: fills W (m x walkDim), topKSim and IPositiveSet.  The sets are built
        on the host from the CSR rows (at config-3 size they are too large to materialise: out of scope)."""
        d, rt = self.data, self.recType
        print('Kind Note: This method will probably take much time.')
        print('Building collaborative user network...')
        arrays = d.to_arrays(rt)
        m, n = d.getSize('user'), d.getSize(rt)
        u_ptr, u_items = arrays['indptr'], arrays['indices']
        users = np.repeat(np.arange(m, dtype=np.int32), np.diff(u_ptr))
        i_ptr = np.concatenate([[0], np.cumsum(np.bincount(u_items, minlength=n))]).astype(np.int64)
        dev = self._device()
        dev.cnet_set_pairs(m, n, u_ptr, u_items, i_ptr, users[np.argsort(u_items, kind='stable')])
        print('Generating random deep walks...')
        self.walks = dev.cnet_walks(self.walkCount, self.walkLength, self.netSeed)
        print('Generating user embedding...')
        self.W = dev.cnet_embed(self.walkDim, self.winSize, self.epoch, self.netSeed)
        print('User embedding generated.')
        print('Constructing similarity matrix...')
        ids, sims = dev.cnet_friends(self.topK)
        unames, inames = d.id2name['user'], d.id2name[rt]
        net = np.flatnonzero(ids[:, 0] >= 0)                    # a network user has at least one neighbour, hence a friend
        self.topKSim = {}
        for i, u in enumerate(net, 1):
            self.topKSim[unames[u]] = [(unames[b], float(s)) for b, s in zip(ids[u], sims[u]) if b >= 0]
            if i % 200 == 0:
                print('progress:', i, '/', len(net))
        print('Similarity matrix finished.')
        print('Preparing item sets...')
        for u in net:                                           # :112-114; a friend's new items in ascending item id
            mine = u_items[u_ptr[u]:u_ptr[u + 1]]
            row = self.IPositiveSet[unames[u]]
            for b in ids[u][ids[u] >= 0]:
                theirs = u_items[u_ptr[b]:u_ptr[b + 1]]
                row += [inames[x] for x in theirs[~np.isin(theirs, mine)]]

    def buildModel(self):
        self._item_sets()
        d, rt = self.data, self.recType
        self._sync_factors_to_device()
        dev = self.dev
        print('Training...')
        iteration = 0
        while iteration < self.maxIter:
            self.loss = 0
            itemList = list(d.name2id[rt].keys())
            for user in self.PositiveSet:
                u = d.getId(user, 'user')
                uu, ii, kk, jj = [], [], [], []
                for item in self.PositiveSet[user]:
                    i = d.getId(item, rt)
                    for _n in range(3):
                        k = -1
                        if len(self.IPositiveSet[user]) > 0:
                            k = d.getId(choice(self.IPositiveSet[user]), rt)
                        item_j = choice(itemList)
                        while user in d.listened[rt][item_j]:
                            item_j = choice(itemList)
                        uu.append(u); ii.append(i); kk.append(k); jj.append(d.getId(item_j, rt))
                for x in dev.cune_steps(uu, ii, kk, jj, self.s, self.lRate, self.regU, self.regI):
                    self.loss += float(x)
                sumP, sumQ = dev.sumsq()
                # :175 inside the user loop: NumPy float32 sums times python floats -> the loss turns float32
                self.loss += self.regU * np.float32(sumP) + self.regI * np.float32(sumQ)
                if isnan(float(self.loss)):
                    break
            iteration += 1
            if self.isConverged(iteration):
                break
        self.P, self.Q = dev.get_factors(self.P, self.Q)
        self._device_factors_current = True
