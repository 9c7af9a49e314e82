#coding:utf8
"""UserKNN (user-based neighbourhood model) behind the reference's plugin hooks.

Replaces the O(m^2) Python set intersections of the reference's recommender/cf/UserKNN.py:44-66 and its per-item loop
(:26-42) with the device calls yue_knn_* (include/yue_hip.h, DESIGN.md section "UserKNN").  What is kept from the reference:
  A_u         the distinct training items of user u (only the keys of its count dict are read, :46-52)
  similarity  2|A_u & A_v| / |A_u | A_v| as a Python float (:68-69): in [0, 2], not Jaccard
  topUsers    the first num.neighbors entries of a stable descending sort over every other training user, inserted in
              ascending user id (:56-63): the order (sim descending, user id ascending); entries with sim 0 never change a
              score, so only the positive ones are kept
  predict     score(i) = sum_r sim_r * count_r(i) / sum_r sim_r over the neighbours in rank order, fp64 (:26-42); items by
              score descending, ties in listened order = ascending item id
  evalRanking the list path of the reference's base class (base/recommender.py:85-150): predict minus the user's training
              items, the first N, possibly shorter; a test user without training records gets ['0']; '*' for a test item,
              '$' for an item of PopTrack
  printing    'Computing user similarities...', 'ind / len finished.' every 100 users, 'The user correlation has been
              figured out.' (printed after the device call: the text is the contract)
``bpr.hip=-gpu N`` selects the device as for the other plugins.  ``-format csr`` data sets rank to integer lists.
"""
from os.path import abspath
from time import localtime, strftime, time

import numpy as np

from ...base.recommender import Recommender
from ...data.arrays import ArrayRecord, ranking_measure_lists
from ...tool import config
from ...tool.file import FileIO
from ..cf.WRMF import wrmf_pairs

HEADER = 'userId: recommendations in (itemId, ranking score) pairs, * means the item matches, $ means the unpop item\n'


def list_line(user, items, wanted, pop):
    """One line of the lists file (base/recommender.py:124-134)."""
    line = user + ':'
    for item in items:
        if item in wanted:
            line += '*'
        if item in pop:
            line += '$'
        line += item + ','
    return line + '\n'


class UserKNN(Recommender):

    def __init__(self, conf, trainingSet=None, testSet=None, fold='[1]'):
        super(UserKNN, self).__init__(conf, trainingSet, testSet, fold)
        self.dev = None

    def readConfiguration(self):
        super(UserKNN, self).readConfiguration()
        self.neighbors = int(self.config['num.neighbors'])

    def printAlgorConfig(self):
        "show algorithm's configuration"
        super(UserKNN, self).printAlgorConfig()
        print('Specified Arguments of', self.config['recommender'] + ':')
        print('num.neighbors:', self.config['num.neighbors'])
        print('=' * 80)

    def _device(self):
        if self.dev is None:
            from ..._shim import Device
            gpu = 0
            if self.config.contains('bpr.hip'):
                opts = config.LineConfig(self.config['bpr.hip'])
                if opts.contains('-gpu'):
                    gpu = int(opts['-gpu'])
            self.dev = Device(gpu)
        return self.dev

    def initModel(self):
        self.computeCorr()

    def computeCorr(self):
        'compute correlation among users'
        d, rt = self.data, self.recType
        arrays = d.to_arrays(rt)                        # asserts that userRecord runs in ascending user id
        m, n = d.getSize('user'), d.getSize(rt)
        if not isinstance(d, ArrayRecord):
            # ties of predict go in listened order: it must be ascending item id, as userRecord is for users
            ids = d.name2id[rt]
            order = [ids[item] for item in d.listened[rt]]
            assert order == sorted(order), 'listened order must follow item ids'
        (u_ptr, u_items, u_counts), (i_ptr, i_users, _) = wrmf_pairs(arrays['ev_ptr'], arrays['ev_i'], n)
        dev = self._device()
        dev.knn_set_pairs(m, n, u_ptr, u_items, u_counts, i_ptr, i_users)
        self.nbr, self.inter, self.union = dev.knn_neighbors(self.neighbors)
        self.trained = np.diff(arrays['ev_ptr']) > 0
        print('Computing user similarities...')
        users = int(self.trained.sum())
        for ind in range(0, users, 100):
            print(ind, '/', users, 'finished.')
        print('The user correlation has been figured out.')

    def topUsers(self, u):
        """[(user name, sim)] of the positive neighbours of user name u, in rank order."""
        uid = self.data.getId(u, 'user')
        names = self.data.id2name['user']
        return [(names[int(v)], float(2 * int(c)) / float(U))
                for v, c, U in zip(self.nbr[uid], self.inter[uid], self.union[uid]) if v >= 0]

    def predict(self, u):
        items, _ = self.dev.knn_predict(self.data.getId(u, 'user'))
        names = self.data.id2name[self.recType]
        return [names[int(i)] for i in items]

    def evalRanking(self):
        top = self._top_list()
        N = int(top[-1])
        if N > 100 or N < 0:
            print('N can not be larger than 100! It has been reassigned with 10')
            N = 10
        if isinstance(self.data, ArrayRecord):
            return self._evalRanking_arrays(top, N)
        d = self.data
        users = list(d.testSet.keys())
        uids = np.array([d.getId(u, 'user') for u in users], np.int32)
        trained = self.trained[uids] if len(uids) else np.zeros(0, bool)
        ids, lens = self._topn(uids[trained], N)
        names = d.id2name[self.recType]
        res = [HEADER]
        recList = {}
        row = 0
        userCount = len(users)
        for i, user in enumerate(users):
            if trained[i]:
                recList[user] = [names[int(x)] for x in ids[row, :lens[row]]]
                row += 1
            else:
                recList[user] = ['0'] if N > 0 else []       # ['0']*N collapses to one item (base/recommender.py:109-120)
            if i % 100 == 0:
                print(self.algorName, self.foldInfo, 'progress:' + str(i) + '/' + str(userCount))
            res.append(list_line(user, recList[user], d.testSet[user], d.PopTrack))
        self._write_results(res, recList, top)

    def _topn(self, uids, N):
        if len(uids) == 0 or N == 0:
            return np.zeros((len(uids), N), np.int32), np.zeros(len(uids), np.int32)
        ids, _, lens = self.dev.knn_topn(uids, N)
        return ids, lens

    def _evalRanking_arrays(self, top, N):
        """Array-native data: the lists stay integer (``self.recUsers``, ``self.recIds`` -1 padded, ``self.recLens``); a user
        without training events gets item 0, as the reference's ['0']; measures by data/arrays.py: ranking_measure_lists."""
        d = self.data
        uids = d.testSet.user_ids().astype(np.int32)
        trained = self.trained[uids]
        rows, lens = self._topn(uids[trained], N)
        ids = np.full((len(uids), N), -1, np.int32)
        self.recLens = np.zeros(len(uids), np.int32)
        ids[trained] = rows
        self.recLens[trained] = lens
        if N > 0:
            ids[~trained, 0] = 0
            self.recLens[~trained] = 1
        self.recUsers, self.recIds = uids, ids
        self.measure = ranking_measure_lists(d.test_indptr, d.test_indices, uids, ids, self.recLens, top, d.getSize(self.recType))
        stamp = strftime("%Y-%m-%d %H-%M-%S", localtime(time()))
        FileIO.writeFile(self.output['-dir'], self.config['recommender'] + '@' + stamp + '-measure' + self.foldInfo + '.txt', self.measure)
        if self.isOutput:
            np.savez(self.output['-dir'] + self.config['recommender'] + '@' + stamp + '-top-' + str(N) + 'items' + self.foldInfo + '.npz',
                     users=uids, ids=ids, lens=self.recLens)
        print('The result has been output to ', abspath(self.output['-dir']), '.')
        print('The result of %s %s:\n%s' % (self.algorName, self.foldInfo, ''.join(self.measure)))
