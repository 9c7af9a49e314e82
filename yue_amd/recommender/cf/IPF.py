#coding:utf8
"""IPF (ranking over the session temporal graph) behind the reference's plugin hooks.

Replaces the per-user Python DFS of the reference's recommender/cf/IPF.py:59-91 with the device calls yue_ipf_*
(include/yue_hip.h, DESIGN.md section "IPF").  What is kept from the reference:
  STG         UL[u] = u's training events in userRecord order, S[u] = UL[u][-10:] (:14-22); item2user = the keys of
              listened[recType][item] in insertion order, item2session = the users whose session holds the item, in
              userRecord order, duplicates kept (:26-33)
  weights     the reference's probability() (:45-56) as Python floats, computed here once and uploaded:
              1/pow(len(UL[b]), rho), 1/pow(len(S[b]), rho), pow(eta/(eta nU + nS), rho), pow(1/(eta nU + nS), rho)
  paths       (user, item2user, user), (user, item2session, session), (session, item2user, user), (session, item2session,
              session), one shared rank dict: the first discoverer of a node gives it its one contribution per path
              (reduced to max-reductions: DESIGN.md section "IPF"); items by (score descending, first insertion)
  config      -rho (outside [0, 1] it becomes 0.5), -beta, -eta
  evalRanking the list path of the reference's base class, as UserKNN runs it (shared code: recommender/cf/UserKNN.py)
One deviation: -eta <= 0 is refused with a message.  The reference divides by zero there (eta = 0 and an item held by
no session) or weighs paths by negative numbers.  ``bpr.hip=-gpu N`` selects the device as for the other plugins.
``-format csr`` data sets rank to integer lists; their item2user order is ascending user id.
"""
import numpy as np

from ...base.recommender import Recommender
from ...data.arrays import ArrayRecord
from ...tool.config import LineConfig
from .UserKNN import UserKNN


def _distinct_first(owner, items, rows, n):
    """Per owner (ascending, entries in order), its distinct items in first-occurrence order: (ptr[rows+1], items)."""
    keys = owner.astype(np.int64) * n + items
    _, first = np.unique(keys, return_index=True)
    first.sort()
    ptr = np.zeros(rows + 1, np.int64)
    np.add.at(ptr, owner[first].astype(np.int64) + 1, 1)
    return np.cumsum(ptr), items[first].astype(np.int32)


def _pow_table(values, fn):
    """fn(v) for every entry of values, one Python call per distinct value (the same float as calling it per entry)."""
    memo = {}
    out = np.zeros(len(values), np.float64)
    for t, v in enumerate(values.tolist()):
        if v not in memo:
            memo[v] = fn(v)
        out[t] = memo[v]
    return out


def ipf_graph(ev_ptr, ev_i, n, rho, beta, eta, i2u=None):
    """The graph and weights yue_ipf_set_graph takes.  ev_ptr / ev_i: training events user-major in userRecord order;
    i2u: optional (hu_ptr, hu_users) in listened order (default: ascending user id, as for -byTime and csr data)."""
    ev_ptr = np.asarray(ev_ptr, np.int64)
    ev_i = np.asarray(ev_i, np.int32)
    m = len(ev_ptr) - 1
    L = np.diff(ev_ptr)
    ev_u = np.repeat(np.arange(m, dtype=np.int32), L)
    u_ptr, u_items = _distinct_first(ev_u, ev_i, m, n)
    at = np.arange(len(ev_i), dtype=np.int64) - ev_ptr[ev_u]
    sess = at >= (L - 10)[ev_u]
    sev_u, sev_i = ev_u[sess], ev_i[sess]
    s_ptr, s_items = _distinct_first(sev_u, sev_i, m, n)
    # item -> session holders with duplicates (user order), then the distinct holders with their first positions
    order = np.argsort(sev_i, kind='stable')
    hu_dup, hi_dup = sev_u[order], sev_i[order]
    nS = np.bincount(sev_i, minlength=n).astype(np.int64)
    row_beg = np.concatenate([[0], np.cumsum(nS)])
    pos = np.arange(len(hu_dup), dtype=np.int64) - row_beg[hi_dup]
    first = np.ones(len(hu_dup), bool)
    first[1:] = (hu_dup[1:] != hu_dup[:-1]) | (hi_dup[1:] != hi_dup[:-1])
    hs_users, hs_pos = hu_dup[first].astype(np.int32), pos[first].astype(np.int32)
    hs_ptr = np.concatenate([[0], np.cumsum(np.bincount(hi_dup[first], minlength=n))]).astype(np.int64)
    if i2u is None:
        order = np.argsort(u_items, kind='stable')
        hu_users = np.repeat(np.arange(m, dtype=np.int32), np.diff(u_ptr))[order]
        hu_ptr = np.concatenate([[0], np.cumsum(np.bincount(u_items, minlength=n))]).astype(np.int64)
    else:
        hu_ptr, hu_users = np.asarray(i2u[0], np.int64), np.asarray(i2u[1], np.int32)
    nU = np.diff(hu_ptr)
    w_user = _pow_table(L, lambda x: 1.0 / pow(x, rho) if x > 0 else 0.0)
    w_sess = _pow_table(np.minimum(L, 10), lambda x: 1.0 / pow(x, rho) if x > 0 else 0.0)
    both = [(int(a), int(b)) for a, b in zip(nU, nS)]
    memo_u, memo_s = {}, {}
    p_i2u, p_i2s = np.zeros(n, np.float64), np.zeros(n, np.float64)
    for c, key in enumerate(both):
        if key[0] == 0:                                  # an item no training user holds is never expanded
            continue
        if key not in memo_u:
            memo_u[key] = pow(eta / (eta * key[0] + key[1]), rho)
            memo_s[key] = pow(1 / (eta * key[0] + key[1]), rho)
        p_i2u[c], p_i2s[c] = memo_u[key], memo_s[key]
    return {'m': m, 'n': n, 'u_ptr': u_ptr, 'u_items': u_items, 's_ptr': s_ptr, 's_items': s_items, 'hu_ptr': hu_ptr,
            'hu_users': hu_users, 'hs_ptr': hs_ptr, 'hs_users': hs_users, 'hs_pos': hs_pos, 'w_user': w_user,
            'w_sess': w_sess, 'p_i2u': p_i2u, 'p_i2s': p_i2s, 'r_user': beta, 'r_sess': 1 - beta}


class IPF(Recommender):

    def __init__(self, conf, trainingSet=None, testSet=None, fold='[1]'):
        super(IPF, self).__init__(conf, trainingSet, testSet, fold)
        self.dev = None

    def readConfiguration(self):
        super(IPF, self).readConfiguration()
        opts = LineConfig(self.config['IPF'])
        self.rho = float(opts['-rho'])
        if self.rho < 0 or self.rho > 1:
            self.rho = 0.5
        self.beta = float(opts['-beta'])
        self.eta = float(opts['-eta'])
        if self.eta <= 0:
            print('IPF: -eta must be positive (got %s)' % opts['-eta'])
            exit(-1)

    _device = UserKNN._device

    def initModel(self):
        super(IPF, self).initModel()
        print('initializing STG...')
        d, rt = self.data, self.recType
        arrays = d.to_arrays(rt)                        # asserts that userRecord runs in ascending user id
        i2u = None
        if not isinstance(d, ArrayRecord):
            ids = d.name2id['user']
            rows = [[ids[user] for user in d.listened[rt][item]] if item in d.listened[rt] else []
                    for item in (d.id2name[rt][c] for c in range(d.getSize(rt)))]
            i2u = (np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64),
                   np.array([b for r in rows for b in r], np.int32))
        self.graph = ipf_graph(arrays['ev_ptr'], arrays['ev_i'], d.getSize(rt), self.rho, self.beta, self.eta, i2u)
        self._device().ipf_set_graph(self.graph)
        self.trained = np.diff(arrays['ev_ptr']) > 0

    def predict(self, u):
        items, _ = self.dev.ipf_predict(self.data.getId(u, 'user'))
        names = self.data.id2name[self.recType]
        return [names[int(i)] for i in items]

    def _topn(self, uids, N):
        if len(uids) == 0 or N == 0:
            return np.zeros((len(uids), N), np.int32), np.zeros(len(uids), np.int32)
        ids, _, lens = self.dev.ipf_topn(uids, N)
        return ids, lens

    # the base class's list path (lists file, ['0'] for test-only users, marks, measures), shared with UserKNN
    evalRanking = UserKNN.evalRanking
    _evalRanking_arrays = UserKNN._evalRanking_arrays
