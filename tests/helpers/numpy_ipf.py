"""NumPy oracle of IPF (reference recommender/cf/IPF.py; device side: include/yue_hip.h yue_ipf_*), in the reduced form of
DESIGN.md section "IPF": per path p = 0..3, (user, item2user, user), (user, item2session, session), (session, item2user,
user), (session, item2session, session):

level 1   the start list (UL[u] on paths 0, 1; S[u] on 2, 3), its distinct items a_k numbered k = 1, 2, ... by first
          occurrence; rank1 = carry1 + r0 * W0(u), carry1 = 0 on paths 0, 1 and beta * W_user[u] on 2, 3
level 2   holders b of the a_k (item2user: listened order; item2session: user order, duplicates, first position), u left
          out on paths 0 and 3; K(b) = max k, pos(b) = b's first position in a_K's holder list (one max over
          k << 32 | ~pos); rank2 = carry2 + rank1 * P(a_K), carry2 = 0 on paths 0, 1, path 0's rank2 (beta for u) on
          path 2, path 1's rank2 on path 3
level 3   item c of the reached b's distinct lists (UL on paths 0, 2, S on 1, 3): parent = the b with the largest (K, pos)
          holding c; score(c) += rank2(parent) * W2(parent), in path order (fp64, products rounded before the add)
output    the reached items by (score desc, first insertion asc), insertion = (path, -K, -pos, j) of the first path
          reaching c, j = c's index in its parent's distinct list.  topn: without the user's own items, the first N.
Weights are Python floats computed exactly as the reference writes them.
"""
import numpy as np


def _distinct(seq):
    seen, out = set(), []
    for x in seq:
        if x not in seen:
            seen.add(x)
            out.append(x)
    return np.array(out, np.int64)


class Graph(object):
    """ev_ptr / ev_i: training events user-major in userRecord order; i2u: per item its users in listened order
    (default ascending user id)."""

    def __init__(self, ev_ptr, ev_i, n, rho, beta, eta, i2u=None):
        m = len(ev_ptr) - 1
        self.m, self.n = m, n
        self.UL = [list(map(int, ev_i[ev_ptr[u]:ev_ptr[u + 1]])) for u in range(m)]
        S = [ul[max(0, len(ul) - 10):] for ul in self.UL]
        self.D = [[_distinct(ul) for ul in self.UL], [_distinct(s) for s in S]]       # [0] user lists, [1] session lists
        if i2u is None:
            rows = [[] for _ in range(n)]
            for u in range(m):
                for c in self.D[0][u]:
                    rows[c].append(u)
            i2u = rows
        i2s = [[] for _ in range(n)]
        for u in range(m):
            for c in S[u]:
                i2s[c].append(u)
        # holder lists: (users, first positions) per item; item2user has no duplicates
        self.H = [[(np.array(r, np.int64), np.arange(len(r), dtype=np.int64)) for r in i2u], []]
        for r in i2s:
            users, pos = [], []
            for t, b in enumerate(r):
                if not users or users[-1] != b:
                    users.append(b)
                    pos.append(t)
            self.H[1].append((np.array(users, np.int64), np.array(pos, np.int64)))
        nU = [len(r) for r in i2u]
        nS = [len(r) for r in i2s]
        self.W = [np.array([1.0 / pow(len(ul), rho) if ul else 0.0 for ul in self.UL]),
                  np.array([1.0 / pow(len(s), rho) if s else 0.0 for s in S])]
        self.P = [np.array([pow(eta / (eta * nU[c] + nS[c]), rho) if nU[c] else 0.0 for c in range(n)]),
                  np.array([pow(1 / (eta * nU[c] + nS[c]), rho) if nU[c] else 0.0 for c in range(n)])]
        self.r = [beta, 1 - beta]


def predict(g, u):
    """(items int64, scores float64) of user u: every reached item by (score desc, first insertion asc)."""
    m, n = g.m, g.n
    score = np.zeros(n)
    ins = np.full((n, 4), -1, np.int64)                 # (p, -K, -pos, j) of the first reach; p = -1: unreached
    r2 = [np.zeros(m), np.zeros(m)]                     # rank2 of user / session nodes
    for p in range(4):
        start = 0 if p < 2 else 1                       # start list UL / S
        h = p & 1                                       # holder lists item2user / item2session; level 2 node type
        L1 = g.D[start][u]
        rank1 = (0.0 if p < 2 else g.r[0] * g.W[0][u]) + g.r[start] * g.W[start][u]
        if len(L1) == 0:
            continue
        parts = [g.H[h][a] for a in L1]
        b = np.concatenate([x[0] for x in parts])
        pos = np.concatenate([x[1] for x in parts])
        k = np.repeat(np.arange(1, len(L1) + 1, dtype=np.int64), [len(x[0]) for x in parts])
        keep = b != u if p in (0, 3) else np.ones(len(b), bool)
        key2 = np.zeros(m, np.int64)
        np.maximum.at(key2, b[keep], (k[keep] << 32) | (0xFFFFFFFF - pos[keep]))
        reached = np.flatnonzero(key2)
        K = key2[reached] >> 32
        pos2 = 0xFFFFFFFF - (key2[reached] & 0xFFFFFFFF)
        if p == 2:
            carry = np.where(reached == u, g.r[0], r2[0][reached])
        elif p == 3:
            carry = r2[1][reached]
        else:
            carry = np.zeros(len(reached))
        rank2 = carry + rank1 * g.P[h][L1[K - 1]]
        r2[h][reached] = rank2
        e3 = (K << 32) | pos2
        lists = [g.D[h][bb] for bb in reached]
        if not any(len(x) for x in lists):
            continue
        c = np.concatenate(lists)
        owner = np.repeat(np.arange(len(reached)), [len(x) for x in lists])
        j = np.concatenate([np.arange(len(x)) for x in lists])
        key3 = np.zeros(n, np.int64)
        np.maximum.at(key3, c, e3[owner])
        win = key3[c] == e3[owner]
        cw, ow = c[win], owner[win]
        score[cw] = score[cw] + rank2[ow] * g.W[h][reached[ow]]
        new = ins[cw, 0] < 0
        ins[cw[new]] = np.stack([np.full(new.sum(), p), -K[ow[new]], -pos2[ow[new]], j[win][new]], axis=1)
    items = np.flatnonzero(ins[:, 0] >= 0)
    order = np.lexsort((ins[items, 3], ins[items, 2], ins[items, 1], ins[items, 0], -score[items]))
    return items[order], score[items][order]


def topn(g, u, N):
    """predict(u) without u's own training items, the first N (may be shorter)."""
    items, scores = predict(g, u)
    keep = ~np.isin(items, g.D[0][u])
    return items[keep][:N], scores[keep][:N]


# the logs of the g12 fixtures (tools/make_ipf_goldens.py): synthetic text logs (users, items, events per user) of
# yue_amd.synth plus extras, the IPF options and the evaluation set-up
CASES = {
    'ipf_z': {'shape': (120, 200, 20), 'ipf': '-rho 1 -beta 0.7 -eta 0.3', 'eval': '-target track -byTime 0.2', 'topN': '5,10'},
    'ipf_b1': {'shape': (150, 600, 40), 'ipf': '-rho 0.5 -beta 1 -eta 1.5', 'eval': '-target track -byTime 0.2', 'topN': '10,20'},
    'ipf_rho2': {'shape': (150, 400, 30), 'ipf': '-rho 2 -beta 0.4 -eta 1.5', 'eval': '-target track -byTime 0.2', 'topN': '5,10'},
    'ipf_t': {'shape': (150, 500, 30), 'ipf': '-rho 1 -beta 0.7 -eta 0.3', 'eval': '-target track -testSet {test}', 'topN': '5,10'},
    'ipf_s': {'shape': (400, 600, 20), 'ipf': '-rho 1 -beta 0.7 -eta 0.3', 'eval': '-target track -byTime 0.2 -sample', 'topN': '5,10'},
}


def write_case_log(tag, path):
    """The text log(s) of one case; returns the test-set path of a -testSet case (else None).
    ipf_z: test-only users zu0..zu3 (one late event each), 'iso' alone on its own tracks (its list is empty once its own
    items go), 'one' with a single training event, and 'rep' playing track t7 thirty times.
    ipf_t: the synthetic log is slot-major (users interleaved in time); slots 0..23 train, the rest is the -testSet
    file: the training set is not grouped by user and item2user order is not user-id order."""
    from yue_amd import synth
    m, n, d = CASES[tag]['shape']
    if tag == 'ipf_t':
        rows = synth.text_events(m, n, d)
        test_path = path[:-4] + '_test.txt'
        with open(path, 'w') as f, open(test_path, 'w') as ft:
            for t, u, i, a in rows:
                (f if int(t) < int(d * 0.8) else ft).write('%s,%s,%s,%s\n' % (t, u, i, a))
        return test_path
    synth.write_text_log(path, m, n, d)
    if tag == 'ipf_z':
        with open(path, 'a') as f:
            for q in range(4):
                f.write('9999999999,zu%d,%s,a0\n' % (q, 'zt%d' % q if q < 2 else 't%d' % (q * 7)))
            for q in range(4):
                f.write('00000000%02d,iso,iso%d,a0\n' % (q, q % 3))
            f.write('0000009999,iso,t3,a0\n')
            f.write('0000000001,one,t11,a0\n0000009999,one,t12,a0\n')
            for q in range(30):
                f.write('00000001%02d,rep,t7,a0\n' % q)
            f.write('0000009999,rep,t9,a0\n')
    return None
