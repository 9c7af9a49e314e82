"""NumPy restatement of the reference's LightGCN (recommender/advanced/LightGCN.py) -- TEST INFRASTRUCTURE.

PARITY UNPINNED: TensorFlow is not installable here and the reference's base/DeepRecommender.py is missing, so nothing in this
file has been checked against the reference's own execution.  It restates the graph as written:
  graph     square, m + n rows; every training EVENT adds (u, m + i) and (m + i, u) with value count(u, i); repeated indices
            are summed by sparse_tensor_dense_matmul, so a pair listened c times weighs c * c; no degree normalisation (:29-34)
  layers    E_0 = [U; V], E_l = A E_{l-1} (the unnormalised product is carried on), F = E_0 + sum_l l2_normalize(E_l),
            l2_normalize(x) = x * rsqrt(max(sum x^2, 1e-12))                                                         (:38-45)
  batches   events in order in slices of batch_size; 5 negatives drawn per event, the LAST one kept (the appends sit outside
            the inner loop): one triplet per event                                                                   (:56-79)
  loss      -sum log sigmoid(F_u.F_i - F_u.F_j) + reg (l2_loss(F_u) + l2_loss(F_i) + l2_loss(F_j)), l2_loss = sum x^2 / 2  (:83-88)
  update    dense Adam on U and V (the gradients pass through the matmul), as oracle/numpy_adam.py forms it
Every function takes dtype = np.float64 (the yardstick) or np.float32 (statement by statement, as TensorFlow computes).
The backward pass is written out by hand and checked against central differences (tests/test_lightgcn_golden.py).
"""
import random as _random

import numpy as np

EPS = 1e-12
BETA1, BETA2, ADAM_EPS = 0.9, 0.999, 1e-8


def graph_from_events(ev_u, ev_i, m, n):
    """The reference's index / value lists (:29-32) and what the matmul makes of them: the sorted unique pairs of both
    sides with the summed weight c * c."""
    ev_u, ev_i = np.asarray(ev_u, np.int64), np.asarray(ev_i, np.int64)
    count = {}
    for u, i in zip(ev_u.tolist(), ev_i.tolist()):
        count[(u, i)] = count.get((u, i), 0) + 1
    indices = [[u, m + i] for u, i in zip(ev_u.tolist(), ev_i.tolist())] + [[m + i, u] for u, i in zip(ev_u.tolist(), ev_i.tolist())]
    values = [float(count[(u, i)]) for u, i in zip(ev_u.tolist(), ev_i.tolist())] * 2
    pairs = sorted(count)
    pu = np.array([p[0] for p in pairs], np.int64).reshape(-1)
    pi = np.array([p[1] for p in pairs], np.int64).reshape(-1)
    w = np.array([float(count[p]) ** 2 for p in pairs], np.float32).reshape(-1)      # c entries of value c each
    g = graph_from_pairs(pu, pi, w, m, n)
    g['indices'], g['values'] = indices, values
    return g


def graph_from_pairs(pu, pi, w, m, n):
    """Both sides' sorted lists of unique (user, item, weight) pairs, and the CSR of the whole (m + n)-row matrix."""
    pu, pi, w = np.asarray(pu, np.int64), np.asarray(pi, np.int64), np.asarray(w, np.float32)
    o = np.lexsort((pi, pu))
    u_ptr = np.zeros(m + 1, np.int64)
    np.add.at(u_ptr, pu + 1, 1)
    u_ptr = np.cumsum(u_ptr)
    o2 = np.lexsort((pu, pi))
    i_ptr = np.zeros(n + 1, np.int64)
    np.add.at(i_ptr, pi + 1, 1)
    i_ptr = np.cumsum(i_ptr)
    g = {'m': m, 'n': n, 'u_ptr': u_ptr, 'u_items': pi[o].astype(np.int32), 'u_w': w[o], 'i_ptr': i_ptr, 'i_users': pu[o2].astype(np.int32),
         'i_w': w[o2]}
    g['ptr'] = np.concatenate([u_ptr, u_ptr[-1] + i_ptr[1:]])
    g['col'] = np.concatenate([m + pi[o], pu[o2]]).astype(np.int64)
    g['w'] = np.concatenate([w[o], w[o2]])
    g['degree'] = np.diff(g['ptr'])
    return g


def spmm(g, X):
    """A X in X's dtype: the products, then one sum per row."""
    out = np.zeros_like(X)
    if len(g['col']) == 0:
        return out
    prod = g['w'].astype(X.dtype)[:, None] * X[g['col']]
    rows = np.flatnonzero(g['degree'] > 0)
    out[rows] = np.add.reduceat(prod, g['ptr'][rows], axis=0)
    return out


def propagate(g, U, V, layers=3, dtype=np.float64):
    """(raw layers E_0 .. E_L, their row sums of squares [L + 1][N], F)."""
    E = [np.concatenate([U, V]).astype(dtype)]
    ss = [(E[0] * E[0]).sum(axis=1)]
    F = E[0].copy()
    for _ in range(layers):
        x = spmm(g, E[-1])
        s = (x * x).sum(axis=1)
        F = F + x * (dtype(1) / np.sqrt(np.maximum(s, dtype(EPS))))[:, None]
        E.append(x)
        ss.append(s)
    return E, ss, F


def _sigmoid(x):
    return (x.dtype.type(1) / (x.dtype.type(1) + np.exp(-x))).astype(x.dtype)


def batch_loss_and_G(F, m, u, i, j, reg, dtype=np.float64):
    """(loss, G = dLoss / dF) of the fed triplets; duplicates sum."""
    u, i, j = np.asarray(u, np.int64), np.asarray(i, np.int64), np.asarray(j, np.int64)
    reg = dtype(reg)
    Fu, Fi, Fj = F[u], F[m + i], F[m + j]
    y = (Fu * Fi).sum(axis=1) - (Fu * Fj).sum(axis=1)
    if dtype == np.float64:
        nll = np.logaddexp(0.0, -y).sum()
    else:
        nll = -np.log(_sigmoid(y)).sum(dtype=dtype)                              # tf.log(tf.sigmoid(y)), :86
    l2 = (Fu * Fu).sum(dtype=dtype) / dtype(2) + (Fi * Fi).sum(dtype=dtype) / dtype(2) + (Fj * Fj).sum(dtype=dtype) / dtype(2)
    loss = nll + reg * l2
    c = (-_sigmoid(-y))[:, None]                                                 # d(-log sigmoid(y)) / dy
    G = np.zeros_like(F)
    np.add.at(G, u, c * (Fi - Fj) + reg * Fu)
    np.add.at(G, m + i, c * Fu + reg * Fi)
    np.add.at(G, m + j, -c * Fu + reg * Fj)
    return dtype(loss), G


def normalize_backward(x, s, g, dtype):
    """J(g) of x * rsqrt(max(sum x^2, 1e-12)) row by row."""
    live = s >= dtype(EPS)
    rinv = dtype(1) / np.sqrt(np.where(live, s, dtype(1)))
    nh = x * rinv[:, None]
    out = (g - nh * (nh * g).sum(axis=1)[:, None]) * rinv[:, None]
    return np.where(live[:, None], out, g * dtype(1e6)).astype(dtype)


def loss_and_grad(g, U, V, u, i, j, reg, layers=3, dtype=np.float64):
    """(loss, dLoss / dU, dLoss / dV, F, raw layers)."""
    m = g['m']
    E, ss, F = propagate(g, U, V, layers, dtype)
    loss, G = batch_loss_and_G(F, m, u, i, j, reg, dtype)
    gE = normalize_backward(E[layers], ss[layers], G, dtype)
    for l in range(layers - 1, 0, -1):
        gE = normalize_backward(E[l], ss[l], G, dtype) + spmm(g, gE)             # A is symmetric
    g0 = G + spmm(g, gE)
    return loss, g0[:m], g0[m:], F, E


def new_state(U, V):
    return {'mU': np.zeros_like(U), 'vU': np.zeros_like(U), 'mV': np.zeros_like(V), 'vV': np.zeros_like(V)}


def adam(var, grad, m, v, lr, t, dtype=np.float64):
    """tf.train.AdamOptimizer's dense apply, in place (statement for statement oracle/numpy_adam.py's)."""
    b1, b2, eps = dtype(BETA1), dtype(BETA2), dtype(ADAM_EPS)
    lr_t = dtype(lr * np.sqrt(1.0 - BETA2 ** t) / (1.0 - BETA1 ** t))
    grad = grad.astype(dtype)
    m *= b1
    m += (dtype(1) - b1) * grad
    v *= b2
    v += (dtype(1) - b2) * grad * grad
    var -= lr_t * m / (np.sqrt(v) + eps)


def step(g, U, V, state, u, i, j, lr, reg, t, layers=3, dtype=np.float64):
    """One sess.run([train, loss]) of :98, in place on U, V and state.  Returns the loss."""
    loss, gU, gV, _, _ = loss_and_grad(g, U, V, u, i, j, reg, layers, dtype)
    adam(U, gU, state['mU'], state['vU'], lr, t, dtype)
    adam(V, gV, state['mV'], state['vV'], lr, t, dtype)
    return loss


def next_batch_pairwise(ev_u, ev_i, listened, n, batch_size, negatives=5, rng=_random):
    """:56-79 on ids: events in order in slices of batch_size (the last one short); per event `negatives` rejection-sampled
    items by rng.randint, of which the last one is kept.  listened[u] = the set of the user's item ids."""
    train_size = len(ev_u)
    batch_id = 0
    while batch_id < train_size:
        end = min(batch_id + batch_size, train_size)
        u_idx, i_idx, j_idx = [], [], []
        for t in range(batch_id, end):
            user = int(ev_u[t])
            item_j = None
            for _ in range(negatives):
                item_j = rng.randint(0, n - 1)
                while item_j in listened[user]:
                    item_j = rng.randint(0, n - 1)
            u_idx.append(user)
            i_idx.append(int(ev_i[t]))
            j_idx.append(item_j)
        batch_id = end
        yield u_idx, i_idx, j_idx


def rel(a, b):
    """max-norm distance of a from the yardstick b, relative to b's max-norm."""
    b = np.asarray(b, np.float64)
    scale = np.abs(b).max()
    return float(np.abs(np.asarray(a, np.float64) - b).max() / (scale if scale > 0 else 1.0))


def truncated_normal(rs, shape, stddev=0.005):
    x = rs.normal(0.0, stddev, size=shape)
    bad = np.abs(x) > 2 * stddev
    while bad.any():
        x[bad] = rs.normal(0.0, stddev, size=int(bad.sum()))
        bad = np.abs(x) > 2 * stddev
    return x.astype(np.float32)


def synthetic_pairs(rs, m, n, degrees, weights=(1.0,)):
    """Unique (user, item, weight) pairs: user u gets degrees[u] distinct items; weights drawn from `weights`."""
    pu, pi = [], []
    for u, d in enumerate(degrees):
        items = rs.choice(n, size=int(d), replace=False)
        pu += [u] * int(d)
        pi += items.tolist()
    w = rs.choice(np.asarray(weights, np.float32), size=len(pu))
    return np.asarray(pu, np.int64), np.asarray(pi, np.int64), w.astype(np.float32)
