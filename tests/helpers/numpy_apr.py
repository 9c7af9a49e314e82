"""NumPy restatement of the reference's APR (recommender/advanced/APR.py) -- TEST INFRASTRUCTURE.

PARITY UNPINNED: TensorFlow is not installable here and the reference's base/DeepRecommender has no .py suffix, so nothing in this
file has been checked against the reference's own execution; the goldens tests/golden/g21_apr_*.json pin this contract, not
TensorFlow.  What it restates (line numbers are APR.py's):
  set-up      U [m,k], V [n,k] truncated_normal(stddev 0.005), U drawn first; the perturbations adv_U, adv_V start at zero   (:27-28)
  batch       batch_size events by np.random.randint over the training events; per event 3 negatives by random.randint with
              rejection against the user's items; one triplet per negative, T = 3 batch_size                              (:95-111)
  margins     x = U_u.V_i - U_u.V_j;  x_adv the same on U + adv_U, V + adv_V                                               (:36-47)
  phase 1     total_loss = sum softplus(-x) + regU l2_loss(U_e) + regU l2_loss(V_e) + regU l2_loss(U_e): the user rows twice,
              the positive rows once, the negative rows never, regU for all three                                         (:61-67)
  phase 2     loss_adv = sum softplus(-x) + regA sum softplus(-x_adv), no l2 term                                         (:69-70)
              adv <- l2_normalize(d loss_adv / d adv, axis 1) * eps at the CURRENT adv, l2_normalize(g) = g * rsqrt(max(sum g^2,
              1e-12)); the assign overwrites the whole variable, so rows outside the batch become 0; both gradients are taken
              before either assign                                                                                        (:49-58)
              then one Adam step on loss_adv with respect to U and V at the new adv, by the optimizer of phase 1: its moments
              and its step count run on                                                                                   (:72-76)
  gradients   TensorFlow's decomposition: d softplus(-x) / dx = -sigmoid(-x); regA enters as the upstream gradient of the sum, so
              the perturbed terms carry -(regA sigmoid(-x_adv)); duplicate rows are summed in feed order (a triplet's positive
              row before its negative one)
  update      dense Adam on U and V: every row moves (numpy_lightgcn.adam, which states oracle/numpy_adam.py's rule)
Every function takes dtype = np.float64 (the yardstick) or np.float32 (statement by statement).  The gradients are written out by
hand and checked against central differences (tests/test_apr_golden.py).
"""
import random as _random

import numpy as np

from . import numpy_lightgcn as nl

NORM_EPS = 1e-12
NEGATIVES = 3

rel = nl.rel
adam = nl.adam
new_state = nl.new_state
truncated_normal = nl.truncated_normal


def _ids(u, i, j):
    return np.asarray(u, np.int64), np.asarray(i, np.int64), np.asarray(j, np.int64)


def _softplus(x):
    return (np.maximum(x, x.dtype.type(0)) + np.log1p(np.exp(-np.abs(x)))).astype(x.dtype)


def _sigmoid(x):
    one = x.dtype.type(1)
    return (one / (one + np.exp(-x))).astype(x.dtype)


def _margin(Ue, Ve, Ne, dtype):
    return ((Ue * Ve).sum(axis=1, dtype=dtype) - (Ue * Ne).sum(axis=1, dtype=dtype)).astype(dtype)


def _scatter_users(shape, u, terms, dtype):
    g = np.zeros(shape, dtype)
    np.add.at(g, u, terms)
    return g


def _scatter_items(shape, i, j, pos, neg, dtype):
    """Both roles' terms summed in feed order: triplet by triplet, the positive row's term before the negative row's."""
    g = np.zeros(shape, dtype)
    np.add.at(g, np.stack([i, j], axis=1).reshape(-1), np.stack([pos, neg], axis=1).reshape(-1, shape[1]))
    return g


# ---- phase 1 ----------------------------------------------------------------------------------------------------------------
def pre_loss_and_grad(U, V, u, i, j, reg, dtype=np.float64):
    """(total_loss, d / dU, d / dV) of :61-67."""
    u, i, j = _ids(u, i, j)
    U, V, reg = U.astype(dtype), V.astype(dtype), dtype(reg)
    Ue, Ve, Ne = U[u], V[i], V[j]
    x = _margin(Ue, Ve, Ne, dtype)
    l2u, l2v = (Ue * Ue).sum(dtype=dtype) / dtype(2), (Ve * Ve).sum(dtype=dtype) / dtype(2)
    loss = _softplus(-x).sum(dtype=dtype) + ((reg * l2u + reg * l2v) + reg * l2u)
    a = (-_sigmoid(-x))[:, None]
    gU = _scatter_users(U.shape, u, (a * Ve - a * Ne) + (dtype(2) * reg) * Ue, dtype)
    gV = _scatter_items(V.shape, i, j, a * Ue + reg * Ve, -(a * Ue), dtype)
    return dtype(loss), gU, gV


# ---- phase 2 ----------------------------------------------------------------------------------------------------------------
def _adv(U, V, dU, dV, u, i, j, regA, dtype):
    U, V, dU, dV = U.astype(dtype), V.astype(dtype), dU.astype(dtype), dV.astype(dtype)
    Ue, Ve, Ne = U[u], V[i], V[j]
    W, Yi, Yj = Ue + dU[u], Ve + dV[i], Ne + dV[j]
    x, xa = _margin(Ue, Ve, Ne, dtype), _margin(W, Yi, Yj, dtype)
    return U, V, Ue, Ve, Ne, W, Yi, Yj, x, xa


def adv_loss(U, V, dU, dV, u, i, j, regA, dtype=np.float64):
    u, i, j = _ids(u, i, j)
    x, xa = _adv(U, V, dU, dV, u, i, j, regA, dtype)[-2:]
    return dtype(_softplus(-x).sum(dtype=dtype) + dtype(regA) * _softplus(-xa).sum(dtype=dtype))


def delta_grad(U, V, dU, dV, u, i, j, regA, dtype=np.float64, norms=False):
    """(d loss_adv / d adv_U, d loss_adv / d adv_V), dense: zero outside the batch.  With norms also, per row of either, the sum
    of its terms' 2-norms (what the row's own norm is held against in the tests' conditioning statement)."""
    u, i, j = _ids(u, i, j)
    U, V, Ue, Ve, Ne, W, Yi, Yj, x, xa = _adv(U, V, dU, dV, u, i, j, regA, dtype)
    c = (-(dtype(regA) * _sigmoid(-xa)))[:, None]
    tu, tp, tn = c * Yi - c * Yj, c * W, -(c * W)
    gU, gV = _scatter_users(U.shape, u, tu, dtype), _scatter_items(V.shape, i, j, tp, tn, dtype)
    if not norms:
        return gU, gV
    nU, nV = np.zeros(U.shape[0]), np.zeros(V.shape[0])
    np.add.at(nU, u, np.linalg.norm(tu.astype(np.float64), axis=1))
    np.add.at(nV, i, np.linalg.norm(tp.astype(np.float64), axis=1))
    np.add.at(nV, j, np.linalg.norm(tn.astype(np.float64), axis=1))
    return gU, gV, nU, nV


def normalize(g, eps, dtype=np.float64):
    """tf.nn.l2_normalize(g, 1) * eps: a zero row stays exactly zero."""
    g = g.astype(dtype)
    ss = (g * g).sum(axis=1, dtype=dtype)
    return ((g * (dtype(1) / np.sqrt(np.maximum(ss, dtype(NORM_EPS))))[:, None]) * dtype(eps)).astype(dtype)


def delta_update(U, V, dU, dV, u, i, j, eps, regA, dtype=np.float64):
    """The first sess.run of a phase-2 step: (raw gU, raw gV, new adv_U, new adv_V).  Both gradients from the old values."""
    gU, gV = delta_grad(U, V, dU, dV, u, i, j, regA, dtype)
    return gU, gV, normalize(gU, eps, dtype), normalize(gV, eps, dtype)


def adv_loss_and_grad(U, V, dU, dV, u, i, j, regA, dtype=np.float64):
    """(loss_adv, d / dU, d / dV) at the given perturbation, which is not trainable."""
    u, i, j = _ids(u, i, j)
    U, V, Ue, Ve, Ne, W, Yi, Yj, x, xa = _adv(U, V, dU, dV, u, i, j, regA, dtype)
    loss = _softplus(-x).sum(dtype=dtype) + dtype(regA) * _softplus(-xa).sum(dtype=dtype)
    a, b = (-_sigmoid(-x))[:, None], (-(dtype(regA) * _sigmoid(-xa)))[:, None]
    gU = _scatter_users(U.shape, u, (a * Ve - a * Ne) + (b * Yi - b * Yj), dtype)
    pos = a * Ue + b * W
    gV = _scatter_items(V.shape, i, j, pos, -pos, dtype)
    return dtype(loss), gU, gV


# ---- steps ------------------------------------------------------------------------------------------------------------------
def pre_step(U, V, state, u, i, j, lr, reg, t, dtype=np.float64):
    """One sess.run([train, total_loss]) of :122, in place on U, V and state.  Returns the loss."""
    loss, gU, gV = pre_loss_and_grad(U, V, u, i, j, reg, dtype)
    adam(U, gU, state['mU'], state['vU'], lr, t, dtype)
    adam(V, gV, state['mV'], state['vV'], lr, t, dtype)
    return loss


def adv_step(U, V, D, state, u, i, j, lr, eps, regA, t, dtype=np.float64):
    """The two sess.run calls of :131-133, in place on U, V, state and D = {'dU', 'dV'} (dense, whole-variable assign).  t is the
    optimizer's step: it runs on from phase 1 (maxIter + e + 1).  Returns loss_adv."""
    _, _, D['dU'], D['dV'] = delta_update(U, V, D['dU'], D['dV'], u, i, j, eps, regA, dtype)
    loss, gU, gV = adv_loss_and_grad(U, V, D['dU'], D['dV'], u, i, j, regA, dtype)
    adam(U, gU, state['mU'], state['vU'], lr, t, dtype)
    adam(V, gV, state['mV'], state['vV'], lr, t, dtype)
    return loss


def new_delta(U, V, dtype=np.float64):
    return {'dU': np.zeros(U.shape, dtype), 'dV': np.zeros(V.shape, dtype)}


def train(U0, V0, batches, max_iter, lr, reg, eps, regA, dtype=np.float64):
    """Both phases on the given batches (max_iter phase-1 ones, then the adversarial ones).  Returns (U, V, losses)."""
    U, V = U0.astype(dtype), V0.astype(dtype)
    st, D, losses = new_state(U, V), new_delta(U0, V0, dtype), []
    for t, (u, i, j) in enumerate(batches, 1):
        if t <= max_iter:
            losses.append(float(pre_step(U, V, st, u, i, j, lr, reg, t, dtype)))
        else:
            losses.append(float(adv_step(U, V, D, st, u, i, j, lr, eps, regA, t, dtype)))
    return U, V, losses


# ---- sampler ----------------------------------------------------------------------------------------------------------------
def next_batch(ev_u, ev_i, listened, n, batch_size, negatives=NEGATIVES, np_rng=np.random, rng=_random):
    """:95-111 on ids: first all batch_size event indices by np_rng.randint, then per event `negatives` draws of
    rng.randint(0, n - 1), each rejected while the item is one of the user's (listened[u]: the set of the user's item ids)."""
    batch_idx = np_rng.randint(len(ev_u), size=batch_size)
    u_idx, i_idx, j_idx = [], [], []
    for idx in batch_idx:
        user = int(ev_u[idx])
        for _ in range(negatives):
            item_j = rng.randint(0, n - 1)
            while item_j in listened[user]:
                item_j = rng.randint(0, n - 1)
            u_idx.append(user)
            i_idx.append(int(ev_i[idx]))
            j_idx.append(item_j)
    return u_idx, i_idx, j_idx


def checksum(a):
    """Position-weighted sum of an array as a float: what the goldens hold in place of the array."""
    a = np.asarray(a, np.float64).reshape(-1)
    return float((a * (1.0 + (np.arange(a.size) % 97) / 97.0)).sum())
