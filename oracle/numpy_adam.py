"""NumPy restatement of the reference's LIVE BPR path -- the TensorFlow-1 graph of recommender/cf/BPR.py:83-129
(embedding lookups, softplus loss, l2 terms, AdamOptimizer) -- TEST INFRASTRUCTURE.  SURVEY 8(a) row a9.

PARITY UNPINNED: TensorFlow is not installable here, so nothing in this file has been checked against the reference's
own execution; it restates the graph as written in the reference and the documented behaviour of the TF-1 ops it names:
  * tf.nn.embedding_lookup gradients are IndexedSlices; the optimizer sums duplicate indices first;
  * tf.nn.l2_loss(x) = sum(x**2) / 2 over every gathered row (a row gathered 100 times counts 100 times);
  * tf.train.AdamOptimizer (beta1 0.9, beta2 0.999, epsilon 1e-8) on IndexedSlices: m <- beta1*m, then the summed
    gradient rows are scatter-added with (1-beta1); v likewise with the squares; var <- var - lr_t * m / (sqrt(v) + eps)
    for ALL rows, lr_t = lr * sqrt(1 - beta2^t) / (1 - beta1^t) -- i.e. dense Adam with a zero gradient on untouched rows;
  * everything in float32.
The device path (yue_adam_step) is compared with THIS restatement (tests/test_gpu_adam.py).
"""
import numpy as np

BETA1, BETA2, EPS = np.float32(0.9), np.float32(0.999), np.float32(1e-8)


def softplus(x):
    x = x.astype(np.float32)
    return (np.maximum(x, 0) + np.log1p(np.exp(-np.abs(x)))).astype(np.float32)


def sigmoid(x):
    x = x.astype(np.float32)
    return (np.float32(1) / (np.float32(1) + np.exp(-x))).astype(np.float32)


def loss_and_grad(U, V, u_idx, i_idx, j_idx, reg, dtype=np.float32):
    """(total_loss, gU [m,k], gV [n,k]) of the graph of BPR.py:101-107 on the fed triplets: in np.float32 statement for statement
    what adam_step differentiates (duplicate rows summed in feed order), in np.float64 the yardstick of the same graph."""
    one, reg = dtype(1), dtype(reg)
    U, V = U.astype(dtype, copy=False), V.astype(dtype, copy=False)
    Ue, Ve, Ne = U[u_idx], V[i_idx], V[j_idx]
    err = (Ue * Ve).sum(axis=1) - (Ue * Ne).sum(axis=1)                      # :101
    with np.errstate(over='ignore'):                                         # exp beyond the format: inf, and 1 / (1 + inf) = 0
        loss = (np.maximum(-err, 0) + np.log1p(np.exp(-np.abs(err)))).astype(dtype).sum(dtype=dtype)              # :102
        loss = loss + reg * ((Ue * Ue).sum(dtype=dtype) + (Ve * Ve).sum(dtype=dtype) + (Ne * Ne).sum(dtype=dtype)) / dtype(2)    # :104-107
        g = -(one / (one + np.exp(err))).astype(dtype)                       # d softplus(-e) / d e = -sigmoid(-e)
    gU = np.zeros(U.shape, dtype)
    gV = np.zeros(V.shape, dtype)
    np.add.at(gU, u_idx, g[:, None] * (Ve - Ne) + reg * Ue)
    np.add.at(gV, i_idx, g[:, None] * Ue + reg * Ve)
    np.add.at(gV, j_idx, -g[:, None] * Ue + reg * Ne)
    return loss, gU, gV


def bounds(U, V, u_idx, i_idx, j_idx, reg):
    """(loss_bound, bU [m,k], bV [n,k]), all in fp64: how far float32 rounding can carry the loss and each gradient element from
    the fp64 graph, in ANY order of summation.  Per element of a row with c contributions (a user row: its triplets; an item row:
    every triplet that names it as i or as j, a triplet with i == j twice)

        bound = 2^-24 * ((c + 8) * A + B)

    A = the sum of the contributions' magnitudes, |a_t| (|V_i| + |V_j|) + reg |U_u| on a user row and |a_t| |U_u| + reg |V_.| on an
    item row, a_t = -sigmoid(-x_t): c - 1 additions of partial sums that never exceed A, and 8 ulps for one term's own arithmetic
    (expf, the add and the division behind a_t; the subtraction, two products and an add); the ulp left over carries the one
    rounding of whoever reads the sum back through a product.
    B = the reach of the margin's own rounding through the sigmoid, whose slope is at most 1/4: x_t is two k-long float32 dot
    products and a subtraction, off by at most 2^-24 (k + 2) (|U_u|.|V_i| + |U_u|.|V_j|); that, times 1/4, times the
    contribution's row factor (|V_i| + |V_j|, or |U_u|), summed over the contributions.  It enters once: it is no rounding of the sum.

    The loss: per triplet 8 ulps of its softplus, k + 4 ulps of its three l2 terms and the margin's rounding itself (softplus has
    slope at most 1), summed -- the device adds the per-triplet float32 terms in double."""
    U, V, reg = U.astype(np.float64), V.astype(np.float64), float(reg)
    k = U.shape[1]
    ulp = 2.0 ** -24
    Ue, Ve, Ne = U[u_idx], V[i_idx], V[j_idx]
    x = (Ue * Ve).sum(axis=1) - (Ue * Ne).sum(axis=1)
    a = (1.0 / (1.0 + np.exp(x)))[:, None]
    aU, aVe, aNe = np.abs(Ue), np.abs(Ve), np.abs(Ne)
    dx = ((k + 2) * ((aU * aVe).sum(axis=1) + (aU * aNe).sum(axis=1)))[:, None]            # in ulps
    cU, cV = np.bincount(u_idx, minlength=len(U)), np.bincount(i_idx, minlength=len(V)) + np.bincount(j_idx, minlength=len(V))
    AU, BU, AV, BV = np.zeros_like(U), np.zeros_like(U), np.zeros_like(V), np.zeros_like(V)
    np.add.at(AU, u_idx, a * (aVe + aNe) + reg * aU)
    np.add.at(BU, u_idx, 0.25 * dx * (aVe + aNe))
    for idx, rows in ((i_idx, aVe), (j_idx, aNe)):
        np.add.at(AV, idx, a * aU + reg * rows)
        np.add.at(BV, idx, 0.25 * dx * aU)
    softplus64 = np.maximum(-x, 0) + np.log1p(np.exp(-np.abs(x)))
    l2 = 0.5 * reg * ((Ue * Ue).sum(axis=1) + (Ve * Ve).sum(axis=1) + (Ne * Ne).sum(axis=1))
    loss_bound = ulp * float((8 * softplus64 + (k + 4) * l2 + dx[:, 0]).sum())
    return loss_bound, ulp * ((cU[:, None] + 8) * AU + BU), ulp * ((cV[:, None] + 8) * AV + BV)


def adam_step(U, V, state, u_idx, i_idx, j_idx, lr, reg, t):
    """One `sess.run(train, total_loss)` of BPR.py:124 on the fed (u, i, j) triplets.  In place on U [m,k], V [n,k]
    (float32) and on state = dict(mU, vU, mV, vV), zeros before the first step; t = 1, 2, ... Returns total_loss."""
    loss, gU, gV = loss_and_grad(U, V, u_idx, i_idx, j_idx, reg, np.float32)
    lr_t = np.float32(lr * np.sqrt(1.0 - float(BETA2) ** t) / (1.0 - float(BETA1) ** t))
    for var, grad, m, v in ((U, gU, state['mU'], state['vU']), (V, gV, state['mV'], state['vV'])):
        m *= BETA1
        m += (np.float32(1) - BETA1) * grad
        v *= BETA2
        v += (np.float32(1) - BETA2) * grad * grad
        var -= lr_t * m / (np.sqrt(v) + EPS)
    return float(loss)


def new_state(U, V):
    return {'mU': np.zeros_like(U), 'vU': np.zeros_like(U), 'mV': np.zeros_like(V), 'vV': np.zeros_like(V)}


def truncated_normal(rs, shape, stddev):
    """tf.truncated_normal: normal(0, stddev), values beyond two standard deviations are drawn again (the stream of a
    NumPy RandomState -- TF's own generator is not reproducible here)."""
    x = rs.normal(0.0, stddev, size=shape)
    bad = np.abs(x) > 2 * stddev
    while bad.any():
        x[bad] = rs.normal(0.0, stddev, size=int(bad.sum()))
        bad = np.abs(x) > 2 * stddev
    return x.astype(np.float32)
