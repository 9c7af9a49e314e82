"""NumPy restatement of the reference's NGCF (recommender/advanced/NGCF.py) -- TEST INFRASTRUCTURE.

PARITY UNPINNED: TensorFlow is not installable here and the reference's base/DeepRecommender.py is missing, so nothing in this
file has been checked against the reference's own execution.  It restates the graph as written:
  counts    userListen[u][t] starts at 1 on first sight and is then incremented: a pair with c events holds c + 1      (:48-54)
  graph     square, N = m + n rows; every training EVENT adds (u, m + t) and (m + u, t) -- the second block is NOT the
            transpose -- with value (c + 1) / sqrt(events of u) / sqrt(events of t); repeated indices are summed by the
            matmul, so a pair weighs c (c + 1) / sqrt(d_u) / sqrt(d_t).  Formed here in Python doubles and rounded once to
            float32; TensorFlow's c sequential float32 additions may differ in the last bits.  form='symmetric' puts
            (m + t, u) in the second block, the formula of :64's comment                                               (:62-73)
  layers    E_0 = [U; V]; S = A E; Z = (S + E) W_1 + (E o S) W_2; H = leaky_relu(Z, 0.2); D = training ? H / keep * mask : H;
            E_l = D (dropped, unnormalised); N_l = l2_normalize(D); F = [E_0 | N_1 | .. | N_L]                         (:90-113)
  mask      TensorFlow's cannot be reproduced; this contract's keeps element (row, column) of layer l (0-based) at `step`
            when cnet_hash(seed ^ TAG, step, l, row, column) >> 40 < floor(keep * 2^24)
  batches   events in order in slices of batch_size, the last one short; one negative per event by random.choice over
            list(trackRecord.keys()); the rejection test compares a track name with record dicts and is never true     (:16-41)
  loss      numpy_lightgcn's on the wide F; dense Adam on U, V and the six weights                                       (:124-141)
Every function takes dtype = np.float64 (the yardstick) or np.float32 (statement by statement).  The backward pass is written
out by hand and checked against central differences (tests/test_ngcf_golden.py).
"""
import math
import random as _random

import numpy as np

from . import numpy_lightgcn as nl

EPS = nl.EPS
SLOPE = 0.2
TAG = 0x4E474346
M64 = (1 << 64) - 1

rel = nl.rel
adam = nl.adam
truncated_normal = nl.truncated_normal


# ---- graph ---------------------------------------------------------------------------------------------------------------
def graph_from_events(ev_u, ev_t, m, n, form='written', du=None, dt=None):
    """The reference's index / value lists and the CSR the matmul makes of them.  With form='written' and a user id >= n the
    second block names a row >= m + n: 'out_of_range' lists such rows and no CSR is built.  du / dt: len(userRecord[u]) and
    len(trackRecord[t]) by id where they are not the events' own counts (under -byTime the records hold the training side only,
    the events the whole log); a zero length gives the value 0 (:67-68)."""
    ev_u, ev_t = [int(x) for x in ev_u], [int(x) for x in ev_t]
    count, cu, ct = {}, {}, {}
    for u, t in zip(ev_u, ev_t):
        count[(u, t)] = count.get((u, t), 0) + 1
        cu[u] = cu.get(u, 0) + 1
        ct[t] = ct.get(t, 0) + 1
    du, dt = cu if du is None else du, ct if dt is None else dt

    def value(u, t):
        return 0.0 if du[u] == 0 or dt[t] == 0 else float(count[(u, t)] + 1) / math.sqrt(du[u]) / math.sqrt(dt[t])
    indices = [[u, m + t] for u, t in zip(ev_u, ev_t)]
    if form == 'written':
        indices += [[m + u, t] for u, t in zip(ev_u, ev_t)]
    else:
        indices += [[m + t, u] for u, t in zip(ev_u, ev_t)]
    values = [value(u, t) for u, t in zip(ev_u, ev_t)] * 2
    g = {'m': m, 'n': n, 'form': form, 'indices': indices, 'values': values}
    g['out_of_range'] = sorted({r for r, _ in indices if r >= m + n})
    if g['out_of_range']:
        return g
    pairs = sorted(count)
    pu = np.array([p[0] for p in pairs], np.int64).reshape(-1)
    pt = np.array([p[1] for p in pairs], np.int64).reshape(-1)
    w = np.array([count[p] * value(*p) for p in pairs], np.float64).astype(np.float32).reshape(-1)
    g.update(graph_from_pairs(pu, pt, w, m, n, form))
    return g


def graph_from_pairs(pu, pt, w, m, n, form='written'):
    """CSR of both blocks from unique (user, track, weight) pairs, and the transpose's."""
    pu, pt, w = np.asarray(pu, np.int64), np.asarray(pt, np.int64), np.asarray(w, np.float32)
    assert form in ('written', 'symmetric')
    if form == 'written':
        assert len(pu) == 0 or pu.max() < n, 'a user id >= n names a row >= m + n'
        rows, cols = np.concatenate([pu, m + pu]), np.concatenate([m + pt, pt])
    else:
        rows, cols = np.concatenate([pu, m + pt]), np.concatenate([m + pt, pu])
    ww = np.concatenate([w, w])
    g = {'m': m, 'n': n, 'form': form}
    g.update(csr(rows, cols, ww, m + n))
    g['T'] = csr(cols, rows, ww, m + n)
    return g


def csr(rows, cols, w, N):
    o = np.lexsort((cols, rows))
    ptr = np.zeros(N + 1, np.int64)
    np.add.at(ptr, rows + 1, 1)
    ptr = np.cumsum(ptr)
    return {'ptr': ptr, 'col': cols[o].astype(np.int64), 'w': w[o].astype(np.float32), 'degree': np.diff(ptr)}


spmm = nl.spmm


# ---- mask ----------------------------------------------------------------------------------------------------------------
def _mix(z):
    z = z ^ (z >> np.uint64(30)); z = z * np.uint64(0xBF58476D1CE4E5B9)
    z = z ^ (z >> np.uint64(27)); z = z * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def mask_bits(seed, step, layer, N, k):
    """The top 24 bits of cnet_hash(seed ^ TAG, step, layer, row, column) for every element of an [N, k] layer."""
    with np.errstate(over='ignore'):
        head = ((int(seed) ^ TAG) + 0x9E3779B97F4A7C15 * (int(step) + 1)) & M64
        z = _mix(np.array([head], np.uint64))
        rows = np.arange(N, dtype=np.uint64)
        z = _mix(z ^ (np.uint64((0xD1B54A32D192ED03 * (int(layer) + 1)) & M64) + np.uint64(0x8CB92BA72F3D8DD7) * rows))
        cols = np.arange(k, dtype=np.uint64)
        z = _mix(z[:, None] ^ (np.uint64(0xA0761D6478BD642F) * (cols + np.uint64(1)))[None, :])
    return (z >> np.uint64(40)).astype(np.int64)


def threshold(keep):
    return int(float(keep) * 16777216.0)


def mask(seed, step, layer, N, k, keep):
    return mask_bits(seed, step, layer, N, k) < threshold(keep)


# ---- forward and backward -------------------------------------------------------------------------------------------------
def xavier(rs, layers, k):
    """[layers][2][k][k] in the order W_0_1, W_0_2, W_1_1, ...: U(-sqrt(6 / 2k), +sqrt(6 / 2k))."""
    lim = math.sqrt(6.0 / (2 * k))
    return rs.uniform(-lim, lim, size=(layers, 2, k, k)).astype(np.float32)


def propagate(g, U, V, W, training=False, keep=0.9, seed=0, step=0, dtype=np.float64):
    """dict of per-layer lists E (inputs, E[0] = [U; V]), S, Z, M (mask / keep factor), D, ss and F."""
    L, k = W.shape[0], U.shape[1]
    W = W.astype(dtype)
    E = [np.concatenate([U, V]).astype(dtype)]
    N = E[0].shape[0]
    out = {'E': E, 'S': [], 'Z': [], 'kept': [], 'D': [], 'ss': [], 'blocks': [E[0]]}
    for l in range(L):
        e = E[-1]
        s = spmm(g, e)
        z = np.matmul(s + e, W[l, 0]) + np.matmul(e * s, W[l, 1])
        h = np.where(z > 0, z, dtype(SLOPE) * z)
        if training:
            kept = mask(seed, step, l, N, k, keep)
            d = np.where(kept, h / dtype(keep), dtype(0))
        else:
            kept = np.ones((N, k), bool)
            d = h
        d = d.astype(dtype)
        ss = (d * d).sum(axis=1)
        out['S'].append(s); out['Z'].append(z); out['kept'].append(kept); out['D'].append(d); out['ss'].append(ss)
        out['blocks'].append(d * (dtype(1) / np.sqrt(np.maximum(ss, dtype(EPS))))[:, None])
        E.append(d)
    out['F'] = np.concatenate(out['blocks'], axis=1)
    return out


def backward(g, W, fw, G, training, keep, dtype):
    """(g[U;V], gW) from dLoss / dF = G and the forward pass's record."""
    L, k = W.shape[0], W.shape[2]
    W = W.astype(dtype)
    gW = np.zeros((L, 2, k, k), dtype)
    gD = np.zeros_like(fw['E'][0])
    for l in range(L - 1, -1, -1):
        e, s, z, d = fw['E'][l], fw['S'][l], fw['Z'][l], fw['D'][l]
        gD = gD + nl.normalize_backward(d, fw['ss'][l], G[:, (l + 1) * k:(l + 2) * k], dtype)
        slope = np.where(z > 0, dtype(1), dtype(SLOPE))
        gz = (np.where(fw['kept'][l], gD / dtype(keep), dtype(0)) if training else gD) * slope
        gx1, gx2 = np.matmul(gz, W[l, 0].T), np.matmul(gz, W[l, 1].T)
        gW[l, 0] = np.matmul((s + e).T, gz)
        gW[l, 1] = np.matmul((e * s).T, gz)
        gs = gx1 + e * gx2
        gD = (gx1 + s * gx2) + spmm(g['T'], gs)
    return gD + G[:, :k], gW


def loss_and_grad(g, U, V, W, u, i, j, reg, training=False, keep=0.9, seed=0, step=0, dtype=np.float64):
    """(loss, gU, gV, gW, forward record)."""
    m = g['m']
    fw = propagate(g, U, V, W, training, keep, seed, step, dtype)
    loss, G = nl.batch_loss_and_G(fw['F'], m, u, i, j, reg, dtype)
    g0, gW = backward(g, W, fw, G, training, keep, dtype)
    return loss, g0[:m], g0[m:], gW, fw


def new_state(U, V, W):
    return {key: np.zeros_like(x) for key, x in (('mU', U), ('vU', U), ('mV', V), ('vV', V), ('mW', W), ('vW', W))}


def step(g, U, V, W, state, u, i, j, lr, reg, t, training=True, keep=0.9, seed=0, dtype=np.float64):
    """One sess.run([train, loss]) of :139, in place on U, V, W and state; the mask is that of step t.  Returns the loss."""
    loss, gU, gV, gW, _ = loss_and_grad(g, U, V, W, u, i, j, reg, training, keep, seed, t, dtype)
    adam(U, gU, state['mU'], state['vU'], lr, t, dtype)
    adam(V, gV, state['mV'], state['vV'], lr, t, dtype)
    adam(W, gW, state['mW'], state['vW'], lr, t, dtype)
    return loss


# ---- sampler -------------------------------------------------------------------------------------------------------------
def next_batch(ev_u, ev_t, track_key_ids, batch_size, rng=_random):
    """:16-41 on ids: events in order in slices of batch_size (the last one short); one negative per event by rng.choice over
    the tracks in trackRecord's key order, never rejected."""
    train_size = len(ev_u)
    item_list = list(track_key_ids)
    batch_id = 0
    while batch_id < train_size:
        end = min(batch_id + batch_size, train_size)
        u_idx, i_idx, j_idx = [], [], []
        for t in range(batch_id, end):
            u_idx.append(int(ev_u[t]))
            i_idx.append(int(ev_t[t]))
            j_idx.append(int(rng.choice(item_list)))
        batch_id = end
        yield u_idx, i_idx, j_idx
