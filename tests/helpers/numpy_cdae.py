"""NumPy restatement of the reference's CDAE (recommender/advanced/CDAE.py) -- TEST INFRASTRUCTURE.

PARITY UNPINNED: TensorFlow is not installable here, so nothing in this file has been checked against the reference's own
execution; the goldens tests/golden/g20_cdae_*.json pin this contract, not TensorFlow.  What it restates:
  parameters  U [m,h] Xavier uniform with limit sqrt(6 / (m + h)); encoder W [n,h], decoder W' [h,n], biases b [h], b' [n] normal
              with `stddev` (1 as written); drawn with NumPy in the order U, W, W', b, b'                                (:31-48)
  counts      userListen[u][t] = the pair's event count c (starts at 1, later events increment it)                      (:50-57)
  batch       B users by random.choice over the user names, with replacement; per slot `sample` holds the user's distinct
              items and neg * len(items) draws of random.choice over the track names, never rejected; a set             (:76-98)
  mask        TensorFlow's / NumPy's streams cannot be reproduced: input entry (slot, item) of `step` is KEPT when the top 24
              bits of cnet_hash(seed ^ TAG, step, slot, item, 0) lie below floor(co * 2^24)                             (:124)
  forward     hid = sigmoid((X o mask) W + b + U[u]); dec = sigmoid(hid W' + b'); y_pred = max(1e-6, sample o dec);
              y_true = sample o X o mask (counts: may exceed 1)                                                  (:59-65, :101-107)
  loss        mean over [B, n] of (-y_true log y_pred - (1 - y_true) log(1 - y_pred)) + regU (l2_loss(W) + l2_loss(W') + l2_loss(b)
              + l2_loss(b') + l2_loss(U[u_batch])); an unsampled element is the constant -log(1 - 1e-6) of float32      (:109-115)
  gradient    TensorFlow's decomposition: through the mean 1 / (B n); -y_true / p + (1 - y_true) / (1 - p); tf.maximum passes it
              where dec > 1e-6 only; the sigmoid's (dy * y) * (1 - y); the reg term does not carry 1 / (B n)
  update      dense Adam on all five variables, every row of U included (numpy_lightgcn.adam)                           (:117)
Every function takes dtype = np.float64 (the yardstick) or np.float32 (statement by statement).  The backward pass is written out by
hand and checked against central differences (tests/test_cdae_golden.py).
"""
import math
import random as _random

import numpy as np

from . import numpy_lightgcn as nl

TAG = 0x43444145
M64 = (1 << 64) - 1
CLAMP = float(np.float32(1e-6))                                                   # tf.maximum(1e-6, .) on float32 tensors
UNSAMPLED = float(np.float32(-np.log(np.float64(np.float32(1) - np.float32(1e-6)))))   # the loss of an element outside `sample`: float32's 1 - 1e-6, its log rounded once
NAMES = ('U', 'W', 'Wd', 'b', 'bd')

rel = nl.rel
adam = nl.adam


# ---- parameters and data -------------------------------------------------------------------------------------------------
def init_params(rs, m, n, h, stddev=1.0):
    """U, W, W' (here Wd [h, n]), b, b' (bd) in creation order, float32."""
    lim = math.sqrt(6.0 / (m + h))
    U = rs.uniform(-lim, lim, size=(m, h)).astype(np.float32)
    W = rs.normal(0.0, stddev, size=(n, h)).astype(np.float32)
    Wd = rs.normal(0.0, stddev, size=(h, n)).astype(np.float32)
    b = rs.normal(0.0, stddev, size=h).astype(np.float32)
    bd = rs.normal(0.0, stddev, size=n).astype(np.float32)
    return {'U': U, 'W': W, 'Wd': Wd, 'b': b, 'bd': bd}


def user_csr(ev_u, ev_t, m):
    """(ptr [m + 1], items ascending, counts): userListen as a CSR."""
    count = {}
    for u, t in zip(ev_u, ev_t):
        count[(int(u), int(t))] = count.get((int(u), int(t)), 0) + 1
    pairs = sorted(count)
    ptr = np.zeros(m + 1, np.int64)
    for u, _ in pairs:
        ptr[u + 1] += 1
    return np.cumsum(ptr), np.array([p[1] for p in pairs], np.int32).reshape(-1), np.array([count[p] for p in pairs], np.int32).reshape(-1)


def sample_csr(sets):
    """(ptr [B + 1], items) of the batch's sample sets, items ascending within a slot."""
    ptr = np.zeros(len(sets) + 1, np.int64)
    ptr[1:] = np.cumsum([len(s) for s in sets])
    items = np.array([i for s in sets for i in sorted(s)], np.int32).reshape(-1)
    return ptr, items


# ---- mask ----------------------------------------------------------------------------------------------------------------
def _mix(z):
    z = z ^ (z >> np.uint64(30)); z = z * np.uint64(0xBF58476D1CE4E5B9)
    z = z ^ (z >> np.uint64(27)); z = z * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


def mask_bits(seed, step, slot, items):
    """The top 24 bits of cnet_hash(seed ^ TAG, step, slot, item, 0) for every item of `items`."""
    items = np.asarray(items, np.uint64).reshape(-1)
    with np.errstate(over='ignore'):
        head = ((int(seed) ^ TAG) + 0x9E3779B97F4A7C15 * (int(step) + 1)) & M64
        z = _mix(np.array([head], np.uint64))
        z = _mix(z ^ (np.uint64((0xD1B54A32D192ED03 * (int(slot) + 1)) & M64) + np.uint64(0x8CB92BA72F3D8DD7) * items))
        z = _mix(z ^ np.uint64(0xA0761D6478BD642F))
    return (z >> np.uint64(40)).astype(np.int64)


def threshold(co):
    return int(float(co) * 16777216.0)


def kept(seed, step, slot, items, co):
    return mask_bits(seed, step, slot, items) < threshold(co)


# ---- forward and backward -------------------------------------------------------------------------------------------------
def _sigmoid(x):
    one = x.dtype.type(1)
    return (one / (one + np.exp(-x))).astype(x.dtype)


def encode(p, data, users, flags, dtype=np.float64):
    """hid [B, h]: flags[s] is the kept flag of every item of users[s] (all ones: the uncorrupted row)."""
    ptr, items, cnt = data
    W, b, U = p['W'].astype(dtype), p['b'].astype(dtype), p['U'].astype(dtype)
    hid = np.zeros((len(users), W.shape[1]), dtype)
    for s, u in enumerate(users):
        it, c = items[ptr[u]:ptr[u + 1]], cnt[ptr[u]:ptr[u + 1]]
        x = (np.where(flags[s], c, 0).astype(dtype)[:, None] * W[it]).sum(axis=0, dtype=dtype)
        hid[s] = _sigmoid((x + b) + U[u])
    return hid


def forward(p, data, users, sptr, sitems, co, seed, step, dtype=np.float64):
    """dict: flags (list per slot), hid, logit / dec / y_pred / y_true per sampled entry, slot per entry, saturated, loss."""
    ptr, items, cnt = data
    B, n = len(users), p['W'].shape[0]
    flags = [kept(seed, step, s, items[ptr[u]:ptr[u + 1]], co) for s, u in enumerate(users)]
    hid = encode(p, data, users, flags, dtype)
    Wd, bd = p['Wd'].astype(dtype), p['bd'].astype(dtype)
    S = int(sptr[-1])
    slot = np.repeat(np.arange(B), np.diff(sptr)).astype(np.int64)
    col = np.asarray(sitems[:S], np.int64)
    logit = ((hid[slot] * Wd[:, col].T).sum(axis=1, dtype=dtype) + bd[col]).astype(dtype) if S else np.zeros(0, dtype)
    dec = _sigmoid(logit)
    y_pred = np.maximum(dtype(CLAMP), dec)
    y_true = np.zeros(S, dtype)
    for s, u in enumerate(users):
        it, c = items[ptr[u]:ptr[u + 1]], cnt[ptr[u]:ptr[u + 1]]
        mine = col[sptr[s]:sptr[s + 1]]
        pos = np.searchsorted(it, mine)
        hit = (pos < len(it)) & (it[np.minimum(pos, max(len(it) - 1, 0))] == mine) if len(it) else np.zeros(len(mine), bool)
        y_true[sptr[s]:sptr[s + 1]][hit] = np.where(flags[s], c, 0)[pos[hit]]
    saturated = int((y_pred.astype(np.float32) == np.float32(1)).sum())
    one = dtype(1)
    with np.errstate(divide='ignore', invalid='ignore'):
        terms = -y_true * np.log(y_pred) - (one - y_true) * np.log(one - y_pred)
    count = B * n
    data_sum = terms.sum(dtype=dtype) + dtype(count - S) * dtype(UNSAMPLED)
    half = dtype(2)
    Ub = p['U'].astype(dtype)[np.asarray(users, np.int64)]
    l2 = sum((p[k].astype(dtype) ** 2).sum(dtype=dtype) / half for k in ('W', 'Wd', 'b', 'bd')) + (Ub * Ub).sum(dtype=dtype) / half
    return {'flags': flags, 'hid': hid, 'slot': slot, 'col': col, 'logit': logit, 'dec': dec, 'y_pred': y_pred, 'y_true': y_true,
            'saturated': saturated, 'data': data_sum / dtype(count), 'l2': l2}


def loss_and_grad(p, data, users, sptr, sitems, co, seed, step, reg, dtype=np.float64):
    """(loss, dict of the five gradients, forward record).  With a saturated output the float32 loss is inf, as TensorFlow's."""
    ptr, items, cnt = data
    fw = forward(p, data, users, sptr, sitems, co, seed, step, dtype)
    B, (n, h) = len(users), p['W'].shape
    reg = dtype(reg)
    loss = fw['data'] + reg * fw['l2']
    if fw['saturated']:
        loss = dtype(np.inf)
    one = dtype(1)
    g0 = one / dtype(B * n)
    pr, t, dec = fw['y_pred'], fw['y_true'], fw['dec']
    with np.errstate(divide='ignore', invalid='ignore'):
        gp = ((-g0) * t) * (one / pr) + (g0 * (one - t)) * (one / (one - pr))
        gp = np.where(dec > dtype(CLAMP), gp, dtype(0))
        e = ((gp * dec) * (one - dec)).astype(dtype)
    hid, slot, col = fw['hid'], fw['slot'], fw['col']
    Wd = p['Wd'].astype(dtype)
    g_hid = np.zeros_like(hid)
    np.add.at(g_hid, slot, e[:, None] * Wd[:, col].T)
    dz = ((g_hid * hid) * (one - hid)).astype(dtype)
    gWdT = np.zeros((n, h), dtype)
    np.add.at(gWdT, col, e[:, None] * hid[slot])
    gbd = np.zeros(n, dtype)
    np.add.at(gbd, col, e)
    gW = np.zeros((n, h), dtype)
    gU = np.zeros(p['U'].shape, dtype)
    U = p['U'].astype(dtype)
    for s, u in enumerate(users):
        it, c = items[ptr[u]:ptr[u + 1]], cnt[ptr[u]:ptr[u + 1]]
        live = fw['flags'][s]
        np.add.at(gW, it[live], c[live].astype(dtype)[:, None] * dz[s][None, :])
        gU[u] = gU[u] + (dz[s] + reg * U[u])
    g = {'U': gU, 'W': gW + reg * p['W'].astype(dtype), 'Wd': (gWdT + reg * Wd.T).T.copy(), 'b': dz.sum(axis=0, dtype=dtype) + reg * p['b'].astype(dtype),
         'bd': gbd + reg * p['bd'].astype(dtype)}
    fw['e'], fw['dz'] = e, dz
    return dtype(loss), g, fw


def new_state(p):
    st = {}
    for k in NAMES:
        st['m' + k], st['v' + k] = np.zeros_like(p[k]), np.zeros_like(p[k])
    return st


def step(p, state, data, users, sptr, sitems, co, seed, t, lr, reg, dtype=np.float64):
    """One sess.run of :127 in place on p and state; the mask is that of step t.  Returns (loss, saturated); a saturated step
    moves nothing (the device's rule; TensorFlow's own step would write NaN)."""
    loss, g, fw = loss_and_grad(p, data, users, sptr, sitems, co, seed, t, reg, dtype)
    if fw['saturated']:
        return loss, fw['saturated']
    for k in NAMES:
        adam(p[k], g[k], state['m' + k], state['v' + k], lr, t, dtype)
    return loss, 0


def factors(p, data, dtype=np.float64):
    """(P [m, h + 1] = [hid of the uncorrupted row | 1], Q [n, h + 1] = [W'^T | b']): P[u] . Q[i] is the decoder's logit."""
    ptr = data[0]
    m = len(ptr) - 1
    hid = encode(p, data, list(range(m)), [np.ones(int(ptr[u + 1] - ptr[u]), bool) for u in range(m)], dtype)
    P = np.concatenate([hid, np.ones((m, 1), dtype)], axis=1)
    Q = np.concatenate([p['Wd'].astype(dtype).T, p['bd'].astype(dtype)[:, None]], axis=1)
    return P, Q


# ---- sampler -------------------------------------------------------------------------------------------------------------
def next_batch(user_key_ids, track_key_ids, data, batch_size, neg=5, rng=_random):
    """:76-98 on ids: per slot one rng.choice over the users in name2id's key order, then neg * len(items) rng.choice draws over
    the tracks in name2id's key order, never rejected.  Returns (users, sample sets)."""
    ptr, items, _ = data
    users, sets = [], []
    for _ in range(batch_size):
        u = int(rng.choice(user_key_ids))
        mine = [int(i) for i in items[ptr[u]:ptr[u + 1]]]
        sample = set(mine)
        for _ in range(neg * len(mine)):
            sample.add(int(rng.choice(track_key_ids)))
        users.append(u)
        sets.append(sample)
    return users, sets


def hub_counts(data, users, sptr, sitems, hub):
    """(hubs, parts) as the device counts them at option cdae_hub: encoder rows, then the segments of the four regroupings
    (sampled entries by item, input entries by item, slots by user, all slots for b) longer than `hub`."""
    ptr = data[0]
    B = len(users)
    lens = [int(ptr[u + 1] - ptr[u]) for u in users]
    lens += np.bincount(np.asarray(sitems[:int(sptr[-1])], np.int64)).tolist() if sptr[-1] else []
    ins = np.concatenate([data[1][ptr[u]:ptr[u + 1]] for u in users]) if B else np.zeros(0, np.int64)
    lens += np.bincount(ins.astype(np.int64)).tolist() if len(ins) else []
    lens += np.bincount(np.asarray(users, np.int64)).tolist() + [B]
    big = [x for x in lens if x > hub]
    return len(big), sum((x + hub - 1) // hub for x in big)
