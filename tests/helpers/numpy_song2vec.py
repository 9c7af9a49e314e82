"""NumPy contract of Song2vec (reference recommender/advanced/Song2vec.py; device side: include/yue_hip.h yue_s2v_*,
yue_cnet_set_sentences, yue_amd/csrc/s2v_kernels.hpp), written the slow obvious way.

iteration  rating_pass and pair_pass restate :165-189 one NumPy call for one NumPy call, on the types the reference has
           (X, Y float32; Bu, Bi float64; count a Python int; sim and globalMean Python numbers), so NumPy 2 rounds as it
           does there: the rating pass forms its row steps in float64 and rounds to float32 once in the ``+=``, the pair
           pass is float32 throughout (a Python float meeting a float32 scalar is rounded to float32 first).
dot        ``dot=np.dot`` makes the reference's call; ``dot=butterfly`` is the device's order: lane l holds elements l and
           l + 64, the 64 lanes are summed as a butterfly (partner lane ^ 1, 2, 4, 8, 16, then lanes 0 + 32), all float32.
square     the reference squares an error with ``error ** 2``: NumPy's scalar power calls libm's pow, which is not correctly
           rounded (on 300,000 normal doubles 271 results differ from the product in the last bit, 215 in float32).  A
           device cannot be held to libm's rounding errors, so the squared errors it returns are the products, and
           ``square=product`` is that form; ``square=power`` (the default) makes the reference's call.  The two differ
           by one unit in the last place of single terms of the loss, nothing else: no squared error feeds back.
levels     level(step) = 1 + max(level of the previous step with the same a, ... the same b) (returned from 0); for pairs
           a and b are rows of one matrix (``shared``).  The level-driven passes run the steps level by level, in any order
           inside a level, and give the sequential passes' result bit for bit.
sentences  the users with MORE than 10 training events, their events' tracks in record order, repeats included.
embed      section 18's embedding contract (numpy_cune_net.embed) for sentences of unequal length: every sentence is cut
           into consecutive segments of at most S words (segment_words), a segment is trained as a walk of its own length,
           alpha runs over the words passed, counts and tables over the real words.
"""
import numpy as np

from .numpy_cune_net import FIX, TAG_INIT, TAG_NEG, TAG_SUB, TAG_WIN, _sum32, cnet_hash

MIN_EVENTS = 10
_LANE = np.arange(64)


def init_from_seed(seed, m, n, k):
    """(X, Y, Bu, Bi) of initModel (:19-26) after np.random.seed(seed): P, Q, then Bu, Bi."""
    rs = np.random.RandomState(seed)
    P = rs.rand(m, k).astype(np.float32) / 10
    Q = rs.rand(n, k).astype(np.float32) / 10
    return P * 10, Q * 10, rs.rand(m) / 10, rs.rand(n) / 10


def power(e):
    return e ** 2


def product(e):
    return e * e


def butterfly(a, b):
    """float32 dot of two float32 rows (k <= 128) in the device's order."""
    k = len(a)
    v = np.zeros(128, np.float32)
    v[:k] = a * b
    acc = (np.zeros(64, np.float32) + v[:64]) + v[64:]
    for s in (1, 2, 4, 8, 16):
        acc = acc + acc[_LANE ^ s]
    return acc[0] + acc[32]


def sentences(ev_ptr, ev_track):
    """(users, list of int32 arrays): the users with more than 10 events (:41) and their play lists in record order."""
    users = [u for u in range(len(ev_ptr) - 1) if ev_ptr[u + 1] - ev_ptr[u] > MIN_EVENTS]
    return users, [np.asarray(ev_track[ev_ptr[u]:ev_ptr[u + 1]], np.int32) for u in users]


def user_listen(ev_ptr, ev_i):
    """(u, i, count) int32: for the users of `sentences` in id order, their items in first-listen order with the number of
    events (:70-75, :165-169)."""
    su, si, sc = [], [], []
    for u in range(len(ev_ptr) - 1):
        if ev_ptr[u + 1] - ev_ptr[u] > MIN_EVENTS:
            row = {}
            for i in ev_i[ev_ptr[u]:ev_ptr[u + 1]]:
                row[int(i)] = row.get(int(i), 0) + 1
            for i, cnt in row.items():
                su.append(u); si.append(i); sc.append(cnt)
    return np.array(su, np.int32), np.array(si, np.int32), np.array(sc, np.int32)


def _rate_step(X, Y, Bu, Bi, u, i, count, bu, lRate, regU, regI, regB, globalMean, dot, square=power):
    bi = Bi[i]                                                                      # :171
    rating = dot(Y[i], X[u]) + globalMean + Bu[u] + Bi[i]                            # :172
    error = count - rating
    X[u] += lRate * (error * Y[i] - regU * X[u])                                     # :175
    Y[i] += lRate * (error * X[u] - regI * Y[i])
    Bu[u] += lRate * (error - regB * bu)                                             # :178
    Bi[i] += lRate * (error - regB * bi)
    return square(error)                                                            # :174


def rating_pass(X, Y, Bu, Bi, su, si, sc, lRate, regU, regI, regB, globalMean=0, dot=np.dot, stale=True, square=power):
    """:165-179 in place; returns the squared errors per step.  stale=False uses the current Bu[u] in :178 (what the
    reference does not do; the edge tests show that the difference is visible)."""
    out = []
    bu = None
    for t in range(len(su)):
        u, i = int(su[t]), int(si[t])
        if t == 0 or su[t - 1] != su[t]:
            bu = Bu[u]                                                              # :167, once per user
        out.append(_rate_step(X, Y, Bu, Bi, u, i, int(sc[t]), bu if stale else Bu[u], lRate, regU, regI, regB, globalMean, dot, square))
    return out


def _pair_step(Y, t1, t2, sim, alpha, lRate, dot, square=power):
    error2 = sim - dot(Y[t1], Y[t2])                                                # :186
    Y[t1] += 0.5 * alpha * lRate * (error2) * Y[t2]
    Y[t2] += 0.5 * alpha * lRate * (error2) * Y[t1]
    return square(error2)                                                           # :187


def pair_pass(Y, t1, t2, sim, alpha, lRate, dot=np.dot, square=power):
    """:181-189 in place; returns the squared errors per pair."""
    return [_pair_step(Y, int(t1[p]), int(t2[p]), float(sim[p]), alpha, lRate, dot, square) for p in range(len(t1))]


def levels(a, b, shared=False):
    """int32 level (from 0) of every step."""
    last_a = {}
    last_b = last_a if shared else {}
    out = np.zeros(len(a), np.int32)
    for t in range(len(a)):
        l = 1 + max(last_a.get(int(a[t]), 0), last_b.get(int(b[t]), 0))
        last_a[int(a[t])] = l
        last_b[int(b[t])] = l
        out[t] = l - 1
    return out


def _level_order(level, rng):
    order = []
    for l in range(int(level.max()) + 1 if len(level) else 0):
        idx = np.flatnonzero(level == l)
        if rng is not None:
            idx = rng.permutation(idx)
        order += [int(t) for t in idx]
    return order


def rating_pass_levels(X, Y, Bu, Bi, su, si, sc, lRate, regU, regI, regB, globalMean=0, dot=np.dot, rng=None, square=power):
    """rating_pass level by level (rng: the steps of a level in a random order).  bu is Bu[u] as the pass began: only a
    user's own steps change it."""
    bu0 = Bu.copy()
    out = [None] * len(su)
    for t in _level_order(levels(su, si), rng):
        u, i = int(su[t]), int(si[t])
        out[t] = _rate_step(X, Y, Bu, Bi, u, i, int(sc[t]), bu0[u], lRate, regU, regI, regB, globalMean, dot, square)
    return out


def pair_pass_levels(Y, t1, t2, sim, alpha, lRate, dot=np.dot, rng=None, square=power):
    out = [None] * len(t1)
    for p in _level_order(levels(t1, t2, shared=True), rng):
        out[p] = _pair_step(Y, int(t1[p]), int(t2[p]), float(sim[p]), alpha, lRate, dot, square)
    return out


def compose_loss(err_steps, err_pairs, X, Y, Bu, Bi, regB):
    """self.loss as :164-190 adds it up."""
    loss = 0
    for e in err_steps:
        loss += e
    for e in err_pairs:
        loss += e
    loss += regB * (Bu * Bu).sum() + regB * (Bi * Bi).sum() + (X * X).sum() + (Y * Y).sum()
    return loss


def iteration(X, Y, Bu, Bi, steps, pairs, lRate, regU, regI, regB, alpha, globalMean=0, dot=np.dot, by_levels=False, rng=None, square=power):
    """One iteration in place; steps = (u, i, count), pairs = (t1, t2, sim).  Returns (loss, err_steps, err_pairs)."""
    if by_levels:
        e1 = rating_pass_levels(X, Y, Bu, Bi, steps[0], steps[1], steps[2], lRate, regU, regI, regB, globalMean, dot, rng, square)
        e2 = pair_pass_levels(Y, pairs[0], pairs[1], pairs[2], alpha, lRate, dot, rng, square)
    else:
        e1 = rating_pass(X, Y, Bu, Bi, steps[0], steps[1], steps[2], lRate, regU, regI, regB, globalMean, dot, True, square)
        e2 = pair_pass(Y, pairs[0], pairs[1], pairs[2], alpha, lRate, dot, square)
    return compose_loss(e1, e2, X, Y, Bu, Bi, regB), e1, e2


def rel(a, b):
    """Largest absolute difference relative to the largest entry of b."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max()) if a.size else 0.0


# ---- the embedding of sentences ----
def segment_words(dim, negative=5):
    """S: the largest value <= 64 for which S (negative + 2) rows of dim floats fit 60 KiB (and, with the ids of the targets
    behind them, 63 KiB)."""
    S = 64
    while S > 0 and (S * (negative + 2) * dim * 4 > 60 * 1024 or S * (negative + 2) * dim * 4 + S * (negative + 1) * 4 > 63 * 1024):
        S -= 1
    return S


def segments(sents, S):
    """The sentences cut into consecutive segments of at most S words, the last one of a sentence shorter."""
    return [np.asarray(s[b:b + S], np.int32) for s in sents for b in range(0, len(s), S)]


def tables(segs, m):
    """numpy_cune_net.tables over the real words."""
    words = np.concatenate(segs)
    cnt = np.bincount(words, minlength=m).astype(np.int64)
    thr = 1e-3 * float(len(words))
    keep = np.zeros(m, np.uint64)
    cum = np.zeros(m, np.uint64)
    z = 0.0
    for u in range(m):
        if cnt[u] > 0:
            x = float(cnt[u])
            z = z + np.sqrt(x) * np.sqrt(np.sqrt(x))
    run = 0.0
    for u in range(m):
        if cnt[u] > 0:
            x = float(cnt[u])
            p = (np.sqrt(x / thr) + 1.0) * (thr / x)
            keep[u] = 1 << 32 if p >= 1.0 else int(p * 4294967296.0)
            run = run + np.sqrt(x) * np.sqrt(np.sqrt(x))
        cum[u] = min(int(run / z * 4294967296.0), 1 << 32)
    for u in range(m - 1, -1, -1):
        cum[u] = 1 << 32
        if cnt[u] > 0:
            break
    return cnt, keep, cum


def embed_sentences(sents, m, dim, window, epochs, seed, negative=5, round_walks=1, dtype=np.float32, stats=None):
    """syn0 [m, dim]: numpy_cune_net.embed with the segments of `sents` as walks of their own length.  stats (a dict,
    filled): 'S', 'segments' (their lengths), 'trained' positions that had a context per (epoch, segment) visit."""
    ft = dtype
    S = segment_words(dim, negative)
    assert S >= 2 * window + 1, 'a segment holds fewer than 2 window + 1 words'
    segs = segments(sents, S)
    nw = len(segs)
    pre = np.concatenate([[0], np.cumsum([len(s) for s in segs])])
    words = int(pre[-1])
    if stats is not None:
        stats.update({'S': S, 'segments': [len(s) for s in segs], 'trained': []})
    cnt, keep, cum = tables(segs, m)
    keep = [int(x) for x in keep]
    syn0 = np.zeros((m, dim), ft)
    for u in np.flatnonzero(cnt > 0):
        U = np.array([cnet_hash(seed ^ TAG_INIT, int(u), 0, d, 0) >> 40 for d in range(dim)], np.float32) * np.float32(1.0 / 16777216.0)
        syn0[u] = ((U - np.float32(0.5)) / np.float32(dim)).astype(ft)
    syn1 = np.zeros((m, dim), ft)
    one = ft(1.0)
    for ep in range(epochs):
        for w0 in range(0, nw, round_walks):
            acc0, acc1 = {}, {}
            for w in range(w0, min(w0 + round_walks, nw)):
                cur0, cur1 = {}, {}
                ids = [int(x) for x in segs[w]]
                kept = [p for p in range(len(ids)) if (cnet_hash(seed ^ TAG_SUB, w, ep, p, 0) >> 32) < keep[ids[p]]]
                done = float(ep * words + int(pre[w])) / float(epochs * words)
                alpha = ft(np.float32(0.025 - (0.025 - 1e-4) * done))
                trained = 0
                for kp, p in enumerate(kept):
                    word = ids[p]
                    b = ((cnet_hash(seed ^ TAG_WIN, w, ep, p, 0) >> 32) * window) >> 32
                    lo, hi = max(0, kp - window + b), min(len(kept), kp + window + 1 - b)
                    ctx = [ids[kept[c]] for c in range(lo, hi) if c != kp]
                    if not ctx:
                        continue
                    trained += 1
                    neu1 = np.zeros(dim, ft)
                    for x in ctx:
                        neu1 = neu1 + cur0.get(x, syn0[x])
                    inv = ft(np.float32(1.0) / np.float32(len(ctx)))
                    neu1 = neu1 * inv
                    work = np.zeros(dim, ft)
                    for d in range(negative + 1):
                        tgt = word
                        if d > 0:
                            tgt = int(np.searchsorted(cum, cnet_hash(seed ^ TAG_NEG, w, ep, p, d) >> 32, side='right'))
                            if tgt == word:
                                continue
                        row = cur1.get(tgt, syn1[tgt])
                        f = ft(np.dot(neu1, row)) if ft is np.float64 else _sum32(neu1 * row)
                        if f >= 6.0 or f <= -6.0:
                            continue
                        g = (ft(1.0 if d == 0 else 0.0) - one / (one + np.exp(-f))) * alpha
                        work = work + g * row
                        cur1[tgt] = row + g * neu1
                    work = work * inv
                    for x in ctx:
                        cur0[x] = cur0.get(x, syn0[x]) + work
                if stats is not None:
                    stats['trained'].append(trained)
                for tab, acc, M in ((cur0, acc0, syn0), (cur1, acc1, syn1)):
                    for x, row in tab.items():
                        q = np.rint((row - M[x]).astype(np.float64) * FIX).astype(np.int64)
                        acc[x] = acc[x] + q if x in acc else q
            for acc, M in ((acc0, syn0), (acc1, syn1)):
                for x, q in acc.items():
                    M[x] = (M[x].astype(np.float64) + q.astype(np.float64) * (1.0 / FIX)).astype(ft)
    return syn0
