"""NumPy contract of CUNE's user-network stage (reference recommender/advanced/CUNE.py:34-118; device side:
include/yue_hip.h yue_cnet_*, yue_amd/csrc/cnet_kernels.hpp), written the slow obvious way.

stream     every random number is cnet_hash(seed ^ tag, a, b, c, d): the mix64 chain of the BPR sampler.
network    cunet(a) is the explicit list of the reference (:39-52): every other user b repeated |items(a) & items(b)|
           times, here in the order (item of a ascending, listener ascending) -- the order entry(a, r) indexes without the
           list: prefix sums of deg(item) - 1 over a's items, the listener by index with a skipped.
walks      T walks of length L per network user (ids ascending); step draws entry mulhi(hash(start, t, step, attempt),
           total(last)) of cunet(last); up to 10 re-draws while the candidate is in visited[start], consulted only where
           last == start (DEVIATION: the reference reads visited[last], whose content for last != start depends on dict
           order).  shuffle(): the walks ordered by (hash(seed ^ shuffle, walk), walk).
embed      gensim's CBOW / negative sampling as documented (see yue_cnet_embed in the header), float32 or float64, in
           rounds of round_walks walks: a walk works on copies of the round-start rows; its row differences are rounded
           to multiples of 2^-36, summed as integers, and row = dtype(fp64(row) + sum 2^-36).  round_walks = 1 is the
           sequential algorithm.
friends    cosine = float(dot) / sqrt(n_a n_b) in fp64 over the float32 values, as tool/qmath.py:36-45 computes it: its
           ``sqrt`` is math.sqrt, both operands are Python floats, so a zero norm raises ZeroDivisionError and the
           reference returns 0 (NumPy's nan-with-a-warning would need a NumPy denominator).  A zero row therefore has
           cosine 0 with everyone; among rows of positive cosines it ranks last.  Order (cosine descending, id ascending).
"""
import numpy as np

M64 = (1 << 64) - 1
TAG_WALK, TAG_SHUFFLE, TAG_INIT, TAG_SUB, TAG_WIN, TAG_NEG = 0, 0x5348554646, 0x494E4954, 0x535542, 0x57494E, 0x4E4547
REDRAWS = 10
FIX = 2.0 ** 36


def mix64(z):
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def cnet_hash(seed, a, b=0, c=0, d=0):
    z = mix64((seed + 0x9E3779B97F4A7C15 * (a + 1)) & M64)
    z = mix64(z ^ ((0xD1B54A32D192ED03 * (b + 1) + 0x8CB92BA72F3D8DD7 * c) & M64))
    return mix64(z ^ ((0xA0761D6478BD642F * (d + 1)) & M64))


def pairs_from_events(ev_u, ev_i, m, n):
    """Distinct (user, item) pairs: user-major (u_ptr, items ascending), item-major (i_ptr, users ascending)."""
    keys = np.unique(np.asarray(ev_u, np.int64) * n + np.asarray(ev_i, np.int64))
    users, items = (keys // n).astype(np.int32), (keys % n).astype(np.int32)
    u_ptr = np.zeros(m + 1, np.int64)
    np.add.at(u_ptr, users.astype(np.int64) + 1, 1)
    i_ptr = np.zeros(n + 1, np.int64)
    np.add.at(i_ptr, items.astype(np.int64) + 1, 1)
    order = np.argsort(items, kind='stable')
    return (np.cumsum(u_ptr), items), (np.cumsum(i_ptr), users[order])


class Net(object):
    def __init__(self, u_ptr, u_items, i_ptr, i_users):
        self.u_ptr, self.u_items, self.i_ptr, self.i_users = u_ptr, u_items, i_ptr, i_users
        self.m = len(u_ptr) - 1
        deg = np.diff(i_ptr)
        self.pref = [np.cumsum(deg[u_items[u_ptr[u]:u_ptr[u + 1]]] - 1) for u in range(self.m)]
        self.total = np.array([int(p[-1]) if len(p) else 0 for p in self.pref], np.int64)
        self.users = np.flatnonzero(self.total > 0)
        self._lists = {}

    def cunet(self, a):
        """The explicit list of :39-52 (item ascending, listener ascending)."""
        if a not in self._lists:
            out = []
            for i in self.u_items[self.u_ptr[a]:self.u_ptr[a + 1]]:
                out += [int(b) for b in self.i_users[self.i_ptr[i]:self.i_ptr[i + 1]] if b != a]
            self._lists[a] = out
        return self._lists[a]

    def entry(self, a, r):
        """Entry r of cunet(a) by the (prefix, item, listener) rule, without the list."""
        pref = self.pref[a]
        e = int(np.searchsorted(pref, r, side='right'))
        off = r - (int(pref[e - 1]) if e else 0)
        i = self.u_items[self.u_ptr[a] + e]
        row = self.i_users[self.i_ptr[i]:self.i_ptr[i + 1]]
        pos = int(np.searchsorted(row, a))
        return int(row[off + (1 if off >= pos else 0)])


def walks_unshuffled(net, T, L, seed, stats=None):
    """int32 [nw, L] in generation order (start ascending, t ascending); explicit CUNet lists."""
    out = []
    for start in net.users:
        start = int(start)
        visited = set()
        for t in range(T):
            path, last = [start], start
            for step in range(1, L):
                lst = net.cunet(last)
                cand = lst[(cnet_hash(seed ^ TAG_WALK, start, t, step, 0) * len(lst)) >> 64]
                if last == start:
                    count = 0
                    while cand in visited:
                        count += 1
                        cand = lst[(cnet_hash(seed ^ TAG_WALK, start, t, step, count) * len(lst)) >> 64]
                        if count == REDRAWS:
                            if stats is not None:
                                stats['cutoffs'] = stats.get('cutoffs', 0) + 1
                            break
                path.append(cand)
                visited.add(cand)
                last = cand
            out.append(path)
    return np.array(out, np.int32).reshape(len(out), L)


def shuffle_order(nw, seed):
    keys = np.array([cnet_hash(seed ^ TAG_SHUFFLE, w) for w in range(nw)], np.uint64)
    return np.lexsort((np.arange(nw), keys))


def walks(net, T, L, seed, stats=None):
    """The walks in training order."""
    w = walks_unshuffled(net, T, L, seed, stats)
    return w[shuffle_order(len(w), seed)]


def tables(walk_arr, m):
    """(cnt, keep, cum): occurrences, the subsampling thresholds and the negative table, as 32-bit thresholds."""
    cnt = np.bincount(walk_arr.ravel(), minlength=m).astype(np.int64)
    thr = 1e-3 * float(walk_arr.size)
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


def embed(walk_arr, m, dim, window, epochs, seed, negative=5, round_walks=1, dtype=np.float32, snapshots=None, stats=None):
    """syn0 [m, dim] after `epochs` epochs over the walks in the given order; snapshots: {epoch count: copy of syn0}.
    stats (a dict, filled): 'evals' logits computed, 'max_abs_f' the largest |logit|, 'cutoffs' how many had |logit| >= 6,
    'cutoff_events' their (walk, epoch, position, d); per (epoch, walk) visit in order: 'kept' words left by subsampling,
    'trained' positions that had a context, 'targets' distinct syn1neg rows used; where stats comes in with a list under
    'f', every logit is appended to it in evaluation order (the order is the same for every dtype)."""
    if stats is not None:
        stats.update({'evals': 0, 'max_abs_f': 0.0, 'cutoffs': 0, 'cutoff_events': [], 'kept': [], 'trained': [], 'targets': []})
        all_f = stats.get('f')
    ft = dtype
    nw, L = walk_arr.shape
    cnt, keep, cum = tables(walk_arr, m)
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
                ids = [int(x) for x in walk_arr[w]]
                kept = [p for p in range(L) if (cnet_hash(seed ^ TAG_SUB, w, ep, p, 0) >> 32) < keep[ids[p]]]
                done = float((ep * nw + w) * L) / float(epochs * nw * L)
                alpha = ft(np.float32(0.025 - (0.025 - 1e-4) * done))
                trained, targets = 0, set()
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
                        if stats is not None:
                            targets.add(tgt)
                            stats['evals'] += 1
                            stats['max_abs_f'] = max(stats['max_abs_f'], abs(float(f)))
                            if all_f is not None:
                                all_f.append(float(f))
                            if f >= 6.0 or f <= -6.0:
                                stats['cutoffs'] += 1
                                stats['cutoff_events'].append((w, ep, p, d))
                        if f >= 6.0 or f <= -6.0:
                            continue
                        g = (ft(1.0 if d == 0 else 0.0) - one / (one + np.exp(-f))) * alpha
                        work = work + g * row
                        cur1[tgt] = row + g * neu1
                    work = work * inv
                    for x in ctx:
                        cur0[x] = cur0.get(x, syn0[x]) + work
                if stats is not None:
                    stats['kept'].append(len(kept)); stats['trained'].append(trained); stats['targets'].append(len(targets))
                for tab, acc, M in ((cur0, acc0, syn0), (cur1, acc1, syn1)):
                    for x, row in tab.items():
                        q = np.rint((row - M[x]).astype(np.float64) * FIX).astype(np.int64)
                        acc[x] = acc[x] + q if x in acc else q
            for acc, M in ((acc0, syn0), (acc1, syn1)):
                for x, q in acc.items():
                    M[x] = (M[x].astype(np.float64) + q.astype(np.float64) * (1.0 / FIX)).astype(ft)
        if snapshots is not None:
            snapshots[ep + 1] = syn0.copy()
    return syn0


def _sum32(v):
    """float32 sum, left to right (the device sums 64 lanes as a butterfly: covered by the tests' tolerance)."""
    s = np.float32(0.0)
    for x in v:
        s = np.float32(s + x)
    return s


def cosine(x1, x2):
    """tool/qmath.py:36-45 on float64 copies of the float32 rows."""
    from math import sqrt
    x1, x2 = x1.astype(np.float64), x2.astype(np.float64)
    total = x1.dot(x2)
    denom = sqrt(x1.dot(x1) * x2.dot(x2))
    try:
        return float(total) / denom
    except ZeroDivisionError:
        return 0


def friends(W, users, K):
    """(ids int32 [m, K] -1 padded, cosines float64 [m, K] 0 padded) for `users` (ascending ids with a row)."""
    W = np.asarray(W, np.float32)
    m = len(W)
    ids = np.full((m, K), -1, np.int32)
    sims = np.zeros((m, K), np.float64)
    users = [int(u) for u in users]
    for a in users:
        lst = [(b, cosine(W[a], W[b])) for b in users if b != a]
        lst = sorted(lst, key=lambda d: d[1], reverse=True)[:K]        # stable: ties stay in id order
        for r, (b, s) in enumerate(lst):
            ids[a, r], sims[a, r] = b, s
    return ids, sims


def friend_items(net_users, ids, u_ptr, u_items, ordered=False):
    """IPositiveSet (:112-114) as item-id lists per user: for every friend in rank order the items the friend listened to
    and the user did not.  Sorted (a multiset: the reference's order inside a friend is that of a Python set), or with
    ``ordered`` by (friend rank, item id ascending) as the plugin lists them."""
    out = {}
    for a in net_users:
        a = int(a)
        mine = set(int(x) for x in u_items[u_ptr[a]:u_ptr[a + 1]])
        row = []
        for b in ids[a]:
            if b >= 0:
                row += [int(x) for x in u_items[u_ptr[b]:u_ptr[b + 1]] if int(x) not in mine]
        out[a] = row if ordered else sorted(row)
    return out


# ---- the planted-groups log of the embedding quality test (tests/test_gpu_cnet.py, tools/make_cune_net_goldens.py) ----
PLANTED = {'groups': 8, 'group_users': 16, 'pool': 30, 'events': 20, 'global_share': 0.1, 'T': 20, 'L': 10, 'dim': 20, 'window': 5,
           'epochs': 10, 'K': 10, 'seeds': [1, 2, 3, 4, 5]}


def planted_log():
    """(ev_u, ev_i, m, n, group of every user): 8 groups of 16 users, 20 events each from the group's pool of 30 items,
    one event in ten from the global pool (all items) instead."""
    p = PLANTED
    rng = np.random.RandomState(20260015)
    m, n = p['groups'] * p['group_users'], p['groups'] * p['pool']
    group = np.arange(m) // p['group_users']
    ev_u = np.repeat(np.arange(m), p['events'])
    own = group[ev_u] * p['pool'] + rng.randint(0, p['pool'], len(ev_u))
    anywhere = rng.randint(0, n, len(ev_u))
    ev_i = np.where(rng.rand(len(ev_u)) < p['global_share'], anywhere, own)
    return ev_u.astype(np.int32), ev_i.astype(np.int32), m, n, group


def planted_score(ids, group):
    """Share of each user's listed friends that are in its own group, averaged over the users."""
    same = [(group[row[row >= 0]] == group[a]).mean() for a, row in enumerate(ids) if (row >= 0).any()]
    return float(np.mean(same))


# ---- the singleton-items log of the walk edge tests (tests/test_gpu_cnet_edges.py, tests/test_cune_net_golden.py) ----
def singleton_log():
    """(ev_u, ev_i, m, n, marked users): item 10 has 300 listeners (users 0..299); items nobody else listens to (zero-width
    entries of the prefix) sit at the start, at the end and as a run in the middle of network users' rows; users 300..304
    have only such items and are outside the network."""
    rows = {0: [0, 10, 20, 21, 22, 30, 40],       # first, a run of three in the middle, last
            1: [1, 10, 30, 41],                   # first and last
            2: [10, 30],
            5: [2, 10],                           # first only
            6: [10, 43],                          # last only
            298: [10, 31],
            299: [10, 23, 24, 31, 42]}            # a run of two in the middle, last
    for u in range(300):
        rows.setdefault(u, [10])
    for u in range(300, 305):
        rows[u] = [50 + u - 300]
    ev_u = np.concatenate([[u] * len(r) for u, r in sorted(rows.items())])
    ev_i = np.concatenate([r for _, r in sorted(rows.items())])
    return ev_u.astype(np.int32), ev_i.astype(np.int32), 305, 55, [0, 1, 5, 6, 299]
