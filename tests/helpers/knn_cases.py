"""Synthetic UserKNN problems from seeds, built to stand on the internal limits of k_knn_neighbors, k_knn_topn and
k_knn_predict_scores (yue_amd/csrc/knn_kernels.hpp).  Shared by tests/test_rank_edge_cases.py, which asserts on the CPU that
every case reaches its branch (`reach`, computed from the events and the oracle tests/helpers/numpy_userknn.py alone, never from
a device result), and by tests/test_gpu_userknn_edges.py.  A case is built once and cached; nothing changes it afterwards.

A case: ev_ptr / ev_i / n (events, no device needed), pairs (the oracle's pair lists), users (the users to check), Ks, Ns,
options (knn_range / knn_gather settings to run at) and reach."""
import numpy as np

from . import numpy_userknn as ok

THREADS = 256                   # kKnnThreads: the chunk of the c0 loop over a user's own items, of the touched-list blocks, and
                                # the block of k_knn_predict_scores
SORT_CAP = 2048                 # kKnnSortCap: running top-K + appended candidates; a block of THREADS must still fit
GATHER = 2048                   # kKnnGather: (item, rank) entries per chunk of k_knn_topn, the upper end of option knn_gather
GATHER_MIN = 256                # kKnnMaxK: the lower end of option knn_gather (width = gather / kp >= 1 item per chunk)
RANGE = 4096                    # kKnnRange: candidate users per counting pass, the upper end of option knn_range
RANGE_MIN = 64                  # the lower end of option knn_range
DEFAULTS = {'knn_range': RANGE, 'knn_gather': GATHER}
SAMPLE = 40                     # users checked per case, where a case has more

_cache = {}


def _events(lists, counts=None):
    """ev_ptr / ev_i of per-user item lists; counts[u][t] repeats item t of user u (events, so counts > 1)."""
    out = []
    for u, items in enumerate(lists):
        c = np.ones(len(items), np.int64) if counts is None else np.asarray(counts[u], np.int64)
        out.append(np.repeat(np.asarray(items, np.int64), c))
    ev_ptr = np.concatenate([[0], np.cumsum([len(x) for x in out])]).astype(np.int64)
    return ev_ptr, (np.concatenate(out) if ev_ptr[-1] else np.zeros(0)).astype(np.int32)


def _sample(rs, m, always):
    """About SAMPLE users: the first, the last, every user of `always`, the rest drawn."""
    keep = set([0, m - 1]) | set(int(u) for u in always)
    rest = [u for u in rs.permutation(m) if u not in keep]
    return np.array(sorted(keep | set(int(u) for u in rest[:max(0, SAMPLE - len(keep))])), np.int64)


def _finish(name, lists, n, users, Ks, Ns, options, counts=None, **extra):
    ev_ptr, ev_i = _events(lists, counts)
    c = dict(name=name, ev_ptr=ev_ptr, ev_i=ev_i, n=n, m=len(lists), users=np.asarray(users, np.int64), Ks=Ks, Ns=Ns, options=options)
    c['pairs'] = ok.pairs_from_events(ev_ptr, ev_i, n)
    c.update(extra)
    return c


def oracle_neighbors(c, K, users=None):
    """The oracle's (nbr, inter, union) of the case's checked users (or `users`), cached per K."""
    users = c['users'] if users is None else np.asarray(users)
    key = (c['name'], K, tuple(users.tolist()))
    if key not in _cache:
        (up, ui, uc), (ip, iu) = c['pairs']
        _cache[key] = ok.neighbors(up, ui, ip, iu, K, users)
    return _cache[key]


def candidates(c, u):
    """Users other than u that share an item with u: the touched counters of k_knn_neighbors minus u itself."""
    (up, ui, uc), (ip, iu) = c['pairs']
    seen = np.unique(np.concatenate([iu[ip[i]:ip[i + 1]] for i in ui[up[u]:up[u + 1]]] + [np.zeros(0, np.int32)]))
    return int((seen != u).sum())


def gathered(c, u, K):
    """(kp, entries): u's positive neighbours and the sum of their list lengths: total_all of k_knn_topn before its clamp."""
    (up, ui, uc), _ = c['pairs']
    nbr, _, _ = oracle_neighbors(c, K, np.array([u]))
    pos = nbr[0][nbr[0] >= 0]
    return len(pos), int(np.diff(up)[pos].sum())


# --- cap_*: the sort capacity of k_knn_neighbors --------------------------------------------------------------------------
# every user holds item 0, so every user's candidate count is m - 1; 1 to 4 more items from a pool of 12 keep the similarities
# to few distinct ratios, so the K-th place lies inside a group of equal ratios for most users
def _cap(name, cand, knn_range=RANGE):
    rs = np.random.RandomState(1400 + cand)
    m, n = cand + 1, 13
    lists = [np.concatenate([[0], 1 + rs.choice(12, rs.randint(1, 5), replace=False)]) for _ in range(m)]
    counts = [rs.randint(1, 3, len(x)) for x in lists]
    c = _finish(name, lists, n, _sample(rs, m, []), Ks=[1, 20, 256], Ns=[10], options=[dict(DEFAULTS, knn_range=knn_range)], counts=counts)
    nbr, inter, uni = oracle_neighbors(c, 21)
    tie = inter[:, 19].astype(np.int64) * uni[:, 20] == inter[:, 20].astype(np.int64) * uni[:, 19]
    c['reach'] = dict(candidates=sorted(set(candidates(c, u) for u in c['users'])), tie_at_20=int((tie & (nbr[:, 20] >= 0)).sum()))
    # with one pass (range >= m) the touched list holds the candidates and u: the mid-run merge comes once a block starts at
    # occupied >= SORT_CAP - THREADS + 1, so for certain when there is a block past SORT_CAP touched entries
    c['reach']['mid_run_merge_certain'] = bool(cand + 1 > SORT_CAP) if knn_range >= m else bool(cand >= SORT_CAP - THREADS + 1 + knn_range)
    return c


# --- row_*: the c0 loop over the user's own items ---------------------------------------------------------------------------
def _row(name, du):
    rs = np.random.RandomState(1500 + du)
    m, n, long_user = 301, 700, 150
    lists = [rs.choice(n, rs.randint(1, 31), replace=False) for _ in range(m)]
    lists[long_user] = rs.choice(n, du, replace=False)
    counts = [rs.randint(1, 4, len(x)) for x in lists]
    c = _finish(name, lists, n, [long_user], Ks=[20], Ns=[20], counts=counts,
                options=[dict(DEFAULTS), dict(DEFAULTS, knn_range=RANGE_MIN)], long_user=long_user)
    nbr, _, _ = oracle_neighbors(c, 20, np.arange(m))
    has_long = np.flatnonzero((nbr == long_user).any(axis=1))
    c['users'] = _sample(rs, m, [long_user] + list(has_long[:SAMPLE - 3]))
    (up, ui, uc), _ = c['pairs']
    c['reach'] = dict(long_row=int(up[long_user + 1] - up[long_user]), users_with_long_neighbour=int(np.isin(c['users'], has_long).sum()),
                      counts_above_1=int((uc > 1).sum()))
    return c


# --- range_*: m against the pass width ----------------------------------------------------------------------------------------
def _range(name, m):
    rs = np.random.RandomState(1600 + m)
    n = 40
    lists = [rs.choice(n, rs.randint(1, 7), replace=False) for _ in range(m)]
    counts = [rs.randint(1, 3, len(x)) for x in lists]
    c = _finish(name, lists, n, np.arange(m), Ks=[10], Ns=[10], counts=counts, options=[dict(DEFAULTS, knn_range=RANGE_MIN)])
    passes = -(-m // RANGE_MIN)
    c['reach'] = dict(m=m, passes=passes, last_pass=m - (passes - 1) * RANGE_MIN)
    return c


# --- kp_*: the rank in the low 8 bits of the scoring key -------------------------------------------------------------------
def _kp(name, K):
    rs = np.random.RandomState(1700 + K)
    m, n = 300, 60                                       # n <= 64: at knn_gather = 256 the width is 1 item per chunk, n chunks
    lists = [np.concatenate([[0], 1 + rs.choice(n - 1, rs.randint(1, 6), replace=False)]) for _ in range(m)]
    counts = [rs.randint(1, 4, len(x)) for x in lists]
    c = _finish(name, lists, n, _sample(rs, m, []), Ks=[K], Ns=[100, 1], counts=counts,
                options=[dict(DEFAULTS), dict(DEFAULTS, knn_gather=GATHER_MIN)])
    nbr, inter, uni = oracle_neighbors(c, K)
    sims = ok.sims(inter, uni)
    c['reach'] = dict(kp_min=int((nbr >= 0).sum(axis=1).min()), width_at_256=GATHER_MIN // K,
                      # the ranks r and r - 128 must differ in similarity for a rank cut to 7 bits to show
                      sims_differ_128_apart=int((sims[:, 128:K] != sims[:, :K - 128]).any(axis=1).sum()))
    return c


# --- gather_*: the chunked decision total_all <= gather ------------------------------------------------------------------------
# two closed blocks of 100 items: a ranked user holding one item, and four neighbours holding that item plus 63 (one of the
# second block's: 64) others, so the lists of the ranked user's positive neighbours sum to 256 and to 257
def _gather(name):
    rs = np.random.RandomState(1800)
    lists = []
    for base, extra in ((0, 0), (100, 1)):
        lists.append(np.array([base]))
        for t in range(4):
            lists.append(np.concatenate([[base], base + 1 + rs.choice(99, 63 + (extra if t == 3 else 0), replace=False)]))
    counts = [rs.randint(1, 4, len(x)) for x in lists]
    u = 0 if name == 'gather_eq' else 5
    c = _finish(name, lists, 200, [u], Ks=[4], Ns=[100, 5], counts=counts, options=[dict(DEFAULTS, knn_gather=GATHER_MIN)])
    kp, entries = gathered(c, u, 4)
    c['reach'] = dict(kp=kp, entries=entries, gather=GATHER_MIN, chunked=int(entries > GATHER_MIN))
    return c


# --- ones: every score exactly 1.0 ---------------------------------------------------------------------------------------------
def _ones(name):
    rs = np.random.RandomState(1900)
    m, n, K = 120, 300, 20
    lists = [rs.choice(n, rs.randint(5, 26), replace=False) for _ in range(m)]
    counts = [np.ones(len(x), np.int64) for x in lists]
    if name == 'ones_few2':                             # a handful of counts of 2, on high item ids: in late chunks
        for u in rs.choice(m, 12, replace=False):
            counts[u][np.argmax(lists[u])] = 2
    c = _finish(name, lists, n, _sample(rs, m, []), Ks=[K], Ns=[1, 7, 100], counts=counts, options=[dict(DEFAULTS, knn_gather=GATHER_MIN)])
    (up, ui, uc), _ = c['pairs']
    nbr, inter, uni = oracle_neighbors(c, K)
    chunked, all_one, above_one, spans, cut100 = 0, 0, 0, 0, 0
    for t, u in enumerate(c['users']):
        kp, entries = gathered(c, u, K)
        chunked += entries > GATHER_MIN
        it, sc = ok.topn(up, ui, uc, u, nbr[t], inter[t], uni[t], n, 101)
        cut100 += len(it) == 101                                               # N = 100 cuts the list
        all_one += bool((sc == 1.0).all())
        above_one += bool((sc > 1.0).any())
        width = GATHER_MIN // max(kp, 1)
        spans += len(it) >= 7 and it[6] // width > it[0] // width              # the first 7 come from more than one chunk
    c['reach'] = dict(users=len(c['users']), chunked=int(chunked), all_scores_one=int(all_one), some_score_above_one=int(above_one),
                      first7_span_chunks=int(spans), cut_at_100=int(cut100), counts_of_2=int((uc == 2).sum()), counts_max=int(uc.max()))
    return c


# --- own_only: neighbours that hold nothing but the user's own items --------------------------------------------------------
def _own_only(name):
    rs = np.random.RandomState(2000)
    m, n = 30, 40
    lists = [3 + rs.choice(n - 3, rs.randint(1, 7), replace=False) for _ in range(m)]
    lists[4], lists[9], lists[17] = np.array([0, 1, 2]), np.array([1, 0]), np.array([2])
    c = _finish(name, lists, n, np.arange(m), Ks=[10], Ns=[10], options=[dict(DEFAULTS)], own_user=4)
    nbr, _, _ = oracle_neighbors(c, 10)
    c['reach'] = dict(neighbours=sorted(int(v) for v in nbr[4] if v >= 0))
    return c


# --- predict_n*: the block edge of k_knn_predict_scores ---------------------------------------------------------------------
def _predict(name, n):
    rs = np.random.RandomState(2100 + n)
    m = 60
    lists = [rs.choice(n, rs.randint(3, 21), replace=False) for _ in range(m)]
    for u in range(6):                                  # users 0..5 share item 0 and hold the last item and item 255 (where there is one past it)
        lists[u] = np.unique(np.concatenate([lists[u], [0, n - 1, min(n - 1, 255), n - 2]]))
    counts = [rs.randint(1, 4, len(x)) for x in lists]
    c = _finish(name, lists, n, np.arange(m), Ks=[20], Ns=[20], counts=counts, options=[dict(DEFAULTS)])
    (up, ui, uc), _ = c['pairs']
    nbr, inter, uni = oracle_neighbors(c, 20)
    it, _ = ok.predict(up, ui, uc, nbr[0], inter[0], uni[0], n)
    c['reach'] = dict(n=n, blocks=-(-n // THREADS), last_item_scored=bool((it == n - 1).any()))
    return c


BUILDERS = {}
for _cand in (1792, 1793, 2048, 2304):
    BUILDERS['cap_%d' % _cand] = (_cap, _cand)
BUILDERS['cap_2304_range64'] = (lambda name, cand: _cap(name, cand, RANGE_MIN), 2304)
for _du in (255, 256, 257, 600):
    BUILDERS['row_%d' % _du] = (_row, _du)
for _m in (64, 65, 128, 129):
    BUILDERS['range_m%d' % _m] = (_range, _m)
for _K in (256, 255):
    BUILDERS['kp_%d' % _K] = (_kp, _K)
for _n in (255, 256, 257):
    BUILDERS['predict_n%d' % _n] = (_predict, _n)
for _name, _fn in (('gather_eq', _gather), ('gather_over', _gather), ('ones', _ones), ('ones_few2', _ones), ('own_only', _own_only)):
    BUILDERS[_name] = (_fn,)

FAMILIES = {
    'cap': ['cap_1792', 'cap_1793', 'cap_2048', 'cap_2304', 'cap_2304_range64'],
    'row': ['row_255', 'row_256', 'row_257', 'row_600'],
    'range': ['range_m64', 'range_m65', 'range_m128', 'range_m129'],
    'kp': ['kp_256', 'kp_255'],
    'gather': ['gather_eq', 'gather_over'],
    'ones': ['ones', 'ones_few2'],
    'own_only': ['own_only'],
    'predict': ['predict_n255', 'predict_n256', 'predict_n257'],
}
NAMES = [name for fam in FAMILIES.values() for name in fam]


def build(name):
    if name not in _cache:
        fn = BUILDERS[name]
        c = fn[0](name, *fn[1:])
        for v in c.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _cache[name] = c
    return _cache[name]
