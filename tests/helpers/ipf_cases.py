"""Synthetic IPF problems from seeds, built to stand on the internal limits of k_ipf_rank (yue_amd/csrc/ipf_kernels.hpp) and of
yue_ipf_set_graph (ipf_host.hip).  Shared by tests/test_rank_edge_cases.py, which asserts on the CPU that every case reaches its
branch (`reach`, computed from the events and the oracle tests/helpers/numpy_ipf.py alone, never from a device result), and by
tests/test_gpu_ipf_edges.py.  Event order matters to IPF: a case is its users' event sequences, written user-major; the oracle's
Graph and the plugin's ipf_graph derive every list from them.  Cases, graphs and oracle results are built once and cached.

A case: ev_ptr / ev_i / n, rho / beta / eta, users (the users to check), Ns and reach."""
import numpy as np

from . import numpy_ipf as oi

THREADS = 256                   # kIpfThreads: the chunk of the level-1 loop (c0), of the reached level-2 nodes (t0), of one scan pass
                                # over a holder list, and of the selection's candidate blocks
SEL = 1024                      # kIpfSel: running top-N + appended candidates of the selection; a block of THREADS must still fit
K_BITS = 18                     # kIpfKBits: a user's distinct items < 2^18 (level-1 index k, level-3 index j in the insertion key)
MAX_LIST = (1 << K_BITS) - 1    # the longest list yue_ipf_set_graph accepts
SAMPLE = 40                     # users checked per case, where a case has more

_cache = {}


def _finish(name, lists, n, users, Ns, rho=0.5, beta=0.7, eta=0.3, **extra):
    ev_ptr = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
    ev_i = np.concatenate([np.asarray(x, np.int64) for x in lists] + [np.zeros(0, np.int64)]).astype(np.int32)
    c = dict(name=name, ev_ptr=ev_ptr, ev_i=ev_i, n=n, m=len(lists), users=np.asarray(users, np.int64), Ns=Ns, rho=rho, beta=beta, eta=eta)
    c.update(extra)
    return c


def _sample(rs, m, always):
    keep = set([0, m - 1]) | set(int(u) for u in always)
    rest = [u for u in rs.permutation(m) if u not in keep]
    return np.array(sorted(keep | set(int(u) for u in rest[:max(0, SAMPLE - len(keep))])), np.int64)


def graph(c):
    """The oracle's Graph of a case."""
    key = ('graph', c['name'])
    if key not in _cache:
        _cache[key] = oi.Graph(c['ev_ptr'], c['ev_i'], c['n'], c['rho'], c['beta'], c['eta'])
    return _cache[key]


def device_graph(c):
    """What yue_ipf_set_graph takes (the plugin's ipf_graph; host arrays only)."""
    from yue_amd.recommender.cf.IPF import ipf_graph
    key = ('device', c['name'])
    if key not in _cache:
        _cache[key] = ipf_graph(c['ev_ptr'], c['ev_i'], c['n'], c['rho'], c['beta'], c['eta'])
    return _cache[key]


def predict(c, u):
    key = ('predict', c['name'], int(u))
    if key not in _cache:
        _cache[key] = oi.predict(graph(c), int(u))
    return _cache[key]


def topn(c, u, N):
    """oi.topn from the cached predict."""
    items, scores = predict(c, u)
    keep = ~np.isin(items, graph(c).D[0][int(u)])
    return items[keep][:N], scores[keep][:N]


def level2_K(g, u, p=0):
    """{b: K} of path p of u's query: K = the largest 1-based index of a start-list item that b holds (u left out on paths 0, 3)."""
    start, h = (0 if p < 2 else 1), p & 1
    K = {}
    for k, a in enumerate(g.D[start][u], 1):
        for b in g.H[h][a][0]:
            K[int(b)] = k
    if p in (0, 3):
        K.pop(int(u), None)
    return K


def tie_reach(c, N):
    """Checked users among whose first N + 1 candidates there are fewer than N distinct scores."""
    count = 0
    for u in c['users']:
        it, sc = topn(c, u, N + 1)
        count += len(it) == N + 1 and len(np.unique(sc)) < N
    return int(count)


def _random_lists(rs, m, n, lo, hi):
    return [rs.randint(0, n, rs.randint(lo, hi + 1)) for _ in range(m)]


# --- l1_*: level 1 with more than one chunk of distinct items ----------------------------------------------------------------
def _l1(name, L):
    rs = np.random.RandomState(2200 + L)
    m, n, long_user = 101, L + 60, 37
    order = rs.permutation(n)[:L]                       # the long list's order is not item-id order
    lists = _random_lists(rs, m, n, 3, 12)
    ev = list(order)
    for at in sorted(rs.randint(L // 2, L, 20)):        # repeats behind their first occurrence: UL is longer than the distinct list
        ev.insert(at, ev[rs.randint(0, 100)])
    lists[long_user] = np.array(ev)
    lists[90] = np.array([order[L - 1], order[0]])      # the last item of the list has a holder
    late = []
    if L > THREADS:                                     # holders of items of the second chunk only
        for b in range(91, 96):
            lists[b] = rs.choice(order[THREADS:min(L, 2 * THREADS)], 3)
            late.append(b)
    if L > 2 * THREADS:                                 # and of the third chunk only
        for b in range(96, 99):
            lists[b] = rs.choice(order[2 * THREADS:], 2)
            late.append(b)
    c = _finish(name, lists, n, _sample(rs, m, [long_user, 90] + late), Ns=[50], long_user=long_user)
    g = graph(c)
    K = level2_K(g, long_user, 0)
    c['reach'] = dict(list_len=len(g.D[0][long_user]), events=len(g.UL[long_user]), K_max=max(K.values()),
                      nodes_K_above_256=sum(k > THREADS for k in K.values()), nodes_K_above_512=sum(k > 2 * THREADS for k in K.values()))
    return c


# --- l2_*: the reached level-2 nodes against the t0 loop; a holder list longer than one scan pass ---------------------------------
def _l2(name, X):
    rs = np.random.RandomState(2300 + X)
    m, n = X + 6, 40
    lists = [np.array([0, n - 1])]                      # the querying user: the hub item and an item of its own
    for b in range(1, X + 1):
        other = rs.randint(1, n - 1, rs.randint(1, 5))
        lists.append(np.insert(other, rs.randint(0, len(other) + 1), 0))
    lists += [rs.randint(1, n - 1, rs.randint(1, 5)) for _ in range(5)]     # users outside the hub
    c = _finish(name, lists, n, _sample(rs, m, [0, 1, X]), Ns=[30])
    g = graph(c)
    K = level2_K(g, 0, 0)
    c['reach'] = dict(level2_nodes=len(K), hub_holders=len(g.H[0][0][0]), pos_max=int(g.H[0][0][1].max()))
    return c


# --- sel_*: the selection's capacity ----------------------------------------------------------------------------------------------
# user 0 holds items 0 and 1; 100 holders of item 0 share out exactly X other items, the low user ids (expanded last: pos desc)
# the short lists (large W2), so candidates that enter the selection late rank high
def _sel(name, X):
    rs = np.random.RandomState(2400 + X)
    H, spare = 100, 28
    n = X + 2 + spare
    sizes = np.maximum(1, (X * np.arange(1, H + 1)) // (H * (H + 1) // 2))
    sizes[-1] += X - sizes.sum()
    assert sizes.min() >= 1 and sizes.sum() == X
    owner = np.repeat(np.arange(H), sizes)
    items = 2 + rs.permutation(X)
    lists = [np.array([0, 1])]
    for b in range(H):
        mine = np.concatenate([items[owner == b], 2 + rs.randint(0, X, 2)])
        lists.append(np.insert(mine, rs.randint(0, len(mine) + 1), 0))
    lists += [X + 2 + rs.randint(0, spare, rs.randint(2, 6)) for _ in range(10)]        # unreachable from user 0
    c = _finish(name, lists, n, [0, 1, H, len(lists) - 1], Ns=[100, 1])
    g = graph(c)
    it, _ = predict(c, 0)
    own = int(np.isin(it, g.D[0][0]).sum())
    c['reach'] = dict(candidates=len(it) - own, reached=len(it), own_reached=own,
                      # the mid-run merge comes once a block of THREADS starts at occupied > SEL - THREADS, for certain when
                      # the reached items run past SEL and fewer than THREADS of them are the user's own
                      mid_run_merge_certain=bool(len(it) > SEL and own < THREADS))
    return c


# --- beta0 / rho0: order by the insertion key alone ---------------------------------------------------------------------------
def _ties(name):
    rs = np.random.RandomState(2500 if name == 'beta0' else 2501)
    if name == 'beta0':
        m, n = 80, 1500                                 # sparse: fewer than 100 items get a score above zero for many users
        c = _finish(name, _random_lists(rs, m, n, 11, 15), n, _sample(rs, m, []), Ns=[100, 10], rho=0.5, beta=0.0, eta=0.3)
    else:
        m, n = 80, 150
        c = _finish(name, _random_lists(rs, m, n, 5, 25), n, _sample(rs, m, []), Ns=[50, 10], rho=0.0, beta=0.5, eta=0.3)
    zeros = 0
    for u in c['users']:
        it, sc = topn(c, u, c['Ns'][0])
        zeros += bool((sc == 0.0).sum() >= 2)
    c['reach'] = dict(users=len(c['users']), users_with_ties_in_cut={N: tie_reach(c, N) for N in c['Ns']}, users_with_zero_scores_in_top=int(zeros))
    return c


# --- limit_k: a list at the end of K's bit field ------------------------------------------------------------------------------------
# oi.Graph builds this graph (262,147 events, 262,144 holder lists) in Python loops: measured 1.1 s on one CPU core, 1.6 s with the
# three users' predicts, well under the 10 s above which the lists would have to be built with vectorised NumPy here instead
def _limit_lists(extra=0):
    last = MAX_LIST - 1
    return [np.arange(MAX_LIST + extra), np.array([last, MAX_LIST]), np.array([last, 5])]


def _limit(name):
    c = _finish(name, _limit_lists(), 1 << K_BITS, [0, 1, 2], Ns=[5], rho=0.5, beta=0.7, eta=0.3)
    g = graph(c)
    K = level2_K(g, 0, 0)
    c['reach'] = dict(list_len=len(g.D[0][0]), K_max=max(K.values()), K_field=MAX_LIST - max(K.values()), n=c['n'])
    return c


def limit_k_over():
    """The device graph of limit_k with one more item on user 0 (host arrays only): 2^18 items, to be refused."""
    from yue_amd.recommender.cf.IPF import ipf_graph
    c = _finish('limit_k_over', _limit_lists(1), 1 << K_BITS, [0], Ns=[5])
    return ipf_graph(c['ev_ptr'], c['ev_i'], c['n'], c['rho'], c['beta'], c['eta'])


# --- combo: one graph with every kind of query, for a slot that serves them in turn -----------------------------------------------
def _combo(name):
    rs = np.random.RandomState(2600)
    L, X, S = 513, 700, 1500
    lists = [None] * 5
    # block L, items [0, 600): user 0 holds 513 distinct items; 60 users with short lists
    order = rs.permutation(600)[:L]
    lists[0] = np.concatenate([order, order[rs.randint(0, 100, 7)]])
    lists[1] = np.array([order[3], order[400]])         # the tiny user
    lists[2] = np.zeros(0, np.int64)                    # the user without events
    for _ in range(60):
        lists.append(rs.randint(0, 600, rs.randint(3, 12)))
    lists.append(np.array([order[512], order[300]]))
    # block H, items [600, 700): user 3 and 700 others hold the hub item 600
    lists[3] = np.array([600, 699])
    for _ in range(X):
        other = rs.randint(601, 699, rs.randint(1, 4))
        lists.append(np.insert(other, rs.randint(0, len(other) + 1), 600))
    # block S, items [700, 2202 + 20): user 4 holds 700 and 701; 100 holders of 700 share out 1500 others
    lists[4] = np.array([700, 701])
    owner = rs.randint(0, 100, S)
    items = 702 + rs.permutation(S)
    for b in range(100):
        mine = np.concatenate([items[owner == b], 702 + rs.randint(0, S, 2)])
        lists.append(np.insert(mine, rs.randint(0, len(mine) + 1), 700))
    n = 702 + S + 20
    c = _finish(name, lists, n, [0, 1, 2, 3, 4], Ns=[100, 20], order=[0, 1, 2, 3, 1, 4, 2, 0, 1])
    g = graph(c)
    it, _ = predict(c, 4)
    c['reach'] = dict(list_len=len(g.D[0][0]), K_max=max(level2_K(g, 0, 0).values()), level2_nodes=len(level2_K(g, 3, 0)),
                      candidates=len(it) - int(np.isin(it, g.D[0][4]).sum()), tiny=len(g.UL[1]), empty=len(g.UL[2]))
    return c


# --- replace_*: graphs set one after the other in one context ------------------------------------------------------------------
REPLACE = {'replace_A': (3000, 120, 200), 'replace_B': (3001, 120, 200), 'replace_C': (3002, 50, 90), 'replace_D': (3003, 400, 700)}


def _replace(name):
    seed, m, n = REPLACE[name]
    rs = np.random.RandomState(seed)
    c = _finish(name, _random_lists(rs, m, n, 0, 30), n, _sample(rs, m, []), Ns=[20], rho=1.0)
    c['reach'] = dict(m=m, n=n)
    return c


BUILDERS = {}
for _L in (256, 257, 513):
    BUILDERS['l1_%d' % _L] = (_l1, _L)
for _X in (255, 256, 257, 700):
    BUILDERS['l2_%d' % _X] = (_l2, _X)
for _X in (768, 769, 1024, 1500):
    BUILDERS['sel_%d' % _X] = (_sel, _X)
for _name, _fn in (('beta0', _ties), ('rho0', _ties), ('limit_k', _limit), ('combo', _combo)):
    BUILDERS[_name] = (_fn,)
for _name in REPLACE:
    BUILDERS[_name] = (_replace,)

FAMILIES = {
    'l1': ['l1_256', 'l1_257', 'l1_513'],
    'l2': ['l2_255', 'l2_256', 'l2_257', 'l2_700'],
    'sel': ['sel_768', 'sel_769', 'sel_1024', 'sel_1500'],
    'ties': ['beta0', 'rho0'],
    'limit': ['limit_k'],
    'combo': ['combo'],
    'replace': sorted(REPLACE),
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
