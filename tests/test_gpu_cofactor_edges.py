"""GPU: CoFactor's kernels (k_cof_solve, k_cof_cooccur, the level schedule) at the factor widths, stage
counts, branch combinations, level extremes, pass geometries and filter thresholds the goldens never reach.  Every input is
built here from a seed.

Yardsticks.  The co-occurrence CSR: bit for bit, dtypes included, against nc.cooccur_from_pairs and against a dense
C = B^T B with the rules as boolean masks written here.  The item sweep: nc.item_sweep / nc.iteration from identical
inputs.  Y and X: 1e-6 of the largest entry (the bound of test_gpu_cofactor.py).  G, w, c: per case
max(CONTRACT_FP64[key], MARGIN x the case's own distance between the fp64 contract and the same sweep in np.longdouble,
nc.item_sweep_ld / nc.iteration_ld): the device is another fp64 evaluation of the same sums, so it is as far from the contract
as the contract is from the exact result.  That figure is computed on the CPU, printed, and must stay below 1e-9 / MARGIN
(a case beyond it could not tell an fp32 solve from an fp64 one); no bound comes from a device run.

Two graphs carry the context counts, because a hub that has every other item as its context leaves no item without one:
'hub' holds 1, 15, 16, 17, 31, 32, 33 and n - 1 contexts, 'nohub' holds 0 (with and without pairs), 1, 15, ..., 33.
"""
import numpy as np
import pytest
from scipy.sparse import csr_matrix

from helpers import numpy_cofactor as nc
from test_cofactor_golden import MARGIN
from test_gpu_cofactor import CONTRACT_FP64

pytestmark = pytest.mark.gpu

ALPHA = 10.0
WORST = 1e-9                     # a bound above this could not tell fp32 state from fp64 state
STATE = ('G', 'w', 'c')


@pytest.fixture(scope='module')
def dev():
    from yue_amd._shim import Device
    d = Device(0, raise_errors=True)
    yield d
    d.close()


# ---- problems ----
class Problem:
    def __init__(self, R, edges, k, seed):
        self.R = np.asarray(R, np.int64)
        self.m, self.n = self.R.shape
        self.k = k
        self.um, self.im = nc.pairs_from_matrix(self.R)
        self.sp = nc.sppmi_from_edges(self.n, edges, seed + 1)
        rs = np.random.RandomState(seed)
        self.X0 = rs.rand(self.m, k).astype(np.float32)
        self.Y0 = rs.rand(self.n, k).astype(np.float32)
        self.G0 = 0.1 * rs.randn(self.n, k)                             # mixed signs: w_i / c_j swapped with w_j / c_i cannot cancel
        self.w0 = 0.3 * rs.randn(self.n)
        self.c0 = 0.3 * rs.randn(self.n)
        assert (self.G0 < 0).any() and (self.w0 < 0).any() and (self.c0 < 0).any() and (self.w0 > 0).any() and (self.c0 > 0).any()
        self.deg = np.diff(self.sp[0])
        self.users = np.diff(self.im[0])

    def start(self):
        return self.X0, self.Y0, self.G0, self.w0, self.c0


def listens(m, n, per_user, seed):
    """m x n event counts: per_user random items per user, 1..3 events each."""
    rng = np.random.RandomState(seed)
    R = np.zeros((m, n), np.int64)
    for u in range(m):
        R[u, rng.choice(n, per_user, replace=False)] = rng.randint(1, 4, per_user)
    return R


A_M, A_N = 96, 80
SPECIAL = [int(x) for x in np.random.RandomState(17).permutation(A_N)[:12]]      # ids spread over the range, fixed
HUB = SPECIAL[0]
DEGREES = dict(zip(SPECIAL[1:8], (1, 15, 16, 17, 31, 32, 33)))


def k_sweep_problem(k):
    rng = np.random.RandomState(23)
    edges = [(i, int(j)) for i in range(A_N) for j in rng.choice(np.delete(np.arange(A_N), i), 3, replace=False)]
    return Problem(listens(A_M, A_N, 8, 1), edges, k, 100 + k)


def context_problem(k, graph, long_rows=False, no_pairs=False):
    R = listens(A_M, A_N, 8, 2)
    degrees = dict(DEGREES)
    if graph == 'nohub':
        degrees.update({SPECIAL[8]: 0, SPECIAL[9]: 0})
        R[:, SPECIAL[9]] = 0                                            # neither pairs nor contexts
        R[:3, SPECIAL[8]] = 2                                           # pairs, no contexts
    if no_pairs:
        degrees.update({SPECIAL[10]: 1, SPECIAL[11]: 20})
        R[:, SPECIAL[10]] = 0
        R[:, SPECIAL[11]] = 0
    if long_rows:
        rng = np.random.RandomState(3)
        R[:70, HUB] = rng.randint(1, 4, 70)
        R[:81, SPECIAL[4]] = rng.randint(1, 4, 81)                      # the item with 17 contexts
    edges = nc.graph_with_degrees(A_N, degrees, HUB if graph == 'hub' else None, 29, filler_edges=40)
    P = Problem(R, edges, k, 200 + k)
    for t, d in degrees.items():
        assert P.deg[t] == d, (t, d)
    if graph == 'hub':
        assert P.deg[HUB] == A_N - 1
    return P


B_M, B_N, B_K = 120, 200, 20
GRAPHS = {
    'empty': [],
    'path': [(i, i + 1) for i in range(B_N - 1)],
    'star_first': [(0, i) for i in range(1, B_N)],
    'star_last': [(B_N - 1, i) for i in range(B_N - 1)],
    'matching': [(2 * t, 2 * t + 1) for t in range(B_N // 2)],
}
LEVELS = {'empty': 1, 'path': B_N, 'star_first': 2, 'star_last': 2, 'matching': 2}


def level_log(which):
    """Two logs of the same m and n whose long rows (more than 32 users) differ."""
    R = listens(B_M, B_N, 10, 40 + which)
    rng = np.random.RandomState(50 + which)
    for item, users in ((0, 100), (7, 70)) if which == 0 else ((0, 45), (150, 90), (199, 77)):
        R[:, item] = 0
        R[:users, item] = rng.randint(1, 4, users)
    return R


def level_problem(graph, which=0):
    return Problem(level_log(which), GRAPHS[graph], B_K, 300)          # one start and one set of SPPMI values for both logs


# ---- references and bounds ----
_REF = {}


def rel_ld(a, exact):
    return float(np.abs(np.asarray(a, nc.LD) - exact).max() / np.abs(exact).max())


def reference(tag, P, regU, regR, iters):
    """The contract after one item sweep and after `iters` iterations from P's start, and per key the distance of the fp64
    contract from the same operations in np.longdouble; computed once per tag."""
    if tag in _REF:
        return _REF[tag]
    X0, Y0, G0, w0, c0 = P.start()
    Yo, Go, wo, co = Y0.copy(), G0.copy(), w0.copy(), c0.copy()
    nc.item_sweep(X0, Yo, Go, wo, co, *P.im, *P.sp, regU, regR)
    Yl, Gl, wl, cl = Y0.copy(), G0.astype(nc.LD), w0.astype(nc.LD), c0.astype(nc.LD)
    nc.item_sweep_ld(X0, Yl, Gl, wl, cl, *P.im, *P.sp, regU, regR)
    ref = {'sweep': (Yo, Go, wo, co), 'fig_sweep': {'G': rel_ld(Go, Gl), 'w': rel_ld(wo, wl), 'c': rel_ld(co, cl)},
           'Y_sweep_same': bool(np.array_equal(Yo, Yl))}
    if iters:
        s = P.start()
        t = (X0, Y0, G0.astype(nc.LD), w0.astype(nc.LD), c0.astype(nc.LD))
        for _ in range(iters):
            s = nc.iteration(*s[:5], P.um, P.im, P.sp, regU, regR)
            t = nc.iteration_ld(*t, P.um, P.im, P.sp, regU, regR)
        ref['iters'] = s
        ref['fig_iters'] = {'G': rel_ld(s[2], t[2]), 'w': rel_ld(s[3], t[3]), 'c': rel_ld(s[4], t[4])}
        ref['XY_iters_same'] = bool(np.array_equal(s[0], t[0]) and np.array_equal(s[1], t[1]))
    for part in ('fig_sweep', 'fig_iters'):
        if part in ref:
            print(tag, part, 'contract vs longdouble', ref[part], 'bounds', {key: bound(ref[part], key) for key in STATE})
            for key in STATE:
                assert bound(ref[part], key) <= WORST, (tag, part, key, ref[part])      # else: the case is too badly conditioned, change its inputs
    _REF[tag] = ref
    return ref


def bound(fig, key):
    return max(CONTRACT_FP64[key], MARGIN * fig[key])


def upload(dev, P):
    dev.set_factors(P.X0, P.Y0)
    dev.wrmf_set_pairs(*(P.um + P.im))
    dev.cof_set_sppmi(*P.sp)
    dev.cof_set_state(P.G0, P.w0, P.c0)


def against(tag, what, got, want, fig):
    """got, want: (Y, G, w, c) or (X, Y, G, w, c)."""
    keys = ('X', 'Y', 'G', 'w', 'c')[5 - len(got):]
    err = {key: nc.rel(a, b) for key, a, b in zip(keys, got, want)}
    print(tag, what, 'device vs contract', err, 'bit-equal', {key: bool(np.array_equal(a, b)) for key, a, b in zip(keys, got, want)})
    for key, a, b in zip(keys, got, want):
        assert a.dtype == b.dtype and a.shape == b.shape, key
        assert np.isfinite(a).all(), key
        assert err[key] <= (1e-6 if key in 'XY' else bound(fig, key)), (tag, what, key, err[key])


def check(dev, tag, P, regU, regR, iters=2, uploaded=False):
    """One item sweep, then `iters` iterations from the start, against the contract; returns the sweep's (Y, G, w, c)."""
    ref = reference(tag, P, regU, regR, iters)
    if not uploaded:
        upload(dev, P)
    assert dev.get_option('cof_levels') == nc.levels_of(P.sp[0], P.sp[1]).max() + 1
    dev.cof_item_sweep(ALPHA, regU, regR)
    X, Y = dev.get_factors()
    G, w, c = dev.cof_get_state()
    assert np.array_equal(X, P.X0)
    against(tag, 'one sweep', (Y, G, w, c), ref['sweep'], ref['fig_sweep'])
    lone = np.flatnonzero((P.deg == 0) & (P.users > 0))                 # pairs, no contexts: G, w, c untouched
    assert np.array_equal(G[lone], P.G0[lone]) and np.array_equal(w[lone], P.w0[lone]) and np.array_equal(c[lone], P.c0[lone])
    none = np.flatnonzero((P.deg == 0) & (P.users == 0))                # neither: exactly 0, state untouched
    assert np.all(Y[none] == 0) and np.array_equal(G[none], P.G0[none]) and np.array_equal(w[none], P.w0[none]) and np.array_equal(c[none], P.c0[none])
    if iters:
        upload(dev, P)
        loss = 0.0
        for _ in range(iters):
            loss = dev.wrmf_half_sweep(0, ALPHA, regU)
            dev.cof_item_sweep(ALPHA, regU, regR)
        s = ref['iters']
        against(tag, '%d iterations' % iters, dev.get_factors() + dev.cof_get_state(), s[:5], ref['fig_iters'])
        print(tag, 'loss', loss, s[5])
        assert abs(loss - s[5]) <= 1e-6 * abs(s[5])
    return Y, G, w, c


# ---- A. k_cof_solve over k and context counts ----
@pytest.mark.parametrize('k,regR', [(1, 1.0), (3, 1.0), (5, 1.0), (15, 1.0), (17, 1.0), (63, 1.0), (65, 1.0), (65, 0.03), (127, 1.0), (127, 0.03)])
def test_factor_widths(dev, k, regR):
    P = k_sweep_problem(k)
    assert P.deg.min() >= 3 and P.users.min() >= 1
    check(dev, 'k%d_r%g' % (k, regR), P, 1.0, regR)


@pytest.mark.parametrize('graph', ['hub', 'nohub'])
@pytest.mark.parametrize('k', [20, 65])
def test_context_counts_at_the_stage_edges(dev, k, graph):
    P = context_problem(k, graph)                                       # asserts the degrees 1, 15, 16, 17, 31, 32, 33 (and n - 1 / 0)
    lone = (P.deg == 0) & (P.users > 0)
    none = (P.deg == 0) & (P.users == 0)
    if graph == 'hub':
        assert P.deg.max() == A_N - 1 and P.deg.min() == 1
    else:
        assert lone[SPECIAL[8]] and none[SPECIAL[9]]
    check(dev, 'contexts_%s_k%d' % (graph, k), P, 1.0, 1.0)             # the lone rows and the empty rows are checked in there


@pytest.mark.parametrize('k', [20, 65])
def test_long_rows_with_contexts(dev, k):
    P = context_problem(k, 'hub', long_rows=True)
    for item, contexts in ((HUB, A_N - 1), (SPECIAL[4], 17)):
        users = int(P.im[0][item + 1] - P.im[0][item])
        assert P.deg[item] == contexts and users > 64 and users % 32 != 0        # the chunk path: three chunks of 32 pairs, the last partial
    dev.set_option('wrmf_long_pairs', 32)
    try:
        check(dev, 'long_rows_k%d' % k, P, 1.0, 1.0)
    finally:
        dev.set_option('wrmf_long_pairs', 2048)


@pytest.mark.parametrize('k', [20, 65])
def test_contexts_without_pairs(dev, k):
    P = context_problem(k, 'hub', no_pairs=True)
    a, b = SPECIAL[10], SPECIAL[11]
    assert P.users[a] == 0 and P.users[b] == 0 and P.deg[a] == 1 and P.deg[b] == 20
    Y, G, w, c = check(dev, 'no_pairs_k%d' % k, P, 1.0, 1.0)
    Yo, Go, wo, co = _REF['no_pairs_k%d' % k]['sweep']
    fig = _REF['no_pairs_k%d' % k]['fig_sweep']
    for r in (a, b):                                                    # the two rows on their own, so that larger rows do not set the scale
        assert np.abs(Yo[r]).max() > 0 and not np.array_equal(Go[r], P.G0[r])
        assert nc.rel(Y[r], Yo[r]) <= 1e-6 and nc.rel(G[r], Go[r]) <= bound(fig, 'G')
        assert abs(w[r] - wo[r]) <= bound(fig, 'w') * np.abs(wo).max() and abs(c[r] - co[r]) <= bound(fig, 'c') * np.abs(co).max()


# ---- B. level-schedule extremes and the schedule cache ----
@pytest.mark.parametrize('graph', list(GRAPHS))
def test_level_schedule_extremes(dev, graph):
    P = level_problem(graph)
    level = nc.levels_of(P.sp[0], P.sp[1])
    assert level.max() + 1 == LEVELS[graph]
    if graph == 'star_first':
        assert level[0] == 0 and (level[1:] == 1).all()                 # every leaf in one launch
    if graph == 'star_last':
        assert level[-1] == 1 and (level[:-1] == 0).all()               # the hub last
    upload(dev, P)
    assert dev.get_option('cof_levels') == LEVELS[graph]
    Y, G, w, c = check(dev, 'levels_' + graph, P, 1.0, 1.0, iters=0, uploaded=True)
    if graph == 'empty':
        assert np.array_equal(G, P.G0) and np.array_equal(w, P.w0) and np.array_equal(c, P.c0)
        upload(dev, P)
        dev.wrmf_half_sweep(1, ALPHA, 1.0)
        Yw = dev.get_factors()[1]
        print('levels_empty: item sweep vs wrmf_half_sweep(1)', nc.rel(Y, Yw), 'bit-equal', bool(np.array_equal(Y, Yw)))
        assert nc.rel(Y, Yw) <= 1e-6


@pytest.mark.parametrize('change', ['sppmi', 'long_pairs', 'pairs'])
def test_schedule_cache_follows_what_it_depends_on(dev, change):
    first = level_problem('path' if change == 'sppmi' else 'star_first')
    second = level_problem('star_first', which=1 if change == 'pairs' else 0)
    assert (second.users > 32).sum() >= 2 and second.users[0] > 32      # long rows, the hub among them
    assert np.array_equal(first.X0, second.X0) and (change == 'sppmi' or all(np.array_equal(a, b) for a, b in zip(first.sp, second.sp)))
    assert not np.array_equal(first.users > 32, second.users > 32) or change != 'pairs'
    tag = 'cache_' + change
    ref = reference(tag, second, 1.0, 1.0, 0)
    try:
        dev.set_option('wrmf_long_pairs', 32 if change == 'pairs' else 2048)
        upload(dev, first)
        dev.cof_item_sweep(ALPHA, 1.0, 1.0)
        if change == 'sppmi':
            dev.cof_set_sppmi(*second.sp)
        elif change == 'long_pairs':
            dev.set_option('wrmf_long_pairs', 32)
        else:
            dev.wrmf_set_pairs(*(second.um + second.im))
        dev.cof_set_state(second.G0, second.w0, second.c0)
        dev.set_factors(second.X0, second.Y0)
        dev.cof_item_sweep(ALPHA, 1.0, 1.0)
        got = (dev.get_factors()[1],) + dev.cof_get_state()
        upload(dev, second)                                             # the same sweep after a fresh sequence of calls
        dev.cof_item_sweep(ALPHA, 1.0, 1.0)
        fresh = (dev.get_factors()[1],) + dev.cof_get_state()
    finally:
        dev.set_option('wrmf_long_pairs', 2048)
    for a, b in zip(got, fresh):
        assert np.array_equal(a, b)
    against(tag, 'after the change', got, ref['sweep'], ref['fig_sweep'])


# ---- C. k_cof_cooccur ----
def dense_cooccur(R, f):
    """C = B^T B on the 0/1 matrix, the three rules as masks: events >= f on both sides, count > f, no diagonal."""
    R = np.asarray(R, np.int64)
    B = (R > 0).astype(np.int64)
    C = B.T @ B
    part = R.sum(0) >= f
    keep = (C > f) & part[:, None] & part[None, :] & ~np.eye(R.shape[1], dtype=bool)
    rows, cols = np.nonzero(keep)
    return np.concatenate([[0], np.cumsum(keep.sum(1))]).astype(np.int64), cols.astype(np.int32), C[rows, cols].astype(np.int32)


def sparse_cooccur(R, f):
    """dense_cooccur for an n too large for an n x n array: the product on sparse matrices, the same masks per entry."""
    R = np.asarray(R, np.int64)
    Bt = csr_matrix((R.T > 0).astype(np.int64))
    C = (Bt @ Bt.T).tocsr()
    C.sort_indices()
    part = R.sum(0) >= f
    rows = np.repeat(np.arange(R.shape[1]), np.diff(C.indptr))
    keep = (C.data > f) & part[rows] & part[C.indices] & (rows != C.indices)
    ptr = np.concatenate([[0], np.cumsum(np.bincount(rows[keep], minlength=R.shape[1]))]).astype(np.int64)
    return ptr, C.indices[keep].astype(np.int32), C.data[keep].astype(np.int32)


def same_csr(got, want, what):
    for a, b in zip(got, want):
        assert a.dtype == b.dtype and np.array_equal(a, b), what


def cooccur(dev, R, f, passes, other=dense_cooccur):
    """The device's CSR for every pass size (the first one twice: no state of a call leaks into the next), each bit-equal
    to both references; returns the CSR."""
    m, n = R.shape
    um, im = nc.pairs_from_matrix(R)
    want = nc.cooccur_from_pairs(im[0], im[1], im[2], m, f)
    same_csr(other(R, f), want, 'the two references')
    dev.set_factors(np.zeros((m, 4), np.float32), np.zeros((n, 4), np.float32))
    dev.wrmf_set_pairs(*(um + im))
    try:
        for p in (passes[0],) + tuple(passes):
            dev.set_option('cof_pass_items', p)
            got = dev.cof_cooccur(f)
            same_csr(got, want, ('cof_pass_items', p, 'filter', f))
            assert got[0].dtype == np.int64 and got[1].dtype == np.int32 and got[2].dtype == np.int32
            assert dev.get_option('cof_cooccur_nnz') == len(want[1])
    finally:
        dev.set_option('cof_pass_items', 8192)
    return want


@pytest.mark.parametrize('f', [0, 1])
def test_pass_sizes_that_do_not_divide_the_read_out(dev, f):
    R = listens(200, 300, 12, 60)
    want = cooccur(dev, R, f, (64, 100, 257, 300, 8192))                # 257: the second pass holds 43 items, its read-out one item past 256
    assert len(want[1]) > 0


@pytest.mark.parametrize('n', [64, 256, 257])
def test_item_count_at_and_one_past_the_pass_size(dev, n):
    want = cooccur(dev, listens(100, n, 10, 61 + n), 0, (64, 256))
    assert len(want[1]) > 0


def test_two_passes_at_the_production_range(dev):
    m, n = 300, 8200
    rng = np.random.RandomState(62)
    R = np.zeros((m, n), np.int64)
    edge = np.concatenate([np.arange(8190, 8200), np.arange(0, 6)])
    for u in range(m):
        R[u, rng.choice(edge, 4, replace=False)] = rng.randint(1, 4, 4)
        free = rng.choice(np.arange(6, 8190), 26, replace=False)
        R[u, free] = rng.randint(1, 4, 26)
    assert ((R > 0).sum(1) == 30).all()
    ptr, idx, cnt = cooccur(dev, R, 0, (8192,), other=sparse_cooccur)
    straddling = 0
    for i in edge:                                                      # the rows on both sides of 8192, by set intersection
        row = dict(zip(idx[ptr[i]:ptr[i + 1]].tolist(), cnt[ptr[i]:ptr[i + 1]].tolist()))
        ui = np.flatnonzero(R[:, i])
        for j in edge:
            common = len(np.intersect1d(ui, np.flatnonzero(R[:, j]))) if j != i else 0
            assert row.get(int(j), 0) == common, (i, j)
            straddling += common > 0 and (i < 8192) != (j < 8192)
    assert straddling > 0


@pytest.mark.parametrize('f', [0, 1])
def test_dense_rows_fill_every_ballot(dev, f):
    R = np.zeros((40, 601), np.int64)
    R[:, :600] = 1
    R[0, 600] = 1                                                       # one item only user 0 has
    ptr, idx, cnt = cooccur(dev, R, f, (8192, 64))
    assert (np.diff(ptr)[:600] == (600 if f == 0 else 599)).all() and ptr[-1] - ptr[-2] == (600 if f == 0 else 0)
    assert set(cnt.tolist()) == ({40, 1} if f == 0 else {40})


def test_item_with_700_users_and_user_with_every_item(dev):
    m, n = 750, 300
    R = listens(m, n, 5, 63)
    R[:, 7] = 0
    R[:700, 7] = 1
    R[3, :] = 2
    assert (R[:, 7] > 0).sum() > 2 * 256 and (R[3] > 0).all()           # three cursor slots per thread; a list through every pass
    cooccur(dev, R, 0, (64, 8192))
    cooccur(dev, R, 2, (64,))


def threshold_log():
    R = np.zeros((8, 7), np.int64)
    R[0, 0], R[1, 0] = 2, 1         # item 0: 2 users, 3 events: takes part at f = 3
    R[0, 1], R[1, 1] = 1, 1         # item 1: 2 events: does not
    R[2:6, 2] = 1                   # items 2 and 3 share 4 users: kept at f = 3
    R[2:6, 3] = 1
    R[2:5, 4] = 1                   # item 4 shares exactly 3 users with 2 and 3: dropped
    R[6, 5] = 5                     # item 5: 1 user, 5 events: takes part, keeps no pair
    R[6, 6], R[7, 6] = 1, 1         # item 6: shares its one user with item 5
    return R


def test_filter_thresholds(dev):
    R = threshold_log()
    events = R.sum(0)
    assert events[0] == 3 and events[1] == 2 and events[5] == 5 and (R[:, 5] > 0).sum() == 1
    ptr, idx, cnt = cooccur(dev, R, 3, (8192, 64))
    assert list(np.diff(ptr)) == [0, 0, 1, 1, 0, 0, 0] and list(idx) == [3, 2] and list(cnt) == [4, 4]
    ptr, idx, cnt = cooccur(dev, R, 0, (8192,))                          # f = 0: every pair with a common user
    B = (R > 0).astype(np.int64)
    assert ptr[-1] == ((B.T @ B) > 0).sum() - 7 and cnt.min() == 1 and ptr[6] - ptr[5] == 1
    ptr, idx, cnt = cooccur(dev, R, 100, (8192,))                        # above every count: an empty CSR
    assert dev.get_option('cof_cooccur_nnz') == 0 and not ptr.any() and len(idx) == 0 and len(cnt) == 0
    ptr, idx, cnt = cooccur(dev, R, 2, (8192,))                          # ... and the next call still works
    assert ptr[-1] == 6                                                 # 2-3, 2-4, 3-4 both ways


def test_event_counts_saturate(dev):
    big = 1 << 30
    R = np.zeros((5, 4), np.int64)
    R[:3, 0] = big                  # item 0: 3 * 2^30 events, more than an int32 holds
    R[:3, 1] = 1                    # item 1 shares the three users
    R[3, 2], R[4, 2] = big, big - 2                                     # item 2: 2^31 - 2 events
    R[3, 3], R[4, 3] = 1, 1
    um, im = nc.pairs_from_matrix(R)
    dev.set_factors(np.zeros((5, 4), np.float32), np.zeros((4, 4), np.float32))
    dev.wrmf_set_pairs(*(um + im))                                      # counts of 2^30 are admitted
    assert R[:, 0].sum() > 2 ** 31 - 1 and R[:, 2].sum() == 2 ** 31 - 2
    ptr, idx, cnt = cooccur(dev, R, 2, (8192,))                          # a sum that wrapped would be negative: item 0 would drop out
    assert list(ptr) == [0, 1, 2, 2, 2] and list(idx) == [1, 0] and list(cnt) == [3, 3]
    ptr, idx, cnt = cooccur(dev, R, 2 ** 31 - 1, (8192,))                # item 0 takes part (INT_MAX >= f), item 2 does not; no count exceeds f
    assert ptr[-1] == 0


# ---- D. refusals of the sweep ----
def refusal_problem(k):
    R = listens(A_M, A_N, 8, 4)
    R[:, 0] = 0                     # item 0: neither pairs nor contexts
    R[:2, 1] = 1                    # item 1: pairs only
    R[:, 2] = 0                     # item 2: nothing either
    edges = nc.graph_with_degrees(A_N, {0: 0, 1: 0, 2: 0}, None, 31, filler_edges=150)
    return Problem(R, edges, k, 400)


def test_k_above_128_is_refused(dev):
    from yue_amd._shim import YueHipError
    upload(dev, refusal_problem(129))
    with pytest.raises(YueHipError, match='k = 129'):
        dev.cof_item_sweep(ALPHA, 1.0, 1.0)
    check(dev, 'refusal_k20', refusal_problem(20), 1.0, 1.0, iters=0)


@pytest.mark.parametrize('which', ['regR', 'regU'])
def test_non_positive_pivot_names_the_first_row(dev, which):
    from yue_amd._shim import YueHipError
    P = refusal_problem(20)
    with_contexts = int(np.flatnonzero(P.deg > 0)[0])
    with_anything = int(np.flatnonzero((P.deg > 0) | (P.users > 0))[0])
    assert with_anything == 1 and with_contexts > 2
    upload(dev, P)
    row = with_contexts if which == 'regR' else with_anything
    with pytest.raises(YueHipError, match=r'non-positive pivot.*item row %d\b' % row):
        dev.cof_item_sweep(ALPHA, -1e6 if which == 'regU' else 1.0, -1e6 if which == 'regR' else 1.0)
    check(dev, 'refusal_k20', P, 1.0, 1.0, iters=0)                     # the context is still usable
