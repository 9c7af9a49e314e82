"""GPU: CUNE's user-network stage (yue_cnet_*) at the shapes where its kernels can break, against
the NumPy contract (tests/helpers/numpy_cune_net.py).  Companion of tests/test_gpu_cnet.py, same yardsticks:

walks      exact.
friends    exact ids, cosines within 1e-12.
embedding  the float64 contract is the yardstick; the tolerance on the device's float32 result is 8 x the largest
           element-wise gap between the contract's own float32 and float64 runs on the same input.

Every case asserts on the contract side that its input reaches the branch it is there for (a case that stops exercising
its branch fails).  Gap, tolerance and device error print before they are asserted; measured values: DESIGN.md section 18."""
import functools

import numpy as np
import pytest

from helpers import numpy_cune_net as cn
from util import gj, gz

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    from yue_amd._shim import Device
    d = Device(0, raise_errors=True)
    yield d
    d.close()


def upload(dev, ev_u, ev_i, m, n):
    (up, ui), (ip, iu) = cn.pairs_from_events(ev_u, ev_i, m, n)
    dev.cnet_set_pairs(m, n, up, ui, ip, iu)
    return cn.Net(up, ui, ip, iu)


# ---------------------------------------------------------------- embedding ----
def check_embedding(dev, label, walks, m, w64, gap, dim, window, epochs, seed, negative, rw):
    tol = 8 * gap
    dev.cnet_set_walks(m, walks)
    W = dev.cnet_embed(dim, window, epochs, seed, negative=negative, round_walks=rw)
    err = float(np.abs(W.astype(np.float64) - w64).max())
    print('embed %s: contract gap %.3e, tolerance %.3e, device error %.3e, max |w| %.3e' % (label, gap, tol, err, np.abs(w64).max()))
    assert W.dtype == np.float32 and W.shape == (m, dim)
    assert gap > 0 and err <= tol
    return W


def test_embedding_trained_regime_from_the_golden(dev):
    """g15_cune_trained (tools/make_cune_net_goldens.py --trained): 64 walks of L = 64 inside 2 groups of 32 users, dim 20,
    40 epochs -- the fewest tens of epochs at which the contract's largest |logit| is >= 4 (4.21; 2.68 at 30) while no
    logit reaches the |f| >= 6 cut-off, so the sigmoid's slope and sign decide the result.  Every lane is active (L = 64:
    bit 63 of the keep and modified masks)."""
    z, q = gz('g15_cune_trained.npz'), gj('g15_cune_trained.json')
    walks = z['walks']
    assert walks.shape == (q['nw'], q['L']) == (64, 64) and (q['m'], q['dim'], q['window'], q['negative'], q['round_walks']) == (64, 20, 5, 5, 8)
    assert (walks // 32 == walks[:, :1] // 32).all() and walks.max() == 63           # every walk stays inside its group
    assert min(q['max_abs_f'].values()) >= 4.0 and max(q['cutoffs'].values()) == 0 and q['epochs'] % 10 == 0
    W = check_embedding(dev, 'trained (largest |f| %.2f, %d epochs)' % (q['max_abs_f']['float64'], q['epochs']), walks, q['m'], z['W'],
                        q['gap'], q['dim'], q['window'], q['epochs'], q['embed_seed'], q['negative'], q['round_walks'])
    assert np.abs(W).max() > 0.5                                                    # trained: the initial rows are below 0.025


def rand_walks(seed, lo, hi, nw, L):
    return np.random.RandomState(seed).randint(lo, hi, (nw, L)).astype(np.int32)


def one_id_walk():
    w = rand_walks(27, 0, 64, 64, 10)
    w[0] = 7
    return w


def case(walks, m, dim=20, window=5, negative=5, rw=8, epochs=2, **expect):
    return dict(walks=walks, m=m, dim=dim, window=window, negative=negative, rw=rw, epochs=epochs, expect=expect)


EDGES = {
    # more than 64 distinct syn1neg rows in one walk: the second 64-wide chunk of the ids1 search; L = 64
    'targets_over_64': lambda: case(rand_walks(21, 0, 200, 16, 64), 200, targets_over=64),
    # a partial last round (70 = 8 * 8 + 6 = 64 + 6) and fewer walks than a round
    'nw70_rw8': lambda: case(rand_walks(22, 0, 64, 70, 10), 64, rw=8),
    'nw70_rw64': lambda: case(rand_walks(22, 0, 64, 70, 10), 64, rw=64),
    'nw5_rw64': lambda: case(rand_walks(23, 0, 64, 5, 10), 64, rw=64),
    # users in no walk: trailing ones (the host loop that closes the negative table), and id 0 with the last three
    'absent_trailing': lambda: case(rand_walks(24, 0, 64, 64, 10), 80, absent=list(range(64, 80))),
    'absent_first_and_last': lambda: case(rand_walks(25, 1, 77, 64, 10), 80, absent=[0, 77, 78, 79]),
    # the edges of the KR split (65: one live element in the second register)
    'dim1': lambda: case(rand_walks(26, 0, 64, 64, 10), 64, dim=1),
    'dim64': lambda: case(rand_walks(26, 0, 64, 64, 10), 64, dim=64),
    'dim65': lambda: case(rand_walks(26, 0, 64, 64, 10), 64, dim=65),
    'negative0': lambda: case(rand_walks(26, 0, 64, 64, 10), 64, negative=0),
    'negative64': lambda: case(rand_walks(26, 0, 64, 64, 10), 64, negative=64),
    'window1': lambda: case(rand_walks(26, 0, 64, 64, 10), 64, window=1),
    'window100': lambda: case(rand_walks(26, 0, 64, 64, 10), 64, window=100),
    # subsampling keeps about one word in ten: walks with no word, with one word (no context), and walks that train
    'mostly_subsampled': lambda: case(rand_walks(28, 0, 3, 16, 10), 3, kept_0_1_and_more=True),
    'one_id_repeated': lambda: case(one_id_walk(), 64, first_walk_one_id=True),
    # the largest layout the LDS check accepts at L = 64, negative = 5 (dim 34 is refused: test_embedding_lds_limit)
    'lds_largest': lambda: case(rand_walks(29, 0, 64, 8, 64), 64, dim=33, epochs=1),
}


@pytest.mark.parametrize('name', sorted(EDGES))
def test_embedding_shape_edges(dev, name):
    c = EDGES[name]()
    walks, m, expect = c['walks'], c['m'], c['expect']
    args = (walks, m, c['dim'], c['window'], c['epochs'], 3)
    kw = dict(negative=c['negative'], round_walks=c['rw'])
    stats = {}
    w32 = cn.embed(*args, dtype=np.float32, **kw)
    w64 = cn.embed(*args, dtype=np.float64, stats=stats, **kw)
    # the input reaches its branch (contract side)
    nw, L = walks.shape
    assert len(stats['kept']) == c['epochs'] * nw and stats['cutoffs'] == 0
    if 'targets_over' in expect:
        assert max(stats['targets']) > expect['targets_over'] and L == 64
    else:
        assert max(stats['targets']) <= L * (c['negative'] + 1)
    if name.startswith('nw'):
        assert nw % c['rw'] != 0
    if 'absent' in expect:
        assert sorted(set(range(m)) - set(walks.ravel().tolist())) == expect['absent']
    if expect.get('kept_0_1_and_more'):
        kept, trained = np.array(stats['kept']), np.array(stats['trained'])
        assert (kept == 0).any() and (kept == 1).any() and (trained > 0).any()
        assert (trained[kept <= 1] == 0).all()
    if expect.get('first_walk_one_id'):
        assert len(set(walks[0].tolist())) == 1 and max(stats['trained'][0::nw]) > 0          # ... and it trains
    if c['window'] == 1:
        assert max(stats['trained']) > 0
    gap = float(np.abs(w32.astype(np.float64) - w64).max())
    W = check_embedding(dev, name, walks, m, w64, gap, c['dim'], c['window'], c['epochs'], 3, c['negative'], c['rw'])
    if 'absent' in expect:
        assert (W[expect['absent']] == 0).all() and (w64[expect['absent']] == 0).all()
        present = np.setdiff1d(np.arange(m), expect['absent'])
        assert (np.abs(W[present]).max(axis=1) > 0).all()


def test_embedding_lds_limit(dev):
    """L (negative + 2) dim 4 + L (negative + 1) 4 <= 61440: at L = 64, negative = 5 dim 33 needs 60672 bytes, dim 34 62464."""
    from yue_amd._shim import YueHipError
    dev.cnet_set_walks(64, rand_walks(29, 0, 64, 8, 64))
    assert dev.cnet_embed(33, 5, 1, 3).shape == (64, 33)
    with pytest.raises(YueHipError, match='must fit 60 KiB of LDS'):
        dev.cnet_embed(34, 5, 1, 3)


def test_embedding_reuses_its_buffers(dev):
    """A second embedding of other sizes on the same context (accumulators, flags and lists are resized, not reallocated)
    gives the bits a fresh context gives."""
    from yue_amd._shim import Device
    long_walks, short_walks = rand_walks(30, 0, 64, 64, 10), rand_walks(31, 0, 48, 21, 6)
    dev.cnet_set_walks(64, long_walks)
    dev.cnet_embed(128, 5, 2, 3, negative=5)
    dev.cnet_set_walks(48, short_walks)
    again = dev.cnet_embed(20, 5, 2, 4, negative=64, round_walks=8)
    fresh = Device(0, raise_errors=True)
    try:
        fresh.cnet_set_walks(48, short_walks)
        want = fresh.cnet_embed(20, 5, 2, 4, negative=64, round_walks=8)
    finally:
        fresh.close()
    assert again.shape == want.shape == (48, 20) and np.abs(want).max() > 0
    assert np.array_equal(again.view(np.uint32), want.view(np.uint32))


# ---------------------------------------------------------------- walks ----
def log_clique():
    return np.repeat(np.arange(6), 2), np.tile([0, 1], 6), 6, 2


@pytest.mark.parametrize('T,L', [(256, 61), (240, 64), (15360, 2)])
def test_walks_at_the_lds_capacity_edge(dev, T, L):
    """visited[start] holds T (L - 1) ids in LDS: 15360 is the limit (60 KiB)."""
    ev_u, ev_i, m, n = log_clique()
    net = upload(dev, ev_u, ev_i, m, n)
    assert T * (L - 1) in (15360, 15120) and len(net.users) == 6
    stats = {}
    want = cn.walks(net, T, L, 5, stats)
    got = dev.cnet_walks(T, L, 5)
    assert got.dtype == np.int32 and got.shape == want.shape == (6 * T, L)
    assert np.array_equal(got, want)
    assert stats['cutoffs'] >= 1


def test_walks_past_the_lds_capacity_are_refused(dev):
    from yue_amd._shim import YueHipError
    ev_u, ev_i, m, n = log_clique()
    upload(dev, ev_u, ev_i, m, n)
    for T, L in ((15361, 2), (257, 61)):
        with pytest.raises(YueHipError, match=r'T \(L - 1\) <= 15360'):
            dev.cnet_walks(T, L, 5)


def test_walks_over_zero_width_prefix_entries_and_a_long_item_row(dev):
    ev_u, ev_i, m, n, marked = cn.singleton_log()
    net = upload(dev, ev_u, ev_i, m, n)
    width = {a: np.diff(np.concatenate([[0], net.pref[a]])) for a in marked}
    assert np.diff(net.i_ptr).max() == 300 and len(net.users) == 300 and all(net.total[a] > 0 for a in marked)
    assert all(width[a][0] == 0 and width[a][1] > 0 for a in (0, 1, 5))                      # a flat stretch at the start of the row,
    assert all(width[a][-1] == 0 and width[a][-2] > 0 for a in (0, 1, 6, 299))               # at its end,
    assert width[0].tolist()[1:6] == [299, 0, 0, 0, 2] and width[299].tolist()[:4] == [299, 0, 0, 1]      # and in the middle
    want = cn.walks(net, 3, 10, 5)
    got = dev.cnet_walks(3, 10, 5)
    assert got.shape == want.shape == (900, 10)
    assert np.array_equal(got, want)
    starts = want[:, 0]
    assert all((starts == a).sum() == 3 for a in marked) and not np.isin(got, np.arange(300, 305)).any()
    assert all(len(set(want[starts == a, 1:].ravel().tolist()) - {1, 2, 298}) > 0 for a in (0, 299))     # ... through the long row


# ---------------------------------------------------------------- friends ----
def spaced(sims, ids, K):
    """No two adjacent cosines of a user's first K + 1 contract entries closer than 1e-9 (the rule of the golden tool)."""
    s, v = sims[:, :K + 1], ids[:, :K + 1] >= 0
    d = s[:, :-1] - s[:, 1:]
    return bool((d[v[:, 1:]] > 1e-9).all())


def check_friends(dev, W, K, want_ids, want_sims):
    """want_*: the contract's lists at some K' >= K (its sort is stable and cut at K': the first K columns are its K-list)."""
    dev.cnet_set_embedding(W)
    ids, sims = dev.cnet_friends(K)
    w_ids, w_sims = want_ids[:, :K], want_sims[:, :K]
    if w_ids.shape[1] < K:
        pad = K - w_ids.shape[1]
        w_ids = np.pad(w_ids, ((0, 0), (0, pad)), constant_values=-1)
        w_sims = np.pad(w_sims, ((0, 0), (0, pad)), constant_values=0.0)
    assert ids.shape == sims.shape == (len(W), K)
    err = float(np.abs(sims - w_sims).max())
    print('friends nnet %d dim %d K %d: largest cosine error %.3e' % (W.shape[0], W.shape[1], K, err))
    assert np.array_equal(ids, w_ids)
    assert err <= 1e-12
    return ids, sims


ARC = {'nnet': 600, 'dim': 20, 'delta': 1.2e-3, 'bend': 1.9e-3, 'pad': 0.05}


@functools.lru_cache(maxsize=None)
def arc():
    """Rows (cos t_u, sin t_u, pad, ..., pad) with t_u = delta (u + bend u^2), 600 users, the whole arc 1.537 < pi / 2.  On an
    evenly spaced arc (bend = 0) users u - k and u + k are at the same angle from u and their cosines differ only by the
    float32 rounding of the rows: no delta makes the contract meet the spacing rule there (delta 2.5e-3: 15 472 of the 60 000
    adjacent pairs within 1e-9; 1e-3: 24 504), so the steps grow slightly (bend) -- the order in which a query meets its
    candidates, which is what the case is about, is that of the even arc.  With these values the contract's closest
    adjacent pair is 5.3e-9 apart."""
    u = np.arange(ARC['nnet'], dtype=np.float64)
    t = ARC['delta'] * (u + ARC['bend'] * u * u)
    assert t[-1] < np.pi / 2 and (np.diff(t) > 0).all()
    W = np.full((ARC['nnet'], ARC['dim']), ARC['pad'], np.float32)
    W[:, 0], W[:, 1] = np.cos(t), np.sin(t)
    ids, sims = cn.friends(W, np.arange(ARC['nnet']), 101)
    return W, ids, sims


@pytest.mark.parametrize('K', [1, 100])
def test_friends_ordered_adversary(dev, K):
    """The last query block meets its candidates from the farthest to the nearest: every candidate beats the running K-th
    entry, is appended, and the lists are merged as often as they can be (every second or third tile); the first block
    meets them in the opposite order and appends nothing once its list is full."""
    W, ids, sims = arc()
    assert spaced(sims, ids, K)
    n = ARC['nnet']
    assert ids[n - 1, :100].tolist() == list(range(n - 2, n - 102, -1)) and ids[0, :100].tolist() == list(range(1, 101))
    for q in range(n - 8, n):                                        # the contract's cosines rise with the candidate id up to the block
        s = [cn.cosine(W[q], W[b]) for b in range(0, n - 8, 37)]
        assert (np.diff(s) > 0).all()
    check_friends(dev, W, K, ids, sims)


@functools.lru_cache(maxsize=None)
def three_directions():
    base = np.abs(np.random.RandomState(41).randn(3, 20)).astype(np.float32)
    W = base[np.arange(300) % 3]                                      # ids interleaved: user u has direction u % 3
    ids, sims = cn.friends(W, np.arange(300), 100)
    return W, ids, sims


@pytest.mark.parametrize('K', [10, 100])
def test_friends_mass_ties(dev, K):
    """100 bit-equal rows per direction: within a direction the cosines are bit-equal and the id decides, across every tile
    and merge boundary, next to the -inf / INT_MAX padding of the merge."""
    W, ids, sims = three_directions()
    for a in (0, 1, 2, 299):
        same = [b for b in range(300) if b % 3 == a % 3 and b != a]
        assert ids[a, :99].tolist() == same and len(set(sims[a, :99].tolist())) == 1          # ascending ids, one cosine
        assert ids[a, 99] % 3 != a % 3 and sims[a, 99] < sims[a, 98] - 1e-6
    got, _ = check_friends(dev, W, K, ids, sims)
    assert (np.diff(got[:, :min(K, 99)], axis=1) > 0).all()


GRID_NNET = [1, 2, 8, 9, 63, 64, 65]


@functools.lru_cache(maxsize=None)
def grid_rows(nnet, dim):
    W = np.random.RandomState(1000 * dim + nnet).randn(nnet, dim).astype(np.float32)
    ids, sims = cn.friends(W, np.arange(nnet), 101)
    return W, ids, sims


def grid_cases():
    out = [(nnet, 20, K) for nnet in GRID_NNET for K in sorted({1, nnet - 1, nnet, 100} - {0})]
    return out + [(65, dim, K) for dim in (1, 127) for K in (1, 64, 65, 100)]


@pytest.mark.parametrize('nnet,dim,K', grid_cases())
def test_friends_size_grid(dev, nnet, dim, K):
    """nnet around the query block (8) and the candidate tile (64), K from 1 to past nnet - 1 (-1 / 0 padded), dim 1 and 127.
    dim = 1: every cosine is exactly 1 or -1 in the contract and on the device (x y / sqrt(x^2 y^2), every operation exact or
    correctly rounded), so the spacing rule is that of the two values and the id decides inside each."""
    W, ids, sims = grid_rows(nnet, dim)
    if dim == 1:
        assert set(np.unique(sims[ids >= 0]).tolist()) <= {1.0, -1.0}
    else:
        assert spaced(sims, ids, K)                                   # no user is excused by a near-tie
    assert ((ids >= 0).sum(axis=1) == min(nnet - 1, 101)).all()
    got, got_sims = check_friends(dev, W, K, ids, sims)
    if nnet == 1:
        assert (got == -1).all() and (got_sims == 0).all()
