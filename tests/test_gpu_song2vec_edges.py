"""GPU: Song2vec's kernels at the shapes where they can go wrong, with the yardsticks of
test_gpu_song2vec.py: the iteration bit for bit against the contract in the device's form under both schedules; the
embedding of sentences against the float64 contract within 8 x the contract's own float32-vs-float64 gap (the rule of
test_gpu_cnet.py).  Each case asserts on the contract side that it reaches the branch it names.
"""
import numpy as np
import pytest

from helpers import numpy_cune_net as cn
from helpers import numpy_song2vec as ns

pytestmark = pytest.mark.gpu

H = dict(lRate=0.02, regU=1.0, regI=0.1, regB=0.2, alpha=0.5)
NONE = (np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.float64))


@pytest.fixture(scope='module')
def dev():
    from yue_amd._shim import Device
    d = Device(0, raise_errors=True)
    yield d
    d.close()


def init(m, n, k, seed=5):
    return [x.copy() for x in ns.init_from_seed(seed, m, n, k)]


def log_steps(lengths, n, seed=9, top=None):
    """(ev_ptr, ev_i, steps) of a log whose user u has lengths[u] events over n items (top: every user's first item)."""
    rng = np.random.RandomState(seed)
    rows = [(n * rng.rand(L) ** 2).astype(np.int32) for L in lengths]
    if top is not None:
        for r in rows:
            if len(r):
                r[0] = top
    ev_ptr = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    ev_i = np.concatenate(rows).astype(np.int32) if len(rows) else np.zeros(0, np.int32)
    return ev_ptr, ev_i, ns.user_listen(ev_ptr, ev_i)


def contract(S, steps, pairs, h, epochs):
    S = [x.copy() for x in S]
    out = []
    for _ in range(epochs):
        _loss, e1, e2 = ns.iteration(S[0], S[1], S[2], S[3], steps, pairs, h['lRate'], h['regU'], h['regI'], h['regB'], h['alpha'], 0,
                                     dot=ns.butterfly, square=ns.product)
        out.append(([x.copy() for x in S], np.array(e1, np.float64), np.array(e2, np.float64)))
    return out


def device(dev, S, steps, pairs, h, epochs, schedule):
    dev.set_option('s2v_schedule', schedule)
    dev.set_factors(S[0], S[1])
    dev.s2v_set_state(S[2], S[3])
    dev.s2v_set_steps(*steps)
    dev.s2v_set_pairs(*pairs)
    out = []
    for _ in range(epochs):
        e1, e2 = dev.s2v_epoch(h['lRate'], h['regU'], h['regI'], h['regB'], h['alpha'], 0.0)
        out.append((list(dev.get_factors() + dev.s2v_get_state()), e1, e2))
    dev.set_option('s2v_schedule', 1)
    return out


def same(got, want, what):
    assert len(got) == len(want)
    for t, ((Sa, a1, a2), (Sb, b1, b2)) in enumerate(zip(got, want)):
        for x, (a, b) in enumerate(zip(Sa, Sb)):
            assert a.dtype == b.dtype and np.array_equal(a, b), (what, t, x)
        assert np.array_equal(a1, b1) and np.array_equal(a2, b2), (what, t)


def check(dev, S, steps, pairs, h=H, epochs=1):
    want = contract(S, steps, pairs, h, epochs)
    for schedule in (1, 0):
        same(device(dev, S, steps, pairs, h, epochs, schedule), want, 'schedule %d' % schedule)
    return want


def pairs_of(W, listen, K):
    ids, sims = cn.friends(W, listen, K)
    t1 = np.repeat(listen, [(ids[a] >= 0).sum() for a in listen]).astype(np.int32)
    keep = ids[listen] >= 0
    return t1, ids[listen][keep].astype(np.int32), sims[listen][keep]


# ---- rating pass ----
@pytest.mark.parametrize('k', [1, 64, 65, 128])
def test_one_item_every_user_listens_to(dev, k):
    m, n = 40, 30
    ev_ptr, ev_i, steps = log_steps([12] * m, n, top=7)
    assert np.bincount(steps[1])[7] == m
    lv = ns.levels(steps[0], steps[1])
    assert lv.max() + 1 >= m                                         # the depth is the number of trained users
    check(dev, init(m, n, k), steps, NONE)
    assert dev.get_option('s2v_levels_steps') == lv.max() + 1 and dev.get_option('s2v_levels_pairs') == 0


def test_nobody_trained_changes_nothing(dev):
    m, n, k = 12, 20, 20
    ev_ptr, ev_i, steps = log_steps([10] * m, n)
    assert len(steps[0]) == 0
    S = init(m, n, k)
    for schedule in (1, 0):
        got = device(dev, S, steps, NONE, H, 1, schedule)
        for a, b in zip(got[0][0], S):
            assert np.array_equal(a, b)
        assert len(got[0][1]) == 0 and len(got[0][2]) == 0


def test_ten_and_eleven_events_and_large_counts(dev):
    m, n, k = 3, 6, 20
    ev_ptr = np.array([0, 10, 21, 21 + 60], np.int64)
    ev_i = np.concatenate([np.arange(10) % 6, np.arange(11) % 6, np.zeros(50, np.int64), np.arange(10) % 5 + 1]).astype(np.int32)
    steps = ns.user_listen(ev_ptr, ev_i)
    assert 0 not in steps[0] and 1 in steps[0] and steps[2].max() == 50      # exactly 10: out; exactly 11: in; counts up to 50
    want = check(dev, init(m, n, k), steps, NONE, epochs=2)
    X0 = init(m, n, k)[0]
    assert np.array_equal(want[-1][0][0][0], X0[0]) and not np.array_equal(want[-1][0][0][1], X0[1])


def test_the_stale_user_bias_is_visible(dev):
    m, n, k = 6, 10, 20
    ev_ptr, ev_i, steps = log_steps([14] * m, n)
    h = dict(H, regB=50.0)
    S = init(m, n, k)
    want = check(dev, S, steps, NONE, h)
    cur = [x.copy() for x in S]
    ns.rating_pass(cur[0], cur[1], cur[2], cur[3], steps[0], steps[1], steps[2], h['lRate'], h['regU'], h['regI'], h['regB'], 0,
                   ns.butterfly, stale=False, square=ns.product)
    assert not np.array_equal(cur[2], want[0][0][2])                 # a contract using the current Bu[u] differs


def test_refusals(dev):
    from yue_amd._shim import YueHipError
    S = init(4, 5, 20)
    dev.set_factors(S[0], S[1])
    with pytest.raises(YueHipError, match='not contiguous'):
        dev.s2v_set_steps([0, 1, 0], [1, 1, 2], [1, 1, 1])
    with pytest.raises(YueHipError, match='paired with itself'):
        dev.s2v_set_pairs([1, 2], [3, 2], [0.5, 0.5])
    with pytest.raises(YueHipError, match='out of range'):
        dev.s2v_set_steps([0, 4], [1, 1], [1, 1])
    with pytest.raises(YueHipError, match='out of range'):
        dev.s2v_set_pairs([1], [5], [0.5])
    with pytest.raises(YueHipError, match='s2v_schedule'):
        dev.set_option('s2v_schedule', 2)


# ---- pair pass ----
@pytest.mark.parametrize('K', [1, 10])
def test_pairs_of_similar_tracks(dev, K):
    m, n, k = 8, 24, 65
    ev_ptr, ev_i, steps = log_steps([15] * m, n)
    listen = np.unique(steps[1])
    W = np.random.RandomState(2).standard_normal((n, k)).astype(np.float32)
    pairs = pairs_of(W, listen, K)
    assert len(pairs[0]) == len(listen) * K
    check(dev, init(m, n, k), steps, pairs, epochs=2)


def test_hub_track_and_mutual_pairs(dev):
    m, n, k = 4, 33, 128
    rng = np.random.RandomState(4)
    others = np.arange(1, n, dtype=np.int32)
    hub = (others, np.zeros(n - 1, np.int32), rng.rand(n - 1))       # track 0 is t2 of every other track
    assert ns.levels(hub[0], hub[1], shared=True).max() + 1 == n - 1  # ... so the pass is one chain
    steps = (np.zeros(0, np.int32),) * 3
    check(dev, init(m, n, k), steps, hub)
    mutual = (np.array([3, 5, 8, 9, 9, 8], np.int32), np.array([5, 3, 9, 8, 8, 9], np.int32), rng.rand(6))   # (a, b) then (b, a)
    check(dev, init(m, n, k), steps, mutual, epochs=2)


# ---- repeated runs ----
def test_second_problem_on_a_used_context_equals_a_fresh_one(dev):
    from yue_amd._shim import Device
    ev_ptr, ev_i, steps = log_steps([13] * 20, 30)
    W = np.random.RandomState(6).standard_normal((30, 20)).astype(np.float32)
    big = (init(20, 30, 20), steps, pairs_of(W, np.unique(steps[1]), 3))
    ev_ptr, ev_i, steps2 = log_steps([12] * 5, 9, seed=3)
    small = (init(5, 9, 65), steps2, pairs_of(W[:9, :20], np.unique(steps2[1]), 2))
    device(dev, big[0], big[1], big[2], H, 2, 1)                     # two epochs back to back (checked against the contract above)
    used = device(dev, small[0], small[1], small[2], H, 2, 1)
    fresh_dev = Device(0, raise_errors=True)
    fresh = device(fresh_dev, small[0], small[1], small[2], H, 2, 1)
    fresh_dev.close()
    same(used, fresh, 'used context')
    same(used, contract(small[0], small[1], small[2], H, 2), 'contract')


# ---- sentences ----
def sentences_of(lengths, m, seed=11):
    rng = np.random.RandomState(seed)
    return [(m * rng.rand(L) ** 2).astype(np.int32) for L in lengths]


def embed_dev(dev, sents, m, dim, window, epochs, seed, round_walks=1):
    ptr = np.concatenate([[0], np.cumsum([len(s) for s in sents])]).astype(np.int64)
    dev.cnet_set_sentences(m, ptr, np.concatenate(sents))
    return dev.cnet_embed(dim, window, epochs, seed, round_walks=round_walks)


@pytest.mark.parametrize('dim,S,lengths', [(20, 64, [11, 64, 65, 129]), (64, 34, [11, 34, 35, 70]), (128, 17, [11, 17, 18, 40])])
def test_sentences_are_cut_into_segments(dev, dim, S, lengths):
    m, window, epochs, seed = 40, 5, 2, 3
    sents = sentences_of(lengths, m) + [np.full(12, 7, np.int32)]    # ... and a sentence of one repeated track
    stats = {}
    w32 = ns.embed_sentences(sents, m, dim, window, epochs, seed, stats=stats)
    assert stats['S'] == S == ns.segment_words(dim)
    if dim == 20:
        assert stats['segments'][:7] == [11, 64, 64, 1, 64, 64, 1]    # 64 | 1 and 64 | 64 | 1
        one = [v for v, L in zip(stats['trained'], stats['segments'] * epochs) if L == 1]
        assert one and not any(one)                                  # a one-word segment updates nothing
    assert stats['segments'][-1] == 12
    w64 = ns.embed_sentences(sents, m, dim, window, epochs, seed, dtype=np.float64)
    gap = np.abs(w32.astype(np.float64) - w64).max()
    got = embed_dev(dev, sents, m, dim, window, epochs, seed)
    err = np.abs(got.astype(np.float64) - w64).max()
    print('dim', dim, 'float32-vs-float64 gap of the contract', gap, 'device vs float64 contract', err)
    assert gap > 0 and err <= 8 * gap
    words = np.unique(np.concatenate(sents))
    idle = np.setdiff1d(np.arange(m), words)
    assert np.all(got[idle] == 0) and np.all(np.abs(got[words]).sum(axis=1) > 0)
    # rounds of 64 segments are bit-reproducible
    a = embed_dev(dev, sents, m, dim, window, epochs, seed, round_walks=0)
    b = embed_dev(dev, sents, m, dim, window, epochs, seed, round_walks=0)
    assert np.array_equal(a, b)


def test_too_short_segments_are_refused(dev):
    from yue_amd._shim import YueHipError
    sents = sentences_of([20, 30], 10)
    ptr = np.concatenate([[0], np.cumsum([len(s) for s in sents])]).astype(np.int64)
    dev.cnet_set_sentences(10, ptr, np.concatenate(sents))
    assert ns.segment_words(128) == 17 < 2 * 9 + 1
    with pytest.raises(YueHipError, match='2 window \\+ 1'):
        dev.cnet_embed(128, 9, 1, 1)
    with pytest.raises(YueHipError, match='out of range'):
        dev.cnet_set_sentences(10, ptr, np.concatenate(sents) + 5)


@pytest.mark.parametrize('dim,L', [(20, 10), (100, 17)])
def test_equal_sentences_equal_walks_bit_for_bit(dev, dim, L):
    m, nw = 50, 150
    walks = (m * np.random.RandomState(8).rand(nw, L) ** 2).astype(np.int32)
    assert L <= ns.segment_words(dim)
    dev.cnet_set_walks(m, walks)
    want = dev.cnet_embed(dim, 5, 2, 4)
    got = embed_dev(dev, list(walks), m, dim, 5, 2, 4, round_walks=0)
    assert np.array_equal(got, want) and np.abs(want).max() > 0
    dev.cnet_set_walks(m, walks)                                      # ... and the walks after sentences are what they were
    assert np.array_equal(dev.cnet_embed(dim, 5, 2, 4), want)


def test_only_tracks_with_a_row_get_similar_tracks(dev):
    m, dim, K = 30, 20, 4
    sents = [np.array([1, 3, 5, 7, 9, 11, 3, 5, 1, 9, 7, 11], np.int32), np.array([5, 7, 13, 15, 5, 13, 15, 7, 1, 3, 9, 11], np.int32)]
    W = embed_dev(dev, sents, m, dim, 5, 3, 2)
    ids, sims = dev.cnet_friends(K)
    listen = np.unique(np.concatenate(sents))
    idle = np.setdiff1d(np.arange(m), listen)
    assert np.all(ids[idle] == -1) and np.all(ids[listen] >= 0) and not np.isin(ids[listen], idle).any()
    want_ids, want_sims = cn.friends(W, listen, K)
    assert np.array_equal(ids, want_ids) and np.allclose(sims, want_sims, rtol=0, atol=1e-12)
