"""CPU: the NumPy contract of CUNE's user-network stage (tests/helpers/numpy_cune_net.py) against the reference's own
outputs (tests/golden/g15_cune_*, tools/make_cune_net_goldens.py): the implicit network's (prefix, item, listener) rule
against CUNet of CUNE.py:39-52, friends and cosines against topKSim of :88-95, friends' items against :104-114."""
from collections import Counter

import numpy as np
import pytest

from helpers import numpy_cune_net as cn
from util import gj, gz


def test_implicit_network_is_the_reference_cunet():
    z = gz('g15_cune_net_c1.npz')
    m, n = int(z['m']), int(z['n'])
    (up, ui), (ip, iu) = cn.pairs_from_events(z['ev_u'], z['ev_i'], m, n)
    net = cn.Net(up, ui, ip, iu)
    ptr, nb, mult = z['ptr'], z['nb'].astype(np.int64), z['mult'].astype(np.int64)
    in_net = 0
    for a in range(m):
        lo, hi = ptr[a], ptr[a + 1]
        assert net.total[a] == mult[lo:hi].sum(), a                   # the reference's list length; 0 for users outside it
        got = Counter(net.entry(a, r) for r in range(int(net.total[a])))
        assert got == dict(zip(nb[lo:hi].tolist(), mult[lo:hi].tolist())), a
        in_net += hi > lo
    assert in_net == len(net.users) > 0


@pytest.fixture(scope='module')
def friends_case():
    z = gz('g15_cune_friends.npz')
    ids, sims = cn.friends(z['W'], z['net'], int(z['K']))
    return z, ids, sims


def test_friends_and_cosines_are_the_reference_topksim(friends_case):
    z, ids, sims = friends_case
    assert np.array_equal(ids, z['ids'])
    assert np.abs(sims - z['sims']).max() <= 1e-12
    assert (ids[z['net']] >= 0).all() and len(z['net']) == int(z['m'])
    gaps = -np.diff(z['sims'], axis=1)                                # the seeded W leaves no near-tie to excuse
    assert gaps.min() > 1e-9


def test_friends_items_are_the_reference_ipositiveset(friends_case):
    z, ids, _ = friends_case
    m, n = int(z['m']), int(z['n'])
    (up, ui), _ = cn.pairs_from_events(z['ev_u'], z['ev_i'], m, n)
    got = cn.friend_items(z['net'], ids, up, ui)
    for u in range(m):
        assert got.get(u, []) == z['ip_items'][z['ip_ptr'][u]:z['ip_ptr'][u + 1]].tolist(), u
    assert z['ip_ptr'][-1] > 0


def test_zero_row_takes_the_reference_zero_division_branch():
    W = np.abs(np.random.RandomState(3).randn(6, 5)).astype(np.float32)
    W[2] = 0
    assert cn.cosine(W[2], W[1]) == 0 and cn.cosine(W[2], W[2]) == 0
    ids, sims = cn.friends(W, np.arange(6), 5)
    assert (ids[[0, 1, 3, 4, 5], -1] == 2).all()                      # positive rows: the zero row ranks last
    assert ids[2].tolist() == [0, 1, 3, 4, 5] and (sims[2] == 0).all()


def test_walk_contract_takes_the_redraw_cutoff_on_a_clique():
    ev_u = np.repeat(np.arange(6), 2)
    ev_i = np.tile([0, 1], 6)
    (up, ui), (ip, iu) = cn.pairs_from_events(ev_u, ev_i, 6, 2)
    stats = {}
    w = cn.walks(cn.Net(up, ui, ip, iu), 20, 10, 1, stats)
    assert w.shape == (120, 10) and stats['cutoffs'] >= 1
    assert (w[:, 1:] != w[:, :-1]).all()                              # a user is never its own neighbour


def test_entry_rule_over_zero_width_prefix_entries():
    """singleton_log: items nobody else listens to at the start, the end and in the middle of a user's row leave flat
    stretches in the prefix; entry(a, r) must index the explicit list over them, for every r."""
    ev_u, ev_i, m, n, marked = cn.singleton_log()
    (up, ui), (ip, iu) = cn.pairs_from_events(ev_u, ev_i, m, n)
    net = cn.Net(up, ui, ip, iu)
    assert np.diff(ip).max() == 300 and len(net.users) == 300
    for a in marked + [2, 150, 298]:
        lst = net.cunet(a)
        width = np.diff(np.concatenate([[0], net.pref[a]]))
        assert len(lst) == net.total[a] >= 299 and (a in (2, 150, 298) or (width == 0).any())
        assert [net.entry(a, r) for r in range(len(lst))] == lst, a
    assert all(net.total[a] == 0 for a in range(300, 305))


def test_embed_contract_statistics():
    """The optional stats of cn.embed count what the walks do and leave the result alone."""
    walks = np.random.RandomState(28).randint(0, 3, (16, 10)).astype(np.int32)
    stats = {'f': []}
    W = cn.embed(walks, 3, 4, 5, 2, 3, round_walks=8, dtype=np.float64, stats=stats)
    assert np.array_equal(W, cn.embed(walks, 3, 4, 5, 2, 3, round_walks=8, dtype=np.float64))
    kept, trained, targets = (np.array(stats[k]) for k in ('kept', 'trained', 'targets'))
    assert len(kept) == len(trained) == len(targets) == 32
    assert (kept == 0).any() and (kept == 1).any() and (trained[kept <= 1] == 0).all() and (trained <= kept).all() and trained.sum() > 0
    assert (targets <= 6 * trained).all() and ((targets > 0) == (trained > 0)).all()
    assert stats['evals'] == len(stats['f']) > 0 and stats['max_abs_f'] == np.abs(stats['f']).max() < 6
    assert stats['cutoffs'] == 0 and stats['cutoff_events'] == []


def test_trained_embedding_golden_meets_its_condition():
    """g15_cune_trained (tools/make_cune_net_goldens.py --trained): logits of at least 4, none cut off, in float32 and float64."""
    z, q = gz('g15_cune_trained.npz'), gj('g15_cune_trained.json')
    assert z['walks'].shape == (q['nw'], q['L']) == (64, 64) and z['walks'].dtype == np.int32
    assert z['W'].shape == (q['m'], q['dim']) == (64, 20) and z['W'].dtype == np.float64
    assert min(q['max_abs_f'].values()) >= 4.0 and max(q['cutoffs'].values()) == 0 and q['epochs'] % 10 == 0 and q['gap'] > 0
    assert abs(np.abs(z['W']).max() - q['max_abs_w']) < 1e-15
    tried = gj('g15_cune_cutoff_search.json')['tried']              # the cut-off fixture: searched, none qualified
    assert len(tried) <= 20 and not any(t['verdict'] == 'qualifies' for t in tried)
