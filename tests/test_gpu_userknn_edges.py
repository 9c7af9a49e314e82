"""GPU: UserKNN's kernels (yue_amd/csrc/knn_kernels.hpp) at their chunk, sort-capacity, pass and tie edges, on the cases of
tests/helpers/knn_cases.py (tests/test_rank_edge_cases.py asserts on the CPU that each case reaches its branch).  Everything is
compared bit for bit with the NumPy oracle (tests/helpers/numpy_userknn.py) through check() of tests/test_gpu_userknn.py:
neighbour ids, intersections, unions, list lengths, item ids and fp64 scores; the padding (-1 / 0.0) is checked here."""
import numpy as np
import pytest

from helpers import knn_cases as kc
from helpers import numpy_userknn as ok
from test_gpu_userknn import check

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    from yue_amd._shim import Device
    d = Device(0, raise_errors=True)
    yield d
    d.close()


def run(dev, c, K, N, options):
    """check() of the case's users at the given options, then the padding of the top-N arrays; returns (nbr, ids, scores, lens)."""
    users = c['users']
    try:
        for key, value in options.items():
            dev.set_option(key, value)
        nbr, lens = check(dev, c['ev_ptr'], c['ev_i'], c['n'], K, users=users, N=N)
        ids, scores, lens2 = dev.knn_topn(users.astype(np.int32), N)
        chunked = dev.get_option('knn_last_chunked_users')
    finally:
        for key, value in kc.DEFAULTS.items():
            dev.set_option(key, value)
    assert np.array_equal(lens, lens2)
    for t in range(len(users)):
        assert (ids[t, lens[t]:] == -1).all() and (scores[t, lens[t]:] == 0.0).all() and (ids[t, :lens[t]] >= 0).all()
    on, oi, oU = kc.oracle_neighbors(c, K)
    pad = on < 0
    assert np.array_equal(nbr[users] < 0, pad)
    return nbr, ids, scores, lens, chunked


@pytest.mark.parametrize('K', [1, 20, 256])
@pytest.mark.parametrize('name', kc.FAMILIES['cap'])
def test_sort_capacity(dev, name, K):
    c = kc.build(name)
    nbr, _, _, _, _ = run(dev, c, K, c['Ns'][0], c['options'][0])
    assert (nbr[c['users']] >= 0).all()                                      # m - 1 candidates >= K: every slot is filled


@pytest.mark.parametrize('knn_range', [kc.RANGE, kc.RANGE_MIN])
@pytest.mark.parametrize('name', kc.FAMILIES['row'])
def test_own_items_past_one_chunk(dev, name, knn_range):
    c = kc.build(name)
    nbr, _, _, _, _ = run(dev, c, 20, 20, dict(kc.DEFAULTS, knn_range=knn_range))
    assert (nbr[c['users']] == c['long_user']).any()


@pytest.mark.parametrize('name', kc.FAMILIES['range'])
def test_last_pass_full_single_or_absent(dev, name):
    c = kc.build(name)
    run(dev, c, 10, 10, c['options'][0])


@pytest.mark.parametrize('N', [100, 1])
@pytest.mark.parametrize('knn_gather', [kc.GATHER, kc.GATHER_MIN])
@pytest.mark.parametrize('name', kc.FAMILIES['kp'])
def test_every_rank_positive(dev, name, knn_gather, N):
    c = kc.build(name)
    K = c['Ks'][0]
    nbr, _, _, _, chunked = run(dev, c, K, N, dict(kc.DEFAULTS, knn_gather=knn_gather))
    assert ((nbr[c['users']] >= 0).sum(axis=1) == K).all()
    if knn_gather == kc.GATHER_MIN:
        assert chunked == len(c['users'])                                    # K lists of 2 or more entries: one item per chunk


@pytest.mark.parametrize('name', kc.FAMILIES['gather'])
def test_chunked_decision(dev, name):
    c = kc.build(name)
    for N in c['Ns']:
        _, _, _, lens, chunked = run(dev, c, 4, N, c['options'][0])          # the one user ranked alone
        assert chunked == c['reach']['chunked'] and lens[0] >= min(N, 63)


@pytest.mark.parametrize('N', [1, 7, 100])
@pytest.mark.parametrize('name', kc.FAMILIES['ones'])
def test_equal_scores_cut_across_chunks(dev, name, N):
    c = kc.build(name)
    _, ids, scores, lens, chunked = run(dev, c, 20, N, c['options'][0])
    assert chunked == c['reach']['chunked']
    if name == 'ones':
        for t in range(len(c['users'])):
            assert (scores[t, :lens[t]] == 1.0).all() and (np.diff(ids[t, :lens[t]]) > 0).all()


def test_neighbours_holding_only_own_items(dev):
    c = kc.build('own_only')
    _, ids, scores, lens, _ = run(dev, c, 10, 10, c['options'][0])
    u = c['own_user']
    assert lens[u] == 0 and (ids[u] == -1).all() and (scores[u] == 0.0).all()
    (up, ui, uc), _ = c['pairs']
    items, _ = dev.knn_predict(u)
    assert np.array_equal(np.sort(items), ui[up[u]:up[u + 1]])               # predict still scores them: the user's own three items


@pytest.mark.parametrize('name', kc.FAMILIES['predict'])
def test_predict_block_edge(dev, name):
    c = kc.build(name)
    run(dev, c, 20, 20, c['options'][0])
    (up, ui, uc), _ = c['pairs']
    nbr, inter, uni = kc.oracle_neighbors(c, 20)
    for u in range(6):                                                       # the users that hold the last item
        items, scores = dev.knn_predict(u)
        oit, osc = ok.predict(up, ui, uc, nbr[u], inter[u], uni[u], c['n'])
        assert np.array_equal(items, oit) and np.array_equal(scores, osc)
        assert u > 0 or (c['n'] - 1) in items
