"""GPU: IPF's kernel (yue_amd/csrc/ipf_kernels.hpp) and graph upload (ipf_host.hip) at their chunk, selection-capacity, bit-field
and tie edges, on the cases of tests/helpers/ipf_cases.py (tests/test_rank_edge_cases.py asserts on the CPU that each case reaches
its branch).  Everything is compared bit for bit with the NumPy oracle (tests/helpers/numpy_ipf.py): list lengths, item ids,
fp64 scores and the -1 / 0.0 padding."""
import numpy as np
import pytest

from helpers import ipf_cases as ic

pytestmark = pytest.mark.gpu
DEFAULT_SLOTS = 1024


@pytest.fixture(scope='module')
def dev():
    from yue_amd._shim import Device
    d = Device(0, raise_errors=True)
    yield d
    d.close()


def equal_topn(c, users, N, got):
    ids, scores, lens = got
    assert ids.shape == (len(users), N) and scores.shape == (len(users), N)
    for t, u in enumerate(users):
        it, sc = ic.topn(c, u, N)
        assert lens[t] == len(it) and np.array_equal(ids[t, :lens[t]], it) and np.array_equal(scores[t, :lens[t]], sc), (c['name'], u, N)
        assert (ids[t, lens[t]:] == -1).all() and (scores[t, lens[t]:] == 0.0).all(), (c['name'], u, N)


def equal_predict(dev, c, users):
    for u in users:
        it, sc = dev.ipf_predict(int(u))
        oit, osc = ic.predict(c, u)
        assert np.array_equal(it, oit) and np.array_equal(sc, osc), (c['name'], u)


def check(dev, c, predict_users=None):
    """Set the case's graph; top-N of its users at each of its N, then predict, against the oracle."""
    dev.ipf_set_graph(ic.device_graph(c))
    users = c['users']
    for N in c['Ns']:
        equal_topn(c, users, N, dev.ipf_topn(users.astype(np.int32), N))
    equal_predict(dev, c, users if predict_users is None else predict_users)


@pytest.mark.parametrize('name', ic.FAMILIES['l1'])
def test_level_1_past_one_chunk(dev, name):
    check(dev, ic.build(name))


@pytest.mark.parametrize('name', ic.FAMILIES['l2'])
def test_level_2_nodes_at_the_block_edge(dev, name):
    check(dev, ic.build(name))


@pytest.mark.parametrize('name', ic.FAMILIES['sel'])
def test_selection_capacity(dev, name):
    c = ic.build(name)
    check(dev, c)
    ids, _, lens = dev.ipf_topn(np.array([0], np.int32), 100)
    assert lens[0] == 100 and len(ic.predict(c, 0)[0]) == c['reach']['reached']


@pytest.mark.parametrize('name', ic.FAMILIES['ties'])
def test_order_by_the_insertion_key_alone(dev, name):
    c = ic.build(name)
    check(dev, c)
    if name == 'beta0':                                  # zero scores are ranked, before the padding and by insertion key
        ids, scores, lens = dev.ipf_topn(c['users'].astype(np.int32), 100)
        zero = [(scores[t, :lens[t]] == 0.0).sum() for t in range(len(c['users']))]
        assert sum(z >= 2 for z in zero) == c['reach']['users_with_zero_scores_in_top']


def test_a_list_at_the_end_of_the_k_field(dev):
    from yue_amd._shim import YueHipError
    c = ic.build('limit_k')
    check(dev, c, predict_users=[1, 2])
    with pytest.raises(YueHipError, match=r'yue_ipf_set_graph: user lists row 0 is too long \(limit 262143\)'):
        dev.ipf_set_graph(ic.limit_k_over())
    equal_topn(c, c['users'], 5, dev.ipf_topn(c['users'].astype(np.int32), 5))      # refused before any device work: the graph stands


def test_one_slot_serves_every_kind_of_query_in_turn(dev):
    c = ic.build('combo')
    dev.ipf_set_graph(ic.device_graph(c))
    order = np.array(c['order'], np.int32)              # large, tiny, no events, large, ...
    wide = dev.ipf_topn(order, 100), dev.ipf_topn(order[::-1].copy(), 20)
    try:
        dev.set_option('ipf_slots', 1)
        first = dev.ipf_topn(order, 100)
        predicted = dev.ipf_predict(1)
        second = dev.ipf_topn(order[::-1].copy(), 20)
    finally:
        dev.set_option('ipf_slots', DEFAULT_SLOTS)
    for one, many, users, N in ((first, wide[0], order, 100), (second, wide[1], order[::-1], 20)):
        equal_topn(c, users, N, one)
        assert all(np.array_equal(x, y) for x, y in zip(one, many))
    oit, osc = ic.predict(c, 1)
    assert np.array_equal(predicted[0], oit) and np.array_equal(predicted[1], osc)
    assert first[2][2] == 0 and first[2][5] == 100      # the user without events, and a full list behind it
    equal_predict(dev, c, c['users'])


def test_replacing_the_graph(dev):
    A, B, C, D = (ic.build('replace_%s' % x) for x in 'ABCD')
    dev.ipf_set_graph(ic.device_graph(A))
    everyone = np.arange(A['m'], dtype=np.int32)
    dev.ipf_topn(everyone, 20)                          # every slot has served a query of A
    for c in (A, B, C, D):                              # the same shape (the work arrays stay), a smaller one, a larger one
        check(dev, c, predict_users=c['users'][:5])
        everyone = np.arange(c['m'], dtype=np.int32)
        ids, scores, lens = dev.ipf_topn(everyone, 20)
        at = c['users']
        equal_topn(c, at, 20, (ids[at], scores[at], lens[at]))
