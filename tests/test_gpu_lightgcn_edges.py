"""GPU: LightGCN's kernels where they can go wrong, with the bounds of test_gpu_lightgcn.py: row
degrees 0, 1, 63, 64, 65 and around the hub threshold (set low through the option lgcn_hub), a hub whose parts do not divide
evenly, batch sizes around a wave, repeated and conflicting triplets, every refusal, the symmetry check, buffer reuse after a
second graph of another shape, and bit-identical repeats on the hub path.  The cases assert on the contract side that they
reach their branches (tests/test_lightgcn_golden.py does so on the CPU for all of them)."""
import numpy as np
import pytest

from helpers import lightgcn_cases as lc
from helpers import numpy_lightgcn as nl
from test_gpu_lightgcn import check_case, upload

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    from yue_amd._shim import Device
    d = Device(0, raise_errors=True)
    yield d
    d.close()


@pytest.mark.parametrize('name', ['deg_k20', 'deg_k64', 'deg_k128'])
def test_degrees_around_a_wave_and_the_hub_threshold(dev, name):
    c = lc.build(name)
    deg = c['g']['degree']
    assert list(deg[:len(lc.EDGE_DEGREES)]) == lc.EDGE_DEGREES and c['hub'] == lc.HUB
    check_case(dev, c)
    # threshold - 1 and the threshold itself stay whole rows; + 1 is cut in two, 2 * 96 + 37 in three uneven parts
    assert dev.get_option('lgcn_last_hubs') == 2 and dev.get_option('lgcn_last_parts') == 2 + 3
    # the same graph with every row whole gives the same result within the bounds, and other bits on the hub rows' sums
    hub_run = dev.lgcn_grad(c['layers'], c['u'], c['i'], c['j'], lc.REG)
    dev.set_option('lgcn_hub', 1024)
    whole = dev.lgcn_grad(c['layers'], c['u'], c['i'], c['j'], lc.REG)
    assert dev.get_option('lgcn_last_hubs') == 0
    assert nl.rel(whole[1], c['gU']) <= 4 * c['d32']['gU'] and nl.rel(whole[2], c['gV']) <= 4 * c['d32']['gV']
    again = dev.lgcn_grad(c['layers'], c['u'], c['i'], c['j'], lc.REG)
    assert whole[0] == again[0] and np.array_equal(whole[1], again[1]) and np.array_equal(whole[2], again[2])
    dev.set_option('lgcn_hub', lc.HUB)
    back = dev.lgcn_grad(c['layers'], c['u'], c['i'], c['j'], lc.REG)
    assert back[0] == hub_run[0] and np.array_equal(back[1], hub_run[1]) and np.array_equal(back[2], hub_run[2])


@pytest.mark.parametrize('name', ['T1', 'T63', 'T64', 'T65', 'repeat', 'posneg'])
def test_batches(dev, name):
    c = lc.build(name)
    if name == 'repeat':
        assert len(c['u']) == 64 and len(set(zip(c['u'], c['i'], c['j']))) == 1
    if name == 'posneg':
        assert c['i'][0] == c['j'][1]
    check_case(dev, c)


def test_refusals(dev):
    from yue_amd._shim import YueHipError
    c = lc.build('k20')
    upload(dev, c)
    L, u, i, j = 3, c['u'], c['i'], c['j']
    for layers in (0, -1, 65):                                   # the layers are kept for the backward pass: 64 at the most
        with pytest.raises(YueHipError, match='yue_lgcn_propagate: needs 1 <= layers <= 64'):
            dev.lgcn_propagate(layers)
        with pytest.raises(YueHipError, match='yue_lgcn_grad: needs 1 <= layers <= 64'):
            dev.lgcn_grad(layers, u, i, j, lc.REG)
        with pytest.raises(YueHipError, match='yue_lgcn_step: needs 1 <= layers <= 64'):
            dev.lgcn_step(layers, u, i, j, 0.002, lc.REG, 1)
    none = np.zeros(0, np.int32)
    with pytest.raises(YueHipError, match='yue_lgcn_grad: needs 1 <= T < 2\\^29'):
        dev.lgcn_grad(L, none, none, none, lc.REG)
    with pytest.raises(YueHipError, match='yue_lgcn_step: needs 1 <= T < 2\\^29'):
        dev.lgcn_step(L, none, none, none, 0.002, lc.REG, 1)
    for which, bad in ((0, c['m']), (0, -1), (1, c['n']), (1, -1), (2, c['n']), (2, -1)):
        t = [u.copy(), i.copy(), j.copy()]
        t[which][5] = bad
        with pytest.raises(YueHipError, match='out of range'):
            dev.lgcn_grad(L, t[0], t[1], t[2], lc.REG)
        with pytest.raises(YueHipError, match='out of range'):
            dev.lgcn_step(L, t[0], t[1], t[2], 0.002, lc.REG, 1)
    with pytest.raises(YueHipError, match='yue_lgcn_step: needs step >= 1'):
        dev.lgcn_step(L, u, i, j, 0.002, lc.REG, 0)
    # nothing above moved the factors
    P, Q = dev.get_factors()
    assert np.array_equal(P, c['U']) and np.array_equal(Q, c['V'])
    # a k beyond what the kernels take
    rs = np.random.RandomState(1)
    dev.set_factors(rs.rand(c['m'], 129).astype(np.float32), rs.rand(c['n'], 129).astype(np.float32))
    with pytest.raises(YueHipError, match='k <= 128'):
        dev.lgcn_propagate(L)
    with pytest.raises(YueHipError, match='k <= 128'):
        dev.lgcn_grad(L, u, i, j, lc.REG)
    # a graph set for other shapes
    dev.set_factors(rs.rand(c['m'] + 1, 20).astype(np.float32), rs.rand(c['n'], 20).astype(np.float32))
    with pytest.raises(YueHipError, match='graph was set for'):
        dev.lgcn_propagate(L)
    with pytest.raises(YueHipError, match='graph was set for'):
        dev.lgcn_step(L, u, i, j, 0.002, lc.REG, 1)


def test_no_graph_is_refused():
    from yue_amd._shim import Device, YueHipError
    d = Device(0, raise_errors=True)
    try:
        c = lc.build('k20')
        d.set_factors(c['U'], c['V'])
        with pytest.raises(YueHipError, match='yue_lgcn_set_graph first'):
            d.lgcn_propagate(3)
        with pytest.raises(YueHipError, match='yue_lgcn_set_graph first'):
            d.lgcn_grad(3, c['u'], c['i'], c['j'], lc.REG)
    finally:
        d.close()


def test_graph_checks_come_before_anything_is_stored(dev):
    from yue_amd._shim import YueHipError
    c = lc.build('k20')
    upload(dev, c)
    g = c['g']
    F0 = dev.lgcn_propagate(3)
    keys = ('u_ptr', 'u_items', 'u_w', 'i_ptr', 'i_users', 'i_w')

    def refused(match, **change):
        lists = [change.get(key, g[key]) for key in keys]
        with pytest.raises(YueHipError, match=match):
            dev.lgcn_set_graph(c['m'], c['n'], *lists)

    w = g['i_w'].copy(); w[3] += 1
    refused('not symmetric', i_w=w)                              # another weight on the item side
    users = g['i_users'].copy()
    last = g['i_ptr'][1:] - 1                                    # an item's last user becomes the next one: the list stays sorted
    row = int(np.flatnonzero((np.diff(g['i_ptr']) >= 1) & (users[np.maximum(last, 0)] < c['m'] - 1))[0])
    users[last[row]] += 1
    refused('not symmetric', i_users=users)                      # another user in an item's list
    ptr = g['i_ptr'].copy(); ptr[-1] -= 1
    refused('not symmetric', i_ptr=ptr)                          # one pair fewer on the item side
    items = g['u_items'].copy(); items[0] = c['n']
    refused('out of range', u_items=items)
    items = g['u_items'].copy(); items[0] = -1
    refused('out of range', u_items=items)
    row = int(np.flatnonzero(np.diff(g['u_ptr']) >= 2)[0])
    items = g['u_items'].copy(); a = g['u_ptr'][row]; items[a], items[a + 1] = items[a + 1], items[a]
    refused('sorted and unique', u_items=items)
    items = g['u_items'].copy(); items[a + 1] = items[a]
    refused('sorted and unique', u_items=items)
    # the graph of before is still in place
    assert np.array_equal(dev.lgcn_propagate(3), F0)


def test_buffers_are_reused_after_a_graph_of_another_shape(dev):
    big, small = lc.build('deg_k64'), lc.build('k20')
    check_case(dev, big)
    check_case(dev, small)                                       # fewer rows, smaller k, no hubs: every buffer is larger than needed
    assert dev.get_option('lgcn_last_hubs') == 0
    check_case(dev, big)


def test_graph_lists_are_checked_against_their_own_bounds():
    # m = 5 users, n = 3 items: a bound or a row count swapped at a call site of the shared check shows
    from helpers import row_list_cases as rl
    from yue_amd._shim import Device, YueHipError
    d = Device(0, raise_errors=True)
    try:
        w = np.full(rl.NNZ, 0.5, np.float32)

        def upload(u_ptr, u_items, i_ptr, i_users, i_w=w):
            d.lgcn_set_graph(rl.M, rl.N, u_ptr, u_items, w, i_ptr, i_users, i_w)
        rl.check_wiring('yue_lgcn_set_graph', upload, rl.lists(), [('u_ptr', 'u_items', rl.N, True), ('i_ptr', 'i_users', rl.M, True)])
        nan = w.copy(); nan[rl.NNZ - 1] = np.nan
        with pytest.raises(YueHipError, match='yue_lgcn_set_graph: item-side row 2: weight not finite'):
            upload(**dict(rl.lists(), i_w=nan))
        upload(**rl.lists())
    finally:
        d.close()
