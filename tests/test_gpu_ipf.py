"""GPU: IPF (yue_ipf_*, DESIGN.md section "IPF") against the NumPy oracle (tests/helpers/numpy_ipf.py) and the reference's
own IPF (tests/golden/g12_*, through the oracle and through the plugin): predict and top-N lists with bit-equal fp64
scores, on the fixtures, on a multi-batch shape, and in the full plugin run."""
import glob

import numpy as np
import pytest

from helpers import numpy_ipf as oi
from test_ipf_golden import case_conf, load_case, oracle_lists
from util import gj

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    from yue_amd._shim import Device
    d = Device(0, raise_errors=True)
    yield d
    d.close()


@pytest.mark.parametrize('tag', sorted(oi.CASES))
def test_goldens(dev, tmp_path, tag):
    from yue_amd.recommender.cf.IPF import ipf_graph
    z, meta, rec, g, arrays = load_case(tmp_path, tag)
    n = rec.getSize('track')
    dev.ipf_set_graph(ipf_graph(arrays['ev_ptr'], arrays['ev_i'], n, meta['rho'], meta['beta'], meta['eta'], (z['hu_ptr'], z['hu_users'])))
    for t, u in enumerate(z['p_users']):
        it, sc = dev.ipf_predict(u)
        lo, hi = z['p_ptr'][t], z['p_ptr'][t + 1]
        assert np.array_equal(it, z['p_items'][lo:hi]) and np.array_equal(sc, z['p_scores'][lo:hi]), u
    N = int(meta['topN'].split(',')[-1])
    lists = oracle_lists(rec, g, N)
    trained = [u for u in rec.testSet if u in rec.userRecord]
    uids = np.array([rec.getId(u, 'user') for u in trained], np.int32)
    ids, scores, lens = dev.ipf_topn(uids, N)
    names = rec.id2name['track']
    for t, u in enumerate(trained):
        assert [names[int(i)] for i in ids[t, :lens[t]]] == lists[u], u
        _, osc = oi.topn(g, uids[t], N)
        assert np.array_equal(scores[t, :lens[t]], osc) and (ids[t, lens[t]:] == -1).all(), u


def test_multi_batch_shape(dev):
    from yue_amd import synth
    from yue_amd.recommender.cf.IPF import ipf_graph
    m, n, d = 3000, 2000, 20
    data = synth.make_arrays(m, n, d)
    ev_ptr, ev_i = data['ev_ptr'].copy(), data['ev_i'].copy()
    ev_i[ev_ptr[5]:ev_ptr[6]] = 17                       # one user plays one item 20 times
    dev.ipf_set_graph(ipf_graph(ev_ptr, ev_i, n, 0.5, 0.7, 0.3))
    users = np.arange(m, dtype=np.int32)
    try:
        dev.set_option('ipf_slots', 64)                  # ~47 queries per workgroup: the slots are reused
        ids, scores, lens = dev.ipf_topn(users, 50)
    finally:
        dev.set_option('ipf_slots', 1024)
    ids2, scores2, lens2 = dev.ipf_topn(users, 50)
    assert np.array_equal(ids, ids2) and np.array_equal(scores, scores2) and np.array_equal(lens, lens2)
    assert dev.get_option('ipf_last_ns') > 0
    g = oi.Graph(ev_ptr, ev_i, n, 0.5, 0.7, 0.3)
    for u in list(range(0, m, 23)) + [5]:
        it, sc = oi.topn(g, u, 50)
        assert lens[u] == len(it) and np.array_equal(ids[u, :lens[u]], it) and np.array_equal(scores[u, :lens[u]], sc), u
    for u in (0, 5, 1234):
        it, sc = dev.ipf_predict(u)
        oit, osc = oi.predict(g, u)
        assert np.array_equal(it, oit) and np.array_equal(sc, osc), u


def test_refusals():
    from yue_amd._shim import Device, YueHipError
    from yue_amd.recommender.cf.IPF import ipf_graph
    fresh = Device(0, raise_errors=True)
    try:
        with pytest.raises(YueHipError, match='yue_ipf_set_graph first'):
            fresh.ipf_topn(np.arange(3, dtype=np.int32), 5)
        ev_ptr = np.array([0, 3, 5, 9], np.int64)
        ev_i = np.array([0, 1, 0, 2, 1, 1, 3, 0, 2], np.int32)
        g = ipf_graph(ev_ptr, ev_i, 4, 1.0, 0.7, 0.3)
        bad = dict(g, u_items=np.array([0, 0, 1, 2, 1, 1, 3, 0][:len(g['u_items'])], np.int32))
        with pytest.raises(YueHipError, match='distinct'):
            fresh.ipf_set_graph(bad)
        fresh.ipf_set_graph(g)
        for N in (0, 101):
            with pytest.raises(YueHipError, match='N = %d' % N):
                fresh.ipf_topn(np.arange(3, dtype=np.int32), N)
        with pytest.raises(YueHipError, match='out of range'):
            fresh.ipf_topn(np.array([3], np.int32), 5)
        with pytest.raises(YueHipError, match='ipf_slots'):
            fresh.set_option('ipf_slots', 0)
        ids, _, lens = fresh.ipf_topn(np.arange(3, dtype=np.int32), 5)          # the context stays usable
        o = oi.Graph(ev_ptr, ev_i, 4, 1.0, 0.7, 0.3)
        for u in range(3):
            assert list(ids[u, :lens[u]]) == list(oi.topn(o, u, 5)[0])
    finally:
        fresh.close()


def test_driver_prints_and_writes_the_reference_output(tmp_path, capsys):
    from yue_amd.yue import Yue
    tag = 'ipf_s'
    meta = gj('g12_%s.json' % tag)
    conf, _ = case_conf(tmp_path, tag)
    Yue(conf).execute()
    out = capsys.readouterr().out.splitlines()
    for block in (meta['init_lines'], meta['progress_lines']):
        start = out.index(block[0])
        assert out[start:start + len(block)] == block
    lists = open(glob.glob(str(tmp_path / 'results' / 'IPF@*-top-*items*.txt'))[0]).read()
    assert lists == meta['lists']
    measure = open(glob.glob(str(tmp_path / 'results' / 'IPF@*measure*.txt'))[0]).read()
    assert measure == ''.join(meta['measure'])


def test_csr_data_set_gives_the_same_lists(tmp_path, capsys):
    from yue_amd.data.arrays import save_csr
    from yue_amd.tool.config import Config
    from yue_amd.yue import Yue
    tag = 'ipf_b1'                                      # -byTime: item2user order is user-id order, as in csr data
    z, meta, rec, g, arrays = load_case(tmp_path, tag)
    m, n = rec.getSize('user'), rec.getSize('track')
    names = rec.id2name['user']
    test = [sorted(rec.getId(i, 'track') for i in rec.testSet[names[u]]) if names[u] in rec.testSet else [] for u in range(m)]
    tp = np.concatenate([[0], np.cumsum([len(t) for t in test])]).astype(np.int64)
    path = str(tmp_path / 'b1.npz')
    save_csr(path, m, n, arrays['ev_ptr'], arrays['ev_i'], tp, np.array(sum(test, []), np.int32))
    text = open(str(tmp_path / (tag + '.conf'))).read()
    text = text.replace('record=' + str(tmp_path / (tag + '.txt')), 'record=' + path).replace(
        '-columns user:1,track:2,time:0 -delim ,', '-format csr').replace('-target track -byTime 0.2', '-target track').replace('results', 'results_csr')
    (tmp_path / 'csr.conf').write_text(text)
    Yue(Config(str(tmp_path / 'csr.conf'))).execute()
    capsys.readouterr()
    got = np.load(glob.glob(str(tmp_path / 'results_csr' / '*items*.npz'))[0])
    expect = {}
    for line in meta['lists'].splitlines()[1:]:
        user, body = line.split(':', 1)
        expect[rec.getId(user, 'user')] = [rec.getId(x.lstrip('*$'), 'track') for x in body.split(',')[:-1]]
    assert sorted(expect) == list(got['users'])
    for t, u in enumerate(got['users']):
        assert list(got['ids'][t, :got['lens'][t]]) == expect[int(u)], u


def test_the_four_lists_are_checked_against_their_own_bounds():
    # m = 5 users, n = 3 items: a bound or a row count swapped at a call site of the shared check shows
    from helpers import row_list_cases as rl
    from yue_amd._shim import Device, YueHipError
    from yue_amd.recommender.cf.IPF import ipf_graph
    d = Device(0, raise_errors=True)
    try:
        g = ipf_graph(rl.U_PTR, rl.U_ITEMS, rl.N, 1.0, 0.7, 0.3)
        rl.check_wiring('yue_ipf_set_graph', lambda **lists: d.ipf_set_graph(lists), g,
                        [('u_ptr', 'u_items', rl.N, False), ('s_ptr', 's_items', rl.N, False), ('hu_ptr', 'hu_users', rl.M, False), ('hs_ptr', 'hs_users', rl.M, False)])
        for key, words in (('u_items', 'user lists'), ('s_items', 'session lists'), ('hu_users', 'item2user lists'), ('hs_users', 'item2session lists')):
            twice = g[key].copy(); twice[-1] = twice[-2]                 # the last row of each holds two ids
            with pytest.raises(YueHipError, match='yue_ipf_set_graph: %s rows must hold distinct ids' % words):
                d.ipf_set_graph(dict(g, **{key: twice}))
            unsorted = g[key].copy(); unsorted[0], unsorted[1] = unsorted[1], unsorted[0]
            d.ipf_set_graph(dict(g, **{key: unsorted}))                  # any order is in order here
    finally:
        d.close()
