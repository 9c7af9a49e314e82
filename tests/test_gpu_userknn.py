"""GPU: UserKNN (yue_knn_*, DESIGN.md section "UserKNN") against the NumPy oracle (tests/helpers/numpy_userknn.py) and the
reference's own UserKNN (tests/golden/g11_*, through the oracle and through the plugin): neighbour ids, intersections and
unions exactly, predict and top-N lists with bit-equal fp64 scores."""
import glob

import numpy as np
import pytest

from helpers import numpy_userknn as ok
from test_userknn_golden import case_conf, load_case, oracle_lists
from util import gj

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    from yue_amd._shim import Device
    d = Device(0, raise_errors=True)
    yield d
    d.close()


def upload(dev, ev_ptr, ev_i, n):
    (up, ui, uc), (ip, iu) = ok.pairs_from_events(ev_ptr, ev_i, n)
    dev.knn_set_pairs(len(ev_ptr) - 1, n, up, ui, uc, ip, iu)
    return (up, ui, uc), (ip, iu)


def check(dev, ev_ptr, ev_i, n, K, users=None, N=20):
    (up, ui, uc), (ip, iu) = upload(dev, ev_ptr, ev_i, n)
    nbr, inter, uni = dev.knn_neighbors(K)
    users = np.arange(len(ev_ptr) - 1) if users is None else np.asarray(users)
    on, oi, oU = ok.neighbors(up, ui, ip, iu, K, users)
    assert np.array_equal(nbr[users], on) and np.array_equal(inter[users], oi) and np.array_equal(uni[users], oU)
    ids, scores, lens = dev.knn_topn(users.astype(np.int32), N)
    for t, u in enumerate(users):
        it, sc = ok.topn(up, ui, uc, u, on[t], oi[t], oU[t], n, N)
        assert lens[t] == len(it) and np.array_equal(ids[t, :lens[t]], it) and np.array_equal(scores[t, :lens[t]], sc), u
        assert (ids[t, lens[t]:] == -1).all()
    for u in users[:: max(1, len(users) // 20)]:
        it, sc = dev.knn_predict(u)
        oit, osc = ok.predict(up, ui, uc, on[list(users).index(u)], oi[list(users).index(u)], oU[list(users).index(u)], n)
        assert np.array_equal(it, oit) and np.array_equal(sc, osc), u
    return nbr, lens


def events(rng, m, n, lo, hi, pool=None):
    lens = rng.randint(lo, hi + 1, m)
    ev_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    pool = n if pool is None else pool
    ev_i = rng.randint(0, pool, int(ev_ptr[-1])).astype(np.int32)       # repeats: counts > 1
    return ev_ptr, ev_i


@pytest.mark.parametrize('tag', sorted(ok.CASES))
def test_goldens(dev, tmp_path, tag):
    z, rec, conf, (up, ui, uc), (ip, iu) = load_case(tmp_path, tag)
    n = rec.getSize('track')
    dev.knn_set_pairs(rec.getSize('user'), n, up, ui, uc, ip, iu)
    nbr, inter, uni = dev.knn_neighbors(int(z['K']))
    assert np.array_equal(nbr, z['nbr']) and np.array_equal(ok.sims(inter, uni), z['sim'])
    for t, u in enumerate(z['p_users']):
        it, sc = dev.knn_predict(u)
        lo, hi = z['p_ptr'][t], z['p_ptr'][t + 1]
        assert np.array_equal(it, z['p_items'][lo:hi]) and np.array_equal(sc, z['p_scores'][lo:hi]), u
    N = int(gj('g11_%s.json' % tag)['topN'].split(',')[-1])
    lists = oracle_lists(rec, up, ui, uc, nbr, inter, uni, N)
    trained = [u for u in rec.testSet if u in rec.userRecord]
    ids, _, lens = dev.knn_topn(np.array([rec.getId(u, 'user') for u in trained], np.int32), N)
    names = rec.id2name['track']
    for t, u in enumerate(trained):
        assert [names[int(i)] for i in ids[t, :lens[t]]] == lists[u], u
    if tag == 'userknn_h_k20':
        assert dev.get_option('knn_last_chunked_users') == len(trained)          # 20 x 240 entries > 2048: item-range chunks


def test_random_shapes_ties_and_empty_rows(dev):
    rng = np.random.RandomState(1)
    m, n = 700, 60
    ev_ptr, ev_i = events(rng, m, n, 1, 6)                                  # small catalogue: many equal similarities
    lens = np.diff(ev_ptr)
    lens[[3, 10]] = 0                                                       # users without training events
    ev_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ev_i = ev_i[:ev_ptr[-1]]
    ev_i[ev_ptr[20]:ev_ptr[21]] = n - 1                                     # user 20 alone on item n-1: no positive neighbour
    ev_i[ev_i == n - 1] = 0
    ev_i[ev_ptr[20]:ev_ptr[21]] = n - 1
    nbr, lens_out = check(dev, ev_ptr, ev_i, n, 20)
    assert (nbr[[3, 10, 20]] == -1).all()


def test_k_covers_all_users_and_an_item_held_by_everyone(dev):
    rng = np.random.RandomState(2)
    m, n = 90, 400
    ev_ptr, ev_i = events(rng, m, n, 2, 30)
    ev_i[ev_ptr[:-1]] = 7                                                    # every user's first event is item 7
    nbr, _ = check(dev, ev_ptr, ev_i, n, 256, N=100)
    assert ((nbr >= 0).sum(axis=1) == m - 1).all()                          # everyone shares item 7


def test_multi_range_and_chunked_paths(dev):
    rng = np.random.RandomState(3)
    m, n = 1500, 3000
    ev_ptr, ev_i = events(rng, m, n, 5, 120, pool=600)
    try:
        dev.set_option('knn_range', 64)
        dev.set_option('knn_gather', 256)
        check(dev, ev_ptr, ev_i, n, 30, users=np.arange(0, m, 7), N=50)
        assert dev.get_option('knn_last_chunked_users') > 0
    finally:
        dev.set_option('knn_range', 4096)
        dev.set_option('knn_gather', 2048)


def test_c2_sampled_users(dev):
    from yue_amd import synth
    m, n, d = 100000, 50000, 50
    data = synth.make_arrays(m, n, d)
    users = np.sort(np.random.RandomState(4).choice(m, 2000, replace=False))
    (up, ui, uc), (ip, iu) = upload(dev, data['ev_ptr'], data['ev_i'], n)
    nbr, inter, uni = dev.knn_neighbors(20)
    on, oi, oU = ok.neighbors(up, ui, ip, iu, 20, users)
    assert np.array_equal(nbr[users], on) and np.array_equal(inter[users], oi) and np.array_equal(uni[users], oU)
    ids, scores, lens = dev.knn_topn(users[:300].astype(np.int32), 20)
    for t, u in enumerate(users[:300]):
        it, sc = ok.topn(up, ui, uc, u, on[t], oi[t], oU[t], n, 20)
        assert np.array_equal(ids[t, :lens[t]], it) and np.array_equal(scores[t, :lens[t]], sc), u


def test_refusals(dev):
    from yue_amd._shim import Device, YueHipError
    fresh = Device(0, raise_errors=True)
    try:
        rng = np.random.RandomState(5)
        ev_ptr, ev_i = events(rng, 40, 50, 1, 5)
        with pytest.raises(YueHipError, match='yue_knn_set_pairs first'):
            fresh.knn_neighbors(5)
        upload(fresh, ev_ptr, ev_i, 50)
        with pytest.raises(YueHipError, match='yue_knn_neighbors first'):
            fresh.knn_topn(np.arange(3, dtype=np.int32), 5)
        for K in (0, 257):
            with pytest.raises(YueHipError, match='K = %d' % K):
                fresh.knn_neighbors(K)
        fresh.knn_neighbors(5)
        for N in (0, 101):
            with pytest.raises(YueHipError, match='N = %d' % N):
                fresh.knn_topn(np.arange(3, dtype=np.int32), N)
        with pytest.raises(YueHipError, match='out of range'):
            fresh.knn_topn(np.array([40], np.int32), 5)
        with pytest.raises(YueHipError, match='knn_range'):
            fresh.set_option('knn_range', 8192)
        assert fresh.knn_topn(np.arange(3, dtype=np.int32), 5)[2].shape == (3,)       # the context stays usable
    finally:
        fresh.close()


def test_driver_prints_and_writes_the_reference_output(tmp_path, capsys):
    from yue_amd.yue import Yue
    tag = 'userknn_c1_k20'
    meta = gj('g11_%s.json' % tag)
    Yue(case_conf(tmp_path, tag)).execute()
    out = capsys.readouterr().out.splitlines()
    for block in (meta['config_lines'], meta['init_lines'], meta['progress_lines']):
        start = out.index(block[0])
        assert out[start:start + len(block)] == block
    lists = open(glob.glob(str(tmp_path / 'results' / 'UserKNN@*-top-*items*.txt'))[0]).read()
    assert lists == meta['lists']
    measure = open(glob.glob(str(tmp_path / 'results' / 'UserKNN@*measure*.txt'))[0]).read()
    assert measure == ''.join(meta['measure'])


def test_csr_data_set_gives_the_same_lists(tmp_path, capsys):
    from yue_amd.data.arrays import save_csr
    from yue_amd.yue import Yue
    tag = 'userknn_c1_k20'
    z, rec, conf, _, _ = load_case(tmp_path, tag)
    meta = gj('g11_%s.json' % tag)
    m, n = rec.getSize('user'), rec.getSize('track')
    arrays = rec.to_arrays('track')
    test = [sorted(rec.getId(i, 'track') for i in rec.testSet[rec.id2name['user'][u]]) if rec.id2name['user'][u] in rec.testSet else []
            for u in range(m)]
    tp = np.concatenate([[0], np.cumsum([len(t) for t in test])]).astype(np.int64)
    path = str(tmp_path / 'c1.npz')
    save_csr(path, m, n, arrays['ev_ptr'], arrays['ev_i'], tp, np.array(sum(test, []), np.int32))
    (tmp_path / 'csr.conf').write_text(open(str(tmp_path / (tag + '.conf'))).read().replace(
        'record=' + str(tmp_path / (tag + '.txt')), 'record=' + path).replace('-columns user:1,track:2,artist:3,time:0 -delim ,', '-format csr')
        .replace('-target track -byTime 0.2', '-target track').replace('results', 'results_csr'))
    from yue_amd.tool.config import Config
    Yue(Config(str(tmp_path / 'csr.conf'))).execute()
    capsys.readouterr()
    got = np.load(glob.glob(str(tmp_path / 'results_csr' / '*items*.npz'))[0])
    names = rec.id2name['track']
    expect = {}
    for line in meta['lists'].splitlines()[1:]:
        user, body = line.split(':', 1)
        expect[rec.getId(user, 'user')] = [rec.getId(x.lstrip('*$'), 'track') for x in body.split(',')[:-1]]
    assert sorted(expect) == list(got['users'])
    for t, u in enumerate(got['users']):
        assert list(got['ids'][t, :got['lens'][t]]) == expect[int(u)], (u, names)
    measure = open(glob.glob(str(tmp_path / 'results_csr' / '*measure*.txt'))[0]).read().splitlines()
    for a, b in zip(measure, ''.join(meta['measure']).splitlines()):       # same lists; users summed in id order here
        assert a.split(':')[0] == b.split(':')[0]
        if ':' in a:
            assert abs(float(a.split(':')[1]) - float(b.split(':')[1])) <= 1e-12


def test_pair_lists_are_checked_against_their_own_bounds():
    # m = 5 users, n = 3 items: a bound or a row count swapped at a call site of the shared check shows
    from helpers import row_list_cases as rl
    from yue_amd._shim import Device, YueHipError
    d = Device(0, raise_errors=True)
    try:
        ones = np.ones(rl.NNZ, np.int32)

        def upload(u_ptr, u_items, i_ptr, i_users):
            d.knn_set_pairs(rl.M, rl.N, u_ptr, u_items, ones, i_ptr, i_users)
        rl.check_wiring('yue_knn_set_pairs', upload, rl.lists(), [('u_ptr', 'u_items', rl.N, True), ('i_ptr', 'i_users', rl.M, True)])
        with pytest.raises(YueHipError, match='yue_knn_set_pairs: .*not the transpose'):
            upload(**dict(rl.lists(), i_users=rl.not_the_transpose()))
        upload(**rl.lists())
    finally:
        d.close()
