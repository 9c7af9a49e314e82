"""CPU: the NumPy contract of Song2vec (tests/helpers/numpy_song2vec.py) against what the reference's own Song2vec class computed
(tests/golden/g16_song2vec_*, tools/make_song2vec_goldens.py) from a seeded table in place of gensim's.

With the reference's visiting order and the table as inputs, the contract with dot=np.dot makes the reference's NumPy calls on
the reference's types, so X, Y, Bu, Bi and the printed losses are equal bit for bit.  The level-driven form equals the
sequential form bit for bit, whatever the order inside a level: that is what lets the device run a level at once.  The
device's form of the contract (dot=butterfly, square=product) is not the reference's arithmetic; its distance is the
'measured' figure of each json, reproduced here, and the GPU tests allow the device four times that.
"""
import functools
import os

import numpy as np
import pytest

from helpers import numpy_song2vec as ns
from util import gj, gz

CASES = ['c1_k20', 's_k65', 's_k128']
MARGIN = 4.0
KEYS = ('X', 'Y', 'Bu', 'Bi')


@functools.lru_cache(maxsize=None)
def load(tag):
    z, st, meta = gz('g16_song2vec_%s.npz' % tag), gz('g16_song2vec_%s_states.npz' % tag), gj('g16_song2vec_%s.json' % tag)
    m = int(z['m'])
    ev_u, ev_i = z['ev_u'].astype(np.int32), z['ev_i'].astype(np.int32)
    ev_ptr = np.concatenate([[0], np.cumsum(np.bincount(ev_u, minlength=m))]).astype(np.int64)
    steps = ns.user_listen(ev_ptr, ev_i)
    pairs = (z['t1'].astype(np.int32), z['t2'].astype(np.int32), z['sim'])
    hyper = dict(lRate=float(z['lRate']), regU=float(z['regU']), regI=float(z['regI']), regB=float(z['regB']), alpha=float(z['alpha']))
    return z, st, meta, ev_ptr, ev_i, steps, pairs, hyper


def start(z):
    return [x.copy() for x in ns.init_from_seed(int(z['seed']), int(z['m']), int(z['n']), int(z['k']))]


@functools.lru_cache(maxsize=None)
def run(tag, form):
    """States, losses and squared errors after every iteration; form: 'npdot', 'device' (butterfly, product), 'levels',
    'shuffled' (np.dot, level-driven)."""
    z, st, meta, ev_ptr, ev_i, steps, pairs, h = load(tag)
    S = start(z)
    kw = {'npdot': {}, 'device': {'dot': ns.butterfly, 'square': ns.product}, 'levels': {'by_levels': True},
          'shuffled': {'by_levels': True, 'rng': np.random.RandomState(7)}}[form]
    out = []
    for _t in range(int(z['iters'])):
        loss, e1, e2 = ns.iteration(S[0], S[1], S[2], S[3], steps, pairs, h['lRate'], h['regU'], h['regI'], h['regB'], h['alpha'], 0, **kw)
        out.append(([x.copy() for x in S], loss, np.array(e1, np.float64), np.array(e2, np.float64)))
    return out


def bound(meta, key, floor=0.0):
    return max(MARGIN * meta['measured']['butterfly_vs_npdot_' + key], floor)


def printed_losses(meta):
    out = []
    for i, ln in enumerate(meta['lines'], 1):
        head, val = ln.split(' loss: ')
        assert head == 'iteration: %d' % i
        out.append(float(val))
    return out


@pytest.mark.parametrize('tag', CASES)
def test_contract_equals_the_reference_bit_for_bit(tag):
    z, st, meta = load(tag)[:3]
    got = run(tag, 'npdot')
    assert len(got) == len(meta['lines']) == int(z['iters'])
    for t, (S, loss, e1, e2) in enumerate(got):
        for a, key in zip(S, KEYS):
            ref = st[key + 's'][t]
            assert a.dtype == ref.dtype and np.array_equal(a, ref), (key, t)
        assert 'iteration: %d loss: %s' % (t + 1, loss) == meta['lines'][t]
    assert got[0][0][0].dtype == np.float32 and got[0][0][2].dtype == np.float64


@pytest.mark.parametrize('tag', CASES)
@pytest.mark.parametrize('form', ['levels', 'shuffled'])
def test_level_driven_form_equals_the_sequential_form(tag, form):
    for (S, loss, e1, e2), (S2, loss2, f1, f2) in zip(run(tag, 'npdot'), run(tag, form)):
        for a, b in zip(S, S2):
            assert np.array_equal(a, b)
        assert loss == loss2 and np.array_equal(e1, f1) and np.array_equal(e2, f2)


@pytest.mark.parametrize('tag', CASES)
def test_levels_keep_the_rows_of_a_level_apart(tag):
    z, st, meta, ev_ptr, ev_i, steps, pairs, h = load(tag)
    lv = ns.levels(steps[0], steps[1])
    assert lv.max() + 1 == meta['levels_steps']
    for l in range(lv.max() + 1):
        at = lv == l
        assert len(set(steps[0][at])) == at.sum() and len(set(steps[1][at])) == at.sum()
    # a level is the earliest the step can run: the previous step of its user or of its item sits one level below
    depth = np.bincount(steps[1]).max()
    assert lv.max() + 1 >= depth
    lp = ns.levels(pairs[0], pairs[1], shared=True)
    assert lp.max() + 1 == meta['levels_pairs']
    for l in range(lp.max() + 1):
        at = lp == l
        tracks = np.concatenate([pairs[0][at], pairs[1][at]])
        assert len(set(tracks)) == 2 * at.sum()


@pytest.mark.parametrize('tag', CASES)
def test_measured_figures_are_reproduced(tag):
    z, st, meta = load(tag)[:3]
    now = {key: 0.0 for key in KEYS + ('loss',)}
    for (S, loss, e1, e2), (D, dloss, d1, d2) in zip(run(tag, 'npdot'), run(tag, 'device')):
        for key, a, b in zip(KEYS, S, D):
            now[key] = max(now[key], ns.rel(b, a))
        now['loss'] = max(now['loss'], abs(float(dloss) - float(loss)) / abs(float(loss)))
    for key, v in now.items():
        assert v == meta['measured']['butterfly_vs_npdot_' + key], key


def test_small_cases_reach_their_branches():
    z, st, meta, ev_ptr, ev_i, steps, pairs, h = load('s_k65')
    users, sents = ns.sentences(ev_ptr, ev_i)
    m = int(z['m'])
    assert 4 * (m - len(users)) >= m and meta['trained_users'] == len(users)          # a quarter of the users has <= 10 events
    assert steps[2].max() > 1                                                          # repeated events
    assert set(steps[0]) == set(users) and sum(len(s) for s in sents) == steps[2].sum()
    assert np.array_equal(np.unique(np.concatenate(sents)), z['listen'])
    # untrained users keep their start rows
    X0 = start(z)[0]
    idle = np.setdiff1d(np.arange(m), users)
    assert np.array_equal(st['Xs'][-1][idle], X0[idle])
    # adjacent cosines of every list are 1e-9 apart (the rule of g15_cune_friends)
    K = int(z['K'])
    sim = z['sim'].reshape(-1, K)
    assert np.all(sim[:, :-1] - sim[:, 1:] > 1e-9) if K > 1 else True


def test_butterfly_is_a_float32_sum_of_all_elements():
    rng = np.random.RandomState(3)
    for k in (1, 20, 64, 65, 128):
        a, b = rng.standard_normal(k).astype(np.float32), rng.standard_normal(k).astype(np.float32)
        got = ns.butterfly(a, b)
        assert got.dtype == np.float32
        assert abs(float(got) - float(np.dot(a.astype(np.float64), b.astype(np.float64)))) <= 1e-5 * k
    one = np.zeros(128, np.float32)
    one[127] = 3.0
    assert ns.butterfly(one, one) == 9.0


def test_menu_and_config_name_the_plugin():
    from yue_amd.main import MENU
    from yue_amd.recommender.advanced.Song2vec import Song2vec
    from yue_amd.tool.config import Config, LineConfig
    assert MENU['a2'] == 'Song2vec' and callable(Song2vec.buildModel)
    conf = Config(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'config', 'Song2vec.conf'))
    assert conf['recommender'] == 'Song2vec'
    opt = LineConfig(conf['Song2vec'])
    assert float(opt['-alpha']) == 0.5 and int(opt['-k']) == 10 and opt['-emb'] == 'hip'
