"""GPU: ExpoMF (yue_expo_*) against the device contract (tests/helpers/numpy_expomf.py, from identical
inputs: within max(4 * e_ref, 1e-6), e_ref read from the fixture's json), against the reference's own ExpoMF
(tests/golden/g13_*: within 4 * e_ref of the last iteration), and through the plugin surface.  Every row is compared."""
import glob
import random

import numpy as np
import pytest

from helpers import numpy_expomf as ne
from helpers.numpy_wrmf import pairs_from_events
from test_expomf_golden import CASES, load
from test_host_golden import _conf_text, _load
from util import gj, gz

pytestmark = pytest.mark.gpu

LAM = ne.LAM_THETA / ne.LAM_Y


@pytest.fixture(scope='module')
def dev():
    from yue_amd._shim import Device
    d = Device(0, raise_errors=True)
    yield d
    d.close()


def bound(e):
    return max(4 * e, 1e-6)


def upload(dev, theta, beta, mu, um, im):
    dev.set_factors(theta, beta)
    dev.expo_set_pairs(*(um + im))
    dev.expo_set_mu(mu)


@pytest.mark.parametrize('tag', CASES)
def test_half_sweeps_and_mu_equal_the_contract(dev, tag):
    z, meta, um, im = load(tag)
    e = meta['e_ref']
    theta0, beta0, mu0 = z['theta0'], z['beta0'], z['mu0']
    m, n = theta0.shape[0], beta0.shape[0]
    upload(dev, theta0, beta0, mu0, um, im)
    dev.expo_half_sweep(0, LAM, ne.LAM_Y, True)
    theta, beta = dev.get_factors()
    assert np.array_equal(beta, beta0)
    want = ne.expo_half_sweep_contract(beta0, theta0, um[0], um[1], um[2], mu0, True, LAM, ne.LAM_Y)
    print(tag, 'theta', ne.rel(theta, want), bound(e['theta']))
    assert ne.rel(theta, want) <= bound(e['theta'])
    assert np.all(theta[z['zero_users']] == 0)
    dev.expo_half_sweep(1, LAM, ne.LAM_Y, m == n)
    theta2, beta = dev.get_factors()
    assert np.array_equal(theta2, theta)
    want = ne.expo_half_sweep_contract(theta, beta0, im[0], im[1], im[2], mu0, m == n, LAM, ne.LAM_Y)
    print(tag, 'beta', ne.rel(beta, want), bound(e['beta']))
    assert ne.rel(beta, want) <= bound(e['beta'])
    assert np.all(beta[z['zero_items']] == 0)
    dev.expo_update_mu(ne.PRIOR_A, ne.PRIOR_B, ne.LAM_Y)
    mu = dev.expo_get_mu()
    want = ne.expo_mu_contract(theta, beta, um[0], um[1], mu0, ne.PRIOR_A, ne.PRIOR_B, ne.LAM_Y)
    print(tag, 'mu', ne.rel(mu, want), bound(e['mu']))
    assert mu.dtype == np.float32 and ne.rel(mu, want) <= bound(e['mu'])


@pytest.mark.parametrize('tag', CASES)
def test_two_iterations_against_the_reference(dev, tag):
    z, meta, um, im = load(tag)
    e = meta['e_ref_last_iteration']
    m, n = int(z['m']), int(z['n'])
    upload(dev, z['theta0'], z['beta0'], z['mu0'], um, im)
    for _ in range(int(z['iters'])):
        dev.expo_half_sweep(0, LAM, ne.LAM_Y, True)
        dev.expo_half_sweep(1, LAM, ne.LAM_Y, m == n)
        dev.expo_update_mu(ne.PRIOR_A, ne.PRIOR_B, ne.LAM_Y)
    theta, beta = dev.get_factors()
    mu = dev.expo_get_mu()
    got = {'theta': ne.rel(theta, z['thetas'][-1]), 'beta': ne.rel(beta, z['betas'][-1]), 'mu': ne.rel(mu, z['mus'][-1])}
    print(tag, got, e)
    for key in got:
        assert got[key] <= 4 * e[key], key


def test_c2_sample_rows(dev):
    z, meta = gz('g13_expomf_c2rows.npz'), gj('g13_expomf_c2rows.json')
    inp = ne.c2_inputs(int(z['seed']))
    um, im = inp['user_major'], inp['item_major']
    users, items = z['users'], z['items']
    upload(dev, inp['theta'], inp['beta'], inp['mu'], um, im)
    dev.expo_half_sweep(0, LAM, ne.LAM_Y, True)
    theta = dev.get_factors()[0]
    want = ne.expo_half_sweep_contract(inp['beta'], inp['theta'], um[0], um[1], um[2], inp['mu'], True, LAM, ne.LAM_Y, rows=users)
    print('c2 theta vs contract', ne.rel(theta[users], want), 'vs reference', ne.rel(theta[users], z['ref_theta']), bound(meta['e_ref']['theta']),
          'ms', dev.get_option('expo_last_ns') * 1e-6, 'gram ms', dev.get_option('expo_last_gram_ns') * 1e-6)
    assert ne.rel(theta[users], want) <= bound(meta['e_ref']['theta'])
    # the item side from the ORIGINAL theta, as the fixture's rows were made: restore it first
    dev.set_factors(inp['theta'], inp['beta'])
    dev.expo_half_sweep(1, LAM, ne.LAM_Y, False)
    beta = dev.get_factors()[1]
    want = ne.expo_half_sweep_contract(inp['theta'], inp['beta'], im[0], im[1], im[2], inp['mu'], False, LAM, ne.LAM_Y, rows=items)
    print('c2 beta vs contract', ne.rel(beta[items], want), 'vs reference', ne.rel(beta[items], z['ref_beta']), bound(meta['e_ref']['beta']),
          'ms', dev.get_option('expo_last_ns') * 1e-6, 'gram ms', dev.get_option('expo_last_gram_ns') * 1e-6)
    assert ne.rel(beta[items], want) <= bound(meta['e_ref']['beta'])
    lens = np.diff(im[0])[items]
    assert np.all(beta[items][lens == 0] == 0)


def _random_case(rng, m, n, k):
    ev_u = np.repeat(np.arange(m, dtype=np.int32), 12)
    ev_i = rng.randint(1, n, len(ev_u)).astype(np.int32)
    users0 = rng.choice(m, 300, replace=False).astype(np.int32)               # item 0: long on the item side
    ev_u, ev_i = np.concatenate([ev_u, users0]), np.concatenate([ev_i, np.zeros(300, np.int32)])
    um, im = pairs_from_events(ev_u, ev_i, m, n)
    theta = (0.01 * rng.randn(m, k)).astype(np.float32)
    beta = (0.01 * rng.randn(n, k)).astype(np.float32)
    mu = (0.005 + 0.05 * rng.rand(n)).astype(np.float32)
    return theta, beta, mu, um, im


def test_bit_reproducible_and_long_rows(dev):
    rng = np.random.RandomState(7)
    m, n, k = 700, 450, 22                                     # k not a multiple of 4
    theta0, beta0, mu0, um, im = _random_case(rng, m, n, k)
    dev.set_option('wrmf_long_pairs', 100)
    runs = []
    for _ in range(2):
        upload(dev, theta0, beta0, mu0, um, im)
        assert dev.get_option('wrmf_long_rows_item') >= 1
        dev.expo_half_sweep(0, LAM, ne.LAM_Y, True)
        dev.expo_half_sweep(1, LAM, ne.LAM_Y, False)
        dev.expo_update_mu(ne.PRIOR_A, ne.PRIOR_B, ne.LAM_Y)
        runs.append(dev.get_factors() + (dev.expo_get_mu(),))
    dev.set_option('wrmf_long_pairs', 2048)
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(a, b)
    theta, beta, mu = runs[0]
    want_t = ne.expo_half_sweep_contract(beta0, theta0, um[0], um[1], um[2], mu0, True, LAM, ne.LAM_Y)
    want_b = ne.expo_half_sweep_contract(theta, beta0, im[0], im[1], im[2], mu0, False, LAM, ne.LAM_Y)
    want_m = ne.expo_mu_contract(theta, beta, um[0], um[1], mu0, ne.PRIOR_A, ne.PRIOR_B, ne.LAM_Y)
    print('k=22', ne.rel(theta, want_t), ne.rel(beta, want_b), ne.rel(mu, want_m), 'long row', ne.rel(beta[0], want_b[0]))
    # no fixture of this shape: the floor of the bound (1e-6, WRMF's device-vs-contract figure)
    assert ne.rel(theta, want_t) <= 1e-6 and ne.rel(beta, want_b) <= 1e-6 and ne.rel(mu, want_m) <= 1e-6
    assert ne.rel(beta[0], want_b[0]) <= 1e-6                  # the long row


def test_small_workspace_runs_in_batches(dev):
    rng = np.random.RandomState(8)
    theta0, beta0, mu0, um, im = _random_case(rng, 700, 450, 64)
    upload(dev, theta0, beta0, mu0, um, im)
    dev.expo_half_sweep(0, LAM, ne.LAM_Y, True)
    one = dev.get_factors()[0]
    dev.set_option('expo_gram_mb', 1)
    upload(dev, theta0, beta0, mu0, um, im)
    dev.expo_half_sweep(0, LAM, ne.LAM_Y, True)
    assert dev.get_option('expo_last_batches') > 1
    dev.set_option('expo_gram_mb', 512)
    assert np.array_equal(dev.get_factors()[0], one)


def test_refusals(dev):
    from yue_amd._shim import YueHipError
    rng = np.random.RandomState(5)
    theta0, beta0, mu0, um, im = _random_case(rng, 400, 350, 16)
    upload(dev, theta0, beta0, mu0, um, im)
    bad = mu0.copy()
    bad[3] = 1.0
    with pytest.raises(YueHipError, match='outside'):
        dev.expo_set_mu(bad)
    with pytest.raises(YueHipError, match='per column'):
        dev.expo_half_sweep(0, LAM, 1.0, False)
    with pytest.raises(YueHipError, match='m == n'):
        dev.expo_half_sweep(1, LAM, 1.0, True)
    with pytest.raises(YueHipError, match='lam_y'):
        dev.expo_half_sweep(0, LAM, 0.0, True)
    broken = list(um + im)
    broken[4] = im[1].copy()
    broken[4][0] = (broken[4][0] + 1) % 400
    with pytest.raises(YueHipError):
        dev.expo_set_pairs(*broken)
    dev.set_factors(rng.rand(400, 130).astype(np.float32), rng.rand(350, 130).astype(np.float32))
    dev.expo_set_pairs(*(um + im))
    dev.expo_set_mu(mu0)
    with pytest.raises(YueHipError, match='k = 130'):
        dev.expo_half_sweep(0, LAM, 1.0, True)
    upload(dev, theta0, beta0, mu0, um, im)
    dev.expo_half_sweep(0, LAM, 1.0, True)                     # the context stays usable


def _golden_log(tmp_path, tag):
    from yue_amd import synth
    meta = gj('g13_%s.json' % tag)
    m, n, d = meta['dataset']
    log = tmp_path / 'log.txt'
    synth.write_text_log(str(log), m, n, d)
    with open(str(log), 'a') as f:
        for ln in meta['append']:
            f.write(ln + '\n')
    return log


def _expo_conf(tmp_path, log, k, iters, topn):
    from yue_amd.tool.config import Config
    kv = {'record': str(log), 'recommender': 'ExpoMF', 'num.factors': str(k), 'num.max.iter': str(iters), 'item.ranking': '-topN ' + topn,
          'output.setup': 'on -dir ' + str(tmp_path / 'results') + '/'}
    path = tmp_path / 'expomf.conf'
    path.write_text(_conf_text(kv, {'bpr.hip': '-gpu 0'}))
    return Config(str(path))


@pytest.mark.parametrize('tag', CASES)
def test_goldens_through_the_plugin(tmp_path, capsys, tag):
    from yue_amd.evaluation.measure import Measure
    from yue_amd.recommender.advanced.ExpoMF import ExpoMF
    z, meta, _um, _im = load(tag)
    e = meta['e_ref_last_iteration']
    conf = _expo_conf(tmp_path, _golden_log(tmp_path, tag), int(z['k']), int(z['iters']), meta['topN'])
    rec = ExpoMF(conf, _load(conf), [])
    rec.readConfiguration()
    random.seed(int(z['seed']))
    np.random.seed(int(z['seed']))
    rec.initModel()
    assert np.array_equal(rec.theta, z['theta0']) and np.array_equal(rec.beta, z['beta0']) and np.array_equal(rec.mu, z['mu0'])
    capsys.readouterr()
    rec.buildModel()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if not ln.startswith('[') and not ln.startswith(' ') and ']' not in ln]
    assert lines == meta['lines']
    assert ne.rel(rec.theta, z['thetas'][-1]) <= 4 * e['theta'] and ne.rel(rec.beta, z['betas'][-1]) <= 4 * e['beta'] and ne.rel(rec.mu, z['mus'][-1]) <= 4 * e['mu']
    N = max(int(x) for x in meta['topN'].split(','))
    users = list(rec.data.testSet.keys())
    assert np.array_equal(np.array([rec.data.getId(u, 'user') for u in users], np.int32), z['test_users'])
    ids = rec._scan(users, N)
    stable = z['stable_users']
    print(tag, 'stable users', int(stable.sum()), 'of', len(stable), 'lists equal', int((ids == z['rec_ids']).all(1).sum()))
    assert np.array_equal(ids[stable], z['rec_ids'][stable])
    assert tag != 'expomf_s_k20' or meta['lists_stable']
    if meta['lists_stable']:                                   # every list equal: the lists file and the measure strings too
        assert np.array_equal(ids, z['rec_ids'])
        rec.evalRanking()
        assert rec.measure == meta['measure']
        names = rec.data.id2name[rec.recType]
        want = [u + ':' + ''.join(names[int(x)] + ('*' if names[int(x)] in rec.data.testSet[u] else '') for x in z['rec_ids'][t]) + '\n'
                for t, u in enumerate(users)]
        got = open(glob.glob(str(tmp_path / 'results' / 'ExpoMF@*-top-*items*.txt'))[0]).readlines()
        assert got[1:] == want


def test_driver_entry_and_saved_model_round_trip(tmp_path, capsys):
    from yue_amd.recommender.advanced.ExpoMF import ExpoMF
    from yue_amd.yue import Yue
    meta = gj('g13_expomf_c1_k20.json')
    conf = _expo_conf(tmp_path, _golden_log(tmp_path, 'expomf_c1_k20'), 20, 2, '5,10')
    random.seed(20260013)
    np.random.seed(20260013)
    Yue(conf).execute()
    out = capsys.readouterr().out.splitlines()
    want = iter(meta['lines'])
    nxt = next(want)
    for ln in out:                                             # the reference's lines, in order, among the driver's own
        if ln == nxt:
            nxt = next(want, None)
            if nxt is None:
                break
    assert nxt is None
    assert glob.glob(str(tmp_path / 'results' / 'ExpoMF@*measure*.txt'))
    rec = ExpoMF(conf, _load(conf), [])
    rec.readConfiguration()
    np.random.seed(1)
    rec.initModel()
    rec.buildModel()
    rec.evalRanking()
    first = list(rec.measure)
    users = list(rec.data.testSet.keys())
    lists = rec._scan(users, 10)
    rec.saveModel()
    again = ExpoMF(conf, _load(conf), [])
    again.isLoadModel = True
    assert again.execute() == first
    assert again.theta.dtype == np.float32 and np.array_equal(again.theta, rec.theta) and np.array_equal(again.beta, rec.beta) and np.array_equal(again.mu, rec.mu)
    assert np.array_equal(again._scan(users, 10), lists)
