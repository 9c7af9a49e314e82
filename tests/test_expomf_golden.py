"""CPU: the NumPy oracles of ExpoMF (tests/helpers/numpy_expomf.py) against what the reference's own ExpoMF computed
(tests/golden/g13_expomf_*, tools/make_expomf_goldens.py).

expo_reference_form restates the reference at its dtypes and reproduces it to fp64 round-off.  The device contract
(everything in fp64 from the fp32 inputs) cannot equal the reference bit for bit: the reference's posterior and Gram are
fp32 BLAS products.  The gap e_ref was measured per case and per output when the fixture was made and lives in its json;
contract against reference must stay within 2 * e_ref here, device against contract within max(4 * e_ref, 1e-6) on the GPU
(tests/test_gpu_expomf.py; the reasons for the factors are in DESIGN.md section 16).
"""
import numpy as np
import pytest

from helpers import numpy_expomf as ne
from helpers.numpy_wrmf import pairs_from_events
from util import gj, gz

CASES = ['expomf_c1_k20', 'expomf_e_k64', 'expomf_f_k128', 'expomf_s_k20', 'expomf_sq_k20', 'expomf_z_k20', 'expomf_r_k30']


def load(tag):
    z = dict(gz('g13_%s.npz' % tag))
    meta = gj('g13_%s.json' % tag)
    m, n = int(z['m']), int(z['n'])
    if 'theta0' not in z:                                    # the k = 128 case keeps its size down: initModel's draws from the seed
        z['theta0'], z['beta0'] = ne.init_from_seed(int(z['seed']), m, n, int(z['k']))
    um, im = pairs_from_events(z['ev_u'], z['ev_i'], m, n)
    return z, meta, um, im


@pytest.mark.parametrize('tag', CASES)
def test_reference_form_reproduces_the_reference(tag):
    z, meta, um, im = load(tag)
    thetas, betas, mus = ne.expo_reference_form(z['theta0'], z['beta0'], z['mu0'], um, im, int(z['iters']))
    for t in range(int(z['iters'])):
        assert thetas[t].dtype == np.float32 and betas[t].dtype == np.float32 and mus[t].dtype == np.float32
        assert ne.rel(thetas[t], z['thetas'][t]) < 1e-12 and ne.rel(betas[t], z['betas'][t]) < 1e-12 and ne.rel(mus[t], z['mus'][t]) < 1e-12


@pytest.mark.parametrize('tag', CASES)
def test_contract_within_twice_the_measured_gap(tag):
    z, meta, um, im = load(tag)
    e = meta['e_ref']
    th, be, mu = z['theta0'], z['beta0'], z['mu0']
    for t in range(int(z['iters'])):
        th, be, mu = ne.expo_iteration_contract(th, be, mu, um, im)
        got = {'theta': ne.rel(z['thetas'][t], th), 'beta': ne.rel(z['betas'][t], be), 'mu': ne.rel(z['mus'][t], mu)}
        print(tag, t, got, e)
        for key in got:
            assert got[key] <= 2 * e[key], (key, t)
    # rows without training pairs: exactly zero in the reference and in the contract
    assert np.all(z['thetas'][-1][z['zero_users']] == 0) and np.all(th[z['zero_users']] == 0)
    assert np.all(z['betas'][-1][z['zero_items']] == 0) and np.all(be[z['zero_items']] == 0)


def test_cases_cover_what_they_are_for():
    assert int(gz('g13_expomf_sq_k20.npz')['m']) == int(gz('g13_expomf_sq_k20.npz')['n'])
    for tag in ('expomf_e_k64', 'expomf_f_k128'):
        assert int(gz('g13_%s.npz' % tag)['m']) != int(gz('g13_%s.npz' % tag)['n'])
    z = gz('g13_expomf_z_k20.npz')
    assert len(z['zero_users']) == 6 and len(z['zero_items']) >= 4
    assert gj('g13_expomf_r_k30.json')['max_count'] >= 8
    assert {int(gz('g13_%s.npz' % t)['k']) for t in CASES} >= {20, 64, 128, 30}


def test_square_case_exercises_the_mu_quirk():
    # m == n: the item half-sweep takes mu per column (a user id).  With mu per row instead the result leaves the bound.
    z, meta, um, im = load('expomf_sq_k20')
    th, be, mu = z['theta0'], z['beta0'], z['mu0']
    for t in range(int(z['iters'])):
        th, be, mu = ne.expo_iteration_contract(th, be, mu, um, im, item_mu_per_column=False)
    assert ne.rel(z['betas'][-1], be) > 2 * meta['e_ref']['beta']
    assert ne.rel(z['mus'][-1], mu) > 2 * meta['e_ref']['mu']


def test_c2_rows_contract_against_the_reference_rows():
    # the large shape regenerated from its seeds: the contract on the 512 sampled rows against what the reference computed
    z, meta = gz('g13_expomf_c2rows.npz'), gj('g13_expomf_c2rows.json')
    assert z['ref_theta'].shape == (256, 64) and z['ref_beta'].shape == (256, 64)
    inp = ne.c2_inputs(int(z['seed']))
    um, im = inp['user_major'], inp['item_major']
    users, items = ne.c2_sample(int(z['seed']), um[0], im[0])
    assert np.array_equal(users, z['users']) and np.array_equal(items, z['items'])
    lam = ne.LAM_THETA / ne.LAM_Y
    con_u = ne.expo_half_sweep_contract(inp['beta'], inp['theta'], um[0], um[1], um[2], inp['mu'], True, lam, ne.LAM_Y, rows=users)
    con_i = ne.expo_half_sweep_contract(inp['theta'], inp['beta'], im[0], im[1], im[2], inp['mu'], False, lam, ne.LAM_Y, rows=items)
    got = {'theta': ne.rel(z['ref_theta'], con_u), 'beta': ne.rel(z['ref_beta'], con_i)}
    print(got, meta['e_ref'])
    for key in got:
        assert 0 < got[key] <= 2 * meta['e_ref'][key], key
    lens = np.diff(im[0])[items]
    assert (lens == 0).sum() == 1 and (lens == 1).sum() >= 1
    assert np.all(z['ref_beta'][lens == 0] == 0) and np.all(con_i[lens == 0] == 0)
    assert set(np.argsort(-np.diff(um[0]), kind='stable')[:16]) <= set(users) and set(np.argsort(-np.diff(im[0]), kind='stable')[:16]) <= set(items)


def test_the_small_case_has_stable_lists_for_every_user():
    # the case on which the GPU test compares the lists file and the measure strings with the reference's
    z, meta, um, im = load('expomf_s_k20')
    assert meta['lists_stable'] and z['stable_users'].all() and len(z['stable_users']) == meta['test_users'] > 0
    th, be, mu = z['theta0'], z['beta0'], z['mu0']
    for _ in range(int(z['iters'])):
        th, be, mu = ne.expo_iteration_contract(th, be, mu, um, im)
    N = max(int(x) for x in meta['topN'].split(','))
    for t, u in enumerate(z['test_users']):
        scores = z['betas'][-1].dot(z['thetas'][-1][u])
        ids, margin = ne.overwrite_scan(scores, set(int(i) for i in um[1][um[0][u]:um[0][u + 1]]), N,
                                        ne.score_error(z['thetas'][-1], z['betas'][-1], th, be, u))
        assert ids == [int(x) for x in z['rec_ids'][t]] and margin > 0


def test_plugin_is_importable_and_in_the_menu():
    from yue_amd.main import MENU
    from yue_amd.recommender.advanced.ExpoMF import ExpoMF
    assert MENU['a6'] == 'ExpoMF' and callable(ExpoMF.buildModel)
