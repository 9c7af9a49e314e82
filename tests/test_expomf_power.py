"""CPU: what the ExpoMF GPU tests can and cannot see.

Every case of tests/test_gpu_expomf_stages.py (numpy_expomf.TRAINED and the trained-scale C2 rows) is run through the fp64
contract once as it is and once per named mutant of the DENSE posterior (numpy_expomf.DEFECTS; the pairs' correction and the
right-hand side stay exact).  Condition, not measurement: every mutant that applies must move every output the GPU test
compares (the Gram read-out, theta, beta, mu) by at least 10 times the bound the GPU test asserts, max(4 * e_ref, 1e-6).  A case
that does not clear it is reshaped in numpy_expomf.TRAINED, not excused here.

The same file records why those cases exist: from the initial factors (0.01 * randn) the user-side half-sweep moves by less than
the 1e-6 floor when every score is forced to 0, so the tests that start there cannot see the dense posterior at all.

It also pins the helpers the bounds come from: the row-list forms of the reference's arithmetic equal expo_reference_form,
the Gram contract is the Gram the half-sweep contract solves with, and the stored e_ref regenerates.
"""
import numpy as np
import pytest

from helpers import numpy_expomf as ne
from test_expomf_golden import load
from util import gj

LAM = ne.LAM_THETA / ne.LAM_Y
META = gj('g13_expomf_trained.json')
POWER = 10.0
# mu sums the posterior over ALL users per item, so exchanging users (rowswap) leaves it where it is: that mutant does not apply
MU_DEFECTS = ('zero', 'colswap', 'scale', 'drop_tail', 'ratio_by_row')
SMALL = ['k1', 'k2', 'k3', 'k4', 'k5', 'k22', 'sq22', 'n1', 'n127', 'n128', 'n129', 'n512', 'n513']


def bound(e):
    return max(4 * e, 1e-6)


def _moved(mut, exact, scale):
    return float(np.abs(mut.astype(np.float64) - exact.astype(np.float64)).max() / np.abs(scale.astype(np.float64)).max())


def _subset(nr, most=300):
    return np.arange(nr)[::max(1, nr // most)]


def test_fixture_lists_the_cases_and_respects_the_cap():
    assert set(META['cases']) == set(ne.TRAINED)
    for tag, c in ne.TRAINED.items():
        stored = META['cases'][tag]
        assert {key: stored[key] for key in c} == c
        assert set(stored['e_ref']) == ({'gram_user', 'gram_item', 'theta', 'beta', 'mu'} if c['what'] == 'sweep' else {'gram_user'})
        assert 0 < max(stored['e_ref'].values()) <= META['e_ref_cap'] == 1e-5
    assert META['c2']['seed'] == ne.C2_TRAINED_SEED and 0 < max(META['c2']['e_ref'].values()) <= 1e-5
    # what the cases are for
    ks = {c['k'] for c in ne.TRAINED.values() if c['what'] == 'sweep'}
    assert ks >= {1, 2, 3, 4, 5, 22, 30, 45, 64, 127, 128}
    assert {c['n'] for c in ne.TRAINED.values()} >= {1, 127, 128, 129, 512, 513, 9001}
    assert ne.TRAINED['sq22']['m'] == ne.TRAINED['sq22']['n']
    for tag in ('k22', 'k64', 'k128', 'n9001'):
        theta, beta, mu, um, im = ne.trained_inputs(tag)
        s = theta.astype(np.float64) @ beta.astype(np.float64).T
        assert 1.4 < s.std() < 1.6 and np.abs(s).max() > 6
        assert mu.min() >= 0.005 and mu.max() < 0.305 and mu.dtype == np.float32 and theta.dtype == np.float32
        assert np.diff(im[0])[0] >= 250 and (np.diff(um[0]) == 0).sum() >= 3 and (np.diff(im[0]) == 0).sum() >= 3
    theta, beta, mu, um, im = ne.trained_inputs('big_s')
    s = np.abs(theta.astype(np.float64) @ beta.astype(np.float64).T).max()
    assert s > 13 and np.sqrt(np.pi / 2) * np.exp(-s * s / 2) < 1e-8                     # pEX below the 1e-8 term
    mu = ne.trained_inputs('mu_edges')[2]
    assert ((mu >= 1e-6) & (mu <= 1e-2)).sum() >= 20 and ((mu >= 0.99) & (mu < 1)).sum() >= 20 and mu.max() < 1.0
    assert (np.diff(ne.trained_inputs('k64')[3][0]) == 0).sum() == 40


@pytest.mark.parametrize('tag', list(ne.TRAINED))
def test_every_mutant_moves_every_output_ten_bounds(tag):
    c, e = ne.TRAINED[tag], META['cases'][tag]['e_ref']
    theta0, beta0, mu0, um, im = ne.trained_inputs(tag)
    sq = c['m'] == c['n']
    sweep = c['what'] == 'sweep'
    sides = [('user', beta0, theta0, um, True)] + ([('item', None, beta0, im, sq)] if sweep else [])
    seen = 0
    for name, F, Fo, (ptr, idx, cnt), pc in sides:
        if name == 'item':                                   # every stage starts from the seeded factors
            F = theta0
        nr, nf = Fo.shape[0], c['n'] if name == 'user' else c['m']
        gF = F
        lists = ne.gram_row_lists(tag, 0 if name == 'user' else 1, ptr)
        grams = [ne.expo_gram_contract(gF, Fo, mu0, pc, ne.LAM_Y, rows) for rows in lists]
        if sweep:
            exact = ne.expo_half_sweep_contract(F, Fo, ptr, idx, cnt, mu0, pc, LAM, ne.LAM_Y)
            sub = _subset(nr)
        for defect in ne.DEFECTS:
            if not ne.defect_applies(defect, nr, nf, pc):
                continue
            for rows, g in zip(lists, grams):
                if defect == 'rowswap' and len(rows) == 1 and nr < 2:
                    continue
                mut = ne.expo_gram_contract(gF, Fo, mu0, pc, ne.LAM_Y, rows, dense_defect=defect)
                moved = ne.gram_rel(mut, g)
                print(tag, name, 'gram', len(rows), defect, moved, bound(e['gram_' + name]))
                assert moved >= POWER * bound(e['gram_' + name]), (name, 'gram', len(rows), defect, moved)
                seen += 1
            if sweep:
                mut = ne.expo_half_sweep_contract(F, Fo, ptr, idx, cnt, mu0, pc, LAM, ne.LAM_Y, rows=sub, dense_defect=defect)
                key = 'theta' if name == 'user' else 'beta'
                moved = _moved(mut, exact[sub], exact)       # a subset of the rows: a lower bound of what all rows move by
                print(tag, name, key, defect, moved, bound(e[key]))
                assert moved >= POWER * bound(e[key]), (key, defect, moved)
                seen += 1
    if sweep:
        th = be = None
        exact = ne.expo_mu_contract(theta0, beta0, um[0], um[1], mu0, ne.PRIOR_A, ne.PRIOR_B, ne.LAM_Y)
        for defect in MU_DEFECTS:
            if not ne.defect_applies(defect, c['m'], c['m'] if defect == 'drop_tail' else c['n'], True):
                continue
            mut = ne.expo_mu_contract(theta0, beta0, um[0], um[1], mu0, ne.PRIOR_A, ne.PRIOR_B, ne.LAM_Y, dense_defect=defect)
            moved = _moved(mut, exact, exact)
            print(tag, 'mu', defect, moved, bound(e['mu']))
            assert moved >= POWER * bound(e['mu']), ('mu', defect, moved)
            seen += 1
    assert seen >= (4 if c['n'] == 1 else 10)


def test_every_mutant_moves_the_c2_rows_ten_bounds():
    e = META['c2']['e_ref']
    inp = ne.c2_trained(META['c2']['seed'])
    theta, beta, mu, um, im = inp['theta'], inp['beta'], inp['mu'], inp['user_major'], inp['item_major']
    users, items = ne.c2_sample(META['c2']['seed'], um[0], im[0])
    assert (np.diff(im[0])[items] == 0).any()
    # sixteen of the 256 sampled rows per side (with pairs): a lower bound of what the 256 move by
    users16 = users[np.diff(um[0])[users] > 0][::16]
    items16 = items[np.diff(im[0])[items] > 0][::16]
    for name, F, Fo, (ptr, idx, cnt), pc, rows, key in (('user', beta, theta, um, True, users16, 'theta'), ('item', theta, beta, im, False, items16, 'beta')):
        g = ne.expo_gram_contract(F, Fo, mu, pc, ne.LAM_Y, rows)
        exact = ne.expo_half_sweep_contract(F, Fo, ptr, idx, cnt, mu, pc, LAM, ne.LAM_Y, rows=rows)
        for defect in ne.DEFECTS:
            if not ne.defect_applies(defect, Fo.shape[0], F.shape[0], pc):
                continue
            moved = ne.gram_rel(ne.expo_gram_contract(F, Fo, mu, pc, ne.LAM_Y, rows, dense_defect=defect), g)
            assert moved >= POWER * bound(e['gram_' + name]), (name, 'gram', defect, moved)
            mut = ne.expo_half_sweep_contract(F, Fo, ptr, idx, cnt, mu, pc, LAM, ne.LAM_Y, rows=rows, dense_defect=defect)
            moved = _moved(mut, exact, exact)
            print('c2', key, defect, moved, bound(e[key]))
            assert moved >= POWER * bound(e[key]), (key, defect, moved)
    exact = ne.expo_mu_contract(theta, beta, um[0], um[1], mu, ne.PRIOR_A, ne.PRIOR_B, ne.LAM_Y, items=items)
    for defect in MU_DEFECTS:
        mut = ne.expo_mu_contract(theta, beta, um[0], um[1], mu, ne.PRIOR_A, ne.PRIOR_B, ne.LAM_Y, items=items, dense_defect=defect)
        moved = _moved(mut, exact, exact)
        print('c2 mu', defect, moved, bound(e['mu']))
        assert moved >= POWER * bound(e['mu']), ('mu', defect, moved)


@pytest.mark.parametrize('tag', ['expomf_s_k20', 'expomf_z_k20', 'expomf_e_k64', 'expomf_r_k30'])
def test_initial_scale_user_side_is_blind_to_the_posterior(tag):
    # why the trained-scale cases exist: from theta, beta = 0.01 * randn every score forced to 0 moves theta by less than the
    # floor of every device bound, so a user-side half-sweep from the initial factors passes with ANY dense scores
    z, meta, um, im = load(tag)
    theta0, beta0, mu0 = z['theta0'], z['beta0'], z['mu0']
    exact = ne.expo_half_sweep_contract(beta0, theta0, um[0], um[1], um[2], mu0, True, LAM, ne.LAM_Y)
    for defect in ('zero', 'colswap', 'rowswap', 'scale'):
        mut = ne.expo_half_sweep_contract(beta0, theta0, um[0], um[1], um[2], mu0, True, LAM, ne.LAM_Y, dense_defect=defect)
        moved = _moved(mut, exact, exact)
        print(tag, defect, moved)
        assert moved < 1e-6 <= bound(meta['e_ref']['theta']), defect


def test_row_list_forms_equal_the_reference_form():
    # expo_reference_rows / _mu (what every trained-scale e_ref is measured with) against expo_reference_form, which
    # tests/test_expomf_golden.py pins to the reference's own class at 1e-12
    for tag in ('k22', 'sq22'):
        theta0, beta0, mu0, um, im = ne.trained_inputs(tag)
        sq = ne.TRAINED[tag]['m'] == ne.TRAINED[tag]['n']
        thetas, betas, mus = ne.expo_reference_form(theta0, beta0, mu0, um, im, 1)
        th = ne.expo_reference_rows(beta0, theta0, um[0], um[1], um[2], LAM, ne.LAM_Y, mu0, True)
        be = ne.expo_reference_rows(th, beta0, im[0], im[1], im[2], LAM, ne.LAM_Y, mu0, sq)
        mu = ne.expo_reference_mu(th, be, mu0, um[0], um[1], ne.PRIOR_A, ne.PRIOR_B)
        assert th.dtype == np.float32 and mu.dtype == np.float32
        assert ne.rel(th, thetas[0]) < 1e-12 and ne.rel(be, betas[0]) < 1e-12 and ne.rel(mu, mus[0]) < 1e-12
        rows = np.array([3, 5, 250], np.int64)
        assert ne.rel(ne.expo_reference_rows(beta0, theta0, um[0], um[1], um[2], LAM, ne.LAM_Y, mu0, True, rows), thetas[0][rows]) < 1e-5
        assert ne.rel(ne.expo_reference_mu(th, be, mu0, um[0], um[1], ne.PRIOR_A, ne.PRIOR_B, items=rows), mus[0][rows]) < 1e-5


def test_gram_contract_is_the_gram_the_half_sweep_solves_with():
    theta0, beta0, mu0, um, im = ne.trained_inputs('k22')
    k = 22
    rows = np.array([0, 1, 17, 300, 699])
    rows = rows[np.diff(um[0])[rows] > 0]
    G = ne.expo_gram_contract(beta0, theta0, mu0, True, ne.LAM_Y, rows)
    want = ne.expo_half_sweep_contract(beta0, theta0, um[0], um[1], um[2], mu0, True, LAM, ne.LAM_Y, rows=rows)
    B64 = beta0.astype(np.float64)
    ratio = (1.0 - mu0.astype(np.float64)) / mu0.astype(np.float64)
    il = np.tril_indices(k)
    for t, r in enumerate(rows):
        ids = um[1][um[0][r]:um[0][r + 1]]
        B = np.zeros((k, k))
        B[il] = G[t]
        B = B + np.tril(B, -1).T
        A = ne.posterior64(B64[ids] @ theta0[r].astype(np.float64), ratio[ids], ne.LAM_Y)
        B += (B64[ids].T * (1.0 - A)) @ B64[ids] + LAM * np.eye(k)
        x = np.linalg.solve(B, um[2][um[0][r]:um[0][r + 1]].astype(np.float64) @ B64[ids])
        assert np.abs(x - want[t]).max() <= 1e-6 * np.abs(want[t]).max()
    # and a defect-free "mutant" path equals the plain one: dense sum + exact correction is the same B
    a = ne.expo_half_sweep_contract(beta0, theta0, um[0], um[1], um[2], mu0, True, LAM, ne.LAM_Y, rows=rows, dense_defect='drop_tail')
    nf = beta0.shape[0]
    b = ne.expo_half_sweep_contract(beta0[:nf // 128 * 128], theta0, um[0], um[1], um[2], mu0[:nf // 128 * 128], True, LAM, ne.LAM_Y, rows=rows[:0])
    assert a.shape == (len(rows), k) and b.shape == (0, k)


@pytest.mark.parametrize('tag', SMALL)
def test_stored_e_ref_regenerates(tag):
    stored = META['cases'][tag]['e_ref']
    again = ne.trained_e_ref(tag)
    print(tag, again, stored)
    for key in stored:
        assert stored[key] / 2 <= again[key] <= 2 * stored[key], key
