"""GPU: the edges APR's kernels can get wrong (tests/helpers/apr_cases.py: EDGE_CASES), under the bounds of tests/test_gpu_apr.py:
k at one live lane, around one and two registers per lane and at the widest (1, 63, 65, 129, 256; 64 and 128 are that file's); a
single triplet; one user in every triplet (a row list of length T); the forced triplets of every case (an item positive for one user
and negative for another, one that is both in one batch, a triplet twice, items 0 and n - 1, user m - 1); a triplet with i == j as its
user's only one; eps = 0; regA = 0; and a perturbation carried from one batch to the next."""
import numpy as np
import pytest

from helpers import apr_cases as ac
from test_gpu_apr import check_case, dev, hold, outputs, upload                    # noqa: F401  (dev: the fixture)

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize('name', ['k1', 'k63', 'k65', 'k129', 'k256'])
def test_every_width_of_a_row(dev, name):
    c = ac.build(name)
    got = check_case(dev, c)
    # the forced triplets: both ends of both axes took part
    for q, rows in (('gU_pre', [c['m'] - 1, 1, 2]), ('gV_pre', [0, c['n'] - 1, ac.A, ac.B]), ('dU', [c['m'] - 1, 1, 2]), ('dV', [0, c['n'] - 1, ac.A, ac.B])):
        assert all(got[q][r].any() for r in rows), q


def test_a_single_triplet(dev):
    c = ac.build('T1')
    got = check_case(dev, c)
    assert dev.get_option('apr_last_longest_row') == 1
    assert int(got['dU'].any(axis=1).sum()) == 1 and int(got['dV'].any(axis=1).sum()) == 2


def test_one_user_in_every_triplet(dev):
    c = ac.build('hubuser')
    assert (c['u'] == ac.HUB_USER).all()
    check_case(dev, c)
    assert dev.get_option('apr_last_longest_row') == c['T']


def test_i_equal_j_cancels_exactly_and_the_floor_keeps_zero(dev):
    c = ac.build('ieqj')
    u, i, j = c['u'], c['i'], c['j']
    assert np.flatnonzero(u == ac.LONE_USER).tolist() == [10] and i[10] == j[10] == ac.LONE_ITEM
    assert c['dU'][ac.LONE_USER].any() and c['dV'][ac.LONE_ITEM].any()          # both rows stand perturbed before the update
    got = check_case(dev, c)
    for q in ('gU_adv', 'rawU', 'dU'):
        assert not bits(got[q][ac.LONE_USER]).any(), q                  # +0.0 in every element: 0 * rsqrt(1e-12) * eps
    for q in ('gV_adv', 'rawV', 'dV'):
        assert not bits(got[q][ac.LONE_ITEM]).any(), q
    # phase 1's regularisation is all that is left of the user row's gradient: 2 reg U_u (the item row adds a U_u and takes it away
    # again, which rounds: check_case's bound holds it)
    assert np.array_equal(got['gU_pre'][ac.LONE_USER], (2 * np.float32(ac.REG)) * c['U'][ac.LONE_USER])
    # ... and through a whole adversarial step
    loss = dev.apr_adv_step(u, i, j, 0.002, c['eps'], c['regA'], 1)
    dU, dV = dev.apr_get_delta()
    P, Q = dev.get_factors()
    assert np.isfinite(loss) and all(np.isfinite(x).all() for x in (dU, dV, P, Q))
    assert not bits(dU[ac.LONE_USER]).any() and not bits(dV[ac.LONE_ITEM]).any()
    assert np.array_equal(P[ac.LONE_USER], c['U'][ac.LONE_USER])        # a zero gradient on zero moments: the row stays


def test_eps_zero_leaves_no_perturbation_and_scales_the_clean_gradient(dev):
    c = ac.build('eps0')
    u, i, j = c['u'], c['i'], c['j']
    got = check_case(dev, c)
    assert c['dU'].any() and not got['dU'].any() and not got['dV'].any()
    # at D = 0 the perturbed margins are the clean ones: the adversarial gradient is (1 + regA) times the clean one
    _, gU, gV = dev.apr_grad(True, u, i, j, c['regA'])
    _, cU, cV = dev.apr_grad(False, u, i, j, 0.0)
    for q, g, clean in (('gU_adv', gU, cU), ('gV_adv', gV, cV)):
        want = (1.0 + c['regA']) * clean.astype(np.float64)
        dist = ac.ap.rel(g, want)
        print('eps0', q, '%.3g' % dist, 'bound %.3g' % ac.bound(c['d32'], c['L'], q))
        assert dist <= ac.bound(c['d32'], c['L'], q)


def test_reg_a_zero(dev):
    c = ac.build('regA0')
    got = check_case(dev, c)
    assert not got['rawU'].any() and not got['dU'].any() and not got['rawV'].any() and not got['dV'].any()
    # loss_adv is the clean loss, its gradient the clean gradient: phase 1's without the l2 term, in the same bits
    loss, cU, cV = dev.apr_grad(False, c['u'], c['i'], c['j'], 0.0)
    upload(dev, c)
    loss_a, gU, gV = dev.apr_grad(True, c['u'], c['i'], c['j'], 0.0)
    assert loss == loss_a and np.array_equal(gU, cU) and np.array_equal(gV, cV)


def test_a_perturbation_is_carried_to_the_rows_both_batches_share(dev):
    c = ac.build('carried')
    first, second = (c['u1'], c['i1'], c['j1']), (c['u'], c['i'], c['j'])
    rows1 = (np.unique(first[0]), np.unique(np.concatenate(first[1:])))
    rows2 = (np.unique(second[0]), np.unique(np.concatenate(second[1:])))
    for a, b in zip(rows1, rows2):                                       # rows of both batches, of the first alone, of the second alone
        assert len(np.intersect1d(a, b)) and len(np.setdiff1d(a, b)) and len(np.setdiff1d(b, a))
    upload(dev, c)
    dev.apr_reset()
    U, V, eps, regA = c['U'], c['V'], c['eps'], c['regA']
    zero = (np.zeros_like(U), np.zeros_like(V))
    want, d32, L = ac.measure(U, V, zero[0], zero[1], *first, eps, regA)
    got1 = outputs(dev, *first, eps, regA)
    hold('carried, first', got1, want, d32, L)
    # the second batch: the yardstick starts from the device's own perturbation, so that it measures this update alone
    D1 = (got1['dU'], got1['dV'])
    want, d32, L = ac.measure(U, V, D1[0], D1[1], *second, eps, regA)
    got2 = outputs(dev, *second, eps, regA)
    hold('carried, second', got2, want, d32, L)
    # the gradient on a shared row was taken at the old perturbation, not at zero
    at_zero = ac.measure(U, V, zero[0], zero[1], *second, eps, regA)[0]
    shared = np.intersect1d(rows1[0], rows2[0])
    assert ac.ap.rel(got2['rawU'][shared], at_zero['rawU'][shared]) > 100 * ac.bound(d32, L, 'rawU')
    # rows of the first batch alone are gone, rows of the second alone came from zero
    gone_u, gone_i = np.setdiff1d(rows1[0], rows2[0]), np.setdiff1d(rows1[1], rows2[1])
    assert got1['dU'][gone_u].any(axis=1).all() and not got2['dU'][gone_u].any() and not got2['dV'][gone_i].any()
    fresh_u = np.setdiff1d(rows2[0], rows1[0])
    assert got2['dU'][fresh_u].any(axis=1).all()
