"""GPU: ExpoMF's device stages against fp64 at trained scale, where the posterior varies from column to column.

tests/test_gpu_expomf.py starts every user-side half-sweep from theta, beta = 0.01 * randn: there |s| <= 4e-3, the posterior
is a constant per column, and any score is as good as another (tests/test_expomf_power.py asserts that blindness).  Here the
inputs are numpy_expomf.trained_case's (scores of standard deviation 1.5 reaching 7..9, mu in [0.005, 0.305)), on which every
named mutant of the dense stage moves every compared output by at least ten times its bound (the same file).

What is compared, always from identical inputs and always against the fp64 contract (tests/helpers/numpy_expomf.py):
  * the dense Gram itself, read out by yue_expo_gram_rows (the half-sweep's own k_expo_gram<NB> with its nb, gy, splits), entry by
    entry and relative to the row's largest entry: k = 1..5 (one pair block, idle waves, K padding), 22 (NB 2), 30 (NB 4),
    45 (first NB 6, gy 2), 64 (gy 3), 127 and 128 (gy 11); both sides, the item side with mu per row and, on the square case,
    per column; 1, 127, 128, 129, 512, 513 and 9001 columns; a lone row, and 33 rows with a row without pairs among them;
  * whole half-sweeps and the mu update on the same k values, every row, each stage from the seeded factors; the 9001-column case; the long item row in chunks;
    a 1 MiB workspace whose last batch holds only rows without pairs; mu at both ends of (0, 1); scores beyond 13;
  * the C2 shape at trained scale on the 256 + 256 sampled rows.
Every bound is max(4 * e_ref, 1e-6) with e_ref = the reference's arithmetic against the contract on the same inputs, computed on
the CPU by tools/make_expomf_goldens.py into tests/golden/g13_expomf_trained.json (capped at 1e-5); nothing was tuned on the
device.  Each test prints its figures before it asserts.
"""
import numpy as np
import pytest

from helpers import numpy_expomf as ne
from util import gj

pytestmark = pytest.mark.gpu

LAM = ne.LAM_THETA / ne.LAM_Y
META = gj('g13_expomf_trained.json')
SWEEP = [t for t, c in ne.TRAINED.items() if c['what'] == 'sweep']


@pytest.fixture(scope='module')
def dev():
    from yue_amd._shim import Device
    d = Device(0, raise_errors=True)
    yield d
    d.close()


def bound(e):
    assert e <= META['e_ref_cap']
    return max(4 * e, 1e-6)


def upload(dev, theta, beta, mu, um, im):
    dev.set_factors(theta, beta)
    dev.expo_set_pairs(*(um + im))
    dev.expo_set_mu(mu)


@pytest.mark.parametrize('tag', list(ne.TRAINED))
def test_gram_equals_the_fp64_gram(dev, tag):
    c, e = ne.TRAINED[tag], META['cases'][tag]['e_ref']
    theta0, beta0, mu0, um, im = ne.trained_inputs(tag)
    upload(dev, theta0, beta0, mu0, um, im)
    sides = [(0, 'gram_user', beta0, theta0, um[0], True)]
    if c['what'] == 'sweep':
        sides.append((1, 'gram_item', theta0, beta0, im[0], c['m'] == c['n']))
    for side, key, F, Fo, ptr, per_column in sides:
        lists = ne.gram_row_lists(tag, side, ptr)
        assert len(lists[0]) == 1 and len(lists[1]) == 33
        assert (np.diff(ptr)[lists[1]] == 0).any()                                        # a row without pairs is in the list
        for rows in lists:
            got = dev.expo_gram_rows(side, per_column, ne.LAM_Y, rows)
            want = ne.expo_gram_contract(F, Fo, mu0, per_column, ne.LAM_Y, rows)
            d = ne.gram_rel(got, want)
            print(tag, key, 'rows', len(rows), 'device vs fp64', d, 'bound', bound(e[key]))
            assert got.shape == want.shape and d <= bound(e[key]), (key, len(rows))
    theta, beta = dev.get_factors()
    assert np.array_equal(theta, theta0) and np.array_equal(beta, beta0)                 # the read-out changes no factor


def _sweeps(dev, tag, theta0, beta0, mu0, um, im):
    """The three stages, each from the SEEDED factors (only those are at trained scale by construction: numpy_expomf.trained_e_ref):
    the user half-sweep, the item half-sweep, the mu update.  Returns the distances to the contract, the results, the contract's."""
    c = ne.TRAINED[tag]
    sq = c['m'] == c['n']
    dev.expo_half_sweep(0, LAM, ne.LAM_Y, True)
    theta, beta = dev.get_factors()
    assert np.array_equal(beta, beta0)
    want_t = ne.expo_half_sweep_contract(beta0, theta0, um[0], um[1], um[2], mu0, True, LAM, ne.LAM_Y)
    dev.set_factors(theta0, beta0)
    dev.expo_half_sweep(1, LAM, ne.LAM_Y, sq)
    theta2, beta = dev.get_factors()
    assert np.array_equal(theta2, theta0)
    want_b = ne.expo_half_sweep_contract(theta0, beta0, im[0], im[1], im[2], mu0, sq, LAM, ne.LAM_Y)
    dev.set_factors(theta0, beta0)
    dev.expo_update_mu(ne.PRIOR_A, ne.PRIOR_B, ne.LAM_Y)
    mu = dev.expo_get_mu()
    want_m = ne.expo_mu_contract(theta0, beta0, um[0], um[1], mu0, ne.PRIOR_A, ne.PRIOR_B, ne.LAM_Y)
    assert mu.dtype == np.float32
    return {'theta': ne.rel(theta, want_t), 'beta': ne.rel(beta, want_b), 'mu': ne.rel(mu, want_m)}, (theta, beta, mu), (want_t, want_b)


@pytest.mark.parametrize('tag', SWEEP)
def test_half_sweeps_and_mu_equal_the_contract(dev, tag):
    e = META['cases'][tag]['e_ref']
    theta0, beta0, mu0, um, im = ne.trained_inputs(tag)
    upload(dev, theta0, beta0, mu0, um, im)
    got, (theta, beta, _mu), _ = _sweeps(dev, tag, theta0, beta0, mu0, um, im)
    print(tag, {key: (got[key], bound(e[key])) for key in got})
    zu, zi = np.diff(um[0]) == 0, np.diff(im[0]) == 0
    assert zu.any() and zi.any()
    assert np.all(theta[zu] == 0) and np.all(beta[zi] == 0)
    for key in ('theta', 'beta', 'mu'):
        assert got[key] <= bound(e[key]), key


def test_long_item_row_in_chunks(dev):
    # item 0 of k22 has 300 users: with wrmf_long_pairs = 100 its pairs' correction runs in chunks (k_expo_chunk)
    tag = 'k22'
    e = META['cases'][tag]['e_ref']
    theta0, beta0, mu0, um, im = ne.trained_inputs(tag)
    dev.set_option('wrmf_long_pairs', 100)
    try:
        runs = []
        for _ in range(2):
            upload(dev, theta0, beta0, mu0, um, im)
            assert dev.get_option('wrmf_long_rows_item') >= 1
            got, res, want = _sweeps(dev, tag, theta0, beta0, mu0, um, im)
            runs.append(res)
    finally:
        dev.set_option('wrmf_long_pairs', 2048)
    long_row = ne.rel(runs[0][1][0], want[1][0])
    print(tag, 'long rows', got, 'item 0', long_row)
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(a, b)                                                      # bit-reproducible
    for key in ('theta', 'beta', 'mu'):
        assert got[key] <= bound(e[key]), key
    assert long_row <= bound(e['beta'])


def test_small_workspace_last_batch_without_pairs(dev):
    # k64: 700 users, 40 of them without pairs.  With a 1 MiB workspace a batch is one tile of 32 rows (5 splits x 2080 pairs x
    # 4 bytes x 32 rows = 1.27 MiB is over, so the floor of one tile holds): 22 batches; the 660 rows with pairs end inside
    # batch 20 (positions 640..671: a tile that straddles the last row with pairs), and batch 21 holds only rows without pairs
    # (no Gram launch at all).  Bit-equal to the one-batch run, and the rows without pairs exactly 0.
    tag = 'k64'
    e = META['cases'][tag]['e_ref']
    theta0, beta0, mu0, um, im = ne.trained_inputs(tag)
    m = ne.TRAINED[tag]['m']
    zu = np.diff(um[0]) == 0
    live = int((~zu).sum())
    assert live % 32 != 0 and (m - 1) // 32 * 32 >= live
    upload(dev, theta0, beta0, mu0, um, im)
    dev.expo_half_sweep(0, LAM, ne.LAM_Y, True)
    assert dev.get_option('expo_last_batches') == 1
    one = dev.get_factors()[0]
    dev.set_option('expo_gram_mb', 1)
    try:
        upload(dev, theta0, beta0, mu0, um, im)
        dev.expo_half_sweep(0, LAM, ne.LAM_Y, True)
        batches = dev.get_option('expo_last_batches')
    finally:
        dev.set_option('expo_gram_mb', 512)
    many = dev.get_factors()[0]
    want = ne.expo_half_sweep_contract(beta0, theta0, um[0], um[1], um[2], mu0, True, LAM, ne.LAM_Y)
    print(tag, 'batches', batches, 'theta vs contract', ne.rel(many, want), bound(e['theta']))
    assert batches == (m + 31) // 32
    assert np.array_equal(many, one)
    assert np.all(many[zu] == 0) and zu.sum() == 40
    assert ne.rel(many, want) <= bound(e['theta'])


def test_c2_at_trained_scale(dev):
    meta = META['c2']
    e = meta['e_ref']
    inp = ne.c2_trained(meta['seed'])
    theta0, beta0, mu0, um, im = inp['theta'], inp['beta'], inp['mu'], inp['user_major'], inp['item_major']
    users, items = ne.c2_sample(meta['seed'], um[0], im[0])
    assert [len(users), len(items)] == meta['rows']
    upload(dev, theta0, beta0, mu0, um, im)
    # the dense stage alone
    for side, key, F, Fo, rows in ((0, 'gram_user', beta0, theta0, users), (1, 'gram_item', theta0, beta0, items)):
        got = dev.expo_gram_rows(side, side == 0, ne.LAM_Y, rows)
        d = ne.gram_rel(got, ne.expo_gram_contract(F, Fo, mu0, side == 0, ne.LAM_Y, rows))
        print('c2', key, d, bound(e[key]))
        assert d <= bound(e[key]), key
    # mu from the seeded factors, on the sampled items
    dev.expo_update_mu(ne.PRIOR_A, ne.PRIOR_B, ne.LAM_Y)
    mu = dev.expo_get_mu()
    d = ne.rel(mu[items], ne.expo_mu_contract(theta0, beta0, um[0], um[1], mu0, ne.PRIOR_A, ne.PRIOR_B, ne.LAM_Y, items=items))
    print('c2 mu', d, bound(e['mu']))
    assert d <= bound(e['mu'])
    dev.expo_set_mu(mu0)
    # rows through real half-sweeps: users; items from the SOLVED theta; items from the seeded theta
    dev.expo_half_sweep(0, LAM, ne.LAM_Y, True)
    theta = dev.get_factors()[0]
    d = ne.rel(theta[users], ne.expo_half_sweep_contract(beta0, theta0, um[0], um[1], um[2], mu0, True, LAM, ne.LAM_Y, rows=users))
    print('c2 theta', d, bound(e['theta']), 'ms', dev.get_option('expo_last_ns') * 1e-6, 'gram ms', dev.get_option('expo_last_gram_ns') * 1e-6)
    assert d <= bound(e['theta'])
    dev.expo_half_sweep(1, LAM, ne.LAM_Y, False)
    beta = dev.get_factors()[1]
    want = ne.expo_half_sweep_contract(theta, beta0, im[0], im[1], im[2], mu0, False, LAM, ne.LAM_Y, rows=items)
    # the solved theta exists on the device only (100,000 fp64 solves on the CPU are hours), so this one e_ref is taken here,
    # by the same rule and under the same cap: the reference's arithmetic against the contract on these very inputs
    e_solved = ne.rel(ne.expo_reference_rows(theta, beta0, im[0], im[1], im[2], LAM, ne.LAM_Y, mu0, False, items), want)
    d = ne.rel(beta[items], want)
    print('c2 beta from the solved theta', d, bound(e_solved), 'ms', dev.get_option('expo_last_ns') * 1e-6)
    assert d <= bound(e_solved)
    lens = np.diff(im[0])[items]
    assert (lens == 0).any() and np.all(beta[items][lens == 0] == 0)
    dev.set_factors(theta0, beta0)
    dev.expo_half_sweep(1, LAM, ne.LAM_Y, False)
    beta = dev.get_factors()[1]
    d = ne.rel(beta[items], ne.expo_half_sweep_contract(theta0, beta0, im[0], im[1], im[2], mu0, False, LAM, ne.LAM_Y, rows=items))
    print('c2 beta from the seeded theta', d, bound(e['beta']))
    assert d <= bound(e['beta'])


def test_gram_rows_refuses_what_the_half_sweep_refuses(dev):
    from yue_amd._shim import YueHipError
    theta0, beta0, mu0, um, im = ne.trained_inputs('k5')
    upload(dev, theta0, beta0, mu0, um, im)
    rows = np.arange(4, dtype=np.int32)
    with pytest.raises(YueHipError, match='per column'):
        dev.expo_gram_rows(0, False, 1.0, rows)
    with pytest.raises(YueHipError, match='m == n'):
        dev.expo_gram_rows(1, True, 1.0, rows)
    with pytest.raises(YueHipError, match='lam_y'):
        dev.expo_gram_rows(0, True, 0.0, rows)
    with pytest.raises(YueHipError, match='outside'):
        dev.expo_gram_rows(0, True, 1.0, np.array([0, 260], np.int32))
    with pytest.raises(YueHipError, match='outside'):
        dev.expo_gram_rows(1, False, 1.0, np.array([-1], np.int32))
    dev.set_factors(np.ones((260, 130), np.float32), np.ones((300, 130), np.float32))
    dev.expo_set_pairs(*(um + im))
    dev.expo_set_mu(mu0)
    with pytest.raises(YueHipError, match='k = 130'):
        dev.expo_gram_rows(0, True, 1.0, rows)
    upload(dev, theta0, beta0, mu0, um, im)
    assert dev.expo_gram_rows(0, True, 1.0, rows).shape == (4, 15)                       # the context stays usable
