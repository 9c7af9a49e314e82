"""GPU: FISM's kernels at their register-width, LDS and touch-count edges (tests/helpers/fism_cases.py; tests/test_fism_golden.py
proves on the CPU that every case reaches the branch it is named for).  Every run is compared with the NumPy oracle
(oracle/numpy_fism.py) under the bounds of tests/test_gpu_fism.py -- sequential form: P and Bi within 1e-11, Q within 1e-6,
the data loss within 1e-10; round forms: 1e-6 -- and the read-only option fism_last_form tells which form ran.  Where nothing
is reordered (one user per round, rows in place) the round form is held to the sequential form bit for bit.  Every case prints
its distances."""
import numpy as np
import pytest

from helpers import fism_cases as fc
from util import rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    from yue_amd._shim import Device
    d = Device(0, raise_errors=True)
    yield d
    d.set_option('fism_lds', 1)
    d.set_option('fism_inplace', 1)
    d.close()


def run(dev, c, round_users=None, lds=1, inplace=1):
    """(half, sums of squares, P, Q, Bi, form) of one pass over the case from its start model."""
    try:
        dev.set_option('fism_lds', lds)
        dev.set_option('fism_inplace', inplace)
        dev.fism_set_model(c['P0'], c['Q0'], c['B0'])
        if round_users is None:
            half, sp, sq, sb = dev.fism_epoch(c['user_ptr'], c['ev_i'], c['negs'], c['rho'], c['coef'], c['lr'], fc.REG_I, fc.REG_B)
            form = None
        else:
            half, sp, sq, sb = dev.fism_rounds(c['user_ptr'], c['ev_i'], c['negs'], c['rho'], c['coef'], round_users, c['lr'], fc.REG_I, fc.REG_B)
            form = dev.get_option('fism_last_form')
        P, Q, Bi = np.empty_like(c['P0']), np.empty_like(c['Q0']), np.empty_like(c['B0'])
        dev.fism_get_model(P, Q, Bi)
    finally:
        dev.set_option('fism_lds', 1)
        dev.set_option('fism_inplace', 1)
    return half, (sp, sq, sb), P, Q, Bi, form


def distances(got, want):
    half, _, P, Q, Bi, _ = got
    half_o, Po, Qo, Bo = want
    return rel_err(P, Po), rel_err(Q, Qo), rel_err(Bi, Bo), abs(half - half_o) / half_o


def check_epoch(dev, name):
    c = fc.build(name)
    d = distances(run(dev, c), fc.oracle(name))
    print('%s k_fism_epoch<%d>: P %.3g Q %.3g Bi %.3g half %.3g' % ((name, fc.kr_of(c['k'])) + d))
    assert d[0] < 1e-11 and d[1] < 1e-6 and d[2] < 1e-11 and d[3] < 1e-10, (name, d)


def check_rounds(dev, name, pairs=fc.OPTION_PAIRS):
    c = fc.build(name)
    for U in c['rounds']:
        for lds, inplace in pairs:
            got = run(dev, c, U, lds, inplace)
            d = distances(got, fc.oracle(name, U))
            print('%s rounds of %d lds %d inplace %d form %d: P %.3g Q %.3g Bi %.3g half %.3g' % ((name, U, lds, inplace, got[5]) + d))
            assert got[5] == (c['form'][U] if lds else 0), (name, U, lds, got[5])
            assert max(d) < 1e-6, (name, U, lds, inplace, d)


@pytest.mark.parametrize('name', fc.WIDTH_CASES)
def test_widths(dev, name):
    # k = 1 .. 256 around every change of the register count (64 | 65, 128 | 129) and of the form (100 | 127, 212 | 256 at 64 touches),
    # at 64 touches (S64) and at 9 (S9: an odd rows_cap, with odd k the padded START layout)
    check_epoch(dev, name)
    check_rounds(dev, name)


def _lds_cases(names):
    # (S64_k256 is left out: 64 rows of k = 256 do not fit, its rounds go through k_fism_round and the difference buffers)
    return [n for n in names if fc.host_form(fc.BY_NAME[n]['sizes'], fc.BY_NAME[n]['rho'], fc.BY_NAME[n]['k'], 1, 256) > 0]


@pytest.mark.parametrize('name', _lds_cases(fc.WIDTH_CASES + ['T63', 'two_rows', 'own_k64', 'own_k100']))
def test_one_user_per_round_in_place_is_the_sequential_pass_bit_for_bit(dev, name):
    # one user per round with fism_lds = fism_inplace = 1: every row has one toucher and is stored in place, and the wave issues
    # k_fism_epoch's double and float operations in its order (the same butterfly, no contraction; the event's row and bias held in
    # registers instead of reloaded, with the same values).  Only the data loss is summed in another order (per user, then atomics).
    c = fc.build(name)
    assert c['form'][1] > 0
    e, r, r2 = run(dev, c), run(dev, c, 1), run(dev, c, 1)
    diff = [int((a != b).sum()) for a, b in zip(e[2:5], r[2:5])]
    print('%s form %d against k_fism_epoch: differing elements P %d Q %d Bi %d, half %.3g rel' % (name, r[5], diff[0], diff[1], diff[2], abs(r[0] - e[0]) / e[0]))
    assert diff == [0, 0, 0], (name, diff)
    assert abs(r[0] - e[0]) <= 1e-12 * e[0]
    assert all(np.array_equal(a, b) for a, b in zip(r[2:5], r2[2:5])) and r[0] == r2[0]


@pytest.mark.parametrize('name', ['T68', 'T63', 'two_rows'])
def test_touch_counts_around_64(dev, name):
    # 64 touches (every lane holds one: S64 above, and two_rows: 64 touches on two working rows), 63, and 68 -> the whole call
    # falls back to the form with working rows in global memory
    check_epoch(dev, name)
    check_rounds(dev, name)


def test_a_round_larger_than_the_cus_hold_drops_the_round_start_rows(dev):
    # 600 users at k = 100 and 64 touches: twice the rows fit in LDS, but one workgroup per CU does not hold 600 -> form 1;
    # rounds of 40 and 41 (a last round shorter than the others) -> form 2
    check_rounds(dev, 'big_round')


@pytest.mark.parametrize('name', ['own_k64', 'own_k100'])
def test_negatives_that_are_other_items_of_the_user_share_their_rows(dev, name):
    check_epoch(dev, name)
    check_rounds(dev, name)


@pytest.mark.parametrize('name', ['own_k64', 'own_k100'])
def test_a_negative_equal_to_its_own_events_item_is_refused_and_changes_nothing(dev, name):
    from yue_amd._shim import ERR_ARG, YueHipError
    c = fc.build(name)
    ptr, rho = c['user_ptr'], c['rho']
    u = 5                                                 # the first user of 16 events
    e = int(ptr[u]) + 9
    t = sum(s * rho for s in c['sizes'][:u] if s > 1) + 9 * rho + 1
    negs = c['negs'].copy()
    negs[t] = c['ev_i'][e]
    dev.fism_set_model(c['P0'], c['Q0'], c['B0'])
    calls = [lambda: dev.fism_epoch(ptr, c['ev_i'], negs, rho, c['coef'], c['lr'], fc.REG_I, fc.REG_B)]
    calls += [lambda U=U: dev.fism_rounds(ptr, c['ev_i'], negs, rho, c['coef'], U, c['lr'], fc.REG_I, fc.REG_B) for U in (1, 5, 100)]
    for lds in (1, 0):
        dev.set_option('fism_lds', lds)
        try:
            for call in calls:
                with pytest.raises(YueHipError, match=r'draw %d \(event %d, user %d\) names its own event' % (t, e, u)) as err:
                    call()
                assert err.value.code == ERR_ARG
        finally:
            dev.set_option('fism_lds', 1)
    P, Q, Bi = np.empty_like(c['P0']), np.empty_like(c['Q0']), np.empty_like(c['B0'])
    dev.fism_get_model(P, Q, Bi)
    assert np.array_equal(P, c['P0']) and np.array_equal(Q, c['Q0']) and np.array_equal(Bi, c['B0'])


@pytest.mark.parametrize('name', ['grid_n', 'grid_nk'])
def test_grid_stride_loops_take_their_second_trip(dev, name):
    # k_fism_apply (1,024 x 256 threads) and k_fism_sumsq (256 x 256) on n k > 262,144 and, grid_n, n > 262,144: rows past the first
    # trip change, the sums cover them, and what no user touches stays as uploaded
    c = fc.build(name)
    for lds in (1, 0):
        got = run(dev, c, 4, lds, 1)
        half, (sp, sq, sb), P, Q, Bi, form = got
        d = distances(got, fc.oracle(name, 4))
        want = ((P * P).sum(), float((Q.astype(np.float64) ** 2).sum()), Bi.dot(Bi))
        ds = (abs(sp - want[0]) / want[0], abs(sq - want[1]) / want[1], abs(sb - want[2]) / want[2])
        print('%s rounds of 4 lds %d form %d: P %.3g Q %.3g Bi %.3g half %.3g; sums of squares P %.3g Q %.3g Bi %.3g' % ((name, lds, form) + d + ds))
        assert form == (c['form'][4] if lds else 0) and max(d) < 1e-6
        assert ds[0] < 1e-10 and ds[2] < 1e-10 and ds[1] < 1e-6
        idle = ~fc.touched(c)
        assert np.array_equal(P[idle], c['P0'][idle]) and np.array_equal(Q[idle], c['Q0'][idle]) and np.array_equal(Bi[idle], c['B0'][idle])
        beyond = np.zeros(c['n'] * c['k'], bool)
        beyond[262144:] = True
        assert ((Q != c['Q0']).ravel() & beyond).any() and ((P != c['P0']).ravel() & beyond).any()
        if c['n'] > 262144:
            assert (Bi != c['B0'])[262144:].any() and Bi[c['n'] - 1] != c['B0'][c['n'] - 1]


@pytest.mark.parametrize('N', [1, 10, 100])
def test_selection_on_equal_scores(dev, N):
    # identical item rows -> bit-equal scores in the seed's stable sort, at the last slot and inside the overwrite scan; 65 listed
    # users (a second block of k_fism_select), an empty row, an unsorted row with duplicates, exactly N and N - 1 candidates
    from oracle.numpy_fism import fism_scores, overwrite_scan
    P, Q, Bi, groups = fc.selection_model(N)
    rows = fc.selection_rows(N)
    dev.fism_set_model(P, Q, Bi)
    rp = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    ids, sc = dev.fism_topn_scan(rp, np.concatenate(rows), N)
    worst = 0.0
    for t, r in enumerate(rows):
        s = dev.fism_scores(r)
        so = fism_scores(P, Q, Bi, r)
        worst = max(worst, np.abs(s - so).max() / np.abs(so).max())
        for g in groups:
            assert len(set(s[g].tolist())) == 1, (t, g)
        want_ids, want_vals = overwrite_scan(s, r, N)
        assert ids[t].tolist() == want_ids, t
        assert sc[t].tolist() == want_vals, t
    print('N %d: 65 users, scores against the oracle %.3g' % (N, worst))
    assert worst < 1e-12
    assert len(set(rows[2].tolist())) == fc.SEL_N - N and not set(ids[2].tolist()) & set(rows[2].tolist())
    # one candidate fewer at position 40 of the call
    free = [x for x in range(fc.SEL_N) if x not in set(rows[2].tolist())]
    short = list(rows)
    short[40] = np.concatenate([rows[2], free[:1]]).astype(np.int32)
    rp = np.concatenate([[0], np.cumsum([len(r) for r in short])]).astype(np.int64)
    with pytest.raises(IndexError, match='user at position 40 has fewer than N candidates'):
        dev.fism_topn_scan(rp, np.concatenate(short), N)


@pytest.mark.parametrize('n,nu', [(128, 2), (64, 4), (257, 1), (256, 1)])
def test_scores_at_and_past_a_multiple_of_the_block(dev, n, nu):
    # k_fism_scores: nu n = 256 fills its last block exactly, 257 leaves one thread in a second block
    from oracle.numpy_fism import fism_scores
    rng = np.random.RandomState(n + nu)
    k = 20
    P, Q, Bi = rng.rand(n, k) / 10, (rng.rand(n, k) / 10).astype(np.float32), rng.rand(n) / 100
    dev.fism_set_model(P, Q, Bi)
    rows = [rng.randint(0, n, 5).astype(np.int32) for _ in range(nu)]
    if nu == 1:
        got = [dev.fism_scores(rows[0])]
        picks = [np.arange(n)]
    else:
        rp = np.arange(nu + 1, dtype=np.int64) * 5
        ids, sc = dev.fism_topn_scan(rp, np.concatenate(rows), 10)
        got, picks = list(sc), list(ids)
    for t in range(nu):
        so = fism_scores(P, Q, Bi, rows[t])
        d = np.abs(got[t] - so[picks[t]]).max() / np.abs(so).max()
        print('n %d nu %d user %d: %.3g' % (n, nu, t, d))
        assert d < 1e-12
    if nu == 1:
        assert got[0].shape == (n,) and np.isfinite(got[0]).all()


def test_refusals_change_nothing(dev):
    from yue_amd._shim import ERR_ARG, Device, YueHipError
    name = 'S9_k65'
    c = fc.build(name)
    ptr, ev_i, negs, rho, coef, n, k = c['user_ptr'], c['ev_i'], c['negs'], c['rho'], c['coef'], c['n'], c['k']
    dev.fism_set_model(c['P0'], c['Q0'], c['B0'])
    rng = np.random.RandomState(1)

    def refused(call, words=None):
        with pytest.raises(YueHipError, match=words) as err:
            call()
        assert err.value.code == ERR_ARG

    def both(ptr_=ptr, ev_=ev_i, negs_=negs, rho_=rho, U=4, words=None):
        refused(lambda: dev.fism_epoch(ptr_, ev_, negs_, rho_, coef, c['lr'], fc.REG_I, fc.REG_B), words)
        refused(lambda: dev.fism_rounds(ptr_, ev_, negs_, rho_, coef, U, c['lr'], fc.REG_I, fc.REG_B), words)

    refused(lambda: dev.fism_set_model(rng.rand(4, 257), rng.rand(4, 257).astype(np.float32), rng.rand(4)), 'yue_fism_set_model')
    refused(lambda: dev.fism_set_model(np.zeros((0, 8)), np.zeros((0, 8), np.float32), np.zeros(0)), 'yue_fism_set_model')
    assert (dev.fn, dev.fk) == (n, k)
    down = ptr.copy()
    down[3] = down[2] - 1
    both(ptr_=down, words='non-decreasing')
    far = ptr.copy()
    far[1] = 10 ** 6                                             # row 0 alone looks fine; its ids would lie far past ev_i
    both(ptr_=far, words='non-decreasing')
    for bad in (-1, n):
        ev = ev_i.copy()
        ev[3] = bad
        both(ev_=ev, words='item id out of range')
        ng = negs.copy()
        ng[len(ng) - 1] = bad
        both(negs_=ng, words='negative item id out of range')
    both(rho_=0, words='bad argument')
    both(negs_=negs[:-1], words='need rho negatives')
    refused(lambda: dev.fism_rounds(ptr, ev_i, negs, rho, coef, 0, c['lr'], fc.REG_I, fc.REG_B), 'bad argument')
    rp, items = np.array([0, 3], np.int64), np.array([1, 2, 3], np.int32)
    for N in (0, 101):
        refused(lambda: dev.fism_topn_scan(rp, items, N), 'N must be in 1..100')
    fresh = Device(0, raise_errors=True)
    try:
        for call in (lambda: fresh.fism_epoch(ptr, ev_i, negs, rho, coef, c['lr'], fc.REG_I, fc.REG_B),
                     lambda: fresh.fism_rounds(ptr, ev_i, negs, rho, coef, 4, c['lr'], fc.REG_I, fc.REG_B),
                     lambda: fresh.fism_scores(items), lambda: fresh.fism_topn_scan(rp, items, 1),
                     lambda: fresh.fism_get_model(np.empty((n, k)), np.empty((n, k), np.float32), np.empty(n))):
            with pytest.raises(YueHipError, match='no FISM model uploaded') as err:
                call()
            assert err.value.code == ERR_ARG
    finally:
        fresh.close()
    # nothing of all that reached the model ...
    P, Q, Bi = np.empty_like(c['P0']), np.empty_like(c['Q0']), np.empty_like(c['B0'])
    dev.fism_get_model(P, Q, Bi)
    assert np.array_equal(P, c['P0']) and np.array_equal(Q, c['Q0']) and np.array_equal(Bi, c['B0'])
    assert dev.fism_scores(items).shape == (n,)
    # ... and a valid call after them gives the oracle's result
    half, sp, sq, sb = dev.fism_rounds(ptr, ev_i, negs, rho, coef, 5, c['lr'], fc.REG_I, fc.REG_B)
    dev.fism_get_model(P, Q, Bi)
    d = distances((half, None, P, Q, Bi, None), fc.oracle(name, 5))
    print('after the refusals, rounds of 5 form %d: P %.3g Q %.3g Bi %.3g half %.3g' % ((dev.get_option('fism_last_form'),) + d))
    assert max(d) < 1e-6 and dev.get_option('fism_last_form') == 2
    # the last item, n - 1, is an event's item like any other (no draw names its own event's item: the case's events stay below 25)
    ev = ev_i.copy()
    ev[3] = n - 1
    assert ev_i.max() < n - 2
    ng = np.where(negs == n - 1, n - 2, negs).astype(np.int32)
    dev.fism_set_model(c['P0'], c['Q0'], c['B0'])
    assert np.isfinite(dev.fism_epoch(ptr, ev, ng, rho, coef, c['lr'], fc.REG_I, fc.REG_B)).all()
    assert np.isfinite(dev.fism_rounds(ptr, ev, ng, rho, coef, 4, c['lr'], fc.REG_I, fc.REG_B)).all()
