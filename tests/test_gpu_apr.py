"""GPU: APR's device path (yue_apr_*) through the shim on problems with explicit triplets
(tests/helpers/apr_cases.py), against the fp64 contract tests/helpers/numpy_apr.py.
Bounds: the two losses, the parameter gradients of both forms, the raw perturbation gradients and the new perturbation within 4 x the
case's d32 (the float32 contract's own distance from fp64) in relative max-norm, with a floor of L 2^-24 (L: the quantity's longest
sum).  Steps: three phase-1 steps, then three adversarial ones, against the contract's float32 Adam fed the device's own gradients:
factors bit-equal, moments within 1e-6.  A second run of every call identical in every bit.  tests/test_apr_golden.py asserts on the
CPU that every case meets its conditioning statement."""
import numpy as np
import pytest

from helpers import apr_cases as ac
from helpers import numpy_apr as ap

pytestmark = pytest.mark.gpu

LR = 0.002


@pytest.fixture(scope='module')
def dev():
    from yue_amd._shim import Device
    d = Device(0, raise_errors=True)
    yield d
    d.close()


def upload(dev, c):
    dev.set_factors(c['U'], c['V'])
    dev.adam_reset()
    dev.apr_set_delta(c['ids_u'], c['rows_u'], c['ids_i'], c['rows_v'])


def outputs(dev, u, i, j, eps, regA):
    """Every QUANTITY at the standing perturbation, in apr_cases.QUANTITIES' order; the update comes last and replaces it."""
    lp, gUp, gVp = dev.apr_grad(False, u, i, j, ac.REG)
    la, gUa, gVa = dev.apr_grad(True, u, i, j, regA)
    rU, rV = dev.apr_delta_update(u, i, j, eps, regA)
    dU, dV = dev.apr_get_delta()
    return dict(zip(ac.QUANTITIES, (lp, gUp, gVp, la, gUa, gVa, rU, rV, dU, dV)))


def distance(got, want, q):
    return abs(got[q] - want[q]) / abs(want[q]) if q.startswith('loss') else ap.rel(got[q], want[q])


def hold(name, got, want, d32, L):
    """Prints each figure with its multiple of d32, then asserts each bound."""
    dist = {q: distance(got, want, q) for q in ac.QUANTITIES}
    print(name, ' '.join('%s %.3g (d32 %.3g, x%.2f)' % (q, dist[q], d32[q], dist[q] / d32[q] if d32[q] else 0.0) for q in ac.QUANTITIES))
    for q in ac.QUANTITIES:
        assert np.isfinite(got[q]).all(), q
        assert dist[q] <= ac.bound(d32, L, q), (q, dist[q], d32[q], ac.bound(d32, L, q))


def check_case(dev, c):
    upload(dev, c)
    got = outputs(dev, c['u'], c['i'], c['j'], c['eps'], c['regA'])
    hold(c['name'], got, c['want'], c['d32'], c['L'])
    # the whole-variable assign: outside the batch's rows the new perturbation is exactly zero, also where the old one was not
    outside_u, outside_i = np.setdiff1d(np.arange(c['m']), c['u']), np.setdiff1d(np.arange(c['n']), np.concatenate([c['i'], c['j']]))
    assert not got['dU'][outside_u].any() and not got['dV'][outside_i].any()
    assert not got['rawU'][outside_u].any() and not got['rawV'][outside_i].any()
    return got


@pytest.mark.parametrize('name', ac.GPU_CASES)
def test_losses_gradients_and_the_perturbation_update(dev, name):
    c = ac.build(name)
    got = check_case(dev, c)
    assert c['dU'][0].any() and not got['dU'][0].any()           # user 0 held a perturbation and is in no batch
    assert all(t > 0 for t in dev.apr_times()[:3:2])             # the update ran the coefficient and the perturbation-row phases


def nonzero_rows(D):
    ids = np.flatnonzero(D.any(axis=1)).astype(np.int32)
    return ids, D[ids]


def check_steps(dev, c, log=None):
    """Three phase-1 steps, then three adversarial ones.  The contract's float32 Adam is fed the device's own gradients: before a
    phase-2 step the update is run once for its result, the gradient is taken at it, and the perturbation is put back."""
    upload(dev, c)
    dev.apr_reset()
    U, V = c['U'].copy(), c['V'].copy()
    st = ap.new_state(U, V)
    batches = ac.step_batches(c)
    u0, i0, j0 = batches[0]
    only_first = (int(u0[4]), int(i0[4]))
    moved = []
    for t, (u, i, j) in enumerate(batches, 1):
        if t <= 3:
            loss_g, gU, gV = dev.apr_grad(False, u, i, j, ac.REG)
            loss = dev.apr_pre_step(u, i, j, LR, ac.REG, t)
        else:
            before = dev.apr_get_delta()
            dev.apr_delta_update(u, i, j, c['eps'], c['regA'])
            loss_g, gU, gV = dev.apr_grad(True, u, i, j, c['regA'])
            after = dev.apr_get_delta()
            dev.apr_set_delta(*(nonzero_rows(before[0]) + nonzero_rows(before[1])))
            loss = dev.apr_adv_step(u, i, j, LR, c['eps'], c['regA'], t)
            now = dev.apr_get_delta()
            assert np.array_equal(now[0], after[0]) and np.array_equal(now[1], after[1])
            assert not gU[only_first[0]].any() and not gV[only_first[1]].any()
        assert loss == loss_g
        P_before = U.copy()
        ap.adam(U, gU, st['mU'], st['vU'], LR, t, np.float32)
        ap.adam(V, gV, st['mV'], st['vV'], LR, t, np.float32)
        P, Q = dev.get_factors()
        mU, vU, mV, vV = dev.adam_get_moments()
        worst = max(ap.rel(mU, st['mU']), ap.rel(vU, st['vU']), ap.rel(mV, st['mV']), ap.rel(vV, st['vV']))
        print(c['name'], 'step', t, 'loss %.6f' % loss, 'factors equal', np.array_equal(P, U) and np.array_equal(Q, V), 'moments %.3g' % worst)
        assert np.array_equal(P, U) and np.array_equal(Q, V)
        assert worst <= 1e-6
        if t > 3:
            moved.append(bool((P[only_first[0]] != P_before[only_first[0]]).any()))
        if log is not None:
            log += [np.float64(loss), gU, gV, P, Q, mU, vU, mV, vV]
        # the contract goes on from the device's state, so that a step's check does not inherit the last one's rounding
        U, V = P.copy(), Q.copy()
        st = {'mU': mU.copy(), 'vU': vU.copy(), 'mV': mV.copy(), 'vV': vV.copy()}
    # Adam is dense and its moments run on from phase 1: a row of phase 1's batches that no phase-2 batch holds (zero gradient)
    # still moves in every phase-2 step
    assert moved == [True, True, True]
    assert all(t > 0 for t in dev.apr_times())


@pytest.mark.parametrize('name', ac.STEP_CASES)
def test_steps_are_the_contracts_adam_on_the_devices_gradients(dev, name):
    check_steps(dev, ac.build(name))


@pytest.mark.parametrize('name', ['k64', 'k129'])
def test_repeat_runs_are_bit_identical(dev, name):
    c = ac.build(name)
    runs = []
    for _ in range(2):
        upload(dev, c)
        got = outputs(dev, c['u'], c['i'], c['j'], c['eps'], c['regA'])
        log = [np.asarray(got[q]) for q in ac.QUANTITIES]
        check_steps(dev, c, log)
        runs.append(log + list(dev.apr_get_delta()))
    assert len(runs[0]) == len(runs[1])
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


def test_refusals(dev):
    from yue_amd._shim import ERR_ARG, Device, YueHipError
    c = ac.build('base')
    upload(dev, c)
    u, i, j = c['u'], c['i'], c['j']

    def refused(f, *a):
        with pytest.raises(YueHipError) as e:
            f(*a)
        assert e.value.code == ERR_ARG, e.value
        return str(e.value)
    for pos, (who, bound) in enumerate((('user', c['m']), ('positive item', c['n']), ('negative item', c['n']))):
        for bad_id in (bound, -1):
            ids = [u.copy(), i.copy(), j.copy()]
            ids[pos][6] = bad_id
            assert 'yue_apr_grad: %s id out of range (position 6)' % who in refused(dev.apr_grad, False, *ids, ac.REG)
            assert 'yue_apr_pre_step: %s id out of range (position 6)' % who in refused(dev.apr_pre_step, *ids, LR, ac.REG, 1)
            assert 'yue_apr_adv_step: %s id out of range (position 6)' % who in refused(dev.apr_adv_step, *ids, LR, 0.5, 1.0, 1)
            assert 'yue_apr_delta_update: %s id out of range (position 6)' % who in refused(dev.apr_delta_update, *ids, 0.5, 1.0)
    assert 'T < 2^29' in refused(dev.apr_pre_step, u[:0], i[:0], j[:0], LR, ac.REG, 1)          # T >= 1
    assert 'T < 2^29' in refused(dev.apr_adv_step, u[:0], i[:0], j[:0], LR, 0.5, 1.0, 1)
    assert 'step >= 1' in refused(dev.apr_pre_step, u, i, j, LR, ac.REG, 0)
    assert 'step >= 1' in refused(dev.apr_adv_step, u, i, j, LR, 0.5, 1.0, 0)
    assert 'eps >= 0' in refused(dev.apr_adv_step, u, i, j, LR, -0.5, 1.0, 1)
    assert 'regA >= 0' in refused(dev.apr_adv_step, u, i, j, LR, 0.5, -1.0, 1)
    assert 'eps >= 0' in refused(dev.apr_delta_update, u, i, j, -0.5, 1.0)
    assert 'eps >= 0' in refused(dev.apr_delta_update, u, i, j, float('nan'), 1.0)
    assert 'regA >= 0' in refused(dev.apr_delta_update, u, i, j, 0.5, -1.0)
    refused(dev.apr_grad, True, u, i, j, -1.0)
    refused(dev.apr_pre_step, u, i, j, LR, -1.0, 1)
    k = c['k']
    row = np.ones((2, k), np.float32)
    assert 'yue_apr_set_delta: user rows must be sorted and unique (row 0)' in refused(dev.apr_set_delta, [3, 3], row, [], [])
    assert 'yue_apr_set_delta: item id out of range (row 0)' in refused(dev.apr_set_delta, [], [], [1, c['n']], row)
    refused(dev.apr_set_delta, [1, 2], row * np.nan, [], [])
    # after the refusals the good state still answers, and nothing moved
    got = outputs(dev, u, i, j, c['eps'], c['regA'])
    hold('after refusals', got, c['want'], c['d32'], c['L'])
    P, Q = dev.get_factors()
    assert np.array_equal(P, c['U']) and np.array_equal(Q, c['V'])
    fresh = Device(0, raise_errors=True)
    try:
        fresh.m, fresh.n, fresh.k = c['m'], c['n'], c['k']
        for f, a in ((fresh.apr_reset, ()), (fresh.apr_get_delta, ()), (fresh.apr_grad, (False, u, i, j, ac.REG)), (fresh.apr_pre_step, (u, i, j, LR, ac.REG, 1)),
                     (fresh.apr_adv_step, (u, i, j, LR, 0.5, 1.0, 1)), (fresh.apr_delta_update, (u, i, j, 0.5, 1.0)),
                     (fresh.apr_set_delta, ([1], row[:1], [], []))):
            assert 'no factors uploaded' in refused(f, *a)
    finally:
        fresh.close()
