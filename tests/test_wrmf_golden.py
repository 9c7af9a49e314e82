"""CPU: the NumPy oracles of WRMF (tests/helpers/numpy_wrmf.py) against what the reference's own WRMF class computed
(tests/golden/g10_wrmf_*, tools/make_wrmf_goldens.py).

wrmf_reference_form restates the reference at its dtypes and reproduces it to fp64 round-off.  The device contract
(wrmf_half_sweep_contract: exact fp32-rounded Gram, fp64 Cholesky) cannot equal the reference bit for bit: the
reference's YtY / XtX is an fp32 BLAS product, whose summation order nobody reproduces.  The gap is that rounding
difference amplified by the conditioning of A, so each case carries its own bound: the figure measured when the
fixture was generated (the json's 'measured'), with margin.
"""
import numpy as np
import pytest

from helpers.numpy_wrmf import pairs_from_events, rows_of, wrmf_half_sweep_contract, wrmf_reference_form
from util import gj, gz, rel_err

# case: (bound on X and Y after every iteration, bound on the loss), contract vs reference
CASES = {
    'wrmf_c1_k20': (5e-6, 1e-7),              # measured 2.4e-6 / 8e-9: k = 20, regU = 1, well conditioned
    'wrmf_d3_k128': (5e-5, 1e-7),             # measured 2.5e-5 / 2e-8: k = 128 with only 120 users: XtX near rank 120
    'wrmf_d3_k128_reg001': (1e-3, 1e-5),      # measured 4.3e-4 / 2.2e-6: m < k, XtX singular, only reg = 0.01 conditions A
    'wrmf_z_k64': (2e-5, 1e-6),               # measured 7.0e-6 / 9e-8: test-only users and items (zero rows)
}


def load(tag):
    z = gz('g10_%s.npz' % tag)
    meta = gj('g10_%s.json' % tag)
    m, n = int(z['m']), int(z['n'])
    (up, ui, uc), (ip, iu, ic) = pairs_from_events(z['ev_u'], z['ev_i'], m, n)
    return z, meta, (up, ui, uc), (ip, iu, ic)


def printed_losses(meta):
    out = []
    for i, ln in enumerate(meta['lines'], 1):
        head, val = ln.split(' loss: ')
        assert head == 'iteration: %d' % i
        out.append(float(val))
    return out


@pytest.mark.parametrize('tag', sorted(CASES))
def test_reference_form_reproduces_the_reference(tag):
    z, meta, (up, ui, uc), (ip, iu, ic) = load(tag)
    iters, reg = int(z['iters']), float(z['reg'])
    X, Y, losses, Xs, Ys = wrmf_reference_form(z['X0'], z['Y0'], rows_of(up, ui, uc), rows_of(ip, iu, ic), iters, reg)
    assert X.dtype == np.float32 and Y.dtype == np.float32
    for t in range(iters):
        assert rel_err(Xs[t], z['Xs'][t]) < 1e-12 and rel_err(Ys[t], z['Ys'][t]) < 1e-12
    for a, b in zip(losses, printed_losses(meta)):
        assert abs(a - b) <= 1e-12 * abs(b)


@pytest.mark.parametrize('tag', sorted(CASES))
def test_contract_within_the_measured_bound(tag):
    z, meta, (up, ui, uc), (ip, iu, ic) = load(tag)
    iters, reg = int(z['iters']), float(z['reg'])
    bound, lbound = CASES[tag]
    assert meta['measured']['contract_vs_reference_X'] <= bound and meta['measured']['contract_vs_reference_loss'] <= lbound
    X, Y = z['X0'].copy(), z['Y0'].copy()
    for t, ref_loss in enumerate(printed_losses(meta)):
        X, loss = wrmf_half_sweep_contract(Y, up, ui, uc, reg, X_old=X)
        Y, _ = wrmf_half_sweep_contract(X, ip, iu, ic, reg)
        assert rel_err(X, z['Xs'][t]) <= bound and rel_err(Y, z['Ys'][t]) <= bound
        assert abs(loss - ref_loss) <= lbound * abs(ref_loss)
    # rows without training pairs: exactly zero in the reference and in the contract
    assert np.all(z['Xs'][-1][z['zero_users']] == 0) and np.all(X[z['zero_users']] == 0)
    assert np.all(z['Ys'][-1][z['zero_items']] == 0) and np.all(Y[z['zero_items']] == 0)


def test_zero_row_case_has_zero_rows():
    z = gz('g10_wrmf_z_k64.npz')
    assert len(z["zero_users"]) == 6 and len(z["zero_items"]) >= 4          # (+ items of d3 that only the test set holds)


def test_plugin_pairs_match_the_oracle_pairs():
    from yue_amd.recommender.cf.WRMF import wrmf_pairs
    z = gz('g10_wrmf_c1_k20.npz')
    m, n = int(z['m']), int(z['n'])
    order = np.argsort(z['ev_u'], kind='stable')
    ev_ptr = np.zeros(m + 1, np.int64)
    np.add.at(ev_ptr, z['ev_u'].astype(np.int64) + 1, 1)
    got = wrmf_pairs(np.cumsum(ev_ptr), z['ev_i'][order], n)
    want = pairs_from_events(z['ev_u'], z['ev_i'], m, n)
    for g, w in zip(got[0] + got[1], want[0] + want[1]):
        assert g.dtype == w.dtype and np.array_equal(g, w)
    assert got[0][2].sum() == len(z['ev_u'])              # counts add up to the events
