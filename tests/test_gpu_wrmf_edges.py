"""GPU: WRMF's kernels (k_wrmf_gram_part, k_wrmf_chunk, k_wrmf_solve, the shared als_tiles.hpp) at the
row lengths, chunk counts, factor widths and fixed-side sizes where their loops and guards change, which tests/test_gpu_wrmf.py
never reaches.  The cases are those of tests/helpers/wrmf_cases.py; tests/test_wrmf_cases.py shows on the CPU that each is well
conditioned (two fp64 solvers agree to 1e-9) and that a lost pair, a lost loss term and a lost or doubled Gram row move it by
more than ten times the bounds used here.

Yardstick: dev.wrmf_half_sweep against wrmf_half_sweep_contract from identical inputs, each half-sweep from the case's X0 and Y0.
Per row rel_err <= 1e-6; the loss within 1e-6 relative, exactly 0.0 where the contract's is 0; rows without pairs exactly 0; the
fixed side unchanged bit for bit; wrmf_long_rows_user / _item equal to the number of rows longer than the threshold.
"""
import numpy as np
import pytest

from helpers import wrmf_cases as wc
from helpers.numpy_wrmf import wrmf_half_sweep_contract
from util import rel_err

pytestmark = pytest.mark.gpu

BOUND = 1e-6
PIVOT = 'yue_wrmf_half_sweep: non-positive pivot in the Cholesky factorisation of %s row %d '


@pytest.fixture(scope='module')
def dev():
    from yue_amd._shim import Device
    d = Device(0, raise_errors=True)
    yield d
    d.close()


_REF = {}


def reference(case, side):
    """The contract's (rows, loss) of one half-sweep of a case, computed once."""
    key = (case.name, side)
    if key not in _REF:
        F, X_old, ptr, idx, cnt = wc.side_of(case, side)
        _REF[key] = wrmf_half_sweep_contract(F, ptr, idx, cnt, case.reg, X_old=X_old, alpha=case.alpha)
    return _REF[key]


def upload(d, case):
    """Call with wrmf_long_pairs restored by the caller."""
    d.set_option('wrmf_long_pairs', case.long_pairs)
    d.set_factors(case.X0, case.Y0)
    d.wrmf_set_pairs(*(case.um + case.im))
    for name, ptr in (('wrmf_long_rows_user', case.um[0]), ('wrmf_long_rows_item', case.im[0])):
        assert d.get_option(name) == int((np.diff(ptr) > case.long_pairs).sum()), (case.name, name)


def half_sweep(d, case, side, reg=None):
    """One half-sweep from X0, Y0 (the pairs are up): (the solved side, the fixed side, the loss)."""
    d.set_factors(case.X0, case.Y0)
    loss = d.wrmf_half_sweep(side, case.alpha, case.reg if reg is None else reg)
    X, Y = d.get_factors()
    return (X, Y, loss) if side == 0 else (Y, X, loss)


def against_contract(case, side, got):
    S, F, loss = got
    So, loss_o = reference(case, side)
    F0, _, ptr = wc.side_of(case, side)[:3]
    assert np.array_equal(F, F0), (case.name, side)
    lens = np.diff(ptr)
    worst = 0.0
    for r in range(len(lens)):
        if lens[r] == 0:
            assert not S[r].any() and not So[r].any(), (case.name, side, r)
        else:
            assert np.isfinite(S[r]).all()
            err = rel_err(S[r], So[r])
            worst = max(worst, err)
            assert err <= BOUND, (case.name, side, r, int(lens[r]), err)
    if side == 0:
        print(case.name, 'side', side, 'worst row', worst, 'loss', loss, loss_o, 'bit-equal rows', bool(np.array_equal(S, So)))
        assert loss == 0.0 if loss_o == 0.0 else abs(loss - loss_o) <= BOUND * loss_o, (case.name, loss, loss_o)
    else:
        print(case.name, 'side', side, 'worst row', worst, 'bit-equal rows', bool(np.array_equal(S, So)))
        assert loss == 0.0


def check(d, case):
    try:
        upload(d, case)
        for side in case.sides:
            against_contract(case, side, half_sweep(d, case, side))
    finally:
        d.set_option('wrmf_long_pairs', wc.DEFAULT_LONG)


# ---- one test per family ----
@pytest.mark.parametrize('side,k', wc.ROWLEN)
def test_row_lengths_at_the_stage_edges(dev, side, k):
    case = wc.rowlen_case(side, k)
    assert case.long_pairs == wc.DEFAULT_LONG                           # 0 .. 97 pairs, all summed inside k_wrmf_solve
    check(dev, case)


@pytest.mark.parametrize('side,k,L', wc.CHUNKS)
def test_rows_at_the_chunk_edges(dev, side, k, L):
    case = wc.chunks_case(side, k, L)
    lens = np.diff(wc.side_of(case, side)[2])
    assert {L - 1, L, L + 1, 2 * L - 1, 2 * L, 2 * L + 1, 3 * L + 7} <= set(lens.tolist())
    assert (lens > L).sum() == 5                                        # upload() holds the library to that count; L itself is not long
    check(dev, case)


@pytest.mark.parametrize('side,k', wc.ALL_LONG)
def test_every_row_with_pairs_is_long(dev, side, k):
    case = wc.all_long_case(side, k)
    lens = np.diff(wc.side_of(case, side)[2])
    assert (lens[lens > 0] > case.long_pairs).all() and (lens == 0).sum() == 2
    check(dev, case)


@pytest.mark.parametrize('k,reg', wc.WIDTHS)
def test_factor_widths_at_the_tile_slot_edges(dev, k, reg):
    case = wc.widths_case(k, reg)
    assert case.sides == (0, 1) and case.long_pairs == 32
    check(dev, case)


@pytest.mark.parametrize('side', [0, 1])
@pytest.mark.parametrize('alpha', wc.GRAM_ALPHAS)
@pytest.mark.parametrize('nf,k', wc.GRAM)
def test_gram_at_the_block_and_stage_edges(dev, nf, k, alpha, side):
    case = wc.gram_case(nf, k, alpha, side)
    assert len(wc.side_of(case, side)[0]) == nf and case.alpha == alpha
    check(dev, case)


@pytest.mark.parametrize('name', list(wc.TINY))
def test_tiny(dev, name):
    case = wc.TINY[name]()
    check(dev, case)
    if name == 'no_pairs':                                              # the rows start non-zero and are written as zeros
        assert case.X0.all() and case.Y0.all() and reference(case, 0)[1] == 0.0


# ---- rows depend on their own pairs only ----
@pytest.mark.parametrize('side', [0, 1])
def test_relabelled_rows_are_bit_identical(dev, side):
    case = wc.chunks_case(side, 20, 32)
    other, perm = wc.relabelled(case, side)
    assert not np.array_equal(perm, np.arange(len(perm)))
    lens = np.diff(wc.side_of(case, side)[2])
    assert len(set(lens.tolist())) == len(lens)                         # distinct lengths: the schedule, and so the loss's order, is the same
    try:
        upload(dev, case)
        S, _, loss = half_sweep(dev, case, side)
        upload(dev, other)
        Sp, _, loss_p = half_sweep(dev, other, side)
    finally:
        dev.set_option('wrmf_long_pairs', wc.DEFAULT_LONG)
    against_contract(case, side, (S, wc.side_of(case, side)[0], loss))
    for r in range(len(perm)):
        assert np.array_equal(Sp[perm[r]], S[r]), (r, int(perm[r]), int(lens[r]))
    assert loss_p == loss


# ---- buffers kept between uploads ----
@pytest.mark.parametrize('side', [0, 1])
def test_a_used_context_equals_a_fresh_one(dev, side):
    from yue_amd._shim import Device
    big = wc.chunks_case(side, *wc.LARGEST_CHUNKS[1:])
    small = wc.rowlen_case(side, 20)
    assert big.um[0][-1] > small.um[0][-1] and max(big.m, big.n) > max(small.m, small.n)
    fresh = Device(0, raise_errors=True)
    try:
        upload(fresh, small)
        want = half_sweep(fresh, small, side)
    finally:
        fresh.close()
    try:
        upload(dev, big)
        first = half_sweep(dev, big, side)
        upload(dev, small)
        second = half_sweep(dev, small, side)
        upload(dev, big)
        third = half_sweep(dev, big, side)
    finally:
        dev.set_option('wrmf_long_pairs', wc.DEFAULT_LONG)
    against_contract(big, side, first)
    against_contract(small, side, want)
    assert np.array_equal(second[0], want[0]) and np.array_equal(second[1], want[1]) and second[2] == want[2]
    assert np.array_equal(third[0], first[0]) and np.array_equal(third[1], first[1]) and third[2] == first[2]


# ---- refusals ----
@pytest.mark.parametrize('side,k,column', wc.REFUSALS)
def test_zero_column_is_refused_and_names_the_first_row_with_pairs(dev, side, k, column):
    from yue_amd._shim import YueHipError
    case = wc.refusal_case(side, k, column)
    _, S0, ptr = wc.side_of(case, side)[:3]
    assert list(np.diff(ptr)[:3]) == [0, 0, 3] and S0[:2].all()         # rows 0 and 1 return before the factorisation
    try:
        upload(dev, case)
        with pytest.raises(YueHipError, match=PIVOT % ('user' if side == 0 else 'item', 2)):
            half_sweep(dev, case, side, reg=0.0)
        X, Y = dev.get_factors()
        S = X if side == 0 else Y
        assert not S[:2].any()                                          # rows without pairs are written all the same
        assert np.array_equal(S[2:], S0[2:])                            # a refused row is not written
        against_contract(case, side, half_sweep(dev, case, side))       # reg = 1.0: the context stays usable
    finally:
        dev.set_option('wrmf_long_pairs', wc.DEFAULT_LONG)


def test_nan_in_the_fixed_side_is_refused_as_a_pivot(dev):
    """yue_set_factors does not look at the values, so a NaN reaches the Gram; every A then has a NaN row and column, and
    !(piv > 0.0) refuses at that column.  No row with pairs is written."""
    from yue_amd._shim import YueHipError
    case = wc.rowlen_case(0, 20)
    Y = case.Y0.copy()
    Y[5, 7] = np.nan
    bad = case._replace(Y0=Y, name=case.name + '_nan')
    assert np.diff(bad.um[0])[0] == 0 and np.diff(bad.um[0])[1] == 1
    try:
        upload(dev, bad)                                                # accepted
        with pytest.raises(YueHipError, match=PIVOT % ('user', 1)):
            half_sweep(dev, bad, 0)
        X, Yd = dev.get_factors()
        assert not X[0].any() and np.array_equal(X[1:], bad.X0[1:]) and np.isfinite(X).all()
        assert np.array_equal(Yd, Y, equal_nan=True)
        against_contract(case, 0, half_sweep(dev, case, 0))             # the pairs are up; clean factors: usable
    finally:
        dev.set_option('wrmf_long_pairs', wc.DEFAULT_LONG)


def test_a_changed_shape_is_refused_until_the_pairs_are_uploaded_again(dev):
    from yue_amd._shim import YueHipError
    case = wc.rowlen_case(0, 20)
    rng = np.random.RandomState(1)
    try:
        upload(dev, case)
        for m, n in ((case.m + 1, case.n), (case.m, case.n - 1)):
            dev.set_factors(rng.rand(m, case.k).astype(np.float32), rng.rand(n, case.k).astype(np.float32))
            for side in (0, 1):
                with pytest.raises(YueHipError, match="yue_wrmf_half_sweep: the factors' shape changed since yue_wrmf_set_pairs"):
                    dev.wrmf_half_sweep(side, case.alpha, case.reg)
        against_contract(case, 0, half_sweep(dev, case, 0))             # the old shape again: the uploaded pairs hold
    finally:
        dev.set_option('wrmf_long_pairs', wc.DEFAULT_LONG)
