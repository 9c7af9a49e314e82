"""CPU: the cases of tests/helpers/wrmf_cases.py can tell a wrong WRMF kernel from a right one.

tests/test_gpu_wrmf_edges.py compares the device with wrmf_half_sweep_contract per row at 1e-6 and the loss at 1e-6 relative (the
device contract of DESIGN.md).  That comparison means something only if (a) every row's system is so well conditioned that two
correct fp64 solvers agree far below 1e-6, and (b) the slips a kernel can make at the edges the cases are built for move the
compared quantity far above it.  Both are checked here on the reference alone:

conditioning  per case and non-empty row, the contract's Cholesky solution against np.linalg.solve in fp64: <= 1e-9 relative.
mutants       the contract with one slip must differ from the contract by >= MARGIN x BOUND in the quantity the GPU test compares:
              the last pair of a row left out of A and b (that row), the last pair's loss term left out (the loss), one row of the
              fixed side left out of the Gram or counted twice (the worst row of the case; every row shares the Gram).
A case that misses either is rebuilt from other inputs; neither figure is loosened.  The smallest distance per family is printed.
"""
import numpy as np
import pytest

from helpers import wrmf_cases as wc
from helpers.numpy_wrmf import gram_fp32, wrmf_half_sweep_contract
from util import rel_err

BOUND = 1e-6                     # the GPU test's bound on a row and, relative, on the loss
MARGIN = 10.0
CONDITIONING = 1e-9

FAMILIES = wc.families()


def sweeps(family):
    return [(case, side) for case in FAMILIES[family] for side in case.sides]


def contract(case, side, **kw):
    F, X_old, ptr, idx, cnt = wc.side_of(case, side)
    return wrmf_half_sweep_contract(F, ptr, idx, cnt, case.reg, X_old=X_old, alpha=case.alpha, **kw)


def row_errors(X, Xo):
    return np.array([rel_err(X[r], Xo[r]) if np.abs(Xo[r]).max() > 0 else float(np.abs(X[r]).max() > 0) for r in range(len(Xo))])


def test_case_sizes():
    names = [case.name for cases in FAMILIES.values() for case in cases]
    assert len(set(names)) == len(names)
    for family, cases in FAMILIES.items():
        for case in cases:
            nnz = int(case.um[0][-1])
            assert nnz < 10000 and nnz == int(case.im[0][-1]), case.name     # one lost loss term stays above 1e-4 of the total
            assert min(case.m, case.n) <= 120 or family == 'GRAM', case.name
            counts = case.um[2]
            assert nnz == 0 or (counts.min() >= 1 and (np.sort(counts)[:-1] <= 4).all() and counts.max() in (1000, 3)), case.name
            assert case.X0.dtype == np.float32 and case.Y0.dtype == np.float32


@pytest.mark.parametrize('family', list(FAMILIES))
def test_every_row_is_well_conditioned(family):
    worst = 0.0
    for case, side in sweeps(family):
        F, _, ptr, idx, cnt = wc.side_of(case, side)
        G = gram_fp32(F)
        Xo, _ = contract(case, side, G=G)
        for r in range(len(ptr) - 1):
            a, b = int(ptr[r]), int(ptr[r + 1])
            if a == b:
                assert not Xo[r].any()
                continue
            Fr = F[idx[a:b]].astype(np.float64)                      # the contract's statements
            c = case.alpha * cnt[a:b].astype(np.float64)
            A = G + (Fr.T * c) @ Fr + case.reg * np.eye(case.k)
            rhs = ((1.0 + c)[:, None] * Fr).sum(0)
            L = np.linalg.cholesky(A)
            x = np.linalg.solve(L.T, np.linalg.solve(L, rhs))
            assert np.array_equal(x.astype(np.float32), Xo[r]), (case.name, side, r)
            other = np.linalg.solve(A, rhs)
            err = float(np.abs(x - other).max() / np.abs(other).max())
            worst = max(worst, err)
            assert err <= CONDITIONING, (case.name, side, r, err)
    print('%s: Cholesky against numpy.linalg.solve, worst row %.2e' % (family, worst))


@pytest.mark.parametrize('family', ['ROWLEN', 'CHUNKS'])
def test_a_lost_pair_moves_its_row(family):
    least = (np.inf, None)
    for case, side in sweeps(family):
        F, X_old, ptr, idx, cnt = wc.side_of(case, side)
        G = gram_fp32(F)
        Xo, _ = contract(case, side, G=G)
        for r in np.flatnonzero(np.diff(ptr) >= 2):
            a, b = int(ptr[r]), int(ptr[r + 1]) - 1                   # without the row's last pair
            Xm, _ = wrmf_half_sweep_contract(F, np.array([0, b - a]), idx[a:b], cnt[a:b], case.reg, alpha=case.alpha, G=G)
            d = rel_err(Xm[0], Xo[r])
            least = min(least, (d, (case.name, side, int(r))))
            assert d >= MARGIN * BOUND, (case.name, side, r, d)
    print('%s: a lost pair moves its row by at least %.2e (%s)' % ((family,) + least))


@pytest.mark.parametrize('family', ['ROWLEN', 'CHUNKS'])
def test_a_lost_loss_term_moves_the_loss(family):
    least = (np.inf, None)
    for case, side in sweeps(family):
        if side != 0:                                                 # the loss is the user half-sweep's
            continue
        F, X_old, ptr, idx, cnt = wc.side_of(case, side)
        _, loss_o = contract(case, side)
        for r in np.flatnonzero(np.diff(ptr) >= 2):
            d = np.float32(F[idx[ptr[r + 1] - 1]].astype(np.float64) @ X_old[r].astype(np.float64))
            moved = (1.0 - float(d)) ** 2 / loss_o
            least = min(least, (moved, (case.name, int(r))))
            assert moved >= MARGIN * BOUND, (case.name, r, moved)
    print('%s: a lost loss term moves the loss by at least %.2e relative (%s)' % ((family,) + least))


@pytest.mark.parametrize('sign,what', [(-1.0, 'lost'), (1.0, 'doubled')])
def test_a_lost_or_doubled_gram_row_moves_a_row(sign, what):
    least = (np.inf, None)
    for case, side in sweeps('GRAM'):
        F = wc.side_of(case, side)[0]
        nf = len(F)
        F64 = F.astype(np.float64)
        G64 = F64.T @ F64
        Xo, _ = contract(case, side, G=G64.astype(np.float32).astype(np.float64))
        assert np.array_equal(Xo, contract(case, side)[0])
        for q in wc.gram_rows(nf):
            Gm = (G64 + sign * np.outer(F64[q], F64[q])).astype(np.float32).astype(np.float64)
            Xm, _ = contract(case, side, G=Gm)
            d = float(row_errors(Xm, Xo).max())
            least = min(least, (d, (case.name, q)))
            assert d >= MARGIN * BOUND, (case.name, side, q, what, d)
    print('GRAM: a %s row of the fixed side moves the worst row by at least %.2e (%s)' % ((what,) + least))


def test_gram_rows_are_the_loop_bounds():
    assert [wc.rows_per_block(nf) for nf in wc.GRAM_NF] == [1, 1, 1, 1, 2, 32, 33, 33, 33]
    assert wc.last_stage_first_row(16385) == 16368 and wc.last_stage_first_row(16416) == 16401       # last blocks of 17 and 15 rows
    assert wc.last_stage_first_row(16896) == 16895 and wc.last_stage_first_row(16384) == 16352       # a stage of one row; of 32
    assert wc.last_stage_first_row(513) == 512 and wc.last_stage_first_row(1) == 0
    assert wc.gram_rows(16385) == [0, 31, 32, 33, 16368, 16384] and wc.gram_rows(1) == [0] and wc.gram_rows(2) == [0, 1]


@pytest.mark.parametrize('params', wc.REFUSALS)
def test_refusal_cases_are_singular_at_reg_0_and_only_there(params):
    side, k, column = params
    case = wc.refusal_case(*params)
    F, X_old, ptr, idx, cnt = wc.side_of(case, side)
    assert not F[:, column].any() and list(np.diff(ptr)[:3]) == [0, 0, 3] and case.reg == 1.0
    G = gram_fp32(F)
    lead = np.delete(np.delete(G, column, 0), column, 1)
    assert np.linalg.eigvalsh(lead).min() > 1e-2                      # every pivot before the zero column is positive
    with pytest.raises(np.linalg.LinAlgError):
        wrmf_half_sweep_contract(F, ptr, idx, cnt, 0.0, alpha=case.alpha, G=G)
