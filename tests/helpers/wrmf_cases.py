"""Named, seeded WRMF problems at the edges of the kernels (yue_amd/csrc/wrmf_kernels.hpp, als_tiles.hpp):
stage and chunk counts of a row, the factor widths where a thread gains a tile slot, the Gram's block and stage bounds.

tests/test_wrmf_cases.py checks on the CPU that every case is well conditioned and that one lost pair, one lost loss term and one
lost or doubled Gram row move a case by at least ten times the bound of tests/test_gpu_wrmf_edges.py, which runs the cases.

A case is a Case tuple: m, n, k, X0, Y0, um = (u_ptr, u_items, u_counts), im = (i_ptr, i_users, i_counts), alpha, reg,
long_pairs (the value of the option wrmf_long_pairs), then its name and the half-sweeps it is made for (0: user rows, 1: item
rows).  Factors are rng.rand fp32; counts are 1..4, one pair per case at 1000.  Every half-sweep starts from X0 and Y0.
"""
import collections
import functools

import numpy as np

STAGE = 32                       # kWrmfStage: gathered rows per LDS stage
GRAM_BLOCKS = 512                # kWrmfGramBlocks
DEFAULT_LONG = 2048

Case = collections.namedtuple('Case', 'm n k X0 Y0 um im alpha reg long_pairs name sides')


def pairs_from_matrix(R):
    """(u_ptr, u_items, u_counts), (i_ptr, i_users, i_counts) of a dense m x n matrix of event counts."""
    R = np.asarray(R, np.int64)
    m, n = R.shape
    u, i = np.nonzero(R)                                                # users ascending, items ascending within a user
    cnt = R[u, i].astype(np.int32)
    u_ptr = np.concatenate([[0], np.cumsum(np.bincount(u, minlength=m))]).astype(np.int64)
    i_ptr = np.concatenate([[0], np.cumsum(np.bincount(i, minlength=n))]).astype(np.int64)
    order = np.argsort(i, kind='stable')                                # users ascending within an item
    return (u_ptr, i.astype(np.int32), cnt), (i_ptr, u[order].astype(np.int32), cnt[order])


def side_of(case, side):
    """(F, X_old, ptr, idx, cnt) of a half-sweep: the fixed side, the solved side before the sweep and its pairs."""
    return (case.Y0, case.X0) + tuple(case.um) if side == 0 else (case.X0, case.Y0) + tuple(case.im)


def rows_matrix(rng, lengths, nf, first=None):
    """len(lengths) x nf event counts: row r names lengths[r] distinct columns, those of first[r] before random others;
    counts 1..4, and 1000 for the middle pair of the longest row."""
    R = np.zeros((len(lengths), nf), np.int64)
    for r, length in enumerate(lengths):
        assert length <= nf
        lead = [] if first is None else list(first[r])[:length]
        rest = np.setdiff1d(np.arange(nf), lead)
        ids = np.concatenate([np.asarray(lead, np.int64), rng.choice(rest, length - len(lead), replace=False)])
        R[r, ids] = rng.randint(1, 5, length)
    longest = int(np.argmax(lengths))
    cols = np.flatnonzero(R[longest])
    R[longest, cols[len(cols) // 2]] = 1000
    return R


def make(name, R, k, seed, sides, alpha=10.0, reg=1.0, long_pairs=DEFAULT_LONG):
    R = np.asarray(R, np.int64)
    m, n = R.shape
    rng = np.random.RandomState(seed)
    X0 = rng.rand(m, k).astype(np.float32)
    Y0 = rng.rand(n, k).astype(np.float32)
    um, im = pairs_from_matrix(R)
    return Case(m, n, k, X0, Y0, um, im, alpha, reg, long_pairs, name, tuple(sides))


def solved_rows(name, lengths, nf, k, seed, side, first=None, **kw):
    """The rows of `lengths` on the solved side of half-sweep `side`, nf rows on the fixed side."""
    R = rows_matrix(np.random.RandomState(seed), lengths, nf, first)
    case = make(name, R if side == 0 else R.T, k, seed + 1, (side,), **kw)
    assert list(np.diff(side_of(case, side)[2])) == list(lengths)
    return case


# ---- ROWLEN: 0, 1 and 2 pairs, then one below, at and one above 1, 2 and 3 full stages; all in k_wrmf_solve itself ----
ROWLEN_LENGTHS = (0, 1, 2, 31, 32, 33, 63, 64, 65, 95, 96, 97)
ROWLEN = [(side, k) for side in (0, 1) for k in (20, 65)]


@functools.lru_cache(None)
def rowlen_case(side, k):
    return solved_rows('rowlen_s%d_k%d' % (side, k), ROWLEN_LENGTHS, 110, k, 1000 + 10 * k + side, side)


# ---- CHUNKS: rows around 1, 2 and 3 chunks of L pairs; rows of L - 1 and L stay in k_wrmf_solve ----
def chunk_lengths(L):
    return (L - 1, L, L + 1, 2 * L - 1, 2 * L, 2 * L + 1, 3 * L + 7, 0, 1, 5, 33 if L > 33 else 9)


@functools.lru_cache(None)
def chunks_case(side, k, L):
    return solved_rows('chunks_s%d_k%d_L%d' % (side, k, L), chunk_lengths(L), 3 * L + 20, k, 2000 + 10 * k + side + L, side, long_pairs=L)


ALL_LONG_LENGTHS = (0, 33, 40, 64, 65, 97, 0, 129)


@functools.lru_cache(None)
def all_long_case(side, k):
    return solved_rows('all_long_s%d_k%d' % (side, k), ALL_LONG_LENGTHS, 140, k, 2500 + 10 * k + side, side, long_pairs=32)


CHUNKS = [(side, k, L) for side in (0, 1) for k in (20, 65) for L in (32, 100)]
ALL_LONG = [(side, k) for side in (0, 1) for k in (20, 65)]
LARGEST_CHUNKS = (0, 65, 100)


def relabelled(case, side, seed=7):
    """The same problem with the solved side's rows renamed: (case', perm), row r of `case` is row perm[r] of case'."""
    rng = np.random.RandomState(seed)
    nr = case.m if side == 0 else case.n
    perm = rng.permutation(nr)
    R = dense(case)
    Rp = np.zeros_like(R)
    X0, Y0 = case.X0.copy(), case.Y0.copy()
    if side == 0:
        Rp[perm] = R
        X0[perm] = case.X0
    else:
        Rp[:, perm] = R
        Y0[perm] = case.Y0
    um, im = pairs_from_matrix(Rp)
    return case._replace(X0=X0, Y0=Y0, um=um, im=im, name=case.name + '_relabelled'), perm


def dense(case):
    R = np.zeros((case.m, case.n), np.int64)
    up, ui, uc = case.um
    R[np.repeat(np.arange(case.m), np.diff(up)), ui] = uc
    return R


# ---- WIDTHS: the first and last k of every tile-slot regime, and the substitution wave's split at 64 ----
WIDTH_KS = (1, 2, 3, 4, 5, 63, 64, 65, 88, 89, 124, 125, 127)
WIDTHS = [(k, 1.0) for k in WIDTH_KS] + [(k, 0.01) for k in (89, 125, 127)]
W_M, W_N = 40, 60
W_USERS = {0: 0, 1: 1, 2: 2, 3: 31, 4: 32, 5: 33, 6: 57}            # user: pairs (33 and 57 are long at wrmf_long_pairs = 32)
W_ITEMS = {57: 1, 58: 33, 59: 37}                                     # item: users, drawn from users 3..39


def widths_matrix():
    rng = np.random.RandomState(31)
    R = np.zeros((W_M, W_N), np.int64)
    for item, users in W_ITEMS.items():
        R[rng.choice(np.arange(3, W_M), users, replace=False), item] = rng.randint(1, 5, users)
    free = np.arange(0, 57)
    for u in range(W_M):
        have = int((R[u] > 0).sum())
        some = int(rng.randint(3, 13))
        want = W_USERS[u] if u in W_USERS else max(some, have)
        assert have <= want <= have + len(free)
        R[u, rng.choice(free, want - have, replace=False)] = rng.randint(1, 5, want - have)
    R[6, np.flatnonzero(R[6])[20]] = 1000
    return R


@functools.lru_cache(None)
def widths_case(k, reg):
    # at reg 0.01 the fixed side (40 or 60 rows) leaves G singular for k = 89, 125, 127, so reg alone conditions A; with the
    # pair at count 1000 and alpha 10 the condition number is about 1e4 |f|^2 / 0.01 = 4e7 and two fp64 solvers differ by 1e-9 to
    # 3e-9 (measured over 12 seeds), which is tests/test_wrmf_cases.py's bound.  alpha = 1 takes one decade off: 1e-10 to 3e-10.
    case = make('widths_k%d_reg%g' % (k, reg), widths_matrix(), k, 3000 + k, (0, 1), alpha=10.0 if reg == 1.0 else 1.0, reg=reg, long_pairs=32)
    lens_u, lens_i = np.diff(case.um[0]), np.diff(case.im[0])
    assert all(lens_u[u] == v for u, v in W_USERS.items()) and all(lens_i[i] == v for i, v in W_ITEMS.items())
    return case


# ---- GRAM: the fixed side's row count at the block and stage bounds of k_wrmf_gram_part ----
GRAM_NF = (1, 2, 511, 512, 513, 16384, 16385, 16416, 16896)
GRAM = [(nf, 8) for nf in GRAM_NF] + [(513, 128), (16385, 128)]
GRAM_LENGTHS = (0, 1, 2, 5, 7, 9, 31, 32, 33, 34, 63, 65)
GRAM_ALPHAS = (10.0, 0.0)                 # at alpha = 0 every A is G + reg I: the rows depend on the Gram alone


def rows_per_block(nf):
    return (nf + GRAM_BLOCKS - 1) // GRAM_BLOCKS


def last_stage_first_row(nf):
    """The first row of the last stage of the last block that has rows."""
    rpb = rows_per_block(nf)
    r0 = (nf - 1) // rpb * rpb
    return r0 + (nf - 1 - r0) // STAGE * STAGE


def gram_rows(nf):
    """The rows of the fixed side at which a wrong loop bound of k_wrmf_gram_part loses or doubles a row."""
    rpb = rows_per_block(nf)
    rows = {0, nf - 1, rpb - 1, rpb, 31, 32, 33, last_stage_first_row(nf)}
    return sorted(r for r in rows if 0 <= r < nf)


def gram_named_rows(nf):
    rpb = rows_per_block(nf)
    near = {0, nf - 1, last_stage_first_row(nf), last_stage_first_row(nf) - 1}
    for base in (rpb, 2 * rpb, (nf - 1) // rpb * rpb, STAGE, 2 * STAGE):
        near.update((base - 1, base, base + 1))
    return sorted(r for r in near if 0 <= r < nf)


@functools.lru_cache(None)
def gram_case(nf, k, alpha, side):
    named = gram_named_rows(nf)
    lengths = tuple(min(x, nf) for x in GRAM_LENGTHS)
    first = [named[r % len(named):] + named[:r % len(named)] for r in range(len(lengths))]
    case = solved_rows('gram_nf%d_k%d_a%g_s%d' % (nf, k, alpha, side), lengths, nf, k, 4000 + nf + k + side, side, first=first, alpha=alpha)
    ptr, idx = side_of(case, side)[2:4]
    assert set(named) <= set(idx.tolist())
    return case


# ---- TINY ----
def one_by_one():
    return make('one_by_one', [[3]], 1, 5000, (0, 1))


def no_pairs():
    return make('no_pairs', np.zeros((3, 4), np.int64), 5, 5001, (0, 1))


TINY = {'one_by_one': one_by_one, 'no_pairs': no_pairs}


# ---- pivot refusals: reg = 0 with one column of the fixed side exactly zero ----
REFUSALS = [(0, 16, 5), (0, 125, 124), (0, 128, 127), (1, 16, 5)]     # the last column of the third tile slot: k = 125 and 128


@functools.lru_cache(None)
def refusal_case(side, k, column, nf=300):
    """Rows 0 and 1 of the solved side without pairs, every other row with three; the fixed side's `column` is zero, so row and
    column `column` of every A are exactly zero at reg = 0 while its leading block stays positive definite (nf > k random rows).
    The case's own reg is 1.0: the half-sweep that must succeed after the refusal."""
    lengths = (0, 0) + (3,) * 10
    case = solved_rows('refusal_s%d_k%d_c%d' % (side, k, column), lengths, nf, k, 6000 + k + side, side)
    F = (case.Y0 if side == 0 else case.X0).copy()
    F[:, column] = 0
    return case._replace(Y0=F) if side == 0 else case._replace(X0=F)


def families():
    """family -> the cases of tests/test_gpu_wrmf_edges.py, each with the half-sweeps it is made for."""
    return {
        'ROWLEN': [rowlen_case(*p) for p in ROWLEN],
        'CHUNKS': [chunks_case(*p) for p in CHUNKS] + [all_long_case(*p) for p in ALL_LONG],
        'WIDTHS': [widths_case(*p) for p in WIDTHS],
        'GRAM': [gram_case(nf, k, alpha, side) for nf, k in GRAM for alpha in GRAM_ALPHAS for side in (0, 1)],
        'TINY': [f() for f in TINY.values()],
        'REFUSALS': [refusal_case(*p) for p in REFUSALS],
    }
