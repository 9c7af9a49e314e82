"""APR problems with their triplets set explicitly, shared by tests/test_apr_golden.py (which checks on the CPU that every case
meets its conditioning statement), tests/test_gpu_apr.py (CASES, STEP_CASES) and tests/test_gpu_apr_edges.py (EDGE_CASES).  A case's
yardstick (the fp64 contract tests/helpers/numpy_apr.py) and its d32 figures (distance of the float32 contract from it) are computed
once and cached.  Only the factors, the standing perturbation's rows and the filler triplets come from the seed.

Every case with T >= 8 opens with the same forced triplets (FORCED): user m - 1 with items 0 and n - 1; item A positive for user 1
and negative for user 2, item B the other way round (so B is both in one batch); the triplet (1, A, B) a second time.

Conditioning.  Factors are drawn at stddev 0.25 (the reference's 0.005 would leave every margin at 0 and every sigmoid at 1/2), so
|x| stays below 10.  The perturbation's normalisation divides a row's gradient g by |g|: where the row's terms cancel, |g| is small
against the sum of their norms and the division amplifies the terms' rounding by that ratio.  Every batch row of every case keeps
|g| >= FRACTION * (sum of its terms' norms), so the amplification is at most 1 / FRACTION = 16.  The one exception is built to
cancel: the user of 'ieqj' whose only triplet has i == j cancels exactly, in every precision (g = 0, and D stays 0)."""
import numpy as np

from . import numpy_apr as ap

REG, REG_A, EPS = 0.01, 1.0, 0.5
STDDEV = 0.25
FRACTION = 1.0 / 16
A, B = 5, 9
QUANTITIES = ('loss_pre', 'gU_pre', 'gV_pre', 'loss_adv', 'gU_adv', 'gV_adv', 'rawU', 'rawV', 'dU', 'dV')


def _case(name, seed, m=40, n=70, k=20, T=96, kind=None, eps=EPS, regA=REG_A):
    return dict(name=name, seed=seed, m=m, n=n, k=k, T=T, kind=kind, eps=eps, regA=regA)


CASES = [_case('base', 11), _case('k64', 12, k=64), _case('k50', 13, k=50, m=60, n=100, T=200), _case('k128', 14, k=128)]
STEP_CASES = ['base', 'k64', 'k50', 'k129']
# (k = 1: a row's terms are scalars and cancel easily; 24 triplets and a seed chosen for the conditioning statement below)
EDGE_CASES = [_case('k1', 301, k=1, T=24)] + [_case('k%d' % k, 100 + k, k=k) for k in (63, 65, 129, 256)]
EDGE_CASES += [_case('T1', 201, T=1), _case('hubuser', 300, n=100, T=200, kind='hubuser'), _case('ieqj', 203, kind='ieqj'),
               _case('eps0', 204, eps=0.0), _case('regA0', 205, regA=0.0), _case('carried', 300, kind='carried')]
BY_NAME = {c['name']: c for c in CASES + EDGE_CASES}
GPU_CASES = [c['name'] for c in CASES]
EDGE_NAMES = [c['name'] for c in EDGE_CASES]
HUB_USER, LONE_USER, LONE_ITEM = 7, 3, 33
_cache = {}


def forced(m, n):
    return [(m - 1, 0, n - 1), (1, A, B), (2, B, A), (1, A, B)]


def _triplets(rs, c):
    m, n, T, kind = c['m'], c['n'], c['T'], c['kind']
    # fillers leave users 0 .. 3 and LONE_ITEM alone, and never have i == j
    out = forced(m, n) if T >= 8 and kind != 'hubuser' else []
    while len(out) < T:
        u, i, j = int(rs.randint(4, m - 1)), int(rs.randint(0, n)), int(rs.randint(0, n))
        if i == j or LONE_ITEM in (i, j):
            continue
        if kind == 'hubuser':
            # one user in every triplet: the user's list has length T.  Every item row's terms are multiples of that one user row,
            # so an item on both sides would cancel: positives come from the lower half of the item axis, negatives from the upper
            u, i, j = HUB_USER, min(i, j) % (n // 2), n // 2 + max(i, j) % (n // 2)
        out.append((u, i, j))
    if kind == 'ieqj':
        out[10] = (LONE_USER, LONE_ITEM, LONE_ITEM)                # the user's and the item's only triplet
    return [np.array(x, np.int32) for x in zip(*out)]


def _standing(rs, c, u, i, j):
    """The perturbation before the batch: rows of norm eps on every second distinct row of the batch and on two rows outside it
    (user 0 and item LONE_ITEM, which no filler names).  'carried' and 'T1' start from none."""
    m, n, k = c['m'], c['n'], c['k']
    if c['kind'] == 'carried' or c['T'] == 1:
        return np.zeros(0, np.int32), np.zeros((0, k), np.float32), np.zeros(0, np.int32), np.zeros((0, k), np.float32)
    ids_u = sorted(set(np.unique(u)[::2].tolist()) | {0})
    ids_i = sorted(set(np.unique(np.concatenate([i, j]))[::2].tolist()) | {LONE_ITEM})

    def rows(count):
        g = rs.normal(size=(count, k))
        return ap.normalize(g, max(c['eps'], EPS), np.float64).astype(np.float32)
    return np.array(ids_u, np.int32), rows(len(ids_u)), np.array(ids_i, np.int32), rows(len(ids_i))


def dense(c, ids_u, rows_u, ids_i, rows_v):
    dU, dV = np.zeros((c['m'], c['k']), np.float32), np.zeros((c['n'], c['k']), np.float32)
    dU[ids_u], dV[ids_i] = rows_u, rows_v
    return dU, dV


def measure(U, V, dU, dV, u, i, j, eps, regA, reg=REG):
    """(want, d32, L): the fp64 contract's QUANTITIES at the standing perturbation (dU, dV), the float32 contract's distance from each,
    and the longest sum behind each (a row's list, a k-long dot product under every coefficient, the k-long sum of squares under
    D; the T-long sum of the loss)."""
    out = []
    for dtype in (np.float64, np.float32):
        lp, gUp, gVp = ap.pre_loss_and_grad(U, V, u, i, j, reg, dtype)
        la, gUa, gVa = ap.adv_loss_and_grad(U, V, dU, dV, u, i, j, regA, dtype)
        rU, rV, nU, nV = ap.delta_update(U, V, dU, dV, u, i, j, eps, regA, dtype)
        assert all(x.dtype == dtype for x in (gUp, gVp, gUa, gVa, rU, rV, nU, nV))
        out.append(dict(zip(QUANTITIES, (float(lp), gUp, gVp, float(la), gUa, gVa, rU, rV, nU, nV))))
    want, got32 = out
    d32 = {q: (abs(got32[q] - want[q]) / abs(want[q]) if q.startswith('loss') else ap.rel(got32[q], want[q])) for q in QUANTITIES}
    T, k = len(u), U.shape[1]
    longest = int(max(np.bincount(u).max(), np.bincount(np.concatenate([i, j])).max()))
    L = {q: (T + k if q.startswith('loss') else longest + 2 * k if q in ('dU', 'dV') else longest + k) for q in QUANTITIES}
    return want, d32, L


def build(name):
    """dict: U, V, the batch u, i, j, the standing perturbation (ids_u, rows_u, ids_i, rows_v; dU, dV dense), eps, regA, the fp64
    yardstick 'want', 'd32' and 'L' per quantity; 'carried' also holds its first batch (u1, i1, j1)."""
    if name in _cache:
        return _cache[name]
    c = dict(BY_NAME[name])
    rs = np.random.RandomState(c['seed'])
    m, n, k = c['m'], c['n'], c['k']
    c['U'], c['V'] = rs.normal(0.0, STDDEV, size=(m, k)).astype(np.float32), rs.normal(0.0, STDDEV, size=(n, k)).astype(np.float32)
    u, i, j = _triplets(rs, c)
    if c['kind'] == 'carried':
        # the first batch: the forced rows and every third filler; the second (u, i, j): the forced rows and the other fillers.
        # Rows of the forced triplets are carried, the fillers' mostly belong to one batch alone.
        first = np.r_[0:4, 4:len(u):3]
        second = np.setdiff1d(np.arange(len(u)), first[4:])
        c['u1'], c['i1'], c['j1'] = u[first], i[first], j[first]
        u, i, j = u[second], i[second], j[second]
    c['u'], c['i'], c['j'] = u, i, j
    c['ids_u'], c['rows_u'], c['ids_i'], c['rows_v'] = _standing(rs, c, u, i, j)
    c['dU'], c['dV'] = dense(c, c['ids_u'], c['rows_u'], c['ids_i'], c['rows_v'])
    c['want'], c['d32'], c['L'] = measure(c['U'], c['V'], c['dU'], c['dV'], u, i, j, c['eps'], c['regA'])
    _cache[name] = c
    return c


def bound(d32, L, key):
    """4 x the case's d32, but no less than L 2^-24: a d32 that happens to be 0 must not demand another summation order's bits."""
    return max(4 * d32[key], L[key] * 2.0 ** -24)


def conditioning(c, dU=None, dV=None, u=None, i=None, j=None):
    """(the smallest |g| / sum |term| over the batch's rows that do not cancel exactly, the rows that do)."""
    dU, dV = (c['dU'], c['dV']) if dU is None else (dU, dV)
    u, i, j = (c['u'], c['i'], c['j']) if u is None else (u, i, j)
    gU, gV, nU, nV = ap.delta_grad(c['U'], c['V'], dU, dV, u, i, j, c['regA'] if c['regA'] else 1.0, np.float64, norms=True)
    ratios, exact = [], []
    for g, nsum, ids, side in ((gU, nU, np.unique(u), 'u'), (gV, nV, np.unique(np.concatenate([i, j])), 'i')):
        for r in ids:
            norm = float(np.linalg.norm(g[r]))
            if norm == 0.0:
                exact.append((side, int(r)))
            else:
                ratios.append(norm / float(nsum[r]))
    return min(ratios), exact


def step_batches(c):
    """Three phase-1 batches (the case's own) and three phase-2 batches that leave user u[4] and items i[4], j[4] out: those rows
    belong to phase 1 only.  The phase-2 batches differ, so that some rows' perturbation is carried and some rows' is not."""
    u, i, j = c['u'], c['i'], c['j']
    keep = np.flatnonzero((u != u[4]) & ~np.isin(i, (i[4], j[4])) & ~np.isin(j, (i[4], j[4])))
    third = len(keep) // 3
    subs = [keep, keep[:2 * third], keep[third:]]
    return [(u, i, j)] * 3 + [(u[s], i[s], j[s]) for s in subs]
