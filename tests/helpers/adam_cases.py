"""The live Adam path's problems (yue_adam_step = k_mb_grad<KR> + k_adam) with their triplets set explicitly, shared by
tests/test_adam_golden.py (which checks on the CPU that every case reaches the branch it exists for, that the float32 contract stays
within the bounds and that named faults leave them by 100 x) and tests/test_gpu_adam_edges.py.  A case's yardstick (the fp64
graph, oracle/numpy_adam.loss_and_grad) and its bounds (oracle/numpy_adam.bounds: a priori, from the formats' rounding alone) are
computed once and cached.  Only the factors and the filler triplets come from the seed.

What k_mb_grad does with a feed: a wave takes CHUNK = 32 consecutive triplets (a workgroup 4 waves = 128), keeps (u, i) of the current
run in registers and flushes the run's two summed rows when (u, i) changes or its chunk ends; every negative's row goes out at once.
KR = 1, 2, 4 registers per lane for k <= 64, <= 128, <= 256.

Width cases and 'big' open with the forced triplets (forced()): user m - 1 with items 0 and n - 1; item A positive for user 1 and negative for
user 2, item B the other way round."""
import numpy as np

from oracle import numpy_adam as na

REG, STDDEV, LR = 0.01, 0.005, 0.02
CHUNK, GROUP = 32, 128
A, B = 5, 9
LONE_USER, LONE_ITEM = 3, 33
ONE_J = 17
RUN_LENGTHS = (1, 1, 2, 3, 5, 8, 17, 40)
ADAM_GRID_REACH = 8192 * 256                 # elements k_adam's capped grid covers in one trip of its loop


def _case(name, seed, m=60, n=90, k=20, T=200, kind='mixed', scale=STDDEV, forced=False):
    return dict(name=name, seed=seed, m=m, n=n, k=k, T=T, kind=kind, scale=scale, forced=forced, reg=REG)


WIDTHS = [_case('k%d' % k, 100 + k, k=k, forced=True) for k in (1, 63, 64, 65, 128, 129, 256)]
SIZES = [_case('T%d' % T, 200 + T, T=T) for T in (1, 31, 32, 33, 127, 128, 129)]
RUNS = [_case('run1', 301, T=96, kind='run1'), _case('u_moves', 302, T=96, kind='u_moves'), _case('i_moves', 303, T=96, kind='i_moves'),
        _case('abab', 304, T=128, kind='abab'), _case('cut', 305, T=160, kind='cut'), _case('cut_group', 306, T=192, kind='cut_group'),
        _case('neg100', 307, T=800, kind='neg100')]
COLLISIONS = [_case('ieqj', 401, T=96, kind='ieqj'), _case('one_j', 402, T=4096, kind='one_j'), _case('repeat', 403, T=64, kind='repeat')]
SATURATED = [_case(name, 500 + x, m=40, n=60, k=16, T=96, kind=name, scale=3.0) for x, name in enumerate(('sat_pos', 'sat_neg', 'sat_mix'))]
BIG = [_case('big', 601, m=3, n=8230, k=255, T=256, forced=True)]
CASES = WIDTHS + SIZES + RUNS + COLLISIONS + SATURATED + BIG
BY_NAME = {c['name']: c for c in CASES}
NAMES = [c['name'] for c in CASES]
WIDTH_NAMES, SAT_NAMES = [c['name'] for c in WIDTHS], [c['name'] for c in SATURATED]
_cache = {}


def kr_of(k):
    return 1 if k <= 64 else 2 if k <= 128 else 4


def forced(m, n):
    return [(m - 1, 0, n - 1), (1, A, B), (2, B, A)]


def runs(u, i):
    """Lengths of the feed's maximal runs of equal (u, i)."""
    cut = np.flatnonzero((np.diff(u) != 0) | (np.diff(i) != 0)) + 1
    return np.diff(np.r_[0, cut, len(u)]).tolist()


def _pair(rs, c, avoid=None):
    """A random (u, i) other than `avoid`; users LONE_USER and items LONE_ITEM, ONE_J stay out of the fillers."""
    while True:
        u, i = int(rs.randint(0, c['m'])), int(rs.randint(0, c['n']))
        if (u, i) != avoid and u != LONE_USER and i not in (LONE_ITEM, ONE_J):
            return u, i


def _neg(rs, c, i):
    while True:
        j = int(rs.randint(0, c['n']))
        if j != i and j not in (LONE_ITEM, ONE_J):
            return j


def _mixed(rs, c, T, out=None):
    """Runs of the lengths RUN_LENGTHS, in seeded order, until T triplets stand."""
    out = [] if out is None else out
    last = None
    while len(out) < T:
        last = _pair(rs, c, last)
        for _ in range(min(int(rs.choice(RUN_LENGTHS)), T - len(out))):
            out.append(last + (_neg(rs, c, last[1]),))
    return out


def _stepped(rs, c, T, every_u, every_i):
    """u changes every `every_u` triplets, i every `every_i` (0: never)."""
    def other(axis, old):
        while True:
            new = _pair(rs, c)[axis]
            if new != old:
                return new
    out, (u, i) = [], _pair(rs, c)
    for t in range(T):
        if t and every_u and t % every_u == 0:
            u = other(0, u)
        if t and every_i and t % every_i == 0:
            i = other(1, i)
        out.append((u, i, _neg(rs, c, i)))
    return out


def _saturated(rs, c, U, V):
    """Triplets chosen by their fp64 margin: a third from the ends of the user's ranking (beyond 90), the others random pairs (0 to
    beyond 20), oriented by the case; LONE_USER's only triplet is its best item against its worst (beyond -90 in 'sat_neg', beyond +90 in the others)."""
    S = U.astype(np.float64) @ V.astype(np.float64).T
    out = []
    for t in range(c['T']):
        u = LONE_USER if t == 10 else _pair(rs, c)[0]
        order = np.argsort(S[u])
        if t % 3 == 1 or t == 10:
            lo, hi = int(order[rs.randint(0, 2)]), int(order[-1 - rs.randint(0, 2)])
        else:
            lo, hi = sorted(rs.choice(c['n'], 2, replace=False).tolist(), key=lambda x: S[u, x])
        up = c['kind'] == 'sat_pos' or (c['kind'] == 'sat_mix' and (t % 2 == 0 or t == 10))
        out.append((u, hi, lo) if up else (u, lo, hi))
    return out


def _triplets(rs, c, U, V):
    T, kind = c['T'], c['kind']
    if kind == 'mixed':
        out = _mixed(rs, c, T, forced(c['m'], c['n']) if c['forced'] else None)
    elif kind == 'run1':
        out, last = [], None
        while len(out) < T:
            last = _pair(rs, c, last)
            out.append(last + (_neg(rs, c, last[1]),))
    elif kind == 'u_moves':
        out = _stepped(rs, c, T, 3, 0)
    elif kind == 'i_moves':
        out = _stepped(rs, c, T, 0, 3)
    elif kind == 'abab':
        p, q = _pair(rs, c), _pair(rs, c)
        assert p[0] != q[0] and p[1] != q[1]
        out = [(p if t % 2 == 0 else q) + (_neg(rs, c, (p if t % 2 == 0 else q)[1]),) for t in range(T)]
    elif kind in ('cut', 'cut_group'):
        # one run of 100 over triplets first .. first + 99, single-triplet runs around it.  'cut' (20 .. 119) crosses the chunk edges
        # 32, 64, 96: four waves of ONE workgroup flush onto the run's two rows.  'cut_group' (60 .. 159) crosses 64, 96 and 128, the
        # workgroup's edge: the flushes come from two workgroups.
        first = 20 if kind == 'cut' else 60
        long_run = _pair(rs, c)
        out, last = [], None
        while len(out) < T:
            if first <= len(out) < first + 100:
                last = long_run
            else:
                last = _pair(rs, c, last)
                while last == long_run:
                    last = _pair(rs, c, last)
            out.append(last + (_neg(rs, c, last[1]),))
    elif kind == 'neg100':
        out, last = [], None
        for _ in range(8):
            last = _pair(rs, c, last)
            out += [last + (_neg(rs, c, last[1]),) for _ in range(100)]
    elif kind == 'ieqj':
        out = _mixed(rs, c, T)
        out[10] = (LONE_USER, LONE_ITEM, LONE_ITEM)                  # the user's and the item's only triplet
    elif kind == 'one_j':
        out = [(u, i, ONE_J) for u, i, _ in _mixed(rs, c, T)]
    elif kind == 'repeat':
        u, i = _pair(rs, c)
        out = [(u, i, _neg(rs, c, i))] * T
    else:
        out = _saturated(rs, c, U, V)
    assert len(out) == T
    return [np.array(x, np.int32) for x in zip(*out)]


def build(name):
    """dict: U, V (float32), the feed u, i, j, reg; the fp64 yardstick loss, gU, gV and margins x; the bounds b_loss, bU, bV; the
    feed's run lengths."""
    if name in _cache:
        return _cache[name]
    c = dict(BY_NAME[name])
    rs = np.random.RandomState(c['seed'])
    c['U'] = na.truncated_normal(rs, (c['m'], c['k']), c['scale'])
    c['V'] = na.truncated_normal(rs, (c['n'], c['k']), c['scale'])
    c['u'], c['i'], c['j'] = u, i, j = _triplets(rs, c, c['U'], c['V'])
    measure(c, c['U'], c['V'], u, i, j)
    c['runs'] = runs(u, i)
    for a in (c['U'], c['V'], u, i, j, c['gU'], c['gV'], c['bU'], c['bV']):
        a.setflags(write=False)
    _cache[name] = c
    return c


def measure(c, U, V, u, i, j):
    """Sets (into c) the yardstick and the bounds of the feed (u, i, j) at the factors (U, V)."""
    c['loss'], c['gU'], c['gV'] = na.loss_and_grad(U, V, u, i, j, c['reg'], np.float64)
    c['loss'] = float(c['loss'])
    c['b_loss'], c['bU'], c['bV'] = na.bounds(U, V, u, i, j, c['reg'])
    U64, V64 = U.astype(np.float64), V.astype(np.float64)
    c['x'] = (U64[u] * (V64[i] - V64[j])).sum(axis=1)
    return c


def ratio(got, want, bound):
    """The largest |got - want| / bound over the elements (an element with bound 0 must be met exactly)."""
    d = np.abs(np.asarray(got, np.float64) - want)
    if ((bound == 0) & (d != 0)).any():
        return np.inf
    return float((d[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0


def lost_flushes(u, i):
    """Triplets whose run goes on across the end of their chunk: what a wave that forgot its last flush would lose."""
    T = len(u)
    lost = np.zeros(T, bool)
    for edge in range(CHUNK, T, CHUNK):
        t = edge - 1
        if (u[t], i[t]) != (u[edge], i[edge]):
            continue
        while t >= edge - CHUNK and (u[t], i[t]) == (u[edge], i[edge]):
            lost[t] = True
            t -= 1
    return lost


FAULTS = ('drop_last', 'lost_flush', 'no_reg_neg', 'neg_sign', 'pad')


def applies(fault, c):
    if fault == 'lost_flush':
        return bool(lost_flushes(c['u'], c['i']).any())
    if fault == 'pad':
        return c['name'] in WIDTH_NAMES and c['k'] % 64 != 0
    return True


def contract(U, V, u, i, j, reg, fault=None):
    """(gU, gV) of the float32 contract, term by term as oracle/numpy_adam.loss_and_grad forms them, with one named fault:
    drop_last   the last triplet never arrives (a t1 clamp or grid one short);
    lost_flush  a run's summed rows are lost where its chunk ends and the run goes on (the negatives' rows still go out);
    no_reg_neg  the negative row's term lacks reg * V_j;
    neg_sign    the negative row gets a * U_u, the positive row's sign;
    pad         the lanes beyond k of the last register count as elements of the row (no `e < k`): the margin and the rows' terms
                run over 64 * KR elements from the row's start, on into the next row (zeros past the matrix), and go out there.
                (With the loads alone unguarded and the stores guarded, only the margin moves: by ONE product of two 0.005
                factors at k = 63, which reaches 20 .. 110 bounds over sixteen seeds -- the bounds see it, but not by 100.)"""
    f = np.float32
    reg, k = f(reg), U.shape[1]
    if fault == 'drop_last':
        u, i, j = u[:-1], i[:-1], j[:-1]
    Ue, Ve, Ne = U[u], V[i], V[j]
    if fault == 'pad':
        W = 64 * kr_of(k)
        flatU, flatV = np.r_[U.ravel(), np.zeros(W, f)], np.r_[V.ravel(), np.zeros(W, f)]
        span = np.arange(W)
        Uw, Vw, Nw = flatU[u[:, None] * k + span], flatV[i[:, None] * k + span], flatV[j[:, None] * k + span]
        err = (Uw * Vw).sum(axis=1) - (Uw * Nw).sum(axis=1)
    else:
        err = (Ue * Ve).sum(axis=1) - (Ue * Ne).sum(axis=1)
    with np.errstate(over='ignore'):
        g = -(f(1) / (f(1) + np.exp(err))).astype(f)
    if fault == 'pad':
        Ue, Ve, Ne = Uw, Vw, Nw
    tu, ti = g[:, None] * (Ve - Ne) + reg * Ue, g[:, None] * Ue + reg * Ve
    tj = -g[:, None] * Ue + reg * Ne
    if fault == 'no_reg_neg':
        tj = -g[:, None] * Ue
    if fault == 'neg_sign':
        tj = g[:, None] * Ue + reg * Ne
    if fault == 'lost_flush':
        lost = lost_flushes(u, i)
        tu[lost], ti[lost] = 0, 0
    if fault == 'pad':
        fU, fV = np.zeros(len(flatU), f), np.zeros(len(flatV), f)
        np.add.at(fU, u[:, None] * k + span, tu)
        np.add.at(fV, i[:, None] * k + span, ti)
        np.add.at(fV, j[:, None] * k + span, tj)
        return fU[:U.size].reshape(U.shape), fV[:V.size].reshape(V.shape)
    gU, gV = np.zeros_like(U), np.zeros_like(V)
    np.add.at(gU, u, tu)
    np.add.at(gV, i, ti)
    np.add.at(gV, j, tj)
    return gU, gV
