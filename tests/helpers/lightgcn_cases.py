"""Synthetic LightGCN problems from seeds, shared by tests/test_lightgcn_golden.py (which checks on the CPU that every case
reaches its branch and keeps d32 small) and the GPU tests.  A case's yardstick (fp64 contract) and its d32 figures (distance of
the float32 contract from it) are computed once and cached."""
import numpy as np

from . import numpy_lightgcn as nl

HUB = 96                                                        # option lgcn_hub of the cases that set it
REG = 0.01


def _case(name, seed, m, n, k, degrees=None, weights=(1.0,), layers=3, T=64, hub=None, batch='random', stddev=0.005):
    return dict(stddev=stddev, name=name, seed=seed, m=m, n=n, k=k, degrees=degrees, weights=weights, layers=layers, T=T, hub=hub, batch=batch)


EDGE_DEGREES = [0, 1, 63, 64, 65, HUB - 1, HUB, HUB + 1, 2 * HUB + 37]      # the last: three parts, 96 + 96 + 37

# k = 1: a normalised row is +-1 and its derivative is exactly 0; in float32 the cancellation leaves 1e-7 |g| / |E_l|, which
# the start rows' 0.005 scale would blow up to 5e-4 of the gradient (measured) -- rows of order 1 keep the case meaningful
CASES = [_case('k%d' % k, 100 + k, 50, 40, k, stddev=1.0 if k == 1 else 0.005) for k in (1, 20, 63, 64, 65, 128)]
CASES += [_case('deg_k%d' % k, 200 + k, 40, 260, k, degrees=EDGE_DEGREES, hub=HUB) for k in (20, 64, 128)]
CASES += [_case('w81', 301, 50, 40, 64, weights=(1.0, 81.0))]
CASES += [_case('layers%d' % L, 310 + L, 50, 40, 20, layers=L) for L in (1, 2, 3)]
CASES += [_case('T%d' % T, 320 + T, 50, 40, 64, T=T) for T in (1, 63, 64, 65)]
CASES += [_case('repeat', 330, 50, 40, 64, batch='repeat'), _case('posneg', 331, 50, 40, 64, batch='posneg')]
BY_NAME = {c['name']: c for c in CASES}
_cache = {}


def build(name):
    """dict with the graph g, U, V, the batch (u, i, j), the fp64 yardstick ('loss', 'gU', 'gV', 'F', 'E') and 'd32'."""
    if name in _cache:
        return _cache[name]
    c = dict(BY_NAME[name])
    rs = np.random.RandomState(c['seed'])
    m, n, k, T = c['m'], c['n'], c['k'], c['T']
    deg = rs.randint(0, 11, size=m)
    deg[0], deg[1] = 0, 10                                      # a user with no events beside users with many
    if c['degrees'] is not None:
        deg[:len(c['degrees'])] = c['degrees']
    pu, pi, w = nl.synthetic_pairs(rs, m, n, deg, c['weights'])
    g = nl.graph_from_pairs(pu, pi, w, m, n)
    U, V = nl.truncated_normal(rs, (m, k), c['stddev']), nl.truncated_normal(rs, (n, k), c['stddev'])
    if c['batch'] == 'repeat':                                  # one triplet 64 times
        u, i, j = np.full(64, 3), np.full(64, 5), np.full(64, 7)
    elif c['batch'] == 'posneg':                                # item 5 is positive in one triplet and negative in another
        u, i, j = rs.randint(0, m, size=T), rs.randint(0, n, size=T), rs.randint(0, n, size=T)
        i[0], j[1], j[0], i[1] = 5, 5, 6, 7
    else:
        u, i, j = rs.randint(0, m, size=T), rs.randint(0, n, size=T), rs.randint(0, n, size=T)
        u[0] = 0                                                # the user without events is trained on too
    c.update(g=g, U=U, V=V, u=u.astype(np.int32), i=i.astype(np.int32), j=j.astype(np.int32), deg=deg)
    L = c['layers']
    loss, gU, gV, F, E = nl.loss_and_grad(g, U.astype(np.float64), V.astype(np.float64), u, i, j, REG, L, np.float64)
    loss32, gU32, gV32, F32, E32 = nl.loss_and_grad(g, U, V, u, i, j, REG, L, np.float32)
    assert loss32.dtype == np.float32 and gU32.dtype == np.float32 and F32.dtype == np.float32
    c.update(loss=float(loss), gU=gU, gV=gV, F=F, E=E)
    d32 = {'F': nl.rel(F32, F), 'gU': nl.rel(gU32, gU), 'gV': nl.rel(gV32, gV), 'loss': abs(float(loss32) - float(loss)) / abs(float(loss))}
    for l in range(1, L + 1):
        d32['E%d' % l] = nl.rel(E32[l], E[l])
    c['d32'] = d32
    _cache[name] = c
    return c
