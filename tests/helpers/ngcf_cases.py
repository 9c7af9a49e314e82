"""Synthetic NGCF problems from seeds, shared by tests/test_ngcf_golden.py (which checks on the CPU that every case reaches
its branch, keeps d32 small and satisfies the leaky-ReLU condition) and the GPU tests.  A case's yardstick (fp64 contract) and its
d32 figures (distance of the float32 contract from it) are computed once and cached."""
import numpy as np

from . import numpy_lightgcn as nl
from . import numpy_ngcf as ng

HUB = 96                                                        # option ngcf_hub of the cases that set it
REG = 0.01
EDGE_DEGREES = [0, 1, 63, 64, 65, 2 * HUB + 37]                 # the last: three parts, 96 + 96 + 37
WCHUNK = 512                                                    # kNgcfWChunk of ngcf_kernels.hpp

# Seeds chosen on the CPU (the first of base, base + 1000, ... ) so that the float32 contract's Z has the fp64 Z's sign at every
# element and min |Z| >= 16 max |Z32 - Z64|: a flipped sign changes a gradient element by a jump that no rounding bound covers.
# The float32 contract's loss must also lie at least 2^-25 (relative) from the fp64 loss: the float32 result's own spacing is 2^-24,
# and a distance far below it is a lucky rounding that says nothing about float32 arithmetic, while the loss bound is 4 x that
# distance.  Nothing the device computes enters the choice.  tests/test_ngcf_golden.py asserts seed_ok for every case.
SEEDS = {'k1': 101, 'k2': 3102, 'k31': 131, 'k32': 5132, 'k33': 2133, 'k64': 9164, 'k128': 228, 'k85': 11185, 'N31': 431, 'N32': 1432, 'N33': 433,
         'chunk': 22513, 'deg_written': 14607, 'deg_symmetric': 25609, 'keep1': 6701, 'eval': 5702, 'symmetric': 703, 'T1': 2721, 'T63': 1783,
         'T64': 2784, 'T65': 785, 'repeat': 730, 'posneg': 731}


def _case(name, seed, m=50, n=60, k=20, layers=3, T=64, hub=None, batch='random', stddev=0.005, form='written', training=True, keep=0.9,
          edges=False, mindeg=0):
    return dict(mindeg=mindeg, name=name, seed=seed, m=m, n=n, k=k, layers=layers, T=T, hub=hub, batch=batch, stddev=stddev, form=form, training=training,
                keep=keep, edges=edges)


# k = 1: a normalised row is +-1 and its derivative is exactly 0; rows of order 1 keep the case meaningful
# (and there every row has events: a dropped row without neighbours would give Z = 0 exactly in the next layer, where the leaky-ReLU
# condition min |Z| >= 16 max |Z32 - Z64| cannot hold)
CASES = [_case('k1', SEEDS['k1'], m=55, n=55, k=1, stddev=1.0, mindeg=1)]
CASES += [_case('k%d' % k, SEEDS['k%d' % k], k=k) for k in (2, 31, 32, 33, 64)]
CASES += [_case('k128', SEEDS['k128'], k=128, layers=1), _case('k85', SEEDS['k85'], k=85, layers=2)]
CASES += [_case('N%d' % (m + n), SEEDS['N%d' % (m + n)], m=m, n=n, T=16) for m, n in ((15, 16), (16, 16), (16, 17))]      # N = 110 is every other case
CASES += [_case('chunk', SEEDS['chunk'], m=250, n=WCHUNK + 1 - 250, k=20)]                                       # one row into the second chunk
CASES += [_case('deg_%s' % f, SEEDS['deg_%s' % f], m=240, n=260, k=20, hub=HUB, edges=True, form=f) for f in ('written', 'symmetric')]
CASES += [_case('keep1', SEEDS['keep1'], k=32, keep=1.0), _case('eval', SEEDS['eval'], k=32, training=False), _case('symmetric', SEEDS['symmetric'], m=60, n=50, k=32, form='symmetric')]
CASES += [_case('T%d' % T, SEEDS['T%d' % T], k=32, T=T) for T in (1, 63, 64, 65)]
CASES += [_case('repeat', SEEDS['repeat'], k=32, batch='repeat'), _case('posneg', SEEDS['posneg'], k=32, batch='posneg')]
BY_NAME = {c['name']: c for c in CASES}
GPU_CASES = [c['name'] for c in CASES]
_cache = {}


def _pairs(rs, c):
    m, n = c['m'], c['n']
    deg = rs.randint(0, 11, size=m)
    deg[0], deg[1] = 0, 10                                      # a user with no events beside users with many
    deg = np.maximum(deg, c['mindeg'])
    if c['edges']:
        deg[:len(EDGE_DEGREES)] = EDGE_DEGREES
    pairs = set()
    for u, d in enumerate(deg):
        lo = 10 if c['edges'] else 0                            # the edge tracks 0 .. 5 get their users below
        for t in rs.choice(np.arange(lo, n), size=int(d), replace=False):
            pairs.add((u, int(t)))
    if c['edges']:
        for t, d in enumerate(EDGE_DEGREES):
            for u in rs.choice(np.arange(10, m), size=int(d), replace=False):
                pairs.add((int(u), t))
    pairs = sorted(pairs)
    pu, pt = np.array([p[0] for p in pairs], np.int64), np.array([p[1] for p in pairs], np.int64)
    # weights of the reference's form c (c + 1) / sqrt(d_u) / sqrt(d_t) with c in {1, 2, 3}, rounded once
    cnt = rs.randint(1, 4, size=len(pairs)).astype(np.float64)
    du, dt = np.bincount(pu, weights=cnt, minlength=m), np.bincount(pt, weights=cnt, minlength=n)
    w = (cnt * (cnt + 1) / np.sqrt(du[pu]) / np.sqrt(dt[pt])).astype(np.float32)
    return pu, pt, w


def seed_ok(c):
    """What a case's seed was chosen for (CPU only); c = build(name)."""
    d = dict(c['d32'])
    if c['k'] == 1:
        d.pop('gW')                 # analytically 0 at k = 1 (a normalised row is +-1): its distance is noise over noise
    ok = c['zsign'] and c['zmin'] >= 16 * c['zerr'] and max(d.values()) <= 1e-5 and c['d32']['loss'] >= 2.0 ** -25
    if c['k'] <= 2:
        ok = ok and sum(int((s < ng.EPS).sum()) for s in c['fw']['ss']) > 0      # a row whose every element is dropped: the clamp branch
    return bool(ok)


def build(name):
    """dict with the graph g, U, V, W, the batch (u, i, j), the fp64 yardstick ('loss', 'gU', 'gV', 'gW', 'fw'), 'd32' and the
    leaky-ReLU figures 'zmin' (min |Z64|), 'zerr' (max |Z32 - Z64|), 'zsign' (every sign equal)."""
    if name in _cache:
        return _cache[name]
    c = dict(BY_NAME[name])
    rs = np.random.RandomState(c['seed'])
    m, n, k, T, L = c['m'], c['n'], c['k'], c['T'], c['layers']
    pu, pt, w = _pairs(rs, c)
    g = ng.graph_from_pairs(pu, pt, w, m, n, c['form'])
    U, V = nl.truncated_normal(rs, (m, k), c['stddev']), nl.truncated_normal(rs, (n, k), c['stddev'])
    W = ng.xavier(rs, L, k)
    if c['batch'] == 'repeat':                                  # one triplet 64 times
        u, i, j = np.full(64, 3), np.full(64, 5), np.full(64, 7)
    elif c['batch'] == 'posneg':                                # item 5 is positive in one triplet and negative in another
        u, i, j = rs.randint(0, m, size=T), rs.randint(0, n, size=T), rs.randint(0, n, size=T)
        i[0], j[1], j[0], i[1] = 5, 5, 6, 7
    else:
        u, i, j = rs.randint(0, m, size=T), rs.randint(0, n, size=T), rs.randint(0, n, size=T)
        u[0] = 0                                                # the user without events is trained on too
    c.update(g=g, U=U, V=V, W=W, u=u.astype(np.int32), i=i.astype(np.int32), j=j.astype(np.int32), mask_seed=c['seed'] * 7919, step=3)
    args = (c['training'], c['keep'], c['mask_seed'], c['step'])
    loss, gU, gV, gW, fw = ng.loss_and_grad(g, U.astype(np.float64), V.astype(np.float64), W, u, i, j, REG, *args, dtype=np.float64)
    loss32, gU32, gV32, gW32, fw32 = ng.loss_and_grad(g, U, V, W, u, i, j, REG, *args, dtype=np.float32)
    assert loss32.dtype == np.float32 and gU32.dtype == np.float32 and gW32.dtype == np.float32 and fw32['F'].dtype == np.float32
    c.update(loss=float(loss), gU=gU, gV=gV, gW=gW, fw=fw)
    d32 = {'F': ng.rel(fw32['F'], fw['F']), 'gU': ng.rel(gU32, gU), 'gV': ng.rel(gV32, gV), 'gW': ng.rel(gW32, gW),
           'loss': abs(float(loss32) - float(loss)) / abs(float(loss))}
    for l in range(L):
        for key in ('S', 'Z', 'D'):
            d32['%s%d' % (key, l + 1)] = ng.rel(fw32[key][l], fw[key][l])
    c['d32'] = d32
    Z64, Z32 = np.stack(fw['Z']), np.stack(fw32['Z']).astype(np.float64)
    c['zmin'], c['zerr'] = float(np.abs(Z64).min()), float(np.abs(Z32 - Z64).max())
    c['zsign'] = bool(np.array_equal(np.sign(Z32), np.sign(Z64)))
    _cache[name] = c
    return c
