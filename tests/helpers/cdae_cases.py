"""Synthetic CDAE problems from seeds, shared by tests/test_cdae_golden.py (which checks on the CPU that every case reaches its
branch and meets its conditioning statement) and tests/test_gpu_cdae.py.  A case's yardstick (the fp64 contract
tests/helpers/numpy_cdae.py) and its d32 figures (distance of the float32 contract from it) are computed once and cached.

Conditioning.  Parameters are drawn at stddev 0.25, so that every sampled logit has |.| <= 10 in fp64: no output is near 1 or near
the 1e-6 clamp, where float32 and fp64 take different branches.  The cases 'low' and 'sat' cross those lines on purpose and by a
wide margin: one decoder column with bias -20 (dec = 2e-9: the clamp's loss term, no gradient) or +40 (y_pred = 1.0f)."""
import numpy as np

from . import numpy_cdae as cd

HUB = 8                                                         # option cdae_hub of the case that sets it
REG = 0.01
STDDEV = 0.25
SPECIAL = 11                                                    # the decoder column of 'low' and 'sat'
QUANTITIES = ('hid', 'logit', 'y_pred', 'loss', 'U', 'W', 'Wd', 'b', 'bd')


def _case(name, seed, m=40, n=70, h=20, B=16, co=0.5, hub=None, special=None):
    return dict(name=name, seed=seed, m=m, n=n, h=h, B=B, co=co, hub=hub, special=special)


CASES = [_case('h%d' % h, 100 + h, h=h) for h in (2, 33, 64, 128)]
CASES += [_case('B1', 201, B=1), _case('B5', 205, B=5)]
CASES += [_case('twice', 301, special='twice'), _case('empty', 302, special='empty'), _case('hub', 303, h=33, hub=HUB, special='hub')]
CASES += [_case('low', 304, special='low'), _case('sat', 305, special='sat')]
CASES += [_case('keep01', 401, co=0.1, m=60, n=90, B=32), _case('keep1', 402, co=1.0), _case('big', 403, m=300, n=500, h=64, B=64)]
BY_NAME = {c['name']: c for c in CASES}
GPU_CASES = [c['name'] for c in CASES]
_cache = {}


def _data(rs, m, n):
    """User 0 has no items, user 1 has 40 (five parts at hub 8), user 2 has one; counts 1 .. 3."""
    deg = rs.randint(1, 9, size=m)
    deg[0], deg[1], deg[2] = 0, 40, 1
    ev_u, ev_t = [], []
    for u, d in enumerate(deg):
        for t in rs.choice(n, size=int(d), replace=False):
            for _ in range(int(rs.randint(1, 4))):
                ev_u.append(u); ev_t.append(int(t))
    return cd.user_csr(ev_u, ev_t, m)


def build(name):
    """dict with the data, the parameters p, the batch (users, sptr, sitems), co, mask_seed, step, the fp64 yardstick ('loss', 'g',
    'fw'), 'd32', 'L' (the longest sum behind every quantity) and 'logit_max' (over the columns other than SPECIAL)."""
    if name in _cache:
        return _cache[name]
    c = dict(BY_NAME[name])
    rs = np.random.RandomState(c['seed'])
    m, n, h, B, co, special = c['m'], c['n'], c['h'], c['B'], c['co'], c['special']
    data = _data(rs, m, n)
    ptr, items, cnt = data
    p = cd.init_params(rs, m, n, h, STDDEV)
    users = [int(u) for u in rs.randint(3, m, size=B)]
    mask_seed, step = c['seed'] * 7919, 3
    if special == 'twice' and B > 1:
        users[1] = users[0]
    if special == 'hub':
        users[0] = 1
    if special == 'empty':
        users[0], users[1] = 0, 2                                # no items at all; one item, dropped at the step chosen here
        item = items[ptr[2]:ptr[3]]
        step = next(t for t in range(1, 200) if not cd.kept(mask_seed, t, 1, item, co)[0])
    sets = []
    for s, u in enumerate(users):                               # the reference's sample: the user's items and 5 draws per item
        mine = [int(i) for i in items[ptr[u]:ptr[u + 1]]]
        sets.append(set(mine) | set(int(i) for i in rs.randint(0, n, size=5 * len(mine))))
    sets[0] |= {0, n - 1}                                       # both ends of the item axis
    if special in ('hub', 'low', 'sat'):
        for s in sets:
            s.add(SPECIAL)                                      # one item sampled by every slot
    if special in ('low', 'sat'):
        p['bd'][SPECIAL] = -20.0 if special == 'low' else 40.0
        p['Wd'][:, SPECIAL] *= np.float32(0.01)
    sptr, sitems = cd.sample_csr(sets)
    c.update(data=data, p=p, users=users, sets=sets, sptr=sptr, sitems=sitems, mask_seed=mask_seed, step=step)
    args = (data, users, sptr, sitems, co, mask_seed, step, REG)
    p64 = {k: v.astype(np.float64) for k, v in p.items()}
    loss, g, fw = cd.loss_and_grad(p64, *args, dtype=np.float64)
    loss32, g32, fw32 = cd.loss_and_grad(p, *args, dtype=np.float32)
    assert fw32['hid'].dtype == np.float32 and fw32['logit'].dtype == np.float32 and all(g32[k].dtype == np.float32 for k in cd.NAMES)
    c.update(loss=float(loss), g=g, fw=fw, loss32=float(loss32), saturated=fw32['saturated'])
    d32 = {'hid': cd.rel(fw32['hid'], fw['hid']), 'logit': cd.rel(fw32['logit'], fw['logit']), 'y_pred': cd.rel(fw32['y_pred'], fw['y_pred'])}
    if not fw32['saturated']:
        d32['loss'] = abs(float(loss32) - float(loss)) / abs(float(loss))
        for k in cd.NAMES:
            d32[k] = cd.rel(g32[k], g[k])
    c['d32'] = d32
    S = int(sptr[-1])
    per_item = np.bincount(sitems[:S].astype(np.int64), minlength=n) if S else np.zeros(n, np.int64)
    longest_in = max(int(ptr[u + 1] - ptr[u]) for u in users)
    c['L'] = {'hid': longest_in + 2, 'logit': h + 1, 'y_pred': h + 1, 'loss': S + 5 + B, 'U': 2 * int(np.bincount(users).max()), 'W': int(per_item.max()) + 1,
              'Wd': int(per_item.max()) + 1, 'b': B + 1, 'bd': int(per_item.max()) + 1}
    other = fw['col'] != SPECIAL if special in ('low', 'sat') else np.ones(S, bool)
    c['logit_max'] = float(np.abs(fw['logit'][other]).max()) if other.any() else 0.0
    c['special_logits'] = fw['logit'][~other]
    _cache[name] = c
    return c


def bound(c, key):
    """4 x the case's d32, but no less than L 2^-24: a d32 that happens to be 0 must not demand another summation order's bits."""
    return max(4 * c['d32'][key], c['L'][key] * 2.0 ** -24)
