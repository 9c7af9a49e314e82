"""Synthetic FISM problems from seeds, shared by tests/test_fism_golden.py (which checks on the CPU that every case reaches
the branch it is named for and that the oracle's result is finite) and tests/test_gpu_fism_edges.py.  A case carries the form
yue_fism_rounds must take for it -- restated here from the arithmetic of yue_amd/csrc/fism_host.hip -- and its NumPy-oracle
results (oracle/numpy_fism.py: fism_epoch / fism_rounds), computed once per (case, round size) and cached."""
import numpy as np

from oracle.numpy_fism import fism_epoch, fism_rounds

LDS_BYTES = 160 * 1024                       # gfx950: LDS of one CU, all of it one workgroup's if asked for
CUS = (64, 256, 304)                         # compute units of this family's parts: no case's form may depend on the count
S64 = [0, 1, 5, 12, 1, 16, 2, 0, 7, 9, 3, 16, 16]       # events per user; with rho = 3 a user of 16 events touches 64 rows
S9 = [0, 1, 3, 2, 3, 1, 3, 0, 2]                        # with rho = 2: 9 touches, an odd rows_cap
WIDTHS = (1, 63, 64, 65, 100, 127, 128, 129, 192, 193, 212, 256)
LR, REG_I, REG_B, ALPHA = 0.02, 0.01, 0.03, 0.5
OPTION_PAIRS = ((1, 1), (1, 0), (0, 1))      # (fism_lds, fism_inplace)


def kr_of(k):
    # host_common.hpp: registers per lane and row
    return 1 if k <= 64 else 2 if k <= 128 else 4


def cnt_max(sizes, rho):
    return max([s + s * rho for s in sizes if s > 1] or [0])


def lds_bytes(sizes, rho, k):
    return cnt_max(sizes, rho) * (12 * k + 8)


def host_form(sizes, rho, k, round_users, cus, lds=1):
    """fism_host.hip: 0 = k_fism_round, 1 = k_fism_round_lds<KR, false>, 2 = k_fism_round_lds<KR, true>."""
    c, b = cnt_max(sizes, rho), lds_bytes(sizes, rho, k)
    if not lds or not 1 <= c <= 64 or b > LDS_BYTES:
        return 0
    rows = (b + 7) & ~7
    start = 2 * rows <= LDS_BYTES and min(len(sizes), round_users) <= cus * (LDS_BYTES // (2 * rows))
    return 2 if start else 1


def _case(name, seed, sizes, rho, k, n=50, rounds=(1, 5, 100), epoch=True, items='lower', lr=LR, special=None):
    return dict(name=name, seed=seed, sizes=list(sizes), rho=rho, k=k, n=n, rounds=tuple(rounds), epoch=epoch, items=items, lr=lr, special=special)


T68 = S64 + [17]                                       # one user of 17 events: 68 touches, the whole call takes form 0
T63 = [0, 1, 5, 21, 2, 7, 21, 3]                       # rho = 2: 63 touches
TWO = [3, 16, 0, 5, 2]                                 # user 1: 16 events on one item, 48 negatives on one other item
BIG = (S64 * 47)[:600]

CASES = [_case('S64_k%d' % k, 1000 + k, S64, 3, k) for k in WIDTHS]
CASES += [_case('S9_k%d' % k, 2000 + k, S9, 2, k) for k in WIDTHS]
CASES += [_case('T68', 3001, T68, 3, 100, rounds=(1, 100)), _case('T63', 3002, T63, 2, 65, rounds=(1, 100)),
          _case('two_rows', 3003, TWO, 3, 100, rounds=(1, 100), special='two_rows')]
CASES += [_case('big_round', 3004, BIG, 3, 100, n=300, rounds=(600, 40, 41), epoch=False, items='popular', lr=0.002)]
CASES += [_case('own_k%d' % k, 3100 + k, S64, 3, k, special='own') for k in (64, 100)]
CASES += [_case('grid_n', 3201, S9, 2, 1, n=262200, rounds=(4,), epoch=False, items='top'),
          _case('grid_nk', 3202, S9, 2, 256, n=1100, rounds=(4,), epoch=False, items='spread')]
BY_NAME = {c['name']: c for c in CASES}
WIDTH_CASES = [c['name'] for c in CASES if c['name'][:4] in ('S64_', 'S9_k')]
_cache = {}


def coefs(ptr, alpha=ALPHA):
    return np.array([pow(int(nu) - 1, -alpha) if nu > 1 else 0.0 for nu in np.diff(ptr)], np.float64)


def build(name):
    """dict with user_ptr, ev_i, negs, coef, the start model P0 / Q0 / B0 and form[round_users] (the same for every CU count)."""
    if name in _cache:
        return _cache[name]
    c = dict(BY_NAME[name])
    rng = np.random.RandomState(c['seed'])
    sizes, rho, n, k = c['sizes'], c['rho'], c['n'], c['k']
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    E = int(ptr[-1])
    if c['items'] == 'lower':                                   # the lower half of the catalogue, repeats inside a user
        ev_i = rng.randint(0, n // 2, E)
    elif c['items'] == 'popular':                               # a popular head: rows that many users of a round share
        pop = 1.0 / np.arange(1, n + 1) ** 0.8
        ev_i = rng.choice(n, size=E, p=pop / pop.sum())
    elif c['items'] == 'spread':                                # the whole catalogue, its last item among them
        ev_i = rng.randint(0, n, E)
        ev_i[::3] = rng.randint(n - 60, n, len(ev_i[::3]))
        ev_i[ptr[2]] = n - 1                                   # (user 2 is the first with more than one event)
    else:                                                       # 'top': items on both sides of 262,144 and the last one
        ev_i = np.where(rng.rand(E) < 0.5, rng.randint(0, 262144, E), rng.randint(262144, n, E))
        ev_i[ptr[2]], ev_i[ptr[2] + 1] = n - 1, 262144          # (user 2 is the first with more than one event)
    ev_i = ev_i.astype(np.int32)
    if c['special'] == 'two_rows':
        ev_i[ptr[1]:ptr[2]] = 7
    negs = []
    for u, s in enumerate(sizes):
        if s > 1:
            mine = set(ev_i[ptr[u]:ptr[u + 1]].tolist())
            if c['items'] == 'top':                             # (both sides of 262,144 again; a draw that names one of the user's items moves down)
                d = [int(x) for x in np.where(rng.rand(s * rho) < 0.5, rng.randint(0, 262144, s * rho), rng.randint(262144, n, s * rho))]
                if u == 4:
                    d[0], d[1] = n - 2, 262145
                for t in range(len(d)):
                    while d[t] in mine:
                        d[t] -= 1
            else:                                               # rejection against the user's items, as FISM.py:50-53
                free = [x for x in range(n) if x not in mine]
                d = [int(rng.choice(free)) for _ in range(s * rho)]
            if c['special'] == 'two_rows' and u == 1:
                d = [31] * (s * rho)
            if c['special'] == 'own':                           # every third draw names ANOTHER item of the same user
                for t in range(0, s * rho, 3):
                    others = sorted(mine - {int(ev_i[ptr[u] + t // rho])})
                    if others:
                        d[t] = int(rng.choice(others))
            negs += d
    negs = np.array(negs, np.int32)
    c.update(user_ptr=ptr, ev_i=ev_i, negs=negs, coef=coefs(ptr), cnt_max=cnt_max(sizes, rho), lds_bytes=lds_bytes(sizes, rho, k),
             P0=rng.rand(n, k) / 100, Q0=(rng.rand(n, k) / 10).astype(np.float32), B0=rng.rand(n) / 100)
    forms = {}
    for U in c['rounds']:
        per_cu = set(host_form(sizes, rho, k, U, cus) for cus in CUS)
        assert len(per_cu) == 1, (name, U, per_cu)
        forms[U] = per_cu.pop()
    c['form'] = forms
    _cache[name] = c
    return c


def oracle(name, round_users=None):
    """(half, P, Q, Bi) of the NumPy oracle: fism_epoch (round_users None) or fism_rounds.  Cached; callers must not write to it."""
    key = (name, round_users)
    if key not in _cache:
        c = build(name)
        P, Q, Bi = c['P0'].copy(), c['Q0'].copy(), c['B0'].copy()
        if round_users is None:
            half = fism_epoch(P, Q, Bi, c['user_ptr'], c['ev_i'], c['negs'], c['rho'], ALPHA, c['lr'], REG_I, REG_B)
        else:
            half = fism_rounds(P, Q, Bi, c['user_ptr'], c['ev_i'], c['negs'], c['rho'], ALPHA, c['lr'], REG_I, REG_B, round_users)
        for a in (P, Q, Bi):
            a.flags.writeable = False
        _cache[key] = (float(half), P, Q, Bi)
    return _cache[key]


def touched(c):
    """bool [n]: items some user with more than one event touches (its events' items and its negatives)."""
    t = np.zeros(c['n'], bool)
    ptr = c['user_ptr']
    for u, s in enumerate(c['sizes']):
        if s > 1:
            t[c['ev_i'][ptr[u]:ptr[u + 1]]] = True
    t[c['negs']] = True
    return t


# ---------------------------------------------------------------------------------------------
# selection: a model whose item rows come in identical groups, so that equal scores sit in the seed, at the last slot and in the scan
# ---------------------------------------------------------------------------------------------
SEL_N, SEL_K = 160, 8


def selection_model(N, seed=77):
    """(P, Q, Bi, groups): six groups of identical item rows (leader's P, Q, Bi copied into the members) with members on both
    sides of position N of the item order (N = 1: the first group alone starts below it), raised so that they fill the head of
    every list; a seventh, wide group follows them."""
    rng = np.random.RandomState(seed + N)
    n, k = SEL_N, SEL_K
    P, Q, Bi = rng.rand(n, k) / 10, (rng.rand(n, k) / 10).astype(np.float32), rng.rand(n) / 100
    taken, groups = set(), []
    for q in range(6):
        want = [q, q + 6, N - 1 - q, N + q, N + 7 + q, n - 1 - q]
        g = []
        for x in want:
            if 0 <= x < n and x not in taken:
                taken.add(x)
                g.append(x)
        g.sort()
        Bi[g[0]] += 0.5 + 0.05 * ((q * 5) % 6)                  # (group order by score differs from group order by id)
        for x in g[1:]:
            P[x], Q[x], Bi[x] = P[g[0]], Q[g[0]], Bi[g[0]]
        groups.append(g)
    # ... and a wide group below them and above the rest, in which the last slot of a long list comes to lie
    g = [x for x in range(n) if x not in taken and x % 4 != 3]
    Bi[g[0]] += 0.3
    for x in g[1:]:
        P[x], Q[x], Bi[x] = P[g[0]], Q[g[0]], Bi[g[0]]
    groups.append(g)
    return P, Q, Bi, groups


def selection_rows(N, seed=78):
    """65 listed users' training rows for selection_model(N): [0] empty, [1] unsorted with duplicates, [2] exactly N candidates
    left, the others a few random items (some of them group members)."""
    rng = np.random.RandomState(seed + N)
    rows = [np.zeros(0, np.int32), np.array([9, 3, 150, 3, 9, 0, 41, 3], np.int32), rng.permutation(SEL_N)[:SEL_N - N].astype(np.int32)]
    rows += [rng.randint(0, SEL_N, rng.randint(1, 9)).astype(np.int32) for _ in range(62)]
    return rows


def chain_scores(P, Q, Bi, items):
    """predict with one chain per item (identical rows give bit-equal scores, as on the device; NumPy's matrix-vector product
    does not promise that)."""
    hist = np.zeros(P.shape[1])
    for it in items:
        hist += P[int(it)]
    Qd = Q.astype(np.float64)
    return Bi + (Qd * hist).sum(axis=1) - (P * Qd).sum(axis=1)


def variant_scan(scores, masked, N, sort_le=False, last_le=False, scan_gt=False):
    """oracle/numpy_fism.py: overwrite_scan with one of its three comparisons moved by an equality (all False: the scan itself):
    sort_le = an equal score passes an earlier one in the seed's sort, last_le = a score equal to the last slot enters,
    scan_gt = the overwrite lands on the first slot not above the score."""
    masked = set(int(x) for x in masked)
    cand = [t for t in range(len(scores)) if t not in masked]
    vals, ids = [], []
    for t in cand[:N]:
        pos = len(vals)
        while pos > 0 and (vals[pos - 1] <= scores[t] if sort_le else vals[pos - 1] < scores[t]):
            pos -= 1
        vals.insert(pos, scores[t])
        ids.insert(pos, t)
    if len(ids) < N:
        raise IndexError('fewer than N candidates')
    for t in cand:
        s = scores[t]
        if (vals[N - 1] <= s) if last_le else (vals[N - 1] < s):
            p = 0
            while p < N - 1 and (vals[p] > s if scan_gt else vals[p] >= s):
                p += 1
            vals[p], ids[p] = s, t
    return ids, vals
