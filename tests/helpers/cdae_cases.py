"""Synthetic CDAE problems from seeds, shared by tests/test_cdae_golden.py (which checks on the CPU that every case reaches its
branch and meets its conditioning statement), tests/test_gpu_cdae.py (CASES) and tests/test_gpu_cdae_edges.py (EDGE_CASES, below).
A case's yardstick (the fp64 contract tests/helpers/numpy_cdae.py) and its d32 figures (distance of the float32 contract from it)
are computed once and cached.

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
    if name in EDGE_BY_NAME:
        return build_edge(name)
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
    _cache[name] = _measure(c)
    return c


def _measure(c):
    """Adds the fp64 yardstick ('loss', 'g', 'fw'), the float32 contract's figures ('loss32', 'saturated', 'd32'), 'L' and the
    logit figures to a case that holds its data, parameters and batch."""
    data, p, users, sptr, sitems = c['data'], c['p'], c['users'], c['sptr'], c['sitems']
    ptr = data[0]
    n, h, B, special = c['n'], c['h'], c['B'], c['special']
    args = (data, users, sptr, sitems, c['co'], c['mask_seed'], c['step'], REG)
    p64 = {k: v.astype(np.float64) for k, v in p.items()}
    loss, g, fw = cd.loss_and_grad(p64, *args, dtype=np.float64)
    loss32, g32, fw32 = cd.loss_and_grad(p, *args, dtype=np.float32)
    assert fw32['hid'].dtype == np.float32 and fw32['logit'].dtype == np.float32 and all(g32[k].dtype == np.float32 for k in cd.NAMES)
    c.update(loss=float(loss), g=g, fw=fw, loss32=float(loss32), saturated=fw32['saturated'])
    d32 = {'hid': rel(fw32['hid'], fw['hid']), 'logit': rel(fw32['logit'], fw['logit']), 'y_pred': rel(fw32['y_pred'], fw['y_pred'])}
    if not fw32['saturated']:
        d32['loss'] = abs(float(loss32) - float(loss)) / abs(float(loss))
        for k in cd.NAMES:
            d32[k] = rel(g32[k], g[k])
    c['d32'] = d32
    S = int(sptr[-1])
    per_item = np.bincount(sitems[:S].astype(np.int64), minlength=n) if S else np.zeros(n, np.int64)
    longest_in = max(int(ptr[u + 1] - ptr[u]) for u in users)
    c['L'] = {'hid': longest_in + 2, 'logit': h + 1, 'y_pred': h + 1, 'loss': S + 5 + B, 'U': 2 * int(np.bincount(users).max()), 'W': int(per_item.max()) + 1,
              'Wd': int(per_item.max()) + 1, 'b': B + 1, 'bd': int(per_item.max()) + 1}
    other = fw['col'] != SPECIAL if special in ('low', 'sat') else np.ones(S, bool)
    c['logit_max'] = float(np.abs(fw['logit'][other]).max()) if other.any() else 0.0
    c['special_logits'] = fw['logit'][~other]
    return c


def rel(a, b):
    """cd.rel; 0 for a quantity without entries (a batch that samples nothing has no logits)."""
    return cd.rel(a, b) if np.size(b) else 0.0


def bound(c, key):
    """4 x the case's d32, but no less than L 2^-24: a d32 that happens to be 0 must not demand another summation order's bits."""
    return max(4 * c['d32'][key], c['L'][key] * 2.0 ** -24)


# ---- edge cases ------------------------------------------------------------------------------------------------------------
# Where CASES draw degrees, batch users and sample sizes, these set them: every list below is the loop or branch edge of
# csrc/cdae_kernels.hpp / cdae_host.hip that the case is there to reach (tests/test_cdae_golden.py asserts that it does).  Only
# the identity of a user's items, their counts 1 .. 3, the parameters and the negatives come from the seed.  A sample set is the
# user's items (ascending; a size below the degree keeps the first ones only: the device does not ask that a sample holds the
# user's items), then the slot's forced items, then draws over the item axis in seed order until the asked size is reached.
CHUNK_LENGTHS = (0, 1, 63, 64, 65, 128, 129)                    # around one and two 64-entry chunks of a wave
GRID = 8192 * 256                                               # elements in the first trip of k_cdae_dense's grid-stride loop
PARTS_HUB = 4
PART_LENGTHS = (PARTS_HUB - 1, PARTS_HUB, PARTS_HUB + 1, 2 * PARTS_HUB, 2 * PARTS_HUB + 1)     # one part, still one, ragged, two, ragged
W_STD_LONG = 0.05                                               # encoder W of the cases with rows of 63 .. 129 items: see _layout_enc
HID_RANGE = (0.01, 0.99)


def _edge(name, seed, kind, m=40, n=70, h=20, B=16, co=0.5, hub=None, w_std=STDDEV):
    return dict(name=name, seed=seed, kind=kind, m=m, n=n, h=h, B=B, co=co, hub=hub, w_std=w_std, special=None)


EDGE_CASES = [_edge('enc_chunks', 501, 'enc', m=16, n=200, B=10, w_std=W_STD_LONG),
              _edge('enc_chunks_hub96', 501, 'enc', m=16, n=200, B=10, w_std=W_STD_LONG, hub=96),
              _edge('dec_chunks', 511, 'dec', n=200, B=7), _edge('dec_chunks_h65', 512, 'dec', n=200, B=7, h=65),
              _edge('nothing', 521, 'nothing', B=2)]
EDGE_CASES += [_edge('h%d' % h, 530 + h, 'small', h=h) for h in (1, 63, 65, 127)]
EDGE_CASES += [_edge('parts', 541, 'parts', B=9, hub=PARTS_HUB), _edge('parts_b', 542, 'parts_b', B=17, hub=PARTS_HUB),
               _edge('parts_rows', 543, 'parts_rows', B=9, hub=PARTS_HUB)]
EDGE_CASES += [_edge('hub1', 551, 'small', hub=1), _edge('all_dropped', 561, 'small', co=1e-9),
               _edge('stride', 571, 'stride', n=16400, h=128, B=8)]
EDGE_BY_NAME = {c['name']: c for c in EDGE_CASES}
EDGE_NAMES = [c['name'] for c in EDGE_CASES]


def _small_deg(m):
    """User 0 has no items, user 1 has 40, user 2 has one; user u >= 3 has 1 + u % 8."""
    return [0, 40, 1] + [1 + u % 8 for u in range(3, m)]


def _layout_enc(c):
    """Users 0 .. 6 hold CHUNK_LENGTHS items, one slot each, then three ordinary users.  At stddev 0.25 a row of 129 items with
    counts up to 3 gives (X o mask) W a standard deviation near 4 and hid leaves [1e-4, 1 - 1e-7], which zeroes dz and blinds the
    checks of gW and gU; at W_STD_LONG the sum's standard deviation is 0.9 (65 kept entries, E c^2 = 4.7) and fp64 hid stays
    inside HID_RANGE, which tests/test_cdae_golden.py asserts."""
    deg = list(CHUNK_LENGTHS) + [1 + u % 8 for u in range(len(CHUNK_LENGTHS), c['m'])]
    users = list(range(c['B']))
    return dict(deg=deg, users=users, sizes=[min(c['n'], deg[u] + 10) for u in users], score_users=list(range(len(CHUNK_LENGTHS))),
                keep=[(4, 64), (6, 128)])                       # the one entry in the last chunk of the rows of 65 and 129


def _layout_dec(c):
    """Ordinary users of 1 .. 8 items, each once; sample sets of exactly CHUNK_LENGTHS entries (the set of one entry belongs to
    the user of one item, the empty one to a user of four)."""
    deg = [1 + u % 8 for u in range(c['m'])]
    return dict(deg=deg, users=[3, 0, 1, 2, 4, 5, 6], sizes=list(CHUNK_LENGTHS), keep=[(0, 0)])


def _layout_nothing(c):
    return dict(deg=_small_deg(c['m']), users=[0, 0], sizes=[0, 0])


def _layout_small(c):
    """The standard small shape: the three special users, one user twice, eleven more."""
    deg = _small_deg(c['m'])
    users = [0, 1, 2, 5, 5] + list(range(6, c['m'], 3))[:11]
    return dict(deg=deg, users=users, sizes=[min(c['n'], 6 * deg[u] + 2) for u in users], score_users=[0, 1, 2, c['m'] - 1])


def _layout_parts(c):
    """B = 2 hub + 1; user 3 (5 items) in five slots, user 4 (8 items) in four; they share item 10 (an input of all nine slots);
    items 60 .. 64 are nobody's input and are sampled by exactly 3, 4, 5, 8 and 9 slots."""
    deg = _small_deg(c['m'])
    deg[3], deg[4] = 5, 8
    users = [3, 4, 3, 4, 3, 4, 3, 4, 3]
    slots = {60: [0, 4, 8], 61: [1, 3, 5, 7], 62: [0, 2, 4, 6, 8], 63: [0, 1, 3, 4, 5, 6, 7, 8], 64: list(range(9))}
    forced = [[i for i in sorted(slots) if s in slots[i]] for s in range(9)]
    return dict(deg=deg, fixed={3: [10], 4: [10]}, forbid=set(slots), users=users, forced=forced,
                sizes=[deg[u] + len(forced[s]) + 4 for s, u in enumerate(users)], sampled_by=dict((i, len(v)) for i, v in slots.items()))


def _layout_parts_b(c):
    """B = 4 hub + 1; user 3 (3 items) in eight slots, user 4 (4 items) in nine; item 10 is an input of all seventeen."""
    deg = _small_deg(c['m'])
    deg[3], deg[4] = 3, 4
    users = [4, 3] * 8 + [4]
    return dict(deg=deg, fixed={3: [10], 4: [10]}, forbid=set(), users=users, sizes=[deg[u] + 6 for u in users])


def _layout_parts_rows(c):
    """B = 2 hub + 1; users 3 .. 7 of 3, 4, 5, 8 and 9 items in 1, 1, 2, 2 and 3 slots.  Items 10 .. 14 are held by all five users,
    by all but user 3, by users 5 and 7, by users 4 and 7, and by user 7 alone: 9, 8, 5, 4 and 3 slots.  Nobody else holds them
    and no negative draws them, so they are also sampled by exactly that many slots."""
    deg = _small_deg(c['m'])
    deg[3:8] = PART_LENGTHS
    fixed = {3: [10], 4: [10, 11, 13], 5: [10, 11, 12], 6: [10, 11], 7: [10, 11, 12, 13, 14]}
    users = [7, 3, 5, 6, 7, 4, 5, 6, 7]
    return dict(deg=deg, fixed=fixed, forbid={10, 11, 12, 13, 14}, users=users, sizes=[deg[u] + 6 for u in users],
                held_by={10: 9, 11: 8, 12: 5, 13: 4, 14: 3})


def _layout_stride(c):
    """n h = GRID + 2048: the last 16 item rows (16384 ..) lie in the second trip of k_cdae_dense's loop.  Of those rows, user 9
    holds 16385, 16388, 16395 and 16399 (inputs of slot 2), slot 0 samples 16390 as a negative, and the other eleven are in no
    user's list and no sample (map < 0: decay alone).  Every other item of the data and every drawn negative lies below 16384."""
    deg = _small_deg(c['m'])
    deg[9] = 6
    users = [3, 6, 9, 12, 15, 18, 21, 24]
    forced = [[16390]] + [[] for _ in users[1:]]
    return dict(deg=deg, fixed={9: [16385, 16388, 16395, 16399]}, forbid=set(range(16384, 16400)), users=users, forced=forced,
                sizes=[6 * deg[u] + 2 + len(forced[s]) for s, u in enumerate(users)], keep=[(2, 5)], drop=[(2, 4)])   # 16399 kept, 16395 dropped


_LAYOUTS = {'enc': _layout_enc, 'dec': _layout_dec, 'nothing': _layout_nothing, 'small': _layout_small, 'parts': _layout_parts,
            'parts_b': _layout_parts_b, 'parts_rows': _layout_parts_rows, 'stride': _layout_stride}


def build_edge(name):
    """build()'s dict for a case of EDGE_CASES, plus 'layout' (what the case set: deg, users, sizes, ...)."""
    if name in _cache:
        return _cache[name]
    c = dict(EDGE_BY_NAME[name])
    rs = np.random.RandomState(c['seed'])
    m, n, h = c['m'], c['n'], c['h']
    lay = _LAYOUTS[c['kind']](c)
    deg, fixed, forbid, users = lay['deg'], lay.get('fixed', {}), lay.get('forbid', set()), lay['users']
    forced = lay.get('forced', [[] for _ in users])
    assert len(deg) == m and len(users) == c['B'] == len(lay['sizes']) == len(forced)
    ev_u, ev_t = [], []
    for u, d in enumerate(deg):
        given = fixed.get(u, [])
        pool = np.setdiff1d(np.arange(n), sorted(forbid | set(given)))
        for t in given + [int(t) for t in rs.choice(pool, size=d - len(given), replace=False)]:
            ev_u += [u] * int(rs.randint(1, 4)); ev_t += [t] * (len(ev_u) - len(ev_t))
    data = cd.user_csr(ev_u, ev_t, m)
    ptr, items, cnt = data
    assert np.diff(ptr).tolist() == deg
    p = cd.init_params(rs, m, n, h, STDDEV)
    if c['w_std'] != STDDEV:
        p['W'] = rs.normal(0.0, c['w_std'], size=(n, h)).astype(np.float32)
    sets = []
    for s, u in enumerate(users):
        size = lay['sizes'][s]
        mine = [int(i) for i in items[ptr[u]:ptr[u + 1]]]
        one = set(mine[:size]) | set(forced[s])
        assert len(one) <= size <= n - len(forbid)
        while len(one) < size:
            i = int(rs.randint(0, n))
            if i not in forbid:
                one.add(i)
        sets.append(one)
    sptr, sitems = cd.sample_csr(sets)
    mask_seed = c['seed'] * 7919

    def flag(t, slot, entry):
        u = users[slot]
        return bool(cd.kept(mask_seed, t, slot, items[ptr[u]:ptr[u + 1]], c['co'])[entry])
    # the first step from 3 on whose mask keeps the entries of lay['keep'] and drops those of lay['drop'] ((slot, entry) pairs)
    step = next(t for t in range(3, 200) if all(flag(t, *e) for e in lay.get('keep', [])) and not any(flag(t, *e) for e in lay.get('drop', [])))
    c.update(data=data, p=p, users=users, sets=sets, sptr=sptr, sitems=sitems, mask_seed=mask_seed, step=step, layout=lay)
    _cache[name] = _measure(c)
    return c


def families(c):
    """The lengths of everything the device cuts at cdae_hub, counted with Python sets (not numpy_cdae.hub_counts' way): encoder
    rows, sampled entries by item, input entries by item, slots by user, the whole batch."""
    ptr, items, _ = c['data']
    users, sets = c['users'], c['sets']
    sampled, held, slots = {}, {}, {}
    for s, u in enumerate(users):
        slots[u] = slots.get(u, 0) + 1
        for i in sets[s]:
            sampled[i] = sampled.get(i, 0) + 1
        for i in items[ptr[u]:ptr[u + 1]].tolist():
            held[i] = held.get(i, 0) + 1
    return {'rows': [int(ptr[u + 1] - ptr[u]) for u in users], 'sampled': sampled, 'inputs': held, 'users': slots, 'batch': [len(users)]}


def family_lengths(c):
    return {k: sorted(v.values() if isinstance(v, dict) else v) for k, v in families(c).items()}


def hubs_and_parts(c, hub):
    """(hubs, parts) from family_lengths: every length above `hub` is a hub of ceil(length / hub) parts."""
    big = [x for v in family_lengths(c).values() for x in v if x > hub]
    return len(big), sum(-(-x // hub) for x in big)
