"""CPU: oracle/numpy_fism.py (the NumPy restatement of the reference's FISM) against outputs of the reference
itself (tests/golden/g8_*, made by tools/make_goldens.py).  The restatement issues the reference's NumPy
operations, so everything is compared for equality.  Below them: the synthetic cases of tests/test_gpu_fism_edges.py
(tests/helpers/fism_cases.py), each checked to reach the branch of the device path it is named for."""
import numpy as np
import pytest

from util import gj, gz

CASES = ['fism_c1_k10_e2', 'fism_d2_k64_e1', 'fism_d3_k130_e3']
LR0, REG = 0.015, 0.01            # FISM.conf: learnRate -init 0.015, reg.lambda -u/-i/-b 0.01


def fism_case(tag):
    z, meta = gz('g8_%s.npz' % tag), gj('g8_%s.json' % tag)
    m = int(z['m'])
    ptr = np.zeros(m + 1, np.int64)
    np.add.at(ptr, z['ev_u'].astype(np.int64) + 1, 1)
    return z, meta, np.cumsum(ptr)


def bold_driver(lr, last, loss, iteration, max_lr=1.0):
    # base/IterativeRecommender.py:47-75 (the lines FISM inherits)
    if not abs(last - loss) < 1e-3:
        if iteration > 1:
            lr = lr * 1.01 if abs(last) > abs(loss) else lr * 0.5
        lr = min(lr, max_lr)
    return lr


@pytest.mark.parametrize('tag', CASES)
def test_numpy_fism_lands_on_the_reference(tag):
    from oracle.numpy_fism import fism_epoch, fism_regulariser, fism_scores, overwrite_scan
    z, meta, ptr = fism_case(tag)
    assert meta['dtypes'] == ['float64', 'float32', 'float64']
    iters, rho, alpha = int(z['iters']), int(z['rho']), float(z['alpha'])
    P, Q, Bi = z['P0'].copy(), z['Q0'].copy(), z['B0'].copy()
    per = len(z['negs']) // iters
    lr, last = LR0, 0
    for ep in range(iters):
        half = fism_epoch(P, Q, Bi, ptr, z['ev_i'], z['negs'][ep * per:(ep + 1) * per], rho, alpha, lr, REG, REG)
        loss = half + fism_regulariser(P, Q, Bi, REG, REG, REG)
        assert 'FISM [1] iteration %d: loss = %.4f, delta_loss = %.5f learning_Rate = %.5f' % (ep + 1, loss, last - loss, lr) == meta['lines'][ep]
        lr = bold_driver(lr, last, loss, ep + 1)
        last = loss
    assert np.array_equal(P, z['P']) and np.array_equal(Q, z['Q']) and np.array_equal(Bi, z['Bi'])
    assert loss == float(z['loss']) and lr == float(z['lRate'])
    tu, N = z['test_users'], z['rec_ids'].shape[1]
    for t in range(16):
        u = int(tu[t])
        assert np.array_equal(fism_scores(P, Q, Bi, z['ev_i'][ptr[u]:ptr[u + 1]]), z['predict16'][t])
    for t in range(0, len(tu), 7):
        items = z['ev_i'][ptr[int(tu[t])]:ptr[int(tu[t]) + 1]]
        assert overwrite_scan(fism_scores(P, Q, Bi, items), items, N)[0] == list(z['rec_ids'][t])


def test_fism_negatives_follow_the_draw_log():
    # the accepted negatives are the logged draws minus the rejected ones (FISM.py:50-53), users with one event skipped
    z, _, ptr = fism_case('fism_d2_k64_e1')
    rho = int(z['rho'])
    it = iter(z['draws'].tolist())
    got = []
    for u in range(len(ptr) - 1):
        items = set(z['ev_i'][ptr[u]:ptr[u + 1]].tolist())
        if ptr[u + 1] - ptr[u] == 1:
            continue
        for _ in range((ptr[u + 1] - ptr[u]) * rho):
            j = next(it)
            while j in items:
                j = next(it)
            got.append(j)
    assert got == z['negs'].tolist() and next(it, None) is None


def test_rounds_of_one_user_are_the_reference_pass():
    # oracle/numpy_fism.py: fism_rounds with one user per round against the reference's own output (pins the round oracle)
    from oracle.numpy_fism import fism_rounds
    z, meta, ptr = fism_case('fism_c1_k10_e2')
    iters, rho, alpha = int(z['iters']), int(z['rho']), float(z['alpha'])
    P, Q, Bi = z['P0'].copy(), z['Q0'].copy(), z['B0'].copy()
    per = len(z['negs']) // iters
    half = fism_rounds(P, Q, Bi, ptr, z['ev_i'], z['negs'][:per], rho, alpha, LR0, REG, REG, 1)
    from oracle.numpy_fism import fism_epoch
    Pe, Qe, Be = z['P0'].copy(), z['Q0'].copy(), z['B0'].copy()
    half_e = fism_epoch(Pe, Qe, Be, ptr, z['ev_i'], z['negs'][:per], rho, alpha, LR0, REG, REG)
    # x + (x' - x) may differ from x' in the last float32 bit of a Q element; what later users read from it moves the
    # float64 arrays by as much
    assert np.abs(P - Pe).max() <= 1e-6 * np.abs(Pe).max() and np.abs(Bi - Be).max() <= 1e-6 * np.abs(Be).max()
    assert np.abs(Q - Qe).max() <= 1e-6 * np.abs(Qe).max() and abs(half - half_e) <= 1e-6 * half_e
    # larger rounds move away from the sequential pass, but only slightly on this data
    P8, Q8, B8 = z['P0'].copy(), z['Q0'].copy(), z['B0'].copy()
    half8 = fism_rounds(P8, Q8, B8, ptr, z['ev_i'], z['negs'][:per], rho, alpha, LR0, REG, REG, 8)
    assert abs(half8 - half_e) < 0.02 * half_e and np.abs(Q8 - Qe).max() > 0


# ---------------------------------------------------------------------------------------------
# the synthetic cases of tests/test_gpu_fism_edges.py (tests/helpers/fism_cases.py): every case reaches the branch it is named for
# ---------------------------------------------------------------------------------------------
def _case_names():
    from helpers import fism_cases as fc
    return [c['name'] for c in fc.CASES]


@pytest.mark.parametrize('name', _case_names())
def test_edge_cases_reach_their_branches_and_the_oracle_stays_finite(name):
    from helpers import fism_cases as fc
    c = fc.build(name)
    ptr, ev_i, negs, rho, k, n = c['user_ptr'], c['ev_i'], c['negs'], c['rho'], c['k'], c['n']
    sizes = np.diff(ptr)
    assert len(negs) == sum(s * rho for s in sizes if s > 1) and 0 <= negs.min() and negs.max() < n and 0 <= ev_i.min() and ev_i.max() < n
    assert (sizes == 0).any() and (sizes == 1).any() or name == 'two_rows'          # users the loop skips, among the others
    # no draw names its own event's item; only the 'own' cases name another item of the same user
    t, shared = 0, 0
    for u, s in enumerate(sizes):
        if s > 1:
            mine = set(ev_i[ptr[u]:ptr[u + 1]].tolist())
            for e in range(ptr[u], ptr[u + 1]):
                for _ in range(rho):
                    assert negs[t] != ev_i[e], (name, t)
                    shared += int(negs[t]) in mine
                    t += 1
    print(name, 'k', k, 'KR', fc.kr_of(k), 'cnt_max', c['cnt_max'], 'lds bytes', c['lds_bytes'], 'forms', c['form'], 'draws on own items', shared)
    if c['special'] == 'own':
        multi = [u for u, s in enumerate(sizes) if s > 1 and len(set(ev_i[ptr[u]:ptr[u + 1]].tolist())) > 1]
        assert shared >= len(multi) >= 8
    else:
        assert shared == 0
    # the forms, from the host's arithmetic (the same for 64, 256 and 304 CUs: asserted in build)
    if name.startswith('S64_k'):
        assert c['cnt_max'] == 64 and all(f == (2 if k <= 100 else 1 if k <= 212 else 0) for f in c['form'].values())
        assert (k == 212) == (163328 == c['lds_bytes']) and (c['lds_bytes'] <= fc.LDS_BYTES) == (k <= 212)
    if name.startswith('S9_k'):
        assert c['cnt_max'] == 9 and all(f == 2 for f in c['form'].values())
        assert (c['cnt_max'] * k) % 2 == k % 2                                     # odd k: the padded float block of the START layout
        assert (c['lds_bytes'] % 8 == 4) == (k % 2 == 1)                           # ... and lds_rows rounds up
    if name.startswith(('S64_k', 'S9_k')):
        # repeats inside a user, an item shared by two users
        assert any(len(set(ev_i[ptr[u]:ptr[u + 1]].tolist())) < s for u, s in enumerate(sizes) if s > 1) or name.startswith('S9_k')
        assert ev_i.max() < n // 2 and set(c['rounds']) == {1, 5, 100} and c['epoch']
    if name == 'T68':
        assert c['cnt_max'] == 68 and sorted(sizes)[-2] == 16 and set(c['form'].values()) == {0} and fc.kr_of(k) == 2
    if name == 'T63':
        assert c['cnt_max'] == 63 and (63 * k) % 2 == 1 and set(c['form'].values()) == {2}
    if name == 'two_rows':
        assert c['cnt_max'] == 64 and set(ev_i[ptr[1]:ptr[2]].tolist()) == {7} and set(negs[9:9 + 48].tolist()) == {31} and set(c['form'].values()) == {2}
    if name == 'big_round':
        assert len(sizes) == 600 and c['cnt_max'] == 64 and c['form'] == {600: 1, 40: 2, 41: 2} and 600 % 41 != 0
        assert 2 * c['lds_bytes'] <= fc.LDS_BYTES < 3 * c['lds_bytes']             # one workgroup of the doubled size per CU: 600 > CUs
        assert np.bincount(ev_i, minlength=n).max() > 100                          # the popular head
    if name == 'grid_n':
        assert n * k > 262144 and n > 262144 and c['form'] == {4: 2}
        assert n - 1 in ev_i[ptr[2]:] and (ev_i[1:] >= 262144).sum() > 3 and (negs >= 262144).sum() > 3 and (negs < 262144).sum() > 3
    if name == 'grid_nk':
        assert n * k > 262144 >= n and c['form'] == {4: 2} and fc.kr_of(k) == 4
        assert n - 1 in ev_i[ptr[2]:] and (ev_i[1:].astype(np.int64) * k >= 262144).sum() > 3 and (negs.astype(np.int64) * k >= 262144).sum() >= 3
    if name.startswith('grid'):
        assert 0 < fc.touched(c).sum() < 60                                        # most rows stay as uploaded
    # with fism_lds = 0 the form is 0 whatever the case
    assert all(fc.host_form(c['sizes'], rho, k, U, 256, lds=0) == 0 for U in c['rounds'])
    for U in ([None] if c['epoch'] else []) + list(c['rounds']):
        half, P, Q, Bi = fc.oracle(name, U)
        assert np.isfinite(half) and np.isfinite(P).all() and np.isfinite(Q).all() and np.isfinite(Bi).all() and half > 0, (name, U)
        assert not np.array_equal(Q, c['Q0'])
    if c['epoch']:                                         # one user per round is the sequential pass up to x + (x' - x) rounding
        e, r = fc.oracle(name, None), fc.oracle(name, 1)
        assert np.abs(r[2] - e[2]).max() <= 1e-6 * np.abs(e[2]).max() and abs(r[0] - e[0]) <= 1e-6 * e[0]


def test_edge_widths_cover_every_register_count_and_form():
    from helpers import fism_cases as fc
    seen = set((fc.kr_of(fc.BY_NAME[name]['k']), f) for name in fc.WIDTH_CASES for f in fc.build(name)['form'].values())
    # KR = 1, 2, 4 with the round-start rows (form 2), KR = 2 and 4 without (form 1), the global form for k = 256 with 64 touches
    assert seen == {(1, 2), (2, 2), (4, 2), (2, 1), (4, 1), (4, 0)}
    assert [fc.kr_of(k) for k in fc.WIDTHS] == [1, 1, 1, 2, 2, 2, 2, 4, 4, 4, 4, 4]


@pytest.mark.parametrize('N', [1, 10, 100])
def test_selection_model_puts_equal_scores_where_the_scan_compares(N):
    """The groups of identical rows straddle position N of the candidate order, and on these scores each comparison of the
    reference's selection matters: moved by an equality it returns other ids (N = 1 has no sort and no inner scan)."""
    from helpers import fism_cases as fc
    from oracle.numpy_fism import overwrite_scan
    P, Q, Bi, groups = fc.selection_model(N)
    assert all(len(g) >= 2 and g[-1] >= N for g in groups) and sum(g[0] < N for g in groups) >= min(N, 5) and len(groups[6]) > 90
    for g in groups:
        assert all(np.array_equal(P[x], P[g[0]]) and np.array_equal(Q[x], Q[g[0]]) and Bi[x] == Bi[g[0]] for x in g)
    rows = fc.selection_rows(N)
    assert len(rows) == 65 and len(rows[0]) == 0 and len(set(rows[1].tolist())) < len(rows[1]) and list(rows[1]) != sorted(rows[1])
    assert fc.SEL_N - len(set(rows[2].tolist())) == N
    differs = {'sort_le': 0, 'last_le': 0, 'scan_gt': 0}
    for r in rows:
        s = fc.chain_scores(P, Q, Bi, r)
        for g in groups:
            assert len(set(s[g].tolist())) == 1                     # identical rows, bit-equal scores
        ids, vals = overwrite_scan(s, r, N)
        assert fc.variant_scan(s, r, N) == (ids, vals)
        for key in differs:
            differs[key] += fc.variant_scan(s, r, N, **{key: True})[0] != ids
    print('N', N, 'users whose list changes when a comparison is moved by an equality:', differs)
    assert differs['last_le'] > 0 and (N == 1 or (differs['sort_le'] > 0 and differs['scan_gt'] > 0))
    with pytest.raises(IndexError):
        overwrite_scan(fc.chain_scores(P, Q, Bi, rows[2]), np.concatenate([rows[2], [x for x in range(fc.SEL_N) if x not in set(rows[2].tolist())][:1]]), N)
