"""CPU: the edge cases of UserKNN's and IPF's ranking kernels (tests/helpers/knn_cases.py, tests/helpers/ipf_cases.py) reach the
branches they are built for, and can tell a right kernel from a wrong one.

reach        every case's `reach` (computed from its events and the NumPy oracle alone) is asserted here, so that a later edit
             of a case cannot silently leave its branch.  The GPU tests (tests/test_gpu_userknn_edges.py,
             tests/test_gpu_ipf_edges.py) run the same cases on the device.
sensitivity  per edge family, a deliberately wrong variant of the oracle (a small function below, never a wrong kernel and never a
             change to the oracle) gives another result than the oracle on that family's case.  Every comparison is exact."""
import numpy as np
import pytest

from helpers import ipf_cases as ic
from helpers import knn_cases as kc
from helpers import numpy_ipf as oi
from helpers import numpy_userknn as ok


# ---------------------------------------------------------------------------------------------------------------- reach: UserKNN
@pytest.mark.parametrize('name,cand', [('cap_1792', 1792), ('cap_1793', 1793), ('cap_2048', 2048), ('cap_2304', 2304), ('cap_2304_range64', 2304)])
def test_knn_cap_cases_stand_at_the_sort_capacity(name, cand):
    c = kc.build(name)
    r = c['reach']
    assert c['m'] == cand + 1 and r['candidates'] == [cand]                 # every checked user has exactly m - 1 candidates
    assert r['tie_at_20'] >= 1                                              # K = 20 cuts inside a group of equal ratios
    assert c['Ks'] == [1, 20, 256] and len(c['users']) == kc.SAMPLE and c['users'][0] == 0 and c['users'][-1] == c['m'] - 1
    # 1792 and 1793: the two sides of SORT_CAP - THREADS; 2048: the full capacity; 2304: a block past it
    assert r['mid_run_merge_certain'] == (cand >= kc.SORT_CAP)
    assert c['options'][0]['knn_range'] == (kc.RANGE_MIN if name.endswith('range64') else kc.RANGE)
    assert kc.SORT_CAP - kc.THREADS == 1792


@pytest.mark.parametrize('du', [255, 256, 257, 600])
def test_knn_row_cases_hold_one_long_user(du):
    c = kc.build('row_%d' % du)
    r = c['reach']
    assert r['long_row'] == du and r['users_with_long_neighbour'] >= 10 and r['counts_above_1'] > 0
    assert c['long_user'] in c['users'] and 0 in c['users'] and c['m'] - 1 in c['users']
    (up, _, _), _ = c['pairs']
    assert np.delete(np.diff(up), c['long_user']).max() <= 30
    assert [o['knn_range'] for o in c['options']] == [kc.RANGE, kc.RANGE_MIN]


@pytest.mark.parametrize('m,passes,last', [(64, 1, 64), (65, 2, 1), (128, 2, 64), (129, 3, 1)])
def test_knn_range_cases_end_on_and_past_a_pass(m, passes, last):
    c = kc.build('range_m%d' % m)
    assert c['reach'] == dict(m=m, passes=passes, last_pass=last)
    assert c['Ks'] == [10] and c['options'] == [dict(kc.DEFAULTS, knn_range=64)] and len(c['users']) == m


@pytest.mark.parametrize('K', [256, 255])
def test_knn_kp_cases_fill_every_rank(K):
    c = kc.build('kp_%d' % K)
    r = c['reach']
    assert r['kp_min'] == K and r['width_at_256'] == 1 and r['sims_differ_128_apart'] == len(c['users'])
    assert c['m'] == 300 and c['n'] <= 64 and c['Ns'] == [100, 1]
    assert [o['knn_gather'] for o in c['options']] == [kc.GATHER, kc.GATHER_MIN]
    (up, ui, _), _ = c['pairs']
    assert all(ui[up[u]] == 0 for u in range(c['m']))                       # the common item


def test_knn_gather_cases_stand_on_both_sides_of_the_chunked_decision():
    eq, over = kc.build('gather_eq'), kc.build('gather_over')
    assert eq['reach'] == dict(kp=4, entries=256, gather=256, chunked=0)
    assert over['reach'] == dict(kp=4, entries=257, gather=256, chunked=1)
    assert len(eq['users']) == 1 and len(over['users']) == 1 and eq['options'][0]['knn_gather'] == kc.GATHER_MIN


def test_knn_ones_cases_tie_every_score():
    c, f = kc.build('ones'), kc.build('ones_few2')
    r = c['reach']
    assert r['counts_max'] == 1 and r['all_scores_one'] == r['users'] == len(c['users'])
    assert r['chunked'] >= 30 and r['first7_span_chunks'] >= 10 and r['cut_at_100'] >= 10       # N = 7 and N = 100 cut a tie group across chunks
    assert c['Ns'] == [1, 7, 100] and c['options'][0]['knn_gather'] == kc.GATHER_MIN
    assert 0 < f['reach']['counts_of_2'] <= 12 and f['reach']['counts_max'] == 2 and f['reach']['some_score_above_one'] >= 10
    assert np.array_equal(c['pairs'][0][1], f['pairs'][0][1])               # the same pairs, a handful of counts apart


def test_knn_own_only_case_leaves_nothing_to_rank():
    c = kc.build('own_only')
    u = c['own_user']
    (up, ui, uc), _ = c['pairs']
    nbr, inter, uni = kc.oracle_neighbors(c, 10)
    assert c['reach']['neighbours'] == [9, 17]
    own = set(ui[up[u]:up[u + 1]])
    assert all(set(ui[up[v]:up[v + 1]]) <= own for v in c['reach']['neighbours'])
    it, sc = ok.topn(up, ui, uc, u, nbr[u], inter[u], uni[u], c['n'], 10)
    assert len(it) == 0 and len(ok.predict(up, ui, uc, nbr[u], inter[u], uni[u], c['n'])[0]) == 3


@pytest.mark.parametrize('n,blocks', [(255, 1), (256, 1), (257, 2)])
def test_knn_predict_cases_stand_at_the_block_edge(n, blocks):
    c = kc.build('predict_n%d' % n)
    assert c['reach'] == dict(n=n, blocks=blocks, last_item_scored=True) and c['n'] == n


def test_the_h_fixture_has_no_row_past_one_chunk(tmp_path):
    # tests/test_gpu_userknn.py's comment on userknn_h_k20 claims the item-range chunks of k_knn_topn (20 x 240 entries), which its
    # counter confirms; it claims nothing of the c0 loop, and could not: the 240 training events of a user (300 x 0.8) give fewer
    # distinct items than one chunk of 256 (row_256 / row_257 / row_600 reach that loop)
    from test_userknn_golden import load_case
    _, _, _, (up, _, _), _ = load_case(tmp_path, 'userknn_h_k20')
    assert 200 < np.diff(up).max() < kc.THREADS


# ---------------------------------------------------------------------------------------------------------------- reach: IPF
@pytest.mark.parametrize('L', [256, 257, 513])
def test_ipf_l1_cases_run_level_1_past_a_chunk(L):
    c = ic.build('l1_%d' % L)
    r = c['reach']
    assert r['list_len'] == L and r['events'] > L and r['K_max'] == L       # the last item of the long list has a holder
    assert (r['nodes_K_above_256'] > 0) == (L > 256) and (r['nodes_K_above_512'] > 0) == (L > 512)
    assert c['long_user'] in c['users'] and c['m'] == 101
    if L > 256:                                                             # holders of nothing but items of the second (third) chunk
        g, order = ic.graph(c), list(ic.graph(c).D[0][c['long_user']])
        assert all(min(order.index(a) for a in g.D[0][b]) >= 256 for b in range(91, 96))
        assert L <= 512 or all(min(order.index(a) for a in g.D[0][b]) >= 512 for b in range(96, 99))


@pytest.mark.parametrize('X', [255, 256, 257, 700])
def test_ipf_l2_cases_reach_that_many_level_2_nodes(X):
    c = ic.build('l2_%d' % X)
    assert c['reach'] == dict(level2_nodes=X, hub_holders=X + 1, pos_max=X)
    assert 0 in c['users'] and len(c['users']) == ic.SAMPLE


@pytest.mark.parametrize('X', [768, 769, 1024, 1500])
def test_ipf_sel_cases_fill_the_selection(X):
    c = ic.build('sel_%d' % X)
    r = c['reach']
    assert r['candidates'] == X and r['reached'] == X + r['own_reached'] and r['own_reached'] == 2
    assert r['mid_run_merge_certain'] == (X >= 1024) and c['Ns'] == [100, 1]
    assert ic.SEL - ic.THREADS == 768


def test_ipf_tie_cases_are_ordered_by_the_insertion_key():
    b, r = ic.build('beta0'), ic.build('rho0')
    assert b['beta'] == 0.0 and r['rho'] == 0.0
    for c in (b, r):
        assert c['reach']['users_with_ties_in_cut'][10] >= 10
    assert b['reach']['users_with_zero_scores_in_top'] >= 10               # zero scores inside a top-100 that is not full
    g = ic.graph(r)
    assert all((w[np.array([len(x) > 0 for x in g.UL])] == 1.0).all() for w in g.W) and set(np.unique(g.P[0])) <= {0.0, 1.0}
    for u in r['users']:
        assert np.array_equal(ic.predict(r, u)[1] * 2, np.round(ic.predict(r, u)[1] * 2))     # multiples of beta = 0.5


def test_ipf_limit_case_ends_the_k_field():
    c = ic.build('limit_k')
    assert c['reach'] == dict(list_len=(1 << 18) - 1, K_max=(1 << 18) - 1, K_field=0, n=1 << 18) and c['m'] == 3
    assert ic.MAX_LIST == (1 << ic.K_BITS) - 1
    g = ic.graph(c)
    assert list(g.D[0][1]) == [ic.MAX_LIST - 1, ic.MAX_LIST] and list(g.D[0][2]) == [ic.MAX_LIST - 1, 5]
    assert [len(ic.topn(c, u, 5)[0]) for u in (0, 1, 2)] == [1, 5, 5]       # user 0 holds every item but user 1's own
    over = ic.limit_k_over()
    assert over['u_ptr'][1] - over['u_ptr'][0] == 1 << 18 and over['n'] == 1 << 18


def test_ipf_combo_case_holds_every_kind_of_query():
    c = ic.build('combo')
    assert c['reach'] == dict(list_len=513, K_max=513, level2_nodes=700, candidates=1500, tiny=2, empty=0)
    assert c['order'][:4] == [0, 1, 2, 3]                                   # large, tiny, no events, large again


def test_ipf_replace_cases_share_one_shape_and_then_leave_it():
    A, B, C, D = (ic.build('replace_%s' % x) for x in 'ABCD')
    assert (A['m'], A['n']) == (B['m'], B['n']) and not np.array_equal(A['ev_i'], B['ev_i'])
    assert C['m'] < A['m'] and C['n'] < A['n'] and D['m'] > A['m'] and D['n'] > A['n']


# ------------------------------------------------------------------------------------------------------ sensitivity: UserKNN
def knn_neighbors_variant(c, u, K, id_desc=False):
    """ok.neighbors of one user; id_desc: ties among equal ratios in id descending order."""
    (up, ui, _), (ip, iu) = c['pairs']
    deg = np.diff(up)
    cnt = np.bincount(np.concatenate([iu[ip[i]:ip[i + 1]] for i in ui[up[u]:up[u + 1]]]), minlength=c['m']).astype(np.int64)
    cnt[u] = 0
    v = np.flatnonzero(cnt)
    U = deg[u] + deg[v] - cnt[v]
    order = np.lexsort((-v if id_desc else v, -(2.0 * cnt[v]) / U.astype(np.float64)))[:K]
    return v[order], cnt[v][order], U[order]


def knn_predict_variant(c, nbr, inter, uni, rank_mod=None):
    """ok.predict; rank_mod: the similarity looked up at rank % rank_mod."""
    (up, ui, uc), _ = c['pairs']
    total, den = np.zeros(c['n']), np.zeros(c['n'])
    for r, v in enumerate(nbr):
        if v < 0:
            break
        q = r % rank_mod if rank_mod else r
        s = float(2 * int(inter[q])) / float(uni[q])
        it = ui[up[v]:up[v + 1]]
        total[it] = total[it] + s * uc[up[v]:up[v + 1]].astype(np.float64)
        den[it] = den[it] + s
    items = np.flatnonzero(den > 0).astype(np.int32)
    scores = total[items] / den[items]
    order = np.lexsort((items, -scores))
    return items[order], scores[order]


def knn_topn_variant(c, u, items, scores, N, width=None, exclude_after_cut=False):
    """ok.topn from a predict list; width: the top-N of every item-range chunk, concatenated in chunk order and cut, instead of
    merged; exclude_after_cut: the user's own items leave after the cut at N."""
    (up, ui, _), _ = c['pairs']
    own = ui[up[u]:up[u + 1]]
    if exclude_after_cut:
        keep = ~np.isin(items[:N], own)
        return items[:N][keep], scores[:N][keep]
    keep = ~np.isin(items, own)
    items, scores = items[keep], scores[keep]
    if width:
        parts = [np.flatnonzero(items // width == ch)[:N] for ch in range(-(-c['n'] // width))]
        order = np.concatenate(parts)
        items, scores = items[order], scores[order]
    return items[:N], scores[:N]


def knn_lists(c, K):
    """Per checked user: (u, oracle neighbour row, oracle predict list)."""
    (up, ui, uc), _ = c['pairs']
    nbr, inter, uni = kc.oracle_neighbors(c, K)
    return [(int(u), (nbr[t], inter[t], uni[t]), ok.predict(up, ui, uc, nbr[t], inter[t], uni[t], c['n'])) for t, u in enumerate(c['users'])]


def same(a, b):
    return all(np.array_equal(x, y) for x, y in zip(a, b)) and len(a) == len(b)


@pytest.mark.parametrize('name', kc.FAMILIES['cap'])
def test_sensitivity_knn_tie_order(name):
    c = kc.build(name)
    nbr, inter, uni = kc.oracle_neighbors(c, 20)
    differ = 0
    for t, u in enumerate(c['users']):
        assert same(knn_neighbors_variant(c, u, 20), (nbr[t], inter[t], uni[t]))            # the variant's own base is the oracle
        differ += not np.array_equal(knn_neighbors_variant(c, u, 20, id_desc=True)[0], nbr[t])
    assert differ == len(c['users'])


def test_sensitivity_knn_rank_in_seven_bits():
    c = kc.build('kp_256')
    differ = 0
    for u, (nbr, inter, uni), (items, scores) in knn_lists(c, 256):
        assert same(knn_predict_variant(c, nbr, inter, uni), (items, scores))
        wrong = knn_predict_variant(c, nbr, inter, uni, rank_mod=128)
        differ += not same(knn_topn_variant(c, u, *wrong, N=100), knn_topn_variant(c, u, items, scores, N=100))
    assert differ == len(c['users'])


def test_sensitivity_knn_chunks_concatenated():
    # on `ones` alone the order is the item id, which is also the chunk order: concatenating the chunks' lists is then the merge, and
    # only a variant that also mis-cuts could show.  ones_few2 is what tells the two apart: a score above 1 in a late chunk.
    for name, expect in (('ones', False), ('ones_few2', True)):
        c = kc.build(name)
        differ = 0
        for u, _, (items, scores) in knn_lists(c, 20):
            kp, entries = kc.gathered(c, u, 20)
            if entries > kc.GATHER_MIN:
                differ += not same(knn_topn_variant(c, u, items, scores, 7, width=kc.GATHER_MIN // kp), knn_topn_variant(c, u, items, scores, 7))
        assert (differ >= 10) == expect and (differ == 0) == (not expect)


def test_sensitivity_knn_own_items_leave_before_the_cut():
    c = kc.build('ones')
    (up, ui, uc), _ = c['pairs']
    differ = 0
    for t, (u, (nbr, inter, uni), (items, scores)) in enumerate(knn_lists(c, 20)):
        right = knn_topn_variant(c, u, items, scores, 7)
        assert same(right, ok.topn(up, ui, uc, u, nbr, inter, uni, c['n'], 7))
        differ += not same(knn_topn_variant(c, u, items, scores, 7, exclude_after_cut=True), right)
    assert differ >= 10


# ---------------------------------------------------------------------------------------------------------- sensitivity: IPF
def ipf_predict_variant(g, u, kmod=None, pos_asc=False):
    """oi.predict, returning (items, scores, insertion keys); kmod: the level-1 index k kept modulo kmod; pos_asc: the insertion
    order takes the parent's position ascending instead of descending."""
    m, n = g.m, g.n
    score = np.zeros(n)
    ins = np.full((n, 4), -1, np.int64)
    r2 = [np.zeros(m), np.zeros(m)]
    for p in range(4):
        start, h = (0 if p < 2 else 1), p & 1
        L1 = g.D[start][u]
        rank1 = (0.0 if p < 2 else g.r[0] * g.W[0][u]) + g.r[start] * g.W[start][u]
        if len(L1) == 0:
            continue
        parts = [g.H[h][a] for a in L1]
        b = np.concatenate([x[0] for x in parts])
        pos = np.concatenate([x[1] for x in parts])
        k = np.repeat(np.arange(1, len(L1) + 1, dtype=np.int64), [len(x[0]) for x in parts])
        if kmod:
            k = k % kmod
        keep = b != u if p in (0, 3) else np.ones(len(b), bool)
        key2 = np.zeros(m, np.int64)
        np.maximum.at(key2, b[keep], (k[keep] << 32) | (0xFFFFFFFF - pos[keep]))
        reached = np.flatnonzero(key2)
        K = key2[reached] >> 32
        pos2 = 0xFFFFFFFF - (key2[reached] & 0xFFFFFFFF)
        carry = np.where(reached == u, g.r[0], r2[0][reached]) if p == 2 else r2[1][reached] if p == 3 else np.zeros(len(reached))
        rank2 = carry + rank1 * g.P[h][L1[K - 1]]
        r2[h][reached] = rank2
        e3 = (K << 32) | pos2
        lists = [g.D[h][bb] for bb in reached]
        if not any(len(x) for x in lists):
            continue
        c = np.concatenate(lists)
        owner = np.repeat(np.arange(len(reached)), [len(x) for x in lists])
        j = np.concatenate([np.arange(len(x)) for x in lists])
        key3 = np.zeros(n, np.int64)
        np.maximum.at(key3, c, e3[owner])
        win = key3[c] == e3[owner]
        cw, ow = c[win], owner[win]
        score[cw] = score[cw] + rank2[ow] * g.W[h][reached[ow]]
        new = ins[cw, 0] < 0
        ins[cw[new]] = np.stack([np.full(new.sum(), p), -K[ow[new]], (pos2 if pos_asc else -pos2)[ow[new]], j[win][new]], axis=1)
    items = np.flatnonzero(ins[:, 0] >= 0)
    order = np.lexsort((ins[items, 3], ins[items, 2], ins[items, 1], ins[items, 0], -score[items]))
    return items[order], score[items][order], ins[items][order]


def ipf_topn_variant(g, u, items, scores, ins, N, drop_zero=False, blind_tail=0):
    """oi.topn from a predict list; drop_zero: items of score zero are left out; blind_tail: the cut at N is made before the last
    blind_tail candidates (in first-insertion order, the order in which a query reaches them) are seen."""
    keep = ~np.isin(items, g.D[0][u])
    if drop_zero:
        keep &= scores > 0.0
    items, scores, ins = items[keep], scores[keep], ins[keep]
    if blind_tail:
        reach_order = np.lexsort((ins[:, 3], ins[:, 2], ins[:, 1], ins[:, 0]))
        seen = np.zeros(len(items), bool)
        seen[reach_order[:max(0, len(items) - blind_tail)]] = True
        items, scores = items[seen], scores[seen]
    return items[:N], scores[:N]


@pytest.mark.parametrize('name', ['l1_257', 'l1_513'])
def test_sensitivity_ipf_k_in_eight_bits(name):
    c = ic.build(name)
    g, u = ic.graph(c), c['long_user']
    assert same(ipf_predict_variant(g, u)[:2], ic.predict(c, u))           # the variant's own base is the oracle
    assert not same(ipf_predict_variant(g, u, kmod=256)[:2], ic.predict(c, u))
    wrong, right = ipf_predict_variant(g, u, kmod=256), ipf_predict_variant(g, u)
    assert not same(ipf_topn_variant(g, u, *wrong, N=50), ipf_topn_variant(g, u, *right, N=50))


def test_sensitivity_ipf_position_order():
    c = ic.build('rho0')
    g = ic.graph(c)
    differ = 0
    for u in c['users']:
        right = ipf_predict_variant(g, u)
        assert same(right[:2], ic.predict(c, u)) and same(ipf_topn_variant(g, u, *right, N=10), ic.topn(c, u, 10))
        differ += not same(ipf_topn_variant(g, u, *ipf_predict_variant(g, u, pos_asc=True), N=10), ic.topn(c, u, 10))
    assert differ >= 10


def test_sensitivity_ipf_zero_scores_kept():
    c = ic.build('beta0')
    g = ic.graph(c)
    differ = 0
    for u in c['users']:
        right = ipf_predict_variant(g, u)
        differ += not same(ipf_topn_variant(g, u, *right, N=100, drop_zero=True), ic.topn(c, u, 100))
    assert differ >= 10


def test_sensitivity_ipf_selection_sees_the_last_block():
    c = ic.build('sel_769')
    g = ic.graph(c)
    right = ipf_predict_variant(g, 0)
    assert same(ipf_topn_variant(g, 0, *right, N=100), oi.topn(g, 0, 100)) and same(ic.topn(c, 0, 100), oi.topn(g, 0, 100))
    for N in (100, 1):
        assert not same(ipf_topn_variant(g, 0, *right, N=N, blind_tail=ic.THREADS), ic.topn(c, 0, N))
