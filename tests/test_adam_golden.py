"""CPU: the yardstick, the bounds and the cases behind tests/test_gpu_adam_edges.py (tests/helpers/adam_cases.py).

oracle/numpy_adam.adam_step still returns the bits it returned before loss_and_grad was lifted out of it; loss_and_grad in fp64 is
the derivative of its own loss; every case reaches the branch of k_mb_grad / k_adam it exists for; the float32 contract stays within
the a-priori bounds in feed order and in three shuffled orders; and (a condition on the cases, in the manner of
tests/test_expomf_power.py) each named fault of the kernel, put into the float32 contract, leaves the bounds by at least 100 x on some
element of every case it applies to.  A case that does not clear that is reshaped in adam_cases.py, not excused here."""
import hashlib

import numpy as np
import pytest

from helpers import adam_cases as ac
from oracle import numpy_adam as na

POWER = 100.0
SHUFFLE_SEEDS = (1, 2, 3)
# three steps of adam_step at the commit before loss_and_grad existed: (seed, m, n, k, events, negs, stddev), the three losses,
# sha256[:16] of U | V and of mU | vU | mV | vV
RECORDED = [
    ((1, 30, 50, 10, 8, 100, 0.005), ['0x1.1543300000000p+9', '0x1.1544740000000p+9', '0x1.1521d60000000p+9'], '9977a67a16c9857f', '730b866c2a013fac'),
    ((2, 50, 80, 200, 7, 3, 0.005), ['0x1.d1e48c0000000p+3', '0x1.d214340000000p+3', '0x1.d2d4e40000000p+3'], 'f8d5bf154616d4cf', 'db019581ba135f93'),
    ((3, 20, 30, 16, 40, 2, 1.0), ['0x1.55c9640000000p+7', '0x1.e6c4c40000000p+7', '0x1.7ab11c0000000p+7'], '9b5f524868fc95d7', '0cda1a69b9da5177'),
]


def _digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()[:16]


@pytest.mark.parametrize('shape,losses,factors,moments', RECORDED)
def test_adam_step_gives_the_recorded_bits(shape, losses, factors, moments):
    seed, m, n, k, events, negs, stddev = shape
    rs = np.random.RandomState(seed)
    U, V = na.truncated_normal(rs, (m, k), stddev), na.truncated_normal(rs, (n, k), stddev)
    st = na.new_state(U, V)
    got = []
    for step in (1, 2, 3):
        u = np.repeat(rs.randint(0, m, size=events), negs).astype(np.int32)
        i = np.repeat(rs.randint(0, n, size=events), negs).astype(np.int32)
        j = rs.randint(0, n, size=events * negs).astype(np.int32)
        got.append(na.adam_step(U, V, st, u, i, j, 0.02, 0.01, step).hex())
    assert got == losses and _digest(U, V) == factors and _digest(st['mU'], st['vU'], st['mV'], st['vV']) == moments


def test_the_fp64_gradient_is_the_derivative_of_the_fp64_loss():
    rs = np.random.RandomState(7)
    m, n, k, reg = 5, 7, 3, 0.01
    U, V = rs.normal(0, 0.7, (m, k)), rs.normal(0, 0.7, (n, k))
    u, i, j = np.array([0, 0, 1, 4, 4, 2, 2]), np.array([1, 1, 1, 6, 0, 3, 5]), np.array([2, 6, 0, 1, 6, 3, 1])       # (2, 3, 3): i == j
    loss, gU, gV = na.loss_and_grad(U, V, u, i, j, reg, np.float64)
    assert gU.dtype == gV.dtype == np.float64 and not gU[3].any() and not gV[4].any()
    h = 1e-6
    for M, g in ((U, gU), (V, gV)):
        for idx in np.ndindex(*M.shape):
            old = M[idx]
            M[idx] = old + h
            up = na.loss_and_grad(U, V, u, i, j, reg, np.float64)[0]
            M[idx] = old - h
            down = na.loss_and_grad(U, V, u, i, j, reg, np.float64)[0]
            M[idx] = old
            assert abs((up - down) / (2 * h) - g[idx]) < 1e-8 * max(1.0, abs(g[idx]))
    l32, gU32, gV32 = na.loss_and_grad(U.astype(np.float32), V.astype(np.float32), u, i, j, reg, np.float32)
    assert l32.dtype == gU32.dtype == gV32.dtype == np.float32


def test_every_case_reaches_its_branch():
    assert len(set(ac.NAMES)) == len(ac.NAMES)
    # widths: both sides of every instance switch, one live lane, a partly filled last register, the widest
    assert [ac.kr_of(ac.build(name)['k']) for name in ac.WIDTH_NAMES] == [1, 1, 1, 2, 2, 4, 4]
    assert [ac.build(name)['k'] % 64 for name in ac.WIDTH_NAMES] == [1, 63, 0, 1, 0, 1, 0]
    for name in ac.WIDTH_NAMES + ['big']:
        c = ac.build(name)
        u, i, j, m, n = c['u'], c['i'], c['j'], c['m'], c['n']
        assert (m - 1) in u and 0 in i and (n - 1) in j and 0 in np.r_[u, i, j]
        pos_users, neg_users = set(u[i == ac.A].tolist()), set(u[j == ac.A].tolist())
        assert pos_users and neg_users and pos_users != neg_users            # an item positive for one user, negative for another
        assert len(u) == (256 if name == 'big' else 200) and min(c['runs']) == 1 and max(c['runs']) >= 17 and len(set(c['runs'])) >= 4
    # batch sizes: one wave short, full and over; one workgroup short, full and over
    assert [(len(ac.build(n)['u']) % ac.CHUNK, len(ac.build(n)['u']) % ac.GROUP) for n in ('T1', 'T31', 'T32', 'T33', 'T127', 'T128', 'T129')] == \
        [(1, 1), (31, 31), (0, 32), (1, 33), (31, 127), (0, 0), (1, 1)]
    assert [-(-(-(-len(ac.build(n)['u']) // 32)) // 4) for n in ('T127', 'T128', 'T129')] == [1, 1, 2]             # workgroups
    # runs
    c = ac.build('run1')
    assert set(c['runs']) == {1}
    c = ac.build('u_moves')
    assert len(set(c['i'].tolist())) == 1 and set(c['runs']) == {3} and (np.diff(c['u'])[2::3] != 0).all()
    c = ac.build('i_moves')
    assert len(set(c['u'].tolist())) == 1 and set(c['runs']) == {3} and (np.diff(c['i'])[2::3] != 0).all()
    c = ac.build('abab')
    pairs = list(zip(c['u'].tolist(), c['i'].tolist()))
    assert len(pairs) == 128 and pairs[0] != pairs[1] and pairs == [pairs[0], pairs[1]] * 64
    for name, first, edges in (('cut', 20, [32, 64, 96]), ('cut_group', 60, [64, 96, 128])):
        c = ac.build(name)
        at = np.cumsum([0] + c['runs'])
        long_run = int(np.argmax(c['runs']))
        assert c['runs'][long_run] == 100 and at[long_run] == first and sorted(set(c['runs'])) == [1, 100]
        crossed = [e for e in range(ac.CHUNK, len(c['u']), ac.CHUNK) if first < e < first + 100]
        assert crossed == edges and [e for e in crossed if e % ac.GROUP == 0] == ([128] if name == 'cut_group' else [])
        assert ac.lost_flushes(c['u'], c['i']).sum() == edges[-1] - first
    c = ac.build('neg100')
    assert c['runs'] == [100] * 8
    # collisions
    c = ac.build('ieqj')
    t = np.flatnonzero(c['u'] == ac.LONE_USER)
    assert t.tolist() == [10] and c['i'][10] == c['j'][10] == ac.LONE_ITEM and (np.r_[c['i'], c['j']] == ac.LONE_ITEM).sum() == 2
    assert (np.delete(c['i'], 10) != np.delete(c['j'], 10)).all()
    c = ac.build('one_j')
    assert len(c['j']) == 4096 and (c['j'] == ac.ONE_J).all() and (c['i'] != ac.ONE_J).all()
    c = ac.build('repeat')
    assert c['runs'] == [64] and len(set(c['j'].tolist())) == 1
    # margins: expf(x) is inf beyond 88.73 and (1 + expf(x)) is 1 below -16.7; every case has margins on both sides of 20 and of 90
    for name in ac.NAMES:
        c = ac.build(name)
        if name not in ac.SAT_NAMES:
            assert np.abs(c['x']).max() < 0.05 and np.abs(c['U']).max() <= 0.01
    x = ac.build('sat_pos')['x']
    assert x.min() >= 0 and x.max() > 90 and ((x > 20) & (x < 88)).any() and (x < 10).any()
    x = ac.build('sat_neg')['x']
    assert x.max() <= 0 and x.min() < -90 and ((x < -20) & (x > -88)).any() and (x > -10).any()
    x = ac.build('sat_mix')['x']
    assert x.max() > 90 and x.min() < -90 and ((x > 20) & (x < 88)).any() and ((x < -20) & (x > -88)).any()
    for name in ac.SAT_NAMES:
        c = ac.build(name)
        assert np.flatnonzero(c['u'] == ac.LONE_USER).tolist() == [10] and c['x'][10] * (-1 if name == 'sat_neg' else 1) > 90 and c['k'] == 16
    # k_adam: a second trip of the grid-stride loop, and a last workgroup that is partly filled
    c = ac.build('big')
    count = c['n'] * c['k']
    assert count == 2098650 and count > ac.ADAM_GRID_REACH and count - ac.ADAM_GRID_REACH == 1498 and count % 256 == 218
    touched = np.unique(np.r_[c['i'], c['j']])
    assert touched.max() == c['n'] - 1 and len(touched) < 520                 # the tail beyond the grid's reach is touched AND mostly idle


@pytest.mark.parametrize('name', ac.NAMES)
def test_the_float32_contract_stays_within_the_bounds_in_any_order(name):
    c = ac.build(name)
    U, V, u, i, j = c['U'], c['V'], c['u'], c['i'], c['j']
    gU, gV = ac.contract(U, V, u, i, j, c['reg'])
    loss, oU, oV = na.loss_and_grad(U, V, u, i, j, c['reg'], np.float32)
    assert np.array_equal(gU, oU) and np.array_equal(gV, oV)                # the contract with no fault IS the oracle's float32 graph
    worst = {}
    for seed in (None,) + SHUFFLE_SEEDS:
        order = np.arange(len(u)) if seed is None else np.random.RandomState(seed).permutation(len(u))
        loss, gU, gV = na.loss_and_grad(U, V, u[order], i[order], j[order], c['reg'], np.float32)
        for key, r in (('gU', ac.ratio(gU, c['gU'], c['bU'])), ('gV', ac.ratio(gV, c['gV'], c['bV'])), ('loss', abs(float(loss) - c['loss']) / c['b_loss'])):
            worst[key] = max(worst.get(key, 0.0), r)
    print('adam contract', name, ' '.join('%s %.3f' % kv for kv in sorted(worst.items())))
    # (the oracle adds the T softplus terms in float32, pairwise, which the loss bound does not name: the device adds them in
    # double.  It stays inside all the same)
    assert worst['gU'] <= 1 and worst['gV'] <= 1 and worst['loss'] <= 1


@pytest.mark.parametrize('fault', ac.FAULTS)
def test_every_fault_leaves_the_bounds_by_a_hundred(fault):
    seen = 0
    for name in ac.NAMES:
        c = ac.build(name)
        if not ac.applies(fault, c):
            continue
        if fault == 'drop_last' and len(c['u']) == 1:
            gU, gV = np.zeros_like(c['U']), np.zeros_like(c['V'])
        else:
            gU, gV = ac.contract(c['U'], c['V'], c['u'], c['i'], c['j'], c['reg'], fault)
        out = max(ac.ratio(gU, c['gU'], c['bU']), ac.ratio(gV, c['gV'], c['bV']))
        print('adam power', fault, name, '%.3g' % out)
        assert out >= POWER, (fault, name, out)
        seen += 1
    assert seen >= {'lost_flush': 6, 'pad': 4}.get(fault, len(ac.NAMES))
