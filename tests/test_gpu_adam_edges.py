"""GPU: the live Adam path (yue_adam_step = k_mb_grad<KR> + k_adam) at its width, run, batch, collision, margin and
grid-stride edges (tests/helpers/adam_cases.py), against the fp64 graph under the a-priori bounds of oracle/numpy_adam.bounds.

How a gradient is read without an entry point of its own: after yue_adam_reset one step leaves m = fl((1 - 0.9f) g), so
g = m / (1 - 0.9f) to one rounding (the bounds' spare ulp); from standing moments g = (m_new - 0.9f m_old) / (1 - 0.9f), and the
bound widens by that subtraction's own rounding, 2^-24 * 3 (|m_new| + |m_old|) / (1 - 0.9f).  v, the factors' step and the rows
no triplet names are then checked against the device's OWN m and v, in k_adam's float32 statements.

Repeated runs of k_mb_grad are not bit-identical (float atomics reorder the sums); nothing here asks for that."""
import numpy as np
import pytest

from helpers import adam_cases as ac
from oracle import numpy_adam as na

pytestmark = pytest.mark.gpu

F = np.float32
B1, B2, EPS = F(0.9), F(0.999), F(1e-8)
ONE_B1, ONE_B2 = F(1) - B1, F(1) - B2                 # k_adam's (1.0f - beta), formed in float32
ULP = 2.0 ** -24
TINY = 2.0 ** -126                                    # below the normal range a float32 keeps no relative precision
LR = ac.LR
WORST = {}


@pytest.fixture(scope='module')
def dev():
    from yue_amd._shim import Device
    d = Device(0, raise_errors=True)
    yield d
    d.close()
    print('adam edges, largest ratios:', ' '.join('%s %.3f (%s)' % (q, r, name) for q, (r, name) in sorted(WORST.items())))


def lr_t(lr, step):
    """As adam_apply_dense forms it: in double from the double constants, rounded to float32 once."""
    return F(lr * np.sqrt(1.0 - 0.999 ** step) / (1.0 - 0.9 ** step))


def note(q, r, name):
    if r > WORST.get(q, (-1.0, ''))[0]:
        WORST[q] = (r, name)


def zero_state(m, n, k):
    return tuple(np.zeros((r, k), F) for r in (m, m, n, n))


def checked_step(dev, name, feed, reg, step, old=None, lr=LR, want=None):
    """One yue_adam_step on the device's standing factors (and moments `old`; None: right after a reset) under every check of this
    file.  `want`: the yardstick dict (loss, gU, gV, b_loss, bU, bV) at those factors; None: computed here.  Returns the new
    (P, Q, moments, loss)."""
    u, i, j = feed
    P0, Q0 = dev.get_factors()
    if want is None:
        want = ac.measure({'reg': reg}, P0, Q0, u, i, j)
    fresh = old is None
    old = zero_state(dev.m, dev.n, dev.k) if fresh else old
    loss = dev.adam_step(u, i, j, lr, reg, step)
    P1, Q1 = dev.get_factors()
    new = dev.adam_get_moments()
    assert np.isfinite(loss) and all(np.isfinite(a).all() for a in (P1, Q1) + new), name
    # the loss: the fp64 graph under its bound, the float32 oracle at the 1e-5 of tests/test_gpu_adam.py
    loss32 = float(na.loss_and_grad(P0, Q0, u, i, j, reg, F)[0])
    r = abs(loss - want['loss']) / want['b_loss']
    note('loss', r, name)
    print(name, 'step', step, 'loss %.9g (fp64 %.9g) ratio %.3f' % (loss, want['loss'], r))
    assert r <= 1 and abs(loss - loss32) < 1e-5 * abs(loss32), (name, loss, want['loss'], loss32)
    touched = (np.bincount(u, minlength=dev.m) > 0, (np.bincount(i, minlength=dev.n) + np.bincount(j, minlength=dev.n)) > 0)
    for side, var0, var1, m0, v0, m1, v1, g64, bound, rows in (('U', P0, P1, old[0], old[1], new[0], new[1], want['gU'], want['bU'], touched[0]),
                                                              ('V', Q0, Q1, old[2], old[3], new[2], new[3], want['gV'], want['bV'], touched[1])):
        m1d, m0d = m1.astype(np.float64), m0.astype(np.float64)
        if fresh:
            g, slack = m1d / float(ONE_B1), 0.0
        else:
            g = (m1d - float(B1) * m0d) / float(ONE_B1)
            slack = ULP * 3 * (np.abs(m1d) + np.abs(m0d)) / float(ONE_B1)
        # rows no triplet names: a zero gradient exactly -- the moments decay in k_adam's own bits, and the row still moves
        idle = ~rows
        assert np.array_equal(m1[idle], B1 * m0[idle]) and np.array_equal(v1[idle], B2 * v0[idle]), (name, side)
        if idle.any() and m0[idle].any():
            assert not np.array_equal(var1[idle], var0[idle]), (name, side)
        r = ac.ratio(g[rows], g64[rows], bound[rows] + (slack[rows] if not fresh else 0.0))
        note('g' + side, r, name)
        # v against that g: two products, one sum and g's own reading, 4 ulps (and the reading's slack where it is wider)
        v_want = float(B2) * v0.astype(np.float64) + float(ONE_B2) * g * g
        v_tol = 4 * ULP * v_want + 2 * float(ONE_B2) * np.abs(g) * slack + TINY
        rv = float((np.abs(v1 - v_want) / v_tol).max())
        note('v', rv, name)
        # the step from the device's own moments, in float32 as k_adam writes it
        step32 = var0 - lr_t(lr, step) * m1 / (np.sqrt(v1) + EPS)
        rs = float(np.abs(var1.astype(np.float64) - step32).max() / (1e-6 * lr))
        note('step', rs, name)
        print(name, 'step', step, 'g%s ratio %.3f  v %.3f  step %.3g' % (side, r, rv, rs))
        assert r <= 1, (name, side, r)
        assert rv <= 1, (name, side, rv)
        assert rs <= 1, (name, side, rs)
    return P1, Q1, new, loss


def from_reset(dev, c):
    dev.set_factors(c['U'], c['V'])
    dev.adam_reset()
    return checked_step(dev, c['name'], (c['u'], c['i'], c['j']), c['reg'], 1, want=c)


@pytest.mark.parametrize('name', ac.NAMES)
def test_every_case_from_a_reset_and_again(dev, name):
    c = ac.build(name)
    P1, Q1, mom, loss = from_reset(dev, c)
    # dP / dQ were left clean: the same triplets from a fresh reset on the same factors give the gradient again
    from_reset(dev, c)
    if name in ac.WIDTH_NAMES or name == 'big':
        # the forced triplets: both ends of both axes took part
        assert mom[0][c['m'] - 1].all() and mom[2][0].all() and mom[2][c['n'] - 1].all() and mom[2][ac.A].all() and mom[2][ac.B].all()
    if name == 'big':
        tail = mom[2].ravel()[ac.ADAM_GRID_REACH:]
        assert len(tail) == 1498 and tail.any() and not np.array_equal(Q1.ravel()[ac.ADAM_GRID_REACH:], c['V'].ravel()[ac.ADAM_GRID_REACH:])
        assert mom[2].ravel()[-218:].all()                                # the last, partly filled workgroup of the second trip: item n - 1
    if name == 'ieqj':
        # V_i - V_j is exactly 0: the user's row gets reg U_u in its own bits.  (On the item's row the positive term and the negative's
        # cancel to 2 reg V_i after one rounding each: the bound above holds that)
        assert np.array_equal(mom[0][ac.LONE_USER], ONE_B1 * (F(c['reg']) * c['U'][ac.LONE_USER]))
        assert np.allclose(c['gV'][ac.LONE_ITEM], 2 * c['reg'] * c['V'][ac.LONE_ITEM].astype(np.float64), rtol=1e-12, atol=0)


@pytest.mark.parametrize('name', ac.SAT_NAMES)
def test_saturated_margins_leave_exactly_the_reg_terms(dev, name):
    c = ac.build(name)
    u, i, j, x = c['u'], c['i'], c['j'], c['x']
    P1, Q1, mom, loss = from_reset(dev, c)
    reg = F(c['reg'])
    # a row whose every margin lies beyond +90: expf is inf, the coefficient -0, and reg * row is all a triplet adds.  With one
    # or two such triplets the sum is exact in any order (x + x rounds nowhere)
    seen = 0
    for side, ids_list, rows, mrow in (('U', (u,), c['U'], mom[0]), ('V', (i, j), c['V'], mom[2])):
        far = np.ones(len(rows), bool)
        count = np.zeros(len(rows), int)
        for ids in ids_list:
            np.logical_and.at(far, ids, x > 90)
            np.add.at(count, ids, 1)
        for r in np.flatnonzero(far & (count >= 1) & (count <= 2)):
            want = reg * rows[r] if count[r] == 1 else reg * rows[r] + reg * rows[r]
            assert np.array_equal(mrow[r], ONE_B1 * want), (name, side, r)
            seen += 1
    assert name == 'sat_neg' or seen >= 1
    if name != 'sat_neg':
        assert np.array_equal(mom[0][ac.LONE_USER], ONE_B1 * (reg * c['U'][ac.LONE_USER]))


@pytest.mark.parametrize('name', ['neg100', 'k129'])
def test_three_steps_without_a_reset(dev, name):
    c = ac.build(name)
    feed = (c['u'], c['i'], c['j'])
    dev.set_factors(c['U'], c['V'])
    dev.adam_reset()
    mom = None
    for step in (1, 2, 3):
        # steps 2 and 3 run from standing moments (the two-sided reading) on the factors the last step left: the yardstick is
        # taken there, so that a step's check does not inherit the last one's rounding
        P, Q, mom, loss = checked_step(dev, '%s/%d' % (name, step), feed, c['reg'], step, old=mom, want=c if step == 1 else None)


def test_the_step_number_enters_through_lr_t_alone(dev):
    c = ac.build('k65')
    feed = (c['u'], c['i'], c['j'])
    out = {}
    for step in (1, 1000):
        dev.set_factors(c['U'], c['V'])
        dev.adam_reset()
        out[step] = checked_step(dev, 'k65/step%d' % step, feed, c['reg'], step, want=c)
    assert lr_t(LR, 1) != lr_t(LR, 1000) and abs(float(lr_t(LR, 1000)) / LR - np.sqrt(1 - 0.999 ** 1000)) < 1e-6
    # (checked_step held each run's factors to ITS lr_t.)  Equal states: the moments do not know the step number, and the rows
    # moved lr_t(1000) / lr_t(1) times as far
    rows = np.unique(c['u'])
    assert ac.ratio(out[1][2][0], out[1000][2][0].astype(np.float64), 2 * float(ONE_B1) * c['bU'] + TINY) <= 1
    moved1, moved1000 = np.abs(out[1][0][rows].astype(np.float64) - c['U'][rows]), np.abs(out[1000][0][rows].astype(np.float64) - c['U'][rows])
    scale = float(lr_t(LR, 1000)) / float(lr_t(LR, 1))
    assert abs(np.median(moved1000) / np.median(moved1) - scale) <= 1e-3 * scale


def bits_of(dev):
    return [a.copy() for a in dev.get_factors() + dev.adam_get_moments()]


def test_the_state_lives_with_the_shape_and_refusals_move_nothing(dev):
    from yue_amd._shim import ERR_ARG, Device, YueHipError
    c, other = ac.build('T33'), ac.build('sat_pos')
    u, i, j = feed = (c['u'], c['i'], c['j'])

    def refused(f, *a):
        with pytest.raises(YueHipError) as e:
            f(*a)
        assert e.value.code == ERR_ARG, e.value
        return str(e.value)
    fresh = Device(0, raise_errors=True)
    try:
        assert 'no Adam state' in refused(fresh.adam_get_moments)
        fresh.set_factors(c['U'], c['V'])
        assert 'no Adam state' in refused(fresh.adam_get_moments)
        # the first step makes the state itself, from zero moments
        checked_step(fresh, 'state/implicit', feed, c['reg'], 1)
    finally:
        fresh.close()
    dev.set_factors(c['U'], c['V'])
    dev.adam_reset()
    P, Q, mom, _ = checked_step(dev, 'state/first', feed, c['reg'], 1, want=c)
    # factors of the same shape keep the moments ...
    dev.set_factors(c['U'], c['V'])
    kept = dev.adam_get_moments()
    assert all(np.array_equal(a, b) for a, b in zip(kept, mom)) and kept[0].any()
    checked_step(dev, 'state/kept', feed, c['reg'], 2, old=kept, want=c)
    # ... another shape has none, and a step there starts from zero
    dev.set_factors(other['U'], other['V'])
    assert 'no Adam state' in refused(dev.adam_get_moments)
    checked_step(dev, 'state/other shape', (other['u'], other['i'], other['j']), other['reg'], 1, want=other)
    # and back: the old shape's moments are gone as well
    dev.set_factors(c['U'], c['V'])
    assert 'no Adam state' in refused(dev.adam_get_moments)
    checked_step(dev, 'state/back', feed, c['reg'], 1, want=c)
    # refusals: each with its message, and nothing moves
    before = bits_of(dev)
    m, n = c['m'], c['n']

    def with_id(arr, t, value):
        out = arr.copy()
        out[t] = value
        return out
    assert 'T > 0' in refused(dev.adam_step, u[:0], i[:0], j[:0], LR, c['reg'], 1)
    assert 'step >= 1' in refused(dev.adam_step, u, i, j, LR, c['reg'], 0)
    for t, bad in ((0, (with_id(u, 0, m), i, j)), (32, (with_id(u, 32, -1), i, j)), (5, (u, with_id(i, 5, n), j)), (31, (u, i, with_id(j, 31, n))), (7, (u, i, with_id(j, 7, -1)))):
        assert 'triplet %d out of range' % t in refused(dev.adam_step, *bad, LR, c['reg'], 2)
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(before, bits_of(dev)))
    # the refused calls left nothing in dP / dQ either
    checked_step(dev, 'state/after refusals', feed, c['reg'], 2, old=tuple(before[2:]))


# ---- the hand-back: whoever used dP / dQ left them as yue_adam_step expects them ----------------------------------------------------
def _feed(m, n, seed, T=200):
    rs = np.random.RandomState(seed)
    return [np.array(x, np.int32) for x in zip(*ac._mixed(rs, {'m': m, 'n': n}, T))]


def _bpr_problem(m, n, k, d, seed):
    from yue_amd import synth
    data = synth.make_arrays(m, n, d, seed=seed)
    P0, Q0 = synth.init_factors(m, n, k, seed)
    return data, P0, Q0


def _epoch(seq, n=90, stage=1):
    """stage = 2 on 20 items: the epoch's pre-pass stages rows of up to two touches, every other contended row is hot (float atomics
    into dQ, folded and cleared behind the round)."""
    def setup(dev):
        data, P0, Q0 = _bpr_problem(120, n, 20, 8, 31)
        dev.set_option('round_user_seq', seq)
        dev.set_option('round_stage', stage)
        dev.set_factors(P0, Q0)
        dev.set_interactions(data['indptr'], data['indices'], data['ev_ptr'], data['ev_i'])

        def run():
            dev.bpr_epoch(42, 0, 256, 0.02, 0.01, 0.01)
            assert dev.get_option('round_last_user_seq') == seq
            assert stage == 1 or dev.get_option('round_last_stage_max') == stage
        return run
    return setup


def _rounds(dev):
    # 20 items under 256-event rounds: every item row is named some 25 times a round (hot rows, summed in dQ)
    from yue_amd import synth
    rs = np.random.RandomState(32)
    m, n, k, T = 200, 20, 20, 1024
    u, i = rs.randint(0, m, T).astype(np.int32), rs.randint(0, n, T).astype(np.int32)
    j = ((i + 1 + rs.randint(0, n - 1, T)) % n).astype(np.int32)
    dev.set_factors(*synth.init_factors(m, n, k, 32))
    assert min(np.bincount(np.r_[i[r:r + 256], j[r:r + 256]], minlength=n).min() for r in range(0, T, 256)) >= 8
    return lambda: dev.bpr_rounds(u, i, j, np.arange(0, T + 1, 256, dtype=np.int64), 0.02, 0.01, 0.01)


def _replay(dev):
    data, P0, Q0 = _bpr_problem(120, 90, 20, 8, 33)
    dev.set_factors(P0, Q0)
    u, i, j = _feed(120, 90, 330, T=500)
    return lambda: dev.bpr_replay(u, i, j, 0.02, 0.01, 0.01)


def _lgcn(step):
    def setup(dev):
        from helpers import lightgcn_cases as lc
        from test_gpu_lightgcn import upload
        c = lc.build('k20')
        upload(dev, c)
        if step:
            return lambda: dev.lgcn_step(c['layers'], c['u'], c['i'], c['j'], 0.002, lc.REG, 2)
        return lambda: dev.lgcn_grad(c['layers'], c['u'], c['i'], c['j'], lc.REG)
    return setup


def _ngcf(dev):
    from helpers import ngcf_cases as nc
    from test_gpu_ngcf import run_args, upload
    c = nc.build('k2')
    upload(dev, c)
    return lambda: dev.ngcf_grad(*run_args(c), c['u'], c['i'], c['j'], nc.REG)


def _apr(what):
    def setup(dev):
        from helpers import apr_cases as pc
        c = pc.build('base')
        u, i, j = c['u'], c['i'], c['j']
        dev.set_factors(c['U'], c['V'])

        def run():
            # (the perturbation is set behind the Adam state's first step: yue_adam_reset is not called again)
            dev.apr_set_delta(c['ids_u'], c['rows_u'], c['ids_i'], c['rows_v'])
            if what == 'grad':
                dev.apr_grad(False, u, i, j, pc.REG)
            elif what == 'grad_adv':
                dev.apr_grad(True, u, i, j, c['regA'])
            elif what == 'pre_step':
                dev.apr_pre_step(u, i, j, 0.002, pc.REG, 2)
            else:
                dev.apr_adv_step(u, i, j, 0.002, c['eps'], c['regA'], 2)
        return run
    return setup


PRODUCERS = {'epoch_user_seq': _epoch(1), 'epoch_user_rounds': _epoch(0), 'epoch_hot_items': _epoch(1, n=20, stage=2),
             'epoch_user_rounds_hot_items': _epoch(0, n=20, stage=2), 'rounds_hot_items': _rounds, 'replay': _replay,
             'lgcn_grad': _lgcn(False), 'lgcn_step': _lgcn(True), 'ngcf_grad': _ngcf,
             'apr_grad': _apr('grad'), 'apr_grad_adv': _apr('grad_adv'), 'apr_pre_step': _apr('pre_step'), 'apr_adv_step': _apr('adv_step')}


@pytest.mark.parametrize('producer', list(PRODUCERS))
def test_the_gradient_buffers_come_back_clean(dev, producer):
    """Factors with an Adam state; one call of the producer; yue_adam_step with NO reset in between (a reset clears dP / dQ and would
    hide a row left behind): its gradient, read from the moments on both sides, is the fp64 gradient at the factors read."""
    try:
        run = PRODUCERS[producer](dev)
        feed = _feed(dev.m, dev.n, 77)
        dev.adam_reset()
        checked_step(dev, producer + '/before', feed, ac.REG, 1)
        run()
        mom = dev.adam_get_moments()
        checked_step(dev, producer + '/after', feed, ac.REG, 3, old=mom)
    finally:
        dev.set_option('round_user_seq', 1)           # the defaults, for the tests behind this one
        dev.set_option('round_stage', 1)
