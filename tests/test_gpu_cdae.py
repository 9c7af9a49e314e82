"""GPU: CDAE's device path (yue_cdae_*) through the shim on synthetic problems from seeds
(tests/helpers/cdae_cases.py), against the fp64 contract tests/helpers/numpy_cdae.py.
Bounds: hid, the sampled logits and y_pred, the loss and the five gradients within 4 x the case's d32 (the float32 contract's own
distance from fp64) in relative max-norm, with a floor of L 2^-24 (L: the quantity's longest sum), so that a d32 of 0 does not
demand the bits of another summation order; the kept flags equal to the host's at every entry; yue_cdae_step within 1e-6 lr of the
contract's float32 Adam fed the device's own gradients (moments within 1e-6 relative), over three steps; a second run of every
call identical in every bit.  tests/test_cdae_golden.py asserts on the CPU that every case meets its conditioning statement."""
import numpy as np
import pytest

from helpers import cdae_cases as cc
from helpers import numpy_cdae as cd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    from yue_amd._shim import Device
    d = Device(0, raise_errors=True)
    yield d
    d.close()


def upload(dev, c, hub=None):
    ptr, items, cnt = c['data']
    dev.set_option('cdae_hub', hub if hub else (c['hub'] if c['hub'] else 1024))
    dev.cdae_set_data(c['m'], c['n'], ptr, items, cnt)
    p = c['p']
    dev.cdae_set_params(p['U'], p['W'], p['Wd'], p['b'], p['bd'])


def batch(c):
    return (c['users'], c['sptr'], c['sitems'], c['co'], c['mask_seed'], c['step'], cc.REG)


def check_forward(dev, c):
    fw = c['fw']
    hid, kept, logit, ypred, loss = dev.cdae_forward(*batch(c))
    got = {'hid': cc.rel(hid, fw['hid']), 'logit': cc.rel(logit, fw['logit']), 'y_pred': cc.rel(ypred, fw['y_pred'])}
    assert np.array_equal(kept, np.concatenate(fw['flags']) if len(kept) else np.zeros(0, bool)), 'kept flags'
    return got, loss, (hid, kept, logit, ypred)


def check_gradients(dev, c, hub=None):
    """Uploads the case (at `hub`, else at its own cdae_hub) and holds forward, loss and the five gradients to the case's bounds,
    the kept flags and the hub and part counts to the host's.  Returns (the gradients, every output in a fixed order)."""
    upload(dev, c, hub)
    got, loss, out = check_forward(dev, c)
    loss_g, g = dev.cdae_grad(*batch(c))
    assert loss_g == loss and dev.get_option('cdae_last_saturated') == 0
    got['loss'] = abs(loss - c['loss']) / abs(c['loss'])
    for k in cd.NAMES:
        got[k] = cd.rel(g[k], c['g'][k])
    print(c['name'], ' '.join('%s %.3g (d32 %.3g, x%.2f)' % (k, got[k], c['d32'][k], got[k] / c['d32'][k] if c['d32'][k] else 0.0) for k in cc.QUANTITIES))
    for k in cc.QUANTITIES:
        assert got[k] <= cc.bound(c, k), (k, got[k], c['d32'][k], cc.bound(c, k))
    hubs, parts = cd.hub_counts(c['data'], c['users'], c['sptr'], c['sitems'], hub if hub else (c['hub'] if c['hub'] else 1024))
    assert dev.get_option('cdae_last_hubs') == hubs and dev.get_option('cdae_last_parts') == parts
    return g, list(out) + [np.float64(loss)] + [g[k] for k in cd.NAMES]


@pytest.mark.parametrize('name', [n for n in cc.GPU_CASES if n != 'sat'])
def test_forward_mask_loss_and_gradients(dev, name):
    c = cc.build(name)
    g, _ = check_gradients(dev, c)
    hubs, parts = cd.hub_counts(c['data'], c['users'], c['sptr'], c['sitems'], c['hub'] if c['hub'] else 1024)
    if c['special'] == 'hub':
        assert hubs >= 3 and parts >= 9                          # the user of 40 items, the item of every slot, the batch itself
    if c['special'] == 'low':                                    # the clamped column passes no gradient: its rows hold the decay alone
        p = c['p']
        assert np.array_equal(g['Wd'][:, cc.SPECIAL], np.float32(cc.REG) * p['Wd'][:, cc.SPECIAL])
        assert g['bd'][cc.SPECIAL] == np.float32(cc.REG) * p['bd'][cc.SPECIAL]


def test_saturated_outputs_are_counted_the_loss_is_inf_and_a_step_moves_nothing(dev):
    c = cc.build('sat')
    upload(dev, c)
    got, loss, _ = check_forward(dev, c)
    print('sat', got, 'saturated', dev.get_option('cdae_last_saturated'), 'host', c['saturated'])
    for k in got:
        assert got[k] <= cc.bound(c, k), (k, got[k])
    assert c['saturated'] == c['B'] and dev.get_option('cdae_last_saturated') == c['saturated'] and loss == np.inf
    before = dev.cdae_get_params(moments=True)
    users, sptr, sitems, co, seed, step, reg = batch(c)
    loss, sat = dev.cdae_step(users, sptr, sitems, co, seed, 0.01, reg, 1)
    assert loss == np.inf and sat == c['saturated']
    after = dev.cdae_get_params(moments=True)
    for k in before:
        assert np.array_equal(before[k], after[k]), k
        assert k in cd.NAMES or not after[k].any()               # the moments: still zero


def check_steps(dev, c, lr=0.002, steps=(1, 2, 3), after=None):
    """yue_cdae_step against the contract's float32 Adam fed the device's own gradients, over whole arrays.  after(t, loss, g, before,
    got) sees each step's loss and gradients and the parameters and moments around it."""
    name = c['name']
    upload(dev, c)
    p = {k: v.copy() for k, v in c['p'].items()}
    st = cd.new_state(p)
    users, sptr, sitems, co, seed, _, reg = batch(c)
    for t in steps:
        before = {k: v.copy() for k, v in list(p.items()) + list(st.items())}
        loss_g, g = dev.cdae_grad(users, sptr, sitems, co, seed, t, reg)
        loss, sat = dev.cdae_step(users, sptr, sitems, co, seed, lr, reg, t)
        assert loss == loss_g and sat == 0
        for k in cd.NAMES:
            cd.adam(p[k], g[k], st['m' + k], st['v' + k], lr, t, np.float32)
        got = dev.cdae_get_params(moments=True)
        worst = max(float(np.abs(got[k] - p[k]).max()) for k in cd.NAMES)
        print(name, 'step', t, 'max |d| %.3g (bound %.3g)' % (worst, 1e-6 * lr))
        assert worst <= 1e-6 * lr
        for k in st:
            assert cd.rel(got[k], st[k]) <= 1e-6, k
        # Adam is dense, but a user outside every batch so far has zero moments: the row stays where it was
        if t == 2:
            outside = np.setdiff1d(np.arange(c['m']), users)
            assert len(outside) and (got['vU'][outside] == 0).all() and (got['U'][outside] == c['p']['U'][outside]).all()
        if after:
            after(t, loss, g, before, got)
        # the contract goes on from the device's state, so that a step's check does not inherit the last one's rounding
        for k in cd.NAMES:
            p[k] = got[k].copy()
        for k in st:
            st[k] = got[k].copy()
    assert all(t > 0 for t in dev.cdae_times())


@pytest.mark.parametrize('name', ['h2', 'h33', 'twice', 'keep01'])
def test_step_is_the_contracts_adam_on_the_devices_gradients(dev, name):
    check_steps(dev, cc.build(name))


@pytest.mark.parametrize('name', ['h64', 'hub'])
def test_repeat_runs_are_bit_identical(dev, name):
    c = cc.build(name)
    runs = []
    for _ in range(2):
        upload(dev, c)
        f = dev.cdae_forward(*batch(c))
        loss, g = dev.cdae_grad(*batch(c))
        users, sptr, sitems, co, seed, step, reg = batch(c)
        dev.cdae_step(users, sptr, sitems, co, seed, 0.002, reg, 1)
        dev.cdae_load_factors()
        runs.append(list(f[:4]) + [f[4], loss] + [g[k] for k in cd.NAMES] + list(dev.cdae_get_params(moments=True).values()) + list(dev.get_factors()))
    for a, b in zip(*runs):
        assert np.array_equal(a, b)


def check_factors(dev, c, users):
    """yue_cdae_load_factors against the contract's factors, then the scores of `users` against its logits."""
    name = c['name']
    upload(dev, c)
    dev.cdae_load_factors()
    p64 = {k: v.astype(np.float64) for k, v in c['p'].items()}
    P64, Q64 = cd.factors(p64, c['data'], np.float64)
    P32, Q32 = cd.factors(c['p'], c['data'], np.float32)
    P, Q = dev.get_factors()
    assert P.shape == (c['m'], c['h'] + 1) and Q.shape == (c['n'], c['h'] + 1) and (P[:, -1] == 1).all()
    assert np.array_equal(Q, Q32)
    want, want32 = P64 @ Q64.T, (P32[:, None, :] * Q32[None, :, :]).sum(axis=2, dtype=np.float32)
    d32 = cd.rel(want32, want)
    longest = int(np.diff(c['data'][0]).max())
    bound = max(4 * d32, max(longest + 2, c['h'] + 1) * 2.0 ** -24)
    worst = 0.0
    for u in users:
        worst = max(worst, float(np.abs(dev.scores(u) - want[u]).max() / np.abs(want).max()))
    print(name, 'scores %.3g (d32 %.3g, bound %.3g)' % (worst, d32, bound), 'hid', cd.rel(P[:, :-1], P64[:, :-1]))
    assert worst <= bound and cd.rel(P, P64) <= max(4 * cd.rel(P32, P64), (longest + 2) * 2.0 ** -24)


@pytest.mark.parametrize('name', ['h128', 'h33', 'hub'])
def test_load_factors_then_scores_are_the_contracts_logits(dev, name):
    c = cc.build(name)
    check_factors(dev, c, (0, 1, 2, c['m'] - 1))                 # no items, 40 items (parts at hub 8), one item, the last user


def test_refusals(dev):
    from yue_amd._shim import ERR_ARG, YueHipError
    c = cc.build('h33')
    upload(dev, c)
    users, sptr, sitems, co, seed, step, reg = batch(c)

    def refused(f, *a, **kw):
        with pytest.raises(YueHipError) as e:
            f(*a, **kw)
        assert e.value.code == ERR_ARG, e.value
        return str(e.value)
    bad = list(users); bad[2] = c['m']
    assert 'user out of range' in refused(dev.cdae_grad, bad, sptr, sitems, co, seed, step, reg)
    bad = sitems.copy(); bad[1] = bad[0]
    assert 'yue_cdae_grad: sample rows must be sorted and unique (row 0)' in refused(dev.cdae_grad, users, sptr, bad, co, seed, step, reg)
    bad = sitems.copy(); bad[int(sptr[1]) - 1] = c['n']
    assert 'yue_cdae_forward: sample id out of range (row 0)' in refused(dev.cdae_forward, users, sptr, bad, co, seed, step, reg)
    refused(dev.cdae_forward, users[:0], sptr[:1], sitems, co, seed, step, reg)              # B < 1
    refused(dev.cdae_forward, users, sptr, sitems, 0.0, seed, step, reg)
    refused(dev.cdae_forward, users, sptr, sitems, 1.5, seed, step, reg)
    refused(dev.cdae_step, users, sptr, sitems, co, seed, 0.01, reg, 0)                       # Adam's step counts from 1
    p = c['p']
    wide = cd.init_params(np.random.RandomState(1), c['m'], c['n'], 129, 0.1)
    assert 'h <= 128' in refused(dev.cdae_set_params, wide['U'], wide['W'], wide['Wd'], wide['b'], wide['bd'])
    W = p['W'].copy(); W[0, 0] = np.nan
    refused(dev.cdae_set_params, p['U'], W, p['Wd'], p['b'], p['bd'])
    ptr, items, cnt = c['data']
    two = items.copy(); two[int(ptr[1]) + 1] = two[int(ptr[1])]
    assert 'yue_cdae_set_data: user-major rows must be sorted and unique (row 1)' in refused(dev.cdae_set_data, c['m'], c['n'], ptr, two, cnt)
    # after the refusals the good state still answers
    loss, g = dev.cdae_grad(*batch(c))
    assert abs(loss - c['loss']) / abs(c['loss']) <= cc.bound(c, 'loss')
    from yue_amd._shim import Device
    fresh = Device(0, raise_errors=True)
    try:
        fresh.cdae_m, fresh.cdae_n, fresh.cdae_h, fresh.cdae_nnz_ptr = c['m'], c['n'], c['h'], ptr
        assert 'set_data first' in refused(fresh.cdae_grad, *batch(c))
        fresh.cdae_set_data(c['m'], c['n'], ptr, items, cnt)
        assert 'set_params first' in refused(fresh.cdae_grad, *batch(c))
        assert 'set_params first' in refused(fresh.cdae_load_factors)
    finally:
        fresh.close()


def test_the_user_lists_are_checked_against_their_own_bound():
    # m = 5 users, n = 3 items: a bound or a row count swapped at a call site of the shared check shows
    from helpers import row_list_cases as rl
    from yue_amd._shim import Device, YueHipError
    d = Device(0, raise_errors=True)
    try:
        ones = np.ones(rl.NNZ, np.int32)

        def upload(ptr, items, counts=ones):
            d.cdae_set_data(rl.M, rl.N, ptr, items, counts)
        base = {'ptr': rl.U_PTR.copy(), 'items': rl.U_ITEMS.copy()}
        rl.check_wiring('yue_cdae_set_data', upload, base, [('ptr', 'items', rl.N, True)])
        for bad in (0, 1 << 24):
            counts = ones.copy(); counts[3] = bad
            with pytest.raises(YueHipError, match=r'yue_cdae_set_data: user-major row 2: a count must be 1 \.\. 2\^24 - 1'):
                upload(counts=counts, **base)
            upload(**base)
    finally:
        d.close()
