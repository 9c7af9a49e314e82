"""GPU: NGCF's device path (yue_ngcf_*) through the shim on synthetic graphs from seeds
(tests/helpers/ngcf_cases.py), against the fp64 contract tests/helpers/numpy_ngcf.py.
Bounds: S, Z, D of every layer, F, gU, gV, gW within 4 x the case's d32 (the float32 contract's own distance from fp64) in relative
max-norm -- the device sums in another order than NumPy; the loss within 4 x the float32 contract's loss distance; the device's
dropout mask equal to the host's at every element; yue_ngcf_step within 1e-6 lr of the contract's float32 Adam fed the device's
own gradients; five steps' losses within 1e-5 of fp64; repeat runs bit-identical.  tests/test_ngcf_golden.py asserts on the CPU
that every case satisfies the leaky-ReLU condition (no sign of Z within reach of float32 rounding)."""
import numpy as np
import pytest

from helpers import lightgcn_cases as lc
from helpers import ngcf_cases as nc
from helpers import numpy_lightgcn as nl
from helpers import numpy_ngcf as ng

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    from yue_amd._shim import Device
    d = Device(0, raise_errors=True)
    yield d
    d.close()


def upload(dev, c, hub=None):
    g = c['g']
    dev.set_option('ngcf_hub', hub if hub else (c['hub'] if c['hub'] else 1024))
    dev.set_factors(c['U'], c['V'])
    dev.ngcf_set_graph(c['m'], c['n'], g['ptr'], g['col'], g['w'])
    dev.ngcf_set_weights(c['W'])


def run_args(c):
    return (c['layers'], c['training'], c['keep'], c['mask_seed'], c['step'])


def parts_of(degree, hub):
    big = degree[degree > hub]
    return len(big), int(((big + hub - 1) // hub).sum())


def check_case(dev, c):
    """Forward, mask, loss and gradients of one case against its bounds; returns the measured figures."""
    d32, L, fw = c['d32'], c['layers'], c['fw']
    upload(dev, c)
    S, Z, D, F = dev.ngcf_propagate(*run_args(c), parts=True)
    loss, gU, gV, gW = dev.ngcf_grad(*run_args(c), c['u'], c['i'], c['j'], nc.REG)
    got = {'F': ng.rel(F, fw['F']), 'gU': ng.rel(gU, c['gU']), 'gV': ng.rel(gV, c['gV']), 'gW': ng.rel(gW, c['gW']),
           'loss': abs(loss - c['loss']) / abs(c['loss'])}
    for l in range(L):
        for key, a in (('S', S), ('Z', Z), ('D', D)):
            got['%s%d' % (key, l + 1)] = ng.rel(a[l], fw[key][l])
    print(c['name'], ' '.join('%s %.3g (d32 %.3g, x%.2f)' % (key, got[key], d32[key], got[key] / d32[key] if d32[key] else 0.0) for key in sorted(got)))
    # the device's mask is the host's: an element with H != 0 is dropped exactly where the host drops it
    for l in range(L):
        H = np.where(Z[l] > 0, Z[l], np.float32(ng.SLOPE) * Z[l])
        assert np.array_equal((D[l] != 0)[H != 0], fw['kept'][l][H != 0]), 'mask of layer %d' % l
        assert c['training'] or np.array_equal(D[l], H)
    for key in got:
        assert got[key] <= 4 * d32[key], (key, got[key], d32[key])
    return got


@pytest.mark.parametrize('name', nc.GPU_CASES)
def test_forward_mask_loss_and_gradients(dev, name):
    c = nc.build(name)
    check_case(dev, c)
    if c['edges']:
        hubs = [parts_of(c['g']['degree'], nc.HUB), parts_of(c['g']['T']['degree'], nc.HUB)]
        assert hubs[0][0] >= 1 and hubs[1][0] >= 1
        assert dev.get_option('ngcf_last_hubs') == hubs[0][0] + hubs[1][0] and dev.get_option('ngcf_last_parts') == hubs[0][1] + hubs[1][1]


@pytest.mark.parametrize('name', ['k2', 'k33', 'k85'])
def test_step_is_the_contracts_adam_on_the_devices_gradients(dev, name):
    c = nc.build(name)
    lr, L = 0.002, c['layers']
    upload(dev, c)
    dev.adam_reset()
    U, V, W = c['U'].copy(), c['V'].copy(), c['W'].copy()
    st = ng.new_state(U, V, W)
    for t in (1, 2, 3):
        args = (L, c['training'], c['keep'], c['mask_seed'])
        loss_g, gU, gV, gW = dev.ngcf_grad(*args, t, c['u'], c['i'], c['j'], nc.REG)
        loss = dev.ngcf_step(*args, c['u'], c['i'], c['j'], lr, nc.REG, t)
        assert loss == loss_g
        for var, grad, mk, vk in ((U, gU, 'mU', 'vU'), (V, gV, 'mV', 'vV'), (W, gW, 'mW', 'vW')):
            ng.adam(var, grad, st[mk], st[vk], lr, t, np.float32)
        P, Q = dev.get_factors()
        Wd, mW, vW = dev.ngcf_get_weights(moments=True)
        mU, vU, mV, vV = dev.adam_get_moments()
        dU, dV, dW = np.abs(P - U).max(), np.abs(Q - V).max(), np.abs(Wd - W).max()
        print(name, 'step', t, 'max |dU| %.3g |dV| %.3g |dW| %.3g (bound %.3g)' % (dU, dV, dW, 1e-6 * lr))
        assert dU <= 1e-6 * lr and dV <= 1e-6 * lr and dW <= 1e-6 * lr
        got = {'mU': mU, 'vU': vU, 'mV': mV, 'vV': vV, 'mW': mW, 'vW': vW}
        for key in got:
            assert ng.rel(got[key], st[key]) <= 1e-6, key
        # the contract goes on from the device's state, so that a step's check does not inherit the last one's rounding
        U, V, W = P.copy(), Q.copy(), Wd.copy()
        for key in got:
            st[key] = got[key].copy()


def test_five_steps_losses_follow_the_fp64_contract(dev):
    rs = np.random.RandomState(78)
    m, n, k, L, lr, keep, seed = 300, 320, 64, 3, 0.002, 0.9, 4242
    pu, pt, w = nl.synthetic_pairs(rs, m, n, rs.randint(1, 12, size=m), (0.1, 0.3, 0.6))
    g = ng.graph_from_pairs(pu, pt, w, m, n, 'written')
    U, V, W = nl.truncated_normal(rs, (m, k)), nl.truncated_normal(rs, (n, k)), ng.xavier(rs, L, k)
    batches = [(rs.randint(0, m, 128), rs.randint(0, n, 128), rs.randint(0, n, 128)) for _ in range(5)]
    dev.set_option('ngcf_hub', 1024)
    dev.set_factors(U, V)
    dev.ngcf_set_graph(m, n, g['ptr'], g['col'], g['w'])
    dev.ngcf_set_weights(W)
    dev.adam_reset()
    U64, V64, W64 = U.astype(np.float64), V.astype(np.float64), W.astype(np.float64)
    st = ng.new_state(U64, V64, W64)
    for t, (u, i, j) in enumerate(batches, 1):
        want = float(ng.step(g, U64, V64, W64, st, u, i, j, lr, nc.REG, t, True, keep, seed, np.float64))
        got = dev.ngcf_step(L, True, keep, seed, u, i, j, lr, nc.REG, t)
        print('step', t, 'loss', got, 'fp64', want, 'rel %.3g' % (abs(got - want) / abs(want)))
        assert abs(got - want) <= 1e-5 * abs(want)
    for key in ('gather', 'dense', 'batch', 'backward', 'wgrad', 'adam'):
        assert dev.get_option('ngcf_last_%s_ns' % key) > 0, key


@pytest.mark.parametrize('name', ['k64', 'deg_written'])
def test_repeat_runs_are_bit_identical_also_across_a_change_of_hub(dev, name):
    c = nc.build(name)
    upload(dev, c)
    a = dev.ngcf_grad(*run_args(c), c['u'], c['i'], c['j'], nc.REG)
    Fa = dev.ngcf_propagate(*run_args(c))
    b = dev.ngcf_grad(*run_args(c), c['u'], c['i'], c['j'], nc.REG)
    Fb = dev.ngcf_propagate(*run_args(c))
    assert a[0] == b[0] and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:])) and np.array_equal(Fa, Fb)
    dev.set_option('ngcf_hub', 7)                                # other parts: other sums, all within the bounds, not the same bits
    other = dev.ngcf_grad(*run_args(c), c['u'], c['i'], c['j'], nc.REG)
    assert dev.get_option('ngcf_last_hubs') > 0 and ng.rel(other[1], c['gU']) <= 4 * c['d32']['gU']
    dev.set_option('ngcf_hub', c['hub'] if c['hub'] else 1024)
    back = dev.ngcf_grad(*run_args(c), c['u'], c['i'], c['j'], nc.REG)
    assert a[0] == back[0] and all(np.array_equal(x, y) for x, y in zip(a[1:], back[1:]))


def test_refusals(dev):
    from yue_amd._shim import ERR_ARG, YueHipError
    c = nc.build('k32')
    g, u, i, j = c['g'], c['u'], c['i'], c['j']

    def refused(f, *a, **kw):
        with pytest.raises(YueHipError) as e:
            f(*a, **kw)
        assert e.value.code == ERR_ARG, e.value
        return str(e.value)
    upload(dev, c)
    L = c['layers']
    assert '(layers + 1) k' in refused(dev.ngcf_propagate, 8)                              # 9 * 32 > 256
    refused(dev.ngcf_propagate, 0)
    refused(dev.ngcf_propagate, L, True, 0.0)
    refused(dev.ngcf_propagate, L, True, 1.5)
    refused(dev.ngcf_propagate, L, True, float('nan'))
    refused(dev.ngcf_grad, L, True, 0.9, 1, 1, u[:0], i[:0], j[:0], nc.REG)               # T < 1
    bad = u.copy(); bad[3] = c['m']
    refused(dev.ngcf_grad, L, True, 0.9, 1, 1, bad, i, j, nc.REG)
    bad = j.copy(); bad[0] = -1
    refused(dev.ngcf_step, L, True, 0.9, 1, u, i, bad, 0.002, nc.REG, 1)
    refused(dev.ngcf_step, L, True, 0.9, 1, u, i, j, 0.002, nc.REG, 0)                    # Adam's step counts from 1
    assert 'weights were set for' in refused(dev.ngcf_propagate, 2)                        # weights for other shapes
    # the graph's checks, before anything is stored: the good graph stays in place
    col = g['col'].copy(); col[0] = c['m'] + c['n']
    assert 'out of range' in refused(dev.ngcf_set_graph, c['m'], c['n'], g['ptr'], col, g['w'])
    row = int(np.flatnonzero(g['degree'] >= 2)[0])
    col = g['col'].copy(); col[g['ptr'][row] + 1] = col[g['ptr'][row]]
    assert 'sorted and unique' in refused(dev.ngcf_set_graph, c['m'], c['n'], g['ptr'], col, g['w'])
    w = g['w'].copy(); w[0] = np.inf
    refused(dev.ngcf_set_graph, c['m'], c['n'], g['ptr'], g['col'], w)
    F = dev.ngcf_propagate(*run_args(c))
    assert ng.rel(F, c['fw']['F']) <= 4 * c['d32']['F']
    # other shapes: factors of another size than the graph's, k > 128, no weights, no graph
    dev.set_factors(c['U'][:-1], c['V'])
    assert 'graph was set for' in refused(dev.ngcf_propagate, L)
    dev.set_factors(np.zeros((c['m'], 129), np.float32), np.zeros((c['n'], 129), np.float32))
    assert 'k <= 128' in refused(dev.ngcf_propagate, 1)
    from yue_amd._shim import Device
    fresh = Device(0, raise_errors=True)
    try:
        fresh.set_factors(c['U'], c['V'])
        assert 'set_graph first' in refused(fresh.ngcf_propagate, L)
        fresh.ngcf_set_graph(c['m'], c['n'], g['ptr'], g['col'], g['w'])
        assert 'set_weights first' in refused(fresh.ngcf_propagate, L)
        refused(fresh.ngcf_set_weights, np.zeros((3, 2, 65, 65), np.float32))               # 4 * 65 > 256
    finally:
        fresh.close()


def test_lightgcn_still_gives_its_result_after_ngcf_calls(dev):
    c = nc.build('k32')
    upload(dev, c)
    dev.ngcf_grad(*run_args(c), c['u'], c['i'], c['j'], nc.REG)
    lg = lc.build('k64')
    g = lg['g']
    dev.set_option('lgcn_hub', 1024)
    dev.set_factors(lg['U'], lg['V'])
    dev.lgcn_set_graph(lg['m'], lg['n'], g['u_ptr'], g['u_items'], g['u_w'], g['i_ptr'], g['i_users'], g['i_w'])
    loss, gU, gV = dev.lgcn_grad(lg['layers'], lg['u'], lg['i'], lg['j'], lc.REG)
    assert nl.rel(gU, lg['gU']) <= 4 * lg['d32']['gU'] and nl.rel(gV, lg['gV']) <= 4 * lg['d32']['gV']
    assert abs(loss - lg['loss']) / abs(lg['loss']) <= 4 * lg['d32']['loss']


def test_the_graph_is_checked_against_its_own_bound():
    # m = 5 users, n = 3 items, the (m + n)-row graph of both directions
    from helpers import row_list_cases as rl
    from yue_amd._shim import Device, YueHipError
    d = Device(0, raise_errors=True)
    try:
        base = {'ptr': np.concatenate([rl.U_PTR, rl.NNZ + rl.I_PTR[1:]]), 'col': np.concatenate([rl.M + rl.U_ITEMS, rl.I_USERS]).astype(np.int32)}
        w = np.full(2 * rl.NNZ, 0.5, np.float32)

        def upload(ptr, col, w=w):
            d.ngcf_set_graph(rl.M, rl.N, ptr, col, w)
        rl.check_wiring('yue_ngcf_set_graph', upload, base, [('ptr', 'col', rl.M + rl.N, True)])
        inf = w.copy(); inf[2] = np.inf
        with pytest.raises(YueHipError, match='yue_ngcf_set_graph: graph row 1: weight not finite'):
            upload(w=inf, **base)
        upload(**base)
    finally:
        d.close()
