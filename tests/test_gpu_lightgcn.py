"""GPU: LightGCN's device path (yue_lgcn_*) through the shim on synthetic graphs from seeds
(tests/helpers/lightgcn_cases.py), against the fp64 contract tests/helpers/numpy_lightgcn.py.
Bounds: raw layers, F, gU, gV within 4 x the case's d32 (the float32 contract's own distance from fp64, required <= 1e-5) in
relative max-norm -- the device sums in another order than NumPy; the loss within 4 x the float32 contract's loss distance;
yue_lgcn_step within 1e-6 lr of the contract's Adam fed the device's own gradient; five steps' losses within 1e-5.
End to end, Yue(conf).execute() on a yue_amd.synth log: the ranking lists equal the top-N oracle's on the fp64 contract's F for
every user the rule of tests/helpers/lightgcn_e2e.py compares, and that rule leaves out at most 5 % of the test users."""
import random

import numpy as np
import pytest

from helpers import lightgcn_cases as lc
from helpers import lightgcn_e2e as le
from helpers import numpy_lightgcn as nl

pytestmark = pytest.mark.gpu

MAIN = ['k1', 'k20', 'k63', 'k64', 'k65', 'k128', 'w81', 'layers1', 'layers2', 'layers3']


@pytest.fixture(scope='module')
def dev():
    from yue_amd._shim import Device
    d = Device(0, raise_errors=True)
    yield d
    d.close()


def upload(dev, c):
    g = c['g']
    dev.set_option('lgcn_hub', c['hub'] if c['hub'] else 1024)
    dev.set_factors(c['U'], c['V'])
    dev.lgcn_set_graph(c['m'], c['n'], g['u_ptr'], g['u_items'], g['u_w'], g['i_ptr'], g['i_users'], g['i_w'])


def check_case(dev, c):
    """Forward, loss and gradient of one case against its bounds; returns the measured figures."""
    d32, L = c['d32'], c['layers']
    assert all(v <= 1e-5 for v in d32.values()), d32
    upload(dev, c)
    E, F = dev.lgcn_propagate(L, raw=True)
    loss, gU, gV = dev.lgcn_grad(L, c['u'], c['i'], c['j'], lc.REG)
    got = {'F': nl.rel(F, c['F']), 'gU': nl.rel(gU, c['gU']), 'gV': nl.rel(gV, c['gV']), 'loss': abs(loss - c['loss']) / abs(c['loss'])}
    for l in range(1, L + 1):
        got['E%d' % l] = nl.rel(E[l - 1], c['E'][l])
    print(c['name'], ' '.join('%s %.3g (d32 %.3g)' % (key, got[key], d32[key]) for key in sorted(got)))
    for key in got:
        assert got[key] <= 4 * d32[key], (key, got[key], d32[key])
    return got


@pytest.mark.parametrize('name', MAIN)
def test_forward_loss_and_gradient(dev, name):
    check_case(dev, lc.build(name))


@pytest.mark.parametrize('name', ['k20', 'k65', 'k128'])
def test_step_is_the_contracts_adam_on_the_devices_gradient(dev, name):
    c = lc.build(name)
    lr = 0.002
    upload(dev, c)
    dev.adam_reset()
    U, V = c['U'].copy(), c['V'].copy()
    st = nl.new_state(U, V)
    for t in (1, 2, 3):
        _, gU, gV = dev.lgcn_grad(c['layers'], c['u'], c['i'], c['j'], lc.REG)
        loss_g = dev.lgcn_grad(c['layers'], c['u'], c['i'], c['j'], lc.REG)[0]
        loss = dev.lgcn_step(c['layers'], c['u'], c['i'], c['j'], lr, lc.REG, t)
        assert loss == loss_g
        nl.adam(U, gU, st['mU'], st['vU'], lr, t, np.float32)
        nl.adam(V, gV, st['mV'], st['vV'], lr, t, np.float32)
        P, Q = dev.get_factors()
        mU, vU, mV, vV = dev.adam_get_moments()
        dU, dV = np.abs(P - U).max(), np.abs(Q - V).max()
        print(name, 'step', t, 'max |dU| %.3g |dV| %.3g (bound %.3g)' % (dU, dV, 1e-6 * lr))
        assert dU <= 1e-6 * lr and dV <= 1e-6 * lr
        for a, b in ((mU, st['mU']), (vU, st['vU']), (mV, st['mV']), (vV, st['vV'])):
            assert nl.rel(a, b) <= 1e-6
        # the contract goes on from the device's factors, so that a step's check does not inherit the last one's rounding
        U, V = P.copy(), Q.copy()
        for key, a in (('mU', mU), ('vU', vU), ('mV', mV), ('vV', vV)):
            st[key] = a.copy()


def test_five_steps_losses_follow_the_fp64_contract(dev):
    rs = np.random.RandomState(77)
    m, n, k, L, lr = 300, 200, 64, 3, 0.002
    pu, pi, w = nl.synthetic_pairs(rs, m, n, rs.randint(1, 12, size=m), (1.0, 4.0, 9.0))
    g = nl.graph_from_pairs(pu, pi, w, m, n)
    U, V = nl.truncated_normal(rs, (m, k)), nl.truncated_normal(rs, (n, k))
    batches = [(rs.randint(0, m, 128), rs.randint(0, n, 128), rs.randint(0, n, 128)) for _ in range(5)]
    dev.set_option('lgcn_hub', 1024)
    dev.set_factors(U, V)
    dev.lgcn_set_graph(m, n, g['u_ptr'], g['u_items'], g['u_w'], g['i_ptr'], g['i_users'], g['i_w'])
    dev.adam_reset()
    U64, V64 = U.astype(np.float64), V.astype(np.float64)
    st = nl.new_state(U64, V64)
    for t, (u, i, j) in enumerate(batches, 1):
        want = float(nl.step(g, U64, V64, st, u, i, j, lr, lc.REG, t, L, np.float64))
        got = dev.lgcn_step(L, u, i, j, lr, lc.REG, t)
        print('step', t, 'loss', got, 'fp64', want, 'rel %.3g' % (abs(got - want) / abs(want)))
        assert abs(got - want) <= 1e-5 * abs(want)


@pytest.mark.parametrize('name', ['k64', 'k128'])
def test_repeat_runs_are_bit_identical(dev, name):
    c = lc.build(name)
    upload(dev, c)
    a = dev.lgcn_grad(c['layers'], c['u'], c['i'], c['j'], lc.REG)
    Fa = dev.lgcn_propagate(c['layers'])
    b = dev.lgcn_grad(c['layers'], c['u'], c['i'], c['j'], lc.REG)
    Fb = dev.lgcn_propagate(c['layers'])
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(Fa, Fb)


@pytest.mark.parametrize('name', sorted(le.PROBLEMS))
def test_execute_ranks_as_the_oracle_on_the_contracts_F(tmp_path, capsys, monkeypatch, orc, name):
    """The plugin on the device from the config file to the lists: the graph through yue_lgcn_set_graph's checks, adam_reset and
    the steps of every epoch, the final propagation, P = F[:m] and Q = F[m:] through the existing scan."""
    from yue_amd.base.IterativeRecommender import IterativeRecommender
    from yue_amd.recommender.advanced.LightGCN import LightGCN
    from yue_amd.yue import Yue
    conf = le.config(tmp_path, name)
    seed, line = le.PROBLEMS[name][4], le.PROBLEMS[name][8]
    kept = {'batches': [], 'scans': []}
    build, sample, scan = LightGCN.buildModel, LightGCN.next_batch_pairwise, IterativeRecommender._scan

    def spy_build(self):
        kept['rec'], kept['U0'], kept['V0'] = self, self.U.copy(), self.V.copy()
        random.seed(seed)
        return build(self)

    def spy_sample(self):
        for batch in sample(self):
            kept['batches'].append(tuple(list(x) for x in batch))
            yield batch

    def spy_scan(self, users, N, mask=None):
        ids = scan(self, users, N, mask)
        kept['scans'].append((list(users), N, mask, ids.copy()))
        return ids
    monkeypatch.setattr(LightGCN, 'buildModel', spy_build)
    monkeypatch.setattr(LightGCN, 'next_batch_pairwise', spy_sample)
    monkeypatch.setattr(IterativeRecommender, '_scan', spy_scan)
    np.random.seed(seed)
    Yue(conf).execute()
    out = capsys.readouterr().out
    rec = kept['rec']
    assert (rec.n_layers, rec.negativeCount) == ((2, 3) if line else (3, 5))
    # the fp64 contract from the plugin's own start, on the plugin's own batches
    F64, batches = le.contract_F(rec, kept['U0'], kept['V0'], seed, np.float64)
    assert kept['batches'] == batches and len(batches[-1][0]) < rec.batch_size
    lines = [ln for ln in out.splitlines() if ln.startswith('training:')]
    per_epoch = len(batches) // rec.maxIter
    assert [ln.split(' loss:')[0] for ln in lines] == ['training: %d batch %d' % (it + 1, b) for it in range(rec.maxIter) for b in range(per_epoch)]
    assert all(np.isfinite(float(ln.split(' loss: ')[1])) for ln in lines)
    # the factors the scan ranked with are the device's F of the trained U, V
    F = np.concatenate([rec.P, rec.Q])
    assert F.dtype == np.float32 and F.shape == F64.shape and rec.U.shape == kept['U0'].shape and not np.array_equal(rec.U, kept['U0'])
    N = max(rec._top_list())
    names, uids, mp, mi = le.ranked_users(rec)
    keep, dist = le.compared_users(F64, rec.m, uids, mp, mi, N, F)
    want = le.oracle_lists(orc, F64, rec.m, uids, mp, mi, N)
    assert len(kept['scans']) == 1                                # evalRanking's one scan
    users, n_asked, mask, got = kept['scans'][0]
    assert users == names and n_asked == N and mask is None and got.shape == want.shape
    differ = ~(got == want).all(axis=1)
    print(name, 'test users', len(uids), 'left out', int((~keep).sum()), 'F distance %.3g abs, %.3g rel' % (dist, nl.rel(F, F64)),
          'lists that differ', int(differ.sum()), 'of them compared', int((differ & keep).sum()))
    assert len(uids) >= 50 and (~keep).sum() <= 0.05 * len(uids)
    assert np.array_equal(got[keep], want[keep])
    assert rec.measure and rec.measure[0] == 'Top 5\n'
