"""CPU: APR's contract (tests/helpers/numpy_apr.py) against its goldens (tests/golden/g21_apr_*.json, tools/make_apr_goldens.py: they
pin the contract, not TensorFlow, which cannot run here), its three hand-derived gradients against central differences in fp64, the
whole-variable assign of the perturbation, the optimizer state running on from phase 1 into phase 2, the plugin's sampler on a
recorded log, the plugin on a stubbed device with its refusals, the conditioning statement of every GPU case, and the end-to-end
logs on the float32 contract."""
import json
import os
import random

import numpy as np
import pytest

from helpers import apr_cases as ac
from helpers import apr_e2e as ae
from helpers import numpy_apr as ap

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def golden(tag):
    return json.load(open(os.path.join(ROOT, 'tests', 'golden', 'g21_apr_%s.json' % tag)))


@pytest.mark.parametrize('name', ['base', 'k50', 'k64', 'ieqj'])
def test_contract_reproduces_the_goldens(name):
    z, c = golden(name), ac.build(name)
    assert z['seed'] == c['seed'] and z['T'] == len(c['u'])
    for q in ac.QUANTITIES:
        if q.startswith('loss'):
            assert abs(c['want'][q] - z[q]) <= 1e-12 * abs(z[q]), q
        else:
            a = np.asarray(c['want'][q], np.float64)
            assert np.allclose([a.sum(), np.abs(a).sum()], z[q], rtol=1e-11, atol=1e-13), q
    U, V, losses = ap.train(c['U'], c['V'], ac.step_batches(c), 3, 0.002, ac.REG, c['eps'], c['regA'], np.float64)
    assert np.allclose(losses, z['losses6'], rtol=1e-11, atol=0)
    for key, a in (('U6', U), ('V6', V)):
        assert np.allclose([a.sum(), np.abs(a).sum()], z[key], rtol=1e-10, atol=1e-13), key
    # the float32 figures depend on the library's float32 kernels to the last bit: the same size, not the same bits
    for q, v in z['d32'].items():
        assert c['d32'][q] <= 4 * v + 2.0 ** -24, q


def _tiny():
    """m = 4, n = 5, k = 3: user 1 in three triplets, item 2 positive and negative, a triplet twice, a non-zero perturbation on some rows."""
    rs = np.random.RandomState(2)
    U, V = rs.normal(0, 0.5, size=(4, 3)), rs.normal(0, 0.5, size=(5, 3))
    dU, dV = np.zeros_like(U), np.zeros_like(V)
    dU[[1, 3]], dV[[0, 2, 4]] = rs.normal(0, 0.3, size=(2, 3)), rs.normal(0, 0.3, size=(3, 3))
    u, i, j = [1, 0, 1, 3, 1, 0], [2, 4, 0, 2, 2, 4], [3, 2, 2, 1, 3, 2]
    return U, V, dU, dV, u, i, j


def _differences(f, arrays, grads, h=1e-5):
    """Worst |central difference - gradient| / max(1e-3, |central difference|) of scalar f() over every element of `arrays`."""
    worst = 0.0
    for X, g in zip(arrays, grads):
        for idx in np.ndindex(X.shape):
            old = X[idx]
            X[idx] = old + h
            lp = f()
            X[idx] = old - h
            lm = f()
            X[idx] = old
            fd = (lp - lm) / (2 * h)
            worst = max(worst, abs(fd - g[idx]) / max(1e-3, abs(fd)))
    return worst


def test_the_three_gradients_match_central_differences_in_fp64():
    U, V, dU, dV, u, i, j = _tiny()
    reg, regA = 0.05, 1.5
    _, gU, gV = ap.pre_loss_and_grad(U, V, u, i, j, reg)
    w_pre = _differences(lambda: float(ap.pre_loss_and_grad(U, V, u, i, j, reg)[0]), (U, V), (gU, gV))
    rU, rV = ap.delta_grad(U, V, dU, dV, u, i, j, regA)
    w_delta = _differences(lambda: float(ap.adv_loss(U, V, dU, dV, u, i, j, regA)), (dU, dV), (rU, rV))
    la, aU, aV = ap.adv_loss_and_grad(U, V, dU, dV, u, i, j, regA)
    w_adv = _differences(lambda: float(ap.adv_loss(U, V, dU, dV, u, i, j, regA)), (U, V), (aU, aV))
    assert abs(float(la) - float(ap.adv_loss(U, V, dU, dV, u, i, j, regA))) == 0
    print('worst relative differences: phase 1 %.3g, perturbation %.3g, adversarial %.3g' % (w_pre, w_delta, w_adv))
    # rows outside the batch: user 2 has no gradient of any kind
    assert not gU[2].any() and not rU[2].any() and not aU[2].any() and rU[1].any() and rV[2].any()
    # central differences at step h = 1e-5: truncation h^2 / 6 |f'''|, where a softplus's third derivative is below 0.1, a margin is
    # bilinear in rows below 2 in norm and at most 6 triplets (weights 1 and 1.5) share an element: |f'''| <= 20, so 3.4e-10;
    # rounding: the loss (below 20) is known to some 10 ulps of 2^-52, divided by 2 h: 2.2e-9; together 2.6e-9 over the 1e-3 floor
    # of the denominators: 2.6e-6
    assert max(w_pre, w_delta, w_adv) <= 3e-6


def test_the_assign_overwrites_the_whole_perturbation_and_the_gradient_is_taken_at_the_old_one():
    c = ac.build('carried')
    U, V, eps, regA = c['U'].astype(np.float64), c['V'].astype(np.float64), c['eps'], c['regA']
    first, second = (c['u1'], c['i1'], c['j1']), (c['u'], c['i'], c['j'])
    zero = (np.zeros_like(U), np.zeros_like(V))
    _, _, d1U, d1V = ap.delta_update(U, V, zero[0], zero[1], *first, eps, regA)
    in1_u, in1_i = np.unique(first[0]), np.unique(np.concatenate(first[1:]))
    assert np.allclose(np.linalg.norm(d1U[in1_u], axis=1), eps) and np.allclose(np.linalg.norm(d1V[in1_i], axis=1), eps)
    assert not np.delete(d1U, in1_u, axis=0).any() and not np.delete(d1V, in1_i, axis=0).any()
    r2U, r2V, d2U, d2V = ap.delta_update(U, V, d1U, d1V, *second, eps, regA)
    in2_u, in2_i = np.unique(second[0]), np.unique(np.concatenate(second[1:]))
    gone = np.setdiff1d(in1_u, in2_u)
    assert len(gone) and d1U[gone].any(axis=1).all() and not d2U[gone].any()             # a row of the first batch alone is zero again
    assert not np.delete(d2U, in2_u, axis=0).any() and not np.delete(d2V, in2_i, axis=0).any()
    # a row of both batches: its gradient is the one at the first batch's perturbation, not the one at zero
    shared = np.intersect1d(in1_u, in2_u)
    at_zero = ap.delta_grad(U, V, zero[0], zero[1], *second, regA)[0]
    by_hand = ap.delta_grad(U, V, d1U, d1V, *second, regA)[0]
    assert len(shared) and np.array_equal(r2U, by_hand) and ap.rel(r2U[shared], at_zero[shared]) > 1e-3


def test_the_step_count_and_the_moments_run_on_from_phase_one():
    c = ac.build('base')
    batches = ac.step_batches(c)
    U, V, losses = ap.train(c['U'], c['V'], batches, 3, 0.002, ac.REG, c['eps'], c['regA'])
    # by hand: one state through both phases, t = 1 .. 6
    U2, V2 = c['U'].astype(np.float64), c['V'].astype(np.float64)
    st, D = ap.new_state(U2, V2), ap.new_delta(U2, V2)
    for t in (1, 2, 3):
        ap.pre_step(U2, V2, st, *batches[t - 1], 0.002, ac.REG, t)
    m3 = st['mU'].copy()
    for t in (4, 5, 6):
        ap.adv_step(U2, V2, D, st, *batches[t - 1], 0.002, c['eps'], c['regA'], t)
    assert np.array_equal(U, U2) and np.array_equal(V, V2) and m3.any()
    # an optimizer of its own for phase 2 (fresh moments, t from 1) would end elsewhere
    U3, V3 = c['U'].astype(np.float64), c['V'].astype(np.float64)
    st, D = ap.new_state(U3, V3), ap.new_delta(U3, V3)
    for t in (1, 2, 3):
        ap.pre_step(U3, V3, st, *batches[t - 1], 0.002, ac.REG, t)
    st = ap.new_state(U3, V3)
    for t in (1, 2, 3):
        ap.adv_step(U3, V3, D, st, *batches[t + 2], 0.002, c['eps'], c['regA'], t)
    assert ap.rel(U3, U) > 1e-3
    # a row of phase 1's batches alone keeps moving in phase 2 on its old moments
    u4 = int(batches[0][0][4])
    assert u4 not in batches[3][0] and u4 not in batches[4][0] and u4 not in batches[5][0]
    after3 = ap.train(c['U'], c['V'], batches[:3], 3, 0.002, ac.REG, c['eps'], c['regA'])[0]
    assert (U[u4] != after3[u4]).all()


def _plugin(tmp_path, events, conf_edits=(), test=None):
    from yue_amd.recommender.advanced.APR import APR
    from yue_amd.tool.config import Config
    log = tmp_path / 'log.txt'
    log.write_text(''.join('%010d,u%d,t%d,a0\n' % (t, u, i) for t, (u, i) in enumerate(events)))
    text = open(os.path.join(ROOT, 'config', 'APR.conf')).read()
    text = text.replace('record=./dataset/log.txt', 'record=%s' % log).replace(' -byTime 0.2', '')
    for old, new in conf_edits:
        assert old in text, old
        text = text.replace(old, new)
    path = tmp_path / 'APR.conf'
    path.write_text(text)
    train = [{'user': 'u%d' % u, 'track': 't%d' % i, 'artist': 'a0', 'time': str(t)} for t, (u, i) in enumerate(events)]
    return APR(Config(str(path)), train, [dict(train[0])] if test is None else test)


def test_next_batch_on_a_fixed_log_and_seeds_gives_the_recorded_triplets(tmp_path, capsys):
    z = golden('sampler')
    rec = _plugin(tmp_path, list(zip(z['ev_u'], z['ev_t'])), [('batch_size=512', 'batch_size=%d' % z['batch_size'])])
    rec.readConfiguration()
    np.random.seed(3)
    rec.initModel()
    assert (rec.m, rec.n, rec.negativeCount, rec.batch_size, rec.train_size) == (z['m'], z['n'], z['neg'], z['batch_size'], len(z['ev_u']))
    # the start factors: truncated_normal(0.005), U first, after the base class's P and Q
    rs = np.random.RandomState(3)
    rs.rand(z['m'], rec.k); rs.rand(z['n'], rec.k)
    assert np.array_equal(rec.U, ap.truncated_normal(rs, (z['m'], rec.k))) and np.array_equal(rec.V, ap.truncated_normal(rs, (z['n'], rec.k)))
    assert np.abs(rec.U).max() <= 0.01
    np.random.seed(z['np_seed'])
    random.seed(z['sampler_seed'])
    for want in z['batches']:
        assert [list(map(int, x)) for x in rec.next_batch()] == want
    # ... which are the contract's sampler's on the plugin's own view of the log
    ev_u, ev_i, listened = ae.events(rec)
    assert ev_u == z['ev_u'] and ev_i == z['ev_t']
    np_rng = np.random.RandomState(z['np_seed'])
    random.seed(z['sampler_seed'])
    for want in z['batches']:
        got = ap.next_batch(ev_u, ev_i, listened, rec.n, rec.batch_size, rec.negativeCount, np_rng, random)
        assert [list(map(int, x)) for x in got] == want
        assert all(j not in listened[u] for u, j in zip(got[0], got[2]))


class StubDevice(object):
    """Records the plugin's calls; a step's loss is its step number."""

    def __init__(self):
        self.calls = []

    def set_factors(self, P, Q):
        self.calls.append(('set_factors', P.copy(), Q.copy()))

    def set_interactions(self, *a):
        self.calls.append(('set_interactions',))

    def adam_reset(self):
        self.calls.append(('adam_reset',))

    def apr_reset(self):
        self.calls.append(('apr_reset',))

    def apr_pre_step(self, u, i, j, lr, reg, step):
        self.calls.append(('pre', len(u), lr, reg, step))
        return float(step)

    def apr_adv_step(self, u, i, j, lr, eps, regA, step):
        self.calls.append(('adv', len(u), lr, eps, regA, step))
        return float(step)

    def get_factors(self, P, Q):
        self.calls.append(('get_factors',))
        P += 1
        return P, Q


def test_plugin_runs_both_phases_on_a_stubbed_device(tmp_path, capsys, monkeypatch):
    from yue_amd.recommender.advanced.APR import APR
    z = golden('sampler')
    rec = _plugin(tmp_path, list(zip(z['ev_u'], z['ev_t'])), [('batch_size=512', 'batch_size=4'), ('num.max.iter=100', 'num.max.iter=2'),
                                                                ('-advEpoch 100', '-advEpoch 3'), ('apr.hip=-neg 3', 'apr.hip=-neg 2')])
    rec.readConfiguration()
    rec.initModel()
    rec.dev = dev = StubDevice()
    monkeypatch.setattr(APR, 'ranking_performance', lambda self: dev.calls.append(('ranking', self.P[0, 0] - self.U0[0, 0])))
    rec.U0 = rec.U.copy()
    capsys.readouterr()
    rec.buildModel()
    out = capsys.readouterr().out.splitlines()
    assert out == ['training...'] + ['iteration: %d loss: %s' % (e, float(t)) for e, t in ((0, 1), (1, 2), (0, 3), (1, 4), (2, 5))]
    names = [c[0] for c in dev.calls]
    assert names == ['set_factors', 'set_interactions', 'adam_reset', 'apr_reset'] + ['pre', 'get_factors', 'ranking'] * 2 + ['adv', 'get_factors', 'ranking'] * 3
    assert np.array_equal(dev.calls[0][1], rec.U0)
    steps = [c for c in dev.calls if c[0] in ('pre', 'adv')]
    assert steps[:2] == [('pre', 8, 0.003, 0.002, 1), ('pre', 8, 0.003, 0.002, 2)]                    # regU, T = 2 * 4
    assert steps[2:] == [('adv', 8, 0.003, 0.5, 2.0, t) for t in (3, 4, 5)]                            # the step count runs on
    assert [round(float(c[1])) for c in dev.calls if c[0] == 'ranking'] == [1, 2, 3, 4, 5]             # P holds the copy before every ranking
    assert rec.U is rec.P and rec.V is rec.Q and rec.loss == 5.0


def test_menu_config_and_read_configuration(tmp_path, capsys):
    from yue_amd.main import MENU
    assert MENU['a10'] == 'APR' and MENU['a4'] == 'CDAE'
    events = [(0, 0), (0, 1), (1, 1), (1, 2)]
    rec = _plugin(tmp_path, events)
    rec.readConfiguration()
    assert (rec.k, rec.maxIter, rec.batch_size, rec.eps, rec.regAdv, rec.advEpoch, rec.negativeCount) == (64, 100, 512, 0.5, 2.0, 100, 3)
    assert (rec.lRate, rec.regU) == (0.003, 0.002)
    rec = _plugin(tmp_path, events, [('apr.hip=-neg 3\n', '')])
    rec.readConfiguration()
    assert rec.negativeCount == 3                                    # hard-coded in the reference
    rec = _plugin(tmp_path, events, [('apr.hip=-neg 3', 'apr.hip=-neg 7')])
    rec.readConfiguration()
    assert rec.negativeCount == 7
    number = 'negative'                                              # (how the line parser reads a leading minus depends on what follows it)
    for edit, words in ((('-eps 0.5', '-eps -0.5'), number), (('-regA 2', '-regA -1'), number), (('-regA 2', '-regA two'), number), (('-eps 0.5', '-eps nan'), '-eps and -regA must not be negative'),
                        (('-advEpoch 100', '-advEpoch -1'), '-advEpoch at least 0'), (('batch_size=512', 'batch_size=0'), 'batch_size and -neg must be at least 1'),
                        (('apr.hip=-neg 3', 'apr.hip=-neg 0'), 'batch_size and -neg must be at least 1')):
        rec = _plugin(tmp_path, events, [edit])
        capsys.readouterr()
        with pytest.raises(SystemExit) as e:
            rec.readConfiguration()
        assert e.value.code == -1 and words in capsys.readouterr().out


def test_plugin_refuses_array_native_data(tmp_path, capsys):
    from yue_amd import synth
    from yue_amd.data.arrays import ArrayRecord
    from yue_amd.recommender.advanced.APR import APR
    rec = _plugin(tmp_path, [(0, 0), (0, 1), (1, 1)])
    rec.readConfiguration()
    arrays = synth.make_arrays(6, 9, 3, seed=1)
    rec.data = ArrayRecord.__new__(ArrayRecord)
    assert isinstance(rec.data, ArrayRecord) and arrays is not None and isinstance(rec, APR)
    capsys.readouterr()
    with pytest.raises(SystemExit) as e:
        rec.initModel()
    assert e.value.code == -1 and 'array-native data is not supported' in capsys.readouterr().out


@pytest.mark.parametrize('name', ac.GPU_CASES + ac.EDGE_NAMES)
def test_every_gpu_case_meets_its_conditioning_statement(name):
    """Nothing a device computes enters here: the conditioning is the fp64 contract's, the edges are read off the case's batch."""
    c = ac.build(name)
    ratio, exact = ac.conditioning(c)
    print(name, 'smallest |g| / sum |term| %.3f' % ratio, 'exact', exact, ' '.join('%s %.3g' % (q, c['d32'][q]) for q in ac.QUANTITIES))
    assert ratio >= ac.FRACTION
    assert exact == ([('u', ac.LONE_USER), ('i', ac.LONE_ITEM)] if name == 'ieqj' else [])
    if name == 'carried':                                            # both of its updates: the first from zero, the second at the first's result
        U, V = c['U'].astype(np.float64), c['V'].astype(np.float64)
        zero = (np.zeros_like(U), np.zeros_like(V))
        first = (c['u1'], c['i1'], c['j1'])
        _, _, dU, dV = ap.delta_update(U, V, zero[0], zero[1], *first, c['eps'], c['regA'])
        assert ac.conditioning(c, zero[0], zero[1], *first)[0] >= ac.FRACTION
        assert ac.conditioning(c, dU, dV)[0] >= ac.FRACTION
    u, i, j = c['u'], c['i'], c['j']
    assert c['m'] <= 60 and c['n'] <= 100 and len(u) <= 200
    x = (c['U'][u].astype(np.float64) * (c['V'][i] - c['V'][j])).sum(axis=1)
    assert np.abs(x).max() < 10
    if len(u) >= 8 and c['kind'] != 'hubuser':
        assert list(zip(u[:4].tolist(), i[:4].tolist(), j[:4].tolist())) == ac.forced(c['m'], c['n'])
    if c['kind'] == 'hubuser':
        assert (u == ac.HUB_USER).all() and len(u) == 200 and not np.intersect1d(i, j).size
    if name not in ('T1', 'carried'):                                # the standing perturbation: rows of the batch with and without one, rows with one outside it
        for ids, rows in ((c['ids_i'], np.unique(np.concatenate([i, j]))),) + (((c['ids_u'], np.unique(u)),) if c['kind'] != 'hubuser' else ()):
            assert np.intersect1d(ids, rows).size and np.setdiff1d(rows, ids).size and (np.setdiff1d(ids, rows).size or name == 'ieqj')


@pytest.mark.parametrize('name', list(ae.PROBLEMS))
def test_e2e_logs_keep_the_float32_contract_inside_the_cap(tmp_path, capsys, orc, name):
    """What tests/test_gpu_apr_plugin.py asks of the device, asked of the float32 contract: the oracle's lists on its factors equal
    those on the fp64 factors for every compared user, and at most 2 % of the test users are left out."""
    rec, batches, seed = ae.plugin_on_cpu(tmp_path, name)
    capsys.readouterr()
    m, n = ae.PROBLEMS[name][:2]
    assert rec.m <= m <= 200 and rec.n <= n <= 150 and len(batches) == rec.maxIter + rec.advEpoch and rec.lRate == ae.LR
    Fc, losses = ae.contract_F(rec, rec.U, rec.V, batches, np.float64)
    F32, _ = ae.contract_F(rec, rec.U, rec.V, batches, np.float32)
    N = max(rec._top_list())
    names, uids, mp, mi = ae.ranked_users(rec)
    keep, dist = ae.compared_users(Fc, rec.m, uids, mp, mi, N, F32)
    want = ae.oracle_lists(orc, Fc, rec.m, uids, mp, mi, N)
    got = ae.oracle_lists(orc, F32, rec.m, uids, mp, mi, N)
    print(name, 'test users', len(uids), 'left out', int((~keep).sum()), 'distance %.3g' % dist, 'flipped elements', ae.flipped(F32, Fc, rec.lRate), 'of', Fc.size,
          'losses', losses)
    assert len(uids) >= 50 and (~keep).sum() <= ae.CAP * len(uids)
    assert np.array_equal(got[keep], want[keep])
    assert ae.flipped(F32, Fc, rec.lRate) == 0
