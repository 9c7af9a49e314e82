"""CPU: the LightGCN contract (tests/helpers/numpy_lightgcn.py) against what the reference's own class computes in plain
Python (tests/golden/g17_lightgcn_*: the graph's lists and the sampler), its hand-written backward pass against central
differences, the float32 contract's distance from the fp64 one for every case the GPU tests use, the plugin's batches and
prints on a stubbed device (defaults and a ``lightgcn.hip`` override), its refusal of array-native data, and the end-to-end
problems' seeds (tests/helpers/lightgcn_e2e.py): the float32 contract alone stays inside the rule the device is held to."""
import json
import os
import random

import numpy as np
import pytest

from helpers import lightgcn_cases as lc
from helpers import lightgcn_e2e as le
from helpers import numpy_lightgcn as nl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')


def golden(tag):
    return json.load(open(os.path.join(GOLDEN, 'g17_lightgcn_%s.json' % tag)))


@pytest.mark.parametrize('tag', ['a', 'b'])
def test_graph_lists_equal_the_reference(tag):
    z = golden(tag)
    g = nl.graph_from_events(z['ev_u'], z['ev_i'], z['m'], z['n'])
    assert g['indices'] == z['indices'] and g['values'] == z['values']
    assert z['dense_shape'] == [z['m'] + z['n']] * 2
    # events are not deduplicated and the matmul sums repeated indices: a pair listened c times weighs c * c
    dense = np.zeros(z['dense_shape'])
    for (r, c), v in zip(z['indices'], z['values']):
        dense[r, c] += v
    ours = np.zeros_like(dense)
    rows = np.repeat(np.arange(z['m'] + z['n']), g['degree'])
    ours[rows, g['col']] = g['w']
    assert np.array_equal(dense, ours) and np.array_equal(dense, dense.T)
    c = int(max(z['values']))
    assert c > 1 and (dense == c * c).any() and g['w'].max() == c * c


@pytest.mark.parametrize('tag', ['a', 'b'])
def test_sampler_equals_the_reference(tag):
    z = golden(tag)
    listened = {}
    for u, i in zip(z['ev_u'], z['ev_i']):
        listened.setdefault(u, set()).add(i)
    random.seed(z['sampler_seed'])
    got = [list(b) for b in nl.next_batch_pairwise(z['ev_u'], z['ev_i'], listened, z['n'], z['batch_size'], z['negatives'], random)]
    assert got == z['batches']
    # one triplet per event (the fifth negative), events in order, the last batch short
    assert sum(len(b[0]) for b in got) == len(z['ev_u']) and len(got[-1][0]) < z['batch_size']
    assert [u for b in got for u in b[0]] == z['ev_u'] and [i for b in got for i in b[1]] == z['ev_i']
    assert all(j not in listened[u] for b in got for u, j in zip(b[0], b[2]))


def test_backward_pass_agrees_with_central_differences():
    """fp64, 3 layers, 20 triplets on m = 7, n = 9, k = 5.  User 5 and item 7 form an isolated pair with E_0 rows of magnitude
    1e-8, so their layers stay in the 1e-12 branch of l2_normalize (where the op is x * 1e6); user 6 and item 8 have no
    neighbour.  The two kinds of rows are measured apart: the clamped rows' derivatives are 1e6 times the others'."""
    rs = np.random.RandomState(5)
    m, n, k, L = 7, 9, 5, 3
    pu = [0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 4, 5]
    pi = [0, 1, 2, 1, 3, 2, 4, 5, 0, 6, 3, 1, 7]
    w = [1, 4, 1, 9, 1, 1, 4, 1, 1, 1, 9, 1, 1]
    g = nl.graph_from_pairs(pu, pi, w, m, n)
    assert g['degree'][6] == 0 and g['degree'][m + 8] == 0 and g['degree'][5] == 1 and g['degree'][m + 7] == 1
    U, V = rs.uniform(-1, 1, (m, k)), rs.uniform(-1, 1, (n, k))
    U[5] *= 1e-8
    V[7] *= 1e-8
    u, i, j = rs.randint(0, m, 20), rs.randint(0, n, 20), rs.randint(0, n, 20)
    u[:3], i[:3], j[:3] = [5, 6, 0], [7, 8, 7], [0, 1, 8]
    E, ss, _ = nl.propagate(g, U, V, L)
    assert all(ss[l][5] < nl.EPS and ss[l][m + 7] < nl.EPS and ss[l][6] == 0 for l in range(1, L + 1))
    assert all((np.delete(ss[l], [5, 6, m + 7, m + 8]) > 1e-3).all() for l in range(1, L + 1))
    loss, gU, gV, _, _ = nl.loss_and_grad(g, U, V, u, i, j, 0.05, L)

    def f(Ux, Vx):
        return float(nl.loss_and_grad(g, Ux, Vx, u, i, j, 0.05, L)[0])

    fdU, fdV = np.zeros_like(U), np.zeros_like(V)
    for X, fd, which in ((U, fdU, 0), (V, fdV, 1)):
        for r in range(X.shape[0]):
            for e in range(X.shape[1]):
                h = 1e-5 if abs(X[r, e]) > 1e-6 else 1e-11         # (a clamped row moves F by 1e6 h)
                Xp, Xm = X.copy(), X.copy()
                Xp[r, e] += h
                Xm[r, e] -= h
                fd[r, e] = (f(Xp, V) - f(Xm, V)) / (2 * h) if which == 0 else (f(U, Xp) - f(U, Xm)) / (2 * h)
    clamped = nl.rel(np.concatenate([fdU[5], fdV[7]]), np.concatenate([gU[5], gV[7]]))
    live = nl.rel(np.concatenate([np.delete(fdU, 5, 0).ravel(), np.delete(fdV, 7, 0).ravel()]),
                  np.concatenate([np.delete(gU, 5, 0).ravel(), np.delete(gV, 7, 0).ravel()]))
    print('finite differences: live rows %.3g, clamped rows %.3g' % (live, clamped))
    assert np.abs(gU[5]).max() > 1e3 and np.abs(gU[6]).max() > 0
    assert live <= 1e-7 and clamped <= 1e-7


@pytest.mark.parametrize('name', [c['name'] for c in lc.CASES])
def test_cases_reach_their_branches_and_float32_stays_close(name):
    c = lc.build(name)
    print(name, ' '.join('%s %.3g' % kv for kv in sorted(c['d32'].items())))
    assert all(v <= 1e-5 for v in c['d32'].values()), c['d32']
    deg = c['g']['degree']
    assert deg[0] == 0 and deg.max() >= 10 and c['g']['ptr'][-1] == 2 * len(c['g']['u_items'])
    if c['degrees'] is not None:
        assert list(deg[:len(lc.EDGE_DEGREES)]) == lc.EDGE_DEGREES
        hubs = deg[deg > c['hub']]
        assert sorted(hubs) == [lc.HUB + 1, 2 * lc.HUB + 37] and (2 * lc.HUB + 37) % lc.HUB != 0
    if len(c['weights']) > 1:
        assert set(np.unique(c['g']['w'])) == {1.0, 81.0}
    if c['batch'] == 'repeat':
        assert len(c['u']) == 64 and len(set(zip(c['u'], c['i'], c['j']))) == 1
    elif c['batch'] == 'posneg':
        assert c['i'][0] == c['j'][1]
    else:
        assert len(c['u']) == c['T'] and c['u'][0] == 0
    assert len(c['E']) == c['layers'] + 1


def test_adam_restates_the_live_path_oracle():
    """Statement for statement oracle/numpy_adam.py's update; lr_t from the decimal betas, as the library's host code forms it
    (the oracle rounds the betas to float32 first, which moves lr_t by 6e-6 at t = 1)."""
    import oracle.numpy_adam as na
    rs = np.random.RandomState(2)
    var, grad = rs.standard_normal((5, 7)).astype(np.float32), rs.standard_normal((5, 7)).astype(np.float32)
    m, v = np.zeros_like(var), np.zeros_like(var)
    ref, rm, rv = var.copy(), m.copy(), v.copy()
    for t in (1, 2, 3):
        nl.adam(var, grad, m, v, 0.002, t, np.float32)
        lr_t = np.float32(0.002 * np.sqrt(1.0 - 0.999 ** t) / (1.0 - 0.9 ** t))
        rm *= na.BETA1
        rm += (np.float32(1) - na.BETA1) * grad
        rv *= na.BETA2
        rv += (np.float32(1) - na.BETA2) * grad * grad
        ref -= lr_t * rm / (np.sqrt(rv) + na.EPS)
        assert np.array_equal(var, ref) and np.array_equal(m, rm) and np.array_equal(v, rv)


class StubDevice(object):
    """Records what the plugin hands to the device; the loss of a step is its number."""

    def __init__(self):
        self.calls, self.steps = [], []

    def set_factors(self, P, Q):
        self.m, self.n, self.k = P.shape[0], Q.shape[0], P.shape[1]
        self.P, self.Q = P.copy(), Q.copy()
        self.calls.append('set_factors')

    def set_interactions(self, *a):
        self.calls.append('set_interactions')

    def lgcn_set_graph(self, m, n, *lists):
        self.graph = (m, n) + tuple(np.asarray(x) for x in lists)
        self.calls.append('lgcn_set_graph')

    def adam_reset(self):
        self.calls.append('adam_reset')

    def lgcn_step(self, layers, u, i, j, lr, reg, step):
        self.steps.append((layers, list(u), list(i), list(j), lr, reg, step))
        return float(step)

    def get_factors(self):
        return self.P, self.Q

    def lgcn_propagate(self, layers):
        self.calls.append('lgcn_propagate')
        self.propagated = getattr(self, 'propagated', []) + [layers]
        return np.concatenate([self.P, self.Q]) * 2


@pytest.mark.parametrize('line,layers,neg', [(None, 3, 5), ('-layers 2 -neg 3', 2, 3), ('-neg 1', 3, 1)])
def test_plugin_batches_and_prints_on_a_stubbed_device(tmp_path, capsys, line, layers, neg):
    from yue_amd.recommender.advanced.LightGCN import LightGCN
    from yue_amd.tool.config import Config
    z = golden('a')
    log = tmp_path / 'log.txt'
    log.write_text(''.join('%010d,u%d,t%d,a0\n' % (t, u, i) for t, (u, i) in enumerate(zip(z['ev_u'], z['ev_i']))))
    conf_path = tmp_path / 'LightGCN.conf'
    text = open(os.path.join(ROOT, 'config', 'LightGCN.conf')).read()
    text = text.replace('record=./dataset/log.txt', 'record=%s' % log).replace('num.max.iter=100', 'num.max.iter=2')
    text = text.replace('batch_size=128', 'batch_size=%d' % z['batch_size']).replace('num.factors=50', 'num.factors=8')
    text = text.replace(' -byTime 0.2', '')                       # ids by first appearance in the log, as in the golden
    assert 'lightgcn.hip=-layers 3 -neg 5\n' in text
    if line:
        text = text.replace('lightgcn.hip=-layers 3 -neg 5\n', 'lightgcn.hip=%s\n' % line)
    conf_path.write_text(text)
    conf = Config(str(conf_path))
    train = [{'user': 'u%d' % u, 'track': 't%d' % i, 'artist': 'a0', 'time': str(t)} for t, (u, i) in enumerate(zip(z['ev_u'], z['ev_i']))]
    test = [dict(train[0])]
    rec = LightGCN(conf, train, test)
    rec.readConfiguration()
    assert rec.n_layers == layers and rec.negativeCount == neg and rec.batch_size == z['batch_size']
    np.random.seed(3)
    rec.initModel()
    assert rec.U.dtype == np.float32 and np.abs(rec.U).max() <= 0.01 and rec.U.shape == (z['m'], 8) and rec.V.shape == (z['n'], 8)
    stub = StubDevice()
    rec.dev = stub
    random.seed(z['sampler_seed'])
    capsys.readouterr()
    rec.buildModel()
    out = capsys.readouterr().out.splitlines()
    nb = len(z['batches'])
    # ids are handed out by first appearance, as in the golden: the first epoch's batches are the reference's (5 negatives), or
    # the contract sampler's with the overriding count
    if neg == z['negatives']:
        want = [tuple(b) for b in z['batches']]
    else:
        listened = {}
        for u, i in zip(z['ev_u'], z['ev_i']):
            listened.setdefault(u, set()).add(i)
        random.seed(z['sampler_seed'])
        want = list(nl.next_batch_pairwise(z['ev_u'], z['ev_i'], listened, z['n'], z['batch_size'], neg, random))
        assert [b[2] for b in want] != [b[2] for b in z['batches']]
    assert [(s[1], s[2], s[3]) for s in stub.steps[:nb]] == want
    assert [s[6] for s in stub.steps] == list(range(1, 2 * nb + 1)) and all(s[0] == layers and s[4] == 0.002 and s[5] == 0.001 for s in stub.steps)
    lines = [ln for ln in out if ln.startswith('training:')]
    assert lines == ['training: %d batch %d loss: %s' % (it + 1, b, float(it * nb + b + 1)) for it in range(2) for b in range(nb)]
    # the graph: both sides, weight = squared count
    g = nl.graph_from_events(z['ev_u'], z['ev_i'], z['m'], z['n'])
    for got, key in zip(stub.graph[2:], ('u_ptr', 'u_items', 'u_w', 'i_ptr', 'i_users', 'i_w')):
        assert np.array_equal(got, g[key]), key
    # one final propagation, ranked through the scoring path's factors
    assert stub.calls.count('lgcn_propagate') == 1 and stub.calls.index('lgcn_propagate') < len(stub.calls) - 2 and stub.propagated == [layers]
    assert np.array_equal(rec.P, rec.U * 2) and np.array_equal(rec.Q, rec.V * 2)


def test_menu_and_config_name_the_plugin():
    from yue_amd.main import MENU
    from yue_amd.recommender.advanced.LightGCN import LightGCN
    from yue_amd.tool.config import Config, LineConfig
    assert MENU['a8'] == 'LightGCN' and callable(LightGCN.buildModel)
    conf = Config(os.path.join(ROOT, 'config', 'LightGCN.conf'))
    assert conf['recommender'] == 'LightGCN' and int(conf['batch_size']) == 128
    opt = LineConfig(conf['lightgcn.hip'])
    assert int(opt['-layers']) == 3 and int(opt['-neg']) == 5


def test_plugin_refuses_array_native_data_and_bad_counts(tmp_path, capsys):
    from yue_amd import synth
    from yue_amd.data.arrays import ArrayRecord
    from yue_amd.recommender.advanced.LightGCN import LightGCN
    m, n, d = 40, 30, 6
    data = synth.make_arrays(m, n, d, seed=9)
    tp, ti = synth.make_test_arrays(m, n, d, 2, data['indptr'], data['indices'], seed=9)
    conf = le.config(tmp_path, 'defaults')
    rec = LightGCN(conf, ArrayRecord(m, n, data['ev_ptr'], data['ev_i'], tp, ti))
    rec.readConfiguration()
    capsys.readouterr()
    with pytest.raises(SystemExit):
        rec.initModel()
    assert 'array-native data is not supported' in capsys.readouterr().out
    for line in ('-layers 0', '-neg 0'):
        conf.config['lightgcn.hip'] = line
        with pytest.raises(SystemExit):
            LightGCN(conf, [], []).readConfiguration()
        assert 'must be at least 1' in capsys.readouterr().out


def e2e_plugin(tmp_path, name):
    """The plugin of an end-to-end problem after initModel, on the CPU (no device call so far), and the problem's seed."""
    from test_host_golden import _load
    from yue_amd.recommender.advanced.LightGCN import LightGCN
    conf = le.config(tmp_path, name)
    seed = le.PROBLEMS[name][4]
    rec = LightGCN(conf, _load(conf), [])
    rec.readConfiguration()
    np.random.seed(seed)
    rec.initModel()
    return rec, seed


@pytest.mark.parametrize('name', sorted(le.PROBLEMS))
def test_e2e_seeds_keep_the_float32_contract_inside_the_rule(tmp_path, capsys, orc, name):
    """What tests/test_gpu_lightgcn.py asks of the device, asked of the float32 contract: the oracle's lists on its F equal
    those on the fp64 F for every compared user, and at most 5 % of the test users are left out."""
    rec, seed = e2e_plugin(tmp_path, name)
    capsys.readouterr()
    F64, batches = le.contract_F(rec, rec.U, rec.V, seed, np.float64)
    F32, again = le.contract_F(rec, rec.U, rec.V, seed, np.float32)
    assert batches == again and len(batches[-1][0]) < rec.batch_size and F32.dtype == np.float32
    assert nl.graph_from_events(*le.events(rec)[:2], rec.m, rec.n)['w'].max() > 1          # repeated pairs: c * c
    N = max(rec._top_list())
    names, uids, mp, mi = le.ranked_users(rec)
    keep, dist = le.compared_users(F64, rec.m, uids, mp, mi, N, F32)
    print(name, 'test users', len(uids), 'left out', int((~keep).sum()), 'F distance %.3g abs, %.3g rel' % (dist, nl.rel(F32, F64)))
    assert len(uids) >= 50 and (~keep).sum() <= 0.05 * len(uids)
    # ... and still would be at 4 times that distance, the margin the device's other bounds grant over the float32 contract
    far = le.compared_users(F64, rec.m, uids, mp, mi, N, F64 + 4 * (F32.astype(np.float64) - F64))[0]
    print(name, 'left out at 4 x the distance', int((~far).sum()))
    assert (~far).sum() <= 0.05 * len(uids)
    want, got = le.oracle_lists(orc, F64, rec.m, uids, mp, mi, N), le.oracle_lists(orc, F32, rec.m, uids, mp, mi, N)
    assert np.array_equal(got[keep], want[keep])
