"""CPU: the NGCF contract (tests/helpers/numpy_ngcf.py) against the goldens recorded from the reference's own
class (tools/make_ngcf_goldens.py: index / value lists of both blocks, batches), its hand-derived backward pass against central
differences in fp64, the dropout mask's properties, the conditions every GPU case's seed was chosen for, the plugin on a
stubbed device and its refusals, and the end-to-end seeds on the float32 contract."""
import json
import os
import random

import numpy as np
import pytest

from helpers import ngcf_cases as nc
from helpers import ngcf_e2e as ne
from helpers import numpy_cune_net as ncn
from helpers import numpy_lightgcn as nl
from helpers import numpy_ngcf as ng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def golden(tag):
    return json.load(open(os.path.join(ROOT, 'tests', 'golden', 'g18_ngcf_%s.json' % tag)))


@pytest.mark.parametrize('tag', ['a', 'b'])
def test_contract_reproduces_the_references_lists_and_batches(tag):
    z = golden(tag)
    m, n, E = z['m'], z['n'], len(z['ev_u'])
    g = ng.graph_from_events(z['ev_u'], z['ev_t'], m, n, 'written')
    assert g['indices'] == z['indices'] and g['values'] == z['values'] and z['dense_shape'] == [m + n, m + n]
    # both blocks as written: (u, m + t), then (m + u, t) -- not the transpose
    assert z['indices'][:E] == [[u, m + t] for u, t in zip(z['ev_u'], z['ev_t'])]
    assert z['indices'][E:] == [[m + u, t] for u, t in zip(z['ev_u'], z['ev_t'])]
    # a pair with c events holds c + 1
    c = {}
    for u, t in zip(z['ev_u'], z['ev_t']):
        c[(u, t)] = c.get((u, t), 0) + 1
    du, dt = np.bincount(z['ev_u']), np.bincount(z['ev_t'])
    assert max(c.values()) >= 2
    assert np.allclose(z['values'][:E], [(c[(u, t)] + 1) / np.sqrt(du[u] * dt[t]) for u, t in zip(z['ev_u'], z['ev_t'])], rtol=1e-14)
    assert z['values'][E:] == z['values'][:E]
    random.seed(z['sampler_seed'])
    batches = [list(b) for b in ng.next_batch(z['ev_u'], z['ev_t'], z['track_keys'], z['batch_size'], random)]
    assert batches == z['batches'] and len(batches[-1][0]) < z['batch_size']
    # negatives are never rejected: some are tracks the user listened to
    mine = {}
    for u, t in zip(z['ev_u'], z['ev_t']):
        mine.setdefault(u, set()).add(t)
    assert sum(j in mine[u] for b in z['batches'] for u, j in zip(b[0], b[2])) > 0
    rows = sorted({r for r, _ in z['indices'] if r >= m + n})
    assert rows == z['out_of_range_rows'] == g['out_of_range']
    if tag == 'a':
        assert m <= n and not rows and max(z['ev_u']) >= min(z['ev_t'])
        # the matmul sums a pair's c entries: c (c + 1) / sqrt(d_u) / sqrt(d_t), rounded once; the written graph is not symmetric
        pairs = sorted(c)
        w = np.array([c[p] * ((c[p] + 1) / np.sqrt(du[p[0]]) / np.sqrt(dt[p[1]])) for p in pairs], np.float32)
        dense = np.zeros((m + n, m + n))
        for (r, col), v in zip(z['indices'], z['values']):
            dense[r, col] += v
        got = np.zeros((m + n, m + n), np.float32)
        for r in range(m + n):
            got[r, g['col'][g['ptr'][r]:g['ptr'][r + 1]]] = g['w'][g['ptr'][r]:g['ptr'][r + 1]]
        assert np.allclose(got, dense, rtol=1e-6) and not np.array_equal(got, got.T) and len(g['w']) == 2 * len(w)
        gt = np.zeros_like(got)
        for r in range(m + n):
            gt[r, g['T']['col'][g['T']['ptr'][r]:g['T']['ptr'][r + 1]]] = g['T']['w'][g['T']['ptr'][r]:g['T']['ptr'][r + 1]]
        assert np.array_equal(gt, got.T)
        sym = ng.graph_from_events(z['ev_u'], z['ev_t'], m, n, 'symmetric')
        assert sym['indices'][E:] == [[m + t, u] for u, t in zip(z['ev_u'], z['ev_t'])] and sym['values'] == z['values']
    else:
        assert max(z['ev_u']) >= n and rows and rows[-1] == m + max(z['ev_u']) and 'ptr' not in g
        assert 'ptr' in ng.graph_from_events(z['ev_u'], z['ev_t'], m, n, 'symmetric')


def _small(seed, form, keep, training=True, k=5, L=2):
    rs = np.random.RandomState(seed)
    m, n = 7, 9
    pu, pt, w = nl.synthetic_pairs(rs, m, n, [0, 3, 1, 4, 2, 5, 2], (0.2, 0.5, 1.1))
    g = ng.graph_from_pairs(pu, pt, w, m, n, form)
    U, V, W = rs.normal(0, 0.5, (m, k)), rs.normal(0, 0.5, (n, k)), ng.xavier(rs, L, k).astype(np.float64)
    u, i, j = rs.randint(0, m, 12), rs.randint(0, n, 12), rs.randint(0, n, 12)
    return g, U, V, W, u, i, j, (training, keep, 99 + seed, 4)


@pytest.mark.parametrize('form,keep,training', [('written', 0.9, True), ('symmetric', 0.6, True), ('written', 1.0, True), ('written', 0.9, False)])
def test_backward_matches_central_differences_in_fp64(form, keep, training):
    g, U, V, W, u, i, j, (_, _, seed, step) = _small(5, form, keep, training)
    args = (training, keep, seed, step)
    loss, gU, gV, gW, fw = ng.loss_and_grad(g, U, V, W, u, i, j, 0.01, *args)
    clamped = np.zeros(U.shape[0] + V.shape[0], bool)
    for ss in fw['ss']:
        clamped |= ss < ng.EPS
    zmin = min(np.abs(z).min() for z in fw['Z'])
    h = 2e-5
    assert zmin > 20 * h                                           # no leaky-ReLU kink within reach of the differences
    rs = np.random.RandomState(1)
    worst = 0.0

    def central(X, idx, step):
        old = X[idx]
        X[idx] = old + step
        lp = ng.loss_and_grad(g, U, V, W, u, i, j, 0.01, *args)[0]
        X[idx] = old - step
        lm = ng.loss_and_grad(g, U, V, W, u, i, j, 0.01, *args)[0]
        X[idx] = old
        return (lp - lm) / (2 * step)
    for name, X, gX in (('U', U, gU), ('V', V, gV), ('W', W, gW)):
        for _ in range(25):
            idx = tuple(rs.randint(0, s) for s in X.shape)
            fd = (4 * central(X, idx, h / 2) - central(X, idx, h)) / 3      # Richardson: the h^2 term of l2_normalize's curvature cancels
            worst = max(worst, abs(fd - gX[idx]) / max(1e-3, abs(fd)))
    print(form, keep, training, 'worst relative difference %.3g' % worst, 'clamped rows', int(clamped.sum()))
    # the differences' own rounding: the loss (about 8) is known to some 10 ulps of 2^-52, divided by h and by the 1e-3 floor of the
    # denominators: 8 * 10 * 2.2e-16 / 2e-5 / 1e-3 = 9e-7
    assert worst <= 1e-6


def test_backward_through_a_fully_dropped_row_is_the_clamp_branch():
    """k = 1 at keep 0.5: rows whose one element is dropped have ss = 0; l2_normalize's derivative there is 1e6, and the mask
    stops it.  Kept apart from the differences above: on such a row the loss has a kink of its own at 0."""
    g, U, V, W, u, i, j, args = _small(8, 'written', 0.5, True, k=1, L=2)
    loss, gU, gV, gW, fw = ng.loss_and_grad(g, U, V, W, u, i, j, 0.01, *args)
    dropped = [ss < ng.EPS for ss in fw['ss']]
    assert any(d.any() for d in dropped) and np.isfinite(gU).all() and np.isfinite(gW).all()
    for l, d in enumerate(dropped):
        assert not fw['kept'][l][d].any() and (fw['D'][l][d] == 0).all() and (fw['blocks'][l + 1][d] == 0).all()


def test_mask_is_a_pure_function_and_keeps_the_asked_share():
    a, b = ng.mask_bits(7, 3, 1, 50, 9), ng.mask_bits(7, 3, 1, 50, 9)
    assert np.array_equal(a, b) and a.min() >= 0 and a.max() < 1 << 24
    # element by element the counter hash of the user-network stage, scalar form
    for row, col in ((0, 0), (13, 8), (49, 3)):
        assert int(a[row, col]) == ncn.cnet_hash(7 ^ ng.TAG, 3, 1, row, col) >> 40
    for other in (ng.mask_bits(8, 3, 1, 50, 9), ng.mask_bits(7, 4, 1, 50, 9), ng.mask_bits(7, 3, 2, 50, 9)):
        assert not np.array_equal(a, other)
    assert np.array_equal(ng.mask_bits(7, 3, 1, 60, 12)[:50, :9], a)          # an element does not depend on the layer's shape
    assert ng.mask(7, 3, 1, 50, 9, 1.0).all()
    for keep in (0.9, 0.5):
        kept = ng.mask(11, 1, 0, 2000, 128, keep)
        share, sd = kept.mean(), np.sqrt(keep * (1 - keep) / kept.size)
        print('keep', keep, 'kept share %.5f' % share, 'in standard deviations %.2f' % ((share - keep) / sd))
        assert abs(share - keep) <= 4 * sd


@pytest.mark.parametrize('name', nc.GPU_CASES)
def test_every_gpu_case_reaches_its_branch_and_keeps_the_leaky_relu_condition(name):
    c = nc.build(name)
    print(name, 'min |Z| %.3g' % c['zmin'], 'max |Z32 - Z64| %.3g' % c['zerr'], ' '.join('%s %.3g' % kv for kv in sorted(c['d32'].items())))
    assert c['zsign'] and c['zmin'] >= 16 * c['zerr'] and nc.seed_ok(c)
    g, N = c['g'], c['m'] + c['n']
    assert len(g['ptr']) == N + 1 and (np.diff(g['col'])[np.diff(np.repeat(np.arange(N), g['degree'])) == 0] > 0).all()
    if c['edges']:
        for deg in (g['degree'], g['T']['degree']):
            assert set(nc.EDGE_DEGREES) <= set(deg.tolist())
        if c['form'] == 'written':
            assert not np.array_equal(np.sort(g['degree']), np.sort(g['T']['degree']))       # other degree profiles on A and its transpose
    if c['name'] == 'chunk':
        assert N == nc.WCHUNK + 1
    if c['k'] <= 2:
        assert sum(int((s < ng.EPS).sum()) for s in c['fw']['ss']) > 0
    if c['training'] and c['keep'] < 1:
        assert all(0 < kept.mean() < 1 for kept in c['fw']['kept'])
    if c['batch'] == 'posneg':
        assert set(c['i'].tolist()) & set(c['j'].tolist())


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

    def ngcf_set_graph(self, m, n, ptr, col, w):
        self.graph = (m, n, np.asarray(ptr), np.asarray(col), np.asarray(w))
        self.calls.append('ngcf_set_graph')

    def ngcf_set_weights(self, W):
        self.W = W.copy()
        self.calls.append('ngcf_set_weights')

    def ngcf_get_weights(self):
        return self.W

    def adam_reset(self):
        self.calls.append('adam_reset')

    def ngcf_step(self, layers, training, keep, seed, u, i, j, lr, reg, step):
        self.steps.append((layers, training, keep, seed, list(u), list(i), list(j), lr, reg, step))
        return float(step)

    def get_factors(self):
        return self.P, self.Q

    def ngcf_propagate(self, layers):
        self.calls.append('ngcf_propagate')
        self.propagated = getattr(self, 'propagated', []) + [layers]
        return np.concatenate([self.P, self.Q]) * 2


def _plugin(tmp_path, tag, line):
    from yue_amd.recommender.advanced.NGCF import NGCF
    from yue_amd.tool.config import Config
    z = golden(tag)
    log = tmp_path / 'log.txt'
    log.write_text(''.join('%010d,u%d,t%d,a0\n' % (t, u, i) for t, (u, i) in enumerate(zip(z['ev_u'], z['ev_t']))))
    text = open(os.path.join(ROOT, 'config', 'NGCF.conf')).read()
    text = text.replace('record=./dataset/log.txt', 'record=%s' % log).replace('num.max.iter=100', 'num.max.iter=2')
    text = text.replace('batch_size=16', 'batch_size=%d' % z['batch_size']).replace('num.factors=64', 'num.factors=8')
    text = text.replace(' -byTime 0.2', '')                       # ids by first appearance in the log, as in the golden
    assert 'ngcf.hip=-layers 3 -keep 0.9 -graph written\n' in text
    if line:
        text = text.replace('ngcf.hip=-layers 3 -keep 0.9 -graph written\n', 'ngcf.hip=%s\n' % line)
    path = tmp_path / 'NGCF.conf'
    path.write_text(text)
    train = [{'user': 'u%d' % u, 'track': 't%d' % i, 'artist': 'a0', 'time': str(t)} for t, (u, i) in enumerate(zip(z['ev_u'], z['ev_t']))]
    return z, NGCF(Config(str(path)), train, [dict(train[0])])


@pytest.mark.parametrize('line,layers,keep,form', [(None, 3, 0.9, 'written'), ('-layers 2 -keep 0.5 -graph symmetric -seed 9', 2, 0.5, 'symmetric')])
def test_plugin_batches_and_prints_on_a_stubbed_device(tmp_path, capsys, line, layers, keep, form):
    z, rec = _plugin(tmp_path, 'a', line)
    rec.readConfiguration()
    assert (rec.n_layers, rec.keep_prob, rec.graph_form, rec.batch_size, rec.mask_seed) == (layers, keep, form, z['batch_size'], 9 if line else 2)
    np.random.seed(3)
    rec.initModel()
    assert rec.U.dtype == np.float32 and np.abs(rec.U).max() <= 0.01 and rec.U.shape == (z['m'], 8) and rec.V.shape == (z['n'], 8)
    # the weights: Xavier uniform, drawn after U and V in the order W_0_1, W_0_2, W_1_1, ...: a plugin with one layer fewer
    # draws the same U and V and the same first weights
    lim = np.sqrt(6.0 / 16)
    assert rec.W.dtype == np.float32 and rec.W.shape == (layers, 2, 8, 8) and lim / 2 < np.abs(rec.W).max() <= lim
    other = _plugin(tmp_path, 'a', '-layers %d -graph %s' % (layers - 1, form))[1]
    other.readConfiguration()
    np.random.seed(3)
    other.initModel()
    assert np.array_equal(other.U, rec.U) and np.array_equal(other.V, rec.V) and np.array_equal(other.W, rec.W[:layers - 1])
    stub = StubDevice()
    rec.dev = stub
    random.seed(z['sampler_seed'])
    capsys.readouterr()
    rec.buildModel()
    out = capsys.readouterr().out.splitlines()
    nb = len(z['batches'])
    assert [(s[4], s[5], s[6]) for s in stub.steps[:nb]] == [tuple(b) for b in z['batches']]         # the reference's own batches
    assert [s[9] for s in stub.steps] == list(range(1, 2 * nb + 1))
    assert all(s[:4] == (layers, True, keep, 9 if line else 2) and s[7] == 0.003 and s[8] == 0.001 for s in stub.steps)
    lines = [ln for ln in out if ln.startswith('training:')]
    assert lines == ['training: %d batch %d loss: %s' % (it + 1, b, float(it * nb + b + 1)) for it in range(2) for b in range(nb)]
    g = ng.graph_from_events(z['ev_u'], z['ev_t'], z['m'], z['n'], form)
    assert stub.graph[:2] == (z['m'], z['n'])
    for got, key in zip(stub.graph[2:], ('ptr', 'col', 'w')):
        assert np.array_equal(got, g[key]), key
    assert stub.calls.index('ngcf_set_weights') < stub.calls.index('adam_reset')
    assert stub.calls.count('ngcf_propagate') == 1 and stub.propagated == [layers]
    assert np.array_equal(rec.P, rec.U * 2) and np.array_equal(rec.Q, rec.V * 2)


def test_plugin_refuses_the_written_graph_of_a_log_with_a_user_id_beyond_the_tracks(tmp_path, capsys):
    z, rec = _plugin(tmp_path, 'b', None)
    rec.readConfiguration()
    capsys.readouterr()
    with pytest.raises(SystemExit):
        rec.initModel()
    out = capsys.readouterr().out
    assert 'TensorFlow refuses such an index with a bounds error' in out and '-graph symmetric' in out and 'row m + %d' % max(z['ev_u']) in out
    z, rec = _plugin(tmp_path, 'b', '-graph symmetric')
    rec.readConfiguration()
    rec.initModel()
    assert np.array_equal(rec._graph_csr[0], ng.graph_from_events(z['ev_u'], z['ev_t'], z['m'], z['n'], 'symmetric')['ptr'])


def test_menu_config_and_the_refusals_of_read_configuration(tmp_path, capsys):
    from yue_amd.main import MENU
    from yue_amd.recommender.advanced.NGCF import NGCF
    from yue_amd.tool.config import Config, LineConfig
    assert MENU['a9'] == 'NGCF' and callable(NGCF.buildModel)
    conf = Config(os.path.join(ROOT, 'config', 'NGCF.conf'))
    assert conf['recommender'] == 'NGCF' and int(conf['batch_size']) == 16 and int(conf['num.factors']) == 64
    opt = LineConfig(conf['ngcf.hip'])
    assert int(opt['-layers']) == 3 and float(opt['-keep']) == 0.9 and opt['-graph'] == 'written'
    NGCF(conf, [], []).readConfiguration()                         # 4 * 64 = 256: the widest that fits
    conf.config['num.factors'] = '65'
    with pytest.raises(SystemExit):
        NGCF(conf, [], []).readConfiguration()
    assert 'the ranking scan takes factors of width 256 at the most' in capsys.readouterr().out
    conf.config['num.factors'] = '64'
    for line, said in (('-layers 4', 'width 256'), ('-layers 0', 'at least 1'), ('-keep 0', '-keep in (0, 1]'), ('-keep 1.5', '-keep in (0, 1]'),
                       ('-graph transposed', 'written or symmetric')):
        conf.config['ngcf.hip'] = line
        with pytest.raises(SystemExit):
            NGCF(conf, [], []).readConfiguration()
        assert said in capsys.readouterr().out, line


def test_plugin_refuses_array_native_data(tmp_path, capsys):
    from yue_amd import synth
    from yue_amd.data.arrays import ArrayRecord
    from yue_amd.recommender.advanced.NGCF import NGCF
    m, n, d = 40, 30, 6
    data = synth.make_arrays(m, n, d, seed=9)
    tp, ti = synth.make_test_arrays(m, n, d, 2, data['indptr'], data['indices'], seed=9)
    rec = NGCF(ne.config(tmp_path, 'written'), ArrayRecord(m, n, data['ev_ptr'], data['ev_i'], tp, ti))
    rec.readConfiguration()
    capsys.readouterr()
    with pytest.raises(SystemExit):
        rec.initModel()
    assert 'array-native data is not supported' in capsys.readouterr().out


@pytest.mark.parametrize('name', sorted(ne.PROBLEMS))
def test_e2e_seeds_keep_the_float32_contract_inside_the_rule(tmp_path, capsys, orc, name):
    """What tests/test_gpu_ngcf_plugin.py asks of the device, asked of the float32 contract: the oracle's lists on its F equal those
    on the fp64 F for every compared user, and at most 5 % of the test users are left out.  The problems train for 1 and 3 steps:
    tests/helpers/ngcf_e2e.py says why, tools/ngcf_e2e_drift.py shows where the rule stops holding."""
    rec, seed = ne.plugin_on_cpu(tmp_path, name)
    capsys.readouterr()
    assert (rec.m <= rec.n) == (rec.graph_form == 'written') and (rec.n_layers + 1) * rec.k <= 256
    F64, batches = ne.contract_F(rec, rec.U, rec.V, rec.W, seed, np.float64)
    F32, again = ne.contract_F(rec, rec.U, rec.V, rec.W, seed, np.float32)
    assert batches == again and len(batches[-1][0]) < rec.batch_size and F32.dtype == np.float32 and F32.shape[1] == (rec.n_layers + 1) * rec.k
    assert len(batches) == (1 if rec.graph_form == 'written' else 3)
    # the plugin's graph is the contract's, repeated pairs included
    ev_u, ev_t, du, dt, keys = ne.events(rec)
    g = ng.graph_from_events(ev_u, ev_t, rec.m, rec.n, rec.graph_form, du, dt)
    for got, key in zip(rec._graph_csr, ('ptr', 'col', 'w')):
        assert np.array_equal(got, g[key]), key
    assert len(set(zip(ev_u, ev_t))) < len(ev_u)
    N = max(rec._top_list())
    names, uids, mp, mi = ne.ranked_users(rec)
    keep, dist = ne.compared_users(F64, rec.m, uids, mp, mi, N, F32)
    print(name, 'test users', len(uids), 'left out', int((~keep).sum()), 'F distance %.3g abs, %.3g rel' % (dist, ng.rel(F32, F64)))
    assert len(uids) >= 50 and (~keep).sum() <= 0.05 * len(uids)
    # ... and still would be at 4 times that distance, the margin the device's other bounds grant over the float32 contract
    far = ne.compared_users(F64, rec.m, uids, mp, mi, N, F64 + 4 * (F32.astype(np.float64) - F64))[0]
    print(name, 'left out at 4 x the distance', int((~far).sum()))
    assert (~far).sum() <= 0.05 * len(uids)
    want, got = ne.oracle_lists(orc, F64, rec.m, uids, mp, mi, N), ne.oracle_lists(orc, F32, rec.m, uids, mp, mi, N)
    assert np.array_equal(got[keep], want[keep])


def test_the_chunk_case_crosses_the_kernels_own_chunk():
    """ngcf_cases.WCHUNK is the kernel header's kNgcfWChunk: the 'chunk' case has one row more."""
    import re
    text = open(os.path.join(ROOT, 'yue_amd', 'csrc', 'ngcf_kernels.hpp')).read()
    found = re.findall(r'constexpr int kNgcfWChunk = (\d+);', text)
    assert found == [str(nc.WCHUNK)]
    c = nc.BY_NAME['chunk']
    assert c['m'] + c['n'] == int(found[0]) + 1
