"""GPU: CoFactor (yue_cof_*) against the CPU contract (tests/helpers/numpy_cofactor.py), against the
reference's own CoFactor (tests/golden/g14_cofactor_*) and through the plugin surface.

Bounds.  The co-occurrence and SPPMI graphs: bit for bit.  Y against the contract from identical inputs: 1e-6 of the largest
entry, what test_gpu_wrmf.py grants the same solve.  G, w, c (fp64 on both sides) against the contract from identical inputs:
CONTRACT_FP64, the largest figure measured on the goldens (G 8.6e-14, w 2.6e-15, c 1.4e-14: fp64 round-off of sums taken in
another association, amplified by the conditioning of the k x k systems) times 4 -- narrow enough that state held or solved in
fp32 (6e-8) cannot pass.  Everything against the reference: the case's contract-vs-reference figure (the json's 'measured')
times 4, and never less than 1e-6.
"""
import glob
import random

import numpy as np
import pytest

from helpers import numpy_cofactor as nc
from helpers.numpy_wrmf import pairs_from_events
from test_cofactor_golden import CASES, MARGIN, load, printed_losses
from test_host_golden import _conf_text, _load

pytestmark = pytest.mark.gpu

ALPHA = 10.0
CONTRACT_FP64 = {'G': 4 * 8.6e-14, 'w': 4 * 2.6e-15, 'c': 4 * 1.4e-14}


@pytest.fixture(scope='module')
def dev():
    from yue_amd._shim import Device
    d = Device(0, raise_errors=True)
    yield d
    d.close()


def bound(meta, key):
    return max(MARGIN * meta['measured']['contract_vs_reference_' + key], 1e-6)


def upload(dev, X, Y, G, w, c, um, im, sp):
    dev.set_factors(X, Y)
    dev.wrmf_set_pairs(*(um + im))
    dev.cof_set_sppmi(*sp)
    dev.cof_set_state(G, w, c)


@pytest.mark.parametrize('tag', CASES)
def test_cooccurrence_and_sppmi_bit_for_bit(dev, tag):
    from yue_amd.recommender.advanced.CoFactor import sppmi_from_counts
    z, st, meta, um, im, co, sp = load(tag)
    m, n, k = int(z['m']), int(z['n']), int(z['k'])
    dev.set_factors(np.zeros((m, k), np.float32), np.zeros((n, k), np.float32))
    dev.wrmf_set_pairs(*(um + im))
    for pass_items in (8192, 64):
        dev.set_option('cof_pass_items', pass_items)
        got = dev.cof_cooccur(int(z['filter']))
        for a, b in zip(got, co):
            assert a.dtype == b.dtype and np.array_equal(a, b), pass_items
        assert dev.get_option('cof_cooccur_nnz') == len(co[1])
    dev.set_option('cof_pass_items', 8192)
    for a, b in zip(sppmi_from_counts(got[0], got[1], got[2], int(z['neg'])), sp):
        assert a.dtype == b.dtype and np.array_equal(a, b)


@pytest.mark.parametrize('tag', CASES)
def test_item_sweep_and_two_iterations_equal_the_contract(dev, tag):
    z, st, meta, um, im, co, sp = load(tag)
    m, n, k = int(z['m']), int(z['n']), int(z['k'])
    regU, regR = float(z['regU']), float(z['regR'])
    X0, Y0, G0, w0, c0 = nc.init_from_seed(int(z['seed']), m, n, k)
    dev.set_option('wrmf_long_pairs', 32)                             # the popular items go through the chunk path
    upload(dev, X0, Y0, G0, w0, c0, um, im, sp)
    assert dev.get_option('cof_levels') == meta['levels']
    dev.cof_item_sweep(ALPHA, regU, regR)
    X, Y = dev.get_factors()
    G, w, c = dev.cof_get_state()
    assert np.array_equal(X, X0)
    Yo, Go, wo, co_ = Y0.copy(), G0.copy(), w0.copy(), c0.copy()
    nc.item_sweep(X0, Yo, Go, wo, co_, im[0], im[1], im[2], sp[0], sp[1], sp[2], regU, regR)
    got = {'Y': nc.rel(Y, Yo), 'G': nc.rel(G, Go), 'w': nc.rel(w, wo), 'c': nc.rel(c, co_)}
    print(tag, 'one sweep', got)
    assert got['Y'] <= 1e-6
    for key in ('G', 'w', 'c'):
        assert got[key] <= CONTRACT_FP64[key], key
    assert np.all(Y[z['zero_items']] == 0)
    lone = np.flatnonzero((np.diff(sp[0]) == 0) & (np.diff(im[0]) > 0))    # pairs but no contexts: G, w, c untouched
    assert np.array_equal(G[lone], G0[lone]) and np.array_equal(w[lone], w0[lone]) and np.array_equal(c[lone], c0[lone])
    assert len(lone) > 0 or tag in ('z_k64', 's_k20')                # (filter 0 / 64 dense items: every item with pairs has contexts)
    # two full iterations, twice: bit-identical runs, within the bounds of the contract
    runs = []
    for _ in range(2):
        upload(dev, X0, Y0, G0, w0, c0, um, im, sp)
        losses = []
        for _it in range(2):
            losses.append(dev.wrmf_half_sweep(0, ALPHA, regU))
            dev.cof_item_sweep(ALPHA, regU, regR)
        runs.append(dev.get_factors() + dev.cof_get_state() + (np.array(losses),))
    dev.set_option('wrmf_long_pairs', 2048)
    for a, b in zip(runs[0], runs[1]):
        assert np.array_equal(a, b)
    s = (X0, Y0, G0, w0, c0)
    for _it in range(2):
        s = nc.iteration(*s[:5], um, im, sp, regU, regR)
    got = {key: nc.rel(a, b) for key, a, b in zip(('X', 'Y', 'G', 'w', 'c'), runs[0][:5], s[:5])}
    print(tag, 'two iterations', got, 'loss', runs[0][5][-1], s[5])
    assert got['X'] <= 1e-6 and got['Y'] <= 1e-6
    for key in ('G', 'w', 'c'):
        assert got[key] <= CONTRACT_FP64[key], key
    assert abs(runs[0][5][-1] - s[5]) <= 1e-6 * abs(s[5])
    # ... and of the reference
    ref = {'X': st['Xs'][-1], 'Y': st['Ys'][-1], 'G': st['Gs'][-1], 'w': st['ws'][-1], 'c': st['cs'][-1]}
    for key, a in zip(('X', 'Y', 'G', 'w', 'c'), runs[0][:5]):
        print(tag, key, 'vs reference', nc.rel(a, ref[key]), bound(meta, key))
        assert nc.rel(a, ref[key]) <= bound(meta, key), key
    assert np.all(runs[0][0][z['zero_users']] == 0) and np.all(runs[0][1][z['zero_items']] == 0)


def _golden_log(tmp_path, tag):
    from yue_amd import synth
    from util import gj
    meta = gj('g14_cofactor_%s.json' % tag)
    m, n, d = meta['dataset'][:3]
    log = tmp_path / 'log.txt'
    synth.write_text_log(str(log), m, n, d)
    with open(str(log), 'a') as f:
        for ln in meta['append']:
            f.write(ln + '\n')
    return log


def _conf(tmp_path, log, z, meta, iters=None, extra=None):
    from yue_amd.tool.config import Config
    o = meta['options']
    kv = {'record': str(log), 'recommender': 'CoFactor', 'num.factors': str(int(z['k'])), 'num.max.iter': str(int(z['iters']) if iters is None else iters),
          'item.ranking': '-topN ' + meta['topN'], 'reg.lambda': '-u %s -i 0.01 -b 0.01 -s 0.1' % o['regU'],
          'CoFactor': '-k %d -gamma %s -filter %d' % (o['k'], o['gamma'], o['filter']), 'output.setup': 'on -dir ' + str(tmp_path / 'results') + '/'}
    kv.update(extra or {})
    path = tmp_path / 'cofactor.conf'
    path.write_text(_conf_text(kv, {'bpr.hip': '-gpu 0'}))
    return Config(str(path))


@pytest.mark.parametrize('tag', CASES)
def test_goldens_through_the_plugin(tmp_path, capsys, tag):
    from yue_amd.recommender.advanced.CoFactor import CoFactor
    z, st, meta, um, im, co, sp = load(tag)
    conf = _conf(tmp_path, _golden_log(tmp_path, tag), z, meta)
    rec = CoFactor(conf, _load(conf), [])
    rec.readConfiguration()
    random.seed(int(z['seed']))
    np.random.seed(int(z['seed']))
    rec.initModel()
    for a, b in zip(rec.cooccur + rec.SPPMI, co + sp):
        assert np.array_equal(a, b)
    capsys.readouterr()
    rec.buildModel()
    out = capsys.readouterr().out.splitlines()
    assert out[0] == 'training...'
    lines = [ln for ln in out if ln.startswith('iteration:')]
    ref_losses = printed_losses(meta)
    assert len(lines) == len(ref_losses)
    for t, (ln, ref) in enumerate(zip(lines, ref_losses)):
        head, val = ln.split(' loss: ')
        assert head == 'iteration: %d' % (t + 1)
        assert abs(float(val) - ref) <= bound(meta, 'loss') * abs(ref)
    ref = {'X': st['Xs'][-1], 'Y': st['Ys'][-1], 'G': st['Gs'][-1], 'w': st['ws'][-1], 'c': st['cs'][-1]}
    for key, a in zip(('X', 'Y', 'G', 'w', 'c'), (rec.X, rec.Y, rec.G, rec.w, rec.c)):
        assert nc.rel(a, ref[key]) <= bound(meta, key), key
    assert rec.G.dtype == np.float64 and rec.Y.dtype == np.float32
    assert np.all(rec.X[z['zero_users']] == 0) and np.all(rec.Y[z['zero_items']] == 0)
    N = max(int(x) for x in meta['topN'].split(','))
    users = list(rec.data.testSet.keys())
    uids = np.array([rec.data.getId(u, 'user') for u in users], np.int32)
    assert np.array_equal(uids, z['test_users'])
    ids = rec._scan(users, N)
    stable = z['stable_users']
    assert stable.sum() >= 0.9 * len(users)
    assert np.array_equal(ids[stable], z['rec_ids'][stable])
    rec.evalRanking()
    if tag == 's_k20':                                                  # the case whose every list is stable (asserted by the golden tool)
        assert stable.all()
    if stable.all():
        assert rec.measure == meta['measure']
    else:                                                               # the measures over the stable users, from the device's lists and the golden's
        from yue_amd.evaluation.measure import Measure
        names = rec.data.id2name[rec.recType]
        top = [int(x) for x in meta['topN'].split(',')]
        origin = {u: rec.data.testSet[u] for t, u in enumerate(users) if stable[t]}
        mine = {u: [names[int(x)] for x in ids[t]] for t, u in enumerate(users) if stable[t]}
        gold = {u: [names[int(x)] for x in z['rec_ids'][t]] for t, u in enumerate(users) if stable[t]}
        size = rec.data.getSize(rec.recType)
        assert Measure.rankingMeasure(origin, mine, top, size) == Measure.rankingMeasure(origin, gold, top, size)


def test_driver_entry_round_trip_and_target_refusal(tmp_path, capsys):
    from yue_amd.recommender.advanced.CoFactor import CoFactor
    from yue_amd.yue import Yue
    tag = 'd3_k64_g003'
    z, st, meta, um, im, co, sp = load(tag)
    log = _golden_log(tmp_path, tag)
    conf = _conf(tmp_path, log, z, meta)
    random.seed(int(z['seed']))
    np.random.seed(int(z['seed']))
    Yue(conf).execute()
    out = capsys.readouterr().out
    lines = [ln for ln in out.splitlines() if ln.startswith('iteration:')]
    assert 'training...' in out.splitlines() and len(lines) == 2
    for ln, ref in zip(lines, printed_losses(meta)):
        assert abs(float(ln.split(' loss: ')[1]) - ref) <= bound(meta, 'loss') * abs(ref)
    assert glob.glob(str(tmp_path / 'results' / 'CoFactor@*measure*.txt'))
    # saved model
    rec = CoFactor(conf, _load(conf), [])
    rec.readConfiguration()
    np.random.seed(1)
    rec.initModel()
    rec.buildModel()
    rec.evalRanking()
    first = list(rec.measure)
    rec.saveModel()
    again = CoFactor(conf, _load(conf), [])
    again.isLoadModel = True
    assert again.execute() == first
    for key in ('X', 'Y', 'G', 'w', 'c'):
        assert np.array_equal(getattr(again, key), getattr(rec, key))
    assert again.G.dtype == np.float64
    # -target other than track
    bad = _conf(tmp_path, log, z, meta, extra={'evaluation.setup': '-target artist -byTime 0.2'})
    other = CoFactor(bad, _load(bad), [])
    with pytest.raises(SystemExit):
        other.readConfiguration()
    assert '-target track' in capsys.readouterr().out


def test_refusals_leave_the_context_usable(dev):
    from yue_amd._shim import YueHipError
    z, st, meta, um, im, co, sp = load('d3_k64_g003')
    m, n, k = int(z['m']), int(z['n']), int(z['k'])
    X0, Y0, G0, w0, c0 = nc.init_from_seed(int(z['seed']), m, n, k)
    dev.set_factors(X0, Y0)
    dev.wrmf_set_pairs(*(um + im))
    fresh_n = n + 1                                                     # another n: no SPPMI and no state for it yet
    (up, ui, uc), (ip, iu, ic) = um, im
    dev.set_factors(X0, np.vstack([Y0, Y0[:1]]))
    dev.wrmf_set_pairs(up, ui, uc, np.append(ip, ip[-1]), iu, ic)
    with pytest.raises(YueHipError, match='yue_cof_set_sppmi first'):
        dev.cof_item_sweep(ALPHA, 1.0, 1.0)
    dev.cof_set_sppmi(np.append(sp[0], sp[0][-1]), sp[1], sp[2])
    with pytest.raises(YueHipError, match='yue_cof_set_state first'):
        dev.cof_item_sweep(ALPHA, 1.0, 1.0)
    assert fresh_n == dev.n
    dev.set_factors(X0, Y0)
    dev.wrmf_set_pairs(*(um + im))
    rows = np.repeat(np.arange(n), np.diff(sp[0]))
    i, j = int(rows[0]), int(sp[1][0])
    ptr, idx, val = sp[0].copy(), sp[1].copy(), sp[2].copy()
    val[0] *= 0.5                                                       # (i, j) != (j, i)
    with pytest.raises(YueHipError, match='not symmetric'):
        dev.cof_set_sppmi(ptr, idx, val)
    idx2 = sp[1].copy()
    r = int(np.flatnonzero(np.diff(sp[0]) >= 2)[0])
    a = int(sp[0][r])
    idx2[a], idx2[a + 1] = idx2[a + 1], idx2[a]
    with pytest.raises(YueHipError, match='yue_cof_set_sppmi: SPPMI rows must be sorted and unique .row %d.' % r):
        dev.cof_set_sppmi(sp[0], idx2, sp[2])
    dptr = np.zeros(n + 1, np.int64)
    dptr[i + 1:] = 1
    with pytest.raises(YueHipError, match='diagonal'):
        dev.cof_set_sppmi(dptr, np.array([i], np.int32), np.array([1.0]))
    assert j != i
    with pytest.raises(YueHipError, match='filter must be >= 0'):
        dev.cof_cooccur(-1)
    # the context is still usable
    upload(dev, X0, Y0, G0, w0, c0, um, im, sp)
    dev.cof_item_sweep(ALPHA, 1.0, 0.03)
    assert np.isfinite(dev.get_factors()[1]).all() and all(np.isfinite(a).all() for a in dev.cof_get_state())


def test_cooccurrence_workspace_overflow_is_refused(dev):
    from yue_amd._shim import YueHipError
    rng = np.random.RandomState(3)
    m, n, k = 3000, 1200, 8
    ev_u = np.repeat(np.arange(m, dtype=np.int32), 40)
    ev_i = rng.randint(0, n, len(ev_u)).astype(np.int32)
    um, im = pairs_from_events(ev_u, ev_i, m, n)
    dev.set_factors(np.zeros((m, k), np.float32), np.zeros((n, k), np.float32))
    dev.wrmf_set_pairs(*(um + im))
    want = nc.cooccur_from_pairs(im[0], im[1], im[2], m, 0)
    assert len(want[1]) > (1 << 20) // 8                                # more than 1 MiB of entries
    dev.set_option('cof_cooccur_mb', 1)
    with pytest.raises(YueHipError, match='cof_cooccur_mb'):
        dev.cof_cooccur(0)
    dev.set_option('cof_cooccur_mb', 1024)
    got = dev.cof_cooccur(0)
    for a, b in zip(got, want):
        assert np.array_equal(a, b)


def test_full_size_cooccurrence_and_one_iteration(dev):
    # C3: 1M users x 200K items, d = 50, k = 128.  The filter starts at 8 and doubles while the co-occurrence CSR does not fit the
    # default workspace (cof_cooccur_mb = 1024); 25 passes over item ranges, the chunk path for the popular items.
    from yue_amd import synth
    from yue_amd._shim import YueHipError
    from yue_amd.recommender.advanced.CoFactor import sppmi_from_counts
    m, n, d, k = 1000000, 200000, 50, 128
    data = synth.make_arrays(m, n, d)
    P0, Q0 = synth.init_factors(m, n, k)
    ev_u = np.repeat(np.arange(m, dtype=np.int32), np.diff(data['ev_ptr']))
    um, im = pairs_from_events(ev_u, data['ev_i'], m, n)
    dev.set_option('wrmf_long_pairs', 2048)
    dev.set_option('cof_cooccur_mb', 1024)
    dev.set_option('cof_pass_items', 8192)
    dev.set_factors(P0 * 10, Q0 * 10)
    dev.wrmf_set_pairs(*(um + im))
    filt = 8
    while True:
        try:
            co = dev.cof_cooccur(filt)
            break
        except YueHipError as err:
            assert 'cof_cooccur_mb' in str(err) and filt < 1 << 20
            filt *= 2
    nnz = len(co[1])
    print('C3 filter', filt, 'cooccur nnz', nnz, 'ms', dev.get_option('cof_last_ns') * 1e-6)
    assert nnz > 0 and co[0][-1] == nnz and dev.get_option('cof_cooccur_nnz') == nnz
    rows = np.repeat(np.arange(n, dtype=np.int64), np.diff(co[0]))
    assert (rows != co[1]).all() and (co[2] > filt).all() and co[1].min() >= 0 and co[1].max() < n
    inner = np.ones(nnz, bool)
    inner[co[0][:-1][np.diff(co[0]) > 0]] = False
    assert (np.diff(co[1])[inner[1:]] > 0).all()                        # ascending inside every row
    fwd, bwd = np.lexsort((co[1], rows)), np.lexsort((rows, co[1]))     # symmetric: the transposed entry list is the same list
    assert np.array_equal(rows[fwd], co[1][bwd]) and np.array_equal(co[1][fwd], rows[bwd]) and np.array_equal(co[2][fwd], co[2][bwd])
    # a sample of rows against set intersections of the posting lists
    rng = np.random.RandomState(4)
    ip, iu, ic = im
    events = np.add.reduceat(np.append(ic, 0).astype(np.int64), np.minimum(ip[:-1], len(ic)))
    events[np.diff(ip) == 0] = 0
    for i in np.concatenate([[0, 1, n - 1], rng.choice(n, 5, replace=False)]):
        ui_ = iu[ip[i]:ip[i + 1]]
        for e in rng.choice(np.arange(co[0][i], co[0][i + 1]), min(5, int(co[0][i + 1] - co[0][i])), replace=False):
            j = co[1][e]
            assert co[2][e] == len(np.intersect1d(ui_, iu[ip[j]:ip[j + 1]], assume_unique=True)) and events[j] >= filt and events[i] >= filt
    sp = sppmi_from_counts(co[0], co[1], co[2], 1)
    rs = np.random.RandomState(2)
    dev.cof_set_sppmi(*sp)
    dev.cof_set_state(rs.rand(n, k) / 10, rs.rand(n) / 10, rs.rand(n) / 10)
    loss = dev.wrmf_half_sweep(0, ALPHA, 1.0)
    dev.cof_item_sweep(ALPHA, 1.0, 1.0)
    print('C3 sppmi nnz', int(sp[0][-1]), 'cof_levels', dev.get_option('cof_levels'), 'item sweep ms', dev.get_option('cof_last_ns') * 1e-6)
    X, Y = dev.get_factors()
    G, w, c = dev.cof_get_state()
    assert np.isfinite(loss) and np.isfinite(X).all() and np.isfinite(Y).all() and np.isfinite(G).all() and np.isfinite(w).all() and np.isfinite(c).all()
    assert dev.get_option('cof_levels') >= 1


def test_the_sppmi_rows_are_checked_against_their_own_bound():
    # m = 5 users, n = 3 items; the SPPMI is n x n: every pair of different items, value 1
    from helpers import row_list_cases as rl
    from yue_amd._shim import Device, YueHipError
    d = Device(0, raise_errors=True)
    try:
        d.set_factors(np.zeros((rl.M, 8), np.float32), np.zeros((rl.N, 8), np.float32))
        base = {'ptr': np.array([0, 2, 4, 6], np.int64), 'idx': np.array([1, 2, 0, 2, 0, 1], np.int32)}
        ones = np.ones(6)

        def upload(ptr, idx, val=ones):
            d.cof_set_sppmi(ptr, idx, val)
        rl.check_wiring('yue_cof_set_sppmi', upload, base, [('ptr', 'idx', rl.N, True)])
        inf = ones.copy(); inf[5] = np.inf
        with pytest.raises(YueHipError, match='yue_cof_set_sppmi: SPPMI row 2: holds a value that is not finite'):
            upload(val=inf, **base)
        upload(**base)
    finally:
        d.close()
