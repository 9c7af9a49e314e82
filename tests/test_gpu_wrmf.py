"""GPU: WRMF half-sweeps (yue_wrmf_*, DESIGN.md section "WRMF") against the device contract (tests/helpers/numpy_wrmf.py:
wrmf_half_sweep_contract, from identical inputs: rel_err <= 1e-6), against the reference's own WRMF (tests/golden/g10_*,
within the bounds measured for each case, tests/test_wrmf_golden.py), and through the plugin surface."""
import glob
import random

import numpy as np
import pytest

from helpers.numpy_wrmf import gram_fp32, pairs_from_events, wrmf_half_sweep_contract
from test_host_golden import _conf_text, _load
from test_wrmf_golden import CASES
from util import gj, gz, mask_rows, rel_err

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def dev():
    from yue_amd._shim import Device
    d = Device(0, raise_errors=True)
    yield d
    d.close()


def random_pairs(rng, m, n):
    """Events with repeats; user 1 / 2 / 3 with 0 / 1 / 2 pairs, item n-1 / n-2 / n-3 with 0 / 1 / 2 users, user 0 and
    item 0 long (more pairs than the lowered long-row threshold of the test)."""
    ev_u, ev_i = [], []
    for u in range(m):
        if u in (1, 2, 3):
            cnt = u - 1
        elif u == 0:
            cnt = 300
        else:
            cnt = rng.randint(4, 30)
        items = rng.choice(n - 3, cnt, replace=False) if cnt else np.zeros(0, np.int64)
        for i in items:
            for _ in range(1 + (rng.rand() < 0.3) * rng.randint(1, 4)):       # repeated events: counts > 1
                ev_u.append(u)
                ev_i.append(i)
    users0 = rng.choice(np.arange(4, m), 250, replace=False)                    # item 0: long on the item side
    ev_u += list(users0)
    ev_i += [0] * len(users0)
    ev_u += [5, 5, 6]
    ev_i += [n - 2, n - 3, n - 3]
    return np.array(ev_u, np.int32), np.array(ev_i, np.int32)


@pytest.mark.parametrize('k', [10, 20, 64, 100, 128])
@pytest.mark.parametrize('reg', [1.0, 0.01])
def test_half_sweeps_equal_the_contract(dev, k, reg):
    rng = np.random.RandomState(k * 7 + int(reg * 100))
    m, n = 400, 600
    ev_u, ev_i = random_pairs(rng, m, n)
    (up, ui, uc), (ip, iu, ic) = pairs_from_events(ev_u, ev_i, m, n)
    X0 = rng.rand(m, k).astype(np.float32)
    Y0 = rng.rand(n, k).astype(np.float32)
    dev.set_option('wrmf_long_pairs', 100)
    dev.set_factors(X0, Y0)
    dev.wrmf_set_pairs(up, ui, uc, ip, iu, ic)
    assert dev.get_option('wrmf_long_rows_user') >= 1 and dev.get_option('wrmf_long_rows_item') >= 1
    loss = dev.wrmf_half_sweep(0, 10.0, reg)
    X, Y = dev.get_factors()
    assert np.array_equal(Y, Y0)
    Xo, loss_o = wrmf_half_sweep_contract(Y0, up, ui, uc, reg, X_old=X0)
    assert rel_err(X, Xo) <= 1e-6 and abs(loss - loss_o) <= 1e-6 * loss_o
    assert np.all(X[1] == 0)                                                    # no pairs: exactly zero
    dev.wrmf_half_sweep(1, 10.0, reg)
    X2, Y = dev.get_factors()
    assert np.array_equal(X2, X)
    Yo, _ = wrmf_half_sweep_contract(X, ip, iu, ic, reg)
    assert rel_err(Y, Yo) <= 1e-6 and np.all(Y[n - 1] == 0)
    dev.set_option('wrmf_long_pairs', 2048)


def test_two_iterations_are_bit_reproducible(dev):
    rng = np.random.RandomState(3)
    m, n, k = 1500, 900, 64
    ev_u, ev_i = random_pairs(rng, m, n)
    (up, ui, uc), (ip, iu, ic) = pairs_from_events(ev_u, ev_i, m, n)
    X0 = rng.rand(m, k).astype(np.float32)
    Y0 = rng.rand(n, k).astype(np.float32)
    runs = []
    for _ in range(2):
        dev.set_factors(X0, Y0)
        dev.wrmf_set_pairs(up, ui, uc, ip, iu, ic)
        losses = []
        for _it in range(2):
            losses.append(dev.wrmf_half_sweep(0, 10.0, 1.0))
            dev.wrmf_half_sweep(1, 10.0, 1.0)
        X, Y = dev.get_factors()
        runs.append((X, Y, losses))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1]) and runs[0][2] == runs[1][2]


def _golden_log(tmp_path, tag):
    from yue_amd import synth
    meta = gj('g10_%s.json' % tag)
    m, n, d = meta['dataset'][:3]
    log = tmp_path / 'log.txt'
    synth.write_text_log(str(log), m, n, d)
    if tag.startswith('wrmf_z'):                             # as tools/make_wrmf_goldens.py: six test-only users
        with open(str(log), 'a') as f:
            for q in range(6):
                f.write('9999999999,zu%d,%s,a0\n' % (q, 'zt%d' % (q % 4) if q < 4 else 't%d' % q))
    return log


def _wrmf_conf(tmp_path, log, k, iters, reg, topn, extra=None):
    from yue_amd.tool.config import Config
    kv = {'record': str(log), 'recommender': 'WRMF', 'num.factors': str(k), 'num.max.iter': str(iters), 'item.ranking': '-topN ' + topn,
          'reg.lambda': '-u %s -i 0.1 -b 0.2 -s 0.2' % reg, 'output.setup': 'on -dir ' + str(tmp_path / 'results') + '/'}
    kv.update(extra or {})
    path = tmp_path / 'wrmf.conf'
    path.write_text(_conf_text(kv, {'bpr.hip': '-gpu 0'}))
    return Config(str(path))


@pytest.mark.parametrize('tag', sorted(CASES))
def test_goldens_through_the_plugin(tmp_path, capsys, orc, tag):
    from yue_amd.evaluation.measure import Measure
    from yue_amd.recommender.cf.WRMF import WRMF
    z, meta = gz('g10_%s.npz' % tag), gj('g10_%s.json' % tag)
    bound, lbound = CASES[tag]
    iters = int(z['iters'])
    conf = _wrmf_conf(tmp_path, _golden_log(tmp_path, tag), int(z['k']), iters, meta['reg'], meta['topN'])
    rec = WRMF(conf, _load(conf), [])
    rec.readConfiguration()
    random.seed(int(z['seed']))
    np.random.seed(int(z['seed']))
    rec.initModel()
    assert np.array_equal(rec.X, z['X0']) and np.array_equal(rec.Y, z['Y0'])
    capsys.readouterr()
    rec.buildModel()
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith('iteration:')]
    assert len(lines) == iters
    for t, (ln, ref) in enumerate(zip(lines, meta['lines'])):
        head, val = ln.split(' loss: ')
        assert head == 'iteration: %d' % (t + 1)
        ref_loss = float(ref.split(' loss: ')[1])
        assert abs(float(val) - ref_loss) <= lbound * abs(ref_loss)
    assert rel_err(rec.X, z['Xs'][-1]) <= bound and rel_err(rec.Y, z['Ys'][-1]) <= bound
    assert np.all(rec.X[z['zero_users']] == 0) and np.all(rec.Y[z['zero_items']] == 0)
    # lists and measures: the overwrite-scan oracle on the device's own X and Y
    N = max(int(x) for x in meta['topN'].split(','))
    users = list(rec.data.testSet.keys())
    uids = np.array([rec.data.getId(u, 'user') for u in users], np.int32)
    arrays = rec.data.to_arrays(rec.recType)
    mp, mi = mask_rows(arrays['indptr'], arrays['indices'], uids)
    oid, _, rc = orc.topn_scan(rec.X, rec.Y, uids, N, mp, mi)
    assert rc == 0
    ids = rec._scan(users, N)
    assert np.array_equal(ids, oid)
    rec.evalRanking()
    names = rec.data.id2name[rec.recType]
    recList = {u: [names[int(x)] for x in oid[t]] for t, u in enumerate(users)}
    top = [int(x) for x in meta['topN'].split(',')]
    assert rec.measure == Measure.rankingMeasure(rec.data.testSet, recList, top, rec.data.getSize(rec.recType))


def test_driver_entry_and_printed_lines(tmp_path, capsys):
    # Yue(conf).execute() with recommender=WRMF on the C1 log: the printed lines are the reference's within the case's bound
    from yue_amd.yue import Yue
    meta = gj('g10_wrmf_c1_k20.json')
    conf = _wrmf_conf(tmp_path, _golden_log(tmp_path, 'wrmf_c1_k20'), 20, 2, '1', '5,10')
    random.seed(20260010)
    np.random.seed(20260010)
    Yue(conf).execute()
    out = capsys.readouterr().out
    lines = [ln for ln in out.splitlines() if ln.startswith('iteration:')]
    assert len(lines) == 2
    for ln, ref in zip(lines, meta['lines']):
        a, b = float(ln.split(' loss: ')[1]), float(ref.split(' loss: ')[1])
        assert abs(a - b) <= CASES['wrmf_c1_k20'][1] * abs(b)
    assert glob.glob(str(tmp_path / 'results' / 'WRMF@*measure*.txt'))


def test_full_size_one_iteration(dev):
    # C3: 1M users x 200K items, d = 50, k = 128 (default long-row threshold: the popular items are split into chunks)
    from yue_amd import synth
    m, n, d, k = 1000000, 200000, 50, 128
    data = synth.make_arrays(m, n, d)
    P0, Q0 = synth.init_factors(m, n, k)
    X0, Y0 = P0 * 10, Q0 * 10
    ev_u = np.repeat(np.arange(m, dtype=np.int32), np.diff(data['ev_ptr']))
    (up, ui, uc), (ip, iu, ic) = pairs_from_events(ev_u, data['ev_i'], m, n)
    dev.set_option('wrmf_long_pairs', 2048)
    dev.set_factors(X0, Y0)
    dev.wrmf_set_pairs(up, ui, uc, ip, iu, ic)
    assert dev.get_option('wrmf_long_rows_item') >= 16
    Y_before = dev.get_factors()[1]
    dev.wrmf_half_sweep(0, 10.0, 1.0)
    X = dev.get_factors()[0]
    rng = np.random.RandomState(12)
    lens = np.diff(up)
    users = np.unique(np.concatenate([rng.choice(m, 1980, replace=False), np.flatnonzero(lens == 1)[:20]]))
    Xo, _ = wrmf_half_sweep_contract(Y_before, up, ui, uc, 1.0, rows=users, G=gram_fp32(Y_before))
    for t, u in enumerate(users):
        assert rel_err(X[u], Xo[t]) <= 1e-6, u
    dev.wrmf_half_sweep(1, 10.0, 1.0)
    Y = dev.get_factors()[1]
    top = np.argsort(-np.diff(ip), kind='stable')[:16]
    items = np.unique(np.concatenate([top, rng.choice(n, 1984, replace=False)]))
    Yo, _ = wrmf_half_sweep_contract(X, ip, iu, ic, 1.0, rows=items, G=gram_fp32(X))
    for t, i in enumerate(items):
        if ip[i + 1] == ip[i]:
            assert np.all(Y[i] == 0)
        else:
            assert rel_err(Y[i], Yo[t]) <= 1e-6, i


def test_refusals(dev):
    from yue_amd._shim import YueHipError
    rng = np.random.RandomState(5)
    m, n = 50, 60
    ev_u = np.repeat(np.arange(m, dtype=np.int32), 3)
    ev_i = rng.randint(0, n, len(ev_u)).astype(np.int32)
    (up, ui, uc), (ip, iu, ic) = pairs_from_events(ev_u, ev_i, m, n)
    dev.set_factors(rng.rand(m, 130).astype(np.float32), rng.rand(n, 130).astype(np.float32))
    dev.wrmf_set_pairs(up, ui, uc, ip, iu, ic)
    with pytest.raises(YueHipError, match='k = 130'):
        dev.wrmf_half_sweep(0, 10.0, 1.0)
    # reg = 0 with a rank-deficient Gram: column 5 of Y is zero, so row and column 5 of every A are exactly zero
    Y = rng.rand(n, 16).astype(np.float32)
    Y[:, 5] = 0
    dev.set_factors(rng.rand(m, 16).astype(np.float32), Y)
    dev.wrmf_set_pairs(up, ui, uc, ip, iu, ic)
    with pytest.raises(YueHipError, match='non-positive pivot.*user row 0'):
        dev.wrmf_half_sweep(0, 10.0, 0.0)
    dev.wrmf_half_sweep(0, 10.0, 1.0)                       # the context stays usable


def test_csr_data_set_through_the_driver(tmp_path, capsys):
    from yue_amd import synth
    from yue_amd.yue import Yue
    m, n, d = 3000, 2000, 20
    path = str(tmp_path / 'w.npz')
    synth.write_csr(path, m, n, d, d_test=5, seed=20260001)
    conf = _wrmf_conf(tmp_path, path, 32, 2, '1', '10,20', {'record.setup': '-format csr', 'evaluation.setup': '-target track'})
    np.random.seed(9)
    Yue(conf).execute()
    out = capsys.readouterr().out
    losses = [float(ln.split(' loss: ')[1]) for ln in out.splitlines() if ln.startswith('iteration:')]
    assert len(losses) == 2 and losses[1] < losses[0]
    measure = open(glob.glob(str(tmp_path / 'results' / '*measure*.txt'))[0]).read()
    assert 0.0 < float(measure.split('Precision:')[1].split()[0]) < 1.0
    lists = np.load(glob.glob(str(tmp_path / 'results' / '*items*.npz'))[0])
    assert lists['ids'].shape[1] == 20 and (lists['ids'] >= 0).all() and (lists['ids'] < n).all()


def test_saved_model_round_trip(tmp_path, capsys):
    from yue_amd.recommender.cf.WRMF import WRMF
    conf = _wrmf_conf(tmp_path, _golden_log(tmp_path, 'wrmf_c1_k20'), 20, 1, '1', '5,10')
    rec = WRMF(conf, _load(conf), [])
    rec.readConfiguration()
    np.random.seed(1)
    rec.initModel()
    rec.buildModel()
    rec.evalRanking()
    first = list(rec.measure)
    rec.saveModel()
    again = WRMF(conf, _load(conf), [])
    again.isLoadModel = True
    assert again.execute() == first
    assert again.X.dtype == np.float32 and np.array_equal(again.X, rec.X) and np.array_equal(again.Y, rec.Y)


def test_pair_lists_are_checked_against_their_own_bounds():
    # m = 5 users, n = 3 items: a bound or a row count swapped at a call site of the shared check shows
    from helpers import row_list_cases as rl
    from yue_amd._shim import Device, YueHipError
    d = Device(0, raise_errors=True)
    try:
        d.set_factors(np.zeros((rl.M, 8), np.float32), np.zeros((rl.N, 8), np.float32))
        ones = np.ones(rl.NNZ, np.int32)

        def upload(u_ptr, u_items, i_ptr, i_users, i_counts=ones):
            d.wrmf_set_pairs(u_ptr, u_items, ones, i_ptr, i_users, i_counts)
        rl.check_wiring('yue_wrmf_set_pairs', upload, rl.lists(), [('u_ptr', 'u_items', rl.N, True), ('i_ptr', 'i_users', rl.M, True)])
        twos = ones.copy(); twos[4] = 2
        for change in ({'i_users': rl.not_the_transpose()}, {'i_counts': twos}):     # another pair; the same pairs, another count
            with pytest.raises(YueHipError, match='yue_wrmf_set_pairs: .*not the transpose'):
                upload(**dict(rl.lists(), **change))
            upload(**rl.lists())
        zero = ones.copy(); zero[rl.NNZ - 1] = 0
        with pytest.raises(YueHipError, match='yue_wrmf_set_pairs: item-major row 2: counts must be >= 1'):
            upload(**dict(rl.lists(), i_counts=zero))
        upload(**rl.lists())
    finally:
        d.close()
