"""CPU: the NumPy contract of CoFactor (tests/helpers/numpy_cofactor.py) against what the reference's own CoFactor class computed
(tests/golden/g14_cofactor_*, tools/make_cofactor_goldens.py).

The co-occurrence and SPPMI graphs are integers and Python doubles: they equal the reference bit for bit.  The sweep cannot: the
reference inverts with np.linalg.inv where the contract factorises, its X^T X is an fp32 BLAS product, and it visits the
contexts in dictionary order.  Each case therefore carries the deviation measured when its fixture was generated (the json's
'measured'), and the contract must stay within four times that figure, the margin test_wrmf_golden.py grants the same kind
of bound.  The level-driven sweep equals the sequential one bit for bit: that is what lets the device run a level at once.
"""
import numpy as np
import pytest

from helpers import numpy_cofactor as nc
from helpers.numpy_wrmf import pairs_from_events
from util import gj, gz

CASES = ['c1_k20', 'd3_k128', 'd3_k64_g003', 's_k20', 'z_k64']
MARGIN = 4.0


def load(tag):
    z, st, meta = gz('g14_cofactor_%s.npz' % tag), gz('g14_cofactor_%s_states.npz' % tag), gj('g14_cofactor_%s.json' % tag)
    m, n = int(z['m']), int(z['n'])
    um, im = pairs_from_events(z['ev_u'].astype(np.int32), z['ev_i'].astype(np.int32), m, n)
    co = (z['co_ptr'].astype(np.int64), z['co_idx'].astype(np.int32), z['co_cnt'].astype(np.int32))
    sp = (z['sp_ptr'].astype(np.int64), z['sp_idx'].astype(np.int32), z['sp_val'])
    return z, st, meta, um, im, co, sp


def bounds(meta):
    return {key: MARGIN * meta['measured']['contract_vs_reference_' + key] for key in ('X', 'Y', 'G', 'w', 'c', 'loss')}


def printed_losses(meta):
    assert meta['lines'][0] == 'training...'
    out = []
    for i, ln in enumerate(meta['lines'][1:], 1):
        head, val = ln.split(' loss: ')
        assert head == 'iteration: %d' % i
        out.append(float(val))
    return out


@pytest.mark.parametrize('tag', CASES)
def test_graphs_equal_the_reference_bit_for_bit(tag):
    from yue_amd.recommender.advanced.CoFactor import sppmi_from_counts
    z, st, meta, um, im, co, sp = load(tag)
    got = nc.cooccur_from_pairs(im[0], im[1], im[2], int(z['m']), int(z['filter']))
    for a, b in zip(got, co):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    assert meta['cooccur_nnz'] == len(co[1])
    for fn in (nc.sppmi_from_cooccur, sppmi_from_counts):            # the contract's loop and the plugin's vectorised form
        got = fn(co[0], co[1], co[2], int(z['neg']))
        for a, b in zip(got, sp):
            assert a.dtype == b.dtype and np.array_equal(a, b), fn.__name__
    # symmetric, no diagonal, values in (0, 1] with the largest equal to 1
    rows = np.repeat(np.arange(int(z['n'])), np.diff(sp[0]))
    assert not (rows == sp[1]).any()
    if len(sp[2]):
        assert sp[2].max() == 1.0 and sp[2].min() > 0
        assert set(zip(rows.tolist(), sp[1].tolist())) == set(zip(sp[1].tolist(), rows.tolist()))


def test_an_empty_graph():
    # a filter no pair passes: empty co-occurrence, empty SPPMI, one level
    z, st, meta, um, im, co, sp = load('d3_k64_g003')
    e = nc.cooccur_from_pairs(im[0], im[1], im[2], int(z['m']), 10 ** 6)
    assert e[0][-1] == 0 and len(e[1]) == 0
    s = nc.sppmi_from_cooccur(e[0], e[1], e[2], 1)
    assert s[0][-1] == 0 and nc.levels_of(s[0], s[1]).max() == 0


@pytest.mark.parametrize('tag', CASES)
def test_level_schedule_equals_the_sequential_sweep_bit_for_bit(tag):
    z, st, meta, um, im, co, sp = load(tag)
    m, n, k = int(z['m']), int(z['n']), int(z['k'])
    regU, regR = float(z['regU']), float(z['regR'])
    level = nc.levels_of(sp[0], sp[1])
    assert int(level.max()) + 1 == meta['levels']
    rows = np.repeat(np.arange(n), np.diff(sp[0]))
    assert not (level[rows] == level[sp[1]]).any()                    # no context edge inside a level
    lower = sp[1] < rows
    assert (level[sp[1]][lower] < level[rows][lower]).all()           # the earlier contexts sit in earlier levels
    X, Y, G, w, c = nc.init_from_seed(int(z['seed']), m, n, k)
    orders = [None, nc.level_order(sp[0], sp[1], im[0]), nc.level_order(sp[0], sp[1], im[0], np.random.RandomState(5))]
    states = [(X, Y, G, w, c)] * 3
    for _ in range(2):
        states = [nc.iteration(*s, um, im, sp, regU, regR, order=o)[:5] for s, o in zip(states, orders)]
        for other in states[1:]:
            for a, b in zip(states[0], other):
                assert np.array_equal(a, b)


@pytest.mark.parametrize('tag', CASES)
def test_contract_within_the_measured_bound(tag):
    z, st, meta, um, im, co, sp = load(tag)
    m, n, k = int(z['m']), int(z['n']), int(z['k'])
    b = bounds(meta)
    X, Y, G, w, c = nc.init_from_seed(int(z['seed']), m, n, k)
    for t, ref_loss in enumerate(printed_losses(meta)):
        X, Y, G, w, c, loss = nc.iteration(X, Y, G, w, c, um, im, sp, float(z['regU']), float(z['regR']))
        got = {'X': nc.rel(X, st['Xs'][t]), 'Y': nc.rel(Y, st['Ys'][t]), 'G': nc.rel(G, st['Gs'][t]), 'w': nc.rel(w, st['ws'][t]),
               'c': nc.rel(c, st['cs'][t]), 'loss': abs(loss - ref_loss) / abs(ref_loss)}
        print(tag, t, got)
        for key in got:
            assert got[key] <= b[key], (key, got[key], b[key])
    assert Y.dtype == np.float32 and G.dtype == np.float64
    # rows without training pairs: exactly zero in the reference and in the contract
    assert np.all(st['Xs'][-1][z['zero_users']] == 0) and np.all(X[z['zero_users']] == 0)
    assert np.all(st['Ys'][-1][z['zero_items']] == 0) and np.all(Y[z['zero_items']] == 0)
    assert z['stable_users'].sum() >= 0.9 * len(z['test_users'])


def test_zero_row_case_has_zero_rows():
    z = gz('g14_cofactor_z_k64.npz')
    assert len(z['zero_users']) == 6 and len(z['zero_items']) >= 4 and int(z['filter']) == 0


def test_plugin_surface():
    import os
    from yue_amd import _shim
    from yue_amd.main import MENU
    from yue_amd.recommender.advanced.CoFactor import CoFactor
    from yue_amd.tool.config import Config, LineConfig
    assert MENU['a7'] == 'CoFactor' and callable(CoFactor.buildModel) and callable(CoFactor.saveModel)
    for name in ('yue_cof_cooccur', 'yue_cof_get_cooccur', 'yue_cof_set_sppmi', 'yue_cof_set_state', 'yue_cof_get_state', 'yue_cof_item_sweep'):
        assert name in _shim.SYMBOLS
    conf = Config(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'config', 'CoFactor.conf'))
    assert conf['recommender'] == 'CoFactor'
    opt = LineConfig(conf['CoFactor'])
    assert int(opt['-k']) == 5 and float(opt['-gamma']) == 0.03 and int(opt['-filter']) >= 0
    assert LineConfig(conf['evaluation.setup'])['-target'] == 'track'
