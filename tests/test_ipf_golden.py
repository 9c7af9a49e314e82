"""CPU: the NumPy oracle of IPF (tests/helpers/numpy_ipf.py) against what the reference's own IPF class computed
(tests/golden/g12_ipf_*, tools/make_ipf_goldens.py): predict lists and scores, the lists file of evalRanking and its
measure strings -- all bit for bit.  Also the product's graph builder (recommender/cf/IPF.py: ipf_graph) against the
oracle's graph, and the plugin's configuration rules."""
import numpy as np
import pytest

from helpers import numpy_ipf as oi
from test_host_golden import _load
from util import gj, gz
from yue_amd.evaluation.measure import Measure
from yue_amd.recommender.cf.UserKNN import HEADER, list_line
from yue_amd.tool.config import Config


def case_conf(tmp_path, tag, out='results'):
    """config/IPF.conf of this repository with the case's log, options and list sizes (as the fixture was made)."""
    log = str(tmp_path / (tag + '.txt'))
    test = oi.write_case_log(tag, log)
    c = oi.CASES[tag]
    text = ('record=%s\nrecord.setup=-columns user:1,track:2,time:0 -delim ,\nevaluation.setup=%s\nrecommender=IPF\n'
            'item.ranking=-topN %s\nIPF=%s\noutput.setup=on -dir %s/\nbpr.hip=-gpu 0\n'
            % (log, c['eval'].format(test=test), c['topN'], c['ipf'], tmp_path / out))
    path = tmp_path / (tag + '.conf')
    path.write_text(text)
    return Config(str(path)), test


def load_case(tmp_path, tag):
    """(fixture arrays, Record as the plugin sees it (after -sample), oracle graph, training arrays, i2u)."""
    from yue_amd.base.recommender import Recommender
    z = gz('g12_%s.npz' % tag)
    meta = gj('g12_%s.json' % tag)
    conf, test = case_conf(tmp_path, tag)
    rec = Recommender(conf, _load(conf), _load_test(conf, test)).data
    arrays = rec.to_arrays('track')
    m, n = rec.getSize('user'), rec.getSize('track')
    ev_u = np.repeat(np.arange(m, dtype=np.int32), np.diff(arrays['ev_ptr']))
    assert m == int(z['m']) and n == int(z['n'])
    assert np.array_equal(ev_u, z['ev_u']) and np.array_equal(arrays['ev_i'], z['ev_i'])
    i2u = [list(z['hu_users'][z['hu_ptr'][c]:z['hu_ptr'][c + 1]]) for c in range(n)]
    g = oi.Graph(arrays['ev_ptr'], arrays['ev_i'], n, meta['rho'], meta['beta'], meta['eta'], i2u)
    return z, meta, rec, g, arrays


def _load_test(conf, test):
    if not test:
        return []
    from yue_amd.tool.config import LineConfig
    from yue_amd.tool.file import FileIO
    setup = LineConfig(conf['record.setup'])
    cols = dict((a, int(b)) for a, b in (c.split(':') for c in setup['-columns'].split(',')))
    return FileIO.loadDataSet(test, columns=cols, delim=setup['-delim'])


def oracle_lists(rec, g, N):
    """{user name: [item names]} of evalRanking's list path from the oracle's topn."""
    names = rec.id2name['track']
    out = {}
    for user in rec.testSet:
        if user not in rec.userRecord:
            out[user] = ['0']
            continue
        items, _ = oi.topn(g, rec.getId(user, 'user'), N)
        out[user] = [names[int(i)] for i in items]
    return out


@pytest.mark.parametrize('tag', sorted(oi.CASES))
def test_oracle_equals_the_reference(tmp_path, tag):
    z, meta, rec, g, _ = load_case(tmp_path, tag)
    for t, u in enumerate(z['p_users']):
        items, scores = oi.predict(g, u)
        lo, hi = z['p_ptr'][t], z['p_ptr'][t + 1]
        assert np.array_equal(items, z['p_items'][lo:hi]) and np.array_equal(scores, z['p_scores'][lo:hi]), u
    top = [int(x) for x in meta['topN'].split(',')]
    lists = oracle_lists(rec, g, top[-1])
    text = HEADER + ''.join(list_line(u, lists[u], rec.testSet[u], rec.PopTrack) for u in rec.testSet)
    assert text == meta['lists']
    assert Measure.rankingMeasure(rec.testSet, lists, top, rec.getSize('track')) == meta['measure']


@pytest.mark.parametrize('tag', sorted(oi.CASES))
def test_plugin_graph_equals_the_oracle_graph(tmp_path, tag):
    from yue_amd.recommender.cf.IPF import ipf_graph
    z, meta, rec, g, arrays = load_case(tmp_path, tag)
    n = rec.getSize('track')
    pg = ipf_graph(arrays['ev_ptr'], arrays['ev_i'], n, meta['rho'], meta['beta'], meta['eta'], (z['hu_ptr'], z['hu_users']))
    for u in range(g.m):
        assert np.array_equal(pg['u_items'][pg['u_ptr'][u]:pg['u_ptr'][u + 1]], g.D[0][u])
        assert np.array_equal(pg['s_items'][pg['s_ptr'][u]:pg['s_ptr'][u + 1]], g.D[1][u])
    for c in range(n):
        lo, hi = pg['hs_ptr'][c], pg['hs_ptr'][c + 1]
        assert np.array_equal(pg['hs_users'][lo:hi], g.H[1][c][0]) and np.array_equal(pg['hs_pos'][lo:hi], g.H[1][c][1])
    assert np.array_equal(pg['w_user'], g.W[0]) and np.array_equal(pg['w_sess'], g.W[1])
    assert np.array_equal(pg['p_i2u'], g.P[0]) and np.array_equal(pg['p_i2s'], g.P[1])
    assert (pg['r_user'], pg['r_sess']) == tuple(g.r)
    if tag != 'ipf_t':                                  # grouped training sets: the default item2user order is the listened one
        dg = ipf_graph(arrays['ev_ptr'], arrays['ev_i'], n, meta['rho'], meta['beta'], meta['eta'])
        assert np.array_equal(dg['hu_ptr'], z['hu_ptr']) and np.array_equal(dg['hu_users'], z['hu_users'])


def test_fixtures_cover_the_quirks(tmp_path):
    t = gz('g12_ipf_t.npz')
    rows = [t['hu_users'][t['hu_ptr'][c]:t['hu_ptr'][c + 1]] for c in range(int(t['n']))]
    assert sum(np.any(np.diff(r) < 0) for r in rows) > 100                 # item2user order is not user-id order
    z = gz('g12_ipf_z.npz')
    zj = gj('g12_ipf_z.json')
    assert zj['init_lines'] == ['initializing STG...']
    assert '\nzu0:$0,\n' in zj['lists'] or '\nzu0:0,\n' in zj['lists']    # test-only users: ['0']
    assert '\niso:\n' in zj['lists']                                        # only its own items are reached
    deg = np.bincount(z['ev_u'], minlength=int(z['m']))
    assert (deg == 0).sum() == 4 and deg[deg > 0].min() == 1                # test-only users; 'one'
    assert np.bincount(z['ev_i'][z['ev_u'] == np.argmax(deg == 24)]).max() == 24   # 'rep' plays t7 24 times
    assert gj('g12_ipf_b1.json')['beta'] == 1.0 and gj('g12_ipf_b1.json')['rho'] == 0.5   # r_sess = 1 - beta = 0
    assert gj('g12_ipf_rho2.json')['rho'] == 0.5
    s = gj('g12_ipf_s.json')
    assert '-sample' in s['eval'] and len(s['progress_lines']) == 1 and s['lists'].count('\n') == 41


def test_eta_must_be_positive(tmp_path, capsys):
    from yue_amd.recommender.cf.IPF import IPF
    conf, _ = case_conf(tmp_path, 'ipf_z')
    conf.config['IPF'] = '-rho 1 -beta 0.7 -eta 0'
    rec = IPF(conf, _load(conf), [])
    with pytest.raises(SystemExit):
        rec.readConfiguration()
    assert '-eta must be positive' in capsys.readouterr().out
    conf.config['IPF'] = '-rho 3 -beta 0.7 -eta 0.3'
    rec.readConfiguration()
    assert rec.rho == 0.5
