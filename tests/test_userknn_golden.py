"""CPU: the NumPy oracle of UserKNN (tests/helpers/numpy_userknn.py) against what the reference's own UserKNN class computed
(tests/golden/g11_userknn_*, tools/make_userknn_goldens.py): neighbour ids and similarities, predict lists and scores, the
lists file of evalRanking and its measure strings -- all bit for bit."""
import os

import numpy as np
import pytest

from helpers import numpy_userknn as ok
from test_host_golden import _load
from util import gj, gz
from yue_amd.data.record import Record
from yue_amd.evaluation.measure import Measure
from yue_amd.recommender.cf.UserKNN import HEADER, list_line
from yue_amd.tool.config import Config


def case_conf(tmp_path, tag):
    """config/UserKNN.conf of this repository with the case's log, neighbours and list sizes (as the fixture was made)."""
    log = str(tmp_path / (tag + '.txt'))
    ok.write_case_log(tag, log)
    c = ok.CASES[tag]
    text = ('record=%s\nrecord.setup=-columns user:1,track:2,artist:3,time:0 -delim ,\nevaluation.setup=-target track -byTime 0.2\n'
            'recommender=UserKNN\nitem.ranking=-topN %s\nnum.neighbors=%d\noutput.setup=on -dir %s/\nbpr.hip=-gpu 0\n'
            % (log, c['topN'], c['K'], tmp_path / 'results'))
    path = tmp_path / (tag + '.conf')
    path.write_text(text)
    return Config(str(path))


def load_case(tmp_path, tag):
    z = gz('g11_%s.npz' % tag)
    conf = case_conf(tmp_path, tag)
    rec = Record(conf, _load(conf), [])
    arrays = rec.to_arrays('track')
    m, n = rec.getSize('user'), rec.getSize('track')
    ev_u = np.repeat(np.arange(m, dtype=np.int32), np.diff(arrays['ev_ptr']))
    assert m == int(z['m']) and n == int(z['n'])
    assert np.array_equal(ev_u, z['ev_u']) and np.array_equal(arrays['ev_i'], z['ev_i'])
    (up, ui, uc), (ip, iu) = ok.pairs_from_events(arrays['ev_ptr'], arrays['ev_i'], n)
    return z, rec, conf, (up, ui, uc), (ip, iu)


def oracle_lists(rec, up, ui, uc, nbr, inter, uni, N):
    """{user name: [item names]} of evalRanking's list path from the oracle's topn."""
    names = rec.id2name['track']
    out = {}
    for user in rec.testSet:
        if user not in rec.userRecord:
            out[user] = ['0']
            continue
        u = rec.getId(user, 'user')
        items, _ = ok.topn(up, ui, uc, u, nbr[u], inter[u], uni[u], rec.getSize('track'), N)
        out[user] = [names[int(i)] for i in items]
    return out


@pytest.mark.parametrize('tag', sorted(ok.CASES))
def test_oracle_equals_the_reference(tmp_path, tag):
    z, rec, conf, (up, ui, uc), (ip, iu) = load_case(tmp_path, tag)
    meta = gj('g11_%s.json' % tag)
    K = int(z['K'])
    nbr, inter, uni = ok.neighbors(up, ui, ip, iu, K)
    assert np.array_equal(nbr, z['nbr'])
    assert np.array_equal(ok.sims(inter, uni), z['sim'])                   # bit for bit
    for t, u in enumerate(z['p_users']):
        items, scores = ok.predict(up, ui, uc, nbr[u], inter[u], uni[u], rec.getSize('track'))
        lo, hi = z['p_ptr'][t], z['p_ptr'][t + 1]
        assert np.array_equal(items, z['p_items'][lo:hi]) and np.array_equal(scores, z['p_scores'][lo:hi]), u
    top = [int(x) for x in meta['topN'].split(',')]
    lists = oracle_lists(rec, up, ui, uc, nbr, inter, uni, top[-1])
    text = HEADER + ''.join(list_line(u, lists[u], rec.testSet[u], rec.PopTrack) for u in rec.testSet)
    assert text == meta['lists']
    assert Measure.rankingMeasure(rec.testSet, lists, top, rec.getSize('track')) == meta['measure']


def test_fixtures_cover_the_quirks():
    c1 = gz('g11_userknn_c1_k20.npz')
    # ties at the K-th boundary (the id order decides who is in); test-only users have no neighbours at all
    assert np.sum(c1['sim'][:, -1] == c1['sim'][:, -2]) > 100
    zz = gz('g11_userknn_z_k10.npz')
    assert (zz['nbr'][np.bincount(zz['ev_u'], minlength=int(zz['m'])) == 0] == -1).all()
    z = gj('g11_userknn_z_k10.json')
    assert '\nzu0:$0,\n' in z['lists'] and ',$0,' in z['lists']          # ['0']*N -> one item, which is in PopTrack
    h = gz('g11_userknn_h_k20.npz')
    deg = np.bincount(h['ev_u'])
    assert deg.min() >= 200                                                   # 20 neighbours x 200+ items: chunked scoring
    for tag in ok.CASES:
        lines = gj('g11_%s.json' % tag)['init_lines']
        assert lines[0] == 'Computing user similarities...' and lines[-1] == 'The user correlation has been figured out.'
