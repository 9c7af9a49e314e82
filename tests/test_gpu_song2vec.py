"""GPU: Song2vec's iteration (yue_s2v_*) against the CPU contract (tests/helpers/numpy_song2vec.py), against
the reference's own Song2vec (tests/golden/g16_song2vec_*) and through the plugin surface.

Bounds.  Device against the contract in the device's form (dot=butterfly, square=product) from identical inputs: bit for bit,
X, Y, Bu, Bi and every returned squared error, under both schedules.  Against the reference: the case's butterfly-vs-np.dot
figure ('measured' in the json, computed on the CPU by the golden tool) times 4, never less than float32 resolution of the
largest entry (2^-24).
"""
import random

import numpy as np
import pytest

from helpers import numpy_song2vec as ns
from test_host_golden import _conf_text, _load
from test_song2vec_golden import CASES, KEYS, bound, load, printed_losses, run, start

pytestmark = pytest.mark.gpu

F32 = 2.0 ** -24


@pytest.fixture(scope='module')
def dev():
    from yue_amd._shim import Device
    d = Device(0, raise_errors=True)
    yield d
    d.close()


def upload(dev, S, steps, pairs):
    dev.set_factors(S[0], S[1])
    dev.s2v_set_state(S[2], S[3])
    dev.s2v_set_steps(*steps)
    dev.s2v_set_pairs(*pairs)


def state(dev):
    return dev.get_factors() + dev.s2v_get_state()


@pytest.mark.parametrize('tag', CASES)
def test_iterations_equal_the_contract_bit_for_bit(dev, tag):
    z, st, meta, ev_ptr, ev_i, steps, pairs, h = load(tag)
    want = run(tag, 'device')
    runs = {}
    for schedule in (1, 0):
        dev.set_option('s2v_schedule', schedule)
        upload(dev, start(z), steps, pairs)
        assert dev.get_option('s2v_levels_steps') == meta['levels_steps'] and dev.get_option('s2v_levels_pairs') == meta['levels_pairs']
        got = []
        for t in range(int(z['iters'])):
            e1, e2 = dev.s2v_epoch(h['lRate'], h['regU'], h['regI'], h['regB'], h['alpha'], 0.0)
            got.append((state(dev), e1, e2))
            if t in (0, int(z['iters']) - 1):                      # after one and after all iterations
                S, loss, w1, w2 = want[t]
                for key, a, b in zip(KEYS, got[t][0], S):
                    assert a.dtype == b.dtype and np.array_equal(a, b), (schedule, key, t)
                assert np.array_equal(e1, w1) and np.array_equal(e2, w2), (schedule, t)
        runs[schedule] = got
    dev.set_option('s2v_schedule', 1)
    for (Sa, a1, a2), (Sb, b1, b2) in zip(runs[1], runs[0]):
        for a, b in zip(Sa, Sb):
            assert np.array_equal(a, b)
        assert np.array_equal(a1, b1) and np.array_equal(a2, b2)
    # ... and within the measured figure of the reference
    for t in range(int(z['iters'])):
        loss = float(ns.compose_loss(runs[1][t][1], runs[1][t][2].astype(np.float32), *runs[1][t][0], regB=h['regB']))
        ref = printed_losses(meta)[t]
        print(tag, t, 'loss', loss, ref, abs(loss - ref) / abs(ref), bound(meta, 'loss', F32))
        assert abs(loss - ref) <= bound(meta, 'loss', F32) * abs(ref)
        for key, a in zip(KEYS, runs[1][t][0]):
            print(tag, t, key, ns.rel(a, st[key + 's'][t]), bound(meta, key, F32))
            assert ns.rel(a, st[key + 's'][t]) <= bound(meta, key, F32), key


def _golden_log(tmp_path, meta):
    from yue_amd import synth
    m, n, d = meta['dataset'][:3]
    log = tmp_path / 'log.txt'
    synth.write_text_log(str(log), m, n, d)
    with open(str(log), 'a') as f:
        for ln in meta['append']:
            f.write(ln + '\n')
    return log


def _conf(tmp_path, log, z, meta, extra=None):
    from yue_amd.tool.config import Config
    o = meta['options']
    kv = {'record': str(log), 'recommender': 'Song2vec', 'num.factors': str(int(z['k'])), 'num.max.iter': str(int(z['iters'])),
          'item.ranking': '-topN ' + meta['topN'], 'learnRate': '-init 0.02 -max 1', 'reg.lambda': '-u 1 -i 0.1 -b 0.2 -s 0.2',
          'Song2vec': '-alpha %s -k %d' % (o['alpha'], o['k']), 'output.setup': 'on -dir ' + str(tmp_path / 'results') + '/'}
    kv.update(extra or {})
    path = tmp_path / 'song2vec.conf'
    path.write_text(_conf_text(kv, {'bpr.hip': '-gpu 0'}))
    return Config(str(path))


@pytest.mark.parametrize('tag', CASES)
def test_goldens_through_the_plugin(tmp_path, capsys, monkeypatch, tag):
    from yue_amd.evaluation.measure import Measure
    from yue_amd.recommender.advanced.Song2vec import Song2vec
    from yue_amd.yue import Yue
    z, st, meta, ev_ptr, ev_i, steps, pairs, h = load(tag)
    assert (h['lRate'], h['regU'], h['regI'], h['regB']) == (0.02, 1.0, 0.1, 0.2)
    conf = _conf(tmp_path, _golden_log(tmp_path, meta), z, meta)
    kept = {}
    build = Song2vec.buildModel

    def spy(self):
        kept['rec'] = self
        return build(self)
    monkeypatch.setattr(Song2vec, 'buildModel', spy)
    monkeypatch.setattr(Song2vec, 'T', z['T'], raising=False)                  # the golden's table ...
    monkeypatch.setattr(Song2vec, 'pairOrder', (pairs[0], pairs[1]), raising=False)   # ... and visiting order
    random.seed(int(z['seed']))
    np.random.seed(int(z['seed']))
    Yue(conf).execute()
    out = capsys.readouterr().out
    rec = kept['rec']
    lines = [ln for ln in out.splitlines() if ln.startswith('iteration:')]
    ref_losses = printed_losses(meta)
    assert 'training...' in out.splitlines() and len(lines) == len(ref_losses)
    for t, (ln, ref) in enumerate(zip(lines, ref_losses)):
        head, val = ln.split(' loss: ')
        assert head == 'iteration: %d' % (t + 1)
        assert abs(float(val) - ref) <= bound(meta, 'loss', F32) * abs(ref)
    for key, a in zip(KEYS, (rec.X, rec.Y, rec.Bu, rec.Bi)):
        assert ns.rel(a, st[key + 's'][-1]) <= bound(meta, key, F32), key
    assert rec.X.dtype == np.float32 and rec.Bu.dtype == np.float64
    assert set(rec.topKSim) == set(rec.data.id2name['track'][int(t)] for t in z['listen'])
    # lists of the stable test users, measures over them
    N = max(int(x) for x in meta['topN'].split(','))
    users = list(rec.data.testSet.keys())
    uids = np.array([rec.data.getId(u, 'user') for u in users], np.int32)
    assert np.array_equal(uids, z['test_users'])
    ids = rec._scan(users, N)
    stable = z['stable_users']
    assert stable.sum() >= 0.9 * len(users)
    assert np.array_equal(ids[stable], z['rec_ids'][stable])
    if stable.all():
        assert rec.measure == meta['measure']
    names = rec.data.id2name[rec.recType]
    top = [int(x) for x in meta['topN'].split(',')]
    origin = {u: rec.data.testSet[u] for t, u in enumerate(users) if stable[t]}
    mine = {u: [names[int(x)] for x in ids[t]] for t, u in enumerate(users) if stable[t]}
    gold = {u: [names[int(x)] for x in z['rec_ids'][t]] for t, u in enumerate(users) if stable[t]}
    size = rec.data.getSize(rec.recType)
    assert Measure.rankingMeasure(origin, mine, top, size) == Measure.rankingMeasure(origin, gold, top, size)
    # predict adds the user's constant on the host, as the reference adds it
    u = users[0]
    sc = rec.predict(u)
    assert sc.dtype == np.float64 and np.array_equal(sc, rec.dev.scores(rec.data.getId(u, 'user')) + 0 + rec.Bu[rec.data.getId(u, 'user')])


def test_plugin_embeds_on_the_device_and_refuses_other_targets(tmp_path, capsys):
    """-emb hip, the default: sentences -> segments -> embedding -> similar tracks -> iterations, from a text log alone."""
    from yue_amd.recommender.advanced.Song2vec import Song2vec
    z, st, meta, ev_ptr, ev_i, steps, pairs, h = load('s_k65')
    log = _golden_log(tmp_path, meta)
    conf = _conf(tmp_path, log, z, meta, {'num.factors': '20'})
    rec = Song2vec(conf, _load(conf), [])
    rec.readConfiguration()
    assert rec.embSource == 'hip'
    np.random.seed(1)
    rec.initModel()
    rec.buildModel()
    out = capsys.readouterr().out
    assert len([ln for ln in out.splitlines() if ln.startswith('iteration:')]) == int(z['iters'])
    assert np.isfinite(float(rec.loss)) and rec.embed_ns > 0
    listen = z['listen'].astype(np.int64)
    assert rec.T.shape == (int(z['n']), 20) and np.all(np.abs(rec.T[listen]).sum(axis=1) > 0)
    assert all(len(v) == int(z['K']) for v in rec.topKSim.values()) and len(rec.topKSim) == len(listen)
    # the same seed gives the same embedding: the stage is bit-reproducible
    again = Song2vec(conf, _load(conf), [])
    again.readConfiguration()
    np.random.seed(1)
    again.initModel()
    again.buildModel()
    assert np.array_equal(again.T, rec.T) and np.array_equal(again.X, rec.X) and np.array_equal(again.Bi, rec.Bi)
    bad = _conf(tmp_path, log, z, meta, {'evaluation.setup': '-target artist -byTime 0.2'})
    with pytest.raises(SystemExit):
        Song2vec(bad, _load(bad), []).readConfiguration()
    assert '-target track' in capsys.readouterr().out
