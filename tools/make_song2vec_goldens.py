#!/usr/bin/env python3
"""Generate tests/golden/g16_song2vec_* by running the REFERENCE's own Song2vec class (recommender/advanced/Song2vec.py).

Only runs where the reference tree exists (the helpers of tools/make_goldens.py are imported, which loads it); run with
PYTHONHASHSEED=0 (the reference visits a set of track names: the order is recorded, whatever it is).  Nothing from the reference
is copied: the fixtures are inputs (seeds, options, our synthetic logs, a seeded table) and what the reference computes from them.

How the reference is driven: config/Song2vec.conf with record / num.factors / num.max.iter / Song2vec / item.ranking /
output.setup changed.  gensim is not installed: the import of gensim.models.word2vec is satisfied by a module object whose
Word2Vec is the small class below -- it trains nothing and returns a seeded float32 table wv[name] (standard normal, by track
number).  The state after every iteration is copied when the class prints its ``iteration:`` line.

Per case the tool asserts that the CPU contract (tests/helpers/numpy_song2vec.py) with dot=np.dot reproduces X, Y, Bu, Bi and
the printed losses bit for bit, and measures the same contract in the device's form (dot=butterfly, square=product) against it
('measured' in the json; the GPU tests allow four times these).  No two adjacent cosines of a list may be closer than 1e-9
(the rule of g15_cune_friends).  A test user's list is stable when no two scores the overwrite-scan compared are closer than the
score error of a device as far from the reference as the butterfly contract is, times 4 (numpy_expomf.score_error); every case
must keep 90 % of its test users stable, or the tool fails.
"""
import contextlib
import json
import os
import random
import sys
import tempfile
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'tests'))

import make_goldens as mg                                       # noqa: E402  (puts the reference on sys.path)
from helpers import numpy_expomf as ne                          # noqa: E402
from helpers import numpy_song2vec as ns                        # noqa: E402
from helpers.numpy_wrmf import pairs_from_events                # noqa: E402

SEED = 20260016


class Word2Vec(object):
    """Stands in for gensim's class: wv[name] = row (track number) of a seeded standard-normal float32 table."""
    rows = 1 << 16

    def __init__(self, sentences, size, window, min_count, iter):
        assert window == 5 and min_count == 0 and iter == 10
        self.sentences = [list(s) for s in sentences]
        table = np.random.RandomState(SEED).standard_normal((self.rows, size)).astype(np.float32)
        self.wv = {name: table[int(name[1:])] for s in self.sentences for name in s}


def install_word2vec():
    for name in ('gensim', 'gensim.models', 'gensim.models.word2vec'):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules['gensim'].models = sys.modules['gensim.models']
    sys.modules['gensim.models'].word2vec = sys.modules['gensim.models.word2vec']
    sys.modules['gensim.models.word2vec'].Word2Vec = Word2Vec


def conf_for(tmp, tag, log_path, k, iters, alpha, K, topn):
    out = []
    for ln in open(os.path.join(mg.REF, 'config/Song2vec.conf')).read().splitlines():
        key = ln.split('=')[0]
        if key == 'record':
            ln = 'record=' + log_path
        elif key == 'num.factors':
            ln = 'num.factors=%d' % k
        elif key == 'num.max.iter':
            ln = 'num.max.iter=%d' % iters
        elif key == 'Song2vec':
            ln = 'Song2vec=-alpha %s -k %d' % (alpha, K)
        elif key == 'item.ranking':
            ln = 'item.ranking=-topN ' + topn
        elif key == 'output.setup':
            ln = 'output.setup=on -dir ' + os.path.join(tmp, 'results_song2vec') + '/'
        out.append(ln)
    path = os.path.join(tmp, 'song2vec_%s.conf' % tag)
    open(path, 'w').write('\n'.join(out) + '\n')
    return path


class Snapshots(object):
    """stdout of buildModel: keeps the text and copies the state whenever an ``iteration:`` line begins."""

    def __init__(self, rec):
        self.rec, self.text, self.states, self.sentences = rec, [], [], None

    def write(self, s):
        if s == 'iteration:':
            r = self.rec
            self.states.append((r.X.copy(), r.Y.copy(), r.Bu.copy(), r.Bi.copy()))
        self.text.append(s)

    def flush(self):
        pass


def small_log_lines():
    """Appended to the (64, 64, 12) log, whose users all keep 9 training events: three users in four get 8 more events
    (16 training events after the split), so a quarter of the users stays untrained; popular tracks repeat."""
    rng = np.random.RandomState(SEED + 1)
    out = []
    for s in range(12, 20):
        for u in range(64):
            if u % 4:
                i = int(64 * rng.rand() ** 2)
                out.append('%010d,u%d,t%d,a%d' % (s, u, i, i % 50))
    return out


def case(tmp, tag, dataset, extra_lines, k, K, iters, alpha='0.5', topn='5,10'):
    import recommender.advanced.Song2vec as sv
    m0, n0, d0 = dataset
    log_path = os.path.join(tmp, tag + '.txt')
    mg.synth.write_text_log(log_path, m0, n0, d0)
    with open(log_path, 'a') as f:
        for ln in extra_lines:
            f.write(ln + '\n')
    conf = mg.Config(conf_for(tmp, tag, log_path, k, iters, alpha, K, topn))
    rec, _ = mg.quiet(sv.Song2vec, conf, mg.load_train(conf), [])
    rec.readConfiguration()
    assert rec.topK == K and rec.alpha == float(alpha) and rec.maxIter == iters
    d_, rt = rec.data, rec.recType
    assert rt == 'track' and d_.globalMean == 0
    random.seed(SEED)
    np.random.seed(SEED)
    mg.quiet(rec.initModel)
    m, n = rec.m, rec.n
    X0, Y0, Bu0, Bi0 = rec.X.copy(), rec.Y.copy(), rec.Bu.copy(), rec.Bi.copy()
    for a, b in zip((X0, Y0, Bu0, Bi0), ns.init_from_seed(SEED, m, n, k)):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    snap = Snapshots(rec)
    t0 = time.time()
    with contextlib.redirect_stdout(snap):
        rec.buildModel()
    build_s = time.time() - t0
    lines = [ln for ln in ''.join(snap.text).splitlines() if ln.startswith('iteration:')]
    assert len(lines) == iters == len(snap.states)
    gid = lambda name: d_.getId(name, 'track')                   # noqa: E731
    # the table and the order in which the reference visited topKSim
    listen = np.array(sorted(gid(t) for t in rec.listenTrack), np.int32)
    T = np.zeros((n, k), np.float32)
    T[listen] = rec.T[listen].astype(np.float32)
    assert np.array_equal(T[listen].astype(np.float64), rec.T[listen])
    t1, t2, sim = [], [], []
    for a, lst in rec.topKSim.items():
        assert len(lst) == min(K, len(listen) - 1)
        sims = [s for _, s in lst]
        assert all(type(s) is float for s in sims)
        assert all(x - y > 1e-9 for x, y in zip(sims, sims[1:])), '%s: two adjacent cosines of %s are closer than 1e-9' % (tag, a)
        for b, s in lst:
            t1.append(gid(a)); t2.append(gid(b)); sim.append(s)
    t1, t2, sim = np.array(t1, np.int32), np.array(t2, np.int32), np.array(sim, np.float64)
    ev_u, ev_i = mg.record_arrays(rec)
    ev_ptr = np.concatenate([[0], np.cumsum(np.bincount(ev_u, minlength=m))]).astype(np.int64)
    assert np.all(np.diff(ev_u) >= 0)
    users, sents = ns.sentences(ev_ptr, ev_i)
    assert [d_.getId(u, 'user') for u in rec.user] == users
    steps = ns.user_listen(ev_ptr, ev_i)
    pairs = (t1, t2, sim)
    lr, regU, regI, regB, al = rec.lRate, rec.regU, rec.regI, rec.regB, rec.alpha
    # the contract, bit for bit; and with the device's summation order
    A = [x.copy() for x in (X0, Y0, Bu0, Bi0)]
    B = [x.copy() for x in (X0, Y0, Bu0, Bi0)]
    meas = {key: 0.0 for key in ('X', 'Y', 'Bu', 'Bi', 'loss')}
    t0 = time.time()
    for t in range(iters):
        loss_a = ns.iteration(A[0], A[1], A[2], A[3], steps, pairs, lr, regU, regI, regB, al, 0, np.dot)[0]
        for a, b in zip(A, snap.states[t]):
            assert a.dtype == b.dtype and np.array_equal(a, b), (tag, t)
        assert 'iteration: %d loss: %s' % (t + 1, loss_a) == lines[t], (lines[t], loss_a)
        loss_b = ns.iteration(B[0], B[1], B[2], B[3], steps, pairs, lr, regU, regI, regB, al, 0, ns.butterfly, square=ns.product)[0]
        now = dict(zip(('X', 'Y', 'Bu', 'Bi'), (ns.rel(b, a) for a, b in zip(A, B))))
        now['loss'] = abs(float(loss_b) - float(loss_a)) / abs(float(loss_a))
        for key in meas:
            meas[key] = max(meas[key], now[key])
    contract_s = time.time() - t0
    # lists
    tu = list(d_.testSet.keys())
    orig = mg.Measure.rankingMeasure
    captured = {}

    def spy(origin, res, N, itemCount):
        captured['res'] = {u: list(v) for u, v in res.items()}
        return orig(origin, res, N, itemCount)
    mg.Measure.rankingMeasure = staticmethod(spy)
    try:
        mg.quiet(rec.evalRanking)
    finally:
        mg.Measure.rankingMeasure = staticmethod(orig)
    ids = np.array([[gid(x) for x in captured['res'][u]] for u in tu], np.int32)
    measure = list(rec.measure)
    tuid = np.array([d_.getId(u, 'user') for u in tu], np.int32)
    um, _im = pairs_from_events(ev_u, ev_i, m, n)
    N = max(int(x) for x in topn.split(','))
    stable = np.zeros(len(tu), bool)
    for t, u in enumerate(tuid):
        scores = A[1].dot(A[0][u])
        masked = set(int(i) for i in um[1][um[0][u]:um[0][u + 1]])
        mine, margin = ne.overwrite_scan(scores, masked, N, ne.score_error(A[0], A[1], B[0], B[1], u))
        assert mine == [int(x) for x in ids[t]], (tag, u)
        stable[t] = margin > 0
    lv_s, lv_p = ns.levels(steps[0], steps[1]), ns.levels(t1, t2, shared=True)
    untrained = m - len(users)
    print('%-8s m=%d n=%d k=%d K=%d: trained users %d of %d, tracks with a row %d, steps %d (levels %d) pairs %d (levels %d), max count %d; '
          'butterfly vs np.dot %s; stable %d/%d (reference buildModel %.1f s, contract %.1f s)'
          % (tag, m, n, k, K, len(users), m, len(listen), len(steps[0]), lv_s.max() + 1 if len(lv_s) else 0, len(t1), lv_p.max() + 1,
             steps[2].max(), ' '.join('%s %.1e' % kv for kv in meas.items()), stable.sum(), len(tu), build_s, contract_s))
    assert stable.sum() >= 0.9 * len(tu), '%s: only %d of %d lists are stable' % (tag, stable.sum(), len(tu))
    if tag.startswith('s_'):
        assert 4 * untrained >= m and steps[2].max() > 1, 'the small log needs a quarter of untrained users and repeated events'
    small = np.int16 if max(m, n) < 32768 else np.int32
    np.savez_compressed(os.path.join(mg.OUT, 'g16_song2vec_%s.npz' % tag), seed=SEED, k=k, iters=iters, m=m, n=n, K=K,
                        alpha=np.float64(al), lRate=np.float64(lr), regU=np.float64(regU), regI=np.float64(regI), regB=np.float64(regB),
                        ev_u=ev_u.astype(small), ev_i=ev_i.astype(small), T=T, listen=listen.astype(small),
                        t1=t1.astype(small), t2=t2.astype(small), sim=sim, test_users=tuid, rec_ids=ids.astype(small), stable_users=stable)
    np.savez_compressed(os.path.join(mg.OUT, 'g16_song2vec_%s_states.npz' % tag), Xs=np.stack([s[0] for s in snap.states]),
                        Ys=np.stack([s[1] for s in snap.states]), Bus=np.stack([s[2] for s in snap.states]),
                        Bis=np.stack([s[3] for s in snap.states]))
    json.dump({'lines': lines, 'measure': measure, 'dataset': list(dataset), 'append': list(extra_lines), 'topN': topn,
               'options': {'alpha': alpha, 'k': K},
               'measured': {'butterfly_vs_npdot_' + key: v for key, v in meas.items()},
               'levels_steps': int(lv_s.max()) + 1 if len(lv_s) else 0, 'levels_pairs': int(lv_p.max()) + 1,
               'trained_users': len(users), 'stable_users': int(stable.sum()), 'test_users': len(tu),
               'reference_seconds': {'buildModel': build_s, 'iterations': iters}},
              open(os.path.join(mg.OUT, 'g16_song2vec_%s.json' % tag), 'w'), indent=1)


def main():
    os.makedirs(mg.OUT, exist_ok=True)
    install_word2vec()
    tmp = tempfile.mkdtemp(prefix='yue_gold_song2vec_')
    only = sys.argv[1:]
    extra = small_log_lines()
    #        tag        dataset           appended  k    K   iters
    cases = [('c1_k20', (1000, 1000, 20), [],       20,  10, 3),            # the shipped config/Song2vec.conf values
             ('s_k65', (64, 64, 12),      extra,    65,  3,  2),
             ('s_k128', (64, 64, 12),     extra,    128, 1,  2)]
    for tag, ds, lines, k, K, iters in cases:
        if not only or tag in only:
            case(tmp, tag, ds, lines, k, K, iters)


if __name__ == '__main__':
    main()
