#!/usr/bin/env python3
"""Generate tests/golden/g13_expomf_* by running the REFERENCE's own ExpoMF (recommender/advanced/ExpoMF.py).

Only runs where the reference tree exists (the helpers of tools/make_goldens.py are imported, which loads it).  Nothing
from the reference is copied: the fixtures are inputs (seeds, our synthetic logs, theta0, beta0) and what the reference
computes from them (theta, beta, mu after every iteration, evalRanking's lists and measure strings: both as shipped, where
evalRanking ranks with the base class's untrained P and Q because ExpoMF overrides predictForRanking and not predict, and
with the class's predictForRanking bound to predict on the instance).

How the reference is driven: config/ExpoMF.conf with record / num.factors / num.max.iter / item.ranking / evaluation.setup
(-byTime 0.2, the split the other fixtures use) / output.setup changed; NumPy and ``random`` seeded here.  The class reads
self.m and self.n in initModel, which only DeepRecommender sets: the tool sets those two attributes on the instance and
otherwise drives the class unchanged.  buildModel runs with maxIter = 1 once per iteration so that theta, beta, mu can be
taken after every iteration; its ``ITERATION #0`` line is renumbered.

Per case and per output the tool measures e_ref = reference against the contract (tests/helpers/numpy_expomf.py, iterated,
max |a - b| / max |b|) and writes it into the json; the tests derive every bound from it.  It also decides whether the
reference's own top-N lists are stable under the score error of a device as close to the contract as the reference is, times 4
(numpy_expomf.score_error; per user: no two scores the overwrite-scan compared are closer than their errors).  The small case
expomf_s_k20 must come out stable for every user, or the tool fails.

g13_expomf_c2rows: C2 (100,000 x 50,000, 50 events per user, the shape of bench.py --workload c2) with seeded factors at
k = 64: the reference's a_row_batch + _solve on 256 sampled users and 256 sampled items; the inputs are regenerated from the
seeds by tests/helpers/numpy_expomf.py: c2_inputs.

g13_expomf_trained.json: no reference run, settings and recorded results only.  The cases of tests/test_gpu_expomf_stages.py
(numpy_expomf.TRAINED: seeded inputs at trained scale, regenerated from the seeds by the tests) with e_ref per case and per
output: the reference's arithmetic (numpy_expomf.expo_reference_rows / _gram / _mu, pinned to the reference's class by
tests/test_expomf_golden.py and tests/test_expomf_power.py) against the fp64 contract on the same inputs.  The tool fails if
any e_ref exceeds 1e-5: a badly conditioned shape must be reshaped, not given a loose bound.
"""
import json
import os
import random
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'tests'))

import make_goldens as mg                                       # noqa: E402  (puts the reference on sys.path)
from helpers import numpy_expomf as ne                          # noqa: E402
from helpers.numpy_wrmf import pairs_from_events                # noqa: E402

SEED = 20260013


def conf_for(tmp, log_path, k, iters, topn):
    out = []
    for ln in open(os.path.join(mg.REF, 'config/ExpoMF.conf')).read().splitlines():
        key = ln.split('=')[0]
        if key == 'record':
            ln = 'record=' + log_path
        elif key == 'num.factors':
            ln = 'num.factors=%d' % k
        elif key == 'num.max.iter':
            ln = 'num.max.iter=%d' % iters
        elif key == 'evaluation.setup':
            ln = 'evaluation.setup=-target track -byTime 0.2'
        elif key == 'item.ranking':
            ln = 'item.ranking=-topN ' + topn
        elif key == 'output.setup':
            ln = 'output.setup=on -dir ' + os.path.join(tmp, 'results_expomf') + '/'
        out.append(ln)
    path = os.path.join(tmp, 'expomf_%s.conf' % os.path.basename(log_path))
    open(path, 'w').write('\n'.join(out) + '\n')
    return path


def case(tmp, tag, dataset, extra_lines, k, iters, topn='5,10', must_be_stable=False):
    import recommender.advanced.ExpoMF as em
    m0, n0, d = dataset
    log_path = os.path.join(tmp, tag + '.txt')
    mg.synth.write_text_log(log_path, m0, n0, d)
    with open(log_path, 'a') as f:
        for ln in extra_lines:
            f.write(ln + '\n')
    conf = mg.Config(conf_for(tmp, log_path, k, iters, topn))
    rec, _ = mg.quiet(em.ExpoMF, conf, mg.load_train(conf), [])
    rec.readConfiguration()
    random.seed(SEED)
    np.random.seed(SEED)
    rec.m = rec.data.getSize('user')
    rec.n = rec.data.getSize(rec.recType)
    rec.initModel()
    m, n = rec.m, rec.n
    theta0, beta0, mu0 = rec.theta.copy(), rec.beta.copy(), rec.mu.copy()
    assert theta0.dtype == np.float32 and beta0.dtype == np.float32 and mu0.dtype == np.float32
    assert all(np.array_equal(x, y) for x, y in zip((theta0, beta0), ne.init_from_seed(SEED, m, n, k)))
    rec.maxIter = 1
    thetas, betas, mus, lines = [], [], [], []
    t0 = time.time()
    for it in range(iters):
        _, out = mg.quiet(rec.buildModel)
        got = out.splitlines()
        assert got[0] == 'training...' and got[1] == 'ITERATION #0' and got[2] == 'update factors...' and got[3] == '\tUpdating exposure prior...'
        if it == 0:
            lines.append(got[0])
        lines += ['ITERATION #%d' % it, got[2], got[3]]
        thetas.append(rec.theta.copy())
        betas.append(rec.beta.copy())
        mus.append(rec.mu.copy())
    ref_s = time.time() - t0
    assert thetas[-1].dtype == np.float32 and mus[-1].dtype == np.float32
    d_, rt = rec.data, rec.recType
    ev_u, ev_i = mg.record_arrays(rec)
    um, im = pairs_from_events(ev_u, ev_i, m, n)
    tu = list(d_.testSet.keys())
    orig = mg.Measure.rankingMeasure

    def ranked():
        captured = {}

        def spy(origin, res, N, itemCount):
            captured['res'] = {u: list(v) for u, v in res.items()}
            return orig(origin, res, N, itemCount)
        mg.Measure.rankingMeasure = staticmethod(spy)
        try:
            mg.quiet(rec.evalRanking)
        finally:
            mg.Measure.rankingMeasure = staticmethod(orig)
        return np.array([[d_.getId(x, rt) for x in captured['res'][u]] for u in tu], np.int32), list(rec.measure)
    # as shipped, evalRanking calls predict(), which ExpoMF does not override: the lists come from the base class's untrained
    # P and Q.  The class's own ranking formula is predictForRanking (beta . theta[u]); binding it to predict on the instance
    # is the third attribute this tool sets, and the lists the device is compared with.
    ids_shipped, measure_shipped = ranked()
    assert np.array_equal(ids_shipped[0], ne.overwrite_scan(rec.Q.dot(rec.P[d_.getId(tu[0], 'user')]), set(int(i) for i in um[1][um[0][d_.getId(tu[0], 'user')]:um[0][d_.getId(tu[0], 'user') + 1]]), max(int(x) for x in topn.split(',')))[0])
    rec.predict = rec.predictForRanking
    ids, measure = ranked()
    tuid = np.array([d_.getId(u, 'user') for u in tu], np.int32)
    # e_ref: the reference against the iterated contract, per output, the largest over the iterations
    th, be, mu = theta0, beta0, mu0
    e = {'theta': 0.0, 'beta': 0.0, 'mu': 0.0}
    e_last = {}
    for t in range(iters):
        th, be, mu = ne.expo_iteration_contract(th, be, mu, um, im)
        e_last = {'theta': ne.rel(thetas[t], th), 'beta': ne.rel(betas[t], be), 'mu': ne.rel(mus[t], mu)}
        for key in e:
            e[key] = max(e[key], e_last[key])
    # list stability: a device as close to the contract as the reference is (times 4) moves a score by at most
    # numpy_expomf.score_error; a user's list is stable when no two scores the overwrite-scan compared are closer than that
    N = max(int(x) for x in topn.split(','))
    stable = np.zeros(len(tu), bool)
    for t, u in enumerate(tuid):
        scores = betas[-1].dot(thetas[-1][u])
        masked = set(int(i) for i in um[1][um[0][u]:um[0][u + 1]])
        mine, margin = ne.overwrite_scan(scores, masked, N, ne.score_error(thetas[-1], betas[-1], th, be, u))
        assert mine == [int(x) for x in ids[t]], (tag, u)
        stable[t] = margin > 0
    assert stable.all() or not must_be_stable, '%s: %d of %d lists are not stable' % (tag, (~stable).sum(), len(tu))
    trained_u = np.zeros(m, bool)
    trained_u[ev_u] = True
    trained_i = np.zeros(n, bool)
    trained_i[ev_i] = True
    np.savez_compressed(os.path.join(mg.OUT, 'g13_%s.npz' % tag), seed=SEED, k=k, iters=iters, m=m, n=n, ev_u=ev_u.astype(np.int16) if max(m, n) < 32768 else ev_u, ev_i=ev_i.astype(np.int16) if max(m, n) < 32768 else ev_i,
                        mu0=mu0, **({} if k == 128 else {'theta0': theta0, 'beta0': beta0}),   # k = 128: numpy_expomf.init_from_seed regenerates them
                        thetas=np.stack(thetas), betas=np.stack(betas), mus=np.stack(mus),
                        test_users=tuid, rec_ids=ids, rec_ids_shipped=ids_shipped, stable_users=stable,
                        zero_users=np.flatnonzero(~trained_u).astype(np.int32), zero_items=np.flatnonzero(~trained_i).astype(np.int32))
    json.dump({'lines': lines, 'measure': measure, 'measure_shipped': measure_shipped, 'dataset': list(dataset), 'append': list(extra_lines), 'topN': topn,
               'e_ref': e, 'e_ref_last_iteration': e_last, 'lists_stable': bool(stable.all()), 'stable_users': int(stable.sum()),
               'test_users': len(tu), 'max_count': int(um[2].max()), 'reference_seconds': ref_s,
               'reference_seconds_per_row': ref_s / (iters * (m + n))},
              open(os.path.join(mg.OUT, 'g13_%s.json' % tag), 'w'), indent=1)
    print('%-18s m=%d n=%d k=%d: e_ref theta %.2e beta %.2e mu %.2e; lists stable %d/%d; max count %d (reference %.1f s)'
          % (tag, m, n, k, e['theta'], e['beta'], e['mu'], stable.sum(), len(tu), um[2].max(), ref_s))


def c2rows():
    import recommender.advanced.ExpoMF as em
    from scipy.sparse import csr_matrix
    inp = ne.c2_inputs(SEED)
    m, n, k = inp['m'], inp['n'], inp['k']
    theta, beta, mu = inp['theta'], inp['beta'], inp['mu']
    (up, ui, uc), (ip, iu, ic) = inp['user_major'], inp['item_major']
    users, items = ne.c2_sample(SEED, up, ip)
    X = csr_matrix((uc.astype(np.int64), ui, up), (m, n))
    XT = csr_matrix((ic.astype(np.int64), iu, ip), (n, m))
    lam = ne.LAM_THETA / ne.LAM_Y
    t0 = time.time()
    A = em.a_row_batch(X[users], theta[users], beta, ne.LAM_Y, mu)
    ref_u = np.empty((len(users), k), np.float32)
    for t, u in enumerate(users):
        ref_u[t] = em._solve(int(u), A[t], beta, X, k, lam, ne.LAM_Y, mu)
    s_user = (time.time() - t0) / len(users)
    t0 = time.time()
    ref_i = np.empty((len(items), k), np.float32)
    for lo in range(0, len(items), 64):
        sel = items[lo:lo + 64]
        A = em.a_row_batch(XT[sel], beta[sel], theta, ne.LAM_Y, mu[sel, np.newaxis])
        for t, i in enumerate(sel):
            ref_i[lo + t] = em._solve(int(i), A[t], theta, XT, k, lam, ne.LAM_Y, mu)
    s_item = (time.time() - t0) / len(items)
    con_u = ne.expo_half_sweep_contract(beta, theta, up, ui, uc, mu, True, lam, ne.LAM_Y, rows=users)
    con_i = ne.expo_half_sweep_contract(theta, beta, ip, iu, ic, mu, False, lam, ne.LAM_Y, rows=items)
    lens_i = np.diff(ip)[items]
    assert (lens_i == 0).any() and (lens_i == 1).any()
    assert np.all(ref_i[lens_i == 0] == 0) and np.all(con_i[lens_i == 0] == 0)
    e = {'theta': ne.rel(ref_u, con_u), 'beta': ne.rel(ref_i, con_i)}
    np.savez_compressed(os.path.join(mg.OUT, 'g13_expomf_c2rows.npz'), seed=SEED, users=users.astype(np.int32), items=items.astype(np.int32),
                        ref_theta=ref_u, ref_beta=ref_i)
    json.dump({'shape': [m, n, 50, k], 'e_ref': e, 'reference_s_per_user_row': s_user, 'reference_s_per_item_row': s_item,
               'reference_s_per_iteration_extrapolated': s_user * m + s_item * n},
              open(os.path.join(mg.OUT, 'g13_expomf_c2rows.json'), 'w'), indent=1)
    print('c2rows: e_ref theta %.2e beta %.2e; reference %.3f s per user row, %.3f s per item row' % (e['theta'], e['beta'], s_user, s_item))


E_REF_CAP = 1e-5


def trained():
    out = {'rule': 'device vs contract <= max(4 * e_ref, 1e-6); e_ref = reference arithmetic vs fp64 contract on the same inputs',
           'e_ref_cap': E_REF_CAP, 'cases': {}}
    for tag, c in ne.TRAINED.items():
        e = ne.trained_e_ref(tag)
        out['cases'][tag] = dict(c, e_ref=e)
        print('%-9s m=%d n=%d k=%d: ' % (tag, c['m'], c['n'], c['k']) + ' '.join('%s %.2e' % kv for kv in sorted(e.items())), flush=True)
    inp = ne.c2_trained()
    users, items = ne.c2_sample(ne.C2_TRAINED_SEED, inp['user_major'][0], inp['item_major'][0])
    e = ne.c2_trained_e_ref(inp, users, items)
    out['c2'] = {'seed': ne.C2_TRAINED_SEED, 'shape': [inp['m'], inp['n'], 50, inp['k']], 'rows': [len(users), len(items)], 'e_ref': e}
    print('c2        ' + ' '.join('%s %.2e' % kv for kv in sorted(e.items())), flush=True)
    worst = max(max(c['e_ref'].values()) for c in list(out['cases'].values()) + [out['c2']])
    assert worst <= E_REF_CAP, 'an e_ref of %.2e exceeds the cap %.0e: reshape that case' % (worst, E_REF_CAP)
    json.dump(out, open(os.path.join(mg.OUT, 'g13_expomf_trained.json'), 'w'), indent=1)


def equalise(m0, n0, d):
    """Lines that make the number of users equal the number of tracks: test-only users (one late event each on track t0)."""
    tracks = set(r[2] for r in mg.synth.text_events(m0, n0, d))
    assert len(tracks) > m0
    return ['9999999999,eu%d,t0,a0' % q for q in range(len(tracks) - m0)]


def main():
    os.makedirs(mg.OUT, exist_ok=True)
    tmp = tempfile.mkdtemp(prefix='yue_gold_expomf_')
    only = sys.argv[1:]
    zlines = ['9999999999,zu%d,%s,a0' % (q, 'zt%d' % (q % 4) if q < 4 else 't%d' % q) for q in range(6)]
    cases = [('expomf_c1_k20', (1000, 1000, 20), [], 20),
             ('expomf_e_k64', (300, 150, 20), [], 64),
             ('expomf_f_k128', (180, 260, 30), [], 128),
             ('expomf_s_k20', (64, 64, 20), [], 20),                                 # small, top-3: every list stable (asserted here)
             ('expomf_sq_k20', (100, 300, 20), equalise(100, 300, 20), 20),          # m == n
             ('expomf_z_k20', (120, 200, 20), zlines, 20),                           # test-only users and items
             ('expomf_r_k30', (150, 48, 40), [], 30)]                                # few items: heavily repeated events
    for tag, ds, extra, k in cases:
        if not only or tag in only:
            case(tmp, tag, ds, extra, k, 2, topn='3' if tag == 'expomf_s_k20' else '5,10', must_be_stable=tag == 'expomf_s_k20')
    if not only or 'c2rows' in only:
        c2rows()
    if not only or 'trained' in only:
        trained()


if __name__ == '__main__':
    main()
