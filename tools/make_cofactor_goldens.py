#!/usr/bin/env python3
"""Generate tests/golden/g14_cofactor_* by running the REFERENCE's own CoFactor class (recommender/advanced/CoFactor.py).

Only runs where the reference tree exists (the helpers of tools/make_goldens.py are imported, which loads it).  Nothing
from the reference is copied: the fixtures are inputs (seeds, options, our synthetic logs) and what the reference computes
from them.

How the reference is driven: config/CoFactor.conf with record / record.setup / evaluation.setup (-byTime 0.2, the split the
other fixtures use) / num.factors / num.max.iter / reg.lambda -u / CoFactor / item.ranking / output.setup changed.  The class
reads self.n and self.m in initModel, which nothing sets: the tool sets those two attributes on the instance.  The
co-occurrence counts are a local of initModel: a profile hook takes them from its frame when it returns.  buildModel
re-initialises X, Y, G, w, c on every call, so the state after iteration t comes from a fresh call with maxIter = t after
np.random is put back to the state it had after initModel; w0, c0, G0 are the three draws repeated from that state (and the
whole initial state is reproduced from the seed alone by tests/helpers/numpy_cofactor.py: init_from_seed, asserted here).
evalRanking calls predict(), which the class does not override: the lists as shipped (rec_ids_shipped) come from the untrained
P and Q; binding the class's predictForRanking to predict on the instance gives rec_ids, the lists the device is compared with.

Per case the tool measures the CPU contract (tests/helpers/numpy_cofactor.py, iterated from the same start) against the
reference for X, Y, G, w, c and the loss ('measured' in the json; the tests allow four times these).  A test user's list is
stable when no two scores the overwrite-scan compared are closer than the score error of a device as far from the reference as
the contract is, times 4 (numpy_expomf.score_error); every case must keep 90 % of its test users stable, or the tool fails.
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
from helpers import numpy_cofactor as nc                        # noqa: E402
from helpers import numpy_expomf as ne                          # noqa: E402
from helpers.numpy_wrmf import pairs_from_events                # noqa: E402

SEED = 20260014


def conf_for(tmp, tag, log_path, k, iters, reg, neg, gamma, filt, topn):
    out = []
    for ln in open(os.path.join(mg.REF, 'config/CoFactor.conf')).read().splitlines():
        key = ln.split('=')[0]
        if key == 'record':
            ln = 'record=' + log_path
        elif key == 'record.setup':
            ln = 'record.setup=-columns user:1,track:2,artist:3,time:0 -delim ,'
        elif key == 'evaluation.setup':
            ln = 'evaluation.setup=-target track -byTime 0.2'
        elif key == 'num.factors':
            ln = 'num.factors=%d' % k
        elif key == 'num.max.iter':
            ln = 'num.max.iter=%d' % iters
        elif key == 'reg.lambda':
            ln = 'reg.lambda=-u %s -i 0.01 -b 0.01 -s 0.1' % reg
        elif key == 'CoFactor':
            ln = 'CoFactor=-k %d -gamma %s -filter %d' % (neg, gamma, filt)
        elif key == 'item.ranking':
            ln = 'item.ranking=-topN ' + topn
        elif key == 'output.setup':
            ln = 'output.setup=on -dir ' + os.path.join(tmp, 'results_cofactor') + '/'
        out.append(ln)
    path = os.path.join(tmp, 'cofactor_%s.conf' % tag)
    open(path, 'w').write('\n'.join(out) + '\n')
    return path


def locals_at_return(fn, code, *names):
    """Runs fn(); returns the named locals of the frame running `code` as they were when it returned."""
    got = {}

    def hook(frame, event, arg):
        if event == 'return' and frame.f_code is code:
            for nm in names:
                got[nm] = frame.f_locals[nm]
    sys.setprofile(hook)
    try:
        fn()
    finally:
        sys.setprofile(None)
    return got


def csr_of(rows, n, dtype):
    """dict id -> dict id -> value  ->  (ptr, idx ascending, val)"""
    ptr = np.zeros(n + 1, np.int64)
    idx, val = [], []
    for i in range(n):
        row = sorted(rows.get(i, {}).items())
        ptr[i + 1] = ptr[i] + len(row)
        idx += [j for j, _ in row]
        val += [v for _, v in row]
    return ptr, np.array(idx, np.int32), np.array(val, dtype)


def case(tmp, tag, dataset, extra_lines, k, reg, neg, gamma, filt, iters=2, topn='5,10'):
    import recommender.advanced.CoFactor as cf
    m0, n0, d0 = dataset
    log_path = os.path.join(tmp, tag + '.txt')
    mg.synth.write_text_log(log_path, m0, n0, d0)
    with open(log_path, 'a') as f:
        for ln in extra_lines:
            f.write(ln + '\n')
    conf = mg.Config(conf_for(tmp, tag, log_path, k, iters, reg, neg, gamma, filt, topn))
    rec, _ = mg.quiet(cf.CoFactor, conf, mg.load_train(conf), [])
    rec.readConfiguration()
    assert rec.negCount == neg and rec.regR == float(gamma) and rec.filter == filt
    d_, rt = rec.data, rec.recType
    rec.m = d_.getSize('user')
    rec.n = d_.getSize(rt)
    m, n = rec.m, rec.n
    random.seed(SEED)
    np.random.seed(SEED)
    t0 = time.time()
    got = locals_at_return(lambda: mg.quiet(rec.initModel), cf.CoFactor.initModel.__code__, 'occurrence')
    init_s = time.time() - t0
    gid = lambda name: d_.getId(name, rt)                       # noqa: E731
    co = csr_of({gid(a): {gid(b): v for b, v in row.items()} for a, row in got['occurrence'].items()}, n, np.int32)
    sp = csr_of({gid(a): {gid(b): v for b, v in row.items()} for a, row in rec.SPPMI.items()}, n, np.float64)
    state = np.random.get_state()
    w0, c0, G0 = np.random.rand(n) / 10, np.random.rand(n) / 10, np.random.rand(n, k) / 10
    X0, Y0 = rec.P * 10, rec.Q * 10
    for a, b in zip((X0, Y0, G0, w0, c0), nc.init_from_seed(SEED, m, n, k)):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    Xs, Ys, Gs, ws, cs, lines = [], [], [], [], [], []
    iter_s = 0.0
    for t in range(1, iters + 1):
        np.random.set_state(state)
        rec.maxIter = t
        t0 = time.time()
        _, out = mg.quiet(rec.buildModel)
        iter_s = (time.time() - t0) / t
        got_lines = out.splitlines()
        assert got_lines[0] == 'training...' and len(got_lines) == t + 1
        assert not lines or got_lines[1:t] == lines             # the earlier iterations repeat exactly
        lines = got_lines[1:]
        Xs.append(rec.X.copy()); Ys.append(rec.Y.copy()); Gs.append(rec.G.copy()); ws.append(rec.w.copy()); cs.append(rec.c.copy())
    assert Xs[-1].dtype == np.float32 and Ys[-1].dtype == np.float32 and Gs[-1].dtype == np.float64 and ws[-1].dtype == np.float64
    ev_u, ev_i = mg.record_arrays(rec)
    um, im = pairs_from_events(ev_u, ev_i, m, n)
    # the contract's graph equals the reference's bit for bit
    cco = nc.cooccur_from_pairs(im[0], im[1], im[2], m, filt)
    csp = nc.sppmi_from_cooccur(cco[0], cco[1], cco[2], neg)
    for a, b in zip(co + sp, cco + csp):
        assert a.dtype == b.dtype and np.array_equal(a, b), tag
    # lists
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
    ids_shipped, measure_shipped = ranked()
    rec.predict = rec.predictForRanking
    ids, measure = ranked()
    tuid = np.array([d_.getId(u, 'user') for u in tu], np.int32)
    # measured: the contract iterated from the same start against the reference, the largest over the iterations
    X, Y, G, w, c = X0, Y0, G0, w0, c0
    meas = {key: 0.0 for key in ('X', 'Y', 'G', 'w', 'c', 'loss')}
    ref_loss = [float(ln.split('loss:')[1]) for ln in lines]
    for t in range(iters):
        X, Y, G, w, c, loss = nc.iteration(X, Y, G, w, c, um, im, sp, float(reg), float(gamma))
        now = {'X': nc.rel(X, Xs[t]), 'Y': nc.rel(Y, Ys[t]), 'G': nc.rel(G, Gs[t]), 'w': nc.rel(w, ws[t]), 'c': nc.rel(c, cs[t]),
               'loss': abs(loss - ref_loss[t]) / abs(ref_loss[t])}
        for key in meas:
            meas[key] = max(meas[key], now[key])
    N = max(int(x) for x in topn.split(','))
    stable = np.zeros(len(tu), bool)
    for t, u in enumerate(tuid):
        scores = Ys[-1].dot(Xs[-1][u])
        masked = set(int(i) for i in um[1][um[0][u]:um[0][u + 1]])
        mine, margin = ne.overwrite_scan(scores, masked, N, ne.score_error(Xs[-1], Ys[-1], X, Y, u))
        assert mine == [int(x) for x in ids[t]], (tag, u)
        stable[t] = margin > 0
    level = nc.levels_of(sp[0], sp[1])
    print('%-10s m=%d n=%d k=%d: cooccur %d sppmi %d levels %d; contract vs reference %s; stable %d/%d (reference init %.1f s, iteration %.1f s)'
          % (tag, m, n, k, co[0][-1], sp[0][-1], level.max() + 1, ' '.join('%s %.1e' % kv for kv in meas.items()), stable.sum(), len(tu), init_s, iter_s))
    assert stable.sum() >= 0.9 * len(tu), '%s: only %d of %d lists are stable' % (tag, stable.sum(), len(tu))
    assert stable.all() or tag != 's_k20', 's_k20: %d of %d lists are not stable' % ((~stable).sum(), len(tu))
    trained_u = np.zeros(m, bool)
    trained_u[ev_u] = True
    trained_i = np.zeros(n, bool)
    trained_i[ev_i] = True
    small = np.int16 if max(m, n) < 32768 else np.int32
    np.savez_compressed(os.path.join(mg.OUT, 'g14_cofactor_%s.npz' % tag), seed=SEED, k=k, iters=iters, m=m, n=n, neg=neg, filter=filt,
                        regU=np.float64(reg), regR=np.float64(gamma), ev_u=ev_u.astype(small), ev_i=ev_i.astype(small),
                        co_ptr=co[0].astype(np.int32), co_idx=co[1].astype(small), co_cnt=co[2].astype(small),
                        sp_ptr=sp[0].astype(np.int32), sp_idx=sp[1].astype(small), sp_val=sp[2],
                        test_users=tuid, rec_ids=ids, rec_ids_shipped=ids_shipped, stable_users=stable,
                        zero_users=np.flatnonzero(~trained_u).astype(np.int32), zero_items=np.flatnonzero(~trained_i).astype(np.int32))
    np.savez_compressed(os.path.join(mg.OUT, 'g14_cofactor_%s_states.npz' % tag), Xs=np.stack(Xs), Ys=np.stack(Ys), Gs=np.stack(Gs),
                        ws=np.stack(ws), cs=np.stack(cs))
    json.dump({'lines': ['training...'] + lines, 'measure': measure, 'measure_shipped': measure_shipped, 'dataset': list(dataset),
               'append': list(extra_lines), 'topN': topn, 'options': {'k': neg, 'gamma': gamma, 'filter': filt, 'regU': reg},
               'measured': {'contract_vs_reference_' + key: v for key, v in meas.items()},
               'cooccur_nnz': int(co[0][-1]), 'sppmi_nnz': int(sp[0][-1]), 'levels': int(level.max()) + 1,
               'stable_users': int(stable.sum()), 'test_users': len(tu),
               'reference_seconds': {'initModel': init_s, 'iteration': iter_s}},
              open(os.path.join(mg.OUT, 'g14_cofactor_%s.json' % tag), 'w'), indent=1)


def main():
    os.makedirs(mg.OUT, exist_ok=True)
    tmp = tempfile.mkdtemp(prefix='yue_gold_cofactor_')
    only = sys.argv[1:]
    zlines = ['9999999999,zu%d,%s,a0' % (q, 'zt%d' % (q % 4) if q < 4 else 't%d' % q) for q in range(6)]
    #        tag        dataset           appended  k    regU  neg gamma  filter topN
    cases = [('c1_k20', (1000, 1000, 20), [],       20,  '1',  1, '1',    2, '5,10'),
             ('d3_k128', (120, 200, 20),  [],       128, '1',  1, '1',    1, '3'),          # m < k: X^T X is singular, the widest deviation; top-3 keeps 90 % of the lists stable
             ('d3_k64_g003', (120, 200, 20), [],    64,  '1',  5, '0.03', 1, '5,10'),     # neg and gamma of the reference's own configuration
             ('z_k64', (120, 200, 20),    zlines,   64,  '1',  1, '1',    0, '3,5'),      # test-only users and items, filter 0
             ('s_k20', (64, 64, 20),      [],       20,  '1',  1, '1',    1, '3')]          # small, top-3: every list stable (asserted here), so the measure strings are pinned
    for tag, ds, extra, k, reg, neg, gamma, filt, topn in cases:
        if not only or tag in only:
            case(tmp, tag, ds, extra, k, reg, neg, gamma, filt, topn=topn)


if __name__ == '__main__':
    main()
