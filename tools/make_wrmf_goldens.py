#!/usr/bin/env python3
"""Generate tests/golden/g10_wrmf_* by running the REFERENCE's own WRMF class (recommender/cf/WRMF.py).

Only runs where the reference tree exists (the helpers of tools/make_goldens.py are imported, which loads it).  Nothing
from the reference is copied: the fixtures are inputs (seeds, our synthetic logs) and what the reference computes from them.

How the reference is driven: config/WRMF.conf with record / num.factors / num.max.iter / reg.lambda -u / item.ranking /
output.setup changed and -sample dropped (evalRanking's lists are the pinned output); NumPy and ``random`` seeded here.
buildModel runs with num.max.iter = 1 once per iteration so that X and Y can be taken after every iteration (its
state lives in self.X / self.Y, and the loss restarts at 0 every iteration: the same computation as one call with
num.max.iter = iters); its printed line is renumbered to the iteration it belongs to.  The bound of every case is measured
here: the device contract (tests/helpers/numpy_wrmf.py: wrmf_half_sweep_contract, iterated) against the reference's X, Y.
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
from helpers.numpy_wrmf import pairs_from_events, wrmf_half_sweep_contract   # noqa: E402

SEED = 20260010


def conf_for(tmp, log_path, k, iters, reg, topn):
    out = []
    for ln in open(os.path.join(mg.REF, 'config/WRMF.conf')).read().splitlines():
        key = ln.split('=')[0]
        if key == 'record':
            ln = 'record=' + log_path
        elif key == 'num.factors':
            ln = 'num.factors=%d' % k
        elif key == 'num.max.iter':
            ln = 'num.max.iter=%d' % iters
        elif key == 'reg.lambda':
            ln = 'reg.lambda=-u %s -i 0.1 -b 0.2 -s 0.2' % reg
        elif key == 'evaluation.setup':
            ln = 'evaluation.setup=-target track -byTime 0.2'
        elif key == 'item.ranking':
            ln = 'item.ranking=-topN ' + topn
        elif key == 'output.setup':
            ln = 'output.setup=on -dir ' + os.path.join(tmp, 'results_wrmf') + '/'
        out.append(ln)
    path = os.path.join(tmp, 'wrmf_%d_%d_%s.conf' % (k, iters, reg))
    open(path, 'w').write('\n'.join(out) + '\n')
    return path


def contract_run(X0, Y0, ev_u, ev_i, iters, reg):
    """The device contract iterated on the CPU: (Xs, Ys, losses) after every iteration."""
    m, n = X0.shape[0], Y0.shape[0]
    (up, ui, uc), (ip, iu, ic) = pairs_from_events(ev_u, ev_i, m, n)
    X, Y = X0.copy(), Y0.copy()
    Xs, Ys, losses = [], [], []
    for _ in range(iters):
        Xn, loss = wrmf_half_sweep_contract(Y, up, ui, uc, reg, X_old=X)
        X = Xn
        Y, _ = wrmf_half_sweep_contract(X, ip, iu, ic, reg)
        Xs.append(X.copy())
        Ys.append(Y.copy())
        losses.append(loss)
    return Xs, Ys, losses


def rel(a, b):
    return float(np.abs(a.astype(np.float64) - b).max() / np.abs(b).max())


def case(tmp, tag, log_path, dataset, k, iters, reg, topn='5,10'):
    import recommender.cf.WRMF as wrmf_mod
    conf = mg.Config(conf_for(tmp, log_path, k, iters, reg, topn))
    rec, _ = mg.quiet(wrmf_mod.WRMF, conf, mg.load_train(conf), [])
    rec.readConfiguration()
    random.seed(SEED)
    np.random.seed(SEED)
    rec.initModel()
    X0, Y0 = rec.X.copy(), rec.Y.copy()
    rec.maxIter = 1
    Xs, Ys, lines = [], [], []
    t0 = time.time()
    for it in range(1, iters + 1):
        _, out = mg.quiet(rec.buildModel)
        line = [ln for ln in out.splitlines() if ln.startswith('iteration:')][0]
        lines.append(line.replace('iteration: 1 ', 'iteration: %d ' % it, 1))
        Xs.append(rec.X.copy())
        Ys.append(rec.Y.copy())
    ref_s = time.time() - t0
    d, rt = rec.data, rec.recType
    ev_u, ev_i = mg.record_arrays(rec)
    tu = list(d.testSet.keys())
    captured = {}
    orig = mg.Measure.rankingMeasure

    def spy(origin, res, N, itemCount):
        captured['res'] = {u: list(v) for u, v in res.items()}
        return orig(origin, res, N, itemCount)
    mg.Measure.rankingMeasure = staticmethod(spy)
    try:
        mg.quiet(rec.evalRanking)
    finally:
        mg.Measure.rankingMeasure = staticmethod(orig)
    ids = np.array([[d.getId(x, rt) for x in captured['res'][u]] for u in tu], np.int32)
    tuid = np.array([d.getId(u, 'user') for u in tu], np.int32)
    # the bound: the device contract against the reference, measured here
    cX, cY, closs = contract_run(X0, Y0, ev_u, ev_i, iters, float(reg))
    dev_x = max(rel(cX[t], Xs[t]) for t in range(iters))
    dev_y = max(rel(cY[t], Ys[t]) for t in range(iters))
    ref_loss = [float(ln.split('loss:')[1]) for ln in lines]
    dev_loss = max(abs(a - b) / abs(b) for a, b in zip(closs, ref_loss))
    m, n = X0.shape[0], Y0.shape[0]
    trained_u = np.zeros(m, bool)
    trained_u[ev_u] = True
    trained_i = np.zeros(n, bool)
    trained_i[ev_i] = True
    np.savez_compressed(os.path.join(mg.OUT, 'g10_%s.npz' % tag), seed=SEED, k=k, iters=iters, reg=np.float64(reg), m=m, n=n,
                        ev_u=ev_u, ev_i=ev_i, X0=X0, Y0=Y0, Xs=np.stack(Xs), Ys=np.stack(Ys), test_users=tuid, rec_ids=ids,
                        zero_users=np.flatnonzero(~trained_u).astype(np.int32), zero_items=np.flatnonzero(~trained_i).astype(np.int32))
    json.dump({'lines': lines, 'measure': rec.measure, 'dataset': dataset, 'topN': topn, 'reg': reg,
               'measured': {'contract_vs_reference_X': dev_x, 'contract_vs_reference_Y': dev_y, 'contract_vs_reference_loss': dev_loss,
                            'reference_seconds': ref_s}},
              open(os.path.join(mg.OUT, 'g10_%s.json' % tag), 'w'), indent=1)
    print('%-22s m=%d n=%d k=%d reg=%s: contract vs reference X %.2e Y %.2e loss %.2e (reference %.1f s)' % (tag, m, n, k, reg, dev_x, dev_y, dev_loss, ref_s))


def main():
    os.makedirs(mg.OUT, exist_ok=True)
    tmp = tempfile.mkdtemp(prefix='yue_gold_wrmf_')
    datasets = {'c1': (1000, 1000, 20), 'd3': (120, 200, 20)}
    logs = {}
    for name, (m, n, d) in datasets.items():
        logs[name] = os.path.join(tmp, name + '.txt')
        mg.synth.write_text_log(logs[name], m, n, d)
    # d3 plus six users with one late event each: int(1 * 0.8) = 0 training events, so the users and the four new items they
    # listen to are names of the test set only -> rows without training pairs (zero rows)
    logs['z'] = os.path.join(tmp, 'z.txt')
    with open(logs['z'], 'w') as f:
        f.write(open(logs['d3']).read())
        for q in range(6):
            f.write('9999999999,zu%d,%s,a0\n' % (q, 'zt%d' % (q % 4) if q < 4 else 't%d' % q))
    case(tmp, 'wrmf_c1_k20', logs['c1'], datasets['c1'], 20, 2, '1')
    case(tmp, 'wrmf_d3_k128', logs['d3'], datasets['d3'], 128, 2, '1')
    case(tmp, 'wrmf_d3_k128_reg001', logs['d3'], datasets['d3'], 128, 2, '0.01')
    case(tmp, 'wrmf_z_k64', logs['z'], list(datasets['d3']) + ['+6 test-only users, +4 test-only items'], 64, 2, '1')


if __name__ == '__main__':
    main()
