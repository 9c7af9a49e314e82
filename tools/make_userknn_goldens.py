#!/usr/bin/env python3
"""Generate tests/golden/g11_userknn_* by running the REFERENCE's own UserKNN class (recommender/cf/UserKNN.py).

Only runs where the reference tree exists (the helpers of tools/make_goldens.py are imported, which loads it).  Nothing
from the reference is copied: the fixtures are inputs (our synthetic logs, tests/helpers/numpy_userknn.py: write_case_log)
and what the reference computes from them.

How the reference is driven: config/UserKNN.conf with record / num.neighbors / item.ranking / output.setup changed and
-sample dropped.  initModel's printed lines are kept as printed.  predict's (item, score) list is taken from the module's
call of ``sorted`` (a spy bound as the module global, which Python resolves before the builtin): the reference returns
the names only.  evalRanking runs as it is; its lists file and measure strings are the pinned output.
"""
import builtins
import glob
import json
import os
import sys
import tempfile
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'tests'))

import make_goldens as mg                                       # noqa: E402  (puts the reference on sys.path)
from helpers.numpy_userknn import CASES, write_case_log         # noqa: E402

SAMPLE = 40          # users whose predict lists are pinned


def conf_for(tmp, tag, log_path):
    c = CASES[tag]
    out = []
    for ln in open(os.path.join(mg.REF, 'config/UserKNN.conf')).read().splitlines():
        key = ln.split('=')[0]
        if key == 'record':
            ln = 'record=' + log_path
        elif key == 'num.neighbors':
            ln = 'num.neighbors=%d' % c['K']
        elif key == 'evaluation.setup':
            ln = 'evaluation.setup=-target track -byTime 0.2'
        elif key == 'item.ranking':
            ln = 'item.ranking=-topN ' + c['topN']
        elif key == 'output.setup':
            ln = 'output.setup=on -dir ' + os.path.join(tmp, 'results_' + tag) + '/'
        out.append(ln)
    path = os.path.join(tmp, tag + '.conf')
    open(path, 'w').write('\n'.join(out) + '\n')
    return path


def case(tmp, tag):
    import recommender.cf.UserKNN as knn_mod
    log_path = os.path.join(tmp, tag + '.txt')
    write_case_log(tag, log_path)
    conf = mg.Config(conf_for(tmp, tag, log_path))
    rec, _ = mg.quiet(knn_mod.UserKNN, conf, mg.load_train(conf), [])
    rec.readConfiguration()
    _, cfg_out = mg.quiet(rec.printAlgorConfig)
    t0 = time.time()
    _, init_out = mg.quiet(rec.initModel)
    ref_s = time.time() - t0
    d, rt = rec.data, rec.recType
    ev_u, ev_i = mg.record_arrays(rec)
    K = CASES[tag]['K']
    m = d.getSize('user')
    nbr = np.full((m, K), -1, np.int32)
    sim = np.zeros((m, K), np.float64)
    for user, lst in rec.topUsers.items():
        pos = [(d.getId(v, 'user'), s) for v, s in lst if s > 0]
        u = d.getId(user, 'user')
        nbr[u, :len(pos)] = [p[0] for p in pos]
        sim[u, :len(pos)] = [p[1] for p in pos]
    # predict of sampled training users, with the scores the reference sorted
    calls = []

    def spy(seq, *a, **kw):
        calls.append(list(seq))
        return builtins.sorted(seq, *a, **kw)
    knn_mod.sorted = spy
    users = list(d.userRecord.keys())
    rng = np.random.RandomState(11)
    sample = sorted(set(rng.choice(len(users), min(SAMPLE, len(users)), replace=False).tolist()) | {0, len(users) - 1})
    p_users, p_ptr, p_items, p_scores = [], [0], [], []
    try:
        for t in sample:
            del calls[:]
            names = rec.predict(users[t])
            scored = dict(calls[-1]) if calls else {}
            p_users.append(d.getId(users[t], 'user'))
            p_items += [d.getId(x, rt) for x in names]
            p_scores += [scored[x] for x in names]
            p_ptr.append(len(p_items))
    finally:
        del knn_mod.sorted
    _, eval_out = mg.quiet(rec.evalRanking)
    lists = open(glob.glob(os.path.join(tmp, 'results_' + tag, '*-top-*items*.txt'))[0]).read()
    np.savez_compressed(os.path.join(mg.OUT, 'g11_%s.npz' % tag), K=K, m=m, n=d.getSize(rt), ev_u=ev_u, ev_i=ev_i, nbr=nbr, sim=sim,
                        p_users=np.array(p_users, np.int32), p_ptr=np.array(p_ptr, np.int64), p_items=np.array(p_items, np.int32),
                        p_scores=np.array(p_scores, np.float64))
    json.dump({'shape': CASES[tag]['shape'], 'K': K, 'topN': CASES[tag]['topN'],
               'config_lines': cfg_out.splitlines()[-3:], 'init_lines': init_out.splitlines(),
               'progress_lines': [ln for ln in eval_out.splitlines() if 'progress:' in ln],
               'lists': lists, 'measure': rec.measure, 'reference_seconds': ref_s},
              open(os.path.join(mg.OUT, 'g11_%s.json' % tag), 'w'), indent=1)
    print('%-16s m=%d n=%d K=%d: %d test users, reference initModel %.2f s' % (tag, m, d.getSize(rt), K, len(d.testSet), ref_s))


def main():
    os.makedirs(mg.OUT, exist_ok=True)
    tmp = tempfile.mkdtemp(prefix='yue_gold_userknn_')
    for tag in CASES:
        case(tmp, tag)


if __name__ == '__main__':
    main()
