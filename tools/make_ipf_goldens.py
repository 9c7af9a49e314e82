#!/usr/bin/env python3
"""Generate tests/golden/g12_ipf_* by running the REFERENCE's own IPF class (recommender/cf/IPF.py).

Only runs where the reference tree exists (the helpers of tools/make_goldens.py are imported, which loads it).  Nothing
from the reference is copied: the fixtures are inputs (our synthetic logs, tests/helpers/numpy_ipf.py: write_case_log)
and what the reference computes from them.

How the reference is driven: config/IPF.conf with record / evaluation.setup / item.ranking / IPF / output.setup changed.
initModel's printed lines are kept as printed.  predict's (item, score) list is taken from the module's call of
``sorted`` (a spy bound as the module global, which Python resolves before the builtin): its input is the rank dict's
items in insertion order, its output the order the reference returns.  evalRanking runs as it is; its progress lines,
lists file and measure strings are the pinned output.
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
from helpers.numpy_ipf import CASES, write_case_log             # noqa: E402

SAMPLE = 30          # users whose predict lists are pinned


def conf_for(tmp, tag, log_path, test_path):
    c = CASES[tag]
    out = []
    for ln in open(os.path.join(mg.REF, 'config/IPF.conf')).read().splitlines():
        key = ln.split('=')[0]
        if key == 'record':
            ln = 'record=' + log_path
        elif key == 'evaluation.setup':
            ln = 'evaluation.setup=' + c['eval'].format(test=test_path)
        elif key == 'item.ranking':
            ln = 'item.ranking=-topN ' + c['topN']
        elif key == 'IPF':
            ln = 'IPF=' + c['ipf']
        elif key == 'output.setup':
            ln = 'output.setup=on -dir ' + os.path.join(tmp, 'results_' + tag) + '/'
        out.append(ln)
    path = os.path.join(tmp, tag + '.conf')
    open(path, 'w').write('\n'.join(out) + '\n')
    return path


def case(tmp, tag):
    import recommender.cf.IPF as ipf_mod
    from tool.config import LineConfig
    from tool.file import FileIO
    log_path = os.path.join(tmp, tag + '.txt')
    test_path = write_case_log(tag, log_path)
    conf = mg.Config(conf_for(tmp, tag, log_path, test_path))
    test = []
    if test_path:
        setup = LineConfig(conf['record.setup'])
        cols = dict((a, int(b)) for a, b in (c.split(':') for c in setup['-columns'].split(',')))
        test, _ = mg.quiet(FileIO.loadDataSet, test_path, columns=cols, delim=setup['-delim'])
    rec, _ = mg.quiet(ipf_mod.IPF, conf, mg.load_train(conf), test)
    rec.readConfiguration()
    _, init_out = mg.quiet(rec.initModel)
    d, rt = rec.data, rec.recType
    ev_u, ev_i = mg.record_arrays(rec)
    m, n = d.getSize('user'), d.getSize(rt)
    hu = [[d.getId(b, 'user') for b in d.listened[rt][d.id2name[rt][c]]] if d.id2name[rt][c] in d.listened[rt] else []
          for c in range(n)]
    calls = []

    def spy(seq, *a, **kw):
        calls.append(list(seq))
        return builtins.sorted(seq, *a, **kw)
    ipf_mod.sorted = spy
    users = list(d.userRecord.keys())
    rng = np.random.RandomState(12)
    sample = sorted(set(rng.choice(len(users), min(SAMPLE, len(users)), replace=False).tolist()) | {0, len(users) - 1})
    if tag == 'ipf_z':
        sample = sorted(set(sample) | {users.index(x) for x in ('iso', 'one', 'rep')})
    p_users, p_ptr, p_items, p_scores = [], [0], [], []
    t0 = time.time()
    try:
        for t in sample:
            del calls[:]
            names = rec.predict(users[t])
            scored = dict(calls[-1])
            assert [x for x, _ in builtins.sorted(calls[-1], key=lambda e: e[1], reverse=True)] == names
            p_users.append(d.getId(users[t], 'user'))
            p_items += [d.getId(x, rt) for x in names]
            p_scores += [scored[x] for x in names]
            p_ptr.append(len(p_items))
    finally:
        del ipf_mod.sorted
    per_user = (time.time() - t0) / len(sample)
    _, eval_out = mg.quiet(rec.evalRanking)
    lists = open(glob.glob(os.path.join(tmp, 'results_' + tag, '*-top-*items*.txt'))[0]).read()
    np.savez_compressed(os.path.join(mg.OUT, 'g12_%s.npz' % tag), m=m, n=n, ev_u=ev_u, ev_i=ev_i,
                        hu_ptr=np.concatenate([[0], np.cumsum([len(r) for r in hu])]).astype(np.int64),
                        hu_users=np.array([b for r in hu for b in r], np.int32),
                        p_users=np.array(p_users, np.int32), p_ptr=np.array(p_ptr, np.int64), p_items=np.array(p_items, np.int32),
                        p_scores=np.array(p_scores, np.float64))
    json.dump({'shape': CASES[tag]['shape'], 'ipf': CASES[tag]['ipf'], 'eval': CASES[tag]['eval'], 'topN': CASES[tag]['topN'],
               'rho': rec.rho, 'beta': rec.beta, 'eta': rec.eta, 'init_lines': init_out.splitlines(),
               'progress_lines': [ln for ln in eval_out.splitlines() if 'progress:' in ln],
               'lists': lists, 'measure': rec.measure, 'reference_seconds_per_predict': per_user},
              open(os.path.join(mg.OUT, 'g12_%s.json' % tag), 'w'), indent=1)
    print('%-10s m=%d n=%d: %d test users, reference predict %.1f ms per user' % (tag, m, n, len(d.testSet), 1e3 * per_user))


def main():
    os.makedirs(mg.OUT, exist_ok=True)
    tmp = tempfile.mkdtemp(prefix='yue_gold_ipf_')
    for tag in (sys.argv[1:] or CASES):
        case(tmp, tag)


if __name__ == '__main__':
    main()
