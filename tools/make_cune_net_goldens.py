#!/usr/bin/env python3
"""Generate tests/golden/g15_cune_* for CUNE's user-network stage (recommender/advanced/CUNE.py:34-118 of the REFERENCE).

Only runs where the reference tree exists (the helpers of tools/make_goldens.py are imported, which loads it); run with
PYTHONHASHSEED=0.  Nothing from the reference is copied: its text is read at run time, dedented and exec'd against a real
CUNE instance (empty module objects named gensim* satisfy its import; Word2Vec is never called); the fixtures are our
synthetic logs, a seeded W, and what the reference computes from them.

  g15_cune_net_c1.npz    the C1 log: CUNet of :39-52 as per-user (neighbour id, multiplicity) counts
  g15_cune_friends.npz   96 users, a seeded float32 W of dim 20 held in float64 as :87 leaves it, K = 10: topKSim of :88-95
                         (users iterated in id order) and the multiset IPositiveSet of :104-114
  g15_cune_quality.json  (--quality; needs no reference) the sequential contract's planted-groups scores over 5 seeds:
                         the yardstick of the device's embedding quality test
"""
import json
import os
import sys
import tempfile
import textwrap
import types
from collections import Counter

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(os.path.dirname(HERE), 'tests'))
OUT = os.path.join(os.path.dirname(HERE), 'tests', 'golden')


def quality():
    from helpers import numpy_cune_net as cn
    p = cn.PLANTED
    ev_u, ev_i, m, n, group = cn.planted_log()
    (up, ui), (ip, iu) = cn.pairs_from_events(ev_u, ev_i, m, n)
    net = cn.Net(up, ui, ip, iu)
    scores = {}
    for rw in (1, 64, 256):
        scores[rw] = []
        for seed in p['seeds']:
            w = cn.walks(net, p['T'], p['L'], seed)
            W = cn.embed(w, m, p['dim'], p['window'], p['epochs'], seed, round_walks=rw)
            ids, _ = cn.friends(W, net.users, p['K'])
            scores[rw].append(cn.planted_score(ids, group))
            print('round_walks %d seed %d: %.4f' % (rw, seed, scores[rw][-1]), flush=True)
    seq = np.array(scores[1])
    json.dump({'planted': p, 'sequential_scores': scores[1], 'mean': float(seq.mean()), 'std': float(seq.std(ddof=1)),
               'contract_round_walks_64_scores': scores[64], 'contract_round_walks_256_scores': scores[256]},
              open(os.path.join(OUT, 'g15_cune_quality.json'), 'w'), indent=1)


def reference():
    import make_goldens as mg
    from yue_amd import synth
    for name in ('gensim', 'gensim.models', 'gensim.models.word2vec'):
        sys.modules.setdefault(name, types.ModuleType(name))
    import recommender.advanced.CUNE as cune_mod
    src = open(os.path.join(mg.REF, 'recommender/advanced/CUNE.py')).read().splitlines()

    def text(first, before, name, ours=''):
        a = next(t for t, ln in enumerate(src) if first in ln)
        b = next(t for t, ln in enumerate(src) if before in ln and t > a)
        scope = dict(cune_mod.__dict__)
        exec('def %s(self):\n' % name + ours + textwrap.indent(textwrap.dedent('\n'.join(src[a:b])), '    '), scope)
        return scope[name]
    build_net = text('userListen = defaultdict(dict)', "print ('Generating random deep walks...')", 'build_net')      # :39-52
    top_k = text('for user1 in self.CUNet:', "print ('Similarity matrix finished.')", 'top_k', '    i = 0\n')       # :88-98 (the counter of :84)
    item_sets = text('self.PositiveSet = defaultdict(list)', "print ('Training...')", 'item_sets')                  # :104-114
    tmp = tempfile.mkdtemp(prefix='yue_gold_cnet_')

    def instance(tag, m, n, d, K):
        log = os.path.join(tmp, tag + '.txt')
        synth.write_text_log(log, m, n, d)
        out = []
        for ln in open(os.path.join(mg.REF, 'config/CUNE.conf')).read().splitlines():
            key = ln.split('=')[0]
            if key == 'record':
                ln = 'record=' + log
            elif key == 'CUNE':
                ln = 'CUNE=-T 20 -L 10 -l 20 -w 5 -k %d -s 2 -ep 10' % K
            elif key == 'output.setup':
                ln = 'output.setup=on -dir ' + os.path.join(tmp, 'results_' + tag) + '/'
            out.append(ln)
        path = os.path.join(tmp, tag + '.conf')
        open(path, 'w').write('\n'.join(out) + '\n')
        conf = mg.Config(path)
        rec, _ = mg.quiet(cune_mod.CUNE, conf, mg.load_train(conf), [])
        rec.readConfiguration()
        mg.quiet(build_net, rec)
        return rec

    # -- the network of the C1 log
    rec = instance('c1', 1000, 1000, 20, 50)
    d = rec.data
    m = d.getSize('user')
    ev_u, ev_i = mg.record_arrays(rec)
    ptr, nb, mult = [0], [], []
    rows = {d.getId(u, 'user'): Counter(d.getId(v, 'user') for v in lst) for u, lst in rec.CUNet.items()}
    for u in range(m):
        for v, c in sorted(rows.get(u, {}).items()):
            nb.append(v); mult.append(c)
        ptr.append(len(nb))
    assert max(mult) < 256 and m < 65536
    np.savez_compressed(os.path.join(OUT, 'g15_cune_net_c1.npz'), m=m, n=d.getSize(rec.recType), ev_u=ev_u, ev_i=ev_i,
                        ptr=np.array(ptr, np.int64), nb=np.array(nb, np.uint16), mult=np.array(mult, np.uint8))
    print('g15_cune_net_c1: %d users in the network, %d (neighbour, multiplicity) entries' % (len(rows), len(nb)))

    # -- friends and friends' items of a seeded W
    m, dim, K = 96, 20, 10
    rec = instance('f96', m, 200, 8, K)
    d = rec.data
    assert d.getSize('user') == m
    by_id = sorted(rec.CUNet, key=lambda u: d.getId(u, 'user'))
    rec.CUNet = {u: rec.CUNet[u] for u in by_id}                      # users iterate in id order
    W = np.random.RandomState(20260015).randn(m, dim).astype(np.float32)
    rec.W = W.astype(np.float64)
    rec.topKSim = {}
    mg.quiet(top_k, rec)
    mg.quiet(item_sets, rec)
    net = np.array([d.getId(u, 'user') for u in by_id], np.int32)
    ids = np.full((m, K), -1, np.int32)
    sims = np.zeros((m, K), np.float64)
    for user, lst in rec.topKSim.items():
        u = d.getId(user, 'user')
        ids[u, :len(lst)] = [d.getId(v, 'user') for v, _ in lst]
        sims[u, :len(lst)] = [s for _, s in lst]
    # no two adjacent cosines of a user's full ordered list closer than 1e-9 within its first K + 1 entries
    from helpers import numpy_cune_net as cn
    for a in net:
        full = sorted((cn.cosine(W[a], W[b]) for b in net if b != a), reverse=True)[:K + 1]
        assert min(np.diff(full[::-1])) > 1e-9, a
    ev_u, ev_i = mg.record_arrays(rec)
    ip_ptr, ip_items = [0], []
    rt = rec.recType
    for u in range(m):
        ip_items += sorted(d.getId(x, rt) for x in rec.IPositiveSet.get(d.id2name['user'][u], []))
        ip_ptr.append(len(ip_items))
    np.savez_compressed(os.path.join(OUT, 'g15_cune_friends.npz'), m=m, n=d.getSize(rt), K=K, W=W, net=net, ids=ids, sims=sims,
                        ev_u=ev_u, ev_i=ev_i, ip_ptr=np.array(ip_ptr, np.int64), ip_items=np.array(ip_items, np.int32))
    print('g15_cune_friends: %d network users, %d friends\' items' % (len(net), len(ip_items)))


if __name__ == '__main__':
    os.makedirs(OUT, exist_ok=True)
    if '--quality' in sys.argv:
        quality()
    else:
        reference()
