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
  g15_cune_trained.npz/.json  (--trained; needs no reference) grouped walks on which the contract's logits reach |f| >= 4
                         with no |f| >= 6 cut-off: the walks, the float64 W, the float32 / float64 gap and the statistics
  g15_cune_cutoff.npz/.json   (--trained, only where the search finds a qualifying run) the same with the cut-off taken at
                         the same events in float32 and float64, every |f| at least 1000 float32 / float64 differences
                         away from 6; g15_cune_cutoff_search.json is the log of the search either way
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


# ---- --trained: the embedding where the sigmoid is not linear (tests/test_gpu_cnet_edges.py) ----
EMB_SEED = 3
TRAINED = {'m': 64, 'groups': 2, 'nw': 64, 'L': 64, 'dim': 20, 'window': 5, 'negative': 5, 'round_walks': 8, 'walk_seed': 20260016}
CUTOFF = {'m': 64, 'groups': 4, 'nw': 128, 'L': 64, 'dim': 8, 'window': 5, 'negative': 5, 'round_walks': 8}
CUTOFF_CANDIDATES = [(ep, seed) for seed in (20260017, 20260018, 20260019, 20260020) for ep in (28, 30, 32, 33, 34)]   # 20
CUTOFF_MARGIN = 1000.0


def grouped_walks(p, seed):
    """int32 [nw, L]: walk w stays inside group w % groups (ids group * size .. + size), ids uniform from the seed."""
    size = p['m'] // p['groups']
    rng = np.random.RandomState(seed)
    return ((np.arange(p['nw']) % p['groups'])[:, None] * size + rng.randint(0, size, (p['nw'], p['L']))).astype(np.int32)


def contract_run(args):
    p, walk_seed, epochs, dtype, keep_f = args
    from helpers import numpy_cune_net as cn
    stats = {'f': []} if keep_f else {}
    W = cn.embed(grouped_walks(p, walk_seed), p['m'], p['dim'], p['window'], epochs, EMB_SEED, negative=p['negative'],
                 round_walks=p['round_walks'], dtype=np.float32 if dtype == 'float32' else np.float64, stats=stats)
    for key in ('kept', 'trained', 'targets'):
        del stats[key]
    if keep_f:
        stats['f'] = np.array(stats['f'], np.float64)
    return W, stats


def save_npz(name, **arrays):
    """np.savez_compressed with fixed member dates: the same arrays give the same bytes."""
    import io
    import zipfile
    with zipfile.ZipFile(os.path.join(OUT, name), 'w', zipfile.ZIP_DEFLATED) as z:
        for key, val in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(val), allow_pickle=False)
            z.writestr(zipfile.ZipInfo(key + '.npy', (1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)


def save_json(name, obj):
    with open(os.path.join(OUT, name), 'w') as f:
        json.dump(obj, f, indent=1, sort_keys=True)
        f.write('\n')


def summary(p, walk_seed, epochs, w32, s32, w64, s64):
    return dict(p, walk_seed=walk_seed, embed_seed=EMB_SEED, epochs=epochs, evals=s64['evals'],
                gap=float(np.abs(w32.astype(np.float64) - w64).max()), max_abs_w=float(np.abs(w64).max()),
                max_abs_f={'float32': s32['max_abs_f'], 'float64': s64['max_abs_f']},
                cutoffs={'float32': s32['cutoffs'], 'float64': s64['cutoffs']})


def trained(pool):
    p = {k: v for k, v in TRAINED.items() if k != 'walk_seed'}
    seed = TRAINED['walk_seed']
    counts = list(range(60, 0, -10))
    runs = pool.map(contract_run, [(p, seed, ep, 'float64', False) for ep in counts])
    epochs = None
    for ep, (_, st) in zip(counts, runs):                            # from 60 downwards: the smallest count that keeps |f| >= 4
        print('trained: %d epochs float64: largest |f| %.4f, %d cut-offs of %d' % (ep, st['max_abs_f'], st['cutoffs'], st['evals']), flush=True)
        if st['max_abs_f'] < 4.0:
            break
        epochs = ep
    assert epochs is not None, 'no epoch count up to 60 reaches |f| >= 4'
    w64, s64 = runs[counts.index(epochs)]
    w32, s32 = contract_run((p, seed, epochs, 'float32', False))
    out = summary(p, seed, epochs, w32, s32, w64, s64)
    print('trained:', out, flush=True)
    assert min(out['max_abs_f'].values()) >= 4.0 and max(out['cutoffs'].values()) == 0 and out['gap'] > 0
    save_npz('g15_cune_trained.npz', walks=grouped_walks(p, seed), W=w64)
    save_json('g15_cune_trained.json', out)


def cutoff_candidate(args):
    p, epochs, seed = args
    w64, s64 = contract_run((p, seed, epochs, 'float64', True))
    log = {'epochs': epochs, 'walk_seed': seed, 'evals': s64['evals'], 'cutoffs_float64': s64['cutoffs'], 'max_abs_f_float64': s64['max_abs_f'],
           'min_distance_to_6_float64': float(np.abs(np.abs(s64['f']) - 6.0).min())}
    if s64['cutoffs'] < 8:
        return dict(log, verdict='fewer than 8 cut-offs'), None
    if log['min_distance_to_6_float64'] < CUTOFF_MARGIN * 2.0 ** -24:    # no float32 run can be 1000 differences away
        return dict(log, verdict='float64 |f| within 1000 x 2^-24 of 6'), None
    w32, s32 = contract_run((p, seed, epochs, 'float32', True))
    diff = float(np.abs(s32['f'] - s64['f']).max())
    dist = float(min(np.abs(np.abs(s32['f']) - 6.0).min(), log['min_distance_to_6_float64']))
    same = s32['cutoff_events'] == s64['cutoff_events']
    log.update(cutoffs_float32=s32['cutoffs'], max_abs_f_float32=s32['max_abs_f'], same_events=same, max_f_difference=diff, min_distance_to_6=dist)
    if not same:
        return dict(log, verdict='float32 and float64 cut off at different events'), None
    if dist < CUTOFF_MARGIN * diff:
        return dict(log, verdict='an |f| is closer to 6 than 1000 x the largest float32 / float64 difference'), None
    out = summary(p, seed, epochs, w32, s32, w64, s64)
    out.update(max_f_difference=diff, min_distance_to_6=dist, cutoff_events=[list(e) for e in s64['cutoff_events']])
    return dict(log, verdict='qualifies'), (out, w64)


def cutoff(pool):
    p = CUTOFF
    assert len(CUTOFF_CANDIDATES) <= 20
    results = pool.map(cutoff_candidate, [(p, ep, seed) for ep, seed in CUTOFF_CANDIDATES], chunksize=1)
    for log, _ in results:
        print('cutoff:', log, flush=True)
    save_json('g15_cune_cutoff_search.json', {'input': p, 'margin': CUTOFF_MARGIN, 'tried': [log for log, _ in results]})
    found = next((hit for _, hit in results if hit is not None), None)   # the first in candidate order
    if found is None:
        print('cutoff: no candidate qualifies; no g15_cune_cutoff fixture')
        return
    out, w64 = found
    save_npz('g15_cune_cutoff.npz', walks=grouped_walks(p, out['walk_seed']), W=w64)
    save_json('g15_cune_cutoff.json', out)
    print('cutoff: committed', {k: v for k, v in out.items() if k != 'cutoff_events'})


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
    elif '--trained' in sys.argv:
        import multiprocessing
        with multiprocessing.Pool(min(8, os.cpu_count() or 1)) as workers:
            if '--cutoff-only' not in sys.argv:
                trained(workers)
            cutoff(workers)
    else:
        reference()
