"""The end-to-end NGCF problems shared by tests/test_ngcf_golden.py (which checks on the CPU that the seeds leave the float32
contract alone inside the rule) and tests/test_gpu_ngcf_plugin.py (which runs Yue(conf).execute() on the device).

A problem is a yue_amd.synth text log behind config/NGCF.conf.  Its yardstick is the fp64 contract trained from the plugin's own
start values (U, V, the six weights), on the plugin's own batches and the contract's masks of the plugin's seed, then
propagated once without dropout: F.  Lists, the rule that decides which users are compared and the 5 % cap are those of
tests/helpers/lightgcn_e2e.py.

How many steps.  The rule holds for the first few Adam steps only, so the problems train for one epoch of 1 and of 3 batches.
l2_normalize's derivative on rows of size 0.005 gives gradients of order 10, Adam's first steps move every element by about lr
whatever its size, lr = 0.003 is as large as the start values, and one flipped sign of Z is a jump: float32 training leaves
fp64 quickly.  tools/ngcf_e2e_drift.py prints, per number of steps, the float32 contract's distance from fp64 and the users
the rule leaves out (measured: within the cap after 1 to 3 steps, all of 150 users out after 30 steps at k 32).
"""
import os
import random

import numpy as np

from . import numpy_ngcf as ng
from .lightgcn_e2e import ROOT, compared_users, oracle_lists, ranked_users  # noqa: F401

# name -> (synth users, items, events per user, synth seed, seed of the start values and the sampler, num.factors, epochs,
#          batch_size, the ngcf.hip line)
PROBLEMS = {
    'written': (150, 400, 12, 20260003, 22, 64, 1, 2048, '-layers 3 -keep 0.9 -graph written'),
    'symmetric_layers2': (200, 150, 6, 20260007, 13, 64, 1, 512, '-graph symmetric -layers 2'),
}


def config(tmp_path, name):
    from yue_amd import synth
    from yue_amd.tool.config import Config
    m, n, d, log_seed, seed, k, iters, batch, line = PROBLEMS[name]
    log = tmp_path / ('%s.txt' % name)
    synth.write_text_log(str(log), m, n, d, seed=log_seed)
    text = open(os.path.join(ROOT, 'config', 'NGCF.conf')).read()
    for old, new in (('record=./dataset/log.txt', 'record=%s' % log), ('num.max.iter=100', 'num.max.iter=%d' % iters),
                     ('batch_size=16', 'batch_size=%d' % batch), ('num.factors=64', 'num.factors=%d' % k),
                     ('output.setup=on -dir ./results/NGCF/', 'output.setup=on -dir %s/' % (tmp_path / 'results')),
                     ('ngcf.hip=-layers 3 -keep 0.9 -graph written\n', 'ngcf.hip=%s\n' % line)):
        assert old in text, old
        text = text.replace(old, new)
    path = tmp_path / ('%s.conf' % name)
    path.write_text(text)
    return Config(str(path))


def events(rec):
    """(ev_u, ev_t, d_u, d_t, track ids in trackRecord's key order) as the plugin's graph and sampler see them."""
    d, rt = rec.data, rec.recType
    ev_u = [d.getId(e['user'], 'user') for e in d.trainingData]
    ev_t = [d.getId(e[rt], rt) for e in d.trainingData]
    du = {d.getId(u, 'user'): len(d.userRecord[u]) if u in d.userRecord else 0 for u in d.name2id['user']}
    dt = {d.getId(t, rt): len(d.trackRecord[t]) if t in d.trackRecord else 0 for t in d.name2id[rt]}
    keys = [d.getId(t, rt) for t in d.trackRecord.keys()]
    return ev_u, ev_t, du, dt, keys


def contract_F(rec, U0, V0, W0, seed, dtype, max_steps=None):
    """(F, the batches): the contract trained as the plugin trains -- random.seed(seed) at the start of buildModel, Adam's step
    and the mask's step counted over all epochs -- and propagated once without dropout.  max_steps stops the training early
    (tools/ngcf_e2e_drift.py)."""
    ev_u, ev_t, du, dt, keys = events(rec)
    g = ng.graph_from_events(ev_u, ev_t, rec.m, rec.n, rec.graph_form, du, dt)
    U, V, W = U0.astype(dtype), V0.astype(dtype), W0.astype(dtype)
    st = ng.new_state(U, V, W)
    random.seed(seed)
    t, batches = 0, []
    for _ in range(rec.maxIter):
        for u, i, j in ng.next_batch(ev_u, ev_t, keys, rec.batch_size, random):
            if max_steps is not None and t >= max_steps:
                break
            t += 1
            batches.append((u, i, j))
            ng.step(g, U, V, W, st, u, i, j, rec.lRate, rec.regU, t, True, rec.keep_prob, rec.mask_seed, dtype)
    return ng.propagate(g, U, V, W, False, dtype=dtype)['F'], batches


def plugin_on_cpu(tmp_path, name, seed=None):
    """The plugin of a problem after initModel (no device call so far) and the problem's seed."""
    from test_host_golden import _load
    from yue_amd.recommender.advanced.NGCF import NGCF
    conf = config(tmp_path, name)
    seed = PROBLEMS[name][4] if seed is None else seed
    rec = NGCF(conf, _load(conf), [])
    rec.readConfiguration()
    np.random.seed(seed)
    rec.initModel()
    return rec, seed
