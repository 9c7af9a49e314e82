"""The end-to-end CDAE problems shared by tests/test_cdae_golden.py (which checks on the CPU that the logs leave the contract alone
inside the rule) and tests/test_gpu_cdae_plugin.py (which runs Yue(conf).execute() on the device).

A problem is a yue_amd.synth text log behind config/CDAE.conf.  Its yardstick is the fp64 contract trained from the plugin's own
start values (U, W, W', b, b'), on the plugin's own batches and the contract's masks of the plugin's seed; the factors are
P[u] = [hid(u) | 1] from the uncorrupted row and Q[i] = [W'[:, i] | b'[i]], F = [P; Q].  Lists, the rule that decides which users
are compared and the way a user is left out are those of tests/helpers/lightgcn_e2e.py: a user is left out only when the gap between
the N-th and the (N + 1)-th fp64 score is smaller than the error the other side's factors can make.  Here at most 2 % of the
compared users may be left out.  The problems train for one and for three steps at stddev 0.1 and a small learning rate: Adam's
first steps move every element by about lr whatever its size, and float32 training leaves fp64 step by step.
"""
import os
import random

import numpy as np

from . import numpy_cdae as cd
from .lightgcn_e2e import ROOT, compared_users, oracle_lists, ranked_users  # noqa: F401

CAP = 0.02

# name -> (synth users, items, events per user, synth seed, seed of the start values and the sampler, steps, batch size, -co,
#          learnRate, the cdae.hip line)
PROBLEMS = {
    'one_step': (150, 400, 12, 20260011, 22, 1, 64, 0.5, 0.002, '-stddev 0.1 -nh 64'),
    'three_steps': (200, 150, 6, 20260013, 13, 3, 32, 0.1, 0.002, '-stddev 0.1 -seed 7 -neg 3'),
    'as_written': (150, 400, 12, 20260011, 22, 2, 64, 0.1, 0.6, None),
}
TRAINING = ('one_step', 'three_steps')


def config(tmp_path, name):
    from yue_amd import synth
    from yue_amd.tool.config import Config
    m, n, d, log_seed, seed, iters, batch, co, lr, line = PROBLEMS[name]
    log = tmp_path / ('%s.txt' % name)
    synth.write_text_log(str(log), m, n, d, seed=log_seed)
    text = open(os.path.join(ROOT, 'config', 'CDAE.conf')).read()
    for old, new in (('record=./dataset/log.txt', 'record=%s' % log), ('num.max.iter=100', 'num.max.iter=%d' % iters),
                     ('CDAE=-batch_size 256 -co 0.1 -nh 128', 'CDAE=-batch_size %d -co %s -nh 128' % (batch, co)),
                     ('learnRate=-init 0.6 -max 10', 'learnRate=-init %s -max 10' % lr),
                     ('output.setup=on -dir ./results/CDAE/', 'output.setup=on -dir %s/' % (tmp_path / 'results')),
                     ('cdae.hip=-stddev 0.25 -seed 2 -neg 5\n', 'cdae.hip=%s\n' % line if line else '')):
        assert old in text, old
        text = text.replace(old, new)
    path = tmp_path / ('%s.conf' % name)
    path.write_text(text)
    return Config(str(path))


def key_ids(rec):
    """(user ids, track ids) in name2id's key order: what random.choice draws from."""
    d, rt = rec.data, rec.recType
    return [d.name2id['user'][u] for u in d.name2id['user'].keys()], [d.name2id[rt][t] for t in d.name2id[rt].keys()]


def params(rec):
    return {'U': rec.U, 'W': rec.W, 'Wd': rec.Wd, 'b': rec.b, 'bd': rec.bd}


def contract_F(rec, p0, seed, dtype, max_steps=None):
    """(F = [P; Q], the batches, the steps' (loss, saturated)): the contract trained as the plugin trains -- random.seed(seed) at the
    start of buildModel, step t = 1, 2, ... for Adam and the mask."""
    data = rec._user_csr
    users_k, tracks_k = key_ids(rec)
    p = {k: v.astype(dtype) for k, v in p0.items()}
    st = cd.new_state(p)
    random.seed(seed)
    batches, losses = [], []
    for t in range(1, rec.maxIter + 1):
        if max_steps is not None and t > max_steps:
            break
        users, sets = cd.next_batch(users_k, tracks_k, data, rec.batch_size, rec.negative_sp, random)
        sptr, sitems = cd.sample_csr(sets)
        batches.append((users, [sorted(s) for s in sets]))
        loss, sat = cd.step(p, st, data, users, sptr, sitems, rec.corruption_level, rec.mask_seed, t, rec.lRate, rec.regU, dtype)
        losses.append((float(loss), sat))
        if sat:
            break
    P, Q = cd.factors(p, data, dtype)
    return np.concatenate([P, Q]), batches, losses


def plugin_on_cpu(tmp_path, name, seed=None):
    """The plugin of a problem after initModel (no device call so far) and the problem's seed."""
    from test_host_golden import _load
    from yue_amd.recommender.advanced.CDAE import CDAE
    conf = config(tmp_path, name)
    seed = PROBLEMS[name][4] if seed is None else seed
    rec = CDAE(conf, _load(conf), [])
    rec.readConfiguration()
    np.random.seed(seed)
    rec.initModel()
    return rec, seed
