"""The end-to-end APR problems shared by tests/test_apr_golden.py (which checks on the CPU that the seeds leave the float32 contract
inside the rule) and tests/test_gpu_apr_plugin.py (which runs Yue(conf).execute() on the device).

A problem is a yue_amd.synth text log behind config/APR.conf with few steps of either phase.  Its yardstick is the fp64 contract
(tests/helpers/numpy_apr.py) trained from the plugin's own start factors on the plugin's own batches: F = [U; V].  Lists, the rule
that decides which users are compared and the way a user is left out are those of tests/helpers/lightgcn_e2e.py: a user is left out
only when the gap between the N-th and the (N + 1)-th fp64 score is smaller than the error the other side's factors can make.  Here
at most 2 % of the test users may be left out: a condition on the problems, not a measurement.

Why few steps.  Adam at its first steps moves an element by about lr * sign(g) whatever |g| is, so an element whose gradient lies
within float32 noise of zero can move the other way in float32 and end 2 lr from the fp64 one (flipped(): how many do).

Why learnRate 0.0003 and not the file's 0.003.  Adam divides every element of the gradient by its own size, so an element's RELATIVE
rounding error becomes an error of lr times that in the factor.  In phase 2 the perturbation (norm eps = 0.5) is a hundred times
the factors (stddev 0.005): a gradient element is a small difference of large terms and carries a relative float32 error near 1e-3.
The float32 contract then ends about 5e-4 lr from the fp64 one in its worst element, and the rule's error bound grows with that
distance: at 0.003 it leaves 10 % of the test users or more out for every seed of 40 tried, at 0.001 2 % or more, at 0.0003 none for
the seeds chosen here.  The seeds (3 and 8 of 1 .. 12) are chosen on the CPU for that; tests/test_apr_golden.py asserts it."""
import os

import numpy as np

from . import numpy_apr as ap
from .lightgcn_e2e import ROOT, compared_users, oracle_lists, ranked_users  # noqa: F401

CAP = 0.02

LR = 0.0003

# name -> (synth users, items, events per user, synth seed, seed of the factors and the sampler, num.factors, num.max.iter, -advEpoch,
#          batch_size, the apr.hip line or None for the default)
PROBLEMS = {
    'one_one': (150, 120, 12, 20260021, 3, 64, 1, 1, 128, None),
    'two_three': (200, 150, 6, 20260023, 8, 50, 2, 3, 96, '-neg 2'),
}


def config(tmp_path, name):
    from yue_amd import synth
    from yue_amd.tool.config import Config
    m, n, d, log_seed, seed, k, iters, adv, batch, line = PROBLEMS[name]
    log = tmp_path / ('%s.txt' % name)
    synth.write_text_log(str(log), m, n, d, seed=log_seed)
    text = open(os.path.join(ROOT, 'config', 'APR.conf')).read()
    for old, new in (('record=./dataset/log.txt', 'record=%s' % log), ('num.max.iter=100', 'num.max.iter=%d' % iters),
                     ('batch_size=512', 'batch_size=%d' % batch), ('num.factors=64', 'num.factors=%d' % k),
                     ('-advEpoch 100', '-advEpoch %d' % adv), ('learnRate=-init 0.003 -max 1', 'learnRate=-init %s -max 1' % LR),
                     ('output.setup=on -dir ./results/APR/', 'output.setup=on -dir %s/' % (tmp_path / 'results')),
                     ('apr.hip=-neg 3\n', 'apr.hip=%s\n' % line if line else '')):
        assert old in text, old
        text = text.replace(old, new)
    path = tmp_path / ('%s.conf' % name)
    path.write_text(text)
    return Config(str(path))


def events(rec):
    """(ev_u, ev_i, listened) on ids: the events the sampler draws from (data.trainingData: every event of the log under -byTime)
    and the items the rejection sees (userRecord: the training side)."""
    d, rt = rec.data, rec.recType
    ev_u = [d.getId(e['user'], 'user') for e in d.trainingData]
    ev_i = [d.getId(e[rt], rt) for e in d.trainingData]
    listened = {d.getId(user, 'user'): {d.getId(e[rt], rt) for e in row} for user, row in d.userRecord.items()}
    return ev_u, ev_i, listened


def contract_F(rec, U0, V0, batches, dtype):
    """(F = [U; V], the losses) of the contract trained on the plugin's batches: num.max.iter phase-1 steps, then the adversarial ones."""
    U, V, losses = ap.train(U0, V0, batches, rec.maxIter, rec.lRate, rec.regU, rec.eps, rec.regAdv, dtype)
    return np.concatenate([U, V]), losses


def flipped(F32, F64, lr):
    """Elements of the float32 contract more than lr from the fp64 one: an Adam step that went the other way."""
    return int((np.abs(np.asarray(F32, np.float64) - F64) > lr).sum())


def plugin_on_cpu(tmp_path, name):
    """(the plugin of a problem after initModel -- no device call so far --, its batches in order, the seed)."""
    import random
    from test_host_golden import _load
    from yue_amd.recommender.advanced.APR import APR
    conf = config(tmp_path, name)
    seed = PROBLEMS[name][4]
    rec = APR(conf, _load(conf), [])
    rec.readConfiguration()
    np.random.seed(seed)
    rec.initModel()
    random.seed(seed)
    batches = [rec.next_batch() for _ in range(rec.maxIter + rec.advEpoch)]
    return rec, batches, seed
