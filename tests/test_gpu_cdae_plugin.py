"""GPU: the CDAE plugin on the device, from the config file to the lists: Yue(conf).execute() behind config/CDAE.conf on two
yue_amd.synth logs, for one and for three steps at a stddev that does not saturate (problems and rule in tests/helpers/cdae_e2e.py;
the logs are checked on the CPU in tests/test_cdae_golden.py).  The yardstick is the fp64 contract trained from the plugin's own
start values on the plugin's own batches and the contract's masks: the printed lines have the reference's form, the losses are the
fp64 contract's within 1e-5, and each compared test user's list equals the top-N oracle's on the fp64 contract's logits.  A user is
left out only when a gap that decides the list is smaller than the float32 contract's own error on that user; at most 2 % are.
A third run with the reference's stddev 1.0 stops with the saturation message and exit status after the inf loss line."""
import random
import re

import numpy as np
import pytest

from helpers import cdae_e2e as ce
from helpers import numpy_cdae as cd

pytestmark = pytest.mark.gpu


def run(tmp_path, monkeypatch, name):
    from yue_amd.base.IterativeRecommender import IterativeRecommender
    from yue_amd.recommender.advanced.CDAE import CDAE
    from yue_amd.yue import Yue
    conf = ce.config(tmp_path, name)
    seed = ce.PROBLEMS[name][4]
    kept = {'batches': [], 'scans': []}
    build, sample, scan = CDAE.buildModel, CDAE.next_batch, IterativeRecommender._scan

    def spy_build(self):
        kept['rec'], kept['p0'] = self, {k: v.copy() for k, v in ce.params(self).items()}
        random.seed(seed)
        return build(self)

    def spy_sample(self):
        users, sets = sample(self)
        kept['batches'].append((list(users), [sorted(s) for s in sets]))
        return users, sets

    def spy_scan(self, users, N, mask=None):
        ids = scan(self, users, N, mask)
        kept['scans'].append((list(users), N, mask, ids.copy()))
        return ids
    monkeypatch.setattr(CDAE, 'buildModel', spy_build)
    monkeypatch.setattr(CDAE, 'next_batch', spy_sample)
    monkeypatch.setattr(IterativeRecommender, '_scan', spy_scan)
    np.random.seed(seed)
    return conf, seed, kept, Yue(conf)


@pytest.mark.parametrize('name', ce.TRAINING)
def test_execute_trains_on_the_device_and_ranks_as_the_oracle_on_the_fp64_contract(tmp_path, capsys, monkeypatch, orc, name):
    conf, seed, kept, yue = run(tmp_path, monkeypatch, name)
    yue.execute()
    out = capsys.readouterr().out
    rec, steps = kept['rec'], ce.PROBLEMS[name][5]
    lines = [ln for ln in out.splitlines() if 'Epoch:' in ln]
    assert len(lines) == steps and all(re.fullmatch(r'\[1\] Epoch: %04d loss= \d+\.\d{9}' % (t + 1), ln) for t, ln in enumerate(lines)), lines
    assert 'Optimization Finished!' in out.splitlines()
    losses = [float(ln.split('loss= ')[1]) for ln in lines]
    # the fp64 contract trained from the plugin's start values, on the plugin's batches and masks
    Fc, batches, want_losses = ce.contract_F(rec, kept['p0'], seed, np.float64)
    F32 = ce.contract_F(rec, kept['p0'], seed, np.float32)[0]
    assert kept['batches'] == batches and len(batches) == steps
    for got, (want, sat) in zip(losses, want_losses):
        print(name, 'loss', got, 'fp64', want, 'rel %.3g' % (abs(got - want) / abs(want)))
        assert sat == 0 and abs(got - want) <= 1e-5 * abs(want)
    assert not np.array_equal(rec.U, kept['p0']['U']) and not np.array_equal(rec.Wd, kept['p0']['Wd'])
    F = np.concatenate([rec.P, rec.Q])
    assert F.dtype == np.float32 and F.shape == Fc.shape == (rec.m + rec.n, rec.n_hidden + 1) and (rec.P[:, -1] == 1).all()
    assert np.array_equal(rec.Q, np.concatenate([rec.Wd.T, rec.bd[:, None]], axis=1))
    N = max(rec._top_list())
    names, uids, mp, mi = ce.ranked_users(rec)
    assert len(kept['scans']) == 1                                # evalRanking's one scan
    users, n_asked, mask, got = kept['scans'][0]
    assert users == names and n_asked == N and mask is None
    keep, dist = ce.compared_users(Fc, rec.m, uids, mp, mi, N, F32)          # the float32 contract's own error decides who is left out
    want = ce.oracle_lists(orc, Fc, rec.m, uids, mp, mi, N)
    differ = ~(got == want).all(axis=1)
    print(name, 'steps', steps, 'test users', len(uids), 'left out', int((~keep).sum()), 'F distance from the fp64 contract: device %.3g, float32 contract %.3g'
          % (cd.rel(F, Fc), cd.rel(F32, Fc)), 'lists that differ', int(differ.sum()), 'of them compared', int((differ & keep).sum()))
    assert len(uids) >= 50 and (~keep).sum() <= ce.CAP * len(uids)
    assert np.array_equal(got[keep], want[keep])
    assert rec.measure and rec.measure[0] == 'Top 5\n'


def test_execute_as_written_stops_with_the_saturation_message(tmp_path, capsys, monkeypatch):
    conf, seed, kept, yue = run(tmp_path, monkeypatch, 'as_written')
    with pytest.raises(SystemExit) as e:
        yue.execute()
    out = capsys.readouterr().out
    rec = kept['rec']
    assert e.value.code == -1 and rec.stddev == 1.0 and rec.n_hidden == 128
    lines = [ln for ln in out.splitlines() if 'Epoch:' in ln]
    assert lines == ['[1] Epoch: 0001 loss= inf'] and 'Optimization Finished!' not in out
    assert 'cdae.hip=-stddev' in out and 'round to 1.0f' in out and len(kept['batches']) == 1 and not kept['scans']
    assert rec.dev.get_option('cdae_last_saturated') >= 1
    after = rec.dev.cdae_get_params(moments=True)
    for k, v in kept['p0'].items():                               # nothing moved
        assert np.array_equal(after[k], v) and not after['m' + k].any() and not after['v' + k].any()
