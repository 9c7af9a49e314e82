"""GPU: the APR plugin on the device, from the config file to the lists: Yue(conf).execute() behind config/APR.conf on two
yue_amd.synth logs, for 1 + 1 and for 2 + 3 steps at k 64 and 50 (problems and rule in tests/helpers/apr_e2e.py; the seeds are
checked on the CPU in tests/test_apr_golden.py).  The yardstick is the fp64 contract trained from the plugin's own start factors on
the plugin's own batches: the printed lines have the reference's form, ranking_performance() follows every step, and each compared
test user's list equals the top-N oracle's on the fp64 contract's factors.  A user is left out only when a gap that decides the list
is smaller than the float32 contract's own error on that user; at most 2 % are."""
import random

import numpy as np
import pytest

from helpers import apr_e2e as ae
from helpers import numpy_apr as ap

pytestmark = pytest.mark.gpu


def run(tmp_path, monkeypatch, name):
    from yue_amd.base.IterativeRecommender import IterativeRecommender
    from yue_amd.recommender.advanced.APR import APR
    from yue_amd.yue import Yue
    conf = ae.config(tmp_path, name)
    seed = ae.PROBLEMS[name][4]
    kept = {'batches': [], 'scans': []}
    build, sample, scan = APR.buildModel, APR.next_batch, IterativeRecommender._scan

    def spy_build(self):
        kept['rec'], kept['U0'], kept['V0'] = self, self.U.copy(), self.V.copy()
        random.seed(seed)
        return build(self)

    def spy_sample(self):
        batch = sample(self)
        kept['batches'].append(batch)
        return batch

    def spy_scan(self, users, N, mask=None):
        ids = scan(self, users, N, mask)
        kept['scans'].append((list(users), N, mask, ids.copy()))
        return ids
    monkeypatch.setattr(APR, 'buildModel', spy_build)
    monkeypatch.setattr(APR, 'next_batch', spy_sample)
    monkeypatch.setattr(IterativeRecommender, '_scan', spy_scan)
    np.random.seed(seed)
    return conf, seed, kept, Yue(conf)


@pytest.mark.parametrize('name', list(ae.PROBLEMS))
def test_execute_trains_on_the_device_and_ranks_as_the_oracle_on_the_fp64_contract(tmp_path, capsys, monkeypatch, orc, name):
    conf, seed, kept, yue = run(tmp_path, monkeypatch, name)
    yue.execute()
    out = capsys.readouterr().out
    rec = kept['rec']
    iters, adv = ae.PROBLEMS[name][6:8]
    steps = iters + adv
    lines = [ln for ln in out.splitlines() if ln.startswith('iteration:')]
    assert [ln.split(' loss:')[0] for ln in lines] == ['iteration: %d' % e for e in list(range(iters)) + list(range(adv))]
    assert out.count('Ranking Performance') == steps and len(kept['batches']) == steps
    losses = [float(ln.split('loss: ')[1]) for ln in lines]
    batches = kept['batches']
    assert all(len(b[0]) == rec.negativeCount * rec.batch_size for b in batches) and rec.lRate == ae.LR
    Fc, want_losses = ae.contract_F(rec, kept['U0'], kept['V0'], batches, np.float64)
    F32 = ae.contract_F(rec, kept['U0'], kept['V0'], batches, np.float32)[0]
    for got, want in zip(losses, want_losses):
        print(name, 'loss', got, 'fp64', want, 'rel %.3g' % (abs(got - want) / abs(want)))
        assert np.isfinite(got)                                  # (reported, not bounded: the lists below are the check)
    assert not np.array_equal(rec.P, kept['U0']) and rec.U is rec.P and rec.V is rec.Q
    F = np.concatenate([rec.P, rec.Q])
    assert F.dtype == np.float32 and F.shape == Fc.shape == (rec.m + rec.n, rec.k)
    N = max(rec._top_list())
    names, uids, mp, mi = ae.ranked_users(rec)
    assert len(kept['scans']) == steps + 1                       # ranking_performance after every step, then evalRanking's one scan
    assert all(s[1] == 10 and s[2] is not None for s in kept['scans'][:-1])
    users, n_asked, mask, got = kept['scans'][-1]
    assert users == names and n_asked == N and mask is None
    keep, dist = ae.compared_users(Fc, rec.m, uids, mp, mi, N, F32)          # the float32 contract's own error decides who is left out
    want = ae.oracle_lists(orc, Fc, rec.m, uids, mp, mi, N)
    differ = ~(got == want).all(axis=1)
    print(name, 'steps', steps, 'test users', len(uids), 'left out', int((~keep).sum()), 'F distance from the fp64 contract: device %.3g, float32 contract %.3g'
          % (ap.rel(F, Fc), ap.rel(F32, Fc)), 'flipped elements: device', ae.flipped(F, Fc, rec.lRate), 'float32 contract', ae.flipped(F32, Fc, rec.lRate),
          'lists that differ', int(differ.sum()), 'of them compared', int((differ & keep).sum()))
    assert len(uids) >= 50 and (~keep).sum() <= ae.CAP * len(uids)
    assert np.array_equal(got[keep], want[keep])
    assert rec.measure and rec.measure[0] == 'Top 5\n'
