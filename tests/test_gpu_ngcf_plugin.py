"""GPU: the NGCF plugin on the device, from the config file to the lists: Yue(conf).execute() behind config/NGCF.conf on two
yue_amd.synth logs (m <= n with -graph written, one step; m > n with -graph symmetric -layers 2, three steps; problems, rule and
the reason for the step counts in tests/helpers/ngcf_e2e.py; the seeds are checked on the CPU in tests/test_ngcf_golden.py).
The yardstick is the fp64 contract trained from the plugin's own start values on the plugin's own batches and masks: the
ranking lists equal the top-N oracle's on its F for every user the near-tie rule compares, which leaves out at most 5 %.
Beside it: the first step's loss is the fp64 contract's within 1e-5; the factors the scan ranked with are the propagation
without dropout of the device's own trained U, V and weights, within 4 x the float32 contract's distance from fp64 on the same
input; the lists equal the oracle's on those factors too."""
import random

import numpy as np
import pytest

from helpers import ngcf_e2e as ne
from helpers import numpy_ngcf as ng

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('name', sorted(ne.PROBLEMS))
def test_execute_trains_on_the_device_and_ranks_its_own_F_as_the_oracle(tmp_path, capsys, monkeypatch, orc, name):
    from yue_amd.base.IterativeRecommender import IterativeRecommender
    from yue_amd.recommender.advanced.NGCF import NGCF
    from yue_amd.yue import Yue
    conf = ne.config(tmp_path, name)
    seed, line = ne.PROBLEMS[name][4], ne.PROBLEMS[name][8]
    kept = {'batches': [], 'scans': []}
    build, sample, scan = NGCF.buildModel, NGCF.next_batch, IterativeRecommender._scan

    def spy_build(self):
        kept['rec'], kept['U0'], kept['V0'], kept['W0'] = self, self.U.copy(), self.V.copy(), self.W.copy()
        random.seed(seed)
        return build(self)

    def spy_sample(self):
        for batch in sample(self):
            kept['batches'].append(tuple(list(x) for x in batch))
            yield batch

    def spy_scan(self, users, N, mask=None):
        ids = scan(self, users, N, mask)
        kept['scans'].append((list(users), N, mask, ids.copy()))
        return ids
    monkeypatch.setattr(NGCF, 'buildModel', spy_build)
    monkeypatch.setattr(NGCF, 'next_batch', spy_sample)
    monkeypatch.setattr(IterativeRecommender, '_scan', spy_scan)
    np.random.seed(seed)
    Yue(conf).execute()
    out = capsys.readouterr().out
    rec = kept['rec']
    assert (rec.graph_form, rec.n_layers) == (('symmetric', 2) if 'symmetric' in line else ('written', 3))
    assert (rec.m <= rec.n) == (rec.graph_form == 'written') and (rec.n_layers + 1) * rec.k <= 256
    # the plugin's graph and batches are the contract's
    ev_u, ev_t, du, dt, keys = ne.events(rec)
    g = ng.graph_from_events(ev_u, ev_t, rec.m, rec.n, rec.graph_form, du, dt)
    for got, key in zip(rec._graph_csr, ('ptr', 'col', 'w')):
        assert np.array_equal(got, g[key]), key
    random.seed(seed)
    batches = [b for _ in range(rec.maxIter) for b in ng.next_batch(ev_u, ev_t, keys, rec.batch_size, random)]
    assert kept['batches'] == batches and len(batches[-1][0]) < rec.batch_size
    lines = [ln for ln in out.splitlines() if ln.startswith('training:')]
    per_epoch = len(batches) // rec.maxIter
    assert [ln.split(' loss:')[0] for ln in lines] == ['training: %d batch %d' % (it + 1, b) for it in range(rec.maxIter) for b in range(per_epoch)]
    losses = [float(ln.split(' loss: ')[1]) for ln in lines]
    assert all(np.isfinite(losses))
    # the first step, before any update: the fp64 contract's loss
    want = float(ng.loss_and_grad(g, kept['U0'].astype(np.float64), kept['V0'].astype(np.float64), kept['W0'], *batches[0], rec.regU, True,
                                  rec.keep_prob, rec.mask_seed, 1, np.float64)[0])
    print(name, 'first loss', losses[0], 'fp64', want, 'rel %.3g' % (abs(losses[0] - want) / abs(want)))
    assert abs(losses[0] - want) <= 1e-5 * abs(want)
    # the factors the scan ranked with: the propagation without dropout of the device's own trained parameters
    assert not np.array_equal(rec.U, kept['U0']) and not np.array_equal(rec.W, kept['W0']) and rec.W.shape == kept['W0'].shape
    F = np.concatenate([rec.P, rec.Q])
    F64 = ng.propagate(g, rec.U.astype(np.float64), rec.V.astype(np.float64), rec.W, False, dtype=np.float64)['F']
    F32 = ng.propagate(g, rec.U, rec.V, rec.W, False, dtype=np.float32)['F']
    assert F.dtype == np.float32 and F.shape == F64.shape == (rec.m + rec.n, (rec.n_layers + 1) * rec.k)
    print(name, 'F distance %.3g (float32 contract %.3g)' % (ng.rel(F, F64), ng.rel(F32, F64)))
    assert ng.rel(F, F64) <= 4 * ng.rel(F32, F64)
    N = max(rec._top_list())
    names, uids, mp, mi = ne.ranked_users(rec)
    assert len(kept['scans']) == 1                                # evalRanking's one scan
    users, n_asked, mask, got = kept['scans'][0]
    assert users == names and n_asked == N and mask is None
    # end to end: the fp64 contract trained from the plugin's start values, on the plugin's batches and masks
    Fc, batches_c = ne.contract_F(rec, kept['U0'], kept['V0'], kept['W0'], seed, np.float64)
    assert kept['batches'] == batches_c and Fc.shape == F.shape
    keep_c, dist_c = ne.compared_users(Fc, rec.m, uids, mp, mi, N, F)
    want_c = ne.oracle_lists(orc, Fc, rec.m, uids, mp, mi, N)
    differ_c = ~(got == want_c).all(axis=1)
    print(name, 'steps', len(batches), 'test users', len(uids), 'left out', int((~keep_c).sum()), 'F distance from the trained fp64 contract %.3g abs, %.3g rel'
          % (dist_c, ng.rel(F, Fc)), 'lists that differ', int(differ_c.sum()), 'of them compared', int((differ_c & keep_c).sum()))
    assert len(uids) >= 50 and (~keep_c).sum() <= 0.05 * len(uids)
    assert np.array_equal(got[keep_c], want_c[keep_c])
    # the lists: also the oracle's on the device's own F
    keep, dist = ne.compared_users(F, rec.m, uids, mp, mi, N, F)
    want = ne.oracle_lists(orc, F, rec.m, uids, mp, mi, N)
    assert got.shape == want.shape
    differ = ~(got == want).all(axis=1)
    print(name, 'test users', len(uids), 'left out', int((~keep).sum()), 'lists that differ', int(differ.sum()), 'of them compared', int((differ & keep).sum()))
    assert len(uids) >= 50 and (~keep).sum() <= 0.05 * len(uids)
    assert np.array_equal(got[keep], want[keep])
    assert rec.measure and rec.measure[0] == 'Top 5\n'
