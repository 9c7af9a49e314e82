"""The epoch path's staged blocks: ticket 0 of a contended row stores its new row, the other touches (new - old), and the fold
launch sums the block without reading the round-start row (yue_amd/csrc/round_kernels.hpp: k_round_meta, k_round_u / k_round_m,
k_round_fold).  The interactions are built so that every round holds rows with about 2..72 touches each: blocks of every size
up to stage_max = 64 (the <= 4-row group path and the long-block path of the fold), hot rows above it, and rows written in
place beside them.  Both update launches, the plain and the bucketed pre-pass, two row widths, against the oracle.

(The form for item matrices of 2 GiB and more, k_round_m<.., BIGQ>, runs the same metadata and fold; its case needs a 2.4 GB
item matrix and is the opt-in test_gpu_baseline_configs.py::test_item_matrix_beyond_two_gib.)
"""
import numpy as np
import pytest

from yue_amd import synth
from yue_amd.dist import epoch_round_ptr
from util import rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-5
USERS_PER_ROUND, D = 512, 24
W = USERS_PER_ROUND * D
COUNTS = np.repeat(np.arange(2, 73), 3)   # positives per contended row and round, 3 rows each (negatives add a touch here and there)


def _interactions(m, n, seed):
    """users in rounds of USERS_PER_ROUND x D events; in every round item 1 + q is the positive of COUNTS[q] events, the
    other events have distinct items from the tail of the catalogue -- no user holds an item twice"""
    rs = np.random.RandomState(seed)
    hot = np.repeat(np.arange(1, 1 + len(COUNTS)), COUNTS).astype(np.int32)
    ev_i = np.empty(m * D, np.int32)
    for r0 in range(0, m, USERS_PER_ROUND):
        users = min(USERS_PER_ROUND, m - r0)
        fill = users * D - len(hot)
        tail = (1000 + rs.permutation(n - 1000)[:fill]).astype(np.int32)
        slots = np.concatenate([hot, tail])            # item-sorted head: copies of one item go to consecutive users
        ev_i[r0 * D:(r0 + users) * D] = slots.reshape(D, users).T.reshape(-1)
    ev_ptr = np.arange(m + 1, dtype=np.int64) * D
    rows = np.sort(ev_i.reshape(m, D), axis=1)
    assert (rows[:, 1:] != rows[:, :-1]).all()
    indptr = ev_ptr.copy()
    return {'ev_ptr': ev_ptr, 'ev_i': ev_i, 'indptr': indptr, 'indices': rows.reshape(-1)}


@pytest.mark.parametrize('k', [128, 40])
@pytest.mark.parametrize('bucket', [0, 1], ids=['plain_pre_pass', 'bucketed_pre_pass'])
@pytest.mark.parametrize('seq', [1, 0], ids=['k_round_u', 'k_round_m'])
def test_staged_blocks_of_every_size(orc, seq, bucket, k):
    from yue_amd._shim import Device
    m, n, seed = 4 * USERS_PER_ROUND, 100000, 7
    data = _interactions(m, n, seed=3)
    P0, Q0 = synth.init_factors(m, n, k, 5)
    ev_u = np.repeat(np.arange(m, dtype=np.int32), D)
    rp = np.array(epoch_round_ptr(data['ev_ptr'], W), np.int64)
    assert len(rp) == 5
    dev = Device(0, raise_errors=True)
    dev.set_option('round_user_seq', seq)
    dev.set_option('round_fast', 0)
    dev.set_option('round_stage', 64)
    dev.set_option('round_bucket', bucket)
    dev.set_factors(P0, Q0)
    dev.set_interactions(data['indptr'], data['indices'], data['ev_ptr'], data['ev_i'])
    assert dev.get_option('round_path') == 1
    Po, Qo = P0.copy(), Q0.copy()
    oracle_epoch = orc.bpr_rounds_seq_user if seq else orc.bpr_rounds
    for epoch in range(2):
        j = orc.sample_counter(seed, epoch, ev_u, n, data['indptr'], data['indices'])
        for r in range(len(rp) - 1 if epoch == 0 else 0):     # every round of the first epoch: blocks of each size 2..64, hot rows, single touches
            sl = slice(rp[r], rp[r + 1])
            ok = j[sl] >= 0
            touches = np.bincount(np.concatenate([data['ev_i'][sl][ok], j[sl][ok]]), minlength=n)
            assert set(range(2, 65)) <= set(touches.tolist()) and (touches > 64).any() and (touches == 1).sum() > 1000
        nll, sp, sq = dev.bpr_epoch(seed, epoch, W, 0.03, 0.01, 0.01)
        assert dev.get_option('round_last_stage_max') == 64
        assert dev.get_option('round_last_user_seq') == seq
        nll_o = oracle_epoch(Po, Qo, ev_u, data['ev_i'], j, rp, 0.03, 0.01, 0.01)
        P, Q = dev.get_factors()
        assert rel_err(P, Po) < TOL and rel_err(Q, Qo) < TOL, epoch
        assert abs(nll - nll_o) <= 1e-9 * abs(nll_o), epoch
        assert abs(sp - orc.sumsq(P)) <= 1e-12 * sp and abs(sq - orc.sumsq(Q)) <= 1e-12 * sq
    dev.close()


@pytest.mark.parametrize('empty_users', [0, 1], ids=['every_user_has_events', 'users_without_events'])
def test_epoch_sums_from_the_round_launches(orc, empty_users):
    """k_round_u sums P*P of the rows it stores and the fold launches sum the loss of their rounds' margins: the epoch's
    (nll, sum P*P, sum Q*Q) equal the oracle's in double precision.  Users without events keep the pass over P."""
    from yue_amd._shim import Device
    m, n, d, k, W = 3000, 2000, 20, 64, 4096
    data = synth.make_arrays(m, n, d, seed=17)
    if empty_users:
        cnt = np.diff(data['ev_ptr'])
        keep = np.ones(m, bool)
        keep[::97] = False
        cnt[~keep] = 0
        ev_ptr = np.zeros(m + 1, np.int64)
        np.cumsum(cnt, out=ev_ptr[1:])
        ev_i = data['ev_i'][np.repeat(keep, d)]
        data = dict(data, ev_ptr=ev_ptr, ev_i=ev_i)
    P0, Q0 = synth.init_factors(m, n, k, 9)
    ev_u = np.repeat(np.arange(m, dtype=np.int32), np.diff(data['ev_ptr']))
    rp = np.array(epoch_round_ptr(data['ev_ptr'], W), np.int64)
    dev = Device(0, raise_errors=True)
    dev.set_option('round_fast', 0)
    dev.set_factors(P0, Q0)
    dev.set_interactions(data['indptr'], data['indices'], data['ev_ptr'], data['ev_i'])
    Po, Qo = P0.copy(), Q0.copy()
    for epoch in range(2):
        j = orc.sample_counter(4, epoch, ev_u, n, data['indptr'], data['indices'])
        nll, sp, sq = dev.bpr_epoch(4, epoch, W, 0.02, 0.01, 0.01)
        assert dev.get_option('round_last_user_seq') == 1
        nll_o = orc.bpr_rounds_seq_user(Po, Qo, ev_u, data['ev_i'], j, rp, 0.02, 0.01, 0.01)
        P, Q = dev.get_factors()
        assert rel_err(P, Po) < TOL and rel_err(Q, Qo) < TOL
        assert abs(nll - nll_o) <= 1e-9 * abs(nll_o), epoch
        assert abs(sp - orc.sumsq(P)) <= 1e-12 * sp and abs(sq - orc.sumsq(Q)) <= 1e-12 * sq, epoch
        sp2, sq2 = dev.sumsq()                   # the plain passes over the same factors
        assert abs(sp - sp2) <= 1e-12 * sp2 and abs(sq - sq2) <= 1e-12 * sq2
    if empty_users:
        assert np.array_equal(P[::97], P0[::97])
    dev.close()
