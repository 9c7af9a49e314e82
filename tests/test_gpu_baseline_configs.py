"""GPU parity at BASELINE.json's full sizes, through the C ABI.

  * config 3 (1M users x 200K items, k=128, 50M triplets, the device's default round size): one full
    epoch against the oracle's restatement of the same rounds (oracle/bpr_oracle.c: orc_bpr_rounds) --
    the bench workload itself, at the real Zipf contention and the default W (344,064: metadata pre-pass,
    round launches without retire phase, fold launches);
  * one GPU's share of config 4 (10M users -> 5.1 GB of replicated user factors, a 125K-item shard,
    60M events) through the communicator code path (1-rank RCCL communicator: all-reduce + range apply
    on the second stream) against the same oracle (world = 1: the sharded spec IS the S-round oracle
    with rounds cut at user blocks, tests/test_dist_cpu.py::test_one_rank_spec_equals_plain_rounds); the same shard
    through the EXACT path (60M triplets, 10M runs) against the oracle's sequential loop;
  * config 3 and config 2 (100K x 50K, k=64): how far one S-round epoch (the throughput semantics) lands from the
    reference's strictly sequential loop (recommender/cf/BPR.py:40-62, orc_bpr_sequential) on the same
    negatives -- the semantic deviation, with a stated bound.

Tolerances: factor matrices within 1e-5 rel fp32 (BASELINE.json north_star; rel = max|a-b| / max|b|), the
element-wise figure is printed and bounded beside it; loss to 1e-9; the sampler's integers bit-exact.
"""
import os
import time

import numpy as np
import pytest

from yue_amd import synth
from yue_amd.dist import epoch_round_ptr
from util import rel_err, rel_err_elem

pytestmark = pytest.mark.gpu

TOL = 1e-5
LR, REG_U, REG_I = 0.02, 0.01, 0.01          # bench.py's hyper-parameters (BPR.conf)


def _fresh_device():
    from yue_amd._shim import Device
    return Device(0, raise_errors=True)


def _epoch_vs_oracle(orc, dev, data, P0, Q0, seed, W, tag):
    m, n = P0.shape[0], Q0.shape[0]
    ev_u = np.repeat(np.arange(m, dtype=np.int32), np.diff(data['ev_ptr']))
    t0 = time.time()
    j_gpu = dev.sample_negatives(seed, 0)
    j_orc = orc.sample_counter(seed, 0, ev_u, n, data['indptr'], data['indices'])
    assert np.array_equal(j_gpu, j_orc)                      # integer work: bit-exact
    nll, sp, sq = dev.bpr_epoch(seed, 0, W, LR, REG_U, REG_I)
    P, Q = dev.get_factors()
    if W == 0:
        W = dev.default_round_events()
    rp = np.array(epoch_round_ptr(data['ev_ptr'], W), np.int64)
    Po, Qo = P0, Q0                                           # the oracle works in place on the initial arrays
    # (one GPU: a wave owns a user and walks the user's events in order; on a communicator the user rows keep round semantics)
    rounds = orc.bpr_rounds_seq_user if dev.get_option('round_last_user_seq') else orc.bpr_rounds
    nll_o = rounds(Po, Qo, ev_u, data['ev_i'], j_orc, rp, LR, REG_U, REG_I)
    eP, eQ = rel_err(P, Po), rel_err(Q, Qo)
    xP, xQ = rel_err_elem(P, Po), rel_err_elem(Q, Qo)
    print('%s: W=%d rounds=%d  rel_err P %.2e Q %.2e  element-wise (|b|>1e-3) P %.2e Q %.2e  nll %.6f vs %.6f  bit-equal Q %.3f  (%.0f s)'
          % (tag, W, len(rp) - 1, eP, eQ, xP, xQ, nll, nll_o, float(np.mean(Q == Qo)), time.time() - t0))
    assert eP < TOL and eQ < TOL
    assert xP < 1e-3 and xQ < 1e-3                            # element-wise, elements above 1e-3 (1 % of the value range)
    # (one GPU: k_round_u's coefficient is single precision by default -- the margins, hence the loss, move in the 7th digit)
    assert abs(nll - nll_o) <= (1e-6 if dev.get_option('round_last_user_seq') else 1e-9) * abs(nll_o)
    # double-precision sums of up to 1.3e9 fp32 squares, added in different orders on the two sides
    assert abs(sp - orc.sumsq(P)) <= 1e-11 * sp and abs(sq - orc.sumsq(Q)) <= 1e-11 * sq


def test_config3_full_epoch_matches_oracle(orc):
    # BASELINE config 3 = the bench workload: same generator seeds as bench.py, default round size
    m, n, d, k = 1000000, 200000, 50, 128
    data = synth.make_arrays(m, n, d, seed=20260001)
    P0, Q0 = synth.init_factors(m, n, k, 20260002)
    dev = _fresh_device()
    try:
        dev.set_factors(P0, Q0)
        dev.set_interactions(data['indptr'], data['indices'], data['ev_ptr'], data['ev_i'])
        _epoch_vs_oracle(orc, dev, data, P0, Q0, 20260003, 0, 'C3')
    finally:
        dev.close()


def test_config4_shard_through_the_communicator_path(orc):
    # one rank's share of BASELINE config 4 on a 1-rank communicator: user blocks, in-place RCCL all-reduce of the
    # blocks' user-factor differences, k_apply_range on the second stream, P / dP beyond 2 GiB
    from yue_amd._shim import comm_unique_id
    m, n, d, k = 10000000, 125000, 6, 128
    data = synth.make_arrays(m, n, d, seed=20260001)
    rng = np.random.default_rng(20260002)
    P0 = rng.random((m, k), dtype=np.float32) / 10
    Q0 = rng.random((n, k), dtype=np.float32) / 10
    dev = _fresh_device()
    try:
        dev.set_factors(P0, Q0)
        dev.set_interactions(data['indptr'], data['indices'], data['ev_ptr'], data['ev_i'])
        dev.comm_init(comm_unique_id(), 0, 1)
        _epoch_vs_oracle(orc, dev, data, P0, Q0, 20260003, 0, 'C4 shard (communicator path)')
    finally:
        dev.close()


def test_config4_shard_exact_epoch_matches_the_sequential_oracle(orc):
    # the reference's sequential semantics on one rank's share of config 4: 10M runs of 6 triplets, user factors beyond 2 GiB
    m, n, d, k = 10000000, 125000, 6, 128
    data = synth.make_arrays(m, n, d, seed=20260001)
    P0, Q0 = synth.init_factors(m, n, k, 20260002)
    ev_u = np.repeat(np.arange(m, dtype=np.int32), np.diff(data['ev_ptr']))
    dev = _fresh_device()
    try:
        dev.set_factors(P0, Q0)
        dev.set_interactions(data['indptr'], data['indices'], data['ev_ptr'], data['ev_i'])
        j = dev.sample_negatives(20260003, 0)
        dev.set_option('epoch_exact', 1)
        t0 = time.time()
        nll_x, _, _ = dev.bpr_epoch(20260003, 0, 0, LR, REG_U, REG_I)
        t_dev = time.time() - t0
        Px, Qx = dev.get_factors()
        # the same epoch with the single-precision coefficient (option chain_fast): north_star's 1e-5 instead of bit-equality
        dev.set_factors(P0, Q0)
        dev.set_option('chain_fast', 1)
        nll_f, _, _ = dev.bpr_epoch(20260003, 0, 0, LR, REG_U, REG_I)
        us_f = dev.get_option('chain_last_us')
        Pf, Qf = dev.get_factors()
    finally:
        dev.close()
    nll_s = orc.bpr_sequential(P0, Q0, ev_u, data['ev_i'], j, LR, REG_U, REG_I)       # in place on the initial arrays
    print('C4 shard exact epoch on the device (%.0f ms incl. first-call allocations) vs the sequential oracle: bit-equal P %.5f Q %.5f, rel P %.1e Q %.1e'
          % (1e3 * t_dev, np.mean(Px == P0), np.mean(Qx == Q0), rel_err(Px, P0), rel_err(Qx, Q0)))
    assert rel_err(Px, P0) < 1e-6 and rel_err(Qx, Q0) < 1e-6 and abs(nll_x - nll_s) <= 1e-9 * nll_s
    assert np.array_equal(Px, P0) and np.array_equal(Qx, Q0)
    print('C4 shard, single-precision coefficient (dataflow launch %.0f ms): bit-equal P %.5f Q %.5f, rel P %.1e Q %.1e, loss rel %.1e'
          % (1e-3 * us_f, np.mean(Pf == P0), np.mean(Qf == Q0), rel_err(Pf, P0), rel_err(Qf, Q0), abs(nll_f - nll_s) / nll_s))
    assert rel_err(Pf, P0) < 1e-5 and rel_err(Qf, Q0) < 1e-5 and abs(nll_f - nll_s) <= 1e-6 * nll_s


def _round_semantics_vs_sequential(orc, m, n, d, k, tag):
    data = synth.make_arrays(m, n, d, seed=20260001)
    P0, Q0 = synth.init_factors(m, n, k, 20260002)
    ev_u = np.repeat(np.arange(m, dtype=np.int32), np.diff(data['ev_ptr']))
    E = len(ev_u)
    dev = _fresh_device()
    try:
        dev.set_factors(P0, Q0)
        dev.set_interactions(data['indptr'], data['indices'], data['ev_ptr'], data['ev_i'])
        W = dev.default_round_events()
        j = dev.sample_negatives(20260003, 0)
        nll_r, _, _ = dev.bpr_epoch(20260003, 0, W, LR, REG_U, REG_I)
        Pr, Qr = dev.get_factors()
        # the same epoch with the reference's exact semantics on the device (chain_kernels.hpp): checked below, at this
        # BASELINE size, against the oracle's sequential loop
        dev.set_factors(P0, Q0)
        dev.set_option('epoch_exact', 1)
        nll_x, _, _ = dev.bpr_epoch(20260003, 0, 0, LR, REG_U, REG_I)
        us_x = dev.get_option('chain_last_us')
        Px, Qx = dev.get_factors()
        # ... and with the single-precision coefficient (option chain_fast: north_star's 1e-5 instead of bit-equality), on all
        # XCDs and with the working waves on one XCD
        fast = []
        for xcd in (0, 1):
            dev.set_factors(P0, Q0)
            dev.set_option('chain_fast', 1)
            dev.set_option('chain_xcd', xcd)
            nll_f, _, _ = dev.bpr_epoch(20260003, 0, 0, LR, REG_U, REG_I)
            fast.append((nll_f, dev.get_option('chain_last_us')) + dev.get_factors())
        dev.set_option('chain_fast', 0)
        dev.set_option('chain_xcd', 0)
    finally:
        dev.close()
    Ps, Qs = P0.copy(), Q0.copy()
    nll_s = orc.bpr_sequential(Ps, Qs, ev_u, data['ev_i'], j, LR, REG_U, REG_I)
    print('%s exact epoch on the device (dataflow launch %.0f ms) vs the sequential oracle: bit-equal P %.5f Q %.5f, rel P %.1e Q %.1e'
          % (tag, 1e-3 * us_x, np.mean(Px == Ps), np.mean(Qx == Qs), rel_err(Px, Ps), rel_err(Qx, Qs)))
    assert rel_err(Px, Ps) < 1e-6 and rel_err(Qx, Qs) < 1e-6 and abs(nll_x - nll_s) <= 1e-9 * nll_s
    assert np.array_equal(Px, Ps) and np.array_equal(Qx, Qs)
    for xcd, (nll_f, us_f, Pf, Qf) in enumerate(fast):
        print('%s, single-precision coefficient%s (dataflow launch %.0f ms = %.3e triplets/s): bit-equal P %.5f Q %.5f, rel P %.1e Q %.1e, loss rel %.1e'
              % (tag, ', one XCD' if xcd else '', 1e-3 * us_f, E / (1e-6 * us_f), np.mean(Pf == Ps), np.mean(Qf == Qs), rel_err(Pf, Ps), rel_err(Qf, Qs), abs(nll_f - nll_s) / nll_s))
        assert rel_err(Pf, Ps) < 1e-5 and rel_err(Qf, Qs) < 1e-5 and abs(nll_f - nll_s) <= 1e-6 * nll_s
    del fast

    def rms(a):
        return float(np.sqrt(np.mean(a.astype(np.float64) ** 2)))
    moved_P, moved_Q = rms(Ps - P0), rms(Qs - Q0)
    dist_P, dist_Q = rms(Pr - Ps), rms(Qr - Qs)
    dloss = abs(nll_r - nll_s) / nll_s
    print('%s, one epoch, W=%d: nll/triplet sequential %.6f  S-round %.6f  (rel diff %.2e);  RMS distance S-round vs sequential '
          'P %.3e Q %.3e  against RMS movement of the epoch P %.3e Q %.3e  (ratio P %.3f Q %.3f);  norm-wise rel P %.2e Q %.2e'
          % (tag, W, nll_s / E, nll_r / E, dloss, dist_P, dist_Q, moved_P, moved_Q, dist_P / moved_P, dist_Q / moved_Q,
             rel_err(Pr, Ps), rel_err(Qr, Qs)))
    return dloss, dist_P / moved_P, dist_Q / moved_Q


def test_config3_round_semantics_vs_the_sequential_loop(orc):
    # the bench workload itself: one epoch of the throughput semantics at the default W (344,064 events per round) against the
    # reference's strictly sequential loop on identical negatives (50M triplets through the C oracle: under a minute).
    # Round 4: on one GPU a wave owns a user and walks the user's events in order (k_round_u), only the item rows keep round
    # semantics -- measured (profiles/r04_deviation_c3_seq1.jsonl): loss +0.026 %, distance / movement 0.0156 (P), 0.0021 (Q);
    # with user rows under round semantics too (round 3, what a communicator still runs) +0.332 %, 0.0902 / 0.0199.
    # Bounds = 1.5 x the measured values.
    dloss, rP, rQ = _round_semantics_vs_sequential(orc, 1000000, 200000, 50, 128, 'C3')
    assert dloss < 4.0e-4 and rP < 0.024 and rQ < 0.0032


def test_config2_round_semantics_vs_the_sequential_loop(orc):
    # How far does ONE epoch of the throughput semantics (S-round, default W = 172,032 = 3.4 events per item row) land from the
    # reference's strictly sequential loop on identical negatives?  Both start from the same factors; the distance is compared
    # with the distance the epoch itself travels.  Measured with sequential user rows (profiles/r04_deviation_c2_seq1.jsonl):
    # loss +0.107 %, distance / movement 0.0396 (P), 0.0072 (Q) (round 3, user rows under round semantics: +0.495 %, 0.0629 /
    # 0.0367).  Bounds = 1.5 x the measured values.
    dloss, rP, rQ = _round_semantics_vs_sequential(orc, 100000, 50000, 50, 64, 'C2')
    assert dloss < 1.6e-3 and rP < 0.060 and rQ < 0.011


@pytest.mark.skipif(not os.environ.get('YUE_TEST_BIG_ITEMS'), reason='opt-in (YUE_TEST_BIG_ITEMS=1): no BASELINE config has an item matrix of 2 GiB, the two cases cost a minute of every GPU run')
@pytest.mark.parametrize('n,k', [(4600000, 128), (2800000, 200)])
def test_item_matrix_beyond_two_gib(orc, n, k):
    """An item matrix of 2.4 GB (2.2 GB) on one GPU (4.6M items x k = 128, 2.8M x 200; 31-bit byte offsets end at 2 GiB): yue_bpr_epoch's default path
    addresses item and staging rows through 64-bit pointers (k_round_m<.., BIGQ>, bucketed pre-pass over 141 item ranges) and
    must match the oracle's rounds; explicit rounds and the exact path refuse such a matrix instead of wrapping around."""
    from yue_amd._shim import YueHipError
    m, d = 40000, 50                                       # (k = 200: the four-registers-per-row instance, f32-MFMA scoring)
    data = synth.make_arrays(m, n, d, seed=20260001)
    P0, Q0 = synth.init_factors(m, n, k, 20260002)
    assert Q0.nbytes > (1 << 31)
    ev_u = np.repeat(np.arange(m, dtype=np.int32), np.diff(data['ev_ptr']))
    dev = _fresh_device()
    try:
        dev.set_factors(P0, Q0)
        dev.set_interactions(data['indptr'], data['indices'], data['ev_ptr'], data['ev_i'])
        with pytest.raises(YueHipError):
            dev.bpr_rounds(ev_u[:64], data['ev_i'][:64], np.zeros(64, np.int32) + 7, np.array([0, 64], np.int64), LR, REG_U, REG_I)
        dev.set_option('epoch_exact', 1)
        with pytest.raises(YueHipError):
            dev.bpr_epoch(20260003, 0, 0, LR, REG_U, REG_I)
        dev.set_option('epoch_exact', 0)
        P, Q = dev.get_factors()
        assert np.array_equal(Q[-1000:], Q0[-1000:]) and np.array_equal(P, P0)        # the refused calls changed nothing
        del P, Q
        _epoch_vs_oracle(orc, dev, data, P0, Q0, 20260003, 0, 'item matrix of %.1f GB, k = %d' % (Q0.nbytes / 1e9, k))
        # the scoring path over the same matrix (P0, Q0 now hold the oracle's state after the epoch: within 1e-5 of the device's;
        # the lists are compared on the device's own factors)
        P, Q = dev.get_factors()
        users = np.array([0, 1, 17, 3999, 20000, m - 1], np.int32)
        ids, sc = dev.topn_scan(users, 20)
        from util import mask_rows
        mp, mi = mask_rows(data['indptr'], data['indices'], users)
        oid, osc, rc = orc.topn_scan(P, Q, users, 20, mp, mi)
        assert np.array_equal(ids, oid) and np.array_equal(sc, osc)
    finally:
        dev.close()
