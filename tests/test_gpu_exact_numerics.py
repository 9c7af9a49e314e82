"""Bit-equality of the EXACT training path (chain_kernels.hpp, through yue_bpr_replay and yue_bpr_epoch with epoch_exact) with
the sequential oracle (oracle/bpr_oracle.c: orc_bpr_sequential), where it is most likely to break:

  * the coefficient c = fp32(lr (1 - sigmoid(x))) read straight from the factors (the k = 2 construction of
    tests/helpers/margin_sweep.py) over every fp32 margin of the cancellation band [8, 32), 2^22 log-uniform margins and the
    edge values, through every kernel that computes chain_sigmoid on the exact path;
  * whole exact epochs at the margins training produces (most triplets with x > 8), in every kernel variant and at every
    row width (k_bpr_chain, k_bpr_chain3 with rings of 8 and 16 triplets, one XCD, two workgroups per CU).

Equality is asserted on the bits of P and Q (NaN or inf cannot hide anything); the loss is a double-precision sum in another
order on the device and stays within 1e-9."""
import numpy as np
import pytest

from helpers import margin_sweep as ms
from yue_amd import synth

pytestmark = pytest.mark.gpu

# BPR.conf's rate, and a rate at which fp32(lr (1 - s)) sits next to a rounding boundary of fp32 for s = 1/2 + 2^-53: a
# reciprocal of 2 - 2^-52 that is off by its last bit (x = 2^-52 in the edge set) moves c there
LRS = (0.02, 0.5 + 2.0 ** -25 + 2.0 ** -53)
BATCH = 1 << 19          # margins per replay (the exact path keeps its granule copy of Q below 2 GiB: 4 rows per margin here)

# margins at which the device's c may differ from the oracle's because glibc's exp is the side that is not correctly
# rounded (checked with mpmath): {(lr, margin bits): bits of the correctly rounded c}.  None so far.
GLIBC_EXCEPTIONS = {}

# every kernel that computes chain_sigmoid on the exact path, and the triplets per user (= per run) of the stream
SWEEP_VARIANTS = [
    ('split0', {'chain_split': 0}, 1),
    ('split1_ring8', {'chain_split': 1, 'chain_ring': 8}, 2),
    ('split1_ring16', {'chain_split': 1, 'chain_ring': 16}, 2),
    ('split1_xcd', {'chain_split': 1, 'chain_xcd': 1}, 2),
    # runs of ONE triplet: wave L1 of k_bpr_chain3 publishes nothing, only the run mailbox keeps wave L0 from running ahead
    ('split1_ring8_one_triplet_runs', {'chain_split': 1, 'chain_ring': 8}, 1),
    ('split1_ring16_one_triplet_runs', {'chain_split': 1, 'chain_ring': 16}, 1),
    ('split1_xcd_one_triplet_runs', {'chain_split': 1, 'chain_xcd': 1}, 1),
]
DEFAULTS = {'chain_split': -1, 'chain_ring': 0, 'chain_xcd': 0, 'chain_waves': 0, 'epoch_exact': 0}


@pytest.fixture(scope='module')
def dev():
    from yue_amd._shim import Device
    d = Device(0, raise_errors=True)
    yield d
    d.close()


def _with_options(dev, opts, fn):
    for key, v in opts.items():
        dev.set_option(key, v)
    try:
        return fn()
    finally:
        for key in opts:
            dev.set_option(key, DEFAULTS[key])


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize('name,opts,per_user', SWEEP_VARIANTS, ids=[v[0] for v in SWEEP_VARIANTS])
def test_coefficient_sweep_is_bit_equal(dev, orc, name, opts, per_user):
    found = []
    for lr in LRS:
        for set_name, x in ms.margin_sets():
            diffs, rows_differ, count = [], 0, 0
            for b in range(0, len(x), BATCH):
                xb = x[b:b + BATCH]
                P, Q, u, i, j, rows = ms.stream(xb, per_user)
                dev.set_factors(P, Q)
                _with_options(dev, opts, lambda: dev.bpr_replay(u, i, j, lr, 0.0, 0.0))
                Pd, Qd = dev.get_factors()
                orc.bpr_sequential(P, Q, u, i, j, lr, 0.0, 0.0)
                cd, co = Qd[rows, 1], Q[rows, 1]
                margin = np.repeat(xb, per_user)
                if per_user == 2:
                    margin[1::2] = xb + co[0::2]         # the second triplet of a user: fl(x + c1)
                for t in np.nonzero(_bits(cd) != _bits(co))[0]:
                    key = (lr, int(_bits(margin[t:t + 1])[0]))
                    if GLIBC_EXCEPTIONS.get(key) != int(_bits(cd[t:t + 1])[0]):
                        diffs.append((float(margin[t]), float(cd[t]), float(co[t])))
                # every other element follows from c; compared anyway (so rows of an excepted margin still count here)
                rows_differ += int(np.count_nonzero(np.any(_bits(Pd) != _bits(P), axis=1)))
                rows_differ += int(np.count_nonzero(np.any(_bits(Qd) != _bits(Q), axis=1)))
                count += len(u)
            print('coefficient sweep %s lr=%r %s: %d triplets, c differs on %d, factor rows that differ %d'
                  % (name, lr, set_name, count, len(diffs), rows_differ))
            if diffs or rows_differ:
                found.append((lr, set_name, len(diffs), rows_differ, diffs[:8]))
    assert not found, found


def test_one_triplet_runs_through_the_wave_group(dev, orc):
    """k_bpr_chain3 (chain_split = 1) on 4096 consecutive runs of one triplet each, at k = 64 on general rows: wave L0 claims
    run after run while wave L1 has nothing to publish -- the run mailbox between them must not be overwritten unread."""
    rs = np.random.RandomState(41)
    m, n, k, T = 5000, 9000, 64, 4096
    P0, Q0 = synth.init_factors(m, n, k, 42)
    u = rs.permutation(m)[:T].astype(np.int32)            # distinct users: every run has one triplet
    i = rs.randint(0, n, size=T).astype(np.int32)
    j = rs.randint(0, n, size=T).astype(np.int32)
    j[j == i] = (i[j == i] + 1) % n
    Po, Qo = P0.copy(), Q0.copy()
    nll_o = orc.bpr_sequential(Po, Qo, u, i, j, 0.02, 0.01, 0.01)
    for ring in (8, 16):
        dev.set_factors(P0, Q0)
        nll = _with_options(dev, {'chain_split': 1, 'chain_ring': ring}, lambda: dev.bpr_replay(u, i, j, 0.02, 0.01, 0.01))
        P, Q = dev.get_factors()
        assert np.array_equal(_bits(P), _bits(Po)) and np.array_equal(_bits(Q), _bits(Qo)), ring
        assert abs(nll - nll_o) <= 1e-9 * abs(nll_o)


def _problem(m, n, d, k, seed):
    data = synth.make_arrays(m, n, d, seed=seed)
    ev_u = np.repeat(np.arange(m, dtype=np.int32), np.diff(data['ev_ptr']))
    P0, Q0 = synth.init_factors(m, n, k, seed + 1)
    return data, ev_u, P0, Q0


def _margins(P, Q, ev_u, ev_i, j):
    live = j >= 0
    u, i, jj = ev_u[live], ev_i[live], j[live]
    return np.einsum('tk,tk->t', P[u].astype(np.float64), Q[i].astype(np.float64) - Q[jj].astype(np.float64))


EPOCH_VARIANTS = [
    ('split0', {'chain_split': 0}),
    ('split0_waves2', {'chain_split': 0, 'chain_waves': 2}),
    ('split1_ring8', {'chain_split': 1, 'chain_ring': 8}),
    ('split1_ring16', {'chain_split': 1, 'chain_ring': 16}),
    ('split1_xcd', {'chain_split': 1, 'chain_xcd': 1}),
    ('split1_waves2', {'chain_split': 1, 'chain_waves': 2}),
]
SEED = 5


@pytest.mark.parametrize('m,n,d,k', [(700, 900, 30, 10), (5000, 64, 12, 64), (3000, 2000, 20, 128), (400, 300, 25, 200)])
def test_exact_epochs_at_trained_margins_are_bit_equal(dev, orc, m, n, d, k):
    """test_gpu_exact.py's problems with the factors scaled until the margins are those of a trained model (a standard
    deviation of about 25: more than a quarter of the first epoch's triplets have x > 8, where 1 - s is a cancellation), then
    two exact epochs in every kernel variant: the same bits as the sequential oracle.  (k = 10, 64, 128, 200: every row width
    of the kernels, and the ring of 16 where it exists, k <= 128.)"""
    data, ev_u, P0, Q0 = _problem(m, n, d, k, 31 + k)
    dev.set_factors(P0, Q0)
    dev.set_interactions(data['indptr'], data['indices'], data['ev_ptr'], data['ev_i'])
    js = [dev.sample_negatives(SEED, ep) for ep in range(2)]
    scale = np.float32(np.sqrt(25.0 / np.std(_margins(P0, Q0, ev_u, data['ev_i'], js[0]))))
    P0, Q0 = P0 * scale, Q0 * scale
    x = _margins(P0, Q0, ev_u, data['ev_i'], js[0])
    print('k=%d: factors x %.1f, margins > 8: %.3f, < -8: %.3f' % (k, scale, np.mean(x > 8), np.mean(x < -8)))
    assert np.mean(x > 8) > 0.25
    Po, Qo = P0.copy(), Q0.copy()
    nll_o = [orc.bpr_sequential(Po, Qo, ev_u, data['ev_i'], js[ep], 0.02, 0.01, 0.01) for ep in range(2)]
    assert np.all(np.isfinite(Po)) and np.all(np.isfinite(Qo)) and np.all(np.isfinite(nll_o))
    bad = []
    for name, opts in EPOCH_VARIANTS:
        dev.set_factors(P0, Q0)
        nll = _with_options(dev, dict(opts, epoch_exact=1), lambda: [dev.bpr_epoch(SEED, ep, 0, 0.02, 0.01, 0.01)[0] for ep in range(2)])
        P, Q = dev.get_factors()
        same = np.array_equal(_bits(P), _bits(Po)) and np.array_equal(_bits(Q), _bits(Qo))
        loss_ok = all(abs(a - b) <= 1e-9 * abs(b) for a, b in zip(nll, nll_o))
        print('k=%d %s: bit-equal P %.6f Q %.6f, loss %s vs %s' % (k, name, np.mean(_bits(P) == _bits(Po)), np.mean(_bits(Q) == _bits(Qo)), nll, nll_o))
        if not (same and loss_ok):
            bad.append((name, same, nll, nll_o))
    assert not bad, bad
