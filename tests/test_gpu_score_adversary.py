"""GPU: the scoring pre-filter at the edge of its bf16 error bound.

Every ranking list for k in {16, 32, 64, 128} passes a bf16 MFMA pre-filter that keeps a (user, item) pair for the exact chain
only if  bf16 score + 1.01 * 2^-7 ||P_u|| max||Q_tile|| > threshold_u  (score_kernels.hpp, score2_kernels.hpp).  On the iid
inputs of test_gpu_score.py the rounding errors cancel and the margin is never needed; on the factors of
tests/helpers/bf16_adversary.py the lists are only right with at least 0.95 .. 0.99 of it, with the norm of the RIGHT tile and
the suffix maximum of the RIGHT position (tests/test_score_adversary.py states that on the CPU).  Lists AND scores must equal
the oracle's in every form of every bf16 kernel.  tools/scan_margin_probe.py shows once (profiles/r08_scan_margin_probe.txt)
that a library built with 0.90 of the bound fails these comparisons in every form."""
import numpy as np
import pytest

from helpers import bf16_adversary as adv

pytestmark = pytest.mark.gpu

_ID = lambda v: str(v) if not isinstance(v, tuple) else 'N' + '-'.join(map(str, v))


@pytest.fixture(scope='module')
def dev():
    from yue_amd._shim import Device
    d = Device(0, raise_errors=True)
    yield d
    d.close()


_oracle_cache = {}


def _oracle(orc, key, P, Q, users, N, mp, mi, true_topn=0):
    """The C oracle once per (data set, N, mode): the kernel forms are looped over inside the tests."""
    key = key + (N, true_topn)
    if key not in _oracle_cache:
        oid, osc, rc = (orc.topn_true if true_topn else orc.topn_scan)(P, Q, users, N, mp, mi)
        assert rc == 0
        _oracle_cache[key] = (oid, osc)
    return _oracle_cache[key]


class _options:
    def __init__(self, dev, **opts):
        self.dev, self.opts = dev, opts

    def __enter__(self):
        self.old = {k: self.dev.get_option(k) for k in self.opts}
        for k, v in self.opts.items():
            self.dev.set_option(k, v)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            self.dev.set_option(k, v)


@pytest.mark.parametrize('fam,n,k,ns', adv.fused_cases(), ids=_ID)
def test_fused_kernels_on_adversarial_factors(dev, orc, fam, n, k, ns):
    """n < 16,384: k_topn_scan_bf16p (scan_batch 0), k_topn_scan_bf16 (scan_batch 1) and the f32 kernel as the control."""
    m = adv.M_FUSED
    P, Q, mp, mi = adv.make(fam, m, n, k)
    users = np.arange(m, dtype=np.int32)
    dev.set_factors(P, Q)
    for N in ns:
        oid, osc = _oracle(orc, (fam, n, k, m), P, Q, users, N, mp, mi)
        for batch, f32 in ((0, 0), (1, 0), (0, 1)):
            with _options(dev, scan_batch=batch, scan_f32=f32):
                ids, sc = dev.topn_scan(users, N, mp, mi)
                ms, events, rescored, used_bf16 = dev.scan_stats()
            assert used_bf16 == (not f32), (fam, n, k, N, batch, f32)
            assert events >= m * N and (f32 or rescored >= events), (fam, n, k, N, batch, f32, events, rescored)
            assert np.array_equal(ids, oid) and np.array_equal(sc, osc), (fam, n, k, N, batch, f32, int((ids != oid).any(axis=1).sum()))


@pytest.mark.parametrize('fam,n,k,ns', adv.two_phase_cases() + adv.long_cases(), ids=_ID)
def test_two_phase_path_on_adversarial_factors(dev, orc, fam, n, k, ns):
    """n >= 16,384: the first 512 items through k_topn_scan_bf16p, the rest through k_scan_filter (all three forms) and
    k_scan_select; overwrite scan and true top-N.  Chunk-start thresholds of growth 2 and of the automatic choice at n = 16,485
    (`under`: both in every form), of growth 64 on the long catalogues (chunks 512 .. 32,768 .. n)."""
    m = adv.M_LONG if n == adv.N_LONG else adv.M_TWO_PHASE
    P, Q, mp, mi = adv.make(fam, m, n, k)
    users = np.arange(m, dtype=np.int32)
    dev.set_factors(P, Q)
    for q, N in enumerate(ns):
        for true_topn in (0, 1):
            oid, osc = _oracle(orc, (fam, n, k, m), P, Q, users, N, mp, mi, true_topn)
            for ub in (3, 2, 1):
                growths = (64,) if n == adv.N_LONG else (0, 2) if fam == 'under' else ((0, 2)[(ub + q + true_topn) % 2],)
                for growth in growths:
                    with _options(dev, scan_filter_ub=ub, scan_growth=growth, topn_true=true_topn):
                        ids, sc = dev.topn_scan(users, N, mp, mi)
                        chunks, settle = dev.get_option('scan_last_chunks'), dev.get_option('scan_last_settle')
                        ms, events, rescored, used_bf16 = dev.scan_stats()
                    what = (fam, n, k, N, true_topn, ub, growth)
                    assert chunks >= 2 and used_bf16 and rescored >= events >= m * N, what + (chunks, events, rescored)
                    if fam in ('settling', 'under'):
                        assert settle == (1 if fam == 'settling' else 0), what
                    assert np.array_equal(ids, oid) and np.array_equal(sc, osc), what + (int((ids != oid).any(axis=1).sum()),)


def test_two_phase_slabs_with_an_explicit_mask_on_adversarial_rows(dev, orc):
    """More users than scan_streams_min_users (lowered to 1,024): slabs on two streams, the explicit mask's row pointer shifted per
    slab.  256 distinct adversarial user rows, each listed several times under its own mask row."""
    fam, n, k, N, m = 'mixed', adv.N_TWO_PHASE, 64, 20, adv.M_TWO_PHASE
    P, Q, indptr, indices = adv.make(fam, m, n, k)
    base = np.arange(m, dtype=np.int32)
    oid, osc = _oracle(orc, (fam, n, k, m), P, Q, base, N, indptr, indices)
    users = ((np.arange(1100) * 37) % m).astype(np.int32)
    rows = [indices[indptr[u]:indptr[u + 1]] for u in users]
    mp, mi = adv._csr(rows)
    dev.set_factors(P, Q)
    for slabs in (2, 7):
        with _options(dev, scan_streams_min_users=1024, scan_slabs=slabs, scan_streams=2):
            ids, sc = dev.topn_scan(users, N, mp, mi)
            assert dev.get_option('scan_last_chunks') >= 2
        assert np.array_equal(ids, oid[users]) and np.array_equal(sc, osc[users]), slabs


def test_heavy_listener_takes_the_fused_pass_over_adversarial_rows(orc):
    """Two users have listened to nearly all of the first 512 items: with the training CSR as the mask they alone go through the
    fused kernel over ALL items (n >= 16,384 there too), the others through the filter / select pair."""
    from yue_amd._shim import Device
    fam, n, k, N, m = 'under', adv.N_TWO_PHASE, 128, 20, adv.M_TWO_PHASE
    P, Q, _, _ = adv.make(fam, m, n, k)
    rows = [np.zeros(0, np.int32) for _ in range(m)]
    rows[7] = np.setdiff1d(np.arange(600, dtype=np.int32), np.array([3, 100, 511], np.int32))
    rows[200] = np.arange(512, dtype=np.int32)
    indptr, indices = adv._csr(rows)
    users = np.arange(m, dtype=np.int32)
    oid, osc, rc = orc.topn_scan(P, Q, users, N, indptr, indices)
    assert rc == 0
    d = Device(0, raise_errors=True)
    try:
        d.set_factors(P, Q)
        d.set_interactions(indptr, indices, indptr, indices)        # (events = the listened items: only the mask matters here)
        ids, sc = d.topn_scan(users, N)
        assert d.get_option('scan_last_chunks') >= 2 and d.get_option('scan_last_few_users') == 2
    finally:
        d.close()
    assert np.array_equal(ids, oid) and np.array_equal(sc, osc)


@pytest.mark.parametrize('fam,n,k,N', [('under', 4096, 64, 5), ('spikes', 4099, 16, 20), ('under', adv.N_TWO_PHASE, 128, 20), ('settling', adv.N_TWO_PHASE, 32, 5)])
def test_power_of_two_rescaling_changes_nothing_but_the_exponent(dev, orc, fam, n, k, N):
    """P * 2^a and Q * 2^b: every product, sum, norm, margin and threshold scales exactly (all squared norms stay normal fp32
    numbers at these scales: DESIGN.md section 7), so the ids must not change and the scores must be 2^(a+b) times the unscaled
    ones, bit for bit -- in the fused kernels (both batch forms) and along the two-phase path."""
    m = adv.M_FUSED if n < 16384 else adv.M_TWO_PHASE
    P, Q, mp, mi = adv.make(fam, m, n, k)
    users = np.arange(m, dtype=np.int32)
    oid, osc = _oracle(orc, (fam, n, k, m), P, Q, users, N, mp, mi)
    for a, b in ((0, 0), (-20, 0), (0, 20), (-30, 30), (12, 12)):
        Ps, Qs = P * np.float32(2.0 ** a), Q * np.float32(2.0 ** b)
        assert np.isfinite(Qs).all() and ((Ps.astype(np.float64) ** 2).sum(1) > 1e-37).all() and ((Qs.astype(np.float64) ** 2).sum(1) > 1e-37).all()
        dev.set_factors(Ps, Qs)
        for batch in ((0, 1) if n < 16384 else (0,)):
            with _options(dev, scan_batch=batch):
                ids, sc = dev.topn_scan(users, N, mp, mi)
                assert dev.scan_stats()[3] and (dev.get_option('scan_last_chunks') >= 2) == (n >= 16384)
            assert np.array_equal(ids, oid), (fam, n, k, a, b, batch)
            assert np.array_equal(sc, osc * np.float32(2.0 ** (a + b))), (fam, n, k, a, b, batch)
