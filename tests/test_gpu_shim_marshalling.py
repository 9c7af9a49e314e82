"""The shim's argument handling on a device, at m = 5, n = 3, k = 4: inputs of another dtype or order are converted as
before, the assertions still come before any call, NULL pointers and the empty-list placeholder reach the library, and the
statuses the shim turns into IndexError still do."""
import numpy as np
import pytest

from oracle.numpy_fism import fism_scores, overwrite_scan

pytestmark = pytest.mark.gpu

M, N_ITEMS, K = 5, 3, 4


@pytest.fixture
def dev():
    from yue_amd._shim import Device
    d = Device(0, raise_errors=True)
    yield d
    d.close()


def factors():
    # small integers: every score is exact in float32, and no two items of a user tie
    P = (np.arange(M * K).reshape(M, K) % 7 - 3).astype(np.float32)
    Q = np.array([[1, 0, 0, 0], [0, 3, 1, 0], [2, 1, 0, 4]], np.float32)
    S = P.dot(Q.T)
    assert all(len(set(row)) == N_ITEMS for row in S.tolist())
    return P, Q, S


def test_set_factors_converts_dtype_and_order(dev):
    P, Q, _ = factors()
    dev.set_factors(P.astype(np.float64), np.asfortranarray(Q))
    Pd, Qd = dev.get_factors()
    for got, want in ((Pd, P), (Qd, Q)):
        assert got.dtype == np.float32 and got.flags.c_contiguous and np.array_equal(got, want)


def test_get_factors_asserts_before_any_call(dev):
    P, Q, _ = factors()
    dev.set_factors(P, Q)

    class NoCalls(object):
        def __getattr__(self, name):
            raise RuntimeError('the shim called ' + name)
    lib, dev._lib = dev._lib, NoCalls()
    try:
        with pytest.raises(AssertionError):
            dev.get_factors(P=np.empty((M, K), np.float64))
        with pytest.raises(AssertionError):
            dev.get_factors(Q=np.empty((K, N_ITEMS), np.float32).T)
    finally:
        dev._lib = lib
    assert np.array_equal(dev.get_factors()[0], P)


def test_adam_moments_come_back_in_four_arrays(dev):
    P, Q, _ = factors()
    dev.set_factors(P, Q)
    dev.adam_reset()
    moments = dev.adam_get_moments()
    assert [x.shape for x in moments] == [(M, K), (M, K), (N_ITEMS, K), (N_ITEMS, K)]
    assert all(x.dtype == np.float32 and not x.any() for x in moments)          # yue_adam_reset clears them


def test_topn_scan_without_a_mask_and_with_an_empty_one(dev):
    P, Q, S = factors()
    dev.set_factors(P, Q)
    own = np.arange(M) % N_ITEMS                                                # one training item per user
    ptr = np.arange(M + 1, dtype=np.int64)
    dev.set_interactions(ptr, own.astype(np.int32), ptr, own.astype(np.int32))
    users = np.arange(M, dtype=np.int32)
    for masked, call in (([[i] for i in own], lambda: dev.topn_scan(users, 2)),                       # NULL mask: the training items
                         ([[]] * M, lambda: dev.topn_scan(users, 2, np.zeros(M + 1, np.int64), []))):    # nothing masked
        ids, sc = call()
        assert ids.dtype == np.int32 and sc.dtype == np.float32 and ids.shape == sc.shape == (M, 2)
        for u in range(M):
            want_ids, want_sc = overwrite_scan(S[u], masked[u], 2)
            assert ids[u].tolist() == want_ids and sc[u].tolist() == want_sc, (u, masked[u])


def test_topn_scan_with_too_few_candidates_is_an_index_error(dev):
    P, Q, _ = factors()
    dev.set_factors(P, Q)
    with pytest.raises(IndexError) as err:
        dev.topn_scan(np.arange(M, dtype=np.int32), N_ITEMS + 1, np.zeros(M + 1, np.int64), [])
    assert err.value.args == ('list index out of range',)


def test_fism_scores_of_an_empty_row(dev):
    rs = np.random.RandomState(2)
    P, Q, Bi = rs.standard_normal((N_ITEMS, K)), rs.standard_normal((N_ITEMS, K)).astype(np.float32), rs.standard_normal(N_ITEMS)
    dev.fism_set_model(P, Q, Bi)
    got, want = dev.fism_scores([]), fism_scores(P, Q, Bi, [])
    assert got.shape == (N_ITEMS,) and got.dtype == np.float64
    assert np.abs(got - want).max() < 1e-12 * np.abs(want).max()                # (the bound of tests/test_gpu_fism.py)
