"""The oracle's step coefficient against the reference's own expression, at the margins tests/test_gpu_exact_numerics.py
sweeps on the device: c = fp32(lr (1 - 1 / (1 + exp(-x)))) with glibc's exp (math.exp), read from the factors through the
k = 2 construction of tests/helpers/margin_sweep.py.  This pins oracle/bpr_oracle.c:coef to the reference exactly where the
device's coefficient is checked against the oracle."""
import numpy as np
import pytest

from helpers import margin_sweep as ms

LRS = (0.02, 0.5 + 2.0 ** -25 + 2.0 ** -53)


def _oracle_coefficients(orc, x, lr):
    P, Q, u, i, j, rows = ms.stream(x, 1)
    orc.bpr_sequential(P, Q, u, i, j, lr, 0.0, 0.0)
    # the construction: the positive row's element 1 is c, the negative row's is -c (+0 for c = 0), the user row keeps its 1
    assert np.array_equal(Q[j, 1], -Q[rows, 1])
    assert np.all(P[:, 1] == 1.0) and np.all(Q[rows, 0] == np.float32(1.0) + Q[rows, 1] * (x + Q[rows, 1]))
    return Q[rows, 1]


@pytest.mark.parametrize('lr', LRS)
@pytest.mark.parametrize('which', ['cancellation sample', 'log-uniform', 'edges'])
def test_oracle_coefficient_is_the_reference_expression(orc, which, lr):
    if which == 'cancellation sample':
        band = ms.cancellation_band()
        x = band[np.random.RandomState(3).choice(len(band), 1 << 19, replace=False)]
    elif which == 'log-uniform':
        x = ms.log_uniform()
    else:
        x = ms.edge_margins()
    c = _oracle_coefficients(orc, x, lr)
    ref = np.array([ms.reference_coefficient(v, lr) for v in x.tolist()], np.float32)
    bad = np.nonzero(c.view(np.uint32) != ref.view(np.uint32))[0]
    assert len(bad) == 0, [(float(x[t]), float(c[t]), float(ref[t])) for t in bad[:10]]
