"""Margin sets and the k = 2 triplet stream that exposes the step coefficient c = fp32(lr (1 - sigmoid(x))) of every triplet
(tests/test_gpu_exact_numerics.py, tests/test_oracle_coefficient.py).

Construction (regU = regI = 0): user row P[u] = (x, 1), positive row (1, 0), negative row (0, 0).  The margin is exactly x on
both sides (dot64 of (x, 1) . (1, 0) minus 0), and after the step the positive row's second element is c and the negative's
is -c, exactly.  With two triplets per user the second pair of item rows sees the margin fl(x + c1)."""
import math

import numpy as np

FLT_MIN = float(np.finfo(np.float32).tiny)
FLT_MAX = float(np.finfo(np.float32).max)


def cancellation_band():
    """Set 1: EVERY fp32 value in [8, 32) (2^24 values): 1 - s is a cancellation, a last-bit change of s moves c."""
    return np.arange(0x41000000, 0x42000000, dtype=np.uint32).view(np.float32)


def log_uniform(count=1 << 22, seed=20261016):
    """Set 2: |x| log-uniform in [2^-40, 700], both signs."""
    rs = np.random.RandomState(seed)
    mag = np.exp(rs.uniform(math.log(2.0 ** -40), math.log(700.0), size=count)).astype(np.float32)
    mag = np.minimum(mag, np.float32(700.0))
    return np.where(rs.rand(count) < 0.5, -mag, mag).astype(np.float32)


def edge_margins():
    """Set 3: signed zeros, the smallest normal, +-2^-53 .. 2^-50 (1 + e^-x has an all-ones significand: the weak case of a
    Newton-corrected reciprocal), both neighbours of +-700 (where chain_sigmoid switches to the library exp), +-745, +-1e30,
    +-FLT_MAX."""
    v = [0.0, -0.0, FLT_MIN, -FLT_MIN]
    for e in range(-53, -49):
        v += [2.0 ** e, -2.0 ** e]
    for a in (700.0, -700.0):
        f = np.float32(a)
        v += [float(np.nextafter(f, np.float32(-np.inf))), a, float(np.nextafter(f, np.float32(np.inf)))]
    v += [745.0, -745.0, 1e30, -1e30, FLT_MAX, -FLT_MAX]
    return np.array(v, np.float32)


def margin_sets():
    return [('cancellation [8, 32)', cancellation_band()), ('log-uniform', log_uniform()), ('edges', edge_margins())]


def stream(x, per_user):
    """Factors and triplets for the margins x: one user per margin, per_user (1 or 2) independent triplets per user, each on
    a fresh pair of item rows.  Returns P, Q, u, i, j and c_rows: the item rows whose element 1 is the triplets' c (in stream order)."""
    x = np.ascontiguousarray(x, np.float32)
    T = len(x)
    P = np.zeros((T, 2), np.float32)
    P[:, 0] = x
    P[:, 1] = 1.0
    Q = np.zeros((2 * per_user * T, 2), np.float32)
    Q[0::2, 0] = 1.0
    u = np.repeat(np.arange(T, dtype=np.int32), per_user)
    i = np.arange(0, 2 * per_user * T, 2, dtype=np.int32)
    j = i + 1
    return P, Q, u, i, j, i


def reference_coefficient(x, lr):
    """The reference's expression (tool/qmath.py sigmoid on the fp32 margin, BPR.py's lr * (1 - s)) with glibc's exp through
    math.exp; an exp that overflows is +inf, as the C library returns it (Python raises instead)."""
    try:
        e = math.exp(-float(x))
    except OverflowError:
        e = math.inf
    return np.float32(lr * (1 - 1 / (1 + e)))
