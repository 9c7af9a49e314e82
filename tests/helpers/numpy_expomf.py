"""NumPy oracles of ExpoMF (recommender/advanced/ExpoMF.py; device: yue_expo_*, DESIGN.md section "ExpoMF").

expo_reference_form        the reference's statements at its dtypes (fp32 factors and posterior, fp32 BLAS Gram, int64
                           counts times fp32 = fp64 right-hand side, fp64 solve, rows rounded to fp32 on assignment, batches
                           of 300 rows), for the CPU pin against the g13 fixtures.
expo_half_sweep_contract   the device contract of one half-sweep: everything in fp64 from the fp32 inputs, the row rounded to
                           fp32 once, rows without pairs exactly 0.  Any subset of rows can be computed.
expo_mu_contract           the exposure prior: column sums of the posterior in fp64, the mu formula in fp64, rounded to fp32 once.

Posterior of row r over every column j (s = f_old[r] . F[j]):
    pEX = sqrt(lam_y * pi / 2) * exp(-lam_y * s^2 / 2)        (the reference's constant, not the normal density's)
    A   = (pEX + 1e-8) / (pEX + 1e-8 + (1 - mu) / mu),  A = 1 on the row's pairs
mu is indexed by the column (mu_per_column: the user side always, and the item side when m == n -- the reference tells the
sides apart by mu.size == X.shape[0]) or by the row (the item side otherwise).
"""
from math import sqrt

import numpy as np

EPS = 1e-8
BATCH = 300
LAM_THETA = LAM_BETA = 1e-5
LAM_Y = 1.0
INIT_MU = 0.01
PRIOR_A = 1.0
PRIOR_B = 99.0


def _posterior_ref(F_old_batch, F, lam_y, mu, ptr, idx, lo):
    pEX = sqrt(lam_y / 2 * np.pi) * np.exp(-lam_y * F_old_batch.dot(F.T) ** 2 / 2)
    A = (pEX + EPS) / (pEX + EPS + (1 - mu) / mu)
    for t in range(A.shape[0]):
        A[t, idx[ptr[lo + t]:ptr[lo + t + 1]]] = 1.
    return A


def _recompute_ref(F, F_old, ptr, idx, cnt, lam, lam_y, mu):
    nr, k = F_old.shape
    out = np.empty_like(F_old)
    for lo in range(0, nr, BATCH):
        hi = min(lo + BATCH, nr)
        if mu.size == F.shape[0]:
            A = _posterior_ref(F_old[lo:hi], F, lam_y, mu, ptr, idx, lo)
        else:
            A = _posterior_ref(F_old[lo:hi], F, lam_y, mu[lo:hi, np.newaxis], ptr, idx, lo)
        for t, r in enumerate(range(lo, hi)):
            ids = idx[ptr[r]:ptr[r + 1]]
            rhs = np.dot(cnt[ptr[r]:ptr[r + 1]].astype(np.int64) * A[t][ids], F[ids])
            B = F.T.dot(A[t][:, np.newaxis] * F) + lam * np.eye(k)
            out[t + lo] = np.linalg.solve(B, rhs)
    return out


def expo_reference_form(theta, beta, mu, user_major, item_major, iters, lam_theta=LAM_THETA, lam_beta=LAM_BETA, lam_y=LAM_Y,
                        a=PRIOR_A, b=PRIOR_B):
    """user_major / item_major = (ptr, ids, counts).  Returns (thetas, betas, mus) after every iteration (fp32)."""
    up, ui, uc = user_major
    ip, iu, ic = item_major
    m = theta.shape[0]
    thetas, betas, mus = [], [], []
    for _ in range(iters):
        theta = _recompute_ref(beta, theta, up, ui, uc, lam_theta / lam_y, lam_y, mu)
        beta = _recompute_ref(theta, beta, ip, iu, ic, lam_beta / lam_y, lam_y, mu)
        A_sum = np.zeros_like(mu)
        for lo in range(0, m, BATCH):
            hi = min(lo + BATCH, m)
            A_sum += _posterior_ref(theta[lo:hi], beta, lam_y, mu, up, ui, lo).sum(axis=0)
        mu = (a + A_sum - 1) / (a + b + m - 2)
        thetas.append(theta.copy())
        betas.append(beta.copy())
        mus.append(mu.copy())
    return thetas, betas, mus


def posterior64(s, ratio, lam_y):
    pex = sqrt(lam_y * np.pi / 2.0) * np.exp(-lam_y * s * s / 2.0)
    return (pex + EPS) / (pex + EPS + ratio)


def expo_half_sweep_contract(F, F_old, ptr, idx, cnt, mu, mu_per_column, lam, lam_y, rows=None):
    """Rows (all by default) of the solved side from the fixed side F (fp32 [nf, k]) and the rows' old values F_old (fp32
    [nr, k]); mu fp32, one per column of the posterior (mu_per_column) or one per row.  Returns fp32 [len(rows), k]."""
    nr, k = F_old.shape
    rows = np.arange(nr) if rows is None else np.asarray(rows)
    F64 = F.astype(np.float64)
    mu64 = np.asarray(mu, np.float32).astype(np.float64)
    ratio = (1.0 - mu64) / mu64
    assert len(mu64) == (F.shape[0] if mu_per_column else nr)
    out = np.zeros((len(rows), k), np.float32)
    for t, r in enumerate(rows):
        p0, p1 = int(ptr[r]), int(ptr[r + 1])
        if p0 == p1:
            continue
        ids = idx[p0:p1]
        A = posterior64(F64 @ F_old[r].astype(np.float64), ratio if mu_per_column else ratio[r], lam_y)
        A[ids] = 1.0
        B = (F64.T * A) @ F64 + lam * np.eye(k)
        rhs = cnt[p0:p1].astype(np.float64) @ F64[ids]
        L = np.linalg.cholesky(B)
        out[t] = np.linalg.solve(L.T, np.linalg.solve(L, rhs)).astype(np.float32)
    return out


def expo_mu_contract(theta, beta, u_ptr, u_items, mu, a, b, lam_y, items=None):
    """mu after the exposure-prior update (fp32 [n], or the given items): A_sum[i] = sum over all users of A_ui."""
    m, n = theta.shape[0], beta.shape[0]
    items = np.arange(n) if items is None else np.asarray(items)
    T64 = theta.astype(np.float64)
    B64 = beta[items].astype(np.float64)
    mu64 = np.asarray(mu, np.float32).astype(np.float64)[items]
    ratio = (1.0 - mu64) / mu64
    pos = np.full(n, -1, np.int64)
    pos[items] = np.arange(len(items))
    A_sum = np.zeros(len(items))
    for lo in range(0, m, 1024):
        hi = min(lo + 1024, m)
        A = posterior64(T64[lo:hi] @ B64.T, ratio[None, :], lam_y)
        for u in range(lo, hi):
            cols = pos[u_items[u_ptr[u]:u_ptr[u + 1]]]
            A[u - lo, cols[cols >= 0]] = 1.0
        A_sum += A.sum(axis=0)
    return ((a + A_sum - 1.0) / (a + b + m - 2.0)).astype(np.float32)


def expo_iteration_contract(theta, beta, mu, user_major, item_major, lam_theta=LAM_THETA, lam_beta=LAM_BETA, lam_y=LAM_Y,
                            a=PRIOR_A, b=PRIOR_B, item_mu_per_column=None):
    """One iteration of the contract: theta from beta, beta from the new theta, mu from both.  item_mu_per_column
    defaults to the reference's rule (m == n)."""
    up, ui, uc = user_major
    ip, iu, ic = item_major
    m, n = theta.shape[0], beta.shape[0]
    if item_mu_per_column is None:
        item_mu_per_column = m == n
    theta = expo_half_sweep_contract(beta, theta, up, ui, uc, mu, True, lam_theta / lam_y, lam_y)
    beta = expo_half_sweep_contract(theta, beta, ip, iu, ic, mu, item_mu_per_column, lam_beta / lam_y, lam_y)
    mu = expo_mu_contract(theta, beta, up, ui, mu, a, b, lam_y)
    return theta, beta, mu


def rel(a, b):
    """max |a - b| / max |b|"""
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64)).max() / np.abs(np.asarray(b, np.float64)).max())


def overwrite_scan(scores, masked, N, err=None):
    """The reference's evalRanking selection for one user (base/IterativeRecommender.py: seed with the first N candidates,
    then the overwrite-scan), on a score vector in item-id order.  Returns (ids, margin): margin is the smallest, over every
    pair of scores the scan compared, of |s_i - s_j| - err_i - err_j (err: a bound on how far each score may move; zeros when
    None).  While the margin is positive no comparison can come out differently, so the list cannot either.  Two scores that
    are equal and both exact (err 0: zero rows) compare the same way on both sides and are left out."""
    err = np.zeros(len(scores)) if err is None else err
    cand = [i for i in range(len(scores)) if i not in masked]
    seed = sorted(cand[:N], key=lambda i: -scores[i])          # stable, as list.sort(reverse=True)
    rec = [scores[i] for i in seed]
    ids = list(seed)
    margin = [np.inf]

    def seen(i, j):
        if i != j and not (err[i] == 0 and err[j] == 0 and scores[i] == scores[j]):
            margin[0] = min(margin[0], abs(float(scores[i]) - float(scores[j])) - err[i] - err[j])
    for a_ in range(len(seed)):
        for b_ in range(a_ + 1, len(seed)):
            seen(ids[a_], ids[b_])
    for i in cand:
        s = scores[i]
        ind, lo, hi = N, 0, N - 1
        seen(i, ids[hi])
        if rec[hi] < s:
            while True:
                mid = (lo + hi) // 2
                seen(i, ids[mid])
                if rec[mid] >= s:
                    lo = mid + 1
                else:
                    hi = mid - 1
                if hi < lo:
                    ind = hi
                    break
        if ind < N - 1:
            rec[ind + 1] = s
            ids[ind + 1] = i
    return ids, float(margin[0])


def score_error(T_ref, B_ref, T_con, B_con, u):
    """How far a score of user u may move on a device that is as close to the contract as the reference is, times 4 (the
    factor of every device bound): 4 * max_i |s_ref(u, i) - s_contract(u, i)|, plus the rounding of the fp32 dot product itself
    (2 ulp-sized terms of sum |theta| |beta|: NumPy's dot against the device's fma chain).  Scores of exact zero rows are exact."""
    t64, B64 = T_ref[u].astype(np.float64), B_ref.astype(np.float64)
    d = np.abs(B64 @ t64 - B_con.astype(np.float64) @ T_con[u].astype(np.float64))
    err = 4.0 * d.max() + 2 * 6e-8 * (np.abs(B64) @ np.abs(t64))
    err[~B_ref.any(axis=1)] = 0.0
    if not T_ref[u].any():
        err[:] = 0.0
    return err


def init_from_seed(seed, m, n, k):
    """theta0, beta0 as initModel draws them after np.random.seed(seed): the base class's P and Q first, then the two randn."""
    rs = np.random.RandomState(seed)
    rs.rand(m, k)
    rs.rand(n, k)
    theta = 0.01 * rs.randn(m, k).astype(np.float32)
    beta = 0.01 * rs.randn(n, k).astype(np.float32)
    return theta, beta


def c2_inputs(seed, m=100000, n=50000, d=50, k=64):
    """The large shape (bench.py --workload c2, two items thinned out) with seeded factors: theta, beta = 0.01 * randn (fp32), mu uniform in
    [0.005, 0.05) (fp32), the distinct pairs both ways."""
    from helpers.numpy_wrmf import pairs_from_events
    from yue_amd import synth
    data = synth.make_arrays(m, n, d)
    ev_u = np.repeat(np.arange(m, dtype=np.int32), np.diff(data['ev_ptr']))
    ev_i = data['ev_i']
    # the log itself has no item with fewer than a few dozen listeners: item n-1 loses all its events and item n-2 all but
    # its first, so that the shape holds a row without pairs and a row with one pair
    keep = ev_i != n - 1
    keep[np.flatnonzero(ev_i == n - 2)[1:]] = False
    um, im = pairs_from_events(ev_u[keep], ev_i[keep], m, n)
    rs = np.random.RandomState(seed)
    theta = (0.01 * rs.randn(m, k)).astype(np.float32)
    beta = (0.01 * rs.randn(n, k)).astype(np.float32)
    mu = (0.005 + 0.045 * rs.rand(n)).astype(np.float32)
    return {'m': m, 'n': n, 'k': k, 'theta': theta, 'beta': beta, 'mu': mu, 'user_major': um, 'item_major': im}


def c2_sample(seed, u_ptr, i_ptr, count=256):
    """256 users and 256 items: the 16 heaviest users, the 16 most popular items, one item without pairs and one with a
    single pair, the rest drawn from a seeded stream."""
    rs = np.random.RandomState(seed + 1)
    lu, li = np.diff(u_ptr), np.diff(i_ptr)
    users = list(np.argsort(-lu, kind='stable')[:16])
    items = list(np.argsort(-li, kind='stable')[:16]) + [int(np.flatnonzero(li == 0)[0]), int(np.flatnonzero(li == 1)[0])]
    for chosen, size in ((users, len(lu)), (items, len(li))):
        for x in rs.permutation(size):
            if len(chosen) == count:
                break
            if x not in chosen[:18]:
                chosen.append(int(x))
    return np.sort(np.array(users, np.int64)), np.sort(np.array(items, np.int64))
