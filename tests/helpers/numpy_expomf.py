"""NumPy oracles of ExpoMF (recommender/advanced/ExpoMF.py; device: yue_expo_*, DESIGN.md section "ExpoMF").

expo_reference_form        the reference's statements at its dtypes (fp32 factors and posterior, fp32 BLAS Gram, int64
                           counts times fp32 = fp64 right-hand side, fp64 solve, rows rounded to fp32 on assignment, batches
                           of 300 rows), for the CPU pin against the g13 fixtures.
expo_half_sweep_contract   the device contract of one half-sweep: everything in fp64 from the fp32 inputs, the row rounded to
                           fp32 once, rows without pairs exactly 0.  Any subset of rows can be computed.
expo_mu_contract           the exposure prior: column sums of the posterior in fp64, the mu formula in fp64, rounded to fp32 once.
expo_gram_contract         the dense stage alone (device: yue_expo_gram_rows): per row the packed lower triangle of
                           sum over all columns of A~ f f^T in fp64, no A = 1 on the pairs.
trained_case / TRAINED     seeded inputs at trained scale (scores of standard deviation 1.5, mu up to 0.3), where the posterior
                           varies from column to column, and the cases tests/test_gpu_expomf_stages.py runs; their e_ref
                           (trained_e_ref: the reference's arithmetic against the contract on the same inputs) is stored in
                           tests/golden/g13_expomf_trained.json by tools/make_expomf_goldens.py.
dense_defect=              named mutants of the contracts' DENSE posterior (never of the pairs' correction or the right-hand
                           side): what tests/test_expomf_power.py uses to show that a case would notice a wrong dense stage.

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


def _posterior_ref_rows(F_old, F, lam_y, mu, mu_per_column, rows):
    """_posterior_ref's fp32 arithmetic for a list of rows, without the A = 1 overwrite."""
    pEX = sqrt(lam_y / 2 * np.pi) * np.exp(-lam_y * F_old[rows].dot(F.T) ** 2 / 2)
    m_ = mu if mu_per_column else mu[rows, np.newaxis]
    return (pEX + EPS) / (pEX + EPS + (1 - m_) / m_)


def expo_reference_rows(F, F_old, ptr, idx, cnt, lam, lam_y, mu, mu_per_column, rows=None):
    """_recompute_ref's statements (the reference's dtypes) for a list of rows, in batches of 300 of the list; rows without
    pairs come out 0, as the reference's solve of a zero right-hand side gives them."""
    nr, k = F_old.shape
    rows = np.arange(nr) if rows is None else np.asarray(rows)
    out = np.zeros((len(rows), k), np.float32)
    for lo in range(0, len(rows), BATCH):
        sel = rows[lo:lo + BATCH]
        A = _posterior_ref_rows(F_old, F, lam_y, mu, mu_per_column, sel)
        for t, r in enumerate(sel):
            ids = idx[ptr[r]:ptr[r + 1]]
            A[t, ids] = 1.
            rhs = np.dot(cnt[ptr[r]:ptr[r + 1]].astype(np.int64) * A[t][ids], F[ids])
            B = F.T.dot(A[t][:, np.newaxis] * F) + lam * np.eye(k)
            out[lo + t] = np.linalg.solve(B, rhs)
    return out


def expo_reference_gram(F, F_old, lam_y, mu, mu_per_column, rows):
    """The reference's arithmetic for the dense stage alone: fp32 posterior (no overwrite), fp32 F.T.dot(A[:, None] * F),
    as the packed lower triangle (fp32 [len(rows), k(k+1)/2])."""
    rows = np.asarray(rows)
    k = F.shape[1]
    il = np.tril_indices(k)
    out = np.empty((len(rows), len(il[0])), np.float32)
    for lo in range(0, len(rows), BATCH):
        A = _posterior_ref_rows(F_old, F, lam_y, mu, mu_per_column, rows[lo:lo + BATCH])
        for t in range(A.shape[0]):
            out[lo + t] = F.T.dot(A[t][:, np.newaxis] * F)[il]
    return out


def expo_reference_mu(theta, beta, mu, u_ptr, u_items, a, b, items=None):
    """The reference's exposure-prior update (expo_reference_form's last statements) for all items or a list of them."""
    m, n = theta.shape[0], beta.shape[0]
    items = np.arange(n) if items is None else np.asarray(items)
    pos = np.full(n, -1, np.int64)
    pos[items] = np.arange(len(items))
    mu_s = mu[items]
    A_sum = np.zeros_like(mu_s)
    for lo in range(0, m, BATCH):
        hi = min(lo + BATCH, m)
        pEX = sqrt(LAM_Y / 2 * np.pi) * np.exp(-LAM_Y * theta[lo:hi].dot(beta[items].T) ** 2 / 2)
        A = (pEX + EPS) / (pEX + EPS + (1 - mu_s) / mu_s)
        for u in range(lo, hi):
            cols = pos[u_items[u_ptr[u]:u_ptr[u + 1]]]
            A[u - lo, cols[cols >= 0]] = 1.
        A_sum += A.sum(axis=0)
    return (a + A_sum - 1) / (a + b + m - 2)


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


DEFECTS = ('zero', 'colswap', 'rowswap', 'scale', 'drop_tail', 'drop_flush', 'ratio_by_row', 'ratio_by_column')
CHUNK, FLUSH = 128, 4                      # the dense kernel's column chunk and chunks per accumulator flush


def defect_applies(defect, nr, nf, mu_per_column, flushes=True):
    """Whether the mutant changes anything on a posterior of nr rows by nf columns."""
    return {'zero': True, 'scale': True, 'colswap': nf >= 2, 'rowswap': nr >= 2, 'drop_tail': nf % CHUNK != 0,
            'drop_flush': flushes and nf % (CHUNK * FLUSH) != 0, 'ratio_by_row': bool(mu_per_column) and nf >= 2,
            'ratio_by_column': not mu_per_column and nr >= 2}[defect]


def _dense_posterior(F64, Fo64, r, ratio, mu_per_column, lam_y, defect):
    """The dense posterior of row r over every column (fp64, no A = 1 overwrite), with the named defect if any:
    zero (scores 0), colswap (column j takes the score of column j^1), rowswap (row r takes the scores of row r^1), scale
    (scores * 1.01), drop_tail (columns past the last whole chunk of 128 contribute nothing), drop_flush (chunks past the
    last whole group of 4 contribute nothing), ratio_by_row / ratio_by_column (mu indexed the other way)."""
    nr, nf = Fo64.shape[0], F64.shape[0]
    assert defect is None or defect in DEFECTS, defect
    rr = r ^ 1 if defect == 'rowswap' and (r ^ 1) < nr else r
    s = F64 @ Fo64[rr]
    if defect == 'zero':
        s = np.zeros_like(s)
    elif defect == 'scale':
        s = s * 1.01
    elif defect == 'colswap':
        j = np.arange(nf) ^ 1
        j[j >= nf] = nf - 1
        s = s[j]
    by_column = mu_per_column != (defect in ('ratio_by_row', 'ratio_by_column'))
    A = posterior64(s, ratio[np.arange(nf) % len(ratio)] if by_column else ratio[r % len(ratio)], lam_y)
    if defect == 'drop_tail':
        A[nf // CHUNK * CHUNK:] = 0.0
    elif defect == 'drop_flush':
        A[nf // (CHUNK * FLUSH) * (CHUNK * FLUSH):] = 0.0
    return A


def expo_gram_contract(F, F_old, mu, mu_per_column, lam_y, rows, dense_defect=None):
    """The dense stage alone: per listed row the packed lower triangle (fp64 [len(rows), k(k+1)/2], entry p(p+1)/2 + q, p >= q)
    of sum over ALL columns j of A~_j f_j f_j^T, A~ the posterior without the A = 1 overwrite; no lam * I."""
    k = F.shape[1]
    F64, Fo64 = F.astype(np.float64), F_old.astype(np.float64)
    mu64 = np.asarray(mu, np.float32).astype(np.float64)
    ratio = (1.0 - mu64) / mu64
    assert len(mu64) == (F.shape[0] if mu_per_column else F_old.shape[0])
    il = np.tril_indices(k)
    out = np.empty((len(rows), len(il[0])))
    for t, r in enumerate(rows):
        A = _dense_posterior(F64, Fo64, int(r), ratio, mu_per_column, lam_y, dense_defect)
        out[t] = ((F64.T * A) @ F64)[il]
    return out


def gram_rel(got, want):
    """Entry-wise distance of packed Grams, each row relative to its own largest entry; the largest over the rows."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float((np.abs(got - want).max(axis=1) / np.abs(want).max(axis=1)).max())


def expo_half_sweep_contract(F, F_old, ptr, idx, cnt, mu, mu_per_column, lam, lam_y, rows=None, dense_defect=None):
    """Rows (all by default) of the solved side from the fixed side F (fp32 [nf, k]) and the rows' old values F_old (fp32
    [nr, k]); mu fp32, one per column of the posterior (mu_per_column) or one per row.  Returns fp32 [len(rows), k].
    dense_defect: a mutant of the dense posterior (DEFECTS); the pairs' correction and the right-hand side stay exact."""
    nr, k = F_old.shape
    rows = np.arange(nr) if rows is None else np.asarray(rows)
    F64 = F.astype(np.float64)
    Fo64 = F_old.astype(np.float64) if dense_defect else None
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
        if dense_defect:                                     # B = dense sum (defective) + pairs' correction (exact) + lam I
            Ad = _dense_posterior(F64, Fo64, int(r), ratio, mu_per_column, lam_y, dense_defect)
            Ad[ids] += 1.0 - A[ids]
            A = Ad
        else:
            A[ids] = 1.0
        B = (F64.T * A) @ F64 + lam * np.eye(k)
        rhs = cnt[p0:p1].astype(np.float64) @ F64[ids]
        L = np.linalg.cholesky(B)
        out[t] = np.linalg.solve(L.T, np.linalg.solve(L, rhs)).astype(np.float32)
    return out


def expo_mu_contract(theta, beta, u_ptr, u_items, mu, a, b, lam_y, items=None, dense_defect=None):
    """mu after the exposure-prior update (fp32 [n], or the given items): A_sum[i] = sum over all users of A_ui.
    dense_defect: a mutant of the dense posterior (rows: users, columns: items, mu per column; the device sums over the users
    in chunks of 128, so drop_tail drops the users past the last whole chunk); the listened entries stay exact."""
    m, n = theta.shape[0], beta.shape[0]
    items = np.arange(n) if items is None else np.asarray(items)
    T64 = theta.astype(np.float64)
    B64 = beta[items].astype(np.float64)
    mu64 = np.asarray(mu, np.float32).astype(np.float64)[items]
    ratio = (1.0 - mu64) / mu64
    pos = np.full(n, -1, np.int64)
    pos[items] = np.arange(len(items))
    A_sum = np.zeros(len(items))
    assert dense_defect is None or (dense_defect in DEFECTS and dense_defect not in ('drop_flush', 'ratio_by_column')), dense_defect
    for lo in range(0, m, 1024):
        hi = min(lo + 1024, m)
        S = T64[lo:hi] @ B64.T
        A = posterior64(S, ratio[None, :], lam_y)
        if dense_defect:
            Sd, rd = S, ratio[None, :]
            if dense_defect == 'zero':
                Sd = np.zeros_like(S)
            elif dense_defect == 'scale':
                Sd = S * 1.01
            elif dense_defect == 'colswap':
                j = np.arange(len(items)) ^ 1
                j[j >= len(items)] = len(items) - 1
                Sd = S[:, j]
            elif dense_defect == 'rowswap':
                u = np.arange(lo, hi) ^ 1
                u[u >= m] = m - 1
                Sd = T64[u] @ B64.T
            elif dense_defect == 'ratio_by_row':
                full = (1.0 - np.asarray(mu, np.float32).astype(np.float64)) / np.asarray(mu, np.float32).astype(np.float64)
                rd = full[np.arange(lo, hi) % n][:, None]
            Ad = posterior64(Sd, rd, lam_y)
            if dense_defect == 'drop_tail':
                Ad[max(m // CHUNK * CHUNK - lo, 0):] = 0.0
        for u in range(lo, hi):
            cols = pos[u_items[u_ptr[u]:u_ptr[u + 1]]]
            cols = cols[cols >= 0]
            if dense_defect:
                Ad[u - lo, cols] += 1.0 - A[u - lo, cols]
            else:
                A[u - lo, cols] = 1.0
        A_sum += (Ad if dense_defect else A).sum(axis=0)
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


# ---- inputs at trained scale ------------------------------------------------------------------------------------------------
# With theta, beta = 0.01 * randn every score is below 4e-3, exp(-s^2 / 2) = 1 - O(1e-5), the posterior is a constant per
# column, and a half-sweep from such factors cannot tell a right dense stage from a wrong one (tests/test_expomf_power.py
# asserts that).  Here the scores have standard deviation 1.5 and reach 7..9, and mu spreads over [0.005, 0.305).

def trained_case(seed, m, n, k, empty=(3, 3), mu_edges=False, score_scale=1.0):
    """Seeded inputs at trained scale.  Pairs: 12 events per user on items 1.., item 0 listened to by min(300, m / 2) users
    (a long row on the item side), `empty` users / items (never item 0) without any pair.  theta, beta =
    sqrt(1.5 * score_scale / sqrt(k)) * randn (fp32), so theta . beta has standard deviation 1.5 * score_scale; mu uniform in
    [0.005, 0.305) (fp32); with mu_edges a tenth of the items take a mu drawn log-uniformly from [1e-6, 1e-2] and another
    tenth one minus such a draw ([0.99, 1 - 1e-6]).  Returns theta, beta, mu, user_major, item_major."""
    from helpers.numpy_wrmf import pairs_from_events
    rs = np.random.RandomState(seed)
    ev_u = np.repeat(np.arange(m, dtype=np.int32), 12)
    ev_i = (rs.randint(1, n, len(ev_u)) if n > 1 else np.zeros(len(ev_u))).astype(np.int32)
    users0 = rs.choice(m, min(300, m // 2), replace=False).astype(np.int32)
    ev_u, ev_i = np.concatenate([ev_u, users0]), np.concatenate([ev_i, np.zeros(len(users0), np.int32)])
    no_u = rs.choice(m, min(empty[0], m - 1), replace=False)
    no_i = 1 + rs.choice(n - 1, min(empty[1], n - 1), replace=False) if n > 1 else np.zeros(0, np.int64)
    keep = ~np.isin(ev_u, no_u) & ~np.isin(ev_i, no_i)
    um, im = pairs_from_events(ev_u[keep], ev_i[keep], m, n)
    sd = sqrt(1.5 * score_scale / sqrt(k))
    theta = (sd * rs.randn(m, k)).astype(np.float32)
    beta = (sd * rs.randn(n, k)).astype(np.float32)
    mu = (0.005 + 0.3 * rs.rand(n)).astype(np.float32)
    if mu_edges:
        sel = rs.permutation(n)
        t = n // 10
        mu[sel[:t]] = 10.0 ** rs.uniform(-6, -2, t)
        mu[sel[t:2 * t]] = 1.0 - 10.0 ** rs.uniform(-6, -2, t)
        assert np.all((mu > 0) & (mu < 1))
    return theta, beta, mu, um, im


# The cases of tests/test_gpu_expomf_stages.py.  what: 'sweep' = Gram read-out on both sides, both half-sweeps and the mu update;
# 'gram' = the Gram read-out on the user side only (the column-count seams: n columns).  n >> k keeps the Gram well conditioned
# (e_ref is capped at 1e-5 by the fixture tool).
TRAINED = {}
for _k in (1, 2, 3, 4, 5):                                  # one pair block, waves 1..3 idle, K padding
    TRAINED['k%d' % _k] = dict(seed=1300 + _k, m=260, n=300, k=_k, what='sweep')
TRAINED.update({
    'k22': dict(seed=1322, m=700, n=450, k=22, what='sweep'),               # NB 2; the long item row (wrmf_long_pairs = 100)
    'k30': dict(seed=1330, m=600, n=500, k=30, what='sweep'),               # NB 4
    'k45': dict(seed=1345, m=700, n=600, k=45, what='sweep'),               # first NB 6, gy = 2
    'k64': dict(seed=1364, m=700, n=600, k=64, what='sweep', kw=dict(empty=[40, 3])),   # gy = 3; expo_gram_mb = 1: see the test
    'k127': dict(seed=1427, m=900, n=520, k=127, what='sweep'),             # gy = 11, K padding
    'k128': dict(seed=1428, m=900, n=520, k=128, what='sweep'),             # gy = 11
    'sq22': dict(seed=1522, m=300, n=300, k=22, what='sweep'),              # m == n: the item side takes mu per column
    'n9001': dict(seed=1622, m=700, n=9001, k=22, what='sweep'),            # 15 splits of 640 columns: a flush + a one-chunk tail each
    'mu_edges': dict(seed=1722, m=3000, n=200, k=22, what='sweep', kw=dict(mu_edges=True)),
    'big_s': dict(seed=1822, m=400, n=600, k=22, what='sweep', kw=dict(score_scale=2.0)),   # max |s| > 13: pEX below the 1e-8 term
})
for _n in (1, 127, 128, 129, 512, 513):                     # the 128-chunk and 512-flush seams
    TRAINED['n%d' % _n] = dict(seed=1900 + _n, m=260, n=_n, k=22, what='gram')
C2_TRAINED_SEED = 20260113


def trained_inputs(tag):
    c = TRAINED[tag]
    return trained_case(c['seed'], c['m'], c['n'], c['k'], **c.get('kw', {}))


def gram_row_lists(tag, side, ptr):
    """The row lists of the Gram read-out: a lone row, and 33 rows (a second tile with one live row) that hold a row without
    pairs where the side has one."""
    rs = np.random.RandomState(TRAINED[tag]['seed'] + 50 + side)
    nr = len(ptr) - 1
    none = np.flatnonzero(np.diff(ptr) == 0)
    rows = [int(x) for x in rs.permutation(nr)[:33]]
    if len(none) and none[0] not in rows:
        rows[7] = int(none[0])
    return [np.array([nr // 2], np.int32), np.array(rows, np.int32)]


def trained_e_ref(tag):
    """e_ref of a trained-scale case, per output: the reference's arithmetic (expo_reference_rows / _gram / _mu: its dtypes
    and statements) against the fp64 contract on the same inputs.  Every stage starts from the SEEDED factors (theta half, beta
    half, mu update, the Grams), because only those are at trained scale by construction: after a user half-sweep against
    9001 columns the solved theta is small again and the item side would be blind once more.  The Grams are compared
    entry-wise per row (gram_rel), the largest over the row lists."""
    c = TRAINED[tag]
    theta0, beta0, mu0, um, im = trained_inputs(tag)
    lam = LAM_THETA / LAM_Y
    sq = c['m'] == c['n']
    e = {}
    for side, (F, Fo, ptr, pc) in enumerate(((beta0, theta0, um[0], True), (theta0, beta0, im[0], sq))):
        if side == 1 and c['what'] == 'gram':
            break
        e['gram_user' if side == 0 else 'gram_item'] = max(
            gram_rel(expo_reference_gram(F, Fo, LAM_Y, mu0, pc, rows), expo_gram_contract(F, Fo, mu0, pc, LAM_Y, rows))
            for rows in gram_row_lists(tag, side, ptr))
    if c['what'] == 'sweep':
        th = expo_half_sweep_contract(beta0, theta0, um[0], um[1], um[2], mu0, True, lam, LAM_Y)
        e['theta'] = rel(expo_reference_rows(beta0, theta0, um[0], um[1], um[2], lam, LAM_Y, mu0, True), th)
        be = expo_half_sweep_contract(theta0, beta0, im[0], im[1], im[2], mu0, sq, lam, LAM_Y)
        e['beta'] = rel(expo_reference_rows(theta0, beta0, im[0], im[1], im[2], lam, LAM_Y, mu0, sq), be)
        e['mu'] = rel(expo_reference_mu(theta0, beta0, mu0, um[0], um[1], PRIOR_A, PRIOR_B),
                      expo_mu_contract(theta0, beta0, um[0], um[1], mu0, PRIOR_A, PRIOR_B, LAM_Y))
    return e


def c2_trained(seed=C2_TRAINED_SEED):
    """c2_inputs' pairs with theta, beta at trained scale (standard deviation of the scores 1.5) and mu in [0.005, 0.305)."""
    inp = c2_inputs(seed)
    rs = np.random.RandomState(seed + 7)
    sd = sqrt(1.5 / sqrt(inp['k']))
    inp['theta'] = (sd * rs.randn(inp['m'], inp['k'])).astype(np.float32)
    inp['beta'] = (sd * rs.randn(inp['n'], inp['k'])).astype(np.float32)
    inp['mu'] = (0.005 + 0.3 * rs.rand(inp['n'])).astype(np.float32)
    return inp


def c2_trained_e_ref(inp, users, items):
    """e_ref of the trained-scale C2 rows: theta (sampled users) and beta (sampled items) from the seeded factors, their
    Grams, and mu on the sampled items."""
    theta, beta, mu = inp['theta'], inp['beta'], inp['mu']
    um, im = inp['user_major'], inp['item_major']
    lam = LAM_THETA / LAM_Y
    return {
        'theta': rel(expo_reference_rows(beta, theta, um[0], um[1], um[2], lam, LAM_Y, mu, True, users),
                     expo_half_sweep_contract(beta, theta, um[0], um[1], um[2], mu, True, lam, LAM_Y, rows=users)),
        'beta': rel(expo_reference_rows(theta, beta, im[0], im[1], im[2], lam, LAM_Y, mu, False, items),
                    expo_half_sweep_contract(theta, beta, im[0], im[1], im[2], mu, False, lam, LAM_Y, rows=items)),
        'gram_user': gram_rel(expo_reference_gram(beta, theta, LAM_Y, mu, True, users), expo_gram_contract(beta, theta, mu, True, LAM_Y, users)),
        'gram_item': gram_rel(expo_reference_gram(theta, beta, LAM_Y, mu, False, items), expo_gram_contract(theta, beta, mu, False, LAM_Y, items)),
        'mu': rel(expo_reference_mu(theta, beta, mu, um[0], um[1], PRIOR_A, PRIOR_B, items),
                  expo_mu_contract(theta, beta, um[0], um[1], mu, PRIOR_A, PRIOR_B, LAM_Y, items=items)),
    }
