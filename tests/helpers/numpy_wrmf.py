"""NumPy oracles of WRMF (recommender/cf/WRMF.py; device: yue_wrmf_half_sweep, DESIGN.md section "WRMF").

wrmf_reference_form       the reference's buildModel statement by statement, at its dtypes (fp32 factors, fp32 YtY, fp64
                          sparse term / b / inverse), for the CPU pin against the g10 fixtures.
wrmf_half_sweep_contract  the device contract of one half-sweep: the fixed side's Gram summed in fp64 and rounded to fp32
                          once, the sparse term and b in fp64, an fp64 Cholesky solve, the row rounded to fp32.  Any subset
                          of rows can be computed, which keeps checks at full size cheap.
"""
import numpy as np
from scipy.sparse import coo_matrix

ALPHA = 10.0


def wrmf_reference_form(X, Y, u_rows, i_rows, iters, reg):
    """u_rows[u] / i_rows[i] = (ids, counts) of a user's items / an item's users.  Returns (X, Y, losses, Xs, Ys), Xs / Ys
    the factors after every iteration.  X, Y are float32 and are not modified."""
    X = X.copy()
    Y = Y.copy()
    m, k = X.shape
    n = Y.shape[0]
    losses, Xs, Ys = [], [], []
    for _it in range(iters):
        loss = 0
        YtY = Y.T.dot(Y)                                            # float32 (WRMF.py:35)
        for uid in range(m):
            items, cnt = u_rows[uid]
            H = np.ones(n)
            P_u = np.zeros(n)
            for iid, r in zip(items, cnt):
                H[iid] += ALPHA * r
                P_u[iid] = 1
                error = (P_u[iid] - X[uid].dot(Y[iid]))
                loss += pow(error, 2)
            C_u = coo_matrix((ALPHA * np.asarray(cnt, np.float64), (items, items)), shape=(n, n))
            A = (YtY + np.dot(Y.T, C_u.dot(Y)) + reg * np.eye(k))
            X[uid] = np.dot(np.linalg.inv(A), (Y.T * H).dot(P_u))
        XtX = X.T.dot(X)
        for iid in range(n):
            users, cnt = i_rows[iid]
            P_i = np.zeros(m)
            H = np.ones(m)
            for uid, r in zip(users, cnt):
                H[uid] += ALPHA * r
                P_i[uid] = 1
            C_i = coo_matrix((ALPHA * np.asarray(cnt, np.float64), (users, users)), shape=(m, m))
            A = (XtX + np.dot(X.T, C_i.dot(X)) + reg * np.eye(k))      # regU on the item side too (WRMF.py:74)
            Y[iid] = np.dot(np.linalg.inv(A), (X.T * H).dot(P_i))
        losses.append(float(loss))
        Xs.append(X.copy())
        Ys.append(Y.copy())
    return X, Y, losses, Xs, Ys


def gram_fp32(F):
    """F^T F summed in fp64 (the products of fp32 factors are exact there), rounded to fp32 once, returned as fp64."""
    F64 = F.astype(np.float64)
    return (F64.T @ F64).astype(np.float32).astype(np.float64)


def wrmf_half_sweep_contract(F, ptr, idx, cnt, reg, rows=None, X_old=None, alpha=ALPHA, G=None):
    """x_r = A_r^-1 b_r for the given rows (all by default) of the solved side, rows without pairs 0.
    F: the fixed side (fp32 [nf, k]); ptr / idx / cnt: the solved side's pairs.  With X_old (the solved side before the
    sweep) the loss terms sum over the rows' pairs of (1 - fp32(x_old . y))^2 are returned too.  Raises
    numpy.linalg.LinAlgError where A is not positive definite.  Returns (rows' fp32 solutions, loss or None)."""
    nr = len(ptr) - 1
    k = F.shape[1]
    rows = np.arange(nr) if rows is None else np.asarray(rows)
    if G is None:
        G = gram_fp32(F)
    out = np.zeros((len(rows), k), np.float32)
    loss = 0.0 if X_old is not None else None
    for t, r in enumerate(rows):
        a, b = int(ptr[r]), int(ptr[r + 1])
        if a == b:
            continue
        Fr = F[idx[a:b]].astype(np.float64)
        c = alpha * cnt[a:b].astype(np.float64)
        A = G + (Fr.T * c) @ Fr + reg * np.eye(k)
        rhs = ((1.0 + c)[:, None] * Fr).sum(0)
        L = np.linalg.cholesky(A)
        z = np.linalg.solve(L, rhs)
        out[t] = np.linalg.solve(L.T, z).astype(np.float32)
        if X_old is not None:
            d = (Fr @ X_old[r].astype(np.float64)).astype(np.float32).astype(np.float64)
            loss += float(((1.0 - d) ** 2).sum())
    return out, loss


def pairs_from_events(ev_u, ev_i, m, n):
    """(u_ptr, u_items, u_counts), (i_ptr, i_users, i_counts): the distinct pairs with their event counts both ways."""
    keys, counts = np.unique(np.asarray(ev_u, np.int64) * n + np.asarray(ev_i, np.int64), return_counts=True)
    users = (keys // n).astype(np.int32)
    items = (keys % n).astype(np.int32)
    counts = counts.astype(np.int32)
    u_ptr = np.zeros(m + 1, np.int64)
    np.add.at(u_ptr, users.astype(np.int64) + 1, 1)
    order = np.argsort(items, kind='stable')
    i_ptr = np.zeros(n + 1, np.int64)
    np.add.at(i_ptr, items.astype(np.int64) + 1, 1)
    return (np.cumsum(u_ptr), items, counts), (np.cumsum(i_ptr), users[order], counts[order])


def rows_of(ptr, ids, cnt):
    return [(ids[ptr[r]:ptr[r + 1]], cnt[ptr[r]:ptr[r + 1]]) for r in range(len(ptr) - 1)]
