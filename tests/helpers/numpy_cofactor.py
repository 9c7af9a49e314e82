"""NumPy contract of CoFactor (recommender/advanced/CoFactor.py; device: yue_cof_*).

cooccur_from_pairs   the item x item co-occurrence CSR (common users, both filter rules of CoFactor.py:46-66)
sppmi_from_cooccur   the shifted positive PMI of CoFactor.py:68-91 in Python doubles, as a symmetric CSR in id space
levels_of            the level schedule of the item sweep: level(i) = 1 + max(level(j): j in S_i, j < i), else 0
item_sweep           the item sweep of CoFactor.py:127-168 for the rows of `order` one after the other (id order: the
                     reference's sequential sweep; level order: the device's schedule).  Per row every right-hand side is
                     evaluated before any write; contexts are visited in ascending id; X^T X is the fp32-rounded Gram of
                     numpy_wrmf.py; the two k x k systems are solved by an fp64 Cholesky factorisation; Y is rounded to fp32
                     once; G, w, c stay fp64.  The products of the item-side outer products Y_j Y_j^T are rounded to fp32
                     before they are summed in fp64, as the reference's float32 outer product does (CoFactor.py:156).
iteration            one iteration: WRMF's user half-sweep with its loss (numpy_wrmf.py), then the item sweep.
item_sweep_ld, iteration_ld   the same operations in the same order in np.longdouble (a hand-written Cholesky and substitution):
                     what the fp64 contract's own round-off is measured against (tests/test_gpu_cofactor_edges.py).
pairs_from_matrix, sppmi_from_edges, graph_with_degrees   builders of small synthetic problems.
"""
import math

import numpy as np
from scipy.sparse import csr_matrix

from helpers.numpy_wrmf import ALPHA, gram_fp32, wrmf_half_sweep_contract


def cooccur_from_pairs(i_ptr, i_users, i_counts, m, f):
    """(ptr int64 [n+1], idx int32 ascending, cnt int32): items with at least f training EVENTS take part, a pair is kept when
    its number of common users is > f; symmetric, no diagonal."""
    n = len(i_ptr) - 1
    events = np.zeros(n, np.int64)
    np.add.at(events, np.repeat(np.arange(n), np.diff(i_ptr)), np.asarray(i_counts, np.int64))
    B = csr_matrix((np.ones(len(i_users), np.int64), np.asarray(i_users, np.int64), np.asarray(i_ptr, np.int64)), shape=(n, m))
    C = (B @ B.T).tocoo()
    part = events >= f
    keep = (C.row != C.col) & part[C.row] & part[C.col] & (C.data > f)
    row, col, dat = C.row[keep], C.col[keep], C.data[keep]
    order = np.lexsort((col, row))
    ptr = np.zeros(n + 1, np.int64)
    np.add.at(ptr, row.astype(np.int64) + 1, 1)
    return np.cumsum(ptr), col[order].astype(np.int32), dat[order].astype(np.int32)


def sppmi_from_cooccur(ptr, idx, cnt, neg):
    """(ptr, idx, val float64): val = max(log(count * D / (freq_i * freq_j)) - log(neg), 0), only val > 0, divided by the
    largest; freq = row sums, D = their sum -- every operation in the reference's order on Python floats."""
    n = len(ptr) - 1
    freq = [float(int(cnt[ptr[i]:ptr[i + 1]].sum())) for i in range(n)]
    D = float(sum(freq))
    shift = math.log(neg)
    rows, vals = [], []
    best = 0
    for i in range(n):
        for e in range(int(ptr[i]), int(ptr[i + 1])):
            j = int(idx[e])
            val = max([math.log(int(cnt[e]) * D / (freq[i] * freq[j])) - shift, 0])
            if val > 0:
                best = max(best, val)
                rows.append((i, j))
                vals.append(val)
    out_ptr = np.zeros(n + 1, np.int64)
    for i, _ in rows:
        out_ptr[i + 1] += 1
    return np.cumsum(out_ptr), np.array([j for _, j in rows], np.int32), np.array([v / best for v in vals], np.float64)


def levels_of(sp_ptr, sp_idx):
    n = len(sp_ptr) - 1
    level = np.zeros(n, np.int64)
    for i in range(n):
        lo = sp_idx[sp_ptr[i]:sp_ptr[i + 1]]
        lo = lo[lo < i]
        if len(lo):
            level[i] = 1 + level[lo].max()
    return level


def level_order(sp_ptr, sp_idx, i_ptr, rng=None):
    """The rows level by level; inside a level longest first (pairs, ties by id), or shuffled by rng."""
    level = levels_of(sp_ptr, sp_idx)
    out = []
    for lv in range(int(level.max()) + 1 if len(level) else 0):
        rows = np.flatnonzero(level == lv)
        if rng is None:
            rows = rows[np.argsort(-np.diff(i_ptr)[rows], kind='stable')]
        else:
            rows = rng.permutation(rows)
        out.extend(int(r) for r in rows)
    return out


def _chol_solve(A, b):
    L = np.linalg.cholesky(A)
    return np.linalg.solve(L.T, np.linalg.solve(L, b))


def item_sweep(X, Y, G, w, c, i_ptr, i_users, i_counts, sp_ptr, sp_idx, sp_val, regU, regR, order=None, alpha=ALPHA):
    """In place on Y (fp32), G, w, c (fp64).  order: the rows in the order they are solved (default: id order)."""
    n, k = Y.shape
    XG = gram_fp32(X)
    eye = np.eye(k)
    for i in (range(n) if order is None else order):
        a, b = int(i_ptr[i]), int(i_ptr[i + 1])
        p, q = int(sp_ptr[i]), int(sp_ptr[i + 1])
        if a == b and p == q:
            Y[i] = 0
            continue
        Fr = X[i_users[a:b]].astype(np.float64)
        cc = alpha * i_counts[a:b].astype(np.float64)
        A = XG + (Fr.T * cc) @ Fr + regU * eye
        rhs = ((1.0 + cc)[:, None] * Fr).sum(0)
        if q > p:
            g1, g2 = np.zeros((k, k)), np.zeros((k, k))
            m1, m2 = np.zeros(k), np.zeros(k)
            uw = uc = 0.0
            yi = Y[i].astype(np.float64)
            for e in range(p, q):
                j, s = int(sp_idx[e]), float(sp_val[e])
                gamma, beta = G[j], Y[j]
                g1 += np.outer(gamma, gamma)
                m1 += (s - w[i] - c[j]) * gamma
                g2 += np.outer(beta, beta).astype(np.float64)          # fp32 products, fp64 sum
                b64 = beta.astype(np.float64)
                m2 += (s - w[j] - c[i]) * b64
                uw += s - float(np.sum(yi * gamma)) - c[j]
                uc += s - float(np.sum(b64 * G[i])) - w[j]
            A = A + g1
            rhs = rhs + m1
        y_new = _chol_solve(A, rhs).astype(np.float32)
        if q > p:
            g_new = _chol_solve(g2 + regR * eye, m2)
            w_new, c_new = uw / (q - p), uc / (q - p)
        Y[i] = y_new
        if q > p:
            G[i], w[i], c[i] = g_new, w_new, c_new


def iteration(X, Y, G, w, c, um, im, sp, regU, regR, order=None):
    """One iteration from (X, Y fp32; G, w, c fp64); returns (X, Y, G, w, c, loss) as new arrays."""
    Xn, loss = wrmf_half_sweep_contract(Y, um[0], um[1], um[2], regU, X_old=X)
    Y, G, w, c = Y.copy(), G.copy(), w.copy(), c.copy()
    item_sweep(Xn, Y, G, w, c, im[0], im[1], im[2], sp[0], sp[1], sp[2], regU, regR, order=order)
    return Xn, Y, G, w, c, loss


def init_from_seed(seed, m, n, k):
    """X0, Y0 (fp32) and w0, c0, G0 (fp64) as initModel and buildModel draw them after np.random.seed(seed): the base class's
    P and Q, then w, c, G in this order (CoFactor.py:97-101)."""
    rs = np.random.RandomState(seed)
    P = rs.rand(m, k).astype(np.float32) / 10
    Q = rs.rand(n, k).astype(np.float32) / 10
    w = rs.rand(n) / 10
    c = rs.rand(n) / 10
    G = rs.rand(n, k) / 10
    return P * 10, Q * 10, G, w, c


def rel(a, b):
    """max |a - b| / max |b|"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / np.abs(b).max()) if b.size else 0.0


# ---- the contract in extended precision ----
LD = np.longdouble


def chol_solve_ld(A, b):
    """A x = b by a column Cholesky factorisation and two substitutions, every operation in np.longdouble."""
    A, b = np.asarray(A, LD), np.asarray(b, LD)
    k = len(b)
    L = np.zeros((k, k), LD)
    for j in range(k):
        col = A[j:, j] - L[j:, :j] @ L[j, :j]
        if not col[0] > 0:
            raise np.linalg.LinAlgError('non-positive pivot %d' % j)
        L[j:, j] = col / np.sqrt(col[0])
    z = np.zeros(k, LD)
    for j in range(k):
        z[j] = (b[j] - L[j, :j] @ z[:j]) / L[j, j]
    x = np.zeros(k, LD)
    for j in range(k - 1, -1, -1):
        x[j] = (z[j] - L[j + 1:, j] @ x[j + 1:]) / L[j, j]
    return x


def half_sweep_ld(F, ptr, idx, cnt, reg, alpha=ALPHA):
    """wrmf_half_sweep_contract's rows in np.longdouble: the fp32-rounded Gram and the fp32 rounding of the rows are kept."""
    nr, k = len(ptr) - 1, F.shape[1]
    G = gram_fp32(F).astype(LD)
    out = np.zeros((nr, k), np.float32)
    for r in range(nr):
        a, b = int(ptr[r]), int(ptr[r + 1])
        if a == b:
            continue
        Fr = F[idx[a:b]].astype(LD)
        c = LD(alpha) * cnt[a:b].astype(LD)
        out[r] = chol_solve_ld(G + (Fr.T * c) @ Fr + LD(reg) * np.eye(k, dtype=LD), ((1 + c)[:, None] * Fr).sum(0)).astype(np.float32)
    return out


def item_sweep_ld(X, Y, G, w, c, i_ptr, i_users, i_counts, sp_ptr, sp_idx, sp_val, regU, regR, alpha=ALPHA):
    """item_sweep in np.longdouble, in place on Y (fp32: rounded once per row, as the contract does) and on G, w, c
    (np.longdouble arrays).  Y's outer products stay fp32 products."""
    n, k = Y.shape
    XG = gram_fp32(X).astype(LD)
    eye = np.eye(k, dtype=LD)
    for i in range(n):
        a, b = int(i_ptr[i]), int(i_ptr[i + 1])
        p, q = int(sp_ptr[i]), int(sp_ptr[i + 1])
        if a == b and p == q:
            Y[i] = 0
            continue
        Fr = X[i_users[a:b]].astype(LD)
        cc = LD(alpha) * i_counts[a:b].astype(LD)
        A = XG + (Fr.T * cc) @ Fr + LD(regU) * eye
        rhs = ((1 + cc)[:, None] * Fr).sum(0)
        if q > p:
            g1, g2 = np.zeros((k, k), LD), np.zeros((k, k), LD)
            m1, m2 = np.zeros(k, LD), np.zeros(k, LD)
            uw = uc = LD(0)
            yi = Y[i].astype(LD)
            for e in range(p, q):
                j, s = int(sp_idx[e]), LD(sp_val[e])
                gamma, beta = G[j], Y[j]
                g1 += np.outer(gamma, gamma)
                m1 += (s - w[i] - c[j]) * gamma
                g2 += np.outer(beta, beta).astype(LD)                  # fp32 products
                b64 = beta.astype(LD)
                m2 += (s - w[j] - c[i]) * b64
                uw += s - np.sum(yi * gamma) - c[j]
                uc += s - np.sum(b64 * G[i]) - w[j]
            A = A + g1
            rhs = rhs + m1
        y_new = chol_solve_ld(A, rhs).astype(np.float32)
        if q > p:
            g_new = chol_solve_ld(g2 + LD(regR) * eye, m2)
            w_new, c_new = uw / (q - p), uc / (q - p)
        Y[i] = y_new
        if q > p:
            G[i], w[i], c[i] = g_new, w_new, c_new


def iteration_ld(X, Y, G, w, c, um, im, sp, regU, regR):
    """iteration in np.longdouble (G, w, c np.longdouble in and out); no loss."""
    Xn = half_sweep_ld(Y, um[0], um[1], um[2], regU)
    Y, G, w, c = Y.copy(), G.copy(), w.copy(), c.copy()
    item_sweep_ld(Xn, Y, G, w, c, im[0], im[1], im[2], sp[0], sp[1], sp[2], regU, regR)
    return Xn, Y, G, w, c


# ---- builders of synthetic problems ----
def pairs_from_matrix(R):
    """(u_ptr, u_items, u_counts), (i_ptr, i_users, i_counts) of a dense user x item matrix of event counts (0: no pair)."""
    R = np.asarray(R)
    m, n = R.shape
    us, it = np.nonzero(R)
    i2, u2 = np.nonzero(R.T)
    u_ptr = np.concatenate([[0], np.cumsum(np.bincount(us, minlength=m))]).astype(np.int64)
    i_ptr = np.concatenate([[0], np.cumsum(np.bincount(i2, minlength=n))]).astype(np.int64)
    return (u_ptr, it.astype(np.int32), R[us, it].astype(np.int32)), (i_ptr, u2.astype(np.int32), R[u2, i2].astype(np.int32))


def sppmi_from_edges(n, edges, seed):
    """A symmetric CSR (ptr int64, idx int32 ascending, val float64 in (0, 1]) over the undirected edges (i, j), i != j."""
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    assert (e[:, 0] != e[:, 1]).all()
    key = np.unique(np.minimum(e[:, 0], e[:, 1]) * n + np.maximum(e[:, 0], e[:, 1]))
    val = 1.0 - np.random.RandomState(seed).rand(len(key))
    row = np.concatenate([key // n, key % n])
    col = np.concatenate([key % n, key // n])
    order = np.lexsort((col, row))
    ptr = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=n))]).astype(np.int64)
    return ptr, col[order].astype(np.int32), np.concatenate([val, val])[order]


def graph_with_degrees(n, degrees, hub, seed, filler_edges=0):
    """Edges of a graph in which item t has exactly degrees[t] neighbours: the items of `degrees` join only the hub (when
    not None: the hub joins every other item) and items outside `degrees`; filler_edges more edges among the latter."""
    rng = np.random.RandomState(seed)
    special = set(degrees) | ({hub} if hub is not None else set())
    filler = np.array([i for i in range(n) if i not in special])
    edges = [(hub, i) for i in range(n) if i != hub] if hub is not None else []
    for t, d in degrees.items():
        d -= hub is not None
        assert 0 <= d <= len(filler)
        edges += [(t, int(j)) for j in rng.choice(filler, d, replace=False)]
    for _ in range(filler_edges):
        a, b = rng.choice(filler, 2, replace=False)
        edges.append((int(a), int(b)))
    return edges
