"""Factors that sit at the edge of the bf16 pre-filter's error bound, and a CPU model of what the filter must keep (NumPy only).

The scoring kernels keep a (user, item) pair for the exact chain only if
    bf16 score + c * 2^-7 ||P_u|| max||Q_tile|| > threshold_u,      c = 1.01 in the library (kScanMargin, score_kernels.hpp).
On iid factors the bf16 rounding errors cancel and c could be 0.  Here they add up: all products positive, user and item rows
nearly collinear (every entry is 2^e_col * (1 + d) with d of a few 2^-9: sum|p q| = p.q = ||P|| ||Q|| to four digits), and every
fp32 mantissa just BELOW a bf16 rounding midpoint (low 16 bits in [lo, 0x7FFF]), so that both factors round DOWN by almost
half a bf16 ulp and the bf16 score under-estimates the exact one by 0.94 .. 0.99 of 2^-7 ||P|| ||Q||.  All the exact scores
lie within 3 % of that margin of each other, so whatever the threshold is, it is a hair away from the item's exact score.

required_margin() replays the reference's selection on exact scores and returns the smallest c that keeps every list right."""
import numpy as np

HALF = 0x8000


def bf16_rne(x):
    """fp32 -> bf16 -> fp32, round to nearest even on the bit pattern (finite values)."""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = ((b + 0x7FFF + ((b >> np.uint64(16)) & np.uint64(1))) >> np.uint64(16)) << np.uint64(16)
    return r.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def chain_scores(P, Q):
    """[m, n] exact scores: acc = fma(P[u][e], Q[i][e], acc), e ascending, fp32 (the oracle's score_chain).  A product of two
    fp32 values is exact in fp64; the sum is rounded to fp64 and then to fp32, which differs from one rounding only when the
    fp64 sum lands within 2^-29 ulp of an fp32 midpoint."""
    P = np.asarray(P, np.float32)
    Q = np.asarray(Q, np.float32)
    acc = np.zeros((P.shape[0], Q.shape[0]), np.float32)
    P64, Q64 = P.astype(np.float64), Q.astype(np.float64)
    for e in range(P.shape[1]):
        acc = (acc.astype(np.float64) + P64[:, e, None] * Q64[None, :, e]).astype(np.float32)
    return acc


def _pattern(rs, ecol, count, lo, hi=0x7FFF):
    """count rows of 2^ecol[e] * (1 + low / 2^23), low 16 bits uniform in [lo, hi]."""
    bits = ((127 + ecol)[None, :].astype(np.uint32) << np.uint32(23)) | rs.randint(lo, hi + 1, size=(count, len(ecol))).astype(np.uint32)
    return bits.view(np.float32)


def _users(rs, ecol, m, lo):
    """User rows: the pattern, low bits of their own, one power-of-two scale per user (user 0: scale 1)."""
    scale = (2.0 ** rs.randint(-4, 4, size=(m, 1))).astype(np.float32)
    scale[0] = 1.0
    return np.ascontiguousarray(_pattern(rs, ecol, m, lo) * scale)


def _no_mask(m):
    return np.zeros(m + 1, np.int64), np.zeros(0, np.int32)


def _csr(rows):
    indptr = np.zeros(len(rows) + 1, np.int64)
    indptr[1:] = np.cumsum([len(r) for r in rows])
    indices = (np.concatenate(rows) if indptr[-1] else np.zeros(0)).astype(np.int32)
    return indptr, indices


def _sorted_pool(rs, ecol, p0, count, lo):
    """count item rows of the pattern, ascending by the exact score of user row p0 -> (rows, scores)."""
    Q = _pattern(rs, ecol, count, lo)
    s = chain_scores(p0[None, :], Q)[0]
    order = np.argsort(s, kind='stable')
    return np.ascontiguousarray(Q[order]), s[order]


def under(m, n, k, seed=1, lo=0x7800):
    """Every item at the edge of the bound: items ascending by the exact score of user 0 (nearly the same order for every user),
    so that almost every item is a list event."""
    rs = np.random.RandomState(seed)
    ecol = rs.randint(-3, 1, size=k)
    P = _users(rs, ecol, m, lo)
    Q, _ = _sorted_pool(rs, ecol, P[0], n, lo)
    return (P, Q) + _no_mask(m)


def _decoys(rs, ecol, p0, targets):
    """One row per target: every coordinate just ABOVE a bf16 midpoint (it rounds up by almost half an ulp: the bf16 score
    over-estimates), but for the coordinate of the smallest weight, whose value is chosen so that user p0's exact score lies just
    below the target."""
    k, cnt = len(ecol), len(targets)
    D = _pattern(rs, ecol, cnt, HALF + 1, HALF + 0x40)
    free = int(np.argmin(ecol + 1e-3 * np.arange(k)))
    D[:, free] = 0.0
    want = (np.asarray(targets, np.float64) - chain_scores(p0[None, :], D)[0].astype(np.float64)) / np.float64(p0[free])
    D[:, free] = want.astype(np.float32)
    targets = np.asarray(targets, np.float32)
    for _ in range(64):                                 # walk the free coordinate by an ulp of the score until the chain score is below
        high = chain_scores(p0[None, :], D)[0] >= targets
        if not high.any():
            break
        dec = (np.spacing(targets[high]).astype(np.float64) / abs(np.float64(p0[free]))).astype(np.float32)
        down = np.float32(-np.inf if p0[free] > 0 else np.inf)
        D[high, free] = np.nextafter(D[high, free] - np.sign(-down) * dec, down)
    else:
        raise AssertionError('decoys do not reach their targets')
    return D


def mixed(m, n, k, seed=2, lo=0x7800, n_max=100):
    """`under` interleaved with what must NOT enter a list or must not disturb it:
    - decoys (one item in five): bf16 over-estimates them and their exact score lies a hair below the scores of the items around
      (half of them below every under-type item, half below the item n_max + 10 places back): rescored and rejected;
    - a block of anti-aligned items (large negative scores) in the middle and at the very head;
    - coordinates whose sign is flipped in P and Q alike (sum|p q| = p.q still holds, with negative factors);
    - dense masks punched into the head of the catalogue, different for every user."""
    rs = np.random.RandomState(seed)
    ecol = rs.randint(-3, 1, size=k)
    P = _users(rs, ecol, m, lo)
    n_anti = max(8, n // 50)
    n_dec = (n - n_anti) // 5
    n_und = n - n_anti - n_dec
    U, su = _sorted_pool(rs, ecol, P[0], n_und, lo)
    kind = np.zeros(n, np.int8)                         # 0 under, 1 decoy, 2 anti-aligned
    kind[:4] = 2
    kind[n // 2:n // 2 + n_anti - 4] = 2
    free_pos = np.where(kind == 0)[0]
    kind[free_pos[rs.choice(len(free_pos) - 8, size=n_dec, replace=False) + 8]] = 1       # (the first places stay under-type)
    Q = np.zeros((n, k), np.float32)
    Q[kind == 0] = U
    before = np.cumsum(kind == 0)[kind == 1]            # under-type items in front of each decoy
    floor_ = np.float32(su[0])
    trail = su[np.maximum(before - (n_max + 10), 0)]
    targets = np.where(np.arange(n_dec) % 2 == 0, floor_, trail).astype(np.float32)
    Q[kind == 1] = _decoys(rs, ecol, P[0], targets)
    Q[kind == 2] = -_pattern(rs, ecol, int((kind == 2).sum()), lo)
    flip = rs.rand(k) < 0.25
    P[:, flip] *= -1.0
    Q[:, flip] *= -1.0
    head = min(n // 4, 256)
    rows = [np.sort(rs.choice(head, size=rs.randint(0, max(1, head - 8)), replace=False)) if u % 3 else np.zeros(0, np.int64) for u in range(m)]
    return (np.ascontiguousarray(P), np.ascontiguousarray(Q)) + _csr(rows)


def spike_positions(n):
    """Where `spikes` puts its full-norm items behind the head of 128: one per stage of 64 items at the stage's (j mod 64)-th
    place (the spike is alone in its tile and the tiles beside it are small; the places no stage of a short catalogue reaches
    go into the other tile of a later stage: n >= 4096 hits all 64), both sides of every power-of-two chunk boundary
    (511/512/513, 1023/1024, ...), and the catalogue's last tile."""
    pos = set()
    for j in range(3, n // 64):
        pos.add(64 * j + j % 64)
    for r in set(range(64)) - set(p % 64 for p in pos):
        j = (r + 32) % 64 + (64 if (r + 32) % 64 < 3 else 0)
        if 64 * j + r < n:
            pos.add(64 * j + r)
    b = 512
    while b < n:
        pos.update((b - 1, b, b + 1))
        b *= 2
    pos.update((n - 1, (n - 1) // 32 * 32))
    return np.array(sorted(p for p in pos if 128 <= p < n), np.int64)


def spikes(m, n, k, seed=3, lo=0x7800):
    """A catalogue of small items (the pattern times 2^-6) with a head of 128 full-norm items (they seed the lists, so the
    thresholds are at full scale from the start) and isolated full-norm items behind it (spike_positions), ascending in score:
    each spike is an event at the edge of the bound -- with ITS tile's norm.  A tile norm, a skip or an exit decided with a
    neighbouring tile's norm (2^-6 of it) drops the spike."""
    rs = np.random.RandomState(seed)
    ecol = rs.randint(-3, 1, size=k)
    P = _users(rs, ecol, m, lo)
    pos = spike_positions(n)
    big, _ = _sorted_pool(rs, ecol, P[0], 128 + len(pos), lo)
    Q = _pattern(rs, ecol, n, lo) * np.float32(2.0 ** -6)
    Q[:128] = big[:128]
    Q[pos] = big[128:]
    rows = [np.array([0, 1, 5, 127][:u % 5], np.int64) for u in range(m)]
    return (P, np.ascontiguousarray(Q)) + _csr(rows)


def settling(m, n, k, seed=4, lo=0x7800, late=None):
    """Item norms that fall along the catalogue (full scale up to item 512, half up to 4096, a quarter behind), so that the scan
    picks the filter variant whose workgroups stop (scan_last_settle == 1).  Three users in four are collinear with the items
    and settled against the tail.  User 0 and every user with u % 4 == 1 live on the first half of the coordinates only; `late`
    items, zero on the second half, are collinear with THEM: norm 0.71 of the head's (the settled users stay settled), exact
    score above every earlier item's by a few ulps, ascending.  Cauchy-Schwarz is tight for these pairs: the exit
    pn * sufmax <= threshold and the tile skip hold by the 1.0001 slacks alone."""
    assert n >= 16384 and k >= 16
    rs = np.random.RandomState(seed)
    ecol = rs.randint(-3, 1, size=k)
    ecol[k // 2:] = rs.permutation(ecol[:k // 2])        # the two halves carry the same weight
    P = _users(rs, ecol, m, lo)
    half = np.zeros(m, bool)
    half[1::4] = True
    half[0] = True
    P[half, k // 2:] = 0.0
    if late is None:
        late = sorted({4095, 4096, 8191, 8192, 8193, 12288, 16383, 16384, n // 2 + 37, n - 4097, n - 4096, n - 65, n - 33, n - 1})
    late = np.array([p for p in late if 512 <= p < n], np.int64)
    pool, _ = _sorted_pool(rs, ecol[:k // 2], P[0, :k // 2], 512 + len(late), lo)        # ascending on the first half
    tailh = _pattern(rs, ecol[k // 2:], 512 + len(late), lo)
    Q = _pattern(rs, ecol, n, lo)
    Q[512:4096] *= np.float32(0.5)
    Q[4096:] *= np.float32(0.25)
    Q[:512, :k // 2] = pool[:512]
    Q[:512, k // 2:] = tailh[:512]
    Q[late, :k // 2] = pool[512:]
    Q[late, k // 2:] = 0.0
    rows = [np.array([2, 3, 700][:u % 4], np.int64) for u in range(m)]
    return (np.ascontiguousarray(P), np.ascontiguousarray(Q)) + _csr(rows)


def ties(m, n, k, seed=5):
    """Small-integer factors (exact in bf16: the filter's scores equal the exact ones, so equal scores meet `bar < score` and the
    state machine's strict comparisons at equality), with equal item rows far apart and equal user rows."""
    rs = np.random.RandomState(seed)
    P = rs.randint(-2, 3, size=(m, k)).astype(np.float32)
    Q = rs.randint(-2, 3, size=(n, k)).astype(np.float32)
    src = rs.randint(0, min(n, 400), size=max(4, n // 16))
    dst = rs.randint(n // 2, n, size=len(src))
    Q[dst] = Q[src]
    Q[n - 1] = Q[0]
    if m > 3:
        P[m - 1] = P[1]
    rows = [np.sort(rs.choice(n, size=rs.randint(0, 9), replace=False)) for _ in range(m)]
    return (P, Q) + _csr(rows)


def chunk_bounds(n, growth, first=512):
    """End of every chunk of the two-phase path (scan_host.hip): first, first * growth, ..., n."""
    cb = [first]
    while cb[-1] < n:
        cb.append(min(n, cb[-1] * growth))
    return cb


def required_margin(P, Q, N, indptr, indices, stale=None, true_topn=False):
    """Replays the reference's selection (seed with the first N candidates, re-scan them, then overwrite without shift; or a
    real top-N) on the exact scores and returns (c, events per item): c is the largest
        (threshold - bf16 score) / (2^-7 ||P_u|| max||Q_tile||)
    over all items that changed a list behind the seeds -- the smallest margin constant with which the pre-filter keeps all of
    them.  bf16 score: fp64 dot product of the bf16-rounded factors (the MFMA's own fp32 accumulation moves it by parts in 1e5).
    stale = ends of the chunks: an item beyond the first chunk is filtered with the threshold its user had when the item's chunk
    began (k_scan_filter); without it, and inside the first chunk, with the running threshold."""
    P = np.asarray(P, np.float32)
    Q = np.asarray(Q, np.float32)
    m, n = P.shape[0], Q.shape[0]
    ex = chain_scores(P, Q)
    bf = bf16_rne(P).astype(np.float64) @ bf16_rne(Q).astype(np.float64).T
    pn = np.sqrt((P.astype(np.float64) ** 2).sum(1))
    qn = np.sqrt((Q.astype(np.float64) ** 2).sum(1))
    qpad = np.concatenate([qn, np.zeros(-n % 32)])
    unit = 2.0 ** -7 * pn[:, None] * qpad.reshape(-1, 32).max(1).repeat(32)[None, :n]
    masked = np.zeros((m, n), bool)
    for u in range(m):
        masked[u, indices[indptr[u]:indptr[u + 1]]] = True
    starts = set(int(b) for b in stale) if stale is not None else set()
    first_end = min(starts) if starts else n
    a = np.full((m, N), -np.inf, np.float32)             # lists, scores descending
    cnt = np.zeros(m, np.int64)
    seeds = np.zeros((m, N), np.float32)
    thr = np.full(m, -np.inf, np.float32)
    thr_chunk = thr.copy()
    worst, events = -np.inf, 0
    rows = np.arange(m)
    for i in range(n):
        if i in starts:
            thr_chunk = thr.copy()
        s = ex[:, i]
        live = ~masked[:, i]
        seeding = live & (cnt < N)
        for u in np.where(seeding)[0]:
            seeds[u, cnt[u]] = s[u]
            cnt[u] += 1
            if cnt[u] == N:
                lst = list(-np.sort(-seeds[u], kind='stable'))
                if not true_topn:                        # the scan starts over from the first candidate (overwrite, no shift)
                    for sq in seeds[u]:
                        if lst[N - 1] < sq:
                            p = N - 1
                            while p > 0 and lst[p - 1] < sq:
                                p -= 1
                            lst[p] = sq
                a[u] = lst
                thr[u] = a[u, N - 1]
        hit = live & ~seeding & (cnt == N) & (thr < s)
        if hit.any():
            hu = rows[hit]
            t_seen = thr[hu] if i < first_end else thr_chunk[hu]
            ratio = (t_seen.astype(np.float64) - bf[hu, i]) / unit[hu, i]
            finite = np.isfinite(ratio)
            if finite.any():
                worst = max(worst, float(ratio[finite].max()))
            events += len(hu)
            p = (a[hu] >= s[hu, None]).sum(1)             # first slot strictly below s
            if true_topn:
                for u, pu in zip(hu, p):
                    a[u, pu + 1:] = a[u, pu:N - 1].copy()
            a[hu, p] = s[hu]
            thr[hu] = a[hu, N - 1]
    return worst, events / float(m * n)


# ---- the cases of tests/test_gpu_score_adversary.py, tests/test_score_adversary.py and tools/scan_margin_probe.py ----
FAMILIES = {'under': under, 'mixed': mixed, 'spikes': spikes, 'settling': settling, 'ties': ties}
KS = (16, 32, 64, 128)
M_FUSED, M_TWO_PHASE = 200, 256          # two workgroups of the one-tile kernel, the second partial / one full workgroup of the others
N_TWO_PHASE = 16384 + 101                # neither a multiple of 32 nor of 64
LONGEST_TWO_PHASE_N = {16: 64, 32: 64, 64: 53, 128: 29}
N_LONG, M_LONG = 32768 + 2048 + 37, 128  # two chunks behind the first even when chunks grow 64-fold (512, 32,768, n)


def fused_cases():
    """(family, n, k, list lengths) below the two-phase size: n = 4096 / 4099 (spikes: every place of a stage), and n = N + 33."""
    out = []
    for k in KS:
        ns = (1, 5, 20, 64) + ((100,) if k == 128 else ())
        a, b = (ns[0::2], ns[1::2]) if k in (16, 64) else (ns[1::2], ns[0::2])      # (the oracle's time: every N at every k in `under`,
        out += [('under', 4096, k, ns), ('mixed', 4099, k, a), ('spikes', 4099, k, b), ('ties', 4099, k, a)]      # half of them elsewhere)
        tiny = {16: 1, 32: 5, 64: 20, 128: 64}[k]
        out += [('under', tiny + 33, k, (tiny,)), ('mixed', tiny + 33, k, (tiny,)), ('ties', tiny + 33, k, (tiny,))]
    return out


def two_phase_cases():
    """(family, n, k, list lengths) of the chunked path: every family at every k, one list length each (all four per family).
    The path is taken while the N slots of 256 users fit beside the first chunk's tiles in LDS: up to N = 64 at k <= 32, 53 at
    k = 64 and 29 at k = 128 -- the longest list stands for 64 there."""
    out = []
    for f, fam in enumerate(('under', 'mixed', 'spikes', 'settling', 'ties')):
        for q, k in enumerate(KS):
            ns = ((1,), (5,), (20,), (LONGEST_TWO_PHASE_N[k],))[(f + q) % 4]
            out.append((fam, N_TWO_PHASE, k, ns))
    return out


def long_cases():
    """(family, n, k, list lengths) for scan_growth 64: the items up to 32,768 are filtered with the thresholds of the first 512."""
    return [('under', N_LONG, 16, (5,)), ('settling', N_LONG, 32, (1,)), ('under', N_LONG, 64, (53,)), ('settling', N_LONG, 128, (20,))]


def make(family, m, n, k):
    return FAMILIES[family](m, n, k)
