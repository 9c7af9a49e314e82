// UserKNN (recommender/cf/UserKNN.py): exact top-K user neighbours by posting-list counting, and neighbourhood scoring.
//   sim(u, v) = 2|A_u & A_v| / |A_u | A_v|   (A_u: distinct training items of u), kept as the integers (v, c, union)
//   order     (sim descending, user id ascending), compared exactly as c_x * U_y vs c_y * U_x in 64-bit integers
//   score(i)  = sum_r sim_r * count_r(i) / sum_r sim_r over the neighbours r that hold i, accumulated in rank order in fp64
// Host side: knn_host.hip.  Integer LDS atomics only (counts commute), no float atomics: every result is deterministic.
#pragma once
#include <hip/hip_runtime.h>

#include "wg_rank.hpp"

#include <climits>
#include <cstdint>

namespace yue {

constexpr int kKnnThreads = 256;
constexpr int kKnnMaxK = 256;          // neighbours per user (the rank travels in 8 bits of the scoring sort key)
constexpr int kKnnMaxN = 100;          // top-N of the ranking (the reference's own cap)
constexpr int kKnnRange = 4096;        // candidate users counted per pass of k_knn_neighbors (LDS counters)
constexpr int kKnnSortCap = 2048;      // running top-K + appended candidates of k_knn_neighbors
constexpr int kKnnGather = 2048;       // (item, rank) entries gathered per chunk of k_knn_topn
constexpr int kKnnSel = 4096;          // running top-N + one chunk's scored items
static_assert(kKnnMaxK <= 256, "the neighbour's rank travels in 8 bits of the gather key");
static_assert((kKnnSortCap & (kKnnSortCap - 1)) == 0 && kKnnSortCap >= kKnnMaxK + kKnnThreads, "running top-K + one batch of appends");
static_assert((kKnnGather & (kKnnGather - 1)) == 0, "a chunk is padded to a power of two inside gkey");
static_assert((kKnnSel & (kKnnSel - 1)) == 0 && kKnnSel >= kKnnMaxN + kKnnGather, "running top-N + one chunk's scored items");

struct KnnArgs {
    int64_t m, n;
    const int64_t *u_ptr;      // user-major pairs: items ascending, with event counts
    const int32_t *u_items;
    const int32_t *u_counts;
    const int64_t *i_ptr;      // item-major pairs: users ascending
    const int32_t *i_users;
    int64_t *cursor;           // [nnz] k_knn_neighbors: per (row, item) the next position in the item's posting list
    int K;
    int range;                 // candidate users per pass (<= kKnnRange)
    int32_t *nbr, *inter, *uni;   // [m][K], padded with -1 / 0 / 0 behind the positive neighbours
    // scoring
    const int32_t *users;      // k_knn_topn: the users to rank
    int N;
    int gather;                // entries per chunk (<= kKnnGather)
    int exclude_own;
    int32_t *ids_out;          // [nu][N] (-1 padded)
    double *scores_out;        // [nu][N] (0 padded)
    int32_t *len_out;          // [nu]
    int *chunked_users;        // users whose neighbour lists went through item-range chunks
    int32_t user;              // k_knn_predict_scores
    double *item_scores;       // [n]: score, or -1 where no neighbour holds the item
};

__device__ inline bool knn_better(int64_t c1, int64_t U1, int32_t v1, int64_t c2, int64_t U2, int32_t v2) {
    const int64_t l = c1 * U2, r = c2 * U1;
    return l > r || (l == r && v1 < v2);
}

// first position p in [cur, end) with a[p] >= bound (a ascending); galloping from cur, since the cursors advance by little
__device__ inline int64_t knn_gallop(const int32_t *a, int64_t cur, int64_t end, int64_t bound) {
    if (cur >= end || a[cur] >= bound) return cur;
    int64_t lo = cur, hi = end, step = 1;          // a[lo] < bound; hi == end or a[hi] >= bound
    while (true) {
        const int64_t probe = lo + step;
        if (probe >= end) break;
        if (a[probe] >= bound) { hi = probe; break; }
        lo = probe;
        step <<= 1;
    }
    while (hi - lo > 1) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] < bound) lo = mid; else hi = mid;
    }
    return hi;
}

// One workgroup per row user u.  Candidates v are counted in passes of `range` consecutive user ids: for every item of
// A_u, the part of its posting list inside the pass is walked (cursor kept across passes) and c[v] += 1 in LDS; the
// first touch of a counter appends v to a touched list, so extraction and clearing cost the distinct candidates.  A
// candidate that beats the running K-th entry is appended behind the running list; the list is re-formed by a sort of
// list + candidates whenever the appended block could overflow, and once at the end.
__global__ __launch_bounds__(kKnnThreads) void k_knn_neighbors(KnnArgs a) {
    __shared__ uint32_t cnt[kKnnRange];
    __shared__ int32_t touched[kKnnRange];
    __shared__ int32_t sv[kKnnSortCap], sc[kKnnSortCap], sU[kKnnSortCap];
    __shared__ int64_t seg_beg[kKnnThreads];
    __shared__ int incl[kKnnThreads];
    __shared__ int nt, nc, nl;
    const int tid = threadIdx.x;
    const int32_t u = (int32_t)blockIdx.x;
    const int K = a.K;
    const int64_t rb = a.u_ptr[u], du = a.u_ptr[u + 1] - rb;
    int32_t *onbr = a.nbr + (int64_t)u * K, *ointer = a.inter + (int64_t)u * K, *ouni = a.uni + (int64_t)u * K;
    if (du == 0) {
        for (int r = tid; r < K; r += kKnnThreads) { onbr[r] = -1; ointer[r] = 0; ouni[r] = 0; }
        return;
    }
    for (int i = tid; i < a.range; i += kKnnThreads) cnt[i] = 0u;
    for (int64_t j = tid; j < du; j += kKnnThreads) a.cursor[rb + j] = a.i_ptr[a.u_items[rb + j]];
    if (tid == 0) { nt = 0; nc = 0; nl = 0; }
    __syncthreads();

    auto less = [&](int x, int y) { return knn_better(sc[x], sU[x], sv[x], sc[y], sU[y], sv[y]); };
    auto swap = [&](int x, int y) {
        int32_t t = sv[x]; sv[x] = sv[y]; sv[y] = t;
        t = sc[x]; sc[x] = sc[y]; sc[y] = t;
        t = sU[x]; sU[x] = sU[y]; sU[y] = t;
    };
    auto pad = [&](int i) { sv[i] = INT_MAX; sc[i] = 0; sU[i] = 1; };   // sim 0: behind every candidate
    auto merge = [&]() { wg_reform<kKnnThreads>(nl, nc, K, pad, less, swap); };

    for (int64_t lo = 0; lo < a.m; lo += a.range) {
        const int64_t hi = lo + a.range < a.m ? lo + a.range : a.m;
        for (int64_t c0 = 0; c0 < du; c0 += kKnnThreads) {
            const int64_t jj = c0 + tid;
            int len = 0;
            int64_t beg = 0;
            if (jj < du) {
                const int32_t it = a.u_items[rb + jj];
                const int64_t end = a.i_ptr[it + 1];
                beg = a.cursor[rb + jj];
                const int64_t p = hi >= a.m ? end : knn_gallop(a.i_users, beg, end, hi);
                len = (int)(p - beg);                   // <= range: the users of one posting list are distinct
                a.cursor[rb + jj] = p;
            }
            seg_beg[tid] = beg;
            const int total = wg_scan<kKnnThreads>(len, incl);
            for (int f = tid; f < total; f += kKnnThreads) {
                const int j = wg_segment_of<kKnnThreads>(incl, f);
                const int excl = j ? incl[j - 1] : 0;
                const int idx = (int)(a.i_users[seg_beg[j] + (f - excl)] - lo);
                if (atomicAdd(&cnt[idx], 1u) == 0u) touched[atomicAdd(&nt, 1)] = idx;
            }
            __syncthreads();
        }
        const int ntouch = nt;
        for (int t0 = 0; t0 < ntouch; t0 += kKnnThreads) {
            const int occupied = nl + nc;
            __syncthreads();
            if (occupied + kKnnThreads > kKnnSortCap) merge();
            const int t = t0 + tid;
            if (t < ntouch) {
                const int idx = touched[t];
                const int32_t c = (int32_t)cnt[idx];
                cnt[idx] = 0u;
                const int32_t v = (int32_t)(lo + idx);
                if (v != u) {
                    const int32_t U = (int32_t)(du + (a.u_ptr[v + 1] - a.u_ptr[v]) - c);
                    if (nl < K || knn_better(c, U, v, sc[K - 1], sU[K - 1], sv[K - 1])) {
                        const int s = nl + atomicAdd(&nc, 1);
                        sv[s] = v; sc[s] = c; sU[s] = U;
                    }
                }
            }
            __syncthreads();
        }
        if (tid == 0) nt = 0;
        __syncthreads();
    }
    merge();
    for (int r = tid; r < K; r += kKnnThreads) {
        const bool have = r < nl;
        onbr[r] = have ? sv[r] : -1;
        ointer[r] = have ? sc[r] : 0;
        ouni[r] = have ? sU[r] : 0;
    }
}

// One workgroup per ranked user: the positive neighbours' user-major lists are gathered as (item, rank) keys -- all at
// once when they fit kKnnGather entries, else in item-range chunks of gather / K' items -- sorted, and every item's
// entries are summed in rank order (sum_r sim_r * count, sum_r sim_r; fp64, products rounded before the add).  The
// scores of a chunk (minus the user's own training items) are merged into the running top-N by a sort on (score
// descending, item ascending).
__global__ __launch_bounds__(kKnnThreads) void k_knn_topn(KnnArgs a) {
    __shared__ unsigned long long gkey[kKnnGather];
    __shared__ int32_t gcnt[kKnnGather];
    __shared__ double ss[kKnnSel];
    __shared__ int32_t si[kKnnSel];
    __shared__ double sim[kKnnMaxK];
    __shared__ int64_t seg_beg[kKnnThreads];
    __shared__ int incl[kKnnThreads];
    __shared__ int nc, nl;
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    const int32_t u = a.users[b];
    const int K = a.K, N = a.N;
    // the positive neighbours are a prefix of the row
    int32_t v = -1;
    if (tid < K) v = a.nbr[(int64_t)u * K + tid];
    const int kp = __syncthreads_count(v >= 0);
    int64_t cur = 0, end = 0;
    if (tid < kp) {
        const int64_t c = a.inter[(int64_t)u * K + tid], U = a.uni[(int64_t)u * K + tid];
        sim[tid] = (double)(2 * c) / (double)U;
        cur = a.u_ptr[v];
        end = a.u_ptr[v + 1];
    }
    const int total_all = wg_scan<kKnnThreads>((int)(end - cur < a.gather + 1 ? end - cur : a.gather + 1), incl);   // clamped: no overflow
    const int64_t width = total_all <= a.gather ? a.n : (int64_t)(a.gather / kp);
    if (tid == 0) {
        nl = 0; nc = 0;
        if (width < a.n) atomicAdd(a.chunked_users, 1);
    }
    const int64_t ob = a.u_ptr[u], oe = a.u_ptr[u + 1];
    __syncthreads();

    auto gless = [&](int x, int y) { return gkey[x] < gkey[y]; };
    auto gswap = [&](int x, int y) {
        const unsigned long long k = gkey[x]; gkey[x] = gkey[y]; gkey[y] = k;
        const int32_t c = gcnt[x]; gcnt[x] = gcnt[y]; gcnt[y] = c;
    };
    auto spad = [&](int f) { ss[f] = -1.0; si[f] = INT_MAX; };   // scores are > 0
    auto sless = [&](int x, int y) { return wg_before(ss[x], si[x], ss[y], si[y]); };
    auto sswap = [&](int x, int y) {
        const double s = ss[x]; ss[x] = ss[y]; ss[y] = s;
        const int32_t i = si[x]; si[x] = si[y]; si[y] = i;
    };

    for (int64_t lo = 0; lo < a.n; lo += width) {
        const int64_t hi = lo + width < a.n ? lo + width : a.n;
        int len = 0;
        if (tid < kp) {
            const int64_t p = hi >= a.n ? end : knn_gallop(a.u_items, cur, end, hi);
            len = (int)(p - cur);                       // <= width: a user's items are distinct
            seg_beg[tid] = cur;
            cur = p;
        }
        const int total = wg_scan<kKnnThreads>(len, incl);          // <= gather: kp * width entries at most
        for (int f = tid; f < total; f += kKnnThreads) {
            const int r = wg_segment_of<kKnnThreads>(incl, f);
            const int excl = r ? incl[r - 1] : 0;
            const int64_t pos = seg_beg[r] + (f - excl);
            gkey[f] = ((unsigned long long)(uint32_t)a.u_items[pos] << 8) | (unsigned)r;
            gcnt[f] = a.u_counts[pos];
        }
        const int P = wg_pow2(total);
        for (int f = total + tid; f < P; f += kKnnThreads) gkey[f] = ~0ull;
        __syncthreads();
        wg_bitonic<kKnnThreads>(1, P, gless, gswap);
        for (int f = tid; f < total; f += kKnnThreads) {
            const unsigned long long item = gkey[f] >> 8;
            if (f > 0 && (gkey[f - 1] >> 8) == item) continue;
            double sum = 0.0, den = 0.0;
            for (int g = f; g < total && (gkey[g] >> 8) == item; ++g) {
                const double s = sim[gkey[g] & 255u];
                sum = sum + s * (double)gcnt[g];
                den = den + s;
            }
            if (a.exclude_own) {
                int64_t l = ob, h = oe;
                while (l < h) {
                    const int64_t mid = l + ((h - l) >> 1);
                    if ((unsigned long long)(uint32_t)a.u_items[mid] < item) l = mid + 1; else h = mid;
                }
                if (l < oe && (unsigned long long)(uint32_t)a.u_items[l] == item) continue;
            }
            const int s = nl + atomicAdd(&nc, 1);
            ss[s] = sum / den;
            si[s] = (int32_t)item;
        }
        wg_reform<kKnnThreads>(nl, nc, N, spad, sless, sswap);
    }
    for (int r = tid; r < N; r += kKnnThreads) {
        const bool have = r < nl;
        a.ids_out[b * N + r] = have ? si[r] : -1;
        a.scores_out[b * N + r] = have ? ss[r] : 0.0;
    }
    if (tid == 0) a.len_out[b] = nl;
}

// predict(u) of one user: one thread per item, the neighbours visited in rank order (binary search in their lists);
// item_scores[i] = sum / den, or -1 where no positive neighbour holds i.  The host orders the scored items.
__global__ __launch_bounds__(kKnnThreads) void k_knn_predict_scores(KnnArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kKnnThreads + threadIdx.x;
    if (i >= a.n) return;
    const int64_t row = (int64_t)a.user * a.K;
    double sum = 0.0, den = 0.0;
    for (int r = 0; r < a.K; ++r) {
        const int32_t v = a.nbr[row + r];
        if (v < 0) break;
        int64_t l = a.u_ptr[v], h = a.u_ptr[v + 1];
        const int64_t e = h;
        while (l < h) {
            const int64_t mid = l + ((h - l) >> 1);
            if (a.u_items[mid] < i) l = mid + 1; else h = mid;
        }
        if (l < e && a.u_items[l] == i) {
            const double s = (double)(2 * (int64_t)a.inter[row + r]) / (double)a.uni[row + r];
            sum = sum + s * (double)a.u_counts[l];
            den = den + s;
        }
    }
    a.item_scores[i] = den > 0.0 ? sum / den : -1.0;
}

}  // namespace yue
