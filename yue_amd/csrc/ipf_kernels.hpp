// IPF (recommender/cf/IPF.py): ranking by four typed 3-hop paths over the session temporal graph (STG).
// The reference's predict is a DFS whose first discoverer of a node gives it its only contribution on a path; it reduces
// to integer max-reductions (DESIGN.md section "IPF"):
//   level 1  the k-th distinct item a_k of the start list (k = 1, 2, ... by first occurrence): rank1 = carry1 + r0 * W0(u)
//   level 2  holder b of a level-1 item: parent a_K with K = max k, pos = b's first position in that holder list;
//            rank2(b) = carry2(b) + rank1 * P(a_K); expansion order E2 = (K desc, pos desc)
//   level 3  item c of a reached b's distinct list: the parent is the b first in E2, i.e. max (K, pos); score(c) +=
//            rank2(parent) * W2(parent), once per path, in path order (fp64, no fused multiply-add)
//   output   every reached item by (score desc, first insertion asc), insertion = (path, E2 position of the parent, j)
// Host side: ipf_host.hip.  Only integer atomics (max commutes), no float atomics: every result is bit-reproducible.
#pragma once
#include <hip/hip_runtime.h>

#include "wg_rank.hpp"

#include <cstdint>

namespace yue {

constexpr int kIpfThreads = 256;
constexpr int kIpfMaxN = 100;                   // top-N of the ranking (the reference's own cap)
constexpr int kIpfSel = 1024;                   // running top-N + appended candidates of the selection (LDS)
static_assert((kIpfSel & (kIpfSel - 1)) == 0 && kIpfSel >= kIpfMaxN + kIpfThreads, "running top-N + one batch of appends");
constexpr int kIpfKBits = 18;                   // distinct items of one user's list  < 2^18 (level-1 index k, level-3 index j)
constexpr int kIpfPosBits = 26;                 // length of one holder list (duplicates counted for sessions) < 2^26
constexpr unsigned long long kIpfUnreached = ~0ull;   // ins[] of an item no path has reached

struct IpfArgs {
    int64_t m, n;
    const int64_t *u_ptr;      // [m+1] each user's distinct training items, first-occurrence order
    const int32_t *u_items;
    const int64_t *s_ptr;      // [m+1] each user's distinct session items (the last 10 events), first-occurrence order
    const int32_t *s_items;
    const int64_t *hu_ptr;     // [n+1] item -> users (listened order); pos = index in the row
    const int32_t *hu_users;
    const int64_t *hs_ptr;     // [n+1] item -> session holders (distinct, user order) with first positions
    const int32_t *hs_users;
    const int32_t *hs_pos;
    const double *w_user, *w_sess;   // [m] 1 / L^rho, 1 / min(10, L)^rho
    const double *p_i2u, *p_i2s;     // [n] (eta / (eta nU + nS))^rho, (1 / (eta nU + nS))^rho
    double r_user, r_sess;           // beta, 1 - beta
    // per-slot work arrays (slot = workgroup): left clean by every query (key2 = key3 = 0, score = 0, ins = unreached)
    unsigned long long *key2;  // [slots][m] level-2 max of (k << 32 | ~pos)
    unsigned long long *e2;    // [slots][m] (K << 32 | pos) of each reached b on the running path
    double *r2u, *r2s;         // [slots][m] rank2 of user / session nodes (paths 0, 2 / 1, 3)
    int32_t *touch2;           // [slots][m] reached b of the running path
    unsigned long long *key3;  // [slots][n] level-3 max of the parents' (K << 32 | pos)
    double *score;             // [slots][n]
    unsigned long long *ins;   // [slots][n] first insertion (path, ~K, ~pos, j)
    int32_t *touch3;           // [slots][n] reached items, first reach order
    // queries
    const int32_t *users;
    int64_t nu;
    int N;                     // 0: predict (the reached items as they are), else top-N without the user's own items
    int32_t *ids_out;          // topn: [nu][N] (-1 padded); predict: [n] reached items
    double *scores_out;        // topn: [nu][N] (0 padded); predict: [n]
    unsigned long long *ins_out;   // predict: [n]
    int32_t *len_out;          // [nu]
};

__device__ inline void ipf_sync() {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // this wave's global stores and atomics are done before the barrier
    __syncthreads();
}

__device__ inline unsigned long long ipf_ld(const unsigned long long *p) {   // served by L2 (written by atomics)
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One workgroup per slot; it ranks users[q] for q = blockIdx.x, + gridDim.x, ...  Per query the four paths run in order:
// level-2 scatter (atomicMax over the level-1 items' holder lists, first touch appends b), the reached b's rank2 and
// E2 key, the level-3 max (atomicMax of the parents' E2 keys over their distinct lists), and the match pass, where the
// one entry whose E2 key equals its item's maximum adds the contribution and clears the maximum.
__global__ __launch_bounds__(kIpfThreads) void k_ipf_rank(IpfArgs a) {
    __shared__ int64_t incl[kIpfThreads];
    __shared__ int64_t seg_beg[kIpfThreads];
    __shared__ unsigned long long seg_key[kIpfThreads];
    __shared__ double seg_val[kIpfThreads];
    __shared__ double ss[kIpfSel];
    __shared__ unsigned long long si[kIpfSel];
    __shared__ int32_t sc[kIpfSel];
    __shared__ int n2, n3, nc, nl;
    const int tid = threadIdx.x;
    const int64_t slot = blockIdx.x;
    unsigned long long *key2 = a.key2 + slot * a.m, *e2 = a.e2 + slot * a.m;
    double *r2u = a.r2u + slot * a.m, *r2s = a.r2s + slot * a.m;
    int32_t *touch2 = a.touch2 + slot * a.m;
    unsigned long long *key3 = a.key3 + slot * a.n, *ins = a.ins + slot * a.n;
    double *score = a.score + slot * a.n;
    int32_t *touch3 = a.touch3 + slot * a.n;
    const unsigned long long kmask = (1ull << kIpfKBits) - 1, pmask = (1ull << kIpfPosBits) - 1;

    for (int64_t q = blockIdx.x; q < a.nu; q += gridDim.x) {
        const int32_t u = a.users[q];
        if (tid == 0) n3 = 0;
        for (int p = 0; p < 4; ++p) {
            const bool user_start = p < 2, i2u = (p & 1) == 0;      // start node type; holder lists item2user / item2session
            const bool exclude_u = p == 0 || p == 3;                // level 2 has the start node's type
            const int64_t *l1_ptr = user_start ? a.u_ptr : a.s_ptr;
            const int32_t *l1_items = user_start ? a.u_items : a.s_items;
            const int64_t *h_ptr = i2u ? a.hu_ptr : a.hs_ptr;
            const int32_t *h_users = i2u ? a.hu_users : a.hs_users;
            const double *P = i2u ? a.p_i2u : a.p_i2s;
            const int64_t *l3_ptr = i2u ? a.u_ptr : a.s_ptr;         // level 2 is a user node on paths 0, 2
            const int32_t *l3_items = i2u ? a.u_items : a.s_items;
            const double *W2 = i2u ? a.w_user : a.w_sess;
            double *r2 = i2u ? r2u : r2s;
            const double carry1 = user_start ? 0.0 : a.r_user * a.w_user[u];
            const double rank1 = carry1 + (user_start ? a.r_user * a.w_user[u] : a.r_sess * a.w_sess[u]);
            const int64_t lb = l1_ptr[u], le = l1_ptr[u + 1];
            if (tid == 0) n2 = 0;
            __syncthreads();
            // level 2: max over (k, ~pos) per holder b
            for (int64_t c0 = lb; c0 < le; c0 += kIpfThreads) {
                int64_t len = 0, beg = 0;
                if (c0 + tid < le) {
                    const int32_t it = l1_items[c0 + tid];
                    beg = h_ptr[it];
                    len = h_ptr[it + 1] - beg;
                }
                seg_beg[tid] = beg;
                const int64_t total = wg_scan<kIpfThreads>(len, incl);
                for (int64_t f = tid; f < total; f += kIpfThreads) {
                    const int s = wg_segment_of<kIpfThreads>(incl, f);
                    const int64_t e = seg_beg[s] + (f - (s ? incl[s - 1] : 0));
                    const int32_t b = h_users[e];
                    if (exclude_u && b == u) continue;
                    const unsigned long long pos = i2u ? (unsigned long long)(e - seg_beg[s]) : (unsigned long long)(uint32_t)a.hs_pos[e];
                    const unsigned long long key = ((unsigned long long)(c0 - lb + s + 1) << 32) | (0xFFFFFFFFull - pos);
                    if (atomicMax(&key2[b], key) == 0ull) touch2[atomicAdd(&n2, 1)] = b;
                }
                __syncthreads();
            }
            ipf_sync();
            const int reached = n2;
            // rank2 and E2 key of every reached b; key2 is left clean
            for (int t = tid; t < reached; t += kIpfThreads) {
                const int32_t b = touch2[t];
                const unsigned long long key = ipf_ld(&key2[b]);
                key2[b] = 0ull;
                const unsigned long long K = key >> 32, pos = 0xFFFFFFFFull - (key & 0xFFFFFFFFull);
                const int32_t aK = l1_items[lb + (int64_t)K - 1];
                double carry2 = 0.0;
                if (p == 2) carry2 = b == u ? a.r_user : r2u[b];
                else if (p == 3) carry2 = r2s[b];
                r2[b] = carry2 + rank1 * P[aK];
                e2[b] = (K << 32) | pos;
            }
            ipf_sync();
            // level 3, two passes over the reached b's distinct lists: the max of the parents' E2 keys, then the match
            for (int pass = 0; pass < 2; ++pass) {
                for (int t0 = 0; t0 < reached; t0 += kIpfThreads) {
                    int64_t len = 0, beg = 0;
                    if (t0 + tid < reached) {
                        const int32_t b = touch2[t0 + tid];
                        beg = l3_ptr[b];
                        len = l3_ptr[b + 1] - beg;
                        seg_key[tid] = e2[b];
                        seg_val[tid] = r2[b] * W2[b];
                    }
                    seg_beg[tid] = beg;
                    const int64_t total = wg_scan<kIpfThreads>(len, incl);
                    for (int64_t f = tid; f < total; f += kIpfThreads) {
                        const int s = wg_segment_of<kIpfThreads>(incl, f);
                        const int64_t j = f - (s ? incl[s - 1] : 0);
                        const int32_t c = l3_items[seg_beg[s] + j];
                        const unsigned long long k3 = seg_key[s];
                        if (pass == 0) {
                            atomicMax(&key3[c], k3);
                        } else if (ipf_ld(&key3[c]) == k3) {        // the parent of c: one entry per c
                            key3[c] = 0ull;
                            score[c] = score[c] + seg_val[s];
                            if (ins[c] == kIpfUnreached) {
                                const unsigned long long K = k3 >> 32, pos = k3 & 0xFFFFFFFFull;
                                ins[c] = ((unsigned long long)p << 62) | ((kmask - K) << (kIpfPosBits + kIpfKBits)) |
                                         ((pmask - pos) << kIpfKBits) | (unsigned long long)j;
                                touch3[atomicAdd(&n3, 1)] = c;
                            }
                        }
                    }
                    __syncthreads();
                }
                ipf_sync();
            }
        }
        const int items = n3;
        if (a.N == 0) {
            // predict: every reached item with its score and insertion key, in first-reach order
            for (int t = tid; t < items; t += kIpfThreads) {
                const int32_t c = touch3[t];
                a.ids_out[t] = c;
                a.scores_out[t] = score[c];
                a.ins_out[t] = ins[c];
            }
            if (tid == 0) a.len_out[q] = items;
        } else {
            // top-N without the user's own training items (marked in key3 for the selection, cleared after it)
            const int N = a.N;
            for (int64_t e = a.u_ptr[u] + tid; e < a.u_ptr[u + 1]; e += kIpfThreads) key3[a.u_items[e]] = 1ull;
            if (tid == 0) { nl = 0; nc = 0; }
            ipf_sync();
            auto less = [&](int x, int y) { return wg_before(ss[x], si[x], ss[y], si[y]); };
            auto swap = [&](int x, int y) {
                const double s = ss[x]; ss[x] = ss[y]; ss[y] = s;
                const unsigned long long w = si[x]; si[x] = si[y]; si[y] = w;
                const int32_t c = sc[x]; sc[x] = sc[y]; sc[y] = c;
            };
            auto pad = [&](int i) { ss[i] = -1.0; si[i] = kIpfUnreached; sc[i] = -1; };   // scores are >= 0
            auto merge = [&]() { wg_reform<kIpfThreads>(nl, nc, N, pad, less, swap); };
            for (int t0 = 0; t0 < items; t0 += kIpfThreads) {
                const int occupied = nl + nc;
                __syncthreads();
                if (occupied + kIpfThreads > kIpfSel) merge();
                const int t = t0 + tid;
                if (t < items) {
                    const int32_t c = touch3[t];
                    if (ipf_ld(&key3[c]) == 0ull) {
                        const double s = score[c];
                        const unsigned long long w = ins[c];
                        if (nl < N || wg_before(s, w, ss[N - 1], si[N - 1])) {
                            const int at = nl + atomicAdd(&nc, 1);
                            ss[at] = s; si[at] = w; sc[at] = c;
                        }
                    }
                }
                __syncthreads();
            }
            merge();
            for (int r = tid; r < N; r += kIpfThreads) {
                const bool have = r < nl;
                a.ids_out[q * N + r] = have ? sc[r] : -1;
                a.scores_out[q * N + r] = have ? ss[r] : 0.0;
            }
            if (tid == 0) a.len_out[q] = nl;
            ipf_sync();
            for (int64_t e = a.u_ptr[u] + tid; e < a.u_ptr[u + 1]; e += kIpfThreads) key3[a.u_items[e]] = 0ull;
        }
        // leave the slot clean for its next query
        for (int t = tid; t < items; t += kIpfThreads) {
            const int32_t c = touch3[t];
            score[c] = 0.0;
            ins[c] = kIpfUnreached;
        }
        ipf_sync();
    }
}

}  // namespace yue
