// CUNE's user-network stage (recommender/advanced/CUNE.py:34-118): the collaborative user network, its random walks, a
// CBOW / negative-sampling user embedding and the cosine top-K friends.  Host side: cnet_host.hip; contract in NumPy:
// tests/helpers/numpy_cune_net.py; DESIGN.md section 18.
//   network    CUNet[a] (every other user b repeated |items(a) & items(b)| times) is never built: a uniform draw over it is
//              a uniform draw over the pairs (item i of a, listener b != a of i).  pref[e] = inclusive sum of deg(i) - 1
//              over a's item row; r < total(a) -> the item by binary search, the listener by index with a skipped.
//   walks      one wave per start user, its T walks one after another, visited[start] in LDS.  Every draw is
//              cnet_hash(seed, start, t, step, attempt): a walk is a pure function of its indices.  DEVIATION from the
//              reference: visited[lastNode] is consulted only where lastNode == start (for any other lastNode the
//              reference reads whatever the walks from lastNode have stored so far -- dict order); empty otherwise.
//   embedding  gensim's CBOW (mean) with negative sampling as documented, with this stream; one wave per walk, rounds of
//              round_walks walks: a wave works on LDS copies of the rows it touches (round-start values + its own
//              changes); the differences go into 64-bit fixed-point accumulators (2^-36, integer atomics: the sum does
//              not depend on the order) and k_cnet_embed_apply adds them to the matrices.  No float atomics.
//   friends    tiles of candidate rows in LDS against a block of query rows, fp64 dots, running top-K per query by
//              (cosine descending, id ascending); no m x m array.
#pragma once
#include "bpr_device.hpp"
#include "counter_hash.hpp"
#include "wg_rank.hpp"

#include <climits>

namespace yue {

constexpr int kCnetMaxL = 64;              // walk length (one lane per position in the embedding kernel)
constexpr int kCnetMaxDim = 128;
constexpr int kCnetMaxK = 100;
constexpr int kCnetMaxVisited = 15360;     // T * (L - 1) ids of visited[start] in LDS (60 KiB)
constexpr int kCnetRedraws = 10;           // CUNE.py:64-69
constexpr int kCnetEmbedLds = 60 * 1024;   // working rows of one walk
constexpr int kCnetSegmentLds = 63 * 1024; // ... of one segment of a sentence, with the ids of its targets (64 KiB less the static arrays)
constexpr double kCnetFix = 68719476736.0;         // 2^36: fixed-point scale of the round's row differences
constexpr double kCnetUnfix = 1.0 / 68719476736.0;
constexpr float kCnetMaxExp = 6.0f;
// stream tags (xor-ed into the seed): one independent stream per use
constexpr uint64_t kCnetTagWalk = 0, kCnetTagShuffle = 0x5348554646ull, kCnetTagInit = 0x494E4954ull, kCnetTagSub = 0x535542ull,
                   kCnetTagWin = 0x57494Eull, kCnetTagNeg = 0x4E4547ull;

struct CnetArgs {
    int64_t m, n;
    const int64_t *u_ptr; const int32_t *u_items;      // user -> items ascending
    const int64_t *i_ptr; const int32_t *i_users;      // item -> users ascending
    int64_t *pref;             // [nnz] inclusive prefix of deg(item) - 1 within the user's row
    int64_t *total;            // [m]
    // walks
    const int32_t *net;        // network users ascending
    const int64_t *dest;       // [nw] walk (rank of start * T + t) -> its place in the shuffled list
    int32_t *walks;            // [nw][L]
    int T, L;
    uint64_t seed;
};

__global__ void k_cnet_prefix(CnetArgs a) {
    const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= a.m) return;
    int64_t s = 0;
    for (int64_t e = a.u_ptr[u]; e < a.u_ptr[u + 1]; ++e) {
        const int32_t i = a.u_items[e];
        s += a.i_ptr[i + 1] - a.i_ptr[i] - 1;
        a.pref[e] = s;
    }
    a.total[u] = s;
}

// the r-th entry (r < total(u)) of the implicit CUNet[u]
__device__ inline int32_t cnet_pick(const CnetArgs &a, int32_t u, uint64_t z) {
    const int64_t rb = a.u_ptr[u], re = a.u_ptr[u + 1];
    const int64_t r = (int64_t)__umul64hi(z, (uint64_t)a.total[u]);
    int64_t lo = rb, hi = re - 1;                       // smallest e with pref[e] > r
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (a.pref[mid] > r) hi = mid; else lo = mid + 1;
    }
    const int64_t off = r - (lo > rb ? a.pref[lo - 1] : 0);
    const int32_t i = a.u_items[lo];
    const int64_t lb = a.i_ptr[i];
    int64_t l = lb, h = a.i_ptr[i + 1];                 // position of u in the item's listener row
    while (l < h) {
        const int64_t mid = l + ((h - l) >> 1);
        if (a.i_users[mid] < u) l = mid + 1; else h = mid;
    }
    return a.i_users[lb + off + (off >= l - lb ? 1 : 0)];
}

// One wave per start user.  Every lane computes the same walk; the lanes share the scan of visited[start].
__global__ __launch_bounds__(64) void k_cnet_walk(CnetArgs a) {
    extern __shared__ int32_t visited[];
    const int lane = threadIdx.x;
    const int32_t start = a.net[blockIdx.x];
    int nv = 0;
    for (int t = 0; t < a.T; ++t) {
        int32_t *out = a.walks + a.dest[(int64_t)blockIdx.x * a.T + t] * a.L;
        if (lane == 0) out[0] = start;
        int32_t last = start;
        for (int step = 1; step < a.L; ++step) {
            int32_t cand = cnet_pick(a, last, cnet_hash(a.seed ^ kCnetTagWalk, (uint64_t)start, (uint64_t)t, (uint64_t)step, 0));
            if (last == start) {
                for (int attempt = 1; attempt <= kCnetRedraws; ++attempt) {
                    bool seen = false;
                    for (int v = lane; v < nv; v += 64) seen |= visited[v] == cand;
                    if (__ballot(seen) == 0ull) break;
                    cand = cnet_pick(a, last, cnet_hash(a.seed ^ kCnetTagWalk, (uint64_t)start, (uint64_t)t, (uint64_t)step, (uint64_t)attempt));
                }
            }
            __syncthreads();
            if (lane == 0) { out[step] = cand; visited[nv] = cand; }
            ++nv;
            __syncthreads();
            last = cand;
        }
    }
}

__global__ void k_cnet_count(const int32_t *walks, int64_t words, int32_t *cnt) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < words) atomicAdd(&cnt[walks[e]], 1);
}

// ... over segments of unequal length (yue_cnet_set_sentences): entry e of the [nw][L] array counts where it is a real word
__global__ void k_sent_count(const int32_t *walks, const int32_t *len, int64_t entries, int L, int32_t *cnt) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e < entries && (int)(e % L) < len[e / L]) atomicAdd(&cnt[walks[e]], 1);
}

struct CnetEmbedArgs {
    int64_t m, nw;
    const int32_t *walks;      // [nw][L] in training order
    const int32_t *cnt;        // [m] occurrences in the walks
    const uint64_t *keep;      // [m] subsampling: a word stays where (32 random bits) < keep
    const uint64_t *cum;       // [m] negative table: target = first id with cum > (32 random bits); cum[m - 1] = 2^32
    float *syn0, *syn1;        // [m][dim]
    long long *acc0, *acc1;    // [m][dim] fixed-point sums of the round's row differences
    int *flag0, *flag1;        // [m] the row has differences to apply
    int32_t *list;             // [round_walks][rows_per_walk] touched rows: syn0 rows, then syn1 rows as -(row + 1)
    int32_t *list_n;           // [round_walks]
    int L, dim, window, negative, epochs, epoch;
    int64_t w_begin, w_count;
    uint64_t seed;
    // behind what the walks use, so that their kernels read their arguments where they did
    const int32_t *len;        // sentences only: [nw] words of the segment (<= L; the rest of its row is padding)
    const int64_t *wpre;       // sentences only: [nw] words of the segments before it
    int64_t words;             // sentences only: all words
};

__global__ void k_cnet_embed_init(CnetEmbedArgs a) {
    const int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= a.m * a.dim) return;
    const int64_t u = x / a.dim, d = x % a.dim;
    float v = 0.0f;
    if (a.cnt[u] > 0) {
        const float U = (float)(cnet_hash(a.seed ^ kCnetTagInit, (uint64_t)u, 0, (uint64_t)d, 0) >> 40) * (1.0f / 16777216.0f);
        v = (U - 0.5f) / (float)a.dim;
    }
    a.syn0[x] = v;
    a.syn1[x] = 0.0f;
}

// One wave per walk of the round.  Lane l holds elements l (+ 64) of every vector.  LDS: cur0[L][dim] the syn0 rows of
// the walk's users (slot = first position of the user), cur1[L * (negative + 1)][dim] the syn1neg rows of its targets in
// first-use order, ids1 their ids.  VAR (sentences cut into segments, yue_cnet_set_sentences): the walk is a segment of
// len[w] <= L words -- lanes and positions beyond it take no part, and alpha runs over the words passed, not over w L.
template <int KR, bool VAR>
__device__ __forceinline__ void cnet_embed_round_body(const CnetEmbedArgs &a) {
    extern __shared__ float lds[];
    __shared__ int32_t sid[kCnetMaxL], sslot[kCnetMaxL], fpos[kCnetMaxL];
    const int lane = threadIdx.x;
    const int L = a.L, dim = a.dim;
    const int rows1 = L * (a.negative + 1);
    float *cur0 = lds, *cur1 = lds + (size_t)L * dim;
    int32_t *ids1 = (int32_t *)(cur1 + (size_t)rows1 * dim);
    const int64_t w = a.w_begin + blockIdx.x;
    const uint64_t ew = (uint64_t)a.epoch;
    const int Lw = VAR ? a.len[w] : L;

    int32_t id = 0;
    bool keep = false;
    if (lane < Lw) {
        id = a.walks[w * L + lane];
        sid[lane] = id;
        keep = (cnet_hash(a.seed ^ kCnetTagSub, (uint64_t)w, ew, (uint64_t)lane, 0) >> 32) < a.keep[id];
    }
    __syncthreads();
    if (lane < Lw) {
        int s = lane;
        for (int q = lane - 1; q >= 0; --q) if (sid[q] == id) s = q;
        sslot[lane] = s;
    }
    const unsigned long long kmask = __ballot(keep);
    const int nk = __popcll(kmask);
    if (keep) fpos[__popcll(kmask & ((1ull << lane) - 1ull))] = lane;
    __syncthreads();
    for (int p = 0; p < Lw; ++p)
        if (sslot[p] == p)
            for (int r = 0; r < KR; ++r) {
                const int e = lane + 64 * r;
                if (e < dim) cur0[p * dim + e] = a.syn0[(int64_t)sid[p] * dim + e];
            }
    unsigned long long mod0 = 0ull;                    // slots of cur0 that were changed
    int n1 = 0;
    const double done = VAR ? (double)((int64_t)a.epoch * a.words + a.wpre[w]) / (double)((int64_t)a.epochs * a.words)
                            : (double)(((int64_t)a.epoch * a.nw + w) * L) / (double)((int64_t)a.epochs * a.nw * L);
    const float alpha = (float)(0.025 - (0.025 - 1e-4) * done);

    for (int kp = 0; kp < nk; ++kp) {
        const int p = fpos[kp];
        const int32_t word = sid[p];
        const int b = (int)(((cnet_hash(a.seed ^ kCnetTagWin, (uint64_t)w, ew, (uint64_t)p, 0) >> 32) * (uint64_t)a.window) >> 32);
        const int lo = kp - a.window + b > 0 ? kp - a.window + b : 0;
        const int hi = kp + a.window + 1 - b < nk ? kp + a.window + 1 - b : nk;
        const int count = hi - lo - 1;
        if (count == 0) continue;
        float neu1[KR], work[KR];
        for (int r = 0; r < KR; ++r) { neu1[r] = 0.0f; work[r] = 0.0f; }
        for (int c = lo; c < hi; ++c) {
            if (c == kp) continue;
            const int s = sslot[fpos[c]];
            for (int r = 0; r < KR; ++r) {
                const int e = lane + 64 * r;
                if (e < dim) neu1[r] = neu1[r] + cur0[s * dim + e];
            }
        }
        const float inv = 1.0f / (float)count;
        for (int r = 0; r < KR; ++r) neu1[r] = neu1[r] * inv;
        for (int d = 0; d <= a.negative; ++d) {
            int32_t tgt = word;
            if (d > 0) {
                const uint64_t rr = cnet_hash(a.seed ^ kCnetTagNeg, (uint64_t)w, ew, (uint64_t)p, (uint64_t)d) >> 32;
                int64_t l = 0, h = a.m - 1;                         // first id with cum > rr
                while (l < h) {
                    const int64_t mid = l + ((h - l) >> 1);
                    if (a.cum[mid] > rr) h = mid; else l = mid + 1;
                }
                tgt = (int32_t)l;
                if (tgt == word) continue;
            }
            int s = -1;
            for (int base = 0; base < n1 && s < 0; base += 64) {
                const unsigned long long hit = __ballot(base + lane < n1 && ids1[base + lane] == tgt);
                if (hit) s = base + __ffsll((long long)hit) - 1;
            }
            if (s < 0) {
                s = n1++;
                if (lane == 0) ids1[s] = tgt;
                for (int r = 0; r < KR; ++r) {
                    const int e = lane + 64 * r;
                    if (e < dim) cur1[s * dim + e] = a.syn1[(int64_t)tgt * dim + e];
                }
                __syncthreads();
            }
            float part = 0.0f;
            for (int r = 0; r < KR; ++r) {
                const int e = lane + 64 * r;
                if (e < dim) part = part + neu1[r] * cur1[s * dim + e];
            }
            const float f = wave_sum(part);
            if (f >= kCnetMaxExp || f <= -kCnetMaxExp) continue;
            const float g = ((d == 0 ? 1.0f : 0.0f) - 1.0f / (1.0f + expf(-f))) * alpha;
            for (int r = 0; r < KR; ++r) {
                const int e = lane + 64 * r;
                if (e < dim) {
                    const float row = cur1[s * dim + e];
                    work[r] = work[r] + g * row;
                    cur1[s * dim + e] = row + g * neu1[r];
                }
            }
        }
        for (int r = 0; r < KR; ++r) work[r] = work[r] * inv;
        for (int c = lo; c < hi; ++c) {
            if (c == kp) continue;
            const int s = sslot[fpos[c]];
            mod0 |= 1ull << s;
            for (int r = 0; r < KR; ++r) {
                const int e = lane + 64 * r;
                if (e < dim) cur0[s * dim + e] = cur0[s * dim + e] + work[r];
            }
        }
    }
    // the walk's differences against the round-start rows, in fixed point
    int32_t *list = a.list + (int64_t)blockIdx.x * (L + rows1);
    int nl = 0;
    for (int p = 0; p < Lw; ++p) {
        if (!((mod0 >> p) & 1ull)) continue;
        const int64_t row = sid[p];
        for (int r = 0; r < KR; ++r) {
            const int e = lane + 64 * r;
            if (e < dim) {
                const float diff = cur0[p * dim + e] - a.syn0[row * dim + e];
                atomicAdd((unsigned long long *)&a.acc0[row * dim + e], (unsigned long long)__double2ll_rn((double)diff * kCnetFix));
            }
        }
        if (lane == 0) { a.flag0[row] = 1; list[nl] = (int32_t)row; }
        ++nl;
    }
    for (int s = 0; s < n1; ++s) {
        const int64_t row = ids1[s];
        for (int r = 0; r < KR; ++r) {
            const int e = lane + 64 * r;
            if (e < dim) {
                const float diff = cur1[s * dim + e] - a.syn1[row * dim + e];
                atomicAdd((unsigned long long *)&a.acc1[row * dim + e], (unsigned long long)__double2ll_rn((double)diff * kCnetFix));
            }
        }
        if (lane == 0) { a.flag1[row] = 1; list[nl] = -(int32_t)row - 1; }
        ++nl;
    }
    if (lane == 0) a.list_n[blockIdx.x] = nl;
}

template <int KR>
__global__ __launch_bounds__(64) void k_cnet_embed_round(CnetEmbedArgs a) { cnet_embed_round_body<KR, false>(a); }
// ... of a round of segments (yue_cnet_set_sentences)
template <int KR>
__global__ __launch_bounds__(64) void k_sent_embed_round(CnetEmbedArgs a) { cnet_embed_round_body<KR, true>(a); }

// One wave per walk of the finished round: every flagged row is applied once (whichever wave clears the flag first; the
// value does not depend on which): row = fp32(fp64(row) + sum * 2^-36), sum = 0.
__global__ __launch_bounds__(64) void k_cnet_embed_apply(CnetEmbedArgs a) {
    const int lane = threadIdx.x;
    const int32_t *list = a.list + (int64_t)blockIdx.x * (a.L + a.L * (a.negative + 1));
    const int nl = a.list_n[blockIdx.x];
    for (int j = 0; j < nl; ++j) {
        const int32_t x = list[j];
        const int64_t row = x >= 0 ? x : -(int64_t)x - 1;
        int won = 0;
        if (lane == 0) won = atomicExch(x >= 0 ? &a.flag0[row] : &a.flag1[row], 0);
        if (!__shfl(won, 0)) continue;
        float *M = x >= 0 ? a.syn0 : a.syn1;
        long long *acc = x >= 0 ? a.acc0 : a.acc1;
        for (int e = lane; e < a.dim; e += 64) {
            M[row * a.dim + e] = (float)((double)M[row * a.dim + e] + (double)acc[row * a.dim + e] * kCnetUnfix);
            acc[row * a.dim + e] = 0;
        }
    }
}

// ---- friends ----
constexpr int kCnetFrThreads = 256;
constexpr int kCnetFrQ = 8;                // query rows per workgroup
constexpr int kCnetFrTile = 64;            // candidate rows per tile
constexpr int kCnetFrList = 256;           // running top-K + appended candidates per query
constexpr int kCnetFrStride = kCnetMaxDim + 1;
static_assert((kCnetFrList & (kCnetFrList - 1)) == 0 && kCnetFrList >= kCnetMaxK + kCnetFrTile, "running top-K + one tile of appends");

struct CnetFriendsArgs {
    int64_t m, nnet;
    const int32_t *net;        // the users with an embedding row, ascending
    const float *W;            // [m][dim]
    double *norm;              // [m] sum of squares in fp64
    int dim, K;
    int32_t *friends;          // [m][K] -1 padded
    double *sims;              // [m][K] 0 padded
};

__global__ void k_cnet_norms(CnetFriendsArgs a) {
    const int64_t u = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (u >= a.m) return;
    double s = 0.0;
    for (int d = 0; d < a.dim; ++d) {
        const double x = (double)a.W[u * a.dim + d];
        s = s + x * x;
    }
    a.norm[u] = s;
    for (int r = 0; r < a.K; ++r) { a.friends[u * a.K + r] = -1; a.sims[u * a.K + r] = 0.0; }
}

// Workgroup b ranks the query users net[8b .. 8b + 8) against every network user, 64 candidate rows at a time.  Thread t
// takes candidate t & 63 for the two queries 2 (t >> 6), + 1.  cosine = dot / sqrt(n_a n_b) in fp64 (tool/qmath.py:36-45;
// 0 where a norm is 0: the reference's ZeroDivisionError branch).  A candidate that beats the running K-th entry is
// appended behind the query's list; the lists are re-formed by one bitonic sort of all eight whenever an appended block
// could overflow, and at the end.
__global__ __launch_bounds__(kCnetFrThreads) void k_cnet_friends(CnetFriendsArgs a) {
    __shared__ float qrow[kCnetFrQ][kCnetMaxDim];
    __shared__ float tile[kCnetFrTile][kCnetFrStride];
    __shared__ double ls[kCnetFrQ][kCnetFrList];
    __shared__ int32_t li[kCnetFrQ][kCnetFrList];
    __shared__ double qn[kCnetFrQ], tn[kCnetFrTile];
    __shared__ int32_t tid_[kCnetFrTile];
    __shared__ int nl[kCnetFrQ], nc[kCnetFrQ];
    const int tid = threadIdx.x;
    const int dim = a.dim, K = a.K;
    const int64_t q0 = (int64_t)blockIdx.x * kCnetFrQ;
    const int nq = (int)(a.nnet - q0 < kCnetFrQ ? a.nnet - q0 : kCnetFrQ);
    for (int x = tid; x < kCnetFrQ * dim; x += kCnetFrThreads) {
        const int q = x / dim, d = x % dim;
        qrow[q][d] = q < nq ? a.W[(int64_t)a.net[q0 + q] * dim + d] : 0.0f;
    }
    if (tid < kCnetFrQ) { qn[tid] = tid < nq ? a.norm[a.net[q0 + tid]] : 0.0; nl[tid] = 0; nc[tid] = 0; }
    __syncthreads();

    double *fs = &ls[0][0];                // the eight lists back to back, by flat index
    int32_t *fi = &li[0][0];
    auto less = [&](int x, int y) { return wg_before(fs[x], fi[x], fs[y], fi[y]); };
    auto swap = [&](int x, int y) {
        const double s = fs[x]; fs[x] = fs[y]; fs[y] = s;
        const int32_t v = fi[x]; fi[x] = fi[y]; fi[y] = v;
    };
    auto merge = [&]() {                   // all threads; sorts the eight lists at once
        for (int x = tid; x < kCnetFrQ * kCnetFrList; x += kCnetFrThreads) {
            const int q = x / kCnetFrList, i = x % kCnetFrList;
            if (i >= nl[q] + nc[q]) { ls[q][i] = -INFINITY; li[q][i] = INT_MAX; }
        }
        __syncthreads();
        wg_bitonic<kCnetFrThreads>(kCnetFrQ, kCnetFrList, less, swap);
        if (tid < kCnetFrQ) { const int tot = nl[tid] + nc[tid]; nl[tid] = tot < K ? tot : K; nc[tid] = 0; }
        __syncthreads();
    };

    for (int64_t c0 = 0; c0 < a.nnet; c0 += kCnetFrTile) {
        const int nt = (int)(a.nnet - c0 < kCnetFrTile ? a.nnet - c0 : kCnetFrTile);
        bool full = false;
        for (int q = 0; q < kCnetFrQ; ++q) full |= nl[q] + nc[q] + kCnetFrTile > kCnetFrList;
        __syncthreads();
        if (full) merge();
        for (int x = tid; x < kCnetFrTile * dim; x += kCnetFrThreads) {
            const int c = x / dim, d = x % dim;
            tile[c][d] = c < nt ? a.W[(int64_t)a.net[c0 + c] * dim + d] : 0.0f;
        }
        if (tid < kCnetFrTile) {
            tid_[tid] = tid < nt ? a.net[c0 + tid] : -1;
            tn[tid] = tid < nt ? a.norm[a.net[c0 + tid]] : 0.0;
        }
        __syncthreads();
        const int c = tid & 63, qa = 2 * (tid >> 6);
        double d0 = 0.0, d1 = 0.0;
        for (int d = 0; d < dim; ++d) {
            const double x = (double)tile[c][d];
            d0 = d0 + (double)qrow[qa][d] * x;
            d1 = d1 + (double)qrow[qa + 1][d] * x;
        }
        const int32_t v = tid_[c];
        for (int h = 0; h < 2; ++h) {
            const int q = qa + h;
            if (q >= nq || v < 0 || v == a.net[q0 + q]) continue;
            const double den = sqrt(qn[q] * tn[c]);
            const double s = den == 0.0 ? 0.0 : (h ? d1 : d0) / den;
            if (nl[q] < K || wg_before(s, v, ls[q][K - 1], li[q][K - 1])) {
                const int at = nl[q] + atomicAdd(&nc[q], 1);
                ls[q][at] = s; li[q][at] = v;
            }
        }
        __syncthreads();
    }
    merge();
    for (int x = tid; x < nq * K; x += kCnetFrThreads) {
        const int q = x / K, r = x % K;
        if (r < nl[q]) {
            const int64_t u = a.net[q0 + q];
            a.friends[u * K + r] = li[q][r];
            a.sims[u * K + r] = ls[q][r];
        }
    }
}

}  // namespace yue
