// libyue_hip.so -- CUNE's user-network stage (recommender/advanced/CUNE.py:34-118): implicit collaborative user network,
// random walks, CBOW user embedding in rounds, cosine top-K friends (include/yue_hip.h).  Kernels: cnet_kernels.hpp.
// Needs no factors: the state is the pair lists of yue_cnet_set_pairs, the walks and the embedding.
#include "host_common.hpp"

#include "cnet_kernels.hpp"

#include <numeric>

using yue_host::fail;
using yue_host::upload;

struct yue_cnet {
    int64_t m = 0, n = 0, nnz = 0;               // pairs (m == 0: none)
    DevBuf<int64_t> u_ptr, i_ptr, pref, total, dest;
    DevBuf<int32_t> u_items, i_users;
    std::vector<int32_t> net_pairs;              // users with total > 0, ascending
    // walks, in training (shuffled) order
    int64_t wm = 0, nw = 0;                      // wm: users the walk ids are below
    int L = 0;
    DevBuf<int32_t> walks, cnt, list, list_n, net, friends;
    // sentences of unequal length (yue_cnet_set_sentences), kept on the host: yue_cnet_embed cuts them into segments
    // once it knows dim and negative
    bool sent = false;
    std::vector<int64_t> s_ptr;
    std::vector<int32_t> s_ids;
    DevBuf<int32_t> seg_len;
    DevBuf<int64_t> seg_pre;
    // embedding
    int64_t em = 0, nnet = 0;                    // em == 0: none
    int dim = 0;
    DevBuf<float> syn0, syn1;
    DevBuf<long long> acc0, acc1;
    DevBuf<int> flag0, flag1;
    DevBuf<uint64_t> keep, cum;
    DevBuf<double> norm, sims;
    Event ev[2];
};

namespace {

constexpr int kDefaultRoundWalks = 64;       // chosen by the planted-groups quality test

int stop_clock(yue_ctx *c, yue_cnet *k) {
    HIPCHK(k->ev[1].record(c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(yue_host::elapsed(k->ev[0], k->ev[1], &c->cnet_ns));
    return YUE_OK;
}

// the walks on the device changed: whatever was trained on the old ones is gone
void new_walks(yue_cnet *k, int64_t wm, int64_t nw, int L) { k->wm = wm; k->nw = nw; k->L = L; k->em = 0; k->sent = false; }

}  // namespace

extern "C" {

int yue_cnet_set_pairs(yue_ctx *c, int64_t m, int64_t n, const int64_t *u_ptr, const int32_t *u_items, const int64_t *i_ptr,
                       const int32_t *i_users, int64_t nnz) {
    if (!c) return fail(YUE_ERR_ARG, "yue_cnet_set_pairs: null context");
    if (m < 1 || n < 1 || nnz < 0 || m >= INT32_MAX || n >= INT32_MAX) return fail(YUE_ERR_ARG, "yue_cnet_set_pairs: need 1 <= m, n < 2^31 - 1 and nnz >= 0");
    int rc = check_rows("yue_cnet_set_pairs: user-major", u_ptr, m, u_items, n, nnz, Order::ascending);
    if (!rc) rc = check_rows("yue_cnet_set_pairs: item-major", i_ptr, n, i_users, m, nnz, Order::ascending);
    // (the skip-self index relies on the transpose)
    if (!rc) rc = check_transpose("yue_cnet_set_pairs", m, u_ptr, u_items, n, i_ptr, i_users, [](int64_t, int64_t) { return true; });
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    yue_cnet *k = nullptr;
    if ((rc = yue_host::state(c, c->cnet, &k))) return rc;
    k->m = 0;
    if ((rc = upload(k->u_ptr, u_ptr, m + 1)) || (rc = upload(k->u_items, u_items, nnz)) || (rc = upload(k->i_ptr, i_ptr, n + 1)) ||
        (rc = upload(k->i_users, i_users, nnz)))
        return rc;
    HIPCHK(k->pref.resize((size_t)std::max<int64_t>(nnz, 1)));
    HIPCHK(k->total.resize((size_t)m));
    yue::CnetArgs a{};
    a.m = m; a.n = n; a.u_ptr = k->u_ptr.p; a.u_items = k->u_items.p; a.i_ptr = k->i_ptr.p; a.i_users = k->i_users.p;
    a.pref = k->pref.p; a.total = k->total.p;
    hipLaunchKernelGGL(yue::k_cnet_prefix, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, c->stream, a);
    HIPCHK(hipGetLastError());
    std::vector<int64_t> total((size_t)m);
    HIPCHK(hipMemcpyAsync(total.data(), k->total.p, (size_t)m * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    k->net_pairs.clear();
    for (int64_t u = 0; u < m; ++u) if (total[(size_t)u] > 0) k->net_pairs.push_back((int32_t)u);
    k->m = m; k->n = n; k->nnz = nnz;
    return YUE_OK;
}

int yue_cnet_walks(yue_ctx *c, int T, int L, uint64_t seed, int32_t *walks_out, int64_t *nw_out) {
    if (!c || !nw_out) return fail(YUE_ERR_ARG, "yue_cnet_walks: null argument");
    yue_cnet *k = c->cnet.get();
    if (!k || k->m == 0) return fail(YUE_ERR_ARG, "yue_cnet_walks: call yue_cnet_set_pairs first");
    if (T < 1 || L < 2 || L > yue::kCnetMaxL || (int64_t)T * (L - 1) > yue::kCnetMaxVisited)
        return fail(YUE_ERR_ARG, "yue_cnet_walks: need T >= 1, 2 <= L <= 64 and T (L - 1) <= 15360 (visited[start] lives in LDS)");
    const int64_t nnet = (int64_t)k->net_pairs.size(), nw = nnet * T;
    if (nw * L >= INT32_MAX) return fail(YUE_ERR_ARG, "yue_cnet_walks: more than 2^31 walk entries");
    *nw_out = nw;
    new_walks(k, k->m, 0, L);
    if (nw == 0) return YUE_OK;
    HIPCHK(hipSetDevice(c->device));
    // shuffle(self.walks) (:74): the walks ordered by (cnet_hash(seed ^ shuffle tag, walk), walk)
    std::vector<uint64_t> key((size_t)nw);
    for (int64_t w = 0; w < nw; ++w) key[(size_t)w] = yue::cnet_hash(seed ^ yue::kCnetTagShuffle, (uint64_t)w, 0, 0, 0);
    std::vector<int64_t> order((size_t)nw), dest((size_t)nw);
    std::iota(order.begin(), order.end(), (int64_t)0);
    std::sort(order.begin(), order.end(), [&](int64_t x, int64_t y) { return key[(size_t)x] < key[(size_t)y] || (key[(size_t)x] == key[(size_t)y] && x < y); });
    for (int64_t r = 0; r < nw; ++r) dest[(size_t)order[(size_t)r]] = r;
    int rc;
    if ((rc = upload(k->dest, dest.data(), nw)) || (rc = upload(k->net, k->net_pairs.data(), nnet))) return rc;
    HIPCHK(k->walks.resize((size_t)(nw * L)));
    yue::CnetArgs a{};
    a.m = k->m; a.n = k->n; a.u_ptr = k->u_ptr.p; a.u_items = k->u_items.p; a.i_ptr = k->i_ptr.p; a.i_users = k->i_users.p;
    a.pref = k->pref.p; a.total = k->total.p; a.net = k->net.p; a.dest = k->dest.p; a.walks = k->walks.p; a.T = T; a.L = L; a.seed = seed;
    HIPCHK(k->ev[0].record(c->stream));
    hipLaunchKernelGGL(yue::k_cnet_walk, dim3((unsigned)nnet), dim3(64), (size_t)T * (L - 1) * sizeof(int32_t), c->stream, a);
    HIPCHK(hipGetLastError());
    if ((rc = stop_clock(c, k))) return rc;
    if (walks_out) HIPCHK(hipMemcpy(walks_out, k->walks.p, (size_t)(nw * L) * sizeof(int32_t), hipMemcpyDeviceToHost));
    new_walks(k, k->m, nw, L);
    return YUE_OK;
}

int yue_cnet_set_walks(yue_ctx *c, int64_t m, int64_t nw, int L, const int32_t *walks) {
    if (!c) return fail(YUE_ERR_ARG, "yue_cnet_set_walks: null context");
    if (m < 1 || m >= INT32_MAX || nw < 1 || L < 2 || L > yue::kCnetMaxL || nw * L >= INT32_MAX || !walks)
        return fail(YUE_ERR_ARG, "yue_cnet_set_walks: need 1 <= m < 2^31 - 1, nw >= 1, 2 <= L <= 64, fewer than 2^31 entries");
    int rc = check_ids("yue_cnet_set_walks: user", walks, nw * L, m);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    yue_cnet *k = nullptr;
    if ((rc = yue_host::state(c, c->cnet, &k))) return rc;
    new_walks(k, m, 0, L);
    if ((rc = upload(k->walks, walks, nw * L))) return rc;
    new_walks(k, m, nw, L);
    return YUE_OK;
}

int yue_cnet_set_sentences(yue_ctx *c, int64_t m, int64_t ns, const int64_t *ptr, const int32_t *ids) {
    if (!c) return fail(YUE_ERR_ARG, "yue_cnet_set_sentences: null context");
    if (m < 1 || m >= INT32_MAX || ns < 1 || !ptr || ptr[0] != 0 || ptr[ns] < 1 || ptr[ns] >= INT32_MAX || !ids)
        return fail(YUE_ERR_ARG, "yue_cnet_set_sentences: need 1 <= m < 2^31 - 1, ns >= 1, a pointer from 0 to the words, 1 <= words < 2^31 - 1");
    int rc = check_rows("yue_cnet_set_sentences: sentence", ptr, ns, ids, m, yue_host::kNoTotal, Order::any);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    yue_cnet *k = nullptr;
    if ((rc = yue_host::state(c, c->cnet, &k))) return rc;
    new_walks(k, m, 0, 0);
    k->s_ptr.assign(ptr, ptr + ns + 1);
    k->s_ids.assign(ids, ids + ptr[ns]);
    k->sent = true;
    return YUE_OK;
}

int yue_cnet_embed(yue_ctx *c, int dim, int window, int epochs, int negative, int64_t round_walks, uint64_t seed, float *W_out) {
    if (!c) return fail(YUE_ERR_ARG, "yue_cnet_embed: null context");
    yue_cnet *k = c->cnet.get();
    if (!k || (k->nw == 0 && !k->sent)) return fail(YUE_ERR_ARG, "yue_cnet_embed: call yue_cnet_walks or yue_cnet_set_walks first (or yue_cnet_set_sentences)");
    if (dim < 1 || dim > yue::kCnetMaxDim || window < 1 || epochs < 1 || negative < 0 || negative > 64 || round_walks < 0)
        return fail(YUE_ERR_ARG, "yue_cnet_embed: need 1 <= dim <= 128, window >= 1, epochs >= 1, 0 <= negative <= 64, round_walks >= 0");
    const int64_t m = k->wm;
    const bool sent = k->sent;
    const auto lds_of = [&](int len) { return (size_t)len * (negative + 2) * dim * sizeof(float) + (size_t)len * (negative + 1) * sizeof(int32_t); };
    std::vector<int32_t> seg_ids, seg_len;
    std::vector<int64_t> seg_pre;
    if (sent) {
        // segments of at most S words: the largest S <= 64 whose S (negative + 2) rows of dim floats fit 60 KiB (and, with
        // the target ids behind them, the workgroup's LDS); windows do not cross a cut
        int S = yue::kCnetMaxL;
        while (S > 0 && ((size_t)S * (negative + 2) * dim * sizeof(float) > (size_t)yue::kCnetEmbedLds || lds_of(S) > (size_t)yue::kCnetSegmentLds)) --S;
        if (S < 2 * window + 1)
            return fail(YUE_ERR_ARG, "yue_cnet_embed: a segment holds " + std::to_string(S) + " words at this dim and negative, fewer than 2 window + 1");
        const int64_t ns = (int64_t)k->s_ptr.size() - 1;
        for (int64_t q = 0; q < ns; ++q)
            for (int64_t b = k->s_ptr[(size_t)q]; b < k->s_ptr[(size_t)q + 1]; b += S) {
                const int64_t e = std::min<int64_t>(b + S, k->s_ptr[(size_t)q + 1]);
                seg_pre.push_back(b);                      // the words passed: a prefix of the lengths
                seg_len.push_back((int32_t)(e - b));
                seg_ids.insert(seg_ids.end(), k->s_ids.begin() + b, k->s_ids.begin() + e);
                seg_ids.resize(seg_len.size() * (size_t)S, 0);
            }
        if ((int64_t)seg_ids.size() >= INT32_MAX) return fail(YUE_ERR_ARG, "yue_cnet_embed: more than 2^31 segment entries");
        k->nw = (int64_t)seg_len.size(); k->L = S;
    }
    const int64_t nw = k->nw;
    const int L = k->L, rows = L * (negative + 2);
    const size_t lds = lds_of(L);
    if (!sent && lds > (size_t)yue::kCnetEmbedLds)
        return fail(YUE_ERR_ARG, "yue_cnet_embed: L (negative + 2) rows of dim floats must fit 60 KiB of LDS (a walk's working rows)");
    if (m * dim >= ((int64_t)1 << 40)) return fail(YUE_ERR_ARG, "yue_cnet_embed: m dim is too large");
    if (round_walks == 0) round_walks = kDefaultRoundWalks;
    round_walks = std::min<int64_t>(round_walks, std::min<int64_t>(nw, 1 << 20));
    HIPCHK(hipSetDevice(c->device));
    const size_t cells = (size_t)(m * dim);
    k->em = 0;
    HIPCHK(k->cnt.resize((size_t)m)); HIPCHK(k->keep.resize((size_t)m)); HIPCHK(k->cum.resize((size_t)m));
    HIPCHK(k->syn0.resize(cells)); HIPCHK(k->syn1.resize(cells)); HIPCHK(k->acc0.resize(cells)); HIPCHK(k->acc1.resize(cells));
    HIPCHK(k->flag0.resize((size_t)m)); HIPCHK(k->flag1.resize((size_t)m));
    HIPCHK(k->list.resize((size_t)(round_walks * rows))); HIPCHK(k->list_n.resize((size_t)round_walks));
    HIPCHK(hipMemsetAsync(k->cnt.p, 0, (size_t)m * sizeof(int32_t), c->stream));
    HIPCHK(hipMemsetAsync(k->acc0.p, 0, cells * sizeof(long long), c->stream));
    HIPCHK(hipMemsetAsync(k->acc1.p, 0, cells * sizeof(long long), c->stream));
    HIPCHK(hipMemsetAsync(k->flag0.p, 0, (size_t)m * sizeof(int), c->stream));
    HIPCHK(hipMemsetAsync(k->flag1.p, 0, (size_t)m * sizeof(int), c->stream));
    const int64_t words = sent ? (int64_t)k->s_ids.size() : nw * L;
    if (sent) {
        int rcs;
        if ((rcs = upload(k->walks, seg_ids.data(), nw * L)) || (rcs = upload(k->seg_len, seg_len.data(), nw)) || (rcs = upload(k->seg_pre, seg_pre.data(), nw))) return rcs;
        hipLaunchKernelGGL(yue::k_sent_count, dim3((unsigned)((nw * L + 255) / 256)), dim3(256), 0, c->stream, k->walks.p, k->seg_len.p, nw * L, L, k->cnt.p);
    } else
        hipLaunchKernelGGL(yue::k_cnet_count, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, c->stream, k->walks.p, words, k->cnt.p);
    HIPCHK(hipGetLastError());
    std::vector<int32_t> cnt((size_t)m);
    HIPCHK(hipMemcpyAsync(cnt.data(), k->cnt.p, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    // subsampling at 1e-3 and the unigram^0.75 table, as 32-bit thresholds.  c^0.75 = sqrt(c) sqrt(sqrt(c)): correctly
    // rounded operations only, so that the contract's NumPy gives the same bits
    std::vector<uint64_t> keep((size_t)m, 0), cum((size_t)m, 0);
    std::vector<int32_t> net;
    const double thr = 1e-3 * (double)words, two32 = 4294967296.0;
    double z = 0.0;
    for (int64_t u = 0; u < m; ++u)
        if (cnt[(size_t)u] > 0) { const double x = (double)cnt[(size_t)u]; z = z + std::sqrt(x) * std::sqrt(std::sqrt(x)); net.push_back((int32_t)u); }
    double run = 0.0;
    for (int64_t u = 0; u < m; ++u) {
        if (cnt[(size_t)u] > 0) {
            const double x = (double)cnt[(size_t)u];
            const double p = (std::sqrt(x / thr) + 1.0) * (thr / x);
            keep[(size_t)u] = p >= 1.0 ? (uint64_t)two32 : (uint64_t)(p * two32);
            run = run + std::sqrt(x) * std::sqrt(std::sqrt(x));
        }
        cum[(size_t)u] = std::min<uint64_t>((uint64_t)(run / z * two32), (uint64_t)two32);
    }
    for (int64_t u = m - 1; u >= 0; --u) {             // the last user of the table closes it, whatever the rounding of run / z
        cum[(size_t)u] = (uint64_t)two32;
        if (cnt[(size_t)u] > 0) break;
    }
    int rc;
    if ((rc = upload(k->keep, keep.data(), m)) || (rc = upload(k->cum, cum.data(), m)) || (rc = upload(k->net, net.data(), (int64_t)net.size()))) return rc;
    yue::CnetEmbedArgs a{};
    a.m = m; a.nw = nw; a.walks = k->walks.p; a.cnt = k->cnt.p; a.keep = k->keep.p; a.cum = k->cum.p;
    a.syn0 = k->syn0.p; a.syn1 = k->syn1.p; a.acc0 = k->acc0.p; a.acc1 = k->acc1.p; a.flag0 = k->flag0.p; a.flag1 = k->flag1.p;
    a.list = k->list.p; a.list_n = k->list_n.p;
    if (sent) { a.len = k->seg_len.p; a.wpre = k->seg_pre.p; a.words = words; }
    a.L = L; a.dim = dim; a.window = window; a.negative = negative; a.epochs = epochs; a.seed = seed;
    HIPCHK(k->ev[0].record(c->stream));
    hipLaunchKernelGGL(yue::k_cnet_embed_init, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, c->stream, a);
    HIPCHK(hipGetLastError());
    for (int ep = 0; ep < epochs; ++ep)
        for (int64_t w0 = 0; w0 < nw; w0 += round_walks) {
            a.epoch = ep; a.w_begin = w0; a.w_count = std::min(round_walks, nw - w0);
            if (sent) {
                if (dim <= 64) hipLaunchKernelGGL(yue::k_sent_embed_round<1>, dim3((unsigned)a.w_count), dim3(64), lds, c->stream, a);
                else hipLaunchKernelGGL(yue::k_sent_embed_round<2>, dim3((unsigned)a.w_count), dim3(64), lds, c->stream, a);
            } else if (dim <= 64) hipLaunchKernelGGL(yue::k_cnet_embed_round<1>, dim3((unsigned)a.w_count), dim3(64), lds, c->stream, a);
            else hipLaunchKernelGGL(yue::k_cnet_embed_round<2>, dim3((unsigned)a.w_count), dim3(64), lds, c->stream, a);
            hipLaunchKernelGGL(yue::k_cnet_embed_apply, dim3((unsigned)a.w_count), dim3(64), 0, c->stream, a);
        }
    HIPCHK(hipGetLastError());
    if ((rc = stop_clock(c, k))) return rc;
    if (W_out) HIPCHK(hipMemcpy(W_out, k->syn0.p, cells * sizeof(float), hipMemcpyDeviceToHost));
    k->em = m; k->dim = dim; k->nnet = (int64_t)net.size();
    return YUE_OK;
}

int yue_cnet_set_embedding(yue_ctx *c, int64_t m, int dim, const float *W, const int32_t *users, int64_t nu) {
    if (!c) return fail(YUE_ERR_ARG, "yue_cnet_set_embedding: null context");
    if (m < 1 || m >= INT32_MAX || dim < 1 || dim > yue::kCnetMaxDim || !W || nu < 0 || nu > m)
        return fail(YUE_ERR_ARG, "yue_cnet_set_embedding: need 1 <= m < 2^31 - 1, 1 <= dim <= 128, 0 <= users <= m");
    std::vector<int32_t> net;
    if (users) {
        for (int64_t t = 0; t < nu; ++t) {
            if (users[t] < 0 || users[t] >= m || (t > 0 && users[t] <= users[t - 1]))
                return fail(YUE_ERR_ARG, "yue_cnet_set_embedding: users must be ascending ids below m");
            net.push_back(users[t]);
        }
    } else {
        net.resize((size_t)m);
        std::iota(net.begin(), net.end(), 0);
    }
    HIPCHK(hipSetDevice(c->device));
    yue_cnet *k = nullptr;
    int rc = yue_host::state(c, c->cnet, &k);
    if (rc) return rc;
    k->em = 0;
    if ((rc = upload(k->syn0, W, m * dim)) || (rc = upload(k->net, net.data(), (int64_t)net.size()))) return rc;
    k->em = m; k->dim = dim; k->nnet = (int64_t)net.size();
    return YUE_OK;
}

int yue_cnet_friends(yue_ctx *c, int K, int32_t *friends_out, double *sims_out) {
    if (!c) return fail(YUE_ERR_ARG, "yue_cnet_friends: null context");
    yue_cnet *k = c->cnet.get();
    if (!k || k->em == 0) return fail(YUE_ERR_ARG, "yue_cnet_friends: call yue_cnet_embed or yue_cnet_set_embedding first");
    if (K < 1 || K > yue::kCnetMaxK) return fail(YUE_ERR_ARG, "yue_cnet_friends: K = " + std::to_string(K) + " is not supported (1 <= K <= 100)");
    HIPCHK(hipSetDevice(c->device));
    const int64_t m = k->em;
    const size_t cells = (size_t)m * (size_t)K;
    HIPCHK(k->norm.resize((size_t)m)); HIPCHK(k->friends.resize(cells)); HIPCHK(k->sims.resize(cells));
    yue::CnetFriendsArgs a{};
    a.m = m; a.nnet = k->nnet; a.net = k->net.p; a.W = k->syn0.p; a.norm = k->norm.p; a.dim = k->dim; a.K = K;
    a.friends = k->friends.p; a.sims = k->sims.p;
    HIPCHK(k->ev[0].record(c->stream));
    hipLaunchKernelGGL(yue::k_cnet_norms, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, c->stream, a);
    if (k->nnet > 0)
        hipLaunchKernelGGL(yue::k_cnet_friends, dim3((unsigned)((k->nnet + yue::kCnetFrQ - 1) / yue::kCnetFrQ)), dim3(yue::kCnetFrThreads), 0, c->stream, a);
    HIPCHK(hipGetLastError());
    int rc = stop_clock(c, k);
    if (rc) return rc;
    if (friends_out) HIPCHK(hipMemcpy(friends_out, k->friends.p, cells * sizeof(int32_t), hipMemcpyDeviceToHost));
    if (sims_out) HIPCHK(hipMemcpy(sims_out, k->sims.p, cells * sizeof(double), hipMemcpyDeviceToHost));
    return YUE_OK;
}

}  // extern "C"
