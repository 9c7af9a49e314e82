// libyue_hip.so -- UserKNN (recommender/cf/UserKNN.py): exact top-K user neighbours and neighbourhood ranking (include/yue_hip.h).
// Kernels: knn_kernels.hpp.  Needs no factors: the state is the pair lists of yue_knn_set_pairs and the neighbour lists.
#include "host_common.hpp"

#include "knn_kernels.hpp"

#include <numeric>

using yue_host::fail;
using yue_host::upload;

static_assert(yue_host::kKnnRangeHost == yue::kKnnRange && yue_host::kKnnMaxKHost == yue::kKnnMaxK && yue_host::kKnnGatherHost == yue::kKnnGather,
              "the option table's ends of knn_range and knn_gather are the kernels' widths");

struct yue_knn {
    int64_t m = 0, n = 0, nnz = 0;
    DevBuf<int64_t> u_ptr, i_ptr, cursor;
    DevBuf<int32_t> u_items, u_counts, i_users;
    int K = 0;                               // 0: no neighbour lists yet
    DevBuf<int32_t> nbr, inter, uni;
    DevBuf<int32_t> users, ids, len;
    DevBuf<double> scores;
    DevBuf<int> chunked;
    Event ev[2];
};

namespace {

yue::KnnArgs base_args(const yue_ctx *c, const yue_knn *k) {
    yue::KnnArgs a{};
    a.m = k->m; a.n = k->n;
    a.u_ptr = k->u_ptr.p; a.u_items = k->u_items.p; a.u_counts = k->u_counts.p;
    a.i_ptr = k->i_ptr.p; a.i_users = k->i_users.p;
    a.K = k->K; a.range = c->opt_knn_range; a.gather = c->opt_knn_gather;
    a.nbr = k->nbr.p; a.inter = k->inter.p; a.uni = k->uni.p;
    return a;
}

int ready(yue_ctx *c, const char *who, yue_knn **out) {
    if (!c) return fail(YUE_ERR_ARG, std::string(who) + ": null context");
    if (!c->knn || c->knn->m == 0) return fail(YUE_ERR_ARG, std::string(who) + ": call yue_knn_set_pairs first");
    if (c->knn->K == 0) return fail(YUE_ERR_ARG, std::string(who) + ": call yue_knn_neighbors first");
    *out = c->knn.get();
    return YUE_OK;
}

}  // namespace

extern "C" {

int yue_knn_set_pairs(yue_ctx *c, int64_t m, int64_t n, const int64_t *u_ptr, const int32_t *u_items, const int32_t *u_counts,
                      const int64_t *i_ptr, const int32_t *i_users, int64_t nnz) {
    if (!c) return fail(YUE_ERR_ARG, "yue_knn_set_pairs: null context");
    if (m < 1 || n < 1 || nnz < 0) return fail(YUE_ERR_ARG, "yue_knn_set_pairs: need m >= 1, n >= 1, nnz >= 0");
    if (m >= INT32_MAX || n >= ((int64_t)1 << 26))
        return fail(YUE_ERR_ARG, "yue_knn_set_pairs: m must be below 2^31 - 1 and n below 2^26 (similarities are compared as exact integer ratios)");
    if (nnz > 0 && !u_counts) return fail(YUE_ERR_ARG, "yue_knn_set_pairs: null user-major counts");
    int rc = check_rows("yue_knn_set_pairs: user-major", u_ptr, m, u_items, n, nnz, Order::ascending, yue_host::kNoLimit,
                        [&](int64_t, int64_t e) { return u_counts[e] < 1 ? "counts must be >= 1" : nullptr; });
    if (!rc) rc = check_rows("yue_knn_set_pairs: item-major", i_ptr, n, i_users, m, nnz, Order::ascending);
    // (users ascending within an item: the cursors rely on it)
    if (!rc) rc = check_transpose("yue_knn_set_pairs", m, u_ptr, u_items, n, i_ptr, i_users, [](int64_t, int64_t) { return true; });
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    yue_knn *k = nullptr;
    if ((rc = yue_host::state(c, c->knn, &k))) return rc;
    k->m = 0; k->K = 0;                                          // invalid until everything is up
    if ((rc = upload(k->u_ptr, u_ptr, m + 1)) || (rc = upload(k->u_items, u_items, nnz)) || (rc = upload(k->u_counts, u_counts, nnz)) ||
        (rc = upload(k->i_ptr, i_ptr, n + 1)) || (rc = upload(k->i_users, i_users, nnz)))
        return rc;
    HIPCHK(k->cursor.resize((size_t)std::max<int64_t>(nnz, 1)));
    HIPCHK(k->chunked.resize(1));
    k->m = m; k->n = n; k->nnz = nnz;
    return YUE_OK;
}

int yue_knn_neighbors(yue_ctx *c, int K, int32_t *nbr_out, int32_t *inter_out, int32_t *union_out) {
    if (!c) return fail(YUE_ERR_ARG, "yue_knn_neighbors: null context");
    yue_knn *k = c->knn.get();
    if (!k || k->m == 0) return fail(YUE_ERR_ARG, "yue_knn_neighbors: call yue_knn_set_pairs first");
    if (K < 1 || K > yue::kKnnMaxK) return fail(YUE_ERR_ARG, "yue_knn_neighbors: K = " + std::to_string(K) + " is not supported (1 <= K <= 256)");
    HIPCHK(hipSetDevice(c->device));
    const size_t cells = (size_t)k->m * (size_t)K;
    HIPCHK(k->nbr.resize(cells)); HIPCHK(k->inter.resize(cells)); HIPCHK(k->uni.resize(cells));
    k->K = K;
    yue::KnnArgs a = base_args(c, k);
    a.cursor = k->cursor.p;
    HIPCHK(k->ev[0].record(c->stream));
    hipLaunchKernelGGL(yue::k_knn_neighbors, dim3((unsigned)k->m), dim3(yue::kKnnThreads), 0, c->stream, a);
    HIPCHK(hipGetLastError());
    HIPCHK(k->ev[1].record(c->stream));
    if (nbr_out) HIPCHK(hipMemcpyAsync(nbr_out, k->nbr.p, cells * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (inter_out) HIPCHK(hipMemcpyAsync(inter_out, k->inter.p, cells * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    if (union_out) HIPCHK(hipMemcpyAsync(union_out, k->uni.p, cells * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(yue_host::elapsed(k->ev[0], k->ev[1], &c->knn_ns));
    return YUE_OK;
}

int yue_knn_topn(yue_ctx *c, const int32_t *users, int64_t nu, int N, int32_t *ids_out, double *scores_out, int32_t *len_out) {
    yue_knn *k = nullptr;
    int rc = ready(c, "yue_knn_topn", &k);
    if (rc) return rc;
    if (N < 1 || N > yue::kKnnMaxN) return fail(YUE_ERR_ARG, "yue_knn_topn: N = " + std::to_string(N) + " is not supported (1 <= N <= 100)");
    if (nu < 0 || nu >= INT32_MAX || (nu > 0 && (!users || !ids_out || !scores_out || !len_out)))
        return fail(YUE_ERR_ARG, "yue_knn_topn: need 0 <= nu < 2^31 - 1 and non-null arrays");
    if ((rc = check_ids("yue_knn_topn: user", users, nu, k->m))) return rc;
    if (nu == 0) return YUE_OK;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(k->users.resize((size_t)nu)); HIPCHK(k->ids.resize((size_t)nu * N)); HIPCHK(k->scores.resize((size_t)nu * N)); HIPCHK(k->len.resize((size_t)nu));
    HIPCHK(hipMemcpyAsync(k->users.p, users, (size_t)nu * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(k->chunked.p, 0, sizeof(int), c->stream));
    yue::KnnArgs a = base_args(c, k);
    a.users = k->users.p; a.N = N; a.exclude_own = 1;
    a.ids_out = k->ids.p; a.scores_out = k->scores.p; a.len_out = k->len.p; a.chunked_users = k->chunked.p;
    HIPCHK(k->ev[0].record(c->stream));
    hipLaunchKernelGGL(yue::k_knn_topn, dim3((unsigned)nu), dim3(yue::kKnnThreads), 0, c->stream, a);
    HIPCHK(hipGetLastError());
    HIPCHK(k->ev[1].record(c->stream));
    int chunked = 0;
    HIPCHK(hipMemcpyAsync(ids_out, k->ids.p, (size_t)nu * N * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(scores_out, k->scores.p, (size_t)nu * N * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(len_out, k->len.p, (size_t)nu * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(&chunked, k->chunked.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(yue_host::elapsed(k->ev[0], k->ev[1], &c->knn_ns));
    c->knn_chunked_users = chunked;
    return YUE_OK;
}

int yue_knn_predict(yue_ctx *c, int32_t user, int64_t cap, int32_t *items_out, double *scores_out, int64_t *len_out) {
    yue_knn *k = nullptr;
    int rc = ready(c, "yue_knn_predict", &k);
    if (rc) return rc;
    if (user < 0 || user >= k->m) return fail(YUE_ERR_ARG, "yue_knn_predict: user id out of range");
    if (cap < 0 || (cap > 0 && (!items_out || !scores_out)) || !len_out) return fail(YUE_ERR_ARG, "yue_knn_predict: need cap >= 0 and non-null arrays");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(k->scores.resize((size_t)k->n));
    yue::KnnArgs a = base_args(c, k);
    a.user = user; a.item_scores = k->scores.p;
    HIPCHK(k->ev[0].record(c->stream));
    hipLaunchKernelGGL(yue::k_knn_predict_scores, dim3((unsigned)((k->n + yue::kKnnThreads - 1) / yue::kKnnThreads)), dim3(yue::kKnnThreads), 0, c->stream, a);
    HIPCHK(hipGetLastError());
    HIPCHK(k->ev[1].record(c->stream));
    std::vector<double> sc((size_t)k->n);
    HIPCHK(hipMemcpyAsync(sc.data(), k->scores.p, (size_t)k->n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(yue_host::elapsed(k->ev[0], k->ev[1], &c->knn_ns));
    // the one-user list: the scored items by (score descending, item ascending)
    std::vector<int32_t> order;
    for (int64_t i = 0; i < k->n; ++i)
        if (sc[(size_t)i] >= 0.0) order.push_back((int32_t)i);
    std::stable_sort(order.begin(), order.end(), [&](int32_t x, int32_t y) { return sc[(size_t)x] > sc[(size_t)y]; });
    const int64_t len = (int64_t)order.size();
    for (int64_t r = 0; r < std::min(len, cap); ++r) {
        items_out[r] = order[(size_t)r];
        scores_out[r] = sc[(size_t)order[(size_t)r]];
    }
    *len_out = len;
    return YUE_OK;
}

}  // extern "C"
