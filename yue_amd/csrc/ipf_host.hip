// libyue_hip.so -- IPF (recommender/cf/IPF.py): session-temporal-graph ranking (include/yue_hip.h).
// Kernels: ipf_kernels.hpp.  Needs no factors: the state is the graph of yue_ipf_set_graph and per-slot work arrays.
#include "host_common.hpp"

#include "ipf_kernels.hpp"

using yue_host::fail;
using yue_host::upload;

struct yue_ipf {
    int64_t m = 0, n = 0;
    DevBuf<int64_t> u_ptr, s_ptr, hu_ptr, hs_ptr;
    DevBuf<int32_t> u_items, s_items, hu_users, hs_users, hs_pos;
    DevBuf<double> w_user, w_sess, p_i2u, p_i2s;
    double r_user = 0.0, r_sess = 0.0;
    // work arrays of `slots` workgroups; clean (key2 = key3 = 0, score = 0, ins = unreached) unless a launch failed
    int64_t slots = 0;
    bool clean = false;
    DevBuf<unsigned long long> key2, e2, key3, ins, ins_out;
    DevBuf<double> r2u, r2s, score, scores_out;
    DevBuf<int32_t> touch2, touch3, users, ids_out, len_out;
    Event ev[2];
};

namespace {

// work arrays for `slots` workgroups, cleared when new or after a failed launch
int ensure_slots(yue_ctx *c, yue_ipf *g, int64_t slots) {
    const size_t sm = (size_t)slots * (size_t)g->m, sn = (size_t)slots * (size_t)g->n;
    if (slots > g->slots) g->clean = false;
    HIPCHK(g->key2.resize(sm)); HIPCHK(g->e2.resize(sm)); HIPCHK(g->r2u.resize(sm)); HIPCHK(g->r2s.resize(sm)); HIPCHK(g->touch2.resize(sm));
    HIPCHK(g->key3.resize(sn)); HIPCHK(g->ins.resize(sn)); HIPCHK(g->score.resize(sn)); HIPCHK(g->touch3.resize(sn));
    if (!g->clean) {
        const int64_t all = std::max(slots, g->slots);
        HIPCHK(hipMemsetAsync(g->key2.p, 0, (size_t)all * g->m * sizeof(unsigned long long), c->stream));
        HIPCHK(hipMemsetAsync(g->key3.p, 0, (size_t)all * g->n * sizeof(unsigned long long), c->stream));
        HIPCHK(hipMemsetAsync(g->score.p, 0, (size_t)all * g->n * sizeof(double), c->stream));
        HIPCHK(hipMemsetAsync(g->ins.p, 0xFF, (size_t)all * g->n * sizeof(unsigned long long), c->stream));
    }
    g->slots = std::max(slots, g->slots);
    return YUE_OK;
}

yue::IpfArgs base_args(yue_ipf *g) {
    yue::IpfArgs a{};
    a.m = g->m; a.n = g->n;
    a.u_ptr = g->u_ptr.p; a.u_items = g->u_items.p; a.s_ptr = g->s_ptr.p; a.s_items = g->s_items.p;
    a.hu_ptr = g->hu_ptr.p; a.hu_users = g->hu_users.p; a.hs_ptr = g->hs_ptr.p; a.hs_users = g->hs_users.p; a.hs_pos = g->hs_pos.p;
    a.w_user = g->w_user.p; a.w_sess = g->w_sess.p; a.p_i2u = g->p_i2u.p; a.p_i2s = g->p_i2s.p;
    a.r_user = g->r_user; a.r_sess = g->r_sess;
    a.key2 = g->key2.p; a.e2 = g->e2.p; a.r2u = g->r2u.p; a.r2s = g->r2s.p; a.touch2 = g->touch2.p;
    a.key3 = g->key3.p; a.score = g->score.p; a.ins = g->ins.p; a.touch3 = g->touch3.p;
    return a;
}

// one launch of k_ipf_rank over nu users (already on the device in g->users), timed
int launch(yue_ctx *c, yue_ipf *g, int64_t nu, int N, int64_t slots) {
    int rc = ensure_slots(c, g, slots);
    if (rc) return rc;
    yue::IpfArgs a = base_args(g);
    a.users = g->users.p; a.nu = nu; a.N = N;
    a.ids_out = g->ids_out.p; a.scores_out = g->scores_out.p; a.ins_out = g->ins_out.p; a.len_out = g->len_out.p;
    g->clean = false;
    HIPCHK(g->ev[0].record(c->stream));
    hipLaunchKernelGGL(yue::k_ipf_rank, dim3((unsigned)slots), dim3(yue::kIpfThreads), 0, c->stream, a);
    HIPCHK(hipGetLastError());
    HIPCHK(g->ev[1].record(c->stream));
    return YUE_OK;
}

int finish(yue_ctx *c, yue_ipf *g) {
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(yue_host::elapsed(g->ev[0], g->ev[1], &c->ipf_ns));
    g->clean = true;
    return YUE_OK;
}

int ready(yue_ctx *c, const char *who, yue_ipf **out) {
    if (!c) return fail(YUE_ERR_ARG, std::string(who) + ": null context");
    if (!c->ipf || c->ipf->m == 0) return fail(YUE_ERR_ARG, std::string(who) + ": call yue_ipf_set_graph first");
    *out = c->ipf.get();
    return YUE_OK;
}

}  // namespace

extern "C" {

int yue_ipf_set_graph(yue_ctx *c, int64_t m, int64_t n, const int64_t *u_ptr, const int32_t *u_items, const int64_t *s_ptr,
                      const int32_t *s_items, const int64_t *hu_ptr, const int32_t *hu_users, const int64_t *hs_ptr,
                      const int32_t *hs_users, const int32_t *hs_pos, const double *w_user, const double *w_sess,
                      const double *p_i2u, const double *p_i2s, double r_user, double r_sess) {
    if (!c) return fail(YUE_ERR_ARG, "yue_ipf_set_graph: null context");
    if (m < 1 || n < 1 || m >= ((int64_t)1 << yue::kIpfPosBits) || n >= ((int64_t)1 << yue::kIpfPosBits))
        return fail(YUE_ERR_ARG, "yue_ipf_set_graph: need 1 <= m, n < 2^26");
    if (!w_user || !w_sess || !p_i2u || !p_i2s) return fail(YUE_ERR_ARG, "yue_ipf_set_graph: null weight array");
    const int64_t max_list = ((int64_t)1 << yue::kIpfKBits) - 1, max_holders = ((int64_t)1 << yue::kIpfPosBits) - 1;
    int rc = check_rows("yue_ipf_set_graph: user lists", u_ptr, m, u_items, n, yue_host::kNoTotal, Order::distinct, max_list);
    if (!rc) rc = check_rows("yue_ipf_set_graph: session lists", s_ptr, m, s_items, n, yue_host::kNoTotal, Order::distinct, max_list);
    if (!rc) rc = check_rows("yue_ipf_set_graph: item2user lists", hu_ptr, n, hu_users, m, yue_host::kNoTotal, Order::distinct, max_holders);
    if (!rc) rc = check_rows("yue_ipf_set_graph: item2session lists", hs_ptr, n, hs_users, m, yue_host::kNoTotal, Order::distinct, max_holders);
    if (rc) return rc;
    if (hs_ptr[n] > 0 && !hs_pos) return fail(YUE_ERR_ARG, "yue_ipf_set_graph: null item2session positions");
    for (int64_t e = 0; e < hs_ptr[n]; ++e)
        if (hs_pos[e] < 0 || hs_pos[e] > max_holders) return fail(YUE_ERR_ARG, "yue_ipf_set_graph: item2session position out of range (limit 2^26 - 1)");
    HIPCHK(hipSetDevice(c->device));
    yue_ipf *g = nullptr;
    if ((rc = yue_host::state(c, c->ipf, &g))) return rc;
    const bool same_shape = g->m == m && g->n == n;
    g->m = 0;                                                    // invalid until everything is up
    if ((rc = upload(g->u_ptr, u_ptr, m + 1)) || (rc = upload(g->u_items, u_items, u_ptr[m])) || (rc = upload(g->s_ptr, s_ptr, m + 1)) ||
        (rc = upload(g->s_items, s_items, s_ptr[m])) || (rc = upload(g->hu_ptr, hu_ptr, n + 1)) || (rc = upload(g->hu_users, hu_users, hu_ptr[n])) ||
        (rc = upload(g->hs_ptr, hs_ptr, n + 1)) || (rc = upload(g->hs_users, hs_users, hs_ptr[n])) || (rc = upload(g->hs_pos, hs_pos, hs_ptr[n])) ||
        (rc = upload(g->w_user, w_user, m)) || (rc = upload(g->w_sess, w_sess, m)) || (rc = upload(g->p_i2u, p_i2u, n)) ||
        (rc = upload(g->p_i2s, p_i2s, n)))
        return rc;
    if (!same_shape) {                                           // work arrays sized for another graph: drop them
        for (auto *b : {&g->key2, &g->e2, &g->key3, &g->ins}) b->release();
        for (auto *b : {&g->r2u, &g->r2s, &g->score}) b->release();
        g->touch2.release(); g->touch3.release();
        g->slots = 0;
        g->clean = false;
    }
    g->r_user = r_user; g->r_sess = r_sess;
    g->m = m; g->n = n;
    return YUE_OK;
}

int yue_ipf_topn(yue_ctx *c, const int32_t *users, int64_t nu, int N, int32_t *ids_out, double *scores_out, int32_t *len_out) {
    yue_ipf *g = nullptr;
    int rc = ready(c, "yue_ipf_topn", &g);
    if (rc) return rc;
    if (N < 1 || N > yue::kIpfMaxN) return fail(YUE_ERR_ARG, "yue_ipf_topn: N = " + std::to_string(N) + " is not supported (1 <= N <= 100)");
    if (nu < 0 || nu >= INT32_MAX || (nu > 0 && (!users || !ids_out || !scores_out || !len_out)))
        return fail(YUE_ERR_ARG, "yue_ipf_topn: need 0 <= nu < 2^31 - 1 and non-null arrays");
    if ((rc = check_ids("yue_ipf_topn: user", users, nu, g->m))) return rc;
    if (nu == 0) return YUE_OK;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(g->users.resize((size_t)nu)); HIPCHK(g->ids_out.resize((size_t)nu * N)); HIPCHK(g->scores_out.resize((size_t)nu * N));
    HIPCHK(g->len_out.resize((size_t)nu)); HIPCHK(g->ins_out.resize(1));
    HIPCHK(hipMemcpyAsync(g->users.p, users, (size_t)nu * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    // slots: at most the option ipf_slots, and at most 4 GiB of work arrays
    const int64_t per_slot = 36 * g->m + 28 * g->n;
    const int64_t slots = std::max<int64_t>(1, std::min<int64_t>({nu, (int64_t)c->opt_ipf_slots, ((int64_t)4 << 30) / per_slot}));
    if ((rc = launch(c, g, nu, N, slots))) return rc;
    HIPCHK(hipMemcpyAsync(ids_out, g->ids_out.p, (size_t)nu * N * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(scores_out, g->scores_out.p, (size_t)nu * N * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(len_out, g->len_out.p, (size_t)nu * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    return finish(c, g);
}

int yue_ipf_predict(yue_ctx *c, int32_t user, int64_t cap, int32_t *items_out, double *scores_out, int64_t *len_out) {
    yue_ipf *g = nullptr;
    int rc = ready(c, "yue_ipf_predict", &g);
    if (rc) return rc;
    if (user < 0 || user >= g->m) return fail(YUE_ERR_ARG, "yue_ipf_predict: user id out of range");
    if (cap < 0 || (cap > 0 && (!items_out || !scores_out)) || !len_out) return fail(YUE_ERR_ARG, "yue_ipf_predict: need cap >= 0 and non-null arrays");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(g->users.resize(1)); HIPCHK(g->ids_out.resize((size_t)g->n)); HIPCHK(g->scores_out.resize((size_t)g->n));
    HIPCHK(g->ins_out.resize((size_t)g->n)); HIPCHK(g->len_out.resize(1));
    HIPCHK(hipMemcpyAsync(g->users.p, &user, sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    if ((rc = launch(c, g, 1, 0, 1))) return rc;
    int32_t len = 0;
    HIPCHK(hipMemcpyAsync(&len, g->len_out.p, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    std::vector<int32_t> it((size_t)len);
    std::vector<double> sc((size_t)len);
    std::vector<unsigned long long> ins((size_t)len);
    if (len > 0) {
        HIPCHK(hipMemcpyAsync(it.data(), g->ids_out.p, (size_t)len * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(sc.data(), g->scores_out.p, (size_t)len * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipMemcpyAsync(ins.data(), g->ins_out.p, (size_t)len * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
    }
    if ((rc = finish(c, g))) return rc;
    // the one-user list: the reached items by (score descending, first insertion ascending)
    std::vector<int32_t> order((size_t)len);
    for (int32_t r = 0; r < len; ++r) order[(size_t)r] = r;
    std::sort(order.begin(), order.end(), [&](int32_t x, int32_t y) {
        return sc[(size_t)x] > sc[(size_t)y] || (sc[(size_t)x] == sc[(size_t)y] && ins[(size_t)x] < ins[(size_t)y]);
    });
    for (int64_t r = 0; r < std::min<int64_t>(len, cap); ++r) {
        items_out[r] = it[(size_t)order[(size_t)r]];
        scores_out[r] = sc[(size_t)order[(size_t)r]];
    }
    *len_out = len;
    return YUE_OK;
}

}  // extern "C"
