// libyue_hip.so -- LightGCN (reference recommender/advanced/LightGCN.py): the user-item graph, the propagation forward and
// backward, the minibatch and the Adam step (include/yue_hip.h).  Kernels: lgcn_kernels.hpp; the graph on
// the device, a product's launches, the minibatch and the phase timer are gcn_host.hpp's, shared with ngcf_host.hip; Adam is
// k_adam on the moments of yue_adam_step (yue_host::adam_apply, bpr_host.hip).  U and V are the context's P and Q.
#include "gcn_host.hpp"

using gcn::launch_product;
using gcn::stamp;
using yue_host::upload;
using yue_host::fail;

struct yue_lgcn {
    int64_t m = 0, n = 0, nnz = 0;                   // the graph's shape: N = m + n rows, nnz entries (both directions)
    bool have_graph = false;
    gcn::Graph A;                                    // symmetric; its hub rows follow the option lgcn_hub
    DevBuf<float> partial;                           // hub parts of the running product
    // work: raw layers E_0 .. E_L, their sums of squares, F, dLoss / dF, two gE buffers
    DevBuf<float> E, ss, F, G, gA, gB;
    gcn::Batch batch;
    gcn::PhaseTimer timer;
};

namespace {

enum { kForward = 0, kBatch = 1, kBackward = 2, kAdam = 3, kPhases = 4 };

int lgcn_ready(yue_ctx *c, yue_lgcn **out, int layers, const char *who) {
    if (!c) return fail(YUE_ERR_ARG, std::string(who) + ": null context");
    if (!c->have_factors) return fail(YUE_ERR_ARG, std::string(who) + ": call yue_set_factors first (U, V)");
    if (c->k > yue::kLgcnMaxK) return fail(YUE_ERR_ARG, std::string(who) + ": needs k <= 128");
    if (layers < 1 || layers > 64) return fail(YUE_ERR_ARG, std::string(who) + ": needs 1 <= layers <= 64");
    yue_lgcn *s = c->lgcn.get();
    if (!s || !s->have_graph) return fail(YUE_ERR_ARG, std::string(who) + ": call yue_lgcn_set_graph first");
    if (s->m != c->m || s->n != c->n)
        return fail(YUE_ERR_ARG, std::string(who) + ": the graph was set for " + std::to_string(s->m) + " users and " + std::to_string(s->n) +
                                     " items, the factors hold " + std::to_string(c->m) + " and " + std::to_string(c->n));
    HIPCHK(hipSetDevice(c->device));
    const int rc = gcn::build_hubs(s->A, s->m + s->n, c->opt_lgcn_hub, "yue_lgcn: lgcn_hub");
    if (rc) return rc;
    c->lgcn_hubs = s->A.H; c->lgcn_parts = s->A.parts;
    s->timer.stamps = 0;
    *out = s;
    return YUE_OK;
}

yue::LgcnArgs graph_args(const yue_ctx *c, const yue_lgcn *s) { return gcn::graph_args(s->A, s->m + s->n, s->m, c->k, s->partial.p); }

// E_0 = [U; V], E_l = A E_{l-1}, F = E_0 + sum_l normalised E_l; all kept for the backward pass
int forward(yue_ctx *c, yue_lgcn *s, int L) {
    const int64_t N = s->m + s->n, k = c->k, mk = s->m * k, nk = s->n * k;
    HIPCHK(s->E.resize((size_t)((L + 1) * N * k))); HIPCHK(s->ss.resize((size_t)(L * N))); HIPCHK(s->F.resize((size_t)(N * k)));
    HIPCHK(s->partial.resize((size_t)std::max<int64_t>(1, s->A.parts * k)));
    HIPCHK(hipMemcpyAsync(s->E.p, c->P.p, (size_t)mk * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(s->E.p + mk, c->Q.p, (size_t)nk * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(s->F.p, s->E.p, (size_t)(N * k) * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    for (int l = 1; l <= L; ++l) {
        yue::LgcnArgs a = graph_args(c, s);
        a.X = s->E.p + (int64_t)(l - 1) * N * k; a.Y = s->E.p + (int64_t)l * N * k; a.ss = s->ss.p + (int64_t)(l - 1) * N; a.F = s->F.p;
        const int rc = launch_product<yue::kLgcnFwd>(c, s->A, a);
        if (rc) return rc;
    }
    return YUE_OK;
}

// gE_L = J_L(G); gE_l = J_l(G) + A gE_{l+1}; g[U;V] = G + A gE_1 into dP, dQ
int backward(yue_ctx *c, yue_lgcn *s, int L) {
    const int64_t N = s->m + s->n, k = c->k;
    HIPCHK(s->gA.resize((size_t)(N * k))); HIPCHK(s->gB.resize((size_t)(N * k)));
    float *cur = s->gA.p, *other = s->gB.p;
    int rc;
    for (int l = L; l >= 1; --l) {
        yue::LgcnArgs a = graph_args(c, s);
        a.gather = l < L; a.X = l < L ? cur : nullptr; a.out = l < L ? other : cur;
        a.G = s->G.p; a.E = s->E.p + (int64_t)l * N * k; a.ssr = s->ss.p + (int64_t)(l - 1) * N;
        if ((rc = launch_product<yue::kLgcnBwd>(c, s->A, a))) return rc;
        if (l < L) std::swap(cur, other);
    }
    yue::LgcnArgs a = graph_args(c, s);
    a.X = cur; a.base = s->G.p; a.outU = c->dP.p; a.outV = c->dQ.p;
    return launch_product<yue::kLgcnPlain>(c, s->A, a);
}

// forward, minibatch, backward: the loss in *loss_out, the gradients in dP / dQ.  A stamp closes each of the three phases.
int gradient(yue_ctx *c, yue_lgcn *s, int L, const int32_t *u, const int32_t *i, const int32_t *j, int64_t T, double reg, double *loss_out) {
    const int64_t N = s->m + s->n, k = c->k;
    int rc;
    if ((rc = gcn::batch_prepare(c, s->batch, s->m, u, i, j, T))) return rc;
    HIPCHK(s->G.resize((size_t)(N * k)));
    if ((rc = stamp(c, s->timer, kForward)) || (rc = forward(c, s, L)) || (rc = stamp(c, s->timer, kForward))) return rc;
    HIPCHK(hipMemsetAsync(s->G.p, 0, (size_t)(N * k) * sizeof(float), c->stream));
    if ((rc = gcn::batch_launch(c, s->batch, s->F.p, s->G.p, s->m, c->k, T, reg)) || (rc = stamp(c, s->timer, kBatch))) return rc;
    if ((rc = backward(c, s, L)) || (rc = stamp(c, s->timer, kBackward))) return rc;
    return gcn::batch_loss(c, s->batch, T, loss_out);
}

}  // namespace

extern "C" {

int yue_lgcn_set_graph(yue_ctx *c, int64_t m, int64_t n, const int64_t *u_ptr, const int32_t *u_items, const float *u_w, const int64_t *i_ptr,
                       const int32_t *i_users, const float *i_w) {
    if (!c || !u_ptr || !i_ptr) return fail(YUE_ERR_ARG, "yue_lgcn_set_graph: null argument");
    if (m <= 0 || n <= 0 || m + n >= (1ll << 31)) return fail(YUE_ERR_ARG, "yue_lgcn_set_graph: need m, n > 0 and m + n < 2^31");
    const int64_t half = u_ptr[m];
    if (half > 0 && (!u_items || !u_w || !i_users || !i_w)) return fail(YUE_ERR_ARG, "yue_lgcn_set_graph: null argument");
    const auto finite = [](const float *w) { return [w](int64_t, int64_t p) { return std::isfinite(w[p]) ? nullptr : "weight not finite"; }; };
    int rc = check_rows("yue_lgcn_set_graph: user-side", u_ptr, m, u_items, n, yue_host::kNoTotal, Order::ascending, yue_host::kNoLimit, finite(u_w));
    if (rc) return rc;
    // symmetry: the user lists transposed (users ascend within an item, as the item lists must) equal the item lists
    if (i_ptr[n] != half) return fail(YUE_ERR_ARG, "yue_lgcn_set_graph: the graph is not symmetric (the two sides hold different numbers of pairs)");
    if ((rc = check_rows("yue_lgcn_set_graph: item-side", i_ptr, n, i_users, m, yue_host::kNoTotal, Order::ascending, yue_host::kNoLimit, finite(i_w))) ||
        (rc = check_transpose("yue_lgcn_set_graph: the graph is not symmetric", m, u_ptr, u_items, n, i_ptr, i_users, [&](int64_t p, int64_t q) { return i_w[q] == u_w[p]; })))
        return rc;
    yue_lgcn *s = nullptr;
    if ((rc = yue_host::state(c, c->lgcn, &s))) return rc;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    s->have_graph = false;
    const int64_t N = m + n, nnz = 2 * half;
    s->A.h_ptr.assign((size_t)N + 1, 0);
    std::vector<int32_t> col((size_t)nnz);
    std::vector<float> w((size_t)nnz);
    for (int64_t u = 0; u < m; ++u) s->A.h_ptr[(size_t)u + 1] = u_ptr[u + 1];
    for (int64_t r = 0; r < n; ++r) s->A.h_ptr[(size_t)(m + r) + 1] = half + i_ptr[r + 1];
    for (int64_t p = 0; p < half; ++p) { col[(size_t)p] = (int32_t)(m + u_items[p]); w[(size_t)p] = u_w[p]; }
    for (int64_t p = 0; p < half; ++p) { col[(size_t)(half + p)] = i_users[p]; w[(size_t)(half + p)] = i_w[p]; }
    if ((rc = upload(s->A.ptr, s->A.h_ptr.data(), N + 1)) || (rc = upload(s->A.col, col.data(), nnz)) || (rc = upload(s->A.w, w.data(), nnz))) return rc;
    s->m = m; s->n = n; s->nnz = nnz; s->A.hub_built = -1;
    s->have_graph = true;
    return YUE_OK;
}

int yue_lgcn_propagate(yue_ctx *c, int layers, float *raw_layers_out, float *F_out) {
    yue_lgcn *s = nullptr;
    int rc = lgcn_ready(c, &s, layers, "yue_lgcn_propagate");
    if (rc) return rc;
    const int64_t N = s->m + s->n, k = c->k;
    if ((rc = stamp(c, s->timer, kForward)) || (rc = forward(c, s, layers)) || (rc = stamp(c, s->timer, kForward))) return rc;
    if (raw_layers_out) HIPCHK(hipMemcpyAsync(raw_layers_out, s->E.p + N * k, (size_t)(layers * N * k) * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (F_out) HIPCHK(hipMemcpyAsync(F_out, s->F.p, (size_t)(N * k) * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return gcn::read_times(s->timer, c->lgcn_ns, kPhases);
}

int yue_lgcn_grad(yue_ctx *c, int layers, const int32_t *u, const int32_t *i, const int32_t *j, int64_t T, double reg, double *loss_out, float *gU_out,
                  float *gV_out) {
    yue_lgcn *s = nullptr;
    int rc = lgcn_ready(c, &s, layers, "yue_lgcn_grad");
    if (rc) return rc;
    if ((rc = gcn::check_batch(c, u, i, j, T, "yue_lgcn_grad"))) return rc;
    if ((rc = gradient(c, s, layers, u, i, j, T, reg, loss_out))) return rc;
    const size_t mk = (size_t)(c->m * c->k), nk = (size_t)(c->n * c->k);
    if (gU_out) HIPCHK(hipMemcpy(gU_out, c->dP.p, mk * sizeof(float), hipMemcpyDeviceToHost));
    if (gV_out) HIPCHK(hipMemcpy(gV_out, c->dQ.p, nk * sizeof(float), hipMemcpyDeviceToHost));
    // dP / dQ are the cleared gradient buffers of yue_adam_step: hand them back as that call expects them
    HIPCHK(hipMemsetAsync(c->dP.p, 0, mk * sizeof(float), c->stream)); HIPCHK(hipMemsetAsync(c->dQ.p, 0, nk * sizeof(float), c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return gcn::read_times(s->timer, c->lgcn_ns, kPhases);
}

int yue_lgcn_step(yue_ctx *c, int layers, const int32_t *u, const int32_t *i, const int32_t *j, int64_t T, double lr, double reg, int64_t step,
                  double *loss_out) {
    yue_lgcn *s = nullptr;
    int rc = lgcn_ready(c, &s, layers, "yue_lgcn_step");
    if (rc) return rc;
    if ((rc = gcn::check_batch(c, u, i, j, T, "yue_lgcn_step"))) return rc;
    if (step < 1) return fail(YUE_ERR_ARG, "yue_lgcn_step: needs step >= 1");
    if (c->adam_m != c->m || c->adam_n != c->n || c->adam_k != c->k) { if ((rc = yue_adam_reset(c))) return rc; }
    if ((rc = gradient(c, s, layers, u, i, j, T, reg, loss_out))) return rc;
    if ((rc = yue_host::adam_apply(c, lr, step))) return rc;
    if ((rc = stamp(c, s->timer, kAdam))) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    return gcn::read_times(s->timer, c->lgcn_ns, kPhases);
}

}  // extern "C"
