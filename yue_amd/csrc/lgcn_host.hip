// libyue_hip.so -- LightGCN (reference recommender/advanced/LightGCN.py): the user-item graph, the propagation forward and
// backward, the minibatch and the Adam step (include/yue_hip.h).  Kernels: lgcn_kernels.hpp; Adam is
// k_adam on the moments of yue_adam_step (yue_host::adam_apply, bpr_host.hip).  U and V are the context's P and Q.
#include "host_common.hpp"

#include "lgcn_kernels.hpp"

#include <utility>

using yue_host::fail;
using yue_host::with_kr;

struct yue_lgcn {
    int64_t m = 0, n = 0, nnz = 0;                   // the graph's shape: N = m + n rows, nnz entries (both directions)
    bool have_graph = false;
    std::vector<int64_t> h_ptr;
    DevBuf<int64_t> ptr;
    DevBuf<int32_t> col;
    DevBuf<float> w;
    int rpw = 1;                                     // rows per wave of k_lgcn_rows
    // hub rows, rebuilt when the option lgcn_hub differs from hub_built
    int64_t hub_built = -1, H = 0, parts = 0;
    DevBuf<int64_t> hub_row, hub_part_ptr, part_beg, part_end;
    DevBuf<float> partial;
    // work: raw layers E_0 .. E_L, their sums of squares, F, dLoss / dF, two gE buffers, the minibatch
    DevBuf<float> E, ss, F, G, gA, gB, coef;
    DevBuf<double> loss;
    DevBuf<int64_t> seg_ptr, seg_row;
    DevBuf<int32_t> ent;
    std::vector<double> h_loss;
    // the minibatch's sorted entries on the host: kept between steps, so that a step allocates nothing once the batch size is seen
    std::vector<std::pair<int64_t, int32_t>> h_ents;
    std::vector<int64_t> h_seg_ptr, h_seg_row;
    std::vector<int32_t> h_ent;
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
};

namespace {

int lgcn_new(yue_ctx *c) {
    if (c->lgcn) return YUE_OK;
    HIPCHK(hipSetDevice(c->device));
    yue_lgcn *s = new yue_lgcn();
    c->lgcn = s;
    for (auto &e : s->ev) HIPCHK(hipEventCreate(&e));
    return YUE_OK;
}

template <typename T>
int upload(DevBuf<T> &buf, const T *src, int64_t count) {
    HIPCHK(buf.resize((size_t)std::max<int64_t>(count, 1)));
    if (count > 0) HIPCHK(hipMemcpy(buf.p, src, (size_t)count * sizeof(T), hipMemcpyHostToDevice));
    return YUE_OK;
}

// one side's lists: ptr[0] = 0, ascending ptr, ids strictly ascending within a row and below `other`, finite weights
int check_side(const char *side, int64_t rows, int64_t other, const int64_t *ptr, const int32_t *ids, const float *w) {
    const std::string who = std::string("yue_lgcn_set_graph: ") + side;
    if (ptr[0] != 0) return fail(YUE_ERR_ARG, who + " ptr[0] must be 0");
    for (int64_t r = 0; r < rows; ++r) {
        if (ptr[r + 1] < ptr[r]) return fail(YUE_ERR_ARG, who + " ptr must ascend (row " + std::to_string(r) + ")");
        for (int64_t p = ptr[r]; p < ptr[r + 1]; ++p) {
            if (ids[p] < 0 || ids[p] >= other) return fail(YUE_ERR_ARG, who + " row " + std::to_string(r) + ": id out of range");
            if (p > ptr[r] && ids[p] <= ids[p - 1]) return fail(YUE_ERR_ARG, who + " row " + std::to_string(r) + ": ids must be sorted and unique");
            if (!std::isfinite(w[p])) return fail(YUE_ERR_ARG, who + " row " + std::to_string(r) + ": weight not finite");
        }
    }
    return YUE_OK;
}

int build_hubs(yue_ctx *c, yue_lgcn *s) {
    const int64_t thr = c->opt_lgcn_hub, N = s->m + s->n;
    if (s->hub_built == thr) return YUE_OK;
    std::vector<int64_t> hub_row, hub_part_ptr{0}, part_beg, part_end;
    int64_t light = 0;                                       // entries of the rows k_lgcn_rows keeps
    for (int64_t r = 0; r < N; ++r) {
        const int64_t b = s->h_ptr[(size_t)r], e = s->h_ptr[(size_t)r + 1];
        if (e - b <= thr) { light += e - b; continue; }
        for (int64_t p = b; p < e; p += thr) {               // parts of `thr` neighbours, the last one short
            part_beg.push_back(p); part_end.push_back(std::min(p + thr, e));
        }
        hub_row.push_back(r);
        hub_part_ptr.push_back((int64_t)part_beg.size());
    }
    s->H = (int64_t)hub_row.size(); s->parts = (int64_t)part_beg.size();
    if (s->parts >= INT32_MAX) return fail(YUE_ERR_ARG, "yue_lgcn: lgcn_hub cuts the hub rows into 2^31 parts or more");
    int rc;
    if ((rc = upload(s->hub_row, hub_row.data(), s->H)) || (rc = upload(s->hub_part_ptr, hub_part_ptr.data(), s->H + 1)) ||
        (rc = upload(s->part_beg, part_beg.data(), s->parts)) || (rc = upload(s->part_end, part_end.data(), s->parts)))
        return rc;
    // many short rows go to one wave: about 64 neighbours' worth, 16 rows at the most
    const int64_t mean = std::max<int64_t>(1, light / std::max<int64_t>(1, N - s->H));
    s->rpw = (int)std::min<int64_t>(16, std::max<int64_t>(1, 64 / mean));
    s->hub_built = thr;
    c->lgcn_hubs = s->H; c->lgcn_parts = s->parts;
    return YUE_OK;
}

int lgcn_ready(yue_ctx *c, yue_lgcn **out, int layers, const char *who) {
    if (!c) return fail(YUE_ERR_ARG, std::string(who) + ": null context");
    if (!c->have_factors) return fail(YUE_ERR_ARG, std::string(who) + ": call yue_set_factors first (U, V)");
    if (c->k > yue::kLgcnMaxK) return fail(YUE_ERR_ARG, std::string(who) + ": needs k <= 128");
    if (layers < 1 || layers > 64) return fail(YUE_ERR_ARG, std::string(who) + ": needs 1 <= layers <= 64");
    yue_lgcn *s = c->lgcn;
    if (!s || !s->have_graph) return fail(YUE_ERR_ARG, std::string(who) + ": call yue_lgcn_set_graph first");
    if (s->m != c->m || s->n != c->n)
        return fail(YUE_ERR_ARG, std::string(who) + ": the graph was set for " + std::to_string(s->m) + " users and " + std::to_string(s->n) +
                                     " items, the factors hold " + std::to_string(c->m) + " and " + std::to_string(c->n));
    HIPCHK(hipSetDevice(c->device));
    const int rc = build_hubs(c, s);
    if (rc) return rc;
    *out = s;
    return YUE_OK;
}

yue::LgcnArgs graph_args(const yue_ctx *c, const yue_lgcn *s) {
    yue::LgcnArgs a{};
    a.ptr = s->ptr.p; a.col = s->col.p; a.w = s->w.p; a.N = s->m + s->n; a.m = s->m; a.k = c->k; a.rpw = s->rpw; a.gather = 1;
    a.hub = s->hub_built;
    a.hub_row = s->hub_row.p; a.hub_part_ptr = s->hub_part_ptr.p; a.part_beg = s->part_beg.p; a.part_end = s->part_end.p;
    a.partial = s->partial.p; a.H = s->H; a.parts = s->parts;
    return a;
}

// one product with its epilogue: the light rows, then the hub rows' parts and their combination
template <int MODE>
int launch_product(yue_ctx *c, const yue_lgcn *s, const yue::LgcnArgs &a) {
    const int64_t waves = (a.N + a.rpw - 1) / a.rpw;
    with_kr(c->k, [&](auto kr) {
        constexpr int KR = kr() > 2 ? 2 : kr();
        hipLaunchKernelGGL((yue::k_lgcn_rows<KR, MODE>), dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, c->stream, a);
        if (a.gather && s->H > 0) {
            hipLaunchKernelGGL((yue::k_lgcn_hub_parts<KR>), dim3((unsigned)((s->parts + 3) / 4)), dim3(256), 0, c->stream, a);
            hipLaunchKernelGGL((yue::k_lgcn_hub_combine<KR, MODE>), dim3((unsigned)((s->H + 3) / 4)), dim3(256), 0, c->stream, a);
        }
    });
    HIPCHK(hipGetLastError());
    return YUE_OK;
}

// E_0 = [U; V], E_l = A E_{l-1}, F = E_0 + sum_l normalised E_l; all kept for the backward pass
int forward(yue_ctx *c, yue_lgcn *s, int L) {
    const int64_t N = s->m + s->n, k = c->k, mk = s->m * k, nk = s->n * k;
    HIPCHK(s->E.resize((size_t)((L + 1) * N * k))); HIPCHK(s->ss.resize((size_t)(L * N))); HIPCHK(s->F.resize((size_t)(N * k)));
    HIPCHK(s->partial.resize((size_t)std::max<int64_t>(1, s->parts * k)));
    HIPCHK(hipMemcpyAsync(s->E.p, c->P.p, (size_t)mk * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(s->E.p + mk, c->Q.p, (size_t)nk * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(s->F.p, s->E.p, (size_t)(N * k) * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    for (int l = 1; l <= L; ++l) {
        yue::LgcnArgs a = graph_args(c, s);
        a.X = s->E.p + (int64_t)(l - 1) * N * k; a.Y = s->E.p + (int64_t)l * N * k; a.ss = s->ss.p + (int64_t)(l - 1) * N; a.F = s->F.p;
        const int rc = launch_product<yue::kLgcnFwd>(c, s, a);
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
        if ((rc = launch_product<yue::kLgcnBwd>(c, s, a))) return rc;
        if (l < L) std::swap(cur, other);
    }
    yue::LgcnArgs a = graph_args(c, s);
    a.X = cur; a.G = s->G.p; a.gU = c->dP.p; a.gV = c->dQ.p;
    return launch_product<yue::kLgcnFin>(c, s, a);
}

int check_batch(yue_ctx *c, const int32_t *u, const int32_t *i, const int32_t *j, int64_t T, const char *who) {
    if (T < 1 || T >= (1ll << 29) || !u || !i || !j) return fail(YUE_ERR_ARG, std::string(who) + ": needs 1 <= T < 2^29 and the three id arrays");
    for (int64_t t = 0; t < T; ++t)
        if (u[t] < 0 || u[t] >= c->m || i[t] < 0 || i[t] >= c->n || j[t] < 0 || j[t] >= c->n) return fail(YUE_ERR_ARG, std::string(who) + ": triplet " + std::to_string(t) + " out of range");
    return YUE_OK;
}

// forward, minibatch, backward: the loss in *loss_out, the gradients in dP / dQ.  Events 0..3 bracket the three phases.
int gradient(yue_ctx *c, yue_lgcn *s, int L, const int32_t *u, const int32_t *i, const int32_t *j, int64_t T, double reg, double *loss_out) {
    const int64_t N = s->m + s->n, k = c->k;
    int rc = yue_host::upload_triplets(c, u, i, j, T, true);
    if (rc) return rc;
    // the 3 T (row of F, triplet, role) entries by row, a row's entries in triplet order: the order k_lgcn_batch_g adds in
    std::vector<std::pair<int64_t, int32_t>> &ents = s->h_ents;
    std::vector<int64_t> &seg_ptr = s->h_seg_ptr, &seg_row = s->h_seg_row;
    std::vector<int32_t> &ent = s->h_ent;
    ents.resize((size_t)(3 * T)); ent.resize((size_t)(3 * T)); seg_ptr.clear(); seg_row.clear();
    for (int64_t t = 0; t < T; ++t) {
        ents[(size_t)(3 * t)] = {u[t], (int32_t)(4 * t)};
        ents[(size_t)(3 * t + 1)] = {s->m + i[t], (int32_t)(4 * t + 1)};
        ents[(size_t)(3 * t + 2)] = {s->m + j[t], (int32_t)(4 * t + 2)};
    }
    std::sort(ents.begin(), ents.end());
    for (int64_t p = 0; p < 3 * T; ++p) {
        if (p == 0 || ents[(size_t)p].first != ents[(size_t)p - 1].first) { seg_ptr.push_back(p); seg_row.push_back(ents[(size_t)p].first); }
        ent[(size_t)p] = ents[(size_t)p].second;
    }
    const int64_t S = (int64_t)seg_row.size();
    seg_ptr.push_back(3 * T);
    HIPCHK(hipStreamSynchronize(c->stream));             // (the blocking uploads below overwrite what an earlier call's kernels read)
    if ((rc = upload(s->seg_ptr, seg_ptr.data(), S + 1)) || (rc = upload(s->seg_row, seg_row.data(), S)) || (rc = upload(s->ent, ent.data(), 3 * T))) return rc;
    HIPCHK(s->coef.resize((size_t)T)); HIPCHK(s->loss.resize((size_t)T)); HIPCHK(s->G.resize((size_t)(N * k)));

    HIPCHK(hipEventRecord(s->ev[0], c->stream));
    if ((rc = forward(c, s, L))) return rc;
    HIPCHK(hipEventRecord(s->ev[1], c->stream));
    HIPCHK(hipMemsetAsync(s->G.p, 0, (size_t)(N * k) * sizeof(float), c->stream));
    yue::LgcnBatchArgs b{};
    b.F = s->F.p; b.G = s->G.p; b.m = s->m; b.k = c->k; b.u = c->xu.p; b.i = c->xi.p; b.j = c->xj.p; b.T = T; b.S = S; b.reg = (float)reg;
    b.c = s->coef.p; b.loss = s->loss.p; b.seg_ptr = s->seg_ptr.p; b.seg_row = s->seg_row.p; b.ent = s->ent.p;
    with_kr(c->k, [&](auto kr) {
        constexpr int KR = kr() > 2 ? 2 : kr();
        hipLaunchKernelGGL((yue::k_lgcn_batch_y<KR>), dim3((unsigned)((T + 3) / 4)), dim3(256), 0, c->stream, b);
        hipLaunchKernelGGL((yue::k_lgcn_batch_g<KR>), dim3((unsigned)((S + 3) / 4)), dim3(256), 0, c->stream, b);
    });
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(s->ev[2], c->stream));
    if ((rc = backward(c, s, L))) return rc;
    HIPCHK(hipEventRecord(s->ev[3], c->stream));
    s->h_loss.resize((size_t)T);
    HIPCHK(hipMemcpyAsync(s->h_loss.data(), s->loss.p, (size_t)T * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    double loss = 0.0;
    for (int64_t t = 0; t < T; ++t) loss += s->h_loss[(size_t)t];      // triplet order
    if (loss_out) *loss_out = loss;
    return YUE_OK;
}

int read_times(yue_ctx *c, yue_lgcn *s, int last) {
    for (int p = 0; p < 4; ++p) c->lgcn_ns[p] = 0;
    for (int p = 0; p < last; ++p) {
        float ms = 0.0f;
        HIPCHK(hipEventElapsedTime(&ms, s->ev[p], s->ev[p + 1]));
        c->lgcn_ns[p] = (int64_t)(1e6 * (double)ms);
    }
    return YUE_OK;
}

}  // namespace

namespace yue_host {

void lgcn_release(yue_ctx *c) {
    yue_lgcn *s = c->lgcn;
    if (!s) return;
    s->ptr.release(); s->col.release(); s->w.release();
    s->hub_row.release(); s->hub_part_ptr.release(); s->part_beg.release(); s->part_end.release(); s->partial.release();
    s->E.release(); s->ss.release(); s->F.release(); s->G.release(); s->gA.release(); s->gB.release(); s->coef.release();
    s->loss.release(); s->seg_ptr.release(); s->seg_row.release(); s->ent.release();
    for (auto &e : s->ev) if (e) (void)hipEventDestroy(e);
    delete s;
    c->lgcn = nullptr;
}

}  // namespace yue_host

extern "C" {

int yue_lgcn_set_graph(yue_ctx *c, int64_t m, int64_t n, const int64_t *u_ptr, const int32_t *u_items, const float *u_w, const int64_t *i_ptr,
                       const int32_t *i_users, const float *i_w) {
    if (!c || !u_ptr || !i_ptr) return fail(YUE_ERR_ARG, "yue_lgcn_set_graph: null argument");
    if (m <= 0 || n <= 0 || m + n >= (1ll << 31)) return fail(YUE_ERR_ARG, "yue_lgcn_set_graph: need m, n > 0 and m + n < 2^31");
    const int64_t half = u_ptr[0] == 0 ? u_ptr[m] : -1;
    if (half > 0 && (!u_items || !u_w || !i_users || !i_w)) return fail(YUE_ERR_ARG, "yue_lgcn_set_graph: null argument");
    int rc;
    if ((rc = check_side("user", m, n, u_ptr, u_items, u_w)) || (rc = check_side("item", n, m, i_ptr, i_users, i_w))) return rc;
    // symmetry: the user lists transposed (users ascend within an item, as the item lists must) equal the item lists
    if (i_ptr[n] != half) return fail(YUE_ERR_ARG, "yue_lgcn_set_graph: the graph is not symmetric (the two sides hold different numbers of pairs)");
    std::vector<int64_t> at((size_t)n + 1, 0);
    for (int64_t p = 0; p < half; ++p) at[(size_t)u_items[p] + 1]++;
    for (int64_t r = 0; r < n; ++r) at[(size_t)r + 1] += at[(size_t)r];
    for (int64_t r = 0; r <= n; ++r)
        if (at[(size_t)r] != i_ptr[r]) return fail(YUE_ERR_ARG, "yue_lgcn_set_graph: the graph is not symmetric (item " + std::to_string(std::max<int64_t>(r - 1, 0)) + ")");
    for (int64_t u = 0; u < m; ++u)
        for (int64_t p = u_ptr[u]; p < u_ptr[u + 1]; ++p) {
            const int64_t q = at[(size_t)u_items[p]]++;
            if (i_users[q] != u || i_w[q] != u_w[p])
                return fail(YUE_ERR_ARG, "yue_lgcn_set_graph: the graph is not symmetric (user " + std::to_string(u) + ", item " + std::to_string(u_items[p]) + ")");
        }
    if ((rc = lgcn_new(c))) return rc;
    yue_lgcn *s = c->lgcn;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    s->have_graph = false;
    const int64_t N = m + n, nnz = 2 * half;
    s->h_ptr.assign((size_t)N + 1, 0);
    std::vector<int32_t> col((size_t)nnz);
    std::vector<float> w((size_t)nnz);
    for (int64_t u = 0; u < m; ++u) s->h_ptr[(size_t)u + 1] = u_ptr[u + 1];
    for (int64_t r = 0; r < n; ++r) s->h_ptr[(size_t)(m + r) + 1] = half + i_ptr[r + 1];
    for (int64_t p = 0; p < half; ++p) { col[(size_t)p] = (int32_t)(m + u_items[p]); w[(size_t)p] = u_w[p]; }
    for (int64_t p = 0; p < half; ++p) { col[(size_t)(half + p)] = i_users[p]; w[(size_t)(half + p)] = i_w[p]; }
    if ((rc = upload(s->ptr, s->h_ptr.data(), N + 1)) || (rc = upload(s->col, col.data(), nnz)) || (rc = upload(s->w, w.data(), nnz))) return rc;
    s->m = m; s->n = n; s->nnz = nnz; s->hub_built = -1;
    s->have_graph = true;
    return YUE_OK;
}

int yue_lgcn_propagate(yue_ctx *c, int layers, float *raw_layers_out, float *F_out) {
    yue_lgcn *s = nullptr;
    int rc = lgcn_ready(c, &s, layers, "yue_lgcn_propagate");
    if (rc) return rc;
    const int64_t N = s->m + s->n, k = c->k;
    HIPCHK(hipEventRecord(s->ev[0], c->stream));
    if ((rc = forward(c, s, layers))) return rc;
    HIPCHK(hipEventRecord(s->ev[1], c->stream));
    if (raw_layers_out) HIPCHK(hipMemcpyAsync(raw_layers_out, s->E.p + N * k, (size_t)(layers * N * k) * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (F_out) HIPCHK(hipMemcpyAsync(F_out, s->F.p, (size_t)(N * k) * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return read_times(c, s, 1);
}

int yue_lgcn_grad(yue_ctx *c, int layers, const int32_t *u, const int32_t *i, const int32_t *j, int64_t T, double reg, double *loss_out, float *gU_out,
                  float *gV_out) {
    yue_lgcn *s = nullptr;
    int rc = lgcn_ready(c, &s, layers, "yue_lgcn_grad");
    if (rc) return rc;
    if ((rc = check_batch(c, u, i, j, T, "yue_lgcn_grad"))) return rc;
    if ((rc = gradient(c, s, layers, u, i, j, T, reg, loss_out))) return rc;
    const size_t mk = (size_t)(c->m * c->k), nk = (size_t)(c->n * c->k);
    if (gU_out) HIPCHK(hipMemcpy(gU_out, c->dP.p, mk * sizeof(float), hipMemcpyDeviceToHost));
    if (gV_out) HIPCHK(hipMemcpy(gV_out, c->dQ.p, nk * sizeof(float), hipMemcpyDeviceToHost));
    // dP / dQ are the cleared gradient buffers of yue_adam_step: hand them back as that call expects them
    HIPCHK(hipMemsetAsync(c->dP.p, 0, mk * sizeof(float), c->stream)); HIPCHK(hipMemsetAsync(c->dQ.p, 0, nk * sizeof(float), c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return read_times(c, s, 3);
}

int yue_lgcn_step(yue_ctx *c, int layers, const int32_t *u, const int32_t *i, const int32_t *j, int64_t T, double lr, double reg, int64_t step,
                  double *loss_out) {
    yue_lgcn *s = nullptr;
    int rc = lgcn_ready(c, &s, layers, "yue_lgcn_step");
    if (rc) return rc;
    if ((rc = check_batch(c, u, i, j, T, "yue_lgcn_step"))) return rc;
    if (step < 1) return fail(YUE_ERR_ARG, "yue_lgcn_step: needs step >= 1");
    if (c->adam_m != c->m || c->adam_n != c->n || c->adam_k != c->k) { if ((rc = yue_adam_reset(c))) return rc; }
    if ((rc = gradient(c, s, layers, u, i, j, T, reg, loss_out))) return rc;
    if ((rc = yue_host::adam_apply(c, lr, step))) return rc;
    HIPCHK(hipEventRecord(s->ev[4], c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return read_times(c, s, 4);
}

}  // extern "C"
