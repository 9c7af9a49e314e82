// libyue_hip.so -- APR (reference recommender/advanced/APR.py): BPR's live minibatch path with an adversarial perturbation of
// the embeddings (include/yue_apr.h).  Kernels: apr_kernels.hpp.  U and V are the context's P and Q, Adam
// is k_adam on the moments of yue_adam_step (yue_host::adam_apply, bpr_host.hip), the phase timer is gcn_host.hpp's.  The host
// side checks a batch, builds its distinct users and items (ascending) and every distinct row's (triplet, role) list by a
// stable counting sort, ships all index arrays of the step in one upload and adds the loss terms in triplet order.
// The perturbation is kept compact: the ids of the last batch's distinct rows on the host, one row for each on the device.
// That is all the reference's dense assign leaves non-zero; a new batch's row finds its old row by id, or none (zero).
#include "gcn_host.hpp"

#include "apr_kernels.hpp"

using yue_host::download;
using yue_host::upload;
using yue_host::fail;

namespace {
enum { kCoef = 0, kRows = 1, kNorm = 2, kAdam = 3, kPhases = 4 };
}

struct yue_apr {
    int64_t m = 0, n = 0;
    int k = 0;
    // the perturbation: ids ascending, rows in dU[cur] / dV[cur]
    std::vector<int32_t> ids_u, ids_i;
    DevBuf<float> dU[2], dV[2];
    int cur = 0;
    // the running batch
    int64_t T = 0, Du = 0, Di = 0;
    std::vector<int32_t> du, di, cu, ci, cj, map_u, map_i, cnt, at, pack;
    size_t o_u = 0, o_i = 0, o_j = 0, o_old = 0, o_new = 0, o_row = 0, o_seg = 0, o_ent = 0;
    DevBuf<int32_t> idx;
    DevBuf<float> a, b, raw;
    DevBuf<double> loss;
    std::vector<double> h_loss;
    gcn::PhaseTimer timer;
};

namespace {

void clear_delta(yue_apr *s) { s->ids_u.clear(); s->ids_i.clear(); }

int apr_ready(yue_ctx *c, yue_apr **out, const char *who) {
    const std::string w(who);
    if (!c) return fail(YUE_ERR_ARG, w + ": null context");
    if (!c->have_factors) return fail(YUE_ERR_ARG, w + ": no factors uploaded");
    static_assert(yue::kAprMaxK == 256, "yue_set_factors admits k <= 256");
    yue_apr *s = nullptr;
    int rc = yue_host::state(c, c->apr, &s);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    if (s->m != c->m || s->n != c->n || s->k != c->k) {             // factors of another shape: their perturbation is gone
        clear_delta(s);
        s->m = c->m; s->n = c->n; s->k = c->k;
        s->map_u.assign((size_t)c->m, -1); s->map_i.assign((size_t)c->n, -1);
    }
    s->timer.stamps = 0;
    *out = s;
    return YUE_OK;
}

int stamp(yue_ctx *c, yue_apr *s, int phase) { return gcn::stamp(c, s->timer, phase); }

// position of `id` in the ascending list, or -1
int32_t find(const std::vector<int32_t> &ids, int32_t id) {
    const auto it = std::lower_bound(ids.begin(), ids.end(), id);
    return it != ids.end() && *it == id ? (int32_t)(it - ids.begin()) : -1;
}

// the batch's checks, then everything the kernels index with; nothing is launched before the last check
int prepare(yue_ctx *c, yue_apr *s, const int32_t *u, const int32_t *i, const int32_t *j, int64_t T, const char *who) {
    const std::string w(who);
    if (T < 1 || T >= (1ll << 29) || !u || !i || !j) return fail(YUE_ERR_ARG, w + ": needs 1 <= T < 2^29 and the three id arrays");
    int rc;
    if ((rc = check_ids(w + ": user", u, T, s->m)) || (rc = check_ids(w + ": positive item", i, T, s->n)) || (rc = check_ids(w + ": negative item", j, T, s->n)))
        return rc;
    // distinct users and items (positives and negatives together), ascending; a triplet's compact rows
    s->du.clear(); s->di.clear();
    for (int64_t t = 0; t < T; ++t) {
        if (s->map_u[(size_t)u[t]] < 0) { s->map_u[(size_t)u[t]] = 0; s->du.push_back(u[t]); }
        if (s->map_i[(size_t)i[t]] < 0) { s->map_i[(size_t)i[t]] = 0; s->di.push_back(i[t]); }
        if (s->map_i[(size_t)j[t]] < 0) { s->map_i[(size_t)j[t]] = 0; s->di.push_back(j[t]); }
    }
    std::sort(s->du.begin(), s->du.end()); std::sort(s->di.begin(), s->di.end());
    const int64_t Du = (int64_t)s->du.size(), Di = (int64_t)s->di.size(), S = Du + Di;
    for (int64_t r = 0; r < Du; ++r) s->map_u[(size_t)s->du[(size_t)r]] = (int32_t)r;
    for (int64_t r = 0; r < Di; ++r) s->map_i[(size_t)s->di[(size_t)r]] = (int32_t)r;
    s->cu.resize((size_t)T); s->ci.resize((size_t)T); s->cj.resize((size_t)T);
    for (int64_t t = 0; t < T; ++t) { s->cu[(size_t)t] = s->map_u[(size_t)u[t]]; s->ci[(size_t)t] = s->map_i[(size_t)i[t]]; s->cj[(size_t)t] = s->map_i[(size_t)j[t]]; }
    for (int64_t r = 0; r < Du; ++r) s->map_u[(size_t)s->du[(size_t)r]] = -1;
    for (int64_t r = 0; r < Di; ++r) s->map_i[(size_t)s->di[(size_t)r]] = -1;
    s->T = T; s->Du = Du; s->Di = Di;
    // every row's entries by a counting sort over the compact rows (users, then items), triplets ascending within a row
    s->cnt.assign((size_t)S + 1, 0);
    for (int64_t t = 0; t < T; ++t) { s->cnt[(size_t)s->cu[(size_t)t] + 1]++; s->cnt[(size_t)(Du + s->ci[(size_t)t]) + 1]++; s->cnt[(size_t)(Du + s->cj[(size_t)t]) + 1]++; }
    int64_t longest = 0;
    for (int64_t r = 0; r < S; ++r) { longest = std::max<int64_t>(longest, s->cnt[(size_t)r + 1]); s->cnt[(size_t)r + 1] += s->cnt[(size_t)r]; }
    c->apr_longest = longest;
    s->at.assign(s->cnt.begin(), s->cnt.end() - 1);
    // one upload: u, i, j | the triplets' rows in the standing perturbation (3 T) | in this batch's (3 T) | row ids | segments | entries
    std::vector<int32_t> &pk = s->pack;
    pk.clear();
    auto add = [&](const int32_t *v, int64_t count) { const size_t o = pk.size(); pk.insert(pk.end(), v, v + count); return o; };
    s->o_u = add(u, T); s->o_i = add(i, T); s->o_j = add(j, T);
    s->o_old = pk.size();
    pk.resize(pk.size() + (size_t)(3 * T));
    for (int64_t t = 0; t < T; ++t) {
        pk[s->o_old + (size_t)t] = find(s->ids_u, u[t]);
        pk[s->o_old + (size_t)(T + t)] = find(s->ids_i, i[t]);
        pk[s->o_old + (size_t)(2 * T + t)] = find(s->ids_i, j[t]);
    }
    s->o_new = add(s->cu.data(), T); add(s->ci.data(), T); add(s->cj.data(), T);
    s->o_row = add(s->du.data(), Du); add(s->di.data(), Di);
    s->o_seg = add(s->cnt.data(), S + 1);
    s->o_ent = pk.size();
    pk.resize(pk.size() + (size_t)(3 * T));
    int32_t *ent = pk.data() + s->o_ent;
    for (int64_t t = 0; t < T; ++t) {
        ent[s->at[(size_t)s->cu[(size_t)t]]++] = (int32_t)t;
        ent[s->at[(size_t)(Du + s->ci[(size_t)t])]++] = (int32_t)(2 * t);
        ent[s->at[(size_t)(Du + s->cj[(size_t)t])]++] = (int32_t)(2 * t + 1);
    }
    HIPCHK(hipStreamSynchronize(c->stream));             // (the blocking upload below overwrites what an earlier call's kernels read)
    if ((rc = upload(s->idx, pk))) return rc;
    const size_t k = (size_t)s->k;
    HIPCHK(s->a.resize((size_t)T)); HIPCHK(s->b.resize((size_t)T)); HIPCHK(s->loss.resize((size_t)T));
    HIPCHK(s->raw.resize((size_t)S * k)); HIPCHK(s->dU[1 - s->cur].resize((size_t)Du * k)); HIPCHK(s->dV[1 - s->cur].resize((size_t)Di * k));
    HIPCHK(s->dU[s->cur].resize(1)); HIPCHK(s->dV[s->cur].resize(1));          // (never a null pointer: null means "no perturbation")
    return YUE_OK;
}

// perturbed: the launch reads the standing perturbation, each triplet's rows through the indices at o_old
yue::AprArgs args(yue_ctx *c, yue_apr *s, bool perturbed) {
    yue::AprArgs a{};
    const int32_t *ix = s->idx.p;
    const int64_t T = s->T;
    a.U = c->P.p; a.V = c->Q.p; a.k = s->k; a.u = ix + s->o_u; a.i = ix + s->o_i; a.j = ix + s->o_j; a.T = T;
    if (perturbed) {
        const int32_t *x = ix + s->o_old;
        a.dU = s->dU[s->cur].p; a.dV = s->dV[s->cur].p; a.xu = x; a.xi = x + T; a.xj = x + 2 * T;
    }
    a.a = s->a.p; a.b = s->b.p; a.loss = s->loss.p;
    a.Du = s->Du; a.Di = s->Di; a.row_id = ix + s->o_row; a.seg_ptr = ix + s->o_seg; a.ent = ix + s->o_ent;
    a.gU = c->dP.p; a.gV = c->dQ.p; a.raw = s->raw.p; a.nU = s->dU[1 - s->cur].p; a.nV = s->dV[1 - s->cur].p;
    return a;
}

int launch_coef(yue_ctx *c, yue_apr *s, const yue::AprArgs &a) {
    yue_host::with_kr(a.k, [&](auto kr) { hipLaunchKernelGGL(yue::k_apr_coef<kr()>, dim3((unsigned)((a.T + 3) / 4)), dim3(256), 0, c->stream, a); });
    HIPCHK(hipGetLastError());
    return stamp(c, s, kCoef);
}

template <int FORM>
int launch_rows(yue_ctx *c, yue_apr *s, const yue::AprArgs &a) {
    yue_host::with_kr(a.k, [&](auto kr) {
        hipLaunchKernelGGL((yue::k_apr_rows<kr(), FORM>), dim3((unsigned)((a.Du + a.Di + 3) / 4)), dim3(256), 0, c->stream, a);
    });
    HIPCHK(hipGetLastError());
    return stamp(c, s, FORM == yue::kAprDelta ? kNorm : kRows);
}

// the first sess.run of a phase-2 step: the gradient with respect to the standing perturbation, normalised into the new one,
// which holds this batch's distinct rows and nothing else (the assign overwrites the whole variable)
int delta_update(yue_ctx *c, yue_apr *s, double eps, double regA) {
    yue::AprArgs a = args(c, s, true);
    a.regA = (float)regA; a.eps = (float)eps;
    int rc;
    if ((rc = launch_coef(c, s, a)) || (rc = launch_rows<yue::kAprDelta>(c, s, a))) return rc;
    s->cur = 1 - s->cur;
    s->ids_u = s->du; s->ids_i = s->di;
    // the standing perturbation is this batch's: a triplet's rows in it are its compact rows
    s->o_old = s->o_new;
    return YUE_OK;
}

// coefficients and the parameter gradient's rows into dP / dQ
int param_grad(yue_ctx *c, yue_apr *s, bool adversarial, double reg) {
    yue::AprArgs a = args(c, s, adversarial);
    a.reg = adversarial ? 0.0f : (float)reg; a.regA = adversarial ? (float)reg : 0.0f;
    int rc;
    if ((rc = launch_coef(c, s, a))) return rc;
    return adversarial ? launch_rows<yue::kAprAdv>(c, s, a) : launch_rows<yue::kAprPre>(c, s, a);
}

// before anything is written into dP / dQ: yue_adam_reset clears them with the moments
int adam_ready(yue_ctx *c) { return c->adam_m != c->m || c->adam_n != c->n || c->adam_k != c->k ? yue_adam_reset(c) : YUE_OK; }

int adam(yue_ctx *c, yue_apr *s, double lr, int64_t step) {
    const int rc = yue_host::adam_apply(c, lr, step);
    return rc ? rc : stamp(c, s, kAdam);
}

// waits for the stream; the loss is the triplets' terms added in triplet order
int finish(yue_ctx *c, yue_apr *s, double *loss_out) {
    if (loss_out) {
        s->h_loss.resize((size_t)s->T);
        HIPCHK(hipMemcpyAsync(s->h_loss.data(), s->loss.p, (size_t)s->T * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    if (loss_out) {
        double loss = 0.0;
        for (int64_t t = 0; t < s->T; ++t) loss += s->h_loss[(size_t)t];
        *loss_out = loss;
    }
    return gcn::read_times(s->timer, c->apr_ns, kPhases);
}

// compact rows scattered into a dense, zeroed [rows, k] (out may be null)
void scatter(float *out, int64_t rows, int k, const std::vector<int32_t> &ids, const float *compact) {
    if (!out) return;
    std::fill(out, out + rows * k, 0.0f);
    for (size_t r = 0; r < ids.size(); ++r) std::copy(compact + r * (size_t)k, compact + (r + 1) * (size_t)k, out + (int64_t)ids[r] * k);
}

int get_delta(yue_apr *s, float *dU_out, float *dV_out) {
    const size_t k = (size_t)s->k;
    std::vector<float> hu(std::max<size_t>(1, s->ids_u.size() * k)), hv(std::max<size_t>(1, s->ids_i.size() * k));
    int rc;
    if ((rc = download(hu.data(), s->dU[s->cur], s->ids_u.size() * k)) || (rc = download(hv.data(), s->dV[s->cur], s->ids_i.size() * k))) return rc;
    scatter(dU_out, s->m, s->k, s->ids_u, hu.data());
    scatter(dV_out, s->n, s->k, s->ids_i, hv.data());
    return YUE_OK;
}

}  // namespace

extern "C" {

int yue_apr_reset(yue_ctx *c) {
    yue_apr *s = nullptr;
    int rc = apr_ready(c, &s, "yue_apr_reset");
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    clear_delta(s);
    return YUE_OK;
}

int yue_apr_set_delta(yue_ctx *c, const int32_t *users, int64_t n_users, const float *rows_u, const int32_t *items, int64_t n_items, const float *rows_v) {
    yue_apr *s = nullptr;
    int rc = apr_ready(c, &s, "yue_apr_set_delta");
    if (rc) return rc;
    if (n_users < 0 || n_items < 0 || n_users > s->m || n_items > s->n || (n_users > 0 && (!users || !rows_u)) || (n_items > 0 && (!items || !rows_v)))
        return fail(YUE_ERR_ARG, "yue_apr_set_delta: needs 0 <= n_users <= m, 0 <= n_items <= n and their ids and rows");
    const int64_t pu[2] = {0, n_users}, pi[2] = {0, n_items};
    if ((rc = check_rows("yue_apr_set_delta: user", pu, 1, users, s->m, yue_host::kNoTotal, Order::ascending)) ||
        (rc = check_rows("yue_apr_set_delta: item", pi, 1, items, s->n, yue_host::kNoTotal, Order::ascending)))
        return rc;
    for (int64_t e = 0; e < n_users * s->k; ++e) if (!std::isfinite(rows_u[e])) return fail(YUE_ERR_ARG, "yue_apr_set_delta: row not finite");
    for (int64_t e = 0; e < n_items * s->k; ++e) if (!std::isfinite(rows_v[e])) return fail(YUE_ERR_ARG, "yue_apr_set_delta: row not finite");
    HIPCHK(hipStreamSynchronize(c->stream));
    if ((rc = upload(s->dU[s->cur], rows_u, n_users * s->k)) || (rc = upload(s->dV[s->cur], rows_v, n_items * s->k))) return rc;
    s->ids_u.assign(users, users + n_users); s->ids_i.assign(items, items + n_items);
    return YUE_OK;
}

int yue_apr_get_delta(yue_ctx *c, float *dU_out, float *dV_out) {
    yue_apr *s = nullptr;
    int rc = apr_ready(c, &s, "yue_apr_get_delta");
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    return get_delta(s, dU_out, dV_out);
}

int yue_apr_delta_update(yue_ctx *c, const int32_t *u, const int32_t *i, const int32_t *j, int64_t T, double eps, double regA, float *gU_raw_out, float *gV_raw_out) {
    yue_apr *s = nullptr;
    int rc = apr_ready(c, &s, "yue_apr_delta_update");
    if (rc) return rc;
    if (!(eps >= 0.0) || !(regA >= 0.0)) return fail(YUE_ERR_ARG, "yue_apr_delta_update: needs eps >= 0 and regA >= 0");
    if ((rc = prepare(c, s, u, i, j, T, "yue_apr_delta_update")) || (rc = stamp(c, s, kCoef)) || (rc = delta_update(c, s, eps, regA)) || (rc = finish(c, s, nullptr))) return rc;
    const size_t k = (size_t)s->k;
    std::vector<float> raw((size_t)(s->Du + s->Di) * k);
    if ((rc = download(raw.data(), s->raw, raw.size()))) return rc;
    scatter(gU_raw_out, s->m, s->k, s->du, raw.data());
    scatter(gV_raw_out, s->n, s->k, s->di, raw.data() + (size_t)s->Du * k);
    return YUE_OK;
}

int yue_apr_grad(yue_ctx *c, int adversarial, const int32_t *u, const int32_t *i, const int32_t *j, int64_t T, double reg, double *loss_out, float *gU_out,
                 float *gV_out) {
    yue_apr *s = nullptr;
    int rc = apr_ready(c, &s, "yue_apr_grad");
    if (rc) return rc;
    if (!(reg >= 0.0)) return fail(YUE_ERR_ARG, "yue_apr_grad: needs reg (phase 1) or regA (adversarial) >= 0");
    if ((rc = prepare(c, s, u, i, j, T, "yue_apr_grad")) || (rc = stamp(c, s, kCoef)) || (rc = param_grad(c, s, adversarial != 0, reg)) || (rc = finish(c, s, loss_out)))
        return rc;
    if ((rc = download(gU_out, c->dP, (size_t)(s->m * s->k))) || (rc = download(gV_out, c->dQ, (size_t)(s->n * s->k)))) return rc;
    // dP / dQ are the cleared gradient buffers of yue_adam_step: hand them back as that call expects them
    HIPCHK(hipMemsetAsync(c->dP.p, 0, (size_t)(s->m * s->k) * sizeof(float), c->stream));
    HIPCHK(hipMemsetAsync(c->dQ.p, 0, (size_t)(s->n * s->k) * sizeof(float), c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return YUE_OK;
}

int yue_apr_pre_step(yue_ctx *c, const int32_t *u, const int32_t *i, const int32_t *j, int64_t T, double lr, double reg, int64_t step, double *loss_out) {
    yue_apr *s = nullptr;
    int rc = apr_ready(c, &s, "yue_apr_pre_step");
    if (rc) return rc;
    if (step < 1 || !(reg >= 0.0)) return fail(YUE_ERR_ARG, "yue_apr_pre_step: needs step >= 1 and reg >= 0");
    if ((rc = adam_ready(c)) || (rc = prepare(c, s, u, i, j, T, "yue_apr_pre_step")) || (rc = stamp(c, s, kCoef)) || (rc = param_grad(c, s, false, reg)) || (rc = adam(c, s, lr, step))) return rc;
    return finish(c, s, loss_out);
}

int yue_apr_adv_step(yue_ctx *c, const int32_t *u, const int32_t *i, const int32_t *j, int64_t T, double lr, double eps, double regA, int64_t step,
                     double *loss_out) {
    yue_apr *s = nullptr;
    int rc = apr_ready(c, &s, "yue_apr_adv_step");
    if (rc) return rc;
    if (step < 1 || !(eps >= 0.0) || !(regA >= 0.0)) return fail(YUE_ERR_ARG, "yue_apr_adv_step: needs step >= 1, eps >= 0 and regA >= 0");
    if ((rc = adam_ready(c)) || (rc = prepare(c, s, u, i, j, T, "yue_apr_adv_step")) || (rc = stamp(c, s, kCoef)) || (rc = delta_update(c, s, eps, regA)) ||
        (rc = param_grad(c, s, true, regA)) || (rc = adam(c, s, lr, step)))
        return rc;
    return finish(c, s, loss_out);
}

int yue_apr_times(yue_ctx *c, int64_t *ns_out) {
    if (!c || !ns_out) return fail(YUE_ERR_ARG, "yue_apr_times: null argument");
    for (int p = 0; p < kPhases; ++p) ns_out[p] = c->apr_ns[p];
    return YUE_OK;
}

}  // extern "C"
