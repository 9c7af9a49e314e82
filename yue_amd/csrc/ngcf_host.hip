// libyue_hip.so -- NGCF (reference recommender/advanced/NGCF.py): the weighted user-item graph and its transpose, the layers
// forward and backward with their two k x k weights, the minibatch and the Adam step (include/yue_hip.h).
// Kernels: ngcf_kernels.hpp (the dense half of a layer, the weight gradients) and lgcn_kernels.hpp (products, minibatch); the
// graphs on the device, a product's launches, the minibatch and the phase timer are gcn_host.hpp's, shared with lgcn_host.hip;
// Adam is k_adam through yue_host::adam_apply (U, V: the context's P, Q and moments) and yue_host::adam_apply_dense (the
// weights, moments kept here).
#include "gcn_host.hpp"

#include "ngcf_kernels.hpp"

using yue_host::upload;
using yue_host::fail;

struct yue_ngcf {
    int64_t m = 0, n = 0, nnz = 0;
    bool have_graph = false;
    gcn::Graph A, At;                                // their hub rows follow the option ngcf_hub
    DevBuf<float> partial;                           // hub parts of the running product, sized for the larger of the two
    // weights [layers][2][k][k], their gradient and Adam moments
    int wl = 0, wk = 0;
    bool have_weights = false;
    DevBuf<float> W, gW, mW, vW, wpart;
    // work: E_0, then per layer S, Z, D [N, k] and ss [N]; F and dLoss / dF [N, (layers + 1) k]; the backward pass's rows
    DevBuf<float> E0, S, Z, D, ss, F, G, gD, gZ, gS;
    gcn::Batch batch;
    gcn::PhaseTimer timer;
};

namespace {

enum { kGather = 0, kDense = 1, kBatch = 2, kBackward = 3, kWgrad = 4, kAdam = 5, kPhases = 6 };

struct Run {                                         // what one call propagates with
    int L, training;
    float keep;
    uint32_t thr;
    uint64_t seed, step;
};

int stamp(yue_ctx *c, yue_ngcf *s, int phase) { return gcn::stamp(c, s->timer, phase); }

int ngcf_ready(yue_ctx *c, yue_ngcf **out, int layers, double keep, const char *who) {
    const std::string w(who);
    if (!c) return fail(YUE_ERR_ARG, w + ": null context");
    if (!c->have_factors) return fail(YUE_ERR_ARG, w + ": call yue_set_factors first (U, V)");
    if (c->k > yue::kNgcfMaxK) return fail(YUE_ERR_ARG, w + ": needs k <= 128");
    if (layers < 1) return fail(YUE_ERR_ARG, w + ": needs layers >= 1");
    if ((int64_t)(layers + 1) * c->k > yue::kNgcfMaxWidth)
        return fail(YUE_ERR_ARG, w + ": needs (layers + 1) k <= 256, the width the minibatch kernels and the scan take");
    if (!(keep > 0.0 && keep <= 1.0)) return fail(YUE_ERR_ARG, w + ": needs 0 < keep <= 1");
    yue_ngcf *s = c->ngcf.get();
    if (!s || !s->have_graph) return fail(YUE_ERR_ARG, w + ": call yue_ngcf_set_graph first");
    if (s->m != c->m || s->n != c->n)
        return fail(YUE_ERR_ARG, w + ": the graph was set for " + std::to_string(s->m) + " users and " + std::to_string(s->n) + " items, the factors hold " +
                                     std::to_string(c->m) + " and " + std::to_string(c->n));
    if (!s->have_weights) return fail(YUE_ERR_ARG, w + ": call yue_ngcf_set_weights first");
    if (s->wl != layers || s->wk != c->k)
        return fail(YUE_ERR_ARG, w + ": the weights were set for " + std::to_string(s->wl) + " layers at k " + std::to_string(s->wk) + ", the call has " +
                                     std::to_string(layers) + " at k " + std::to_string(c->k));
    HIPCHK(hipSetDevice(c->device));
    int rc;
    if ((rc = gcn::build_hubs(s->A, s->m + s->n, c->opt_ngcf_hub, "yue_ngcf: ngcf_hub")) ||
        (rc = gcn::build_hubs(s->At, s->m + s->n, c->opt_ngcf_hub, "yue_ngcf: ngcf_hub")))
        return rc;
    c->ngcf_hubs = s->A.H + s->At.H; c->ngcf_parts = s->A.parts + s->At.parts;
    HIPCHK(s->partial.resize((size_t)std::max<int64_t>(1, std::max(s->A.parts, s->At.parts) * c->k)));
    s->timer.stamps = 0;
    *out = s;
    return YUE_OK;
}

// out = base + M X (base may be null, out may be base); rows below m to outU, the others to outV
int product(yue_ctx *c, yue_ngcf *s, const gcn::Graph &g, const float *X, const float *base, float *outU, float *outV) {
    yue::LgcnArgs a = gcn::graph_args(g, s->m + s->n, s->m, c->k, s->partial.p);
    a.X = X; a.base = base; a.outU = outU; a.outV = outV;
    return gcn::launch_product<yue::kLgcnPlain>(c, g, a);
}

yue::NgcfLayerArgs layer_args(const yue_ctx *c, const yue_ngcf *s, const Run &r, int l) {
    const int64_t N = s->m + s->n, k = c->k, Nk = N * k;
    yue::NgcfLayerArgs a{};
    a.E = l == 1 ? s->E0.p : s->D.p + (int64_t)(l - 2) * Nk;
    a.S = s->S.p + (int64_t)(l - 1) * Nk;
    a.W = s->W.p + (int64_t)(l - 1) * 2 * k * k;
    a.N = N; a.k = c->k; a.ldF = (r.L + 1) * c->k; a.layer = l - 1; a.training = r.training;
    a.keep = r.keep; a.thr = r.thr; a.seed = r.seed; a.step = r.step;
    return a;
}

size_t fwd_lds(int k) { const int KP = (k + 31) & ~31; return (size_t)yue::kNgcfTile * (size_t)(2 * KP + 1 + KP + 1) * sizeof(float); }
size_t bwd_lds(int k) { const int KP = (k + 31) & ~31; return (size_t)yue::kNgcfTile * (size_t)(KP + 1) * sizeof(float); }

// E_0 = [U; V]; per layer S = A E, Z, D and F's block; all kept for the backward pass
int forward(yue_ctx *c, yue_ngcf *s, const Run &r) {
    const int64_t N = s->m + s->n, k = c->k, Nk = N * k, mk = s->m * k, nk = s->n * k, ld = (int64_t)(r.L + 1) * k;
    HIPCHK(s->E0.resize((size_t)Nk)); HIPCHK(s->S.resize((size_t)(r.L * Nk))); HIPCHK(s->Z.resize((size_t)(r.L * Nk)));
    HIPCHK(s->D.resize((size_t)(r.L * Nk))); HIPCHK(s->ss.resize((size_t)(r.L * N))); HIPCHK(s->F.resize((size_t)(N * ld)));
    int rc;
    if ((rc = stamp(c, s, kGather))) return rc;
    HIPCHK(hipMemcpyAsync(s->E0.p, c->P.p, (size_t)mk * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(s->E0.p + mk, c->Q.p, (size_t)nk * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
    HIPCHK(hipMemcpy2DAsync(s->F.p, (size_t)ld * sizeof(float), s->E0.p, (size_t)k * sizeof(float), (size_t)k * sizeof(float), (size_t)N,
                            hipMemcpyDeviceToDevice, c->stream));
    const unsigned tiles = (unsigned)((N + yue::kNgcfTile - 1) / yue::kNgcfTile);
    for (int l = 1; l <= r.L; ++l) {
        yue::NgcfLayerArgs a = layer_args(c, s, r, l);
        float *Sl = s->S.p + (int64_t)(l - 1) * Nk;
        if ((rc = product(c, s, s->A, a.E, nullptr, Sl, Sl + mk))) return rc;
        if ((rc = stamp(c, s, kGather))) return rc;
        a.Z = s->Z.p + (int64_t)(l - 1) * Nk; a.D = s->D.p + (int64_t)(l - 1) * Nk; a.ss = s->ss.p + (int64_t)(l - 1) * N; a.F = s->F.p + (int64_t)l * k;
        hipLaunchKernelGGL(yue::k_ngcf_layer_fwd, dim3(tiles), dim3(256), fwd_lds(c->k), c->stream, a);
        HIPCHK(hipGetLastError());
        if ((rc = stamp(c, s, kDense))) return rc;
    }
    return YUE_OK;
}

// from the last layer down: gZ, the two gZ W^T products, gS and the local part; the weights' gradient; then A^T gS on top
int backward(yue_ctx *c, yue_ngcf *s, const Run &r) {
    const int64_t N = s->m + s->n, k = c->k, Nk = N * k;
    const int KP = (c->k + 31) & ~31;
    HIPCHK(s->gD.resize((size_t)Nk)); HIPCHK(s->gZ.resize((size_t)Nk)); HIPCHK(s->gS.resize((size_t)Nk));
    const int64_t chunks = (N + yue::kNgcfWChunk - 1) / yue::kNgcfWChunk;
    HIPCHK(s->wpart.resize((size_t)(chunks * 2 * k * k)));
    const unsigned tiles = (unsigned)((N + yue::kNgcfTile - 1) / yue::kNgcfTile);
    int rc;
    for (int l = r.L; l >= 1; --l) {
        yue::NgcfLayerArgs a = layer_args(c, s, r, l);
        a.Zr = s->Z.p + (int64_t)(l - 1) * Nk; a.Dr = s->D.p + (int64_t)(l - 1) * Nk; a.ssr = s->ss.p + (int64_t)(l - 1) * N;
        a.gD_in = l < r.L ? s->gD.p : nullptr; a.G = s->G.p + (int64_t)l * k; a.G0 = l == 1 ? s->G.p : nullptr;
        a.gZ = s->gZ.p; a.gS = s->gS.p; a.loc = s->gD.p;
        hipLaunchKernelGGL(yue::k_ngcf_layer_bwd, dim3(tiles), dim3(256), bwd_lds(c->k), c->stream, a);
        HIPCHK(hipGetLastError());
        if ((rc = stamp(c, s, kBackward))) return rc;
        yue::NgcfWgradArgs g{};
        g.E = a.E; g.S = a.S; g.gZ = s->gZ.p; g.N = N; g.chunks = chunks; g.k = c->k; g.partial = s->wpart.p;
        g.gW = s->gW.p + (int64_t)(l - 1) * 2 * k * k;
        const size_t wlds = (size_t)yue::kNgcfTile * 3 * KP * sizeof(float);
        switch (KP / 32) {
            case 1: hipLaunchKernelGGL(yue::k_ngcf_wgrad<1>, dim3((unsigned)chunks), dim3(256), wlds, c->stream, g); break;
            case 2: hipLaunchKernelGGL(yue::k_ngcf_wgrad<2>, dim3((unsigned)chunks), dim3(256), wlds, c->stream, g); break;
            case 3: hipLaunchKernelGGL(yue::k_ngcf_wgrad<3>, dim3((unsigned)chunks), dim3(256), wlds, c->stream, g); break;
            default: hipLaunchKernelGGL(yue::k_ngcf_wgrad<4>, dim3((unsigned)chunks), dim3(256), wlds, c->stream, g); break;
        }
        hipLaunchKernelGGL(yue::k_ngcf_wsum, dim3((unsigned)((2 * k * k + 255) / 256)), dim3(256), 0, c->stream, g);
        HIPCHK(hipGetLastError());
        if ((rc = stamp(c, s, kWgrad))) return rc;
        if (l > 1) rc = product(c, s, s->At, s->gS.p, s->gD.p, s->gD.p, s->gD.p + s->m * k);
        else rc = product(c, s, s->At, s->gS.p, s->gD.p, c->dP.p, c->dQ.p);
        if (rc) return rc;
        if ((rc = stamp(c, s, kBackward))) return rc;
    }
    return YUE_OK;
}

// forward, minibatch (LightGCN's kernels at width (layers + 1) k), backward: the loss, the gradients in dP / dQ / gW
int gradient(yue_ctx *c, yue_ngcf *s, const Run &r, const int32_t *u, const int32_t *i, const int32_t *j, int64_t T, double reg, double *loss_out) {
    const int64_t N = s->m + s->n;
    const int width = (r.L + 1) * c->k;
    int rc;
    if ((rc = gcn::batch_prepare(c, s->batch, s->m, u, i, j, T))) return rc;
    HIPCHK(s->G.resize((size_t)(N * width)));
    if ((rc = forward(c, s, r))) return rc;
    HIPCHK(hipMemsetAsync(s->G.p, 0, (size_t)(N * width) * sizeof(float), c->stream));
    if ((rc = gcn::batch_launch(c, s->batch, s->F.p, s->G.p, s->m, width, T, reg)) || (rc = stamp(c, s, kBatch))) return rc;
    if ((rc = backward(c, s, r))) return rc;
    return gcn::batch_loss(c, s->batch, T, loss_out);
}

Run make_run(int layers, int training, double keep, uint64_t seed, int64_t step) {
    Run r;
    r.L = layers; r.training = training != 0; r.keep = (float)keep; r.thr = (uint32_t)(keep * 16777216.0); r.seed = seed; r.step = (uint64_t)step;
    return r;
}

}  // namespace

extern "C" {

int yue_ngcf_set_graph(yue_ctx *c, int64_t m, int64_t n, const int64_t *ptr, const int32_t *col, const float *w) {
    if (!c || !ptr) return fail(YUE_ERR_ARG, "yue_ngcf_set_graph: null argument");
    if (m <= 0 || n <= 0 || m + n >= (1ll << 31)) return fail(YUE_ERR_ARG, "yue_ngcf_set_graph: need m, n > 0 and m + n < 2^31");
    const int64_t N = m + n;
    const int64_t nnz = ptr[N];
    if (nnz >= (1ll << 31)) return fail(YUE_ERR_ARG, "yue_ngcf_set_graph: needs fewer than 2^31 entries");
    if (nnz > 0 && (!col || !w)) return fail(YUE_ERR_ARG, "yue_ngcf_set_graph: null argument");
    int rc = check_rows("yue_ngcf_set_graph: graph", ptr, N, col, N, yue_host::kNoTotal, Order::ascending, yue_host::kNoLimit,
                        [&](int64_t, int64_t p) { return std::isfinite(w[p]) ? nullptr : "weight not finite"; });
    if (rc) return rc;
    yue_ngcf *s = nullptr;
    if ((rc = yue_host::state(c, c->ngcf, &s))) return rc;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    s->have_graph = false;
    // the transpose by a stable counting sort: a column's entries in ascending source row
    std::vector<int64_t> t_ptr((size_t)N + 1, 0), at((size_t)N, 0);
    for (int64_t p = 0; p < nnz; ++p) t_ptr[(size_t)col[p] + 1]++;
    for (int64_t r = 0; r < N; ++r) { t_ptr[(size_t)r + 1] += t_ptr[(size_t)r]; at[(size_t)r] = t_ptr[(size_t)r]; }
    std::vector<int32_t> t_col((size_t)nnz);
    std::vector<float> t_w((size_t)nnz);
    for (int64_t r = 0; r < N; ++r)
        for (int64_t p = ptr[r]; p < ptr[r + 1]; ++p) {
            const int64_t q = at[(size_t)col[p]]++;
            t_col[(size_t)q] = (int32_t)r; t_w[(size_t)q] = w[p];
        }
    s->A.h_ptr.assign(ptr, ptr + N + 1);
    s->At.h_ptr = t_ptr;
    if ((rc = upload(s->A.ptr, ptr, N + 1)) || (rc = upload(s->A.col, col, nnz)) || (rc = upload(s->A.w, w, nnz)) ||
        (rc = upload(s->At.ptr, t_ptr.data(), N + 1)) || (rc = upload(s->At.col, t_col.data(), nnz)) || (rc = upload(s->At.w, t_w.data(), nnz)))
        return rc;
    s->m = m; s->n = n; s->nnz = nnz; s->A.hub_built = -1; s->At.hub_built = -1;
    s->have_graph = true;
    return YUE_OK;
}

int yue_ngcf_set_weights(yue_ctx *c, int layers, int k, const float *W) {
    if (!c || !W) return fail(YUE_ERR_ARG, "yue_ngcf_set_weights: null argument");
    if (layers < 1 || k < 1 || k > yue::kNgcfMaxK || (int64_t)(layers + 1) * k > yue::kNgcfMaxWidth)
        return fail(YUE_ERR_ARG, "yue_ngcf_set_weights: needs layers >= 1, 1 <= k <= 128 and (layers + 1) k <= 256");
    const int64_t count = (int64_t)layers * 2 * k * k;
    for (int64_t t = 0; t < count; ++t)
        if (!std::isfinite(W[t])) return fail(YUE_ERR_ARG, "yue_ngcf_set_weights: weight not finite");
    int rc;
    yue_ngcf *s = nullptr;
    if ((rc = yue_host::state(c, c->ngcf, &s))) return rc;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    s->have_weights = false;
    if ((rc = upload(s->W, W, count))) return rc;
    HIPCHK(s->gW.resize((size_t)count)); HIPCHK(s->mW.resize((size_t)count)); HIPCHK(s->vW.resize((size_t)count));
    HIPCHK(hipMemset(s->gW.p, 0, (size_t)count * sizeof(float)));
    HIPCHK(hipMemset(s->mW.p, 0, (size_t)count * sizeof(float)));
    HIPCHK(hipMemset(s->vW.p, 0, (size_t)count * sizeof(float)));
    s->wl = layers; s->wk = k;
    s->have_weights = true;
    return YUE_OK;
}

int yue_ngcf_get_weights(yue_ctx *c, float *W, float *mW, float *vW) {
    if (!c || !c->ngcf || !c->ngcf->have_weights) return fail(YUE_ERR_ARG, "yue_ngcf_get_weights: call yue_ngcf_set_weights first");
    yue_ngcf *s = c->ngcf.get();
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    const size_t bytes = (size_t)s->wl * 2 * s->wk * s->wk * sizeof(float);
    if (W) HIPCHK(hipMemcpy(W, s->W.p, bytes, hipMemcpyDeviceToHost));
    if (mW) HIPCHK(hipMemcpy(mW, s->mW.p, bytes, hipMemcpyDeviceToHost));
    if (vW) HIPCHK(hipMemcpy(vW, s->vW.p, bytes, hipMemcpyDeviceToHost));
    return YUE_OK;
}

int yue_ngcf_propagate(yue_ctx *c, int layers, int training, double keep, uint64_t seed, int64_t step, float *S_out, float *Z_out, float *D_out,
                       float *F_out) {
    yue_ngcf *s = nullptr;
    int rc = ngcf_ready(c, &s, layers, keep, "yue_ngcf_propagate");
    if (rc) return rc;
    if (step < 0) return fail(YUE_ERR_ARG, "yue_ngcf_propagate: needs step >= 0");
    const Run r = make_run(layers, training, keep, seed, step);
    const size_t N = (size_t)(s->m + s->n), k = (size_t)c->k, layer_bytes = (size_t)layers * N * k * sizeof(float);
    if ((rc = forward(c, s, r))) return rc;
    if (S_out) HIPCHK(hipMemcpyAsync(S_out, s->S.p, layer_bytes, hipMemcpyDeviceToHost, c->stream));
    if (Z_out) HIPCHK(hipMemcpyAsync(Z_out, s->Z.p, layer_bytes, hipMemcpyDeviceToHost, c->stream));
    if (D_out) HIPCHK(hipMemcpyAsync(D_out, s->D.p, layer_bytes, hipMemcpyDeviceToHost, c->stream));
    if (F_out) HIPCHK(hipMemcpyAsync(F_out, s->F.p, N * (size_t)(layers + 1) * k * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return gcn::read_times(s->timer, c->ngcf_ns, kPhases);
}

int yue_ngcf_grad(yue_ctx *c, int layers, int training, double keep, uint64_t seed, int64_t step, const int32_t *u, const int32_t *i, const int32_t *j,
                  int64_t T, double reg, double *loss_out, float *gU_out, float *gV_out, float *gW_out) {
    yue_ngcf *s = nullptr;
    int rc = ngcf_ready(c, &s, layers, keep, "yue_ngcf_grad");
    if (rc) return rc;
    if (step < 0) return fail(YUE_ERR_ARG, "yue_ngcf_grad: needs step >= 0");
    if ((rc = gcn::check_batch(c, u, i, j, T, "yue_ngcf_grad"))) return rc;
    if ((rc = gradient(c, s, make_run(layers, training, keep, seed, step), u, i, j, T, reg, loss_out))) return rc;
    const size_t mk = (size_t)(c->m * c->k), nk = (size_t)(c->n * c->k);
    if (gU_out) HIPCHK(hipMemcpy(gU_out, c->dP.p, mk * sizeof(float), hipMemcpyDeviceToHost));
    if (gV_out) HIPCHK(hipMemcpy(gV_out, c->dQ.p, nk * sizeof(float), hipMemcpyDeviceToHost));
    if (gW_out) HIPCHK(hipMemcpy(gW_out, s->gW.p, (size_t)layers * 2 * c->k * c->k * sizeof(float), hipMemcpyDeviceToHost));
    // dP / dQ are the cleared gradient buffers of yue_adam_step: hand them back as that call expects them
    HIPCHK(hipMemsetAsync(c->dP.p, 0, mk * sizeof(float), c->stream)); HIPCHK(hipMemsetAsync(c->dQ.p, 0, nk * sizeof(float), c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return gcn::read_times(s->timer, c->ngcf_ns, kPhases);
}

int yue_ngcf_step(yue_ctx *c, int layers, int training, double keep, uint64_t seed, const int32_t *u, const int32_t *i, const int32_t *j, int64_t T,
                  double lr, double reg, int64_t step, double *loss_out) {
    yue_ngcf *s = nullptr;
    int rc = ngcf_ready(c, &s, layers, keep, "yue_ngcf_step");
    if (rc) return rc;
    if ((rc = gcn::check_batch(c, u, i, j, T, "yue_ngcf_step"))) return rc;
    if (step < 1) return fail(YUE_ERR_ARG, "yue_ngcf_step: needs step >= 1");
    if (c->adam_m != c->m || c->adam_n != c->n || c->adam_k != c->k) { if ((rc = yue_adam_reset(c))) return rc; }
    if ((rc = gradient(c, s, make_run(layers, training, keep, seed, step), u, i, j, T, reg, loss_out))) return rc;
    if ((rc = yue_host::adam_apply(c, lr, step))) return rc;
    if ((rc = yue_host::adam_apply_dense(c, s->W.p, s->mW.p, s->vW.p, s->gW.p, (int64_t)layers * 2 * c->k * c->k, lr, step))) return rc;
    if ((rc = stamp(c, s, kAdam))) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    return gcn::read_times(s->timer, c->ngcf_ns, kPhases);
}

}  // extern "C"
