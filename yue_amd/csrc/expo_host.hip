// libyue_hip.so -- ExpoMF (recommender/advanced/ExpoMF.py): exposure-weighted ALS half-sweeps and the exposure prior
// (include/yue_hip.h).  Kernels: expo_kernels.hpp.  The factors are the context's P (theta, users) and Q (beta, items); the
// pairs, the longest-first schedule and the long rows' chunks are those of yue_wrmf_set_pairs (wrmf_host.hip).
#include "host_common.hpp"

#include "expo_kernels.hpp"

#include <climits>

using yue_host::fail;

struct yue_expo {
    DevBuf<float> mu, gws;
    DevBuf<double> ws, part;
    DevBuf<int> status, rows;        // rows: the caller's list of yue_expo_gram_rows
    int64_t n_mu = 0;
    Event ev[2];
    std::vector<std::pair<Event, Event>> gram_ev;     // brackets of the Gram launches of the last half-sweep
};

namespace {

// column splits of a dense kernel: enough workgroups to fill the device for small shapes, a function of the shapes alone
int splits_for(int64_t groups, int64_t cols, int64_t *cols_per_split) {
    const int64_t chunks = std::max<int64_t>(1, (cols + yue::kExpoChunk - 1) / yue::kExpoChunk);
    int64_t s = (1024 + groups - 1) / groups;
    s = std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(s, 16), chunks));
    const int64_t per = (chunks + s - 1) / s;
    *cols_per_split = per * yue::kExpoChunk;
    return (int)((chunks + per - 1) / per);
}

// shapes of the dense Gram for a side of `rows` rows against nf columns: pair blocks of 32 over gy groups of four waves with nb
// blocks each, column splits.  One place for yue_expo_half_sweep and yue_expo_gram_rows.
struct GramPlan { int npairs, gy, nb, splits; int64_t cols_per_split, tiles_all; };
GramPlan gram_plan(int k, int64_t rows, int64_t nf) {
    GramPlan g{};
    g.npairs = k * (k + 1) / 2;
    const int nblk = (g.npairs + 31) / 32;
    g.gy = (nblk + 23) / 24;                                         // at most 6 blocks per wave: 96 + 96 accumulator registers
    const int need = (nblk + 4 * g.gy - 1) / (4 * g.gy);
    g.nb = need <= 2 ? 2 : need <= 4 ? 4 : 6;
    g.tiles_all = (rows + yue::kExpoTile - 1) / yue::kExpoTile;
    g.splits = splits_for(g.tiles_all * g.gy, nf, &g.cols_per_split);
    return g;
}

template <int NB>
int launch_gram(const yue::ExpoArgs &a, dim3 grid, int lds, hipStream_t st) {
    HIPCHK(hipFuncSetAttribute((const void *)yue::k_expo_gram<NB>, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    hipLaunchKernelGGL(yue::k_expo_gram<NB>, grid, dim3(256), lds, st, a);
    return YUE_OK;
}

int launch_gram_nb(int nb, const yue::ExpoArgs &a, dim3 grid, int lds, hipStream_t st) {
    return nb == 2 ? launch_gram<2>(a, grid, lds, st) : nb == 4 ? launch_gram<4>(a, grid, lds, st) : launch_gram<6>(a, grid, lds, st);
}

// what a half-sweep and the Gram read-out refuse alike
int side_checks(yue_ctx *c, const std::string &who, int side, int mu_per_column) {
    if (side != 0 && side != 1) return fail(YUE_ERR_ARG, who + ": side must be 0 (user rows) or 1 (item rows)");
    if (mu_per_column != 0 && mu_per_column != 1) return fail(YUE_ERR_ARG, who + ": mu_per_column must be 0 or 1");
    // mu holds one value per item: the columns of the user side are items; those of the item side are users, which mu can
    // index only when m == n (the reference's own rule for that case)
    if (side == 0 && !mu_per_column) return fail(YUE_ERR_ARG, who + ": the user side takes mu per column (per item)");
    if (side == 1 && mu_per_column && c->m != c->n) return fail(YUE_ERR_ARG, who + ": mu per column on the item side needs m == n");
    return YUE_OK;
}

int common_checks(yue_ctx *c, const char *who, yue_expo **x, double lam_y) {
    if (!c || !c->have_factors) return fail(YUE_ERR_ARG, std::string(who) + ": no factors uploaded");
    if (c->k > yue::kWrmfMaxK) return fail(YUE_ERR_ARG, std::string(who) + ": k = " + std::to_string(c->k) + " is not supported (ExpoMF solves need 1 <= k <= 128)");
    if (c->m >= (1 << 26) || c->n >= (1 << 26)) return fail(YUE_ERR_ARG, std::string(who) + ": m and n must be below 2^26");
    *x = c->expo.get();
    if (!*x || (*x)->n_mu != c->n) return fail(YUE_ERR_ARG, std::string(who) + ": call yue_expo_set_mu first (n values)");
    if (!std::isfinite(lam_y) || !(lam_y > 0)) return fail(YUE_ERR_ARG, std::string(who) + ": lam_y must be finite and positive");
    return YUE_OK;
}

}  // namespace

extern "C" {

int yue_expo_set_pairs(yue_ctx *c, const int64_t *u_ptr, const int32_t *u_items, const int32_t *u_counts,
                       const int64_t *i_ptr, const int32_t *i_users, const int32_t *i_counts, int64_t nnz) {
    if (c && c->have_factors && (c->m >= (1 << 26) || c->n >= (1 << 26))) return fail(YUE_ERR_ARG, "yue_expo_set_pairs: m and n must be below 2^26");
    return yue_wrmf_set_pairs(c, u_ptr, u_items, u_counts, i_ptr, i_users, i_counts, nnz);
}

int yue_expo_set_mu(yue_ctx *c, const float *mu, int64_t n) {
    if (!c || !c->have_factors) return fail(YUE_ERR_ARG, "yue_expo_set_mu: call yue_set_factors first (n)");
    if (!mu || n != c->n) return fail(YUE_ERR_ARG, "yue_expo_set_mu: mu must hold one value per item (n of yue_set_factors)");
    for (int64_t i = 0; i < n; ++i)
        if (!(mu[i] > 0.0f && mu[i] < 1.0f)) return fail(YUE_ERR_ARG, "yue_expo_set_mu: mu[" + std::to_string(i) + "] is outside (0, 1)");
    yue_expo *x = nullptr;
    int rc = yue_host::state(c, c->expo, &x);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(x->mu.resize((size_t)n));
    HIPCHK(hipMemcpy(x->mu.p, mu, (size_t)n * sizeof(float), hipMemcpyHostToDevice));
    x->n_mu = n;
    return YUE_OK;
}

int yue_expo_get_mu(yue_ctx *c, float *mu, int64_t n) {
    if (!c || !c->expo || c->expo->n_mu == 0) return fail(YUE_ERR_ARG, "yue_expo_get_mu: no mu on the device");
    if (!mu || n != c->expo->n_mu) return fail(YUE_ERR_ARG, "yue_expo_get_mu: n must be the n of yue_expo_set_mu");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(mu, c->expo->mu.p, (size_t)n * sizeof(float), hipMemcpyDeviceToHost));
    return YUE_OK;
}

int yue_expo_half_sweep(yue_ctx *c, int side, double lam, double lam_y, int mu_per_column) {
    yue_expo *x = nullptr;
    int rc = common_checks(c, "yue_expo_half_sweep", &x, lam_y);
    if (rc) return rc;
    if ((rc = side_checks(c, "yue_expo_half_sweep", side, mu_per_column))) return rc;
    if (!std::isfinite(lam) || lam < 0) return fail(YUE_ERR_ARG, "yue_expo_half_sweep: lam must be finite and >= 0");
    yue_host::WrmfPairsView v;
    if (!yue_host::wrmf_pairs_view(c, side, &v)) return fail(YUE_ERR_ARG, "yue_expo_half_sweep: call yue_expo_set_pairs first (after yue_set_factors)");
    HIPCHK(hipSetDevice(c->device));
    const int k = c->k;
    yue::ExpoArgs a{};
    a.F = side == 0 ? c->Q.p : c->P.p; a.nf = side == 0 ? c->n : c->m;
    a.X = side == 0 ? c->P.p : c->Q.p; a.nr = v.rows; a.k = k;
    a.ptr = v.ptr; a.idx = v.idx; a.cnt = v.cnt; a.sched = v.sched;
    a.n_long = v.n_long; a.cptr = v.cptr; a.cpos = v.cpos; a.cbeg = v.cbeg; a.cend = v.cend;
    a.mu = x->mu.p; a.mu_per_column = mu_per_column;
    a.lam = lam; a.c0 = std::sqrt(lam_y * M_PI / 2.0); a.hl = lam_y / 2.0;
    const GramPlan g = gram_plan(k, v.rows, a.nf);
    const int gy = g.gy, nb = g.nb;
    const int64_t tiles_all = g.tiles_all;
    a.npairs = g.npairs; a.splits = g.splits; a.cols_per_split = g.cols_per_split;
    // rows per batch: the workspace [splits][rows][npairs] fp32 within the budget, a multiple of the tile
    int64_t rows_batch = (c->opt_expo_gram_mb << 20) / ((int64_t)a.splits * a.npairs * 4);
    rows_batch = std::max<int64_t>(yue::kExpoTile, rows_batch / yue::kExpoTile * yue::kExpoTile);
    rows_batch = std::min<int64_t>(rows_batch, tiles_all * yue::kExpoTile);
    HIPCHK(x->gws.resize((size_t)a.splits * (size_t)rows_batch * (size_t)a.npairs));
    HIPCHK(x->ws.resize((size_t)std::max<int64_t>(v.chunks, 1) * yue::kWrmfWsStride));
    HIPCHK(x->status.resize(1));
    a.gws = x->gws.p; a.ws = x->ws.p; a.status = x->status.p;
    const int64_t batches = (v.rows + rows_batch - 1) / rows_batch;
    if ((int64_t)x->gram_ev.size() < batches) x->gram_ev.resize((size_t)batches);
    const int none = INT_MAX;
    HIPCHK(hipMemcpyAsync(x->status.p, &none, sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHK(x->ev[0].record(c->stream));
    if (v.chunks > 0) hipLaunchKernelGGL(yue::k_expo_chunk, dim3((unsigned)v.chunks), dim3(yue::kWrmfThreads), 0, c->stream, a);
    const int lds_gram = yue::expo_dyn_lds(k), lds_solve = yue::wrmf_dyn_lds(k);
    HIPCHK(hipFuncSetAttribute((const void *)yue::k_expo_solve, hipFuncAttributeMaxDynamicSharedMemorySize, lds_solve));
    for (int64_t b = 0; b < batches; ++b) {
        a.pos0 = b * rows_batch;
        a.pos1 = std::min<int64_t>(a.pos0 + rows_batch, v.rows);
        // rows without pairs become 0 in the solve whatever their Gram: they are the last positions of sched and get no tile
        const int64_t dense = std::min<int64_t>(a.pos1, v.n_nonempty) - a.pos0;
        const dim3 grid((unsigned)((std::max<int64_t>(dense, 0) + yue::kExpoTile - 1) / yue::kExpoTile), (unsigned)gy, (unsigned)a.splits);
        HIPCHK(x->gram_ev[(size_t)b].first.record(c->stream));
        if (grid.x > 0) {
            if ((rc = launch_gram_nb(nb, a, grid, lds_gram, c->stream))) return rc;
        }
        HIPCHK(x->gram_ev[(size_t)b].second.record(c->stream));
        hipLaunchKernelGGL(yue::k_expo_solve, dim3((unsigned)(a.pos1 - a.pos0)), dim3(yue::kWrmfThreads), lds_solve, c->stream, a);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(x->ev[1].record(c->stream));
    int status = INT_MAX;
    HIPCHK(hipMemcpyAsync(&status, x->status.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(yue_host::elapsed(x->ev[0], x->ev[1], &c->expo_ns[0]));
    double gram_ms = 0.0, ms = 0.0;
    for (int64_t b = 0; b < batches; ++b) {
        HIPCHK(yue_host::elapsed(x->gram_ev[(size_t)b].first, x->gram_ev[(size_t)b].second, &ms));
        gram_ms += ms;
    }
    c->expo_ns[1] = yue_host::ns_of(gram_ms);
    c->expo_batches = batches;
    if (status != INT_MAX)
        return fail(YUE_ERR_ARG, std::string("yue_expo_half_sweep: non-positive pivot in the Cholesky factorisation of ") + (side == 0 ? "user" : "item") +
                                     " row " + std::to_string(status) + " (B = F^T diag(A) F + lam*I is not positive definite: raise lam)");
    return YUE_OK;
}

int yue_expo_gram_rows(yue_ctx *c, int side, int mu_per_column, double lam_y, const int32_t *rows, int64_t nrows, double *out) {
    yue_expo *x = nullptr;
    int rc = common_checks(c, "yue_expo_gram_rows", &x, lam_y);
    if (rc) return rc;
    if ((rc = side_checks(c, "yue_expo_gram_rows", side, mu_per_column))) return rc;
    yue_host::WrmfPairsView v;
    if (!yue_host::wrmf_pairs_view(c, side, &v)) return fail(YUE_ERR_ARG, "yue_expo_gram_rows: call yue_expo_set_pairs first (after yue_set_factors)");
    if (!rows || !out || nrows < 1) return fail(YUE_ERR_ARG, "yue_expo_gram_rows: rows and out must hold nrows >= 1 entries");
    for (int64_t t = 0; t < nrows; ++t)
        if (rows[t] < 0 || rows[t] >= v.rows) return fail(YUE_ERR_ARG, "yue_expo_gram_rows: rows[" + std::to_string(t) + "] is outside the side's rows");
    HIPCHK(hipSetDevice(c->device));
    const int k = c->k;
    yue::ExpoArgs a{};
    a.F = side == 0 ? c->Q.p : c->P.p; a.nf = side == 0 ? c->n : c->m;
    a.X = side == 0 ? c->P.p : c->Q.p; a.nr = v.rows; a.k = k;
    a.mu = x->mu.p; a.mu_per_column = mu_per_column;
    a.c0 = std::sqrt(lam_y * M_PI / 2.0); a.hl = lam_y / 2.0;
    // the production shapes: those of a half-sweep over ALL the side's rows, not of this list
    const GramPlan g = gram_plan(k, v.rows, a.nf);
    a.npairs = g.npairs; a.splits = g.splits; a.cols_per_split = g.cols_per_split;
    const size_t cells = (size_t)a.splits * (size_t)nrows * (size_t)a.npairs;
    if (cells * 4 > ((size_t)c->opt_expo_gram_mb << 20)) return fail(YUE_ERR_ARG, "yue_expo_gram_rows: the list's Grams do not fit expo_gram_mb");
    HIPCHK(x->gws.resize(cells));
    HIPCHK(x->rows.resize((size_t)nrows));
    HIPCHK(hipMemcpyAsync(x->rows.p, rows, (size_t)nrows * sizeof(int32_t), hipMemcpyHostToDevice, c->stream));
    a.sched = x->rows.p; a.gws = x->gws.p;
    a.pos0 = 0; a.pos1 = nrows;
    const dim3 grid((unsigned)((nrows + yue::kExpoTile - 1) / yue::kExpoTile), (unsigned)g.gy, (unsigned)a.splits);
    if ((rc = launch_gram_nb(g.nb, a, grid, yue::expo_dyn_lds(k), c->stream))) return rc;
    HIPCHK(hipGetLastError());
    std::vector<float> host(cells);
    HIPCHK(hipMemcpyAsync(host.data(), x->gws.p, cells * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    const size_t per = (size_t)nrows * (size_t)a.npairs;
    for (size_t e = 0; e < per; ++e) {                               // the splits in order in fp64, as k_expo_solve sums them
        double s = 0.0;
        for (int sp = 0; sp < a.splits; ++sp) s += (double)host[(size_t)sp * per + e];
        out[e] = s;
    }
    return YUE_OK;
}

int yue_expo_update_mu(yue_ctx *c, double pa, double pb, double lam_y) {
    yue_expo *x = nullptr;
    int rc = common_checks(c, "yue_expo_update_mu", &x, lam_y);
    if (rc) return rc;
    if (!std::isfinite(pa) || !std::isfinite(pb) || !(pa + pb + (double)c->m - 2.0 > 0)) return fail(YUE_ERR_ARG, "yue_expo_update_mu: a + b + m - 2 must be positive");
    yue_host::WrmfPairsView v;
    if (!yue_host::wrmf_pairs_view(c, 1, &v)) return fail(YUE_ERR_ARG, "yue_expo_update_mu: call yue_expo_set_pairs first (after yue_set_factors)");
    HIPCHK(hipSetDevice(c->device));
    const int k = c->k;
    yue::ExpoArgs a{};
    a.F = c->P.p; a.nf = c->m; a.X = c->Q.p; a.nr = c->n; a.k = k;     // rows: items; columns: users
    a.ptr = v.ptr; a.idx = v.idx; a.cnt = v.cnt;
    a.mu = x->mu.p; a.mu_per_column = 0;
    a.c0 = std::sqrt(lam_y * M_PI / 2.0); a.hl = lam_y / 2.0;
    const int64_t tiles = (c->n + yue::kExpoTile - 1) / yue::kExpoTile;
    a.splits = splits_for(tiles, a.nf, &a.cols_per_split);
    HIPCHK(x->part.resize((size_t)a.splits * (size_t)c->n));
    const int lds = (yue::kExpoChunk + yue::kExpoTile) * yue::expo_ld(k) * 4;
    HIPCHK(hipFuncSetAttribute((const void *)yue::k_expo_asum, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    HIPCHK(x->ev[0].record(c->stream));
    hipLaunchKernelGGL(yue::k_expo_asum, dim3((unsigned)tiles, (unsigned)a.splits), dim3(256), lds, c->stream, a, x->part.p);
    hipLaunchKernelGGL(yue::k_expo_mu, dim3((unsigned)((c->n + 3) / 4)), dim3(256), 0, c->stream, a, (const double *)x->part.p, a.splits, pa, pb, x->mu.p);
    HIPCHK(hipGetLastError());
    HIPCHK(x->ev[1].record(c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(yue_host::elapsed(x->ev[0], x->ev[1], &c->expo_ns[0]));
    c->expo_ns[1] = 0;
    return YUE_OK;
}

}  // extern "C"
