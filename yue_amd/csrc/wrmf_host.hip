// libyue_hip.so -- WRMF (recommender/cf/WRMF.py): implicit ALS half-sweeps with exact fp64 per-row solves (include/yue_hip.h).
// Kernels: wrmf_kernels.hpp.  The factors are the context's P (X, users) and Q (Y, items), so scoring needs nothing else.
#include "host_common.hpp"

#include "wrmf_kernels.hpp"

#include <climits>
#include <numeric>

using yue_host::fail;

static_assert(yue_host::kWrmfStageHost == yue::kWrmfStage, "the option table's lower end of wrmf_long_pairs is the kernels' stage");

// Per side (0: user rows solved from Y, 1: item rows solved from X): the pairs, the longest-first schedule and the chunks
// of the long rows.  Built once per data set by yue_wrmf_set_pairs.
struct yue_wrmf_side {
    DevBuf<int64_t> ptr, cptr, cbeg, cend;
    DevBuf<int32_t> idx, cnt, sched, cpos;
    int64_t rows = 0, n_long = 0, chunks = 0, long_pairs = 0;
    int64_t n_nonempty = 0;          // rows with pairs: the first n_nonempty positions of sched
};

struct yue_wrmf {
    int64_t m = 0, n = 0, nnz = 0;
    int64_t generation = 0;          // bumped by every yue_wrmf_set_pairs: lets a dependent schedule (cof_host.hip) see a new upload
    yue_wrmf_side side[2];
    DevBuf<double> gram_part, G, ws, row_loss, loss;
    DevBuf<int> status;
    Event ev[4];
};

namespace {

int upload_side(int64_t long_pairs, yue_wrmf_side &s, const int64_t *ptr, const int32_t *ids, const int32_t *cnt, int64_t rows, int64_t nnz) {
    s.rows = rows;
    // longest first (stable: equal lengths keep row order), then the long rows' chunks
    std::vector<int32_t> sched((size_t)rows);
    std::iota(sched.begin(), sched.end(), 0);
    std::stable_sort(sched.begin(), sched.end(), [&](int32_t x, int32_t y) { return ptr[x + 1] - ptr[x] > ptr[y + 1] - ptr[y]; });
    std::vector<int64_t> cptr(1, 0), cbeg, cend;
    std::vector<int32_t> cpos;
    s.long_pairs = 0;
    for (int64_t p = 0; p < rows; ++p) {
        const int32_t r = sched[(size_t)p];
        const int64_t len = ptr[r + 1] - ptr[r];
        if (len <= long_pairs) break;
        for (int64_t q = ptr[r]; q < ptr[r + 1]; q += long_pairs) {
            cbeg.push_back(q);
            cend.push_back(std::min(q + long_pairs, ptr[r + 1]));
            cpos.push_back((int32_t)p);
        }
        cptr.push_back((int64_t)cbeg.size());
        s.long_pairs += len;
    }
    s.n_nonempty = 0;
    for (int64_t r = 0; r < rows; ++r) s.n_nonempty += ptr[r + 1] > ptr[r] ? 1 : 0;
    s.n_long = (int64_t)cptr.size() - 1;
    s.chunks = (int64_t)cbeg.size();
    HIPCHK(s.ptr.resize((size_t)rows + 1)); HIPCHK(s.idx.resize((size_t)std::max<int64_t>(nnz, 1))); HIPCHK(s.cnt.resize((size_t)std::max<int64_t>(nnz, 1)));
    HIPCHK(s.sched.resize((size_t)rows)); HIPCHK(s.cptr.resize(cptr.size()));
    HIPCHK(s.cbeg.resize(std::max<size_t>(cbeg.size(), 1))); HIPCHK(s.cend.resize(std::max<size_t>(cend.size(), 1))); HIPCHK(s.cpos.resize(std::max<size_t>(cpos.size(), 1)));
    HIPCHK(hipMemcpy(s.ptr.p, ptr, ((size_t)rows + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
    if (nnz > 0) {
        HIPCHK(hipMemcpy(s.idx.p, ids, (size_t)nnz * sizeof(int32_t), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(s.cnt.p, cnt, (size_t)nnz * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    HIPCHK(hipMemcpy(s.sched.p, sched.data(), (size_t)rows * sizeof(int32_t), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(s.cptr.p, cptr.data(), cptr.size() * sizeof(int64_t), hipMemcpyHostToDevice));
    if (!cbeg.empty()) {
        HIPCHK(hipMemcpy(s.cbeg.p, cbeg.data(), cbeg.size() * sizeof(int64_t), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(s.cend.p, cend.data(), cend.size() * sizeof(int64_t), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(s.cpos.p, cpos.data(), cpos.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    }
    return YUE_OK;
}

}  // namespace

namespace yue_host {

bool wrmf_pairs_view(const yue_ctx *c, int side, WrmfPairsView *v) {
    const yue_wrmf *w = c->wrmf.get();
    if (!w || w->m == 0 || w->m != c->m || w->n != c->n) return false;
    const yue_wrmf_side &s = w->side[side];
    v->ptr = s.ptr.p; v->cptr = s.cptr.p; v->cbeg = s.cbeg.p; v->cend = s.cend.p;
    v->idx = s.idx.p; v->cnt = s.cnt.p; v->sched = s.sched.p; v->cpos = s.cpos.p;
    v->rows = s.rows; v->n_long = s.n_long; v->chunks = s.chunks; v->n_nonempty = s.n_nonempty;
    v->generation = w->generation;
    return true;
}

int wrmf_gram(yue_ctx *c, int side, const double **G) {
    yue_wrmf *w = c->wrmf.get();
    if (!w || w->m == 0 || w->m != c->m || w->n != c->n) return fail(YUE_ERR_ARG, "wrmf_gram: call yue_wrmf_set_pairs first");
    const float *F = side == 0 ? c->Q.p : c->P.p;
    const int64_t nf = side == 0 ? c->n : c->m;
    const int64_t rpb = (nf + yue::kWrmfGramBlocks - 1) / yue::kWrmfGramBlocks;
    hipLaunchKernelGGL(yue::k_wrmf_gram_part, dim3(yue::kWrmfGramBlocks), dim3(yue::kWrmfThreads), 0, c->stream, F, nf, c->k, rpb, w->gram_part.p);
    hipLaunchKernelGGL(yue::k_wrmf_gram_sum, dim3(yue::kWrmfSlots), dim3(yue::kWrmfThreads), 0, c->stream, (const double *)w->gram_part.p, yue::kWrmfGramBlocks, w->G.p);
    HIPCHK(hipGetLastError());
    *G = w->G.p;
    return YUE_OK;
}

int64_t wrmf_long_rows(const yue_ctx *c, int side) { return c->wrmf ? c->wrmf->side[side].n_long : 0; }

}  // namespace yue_host

extern "C" {

int yue_wrmf_set_pairs(yue_ctx *c, const int64_t *u_ptr, const int32_t *u_items, const int32_t *u_counts,
                       const int64_t *i_ptr, const int32_t *i_users, const int32_t *i_counts, int64_t nnz) {
    if (!c || !c->have_factors) return fail(YUE_ERR_ARG, "yue_wrmf_set_pairs: call yue_set_factors first (m, n)");
    if (nnz < 0) return fail(YUE_ERR_ARG, "yue_wrmf_set_pairs: nnz must be >= 0");
    const int64_t m = c->m, n = c->n;
    if (nnz > 0 && (!u_counts || !i_counts)) return fail(YUE_ERR_ARG, "yue_wrmf_set_pairs: null counts array");
    const auto counted = [](const int32_t *cnt) { return [cnt](int64_t, int64_t e) { return cnt[e] < 1 ? "counts must be >= 1" : nullptr; }; };
    int rc = check_rows("yue_wrmf_set_pairs: user-major", u_ptr, m, u_items, n, nnz, Order::ascending, yue_host::kNoLimit, counted(u_counts));
    if (!rc) rc = check_rows("yue_wrmf_set_pairs: item-major", i_ptr, n, i_users, m, nnz, Order::ascending, yue_host::kNoLimit, counted(i_counts));
    if (!rc) rc = check_transpose("yue_wrmf_set_pairs", m, u_ptr, u_items, n, i_ptr, i_users, [&](int64_t e, int64_t q) { return i_counts[q] == u_counts[e]; });
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    yue_wrmf *w = nullptr;
    if ((rc = yue_host::state(c, c->wrmf, &w))) return rc;
    w->m = 0;                                                  // invalid until both sides are up
    if ((rc = upload_side(c->opt_wrmf_long_pairs, w->side[0], u_ptr, u_items, u_counts, m, nnz))) return rc;
    if ((rc = upload_side(c->opt_wrmf_long_pairs, w->side[1], i_ptr, i_users, i_counts, n, nnz))) return rc;
    const int64_t chunks = std::max(w->side[0].chunks, w->side[1].chunks);
    HIPCHK(w->gram_part.resize((size_t)yue::kWrmfGramBlocks * yue::kWrmfWsStride));
    HIPCHK(w->G.resize((size_t)yue::kWrmfSlots * yue::kWrmfThreads));
    HIPCHK(w->ws.resize((size_t)std::max<int64_t>(chunks, 1) * yue::kWrmfWsStride));
    HIPCHK(w->row_loss.resize((size_t)std::max(m, n)));
    HIPCHK(w->loss.resize(1));
    HIPCHK(w->status.resize(1));
    w->m = m; w->n = n; w->nnz = nnz;
    w->generation++;
    return YUE_OK;
}

int yue_wrmf_half_sweep(yue_ctx *c, int side, double alpha, double reg, double *loss_out) {
    if (!c || !c->have_factors) return fail(YUE_ERR_ARG, "yue_wrmf_half_sweep: no factors uploaded");
    yue_wrmf *w = c->wrmf.get();
    if (!w || w->m == 0) return fail(YUE_ERR_ARG, "yue_wrmf_half_sweep: call yue_wrmf_set_pairs first");
    if (w->m != c->m || w->n != c->n) return fail(YUE_ERR_ARG, "yue_wrmf_half_sweep: the factors' shape changed since yue_wrmf_set_pairs");
    if (side != 0 && side != 1) return fail(YUE_ERR_ARG, "yue_wrmf_half_sweep: side must be 0 (user rows) or 1 (item rows)");
    if (c->k > yue::kWrmfMaxK)
        return fail(YUE_ERR_ARG, "yue_wrmf_half_sweep: k = " + std::to_string(c->k) + " is not supported (WRMF solves need 1 <= k <= 128)");
    if (!std::isfinite(alpha) || !std::isfinite(reg) || alpha < 0) return fail(YUE_ERR_ARG, "yue_wrmf_half_sweep: alpha and reg must be finite, alpha >= 0");
    HIPCHK(hipSetDevice(c->device));
    const int k = c->k;
    const yue_wrmf_side &s = w->side[side];
    const int64_t nf = side == 0 ? c->n : c->m;
    yue::WrmfArgs a{};
    a.F = side == 0 ? c->Q.p : c->P.p; a.nf = nf;
    a.X = side == 0 ? c->P.p : c->Q.p; a.nr = s.rows; a.k = k;
    a.ptr = s.ptr.p; a.idx = s.idx.p; a.cnt = s.cnt.p; a.sched = s.sched.p;
    a.n_long = s.n_long; a.cptr = s.cptr.p; a.cpos = s.cpos.p; a.cbeg = s.cbeg.p; a.cend = s.cend.p;
    a.ws = w->ws.p; a.alpha = alpha; a.reg = reg;
    a.want_loss = side == 0 ? 1 : 0; a.row_loss = w->row_loss.p; a.status = w->status.p;
    const int none = INT_MAX;
    HIPCHK(hipMemcpyAsync(w->status.p, &none, sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHK(w->ev[0].record(c->stream));
    int rc = yue_host::wrmf_gram(c, side, &a.G);                // F^T F of the fixed side, rounded to fp32 once
    if (rc) return rc;
    HIPCHK(w->ev[1].record(c->stream));
    if (s.chunks > 0) hipLaunchKernelGGL(yue::k_wrmf_chunk, dim3((unsigned)s.chunks), dim3(yue::kWrmfThreads), 0, c->stream, a);
    HIPCHK(w->ev[2].record(c->stream));
    const int lds = yue::wrmf_dyn_lds(k);
    HIPCHK(hipFuncSetAttribute((const void *)yue::k_wrmf_solve, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    hipLaunchKernelGGL(yue::k_wrmf_solve, dim3((unsigned)s.rows), dim3(yue::kWrmfThreads), lds, c->stream, a);
    if (side == 0) hipLaunchKernelGGL(yue::k_wrmf_loss_sum, dim3(1), dim3(yue::kWrmfThreads), 0, c->stream, (const double *)w->row_loss.p, s.rows, w->loss.p);
    HIPCHK(hipGetLastError());
    HIPCHK(w->ev[3].record(c->stream));
    int status = INT_MAX;
    double loss = 0.0;
    HIPCHK(hipMemcpyAsync(&status, w->status.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    if (side == 0) HIPCHK(hipMemcpyAsync(&loss, w->loss.p, sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(yue_host::elapsed(w->ev[0], w->ev[3], &c->wrmf_ns[0]));
    HIPCHK(yue_host::elapsed(w->ev[1], w->ev[2], &c->wrmf_ns[1]));
    if (status != INT_MAX)
        return fail(YUE_ERR_ARG, std::string("yue_wrmf_half_sweep: non-positive pivot in the Cholesky factorisation of ") + (side == 0 ? "user" : "item") +
                                     " row " + std::to_string(status) + " (A = F^T F + C + reg*I is not positive definite: raise reg)");
    if (loss_out) *loss_out = side == 0 ? loss : 0.0;
    return YUE_OK;
}

}  // extern "C"
