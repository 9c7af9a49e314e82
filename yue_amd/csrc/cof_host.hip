// libyue_hip.so -- CoFactor (recommender/advanced/CoFactor.py): the co-occurrence CSR and the level-scheduled item sweep
// (include/yue_hip.h).  Kernels: cof_kernels.hpp.  The factors are the context's P (X, users) and Q (Y, items); the pairs are
// those of yue_wrmf_set_pairs (wrmf_host.hip), whose Gram kernels the sweep reuses; the user half-sweep is yue_wrmf_half_sweep.
#include "host_common.hpp"

#include "cof_kernels.hpp"

#include <climits>
#include <numeric>

using yue_host::fail;
using yue_host::upload;

static_assert(yue_host::kCofRangeHost == yue::kCofRange, "the option table's upper end of cof_pass_items is the count kernel's range");

struct yue_cof {
    // co-occurrence
    DevBuf<int64_t> co_ptr, row_nnz, cursor;
    DevBuf<int32_t> co_idx, co_cnt, events;
    int64_t co_n = -1, co_nnz = 0;
    // SPPMI and the level schedule
    DevBuf<int64_t> sp_ptr;
    DevBuf<int32_t> sp_idx;
    DevBuf<double> sp_val;
    std::vector<int64_t> h_sp_ptr;
    std::vector<int32_t> level;      // per item
    int64_t sp_n = -1, levels = 0;
    // schedule of the uploaded pairs: rows by (level, pairs descending, id), the long rows' chunks
    std::vector<int64_t> level_ptr;
    int64_t sched_long_pairs = 0, sched_generation = -1, chunks = 0;
    bool sched_valid = false;
    DevBuf<int32_t> sched, lpos;
    DevBuf<int64_t> cptr, cbeg, cend;
    DevBuf<double> ws;
    // state
    DevBuf<double> G, w, c;
    int64_t st_n = -1;
    int st_k = 0;
    DevBuf<int> status;
    Event ev[2];
    std::vector<Event> lev_ev;       // one in front of every level's launch and one behind the last
};

namespace {

// The rows level by level (inside a level: most pairs first, ties by id) and the chunks of the rows with more than long_pairs
// pairs; rebuilt when the pairs (a new yue_wrmf_set_pairs), the SPPMI or wrmf_long_pairs changed.
int ensure_schedule(yue_ctx *c, yue_cof *x, const yue_host::WrmfPairsView &v, int64_t long_pairs) {
    if (x->sched_valid && x->sched_long_pairs == long_pairs && x->sched_generation == v.generation) return YUE_OK;
    x->sched_valid = false;
    const int64_t n = c->n;
    std::vector<int64_t> iptr((size_t)n + 1);
    HIPCHK(hipMemcpy(iptr.data(), v.ptr, ((size_t)n + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
    std::vector<int32_t> sched((size_t)n);
    std::iota(sched.begin(), sched.end(), 0);
    std::stable_sort(sched.begin(), sched.end(), [&](int32_t a, int32_t b) {
        if (x->level[(size_t)a] != x->level[(size_t)b]) return x->level[(size_t)a] < x->level[(size_t)b];
        return iptr[(size_t)a + 1] - iptr[(size_t)a] > iptr[(size_t)b + 1] - iptr[(size_t)b];
    });
    x->level_ptr.assign((size_t)x->levels + 1, 0);
    for (int64_t i = 0; i < n; ++i) x->level_ptr[(size_t)x->level[(size_t)i] + 1]++;
    for (int64_t l = 0; l < x->levels; ++l) x->level_ptr[(size_t)l + 1] += x->level_ptr[(size_t)l];
    std::vector<int32_t> lpos((size_t)n, -1);
    std::vector<int64_t> cptr(1, 0), cbeg, cend;
    for (int64_t p = 0; p < n; ++p) {
        const int32_t r = sched[(size_t)p];
        const int64_t b = iptr[(size_t)r], e = iptr[(size_t)r + 1];
        if (e - b <= long_pairs) continue;
        lpos[(size_t)p] = (int32_t)cptr.size() - 1;
        for (int64_t q = b; q < e; q += long_pairs) {
            cbeg.push_back(q);
            cend.push_back(std::min(q + long_pairs, e));
        }
        cptr.push_back((int64_t)cbeg.size());
    }
    int rc;
    if ((rc = upload(x->sched, sched)) || (rc = upload(x->lpos, lpos)) || (rc = upload(x->cptr, cptr)) ||
        (rc = upload(x->cbeg, cbeg)) || (rc = upload(x->cend, cend)))
        return rc;
    x->chunks = (int64_t)cbeg.size();
    HIPCHK(x->ws.resize((size_t)std::max<int64_t>(x->chunks, 1) * yue::kWrmfWsStride));
    x->sched_generation = v.generation;
    x->sched_long_pairs = long_pairs;
    x->sched_valid = true;
    return YUE_OK;
}

}  // namespace

namespace yue_host {

int64_t cof_levels(const yue_ctx *c) { return c->cof ? c->cof->levels : 0; }     // of the SPPMI of yue_cof_set_sppmi
int64_t cof_cooccur_nnz(const yue_ctx *c) { return c->cof && c->cof->co_n >= 0 ? c->cof->co_nnz : 0; }

}  // namespace yue_host

extern "C" {

int yue_cof_cooccur(yue_ctx *c, int filter, int64_t *nnz_out) {
    if (!c || !c->have_factors) return fail(YUE_ERR_ARG, "yue_cof_cooccur: call yue_set_factors first (m, n)");
    if (filter < 0) return fail(YUE_ERR_ARG, "yue_cof_cooccur: filter must be >= 0");
    yue_host::WrmfPairsView vu, vi;
    if (!yue_host::wrmf_pairs_view(c, 0, &vu) || !yue_host::wrmf_pairs_view(c, 1, &vi))
        return fail(YUE_ERR_ARG, "yue_cof_cooccur: call yue_wrmf_set_pairs first (after yue_set_factors)");
    yue_cof *x = nullptr;
    int rc = yue_host::state(c, c->cof, &x);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    const int64_t n = c->n;
    x->co_n = -1;
    int64_t nnz_pairs = 0;
    HIPCHK(hipMemcpy(&nnz_pairs, vi.ptr + n, sizeof(int64_t), hipMemcpyDeviceToHost));
    HIPCHK(x->cursor.resize((size_t)std::max<int64_t>(nnz_pairs, 1)));
    HIPCHK(x->events.resize((size_t)n));
    HIPCHK(x->row_nnz.resize((size_t)n));
    HIPCHK(x->co_ptr.resize((size_t)n + 1));
    yue::CofCoArgs a{};
    a.n = n; a.u_ptr = vu.ptr; a.u_items = vu.idx; a.i_ptr = vi.ptr; a.i_users = vi.idx; a.i_counts = vi.cnt;
    a.cursor = x->cursor.p; a.events = x->events.p; a.filter = filter; a.range = (int)c->opt_cof_pass_items;
    a.row_nnz = x->row_nnz.p; a.fill = 0;
    HIPCHK(x->ev[0].record(c->stream));
    hipLaunchKernelGGL(yue::k_cof_events, dim3((unsigned)((n + yue::kCofThreads - 1) / yue::kCofThreads)), dim3(yue::kCofThreads), 0, c->stream, a);
    hipLaunchKernelGGL(yue::k_cof_cooccur, dim3((unsigned)n), dim3(yue::kCofThreads), 0, c->stream, a);
    HIPCHK(hipGetLastError());
    std::vector<int64_t> ptr((size_t)n + 1, 0);
    HIPCHK(hipMemcpyAsync(ptr.data() + 1, x->row_nnz.p, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    for (int64_t i = 0; i < n; ++i) ptr[(size_t)i + 1] += ptr[(size_t)i];
    const int64_t nnz = ptr[(size_t)n];
    if (nnz > (c->opt_cof_cooccur_mb << 20) / 8)
        return fail(YUE_ERR_ARG, "yue_cof_cooccur: the co-occurrence CSR holds " + std::to_string(nnz) + " entries, more than option cof_cooccur_mb = " +
                                     std::to_string(c->opt_cof_cooccur_mb) + " MiB allows (8 bytes per entry): raise cof_cooccur_mb or the filter");
    HIPCHK(x->co_idx.resize((size_t)std::max<int64_t>(nnz, 1)));
    HIPCHK(x->co_cnt.resize((size_t)std::max<int64_t>(nnz, 1)));
    HIPCHK(hipMemcpyAsync(x->co_ptr.p, ptr.data(), ((size_t)n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, c->stream));
    a.fill = 1; a.ptr = x->co_ptr.p; a.idx = x->co_idx.p; a.cnt = x->co_cnt.p;
    hipLaunchKernelGGL(yue::k_cof_cooccur, dim3((unsigned)n), dim3(yue::kCofThreads), 0, c->stream, a);
    HIPCHK(hipGetLastError());
    HIPCHK(x->ev[1].record(c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(yue_host::elapsed(x->ev[0], x->ev[1], &c->cof_ns[0]));
    x->co_n = n;
    x->co_nnz = nnz;
    if (nnz_out) *nnz_out = nnz;
    return YUE_OK;
}

int yue_cof_get_cooccur(yue_ctx *c, int64_t *ptr, int32_t *idx, int32_t *cnt) {
    if (!c || !c->cof || c->cof->co_n < 0) return fail(YUE_ERR_ARG, "yue_cof_get_cooccur: call yue_cof_cooccur first");
    yue_cof *x = c->cof.get();
    if (!ptr || (x->co_nnz > 0 && (!idx || !cnt))) return fail(YUE_ERR_ARG, "yue_cof_get_cooccur: null output array");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpy(ptr, x->co_ptr.p, ((size_t)x->co_n + 1) * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (x->co_nnz > 0) {
        HIPCHK(hipMemcpy(idx, x->co_idx.p, (size_t)x->co_nnz * sizeof(int32_t), hipMemcpyDeviceToHost));
        HIPCHK(hipMemcpy(cnt, x->co_cnt.p, (size_t)x->co_nnz * sizeof(int32_t), hipMemcpyDeviceToHost));
    }
    return YUE_OK;
}

int yue_cof_set_sppmi(yue_ctx *c, const int64_t *ptr, const int32_t *idx, const double *val, int64_t nnz) {
    if (!c || !c->have_factors) return fail(YUE_ERR_ARG, "yue_cof_set_sppmi: call yue_set_factors first (n)");
    if (nnz < 0 || !ptr || (nnz > 0 && (!idx || !val))) return fail(YUE_ERR_ARG, "yue_cof_set_sppmi: null array or negative nnz");
    const int64_t n = c->n;
    int rc = check_rows("yue_cof_set_sppmi: SPPMI", ptr, n, idx, n, nnz, Order::ascending, yue_host::kNoLimit, [&](int64_t i, int64_t e) {
        return idx[e] == i ? "holds a diagonal entry" : !std::isfinite(val[e]) ? "holds a value that is not finite" : nullptr;
    });
    if (rc) return rc;
    for (int64_t i = 0; i < n; ++i)                      // symmetric: (j, i) exists with the same value (rows ascending: binary search)
        for (int64_t e = ptr[i]; e < ptr[i + 1]; ++e) {
            const int32_t j = idx[e];
            const int32_t *b = idx + ptr[j], *en = idx + ptr[j + 1];
            const int32_t *at = std::lower_bound(b, en, (int32_t)i);
            if (at == en || *at != (int32_t)i || val[at - idx] != val[e])
                return fail(YUE_ERR_ARG, "yue_cof_set_sppmi: not symmetric at (" + std::to_string(i) + ", " + std::to_string(j) + ")");
        }
    yue_cof *x = nullptr;
    if ((rc = yue_host::state(c, c->cof, &x))) return rc;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    x->sp_n = -1;
    x->sched_valid = false;
    HIPCHK(x->sp_ptr.resize((size_t)n + 1));
    HIPCHK(x->sp_idx.resize((size_t)std::max<int64_t>(nnz, 1)));
    HIPCHK(x->sp_val.resize((size_t)std::max<int64_t>(nnz, 1)));
    HIPCHK(hipMemcpy(x->sp_ptr.p, ptr, ((size_t)n + 1) * sizeof(int64_t), hipMemcpyHostToDevice));
    if (nnz > 0) {
        HIPCHK(hipMemcpy(x->sp_idx.p, idx, (size_t)nnz * sizeof(int32_t), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(x->sp_val.p, val, (size_t)nnz * sizeof(double), hipMemcpyHostToDevice));
    }
    // level(i) = 1 + max level of the contexts with a smaller id (those the sequential sweep has updated before it reaches i)
    x->level.assign((size_t)n, 0);
    int32_t top = -1;
    for (int64_t i = 0; i < n; ++i) {
        int32_t l = 0;
        for (int64_t e = ptr[i]; e < ptr[i + 1] && idx[e] < i; ++e) l = std::max(l, x->level[(size_t)idx[e]] + 1);
        x->level[(size_t)i] = l;
        top = std::max(top, l);
    }
    x->levels = (int64_t)top + 1;
    x->h_sp_ptr.assign(ptr, ptr + n + 1);
    x->sp_n = n;
    return YUE_OK;
}

int yue_cof_set_state(yue_ctx *c, const double *G, const double *w, const double *cb) {
    if (!c || !c->have_factors) return fail(YUE_ERR_ARG, "yue_cof_set_state: call yue_set_factors first (n, k)");
    if (!G || !w || !cb) return fail(YUE_ERR_ARG, "yue_cof_set_state: null array");
    yue_cof *x = nullptr;
    int rc = yue_host::state(c, c->cof, &x);
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    const size_t n = (size_t)c->n, k = (size_t)c->k;
    x->st_n = -1;
    HIPCHK(x->G.resize(std::max<size_t>(n * k, 1))); HIPCHK(x->w.resize(std::max<size_t>(n, 1))); HIPCHK(x->c.resize(std::max<size_t>(n, 1)));
    HIPCHK(hipMemcpy(x->G.p, G, n * k * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(x->w.p, w, n * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(x->c.p, cb, n * sizeof(double), hipMemcpyHostToDevice));
    x->st_n = c->n;
    x->st_k = c->k;
    return YUE_OK;
}

int yue_cof_get_state(yue_ctx *c, double *G, double *w, double *cb) {
    if (!c || !c->cof || c->cof->st_n < 0) return fail(YUE_ERR_ARG, "yue_cof_get_state: call yue_cof_set_state first");
    if (!G || !w || !cb) return fail(YUE_ERR_ARG, "yue_cof_get_state: null array");
    yue_cof *x = c->cof.get();
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    const size_t n = (size_t)x->st_n, k = (size_t)x->st_k;
    HIPCHK(hipMemcpy(G, x->G.p, n * k * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(w, x->w.p, n * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(cb, x->c.p, n * sizeof(double), hipMemcpyDeviceToHost));
    return YUE_OK;
}

int yue_cof_item_sweep(yue_ctx *c, double alpha, double regU, double regR) {
    if (!c || !c->have_factors) return fail(YUE_ERR_ARG, "yue_cof_item_sweep: no factors uploaded");
    if (c->k > yue::kWrmfMaxK)
        return fail(YUE_ERR_ARG, "yue_cof_item_sweep: k = " + std::to_string(c->k) + " is not supported (CoFactor solves need 1 <= k <= 128)");
    if (!std::isfinite(alpha) || !std::isfinite(regU) || !std::isfinite(regR) || alpha < 0)
        return fail(YUE_ERR_ARG, "yue_cof_item_sweep: alpha, regU and regR must be finite, alpha >= 0");
    yue_host::WrmfPairsView v;
    if (!yue_host::wrmf_pairs_view(c, 1, &v)) return fail(YUE_ERR_ARG, "yue_cof_item_sweep: call yue_wrmf_set_pairs first (after yue_set_factors)");
    yue_cof *x = c->cof.get();
    if (!x || x->sp_n != c->n) return fail(YUE_ERR_ARG, "yue_cof_item_sweep: call yue_cof_set_sppmi first (after yue_set_factors)");
    if (x->st_n != c->n || x->st_k != c->k) return fail(YUE_ERR_ARG, "yue_cof_item_sweep: call yue_cof_set_state first (G, w, c for the current n and k)");
    HIPCHK(hipSetDevice(c->device));
    int rc = ensure_schedule(c, x, v, c->opt_wrmf_long_pairs);
    if (rc) return rc;
    const int k = c->k;
    yue::CofArgs a{};
    a.w.F = c->P.p; a.w.nf = c->m; a.w.X = c->Q.p; a.w.nr = c->n; a.w.k = k;
    a.w.ptr = v.ptr; a.w.idx = v.idx; a.w.cnt = v.cnt; a.w.sched = x->sched.p;
    a.w.cptr = x->cptr.p; a.w.cbeg = x->cbeg.p; a.w.cend = x->cend.p; a.w.ws = x->ws.p;
    a.w.alpha = alpha; a.w.reg = regU; a.w.want_loss = 0;
    a.lpos = x->lpos.p;
    a.sp_ptr = x->sp_ptr.p; a.sp_idx = x->sp_idx.p; a.sp_val = x->sp_val.p;
    a.G = x->G.p; a.wb = x->w.p; a.cb = x->c.p; a.regR = regR;
    HIPCHK(x->status.resize(1));
    a.w.status = x->status.p;
    const int none = INT_MAX;
    HIPCHK(hipMemcpyAsync(x->status.p, &none, sizeof(int), hipMemcpyHostToDevice, c->stream));
    HIPCHK(x->ev[0].record(c->stream));
    if ((rc = yue_host::wrmf_gram(c, 1, &a.w.G))) return rc;           // X^T X, rounded to fp32 once
    if (x->chunks > 0) hipLaunchKernelGGL(yue::k_cof_chunk, dim3((unsigned)x->chunks), dim3(yue::kWrmfThreads), 0, c->stream, a);
    const int lds = yue::wrmf_dyn_lds(k);
    HIPCHK(hipFuncSetAttribute((const void *)yue::k_cof_solve, hipFuncAttributeMaxDynamicSharedMemorySize, lds));
    const bool timed = c->opt_cof_level_timing != 0;
    if (timed && (int64_t)x->lev_ev.size() < x->levels + 1) x->lev_ev.resize((size_t)x->levels + 1);
    for (int64_t l = 0; l < x->levels; ++l) {                          // one launch per level: the stream orders the levels
        const int64_t rows = x->level_ptr[(size_t)l + 1] - x->level_ptr[(size_t)l];
        a.pos0 = x->level_ptr[(size_t)l];
        if (timed) HIPCHK(x->lev_ev[(size_t)l].record(c->stream));
        hipLaunchKernelGGL(yue::k_cof_solve, dim3((unsigned)rows), dim3(yue::kWrmfThreads), lds, c->stream, a);
    }
    if (timed) HIPCHK(x->lev_ev[(size_t)x->levels].record(c->stream));
    HIPCHK(hipGetLastError());
    HIPCHK(x->ev[1].record(c->stream));
    int status = INT_MAX;
    HIPCHK(hipMemcpyAsync(&status, x->status.p, sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(yue_host::elapsed(x->ev[0], x->ev[1], &c->cof_ns[0]));
    double small_ms = 0.0, ms = 0.0;
    for (int64_t l = 0; timed && l < x->levels; ++l)
        if (x->level_ptr[(size_t)l + 1] - x->level_ptr[(size_t)l] < 256) {
            HIPCHK(yue_host::elapsed(x->lev_ev[(size_t)l], x->lev_ev[(size_t)l + 1], &ms));
            small_ms += ms;
        }
    c->cof_ns[1] = yue_host::ns_of(small_ms);
    if (status != INT_MAX)
        return fail(YUE_ERR_ARG, "yue_cof_item_sweep: non-positive pivot in a Cholesky factorisation of item row " + std::to_string(status) +
                                     " (raise regU or regR)");
    return YUE_OK;
}

}  // extern "C"
