// Host code the graph models share (lgcn_host.hip: LightGCN, ngcf_host.hip: NGCF; DESIGN.md sections 20 and 21): a sparse
// matrix on the device with its hub rows' parts, one product through the kernels of lgcn_kernels.hpp, the minibatch on the
// gathered rows of F, and the phase timer.  Nothing here knows which model calls it: graph checking and assembly, forward and
// backward, the dense layers, the weights, the phase names and the options are each model's own file.
#pragma once
#include "host_common.hpp"

#include "lgcn_kernels.hpp"

#include <utility>

namespace gcn {

using yue_host::fail;
using yue_host::upload;
using yue_host::with_kr;

// one sparse matrix: CSR on host (row pointers) and device, and the hub rows' parts for the threshold they were built with.
// The hub parts' partial rows are the caller's buffer: a model with two matrices shares one, sized for the larger.
struct Graph {
    std::vector<int64_t> h_ptr;
    DevBuf<int64_t> ptr;
    DevBuf<int32_t> col;
    DevBuf<float> w;
    int rpw = 1;                                     // rows per wave of k_lgcn_rows
    int64_t hub_built = -1, H = 0, parts = 0;        // hub rows, rebuilt when the model's hub option differs from hub_built
    DevBuf<int64_t> hub_row, hub_part_ptr, part_beg, part_end;
};

// `who` names the model and its option in the refusal ("yue_lgcn: lgcn_hub")
inline int build_hubs(Graph &g, int64_t N, int64_t thr, const char *who) {
    if (g.hub_built == thr) return YUE_OK;
    std::vector<int64_t> hub_row, hub_part_ptr{0}, part_beg, part_end;
    int64_t light = 0;                                       // entries of the rows k_lgcn_rows keeps
    for (int64_t r = 0; r < N; ++r) {
        const int64_t b = g.h_ptr[(size_t)r], e = g.h_ptr[(size_t)r + 1];
        if (e - b <= thr) { light += e - b; continue; }
        for (int64_t p = b; p < e; p += thr) {               // parts of `thr` neighbours, the last one short
            part_beg.push_back(p); part_end.push_back(std::min(p + thr, e));
        }
        hub_row.push_back(r);
        hub_part_ptr.push_back((int64_t)part_beg.size());
    }
    g.H = (int64_t)hub_row.size(); g.parts = (int64_t)part_beg.size();
    if (g.parts >= INT32_MAX) return fail(YUE_ERR_ARG, std::string(who) + " cuts the hub rows into 2^31 parts or more");
    int rc;
    if ((rc = upload(g.hub_row, hub_row.data(), g.H)) || (rc = upload(g.hub_part_ptr, hub_part_ptr.data(), g.H + 1)) ||
        (rc = upload(g.part_beg, part_beg.data(), g.parts)) || (rc = upload(g.part_end, part_end.data(), g.parts)))
        return rc;
    // many short rows go to one wave: about 64 neighbours' worth, 16 rows at the most
    const int64_t mean = std::max<int64_t>(1, light / std::max<int64_t>(1, N - g.H));
    g.rpw = (int)std::min<int64_t>(16, std::max<int64_t>(1, 64 / mean));
    g.hub_built = thr;
    return YUE_OK;
}

// the graph's part of a product's arguments; the caller adds X and the epilogue's pointers
inline yue::LgcnArgs graph_args(const Graph &g, int64_t N, int64_t m, int k, float *partial) {
    yue::LgcnArgs a{};
    a.ptr = g.ptr.p; a.col = g.col.p; a.w = g.w.p; a.N = N; a.m = m; a.k = k; a.rpw = g.rpw; a.gather = 1;
    a.hub = g.hub_built;
    a.hub_row = g.hub_row.p; a.hub_part_ptr = g.hub_part_ptr.p; a.part_beg = g.part_beg.p; a.part_end = g.part_end.p;
    a.partial = partial; a.H = g.H; a.parts = g.parts;
    return a;
}

// one product with its epilogue: the light rows, then the hub rows' parts and their combination  (k <= 128: KR 1 or 2)
template <int MODE>
int launch_product(yue_ctx *c, const Graph &g, const yue::LgcnArgs &a) {
    const int64_t waves = (a.N + a.rpw - 1) / a.rpw;
    with_kr(a.k, [&](auto kr) {
        constexpr int KR = kr() > 2 ? 2 : kr();
        hipLaunchKernelGGL((yue::k_lgcn_rows<KR, MODE>), dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, c->stream, a);
        if (a.gather && g.H > 0) {
            hipLaunchKernelGGL((yue::k_lgcn_hub_parts<KR>), dim3((unsigned)((g.parts + 3) / 4)), dim3(256), 0, c->stream, a);
            hipLaunchKernelGGL((yue::k_lgcn_hub_combine<KR, MODE>), dim3((unsigned)((g.H + 3) / 4)), dim3(256), 0, c->stream, a);
        }
    });
    HIPCHK(hipGetLastError());
    return YUE_OK;
}

inline int check_batch(yue_ctx *c, const int32_t *u, const int32_t *i, const int32_t *j, int64_t T, const char *who) {
    if (T < 1 || T >= (1ll << 29) || !u || !i || !j) return fail(YUE_ERR_ARG, std::string(who) + ": needs 1 <= T < 2^29 and the three id arrays");
    for (int64_t t = 0; t < T; ++t)
        if (u[t] < 0 || u[t] >= c->m || i[t] < 0 || i[t] >= c->n || j[t] < 0 || j[t] >= c->n)
            return fail(YUE_ERR_ARG, std::string(who) + ": triplet " + std::to_string(t) + " out of range");
    return YUE_OK;
}

// the minibatch's device buffers, and its sorted entries on the host: kept between steps, so that a step allocates nothing
// once the batch size is seen
struct Batch {
    DevBuf<float> coef;
    DevBuf<double> loss;
    DevBuf<int64_t> seg_ptr, seg_row;
    DevBuf<int32_t> ent;
    std::vector<std::pair<int64_t, int32_t>> h_ents;
    std::vector<int64_t> h_seg_ptr, h_seg_row;
    std::vector<int32_t> h_ent;
    std::vector<double> h_loss;
};

// the triplets to the device, then the 3 T (row of F, triplet, role) entries by row, a row's entries in triplet order: the
// order k_lgcn_batch_g adds in.  Item rows of F start at m.
inline int batch_prepare(yue_ctx *c, Batch &b, int64_t m, const int32_t *u, const int32_t *i, const int32_t *j, int64_t T) {
    int rc = yue_host::upload_triplets(c, u, i, j, T, true);
    if (rc) return rc;
    std::vector<std::pair<int64_t, int32_t>> &ents = b.h_ents;
    std::vector<int64_t> &seg_ptr = b.h_seg_ptr, &seg_row = b.h_seg_row;
    std::vector<int32_t> &ent = b.h_ent;
    ents.resize((size_t)(3 * T)); ent.resize((size_t)(3 * T)); seg_ptr.clear(); seg_row.clear();
    for (int64_t t = 0; t < T; ++t) {
        ents[(size_t)(3 * t)] = {u[t], (int32_t)(4 * t)};
        ents[(size_t)(3 * t + 1)] = {m + i[t], (int32_t)(4 * t + 1)};
        ents[(size_t)(3 * t + 2)] = {m + j[t], (int32_t)(4 * t + 2)};
    }
    std::sort(ents.begin(), ents.end());
    for (int64_t p = 0; p < 3 * T; ++p) {
        if (p == 0 || ents[(size_t)p].first != ents[(size_t)p - 1].first) { seg_ptr.push_back(p); seg_row.push_back(ents[(size_t)p].first); }
        ent[(size_t)p] = ents[(size_t)p].second;
    }
    const int64_t S = (int64_t)seg_row.size();
    seg_ptr.push_back(3 * T);
    HIPCHK(hipStreamSynchronize(c->stream));             // (the blocking uploads below overwrite what an earlier call's kernels read)
    if ((rc = upload(b.seg_ptr, seg_ptr.data(), S + 1)) || (rc = upload(b.seg_row, seg_row.data(), S)) || (rc = upload(b.ent, ent.data(), 3 * T))) return rc;
    HIPCHK(b.coef.resize((size_t)T)); HIPCHK(b.loss.resize((size_t)T));
    return YUE_OK;
}

// the prepared batch's loss and dLoss / dF on F [N, width] into G [N, width], which the caller cleared
inline int batch_launch(yue_ctx *c, const Batch &b, const float *F, float *G, int64_t m, int width, int64_t T, double reg) {
    const int64_t S = (int64_t)b.h_seg_row.size();
    yue::LgcnBatchArgs a{};
    a.F = F; a.G = G; a.m = m; a.k = width; a.u = c->xu.p; a.i = c->xi.p; a.j = c->xj.p; a.T = T; a.S = S; a.reg = (float)reg;
    a.c = b.coef.p; a.loss = b.loss.p; a.seg_ptr = b.seg_ptr.p; a.seg_row = b.seg_row.p; a.ent = b.ent.p;
    with_kr(width, [&](auto kr) {
        constexpr int KR = kr();
        hipLaunchKernelGGL((yue::k_lgcn_batch_y<KR>), dim3((unsigned)((T + 3) / 4)), dim3(256), 0, c->stream, a);
        hipLaunchKernelGGL((yue::k_lgcn_batch_g<KR>), dim3((unsigned)((S + 3) / 4)), dim3(256), 0, c->stream, a);
    });
    HIPCHK(hipGetLastError());
    return YUE_OK;
}

// waits for the stream; the batch's loss is the triplets' losses added in triplet order
inline int batch_loss(yue_ctx *c, Batch &b, int64_t T, double *loss_out) {
    b.h_loss.resize((size_t)T);
    HIPCHK(hipMemcpyAsync(b.h_loss.data(), b.loss.p, (size_t)T * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    double loss = 0.0;
    for (int64_t t = 0; t < T; ++t) loss += b.h_loss[(size_t)t];      // triplet order
    if (loss_out) *loss_out = loss;
    return YUE_OK;
}

// time stamps of one call: event t closes an interval that belongs to phase[t] (the first stamp opens the first interval).
// Events are created on demand and kept; a call starts over with stamps = 0.
struct PhaseTimer {
    std::vector<Event> ev;
    std::vector<int> phase;
    size_t stamps = 0;
};

inline int stamp(yue_ctx *c, PhaseTimer &t, int phase) {
    if (t.stamps == t.ev.size()) { t.ev.emplace_back(); t.phase.push_back(0); }
    t.phase[t.stamps] = phase;
    HIPCHK(t.ev[t.stamps++].record(c->stream));
    return YUE_OK;
}

// ns[p] = the device time of phase p's intervals, 0 for a phase that did not run; the stream must have been waited for
inline int read_times(const PhaseTimer &t, int64_t *ns, int phases) {
    for (int p = 0; p < phases; ++p) ns[p] = 0;
    for (size_t s = 1; s < t.stamps; ++s) {
        int64_t interval = 0;
        HIPCHK(yue_host::elapsed(t.ev[s - 1], t.ev[s], &interval));
        ns[t.phase[s]] += interval;
    }
    return YUE_OK;
}

}  // namespace gcn
