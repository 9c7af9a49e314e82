// libyue_hip.so -- CDAE (reference recommender/advanced/CDAE.py): the denoising autoencoder on a sparse, row-masked input and
// sampled outputs, its gradients regrouped by item and by user, and the dense Adam pass over all five variables
// (include/yue_hip.h).  Kernels: cdae_kernels.hpp.  The host side checks a batch, cuts rows and segments
// longer than the option cdae_hub into parts, builds the two by-item patterns with a counting sort (a stable one: an item's
// entries stay in slot order), ships every index array of the step in one upload and adds the loss in a fixed order.  The phase
// timer is gcn_host.hpp's.
#include "gcn_host.hpp"

#include "cdae_kernels.hpp"

#include <limits>

using yue_host::download;
using yue_host::upload;
using yue_host::fail;

namespace {

enum { kEncode = 0, kDecode = 1, kRegroup = 2, kAdam = 3, kPhases = 4 };
enum { vU = 0, vW = 1, vWd = 2, vB = 3, vBd = 4, kVars = 5 };

// rows / segments cut into parts of at most `hub` entries (host side of yue::CdaeParts)
struct Parts {
    std::vector<int64_t> seg, beg, end, out, off, hub_seg, hub_ptr;
    int64_t partials = 0;
    void clear() { seg.clear(); beg.clear(); end.clear(); out.clear(); off.clear(); hub_seg.clear(); hub_ptr.assign(1, 0); partials = 0; }
    void add(int64_t s, int64_t b, int64_t e, int64_t hub, int64_t o = 0) {
        if (e - b <= hub) { seg.push_back(s); beg.push_back(b); end.push_back(e); out.push_back(-1); off.push_back(o); return; }
        for (int64_t p = b; p < e; p += hub) {
            seg.push_back(s); beg.push_back(p); end.push_back(std::min(p + hub, e)); out.push_back(partials++); off.push_back(o);
        }
        hub_seg.push_back(s); hub_ptr.push_back(partials);
    }
};

// every index array of a call, one after the other in one buffer: one upload
struct Pack {
    std::vector<int64_t> h;
    size_t add(const std::vector<int64_t> &v) { const size_t at = h.size(); h.insert(h.end(), v.begin(), v.end()); return at; }
};

struct PartsAt { size_t seg, beg, end, out, off, hub_seg, hub_ptr; int64_t parts, H; };

PartsAt pack_parts(Pack &pk, const Parts &p) {
    PartsAt a;
    a.seg = pk.add(p.seg); a.beg = pk.add(p.beg); a.end = pk.add(p.end); a.out = pk.add(p.out); a.off = pk.add(p.off);
    a.hub_seg = pk.add(p.hub_seg); a.hub_ptr = pk.add(p.hub_ptr);
    a.parts = (int64_t)p.seg.size(); a.H = (int64_t)p.hub_seg.size();
    return a;
}

}  // namespace

struct yue_cdae {
    int64_t m = 0, n = 0;
    int h = 0;
    bool have_data = false, have_params = false;
    std::vector<int64_t> h_uptr;
    std::vector<int32_t> h_uitems;
    DevBuf<int64_t> uptr;
    DevBuf<int32_t> uitems, ucnt;
    DevBuf<float> var[kVars], mom[kVars], vel[kVars];            // U [m,h], W [n,h], W'^T [n,h], b [h], b' [n]; Adam's m and v
    DevBuf<int32_t> imap, umap;                                  // compact gradient row of an item / a user in the running batch
    // the running batch
    DevBuf<int64_t> idx;
    DevBuf<float> xw, hid, dz, logit, ypred, e, partial, partial_b, gWd, gBd, gWe, gU, gB;
    DevBuf<double> usq, loss, sq;
    DevBuf<int32_t> sat;
    Pack pk;
    Parts enc, seg_dec, seg_enc, seg_usr, seg_all;
    std::vector<int64_t> row_user, sptr64, sitems64, ysrc, src_dec, row_dec, src_enc, row_enc, row_id, titems, dusers, in_ptr, at, cnt_s, cnt_i;
    std::vector<int32_t> h_imap;                                 // host twin of imap, kept at -1 between calls
    size_t o_row_user = 0, o_sptr = 0, o_sitems = 0, o_ysrc = 0, o_src_dec = 0, o_row_dec = 0, o_src_enc = 0, o_row_enc = 0, o_row_id = 0, o_titems = 0, o_dusers = 0;
    PartsAt a_enc{}, a_dec{}, a_ie{}, a_usr{}, a_all{};
    int64_t B = 0, S = 0, Qin = 0, T = 0, D = 0;
    std::vector<double> h_loss, h_usq, h_sq;
    std::vector<int32_t> h_sat;
    int64_t sq_blocks[kVars] = {0, 0, 0, 0, 0};
    gcn::PhaseTimer timer;
};

namespace {

int64_t var_count(const yue_cdae *s, int v) {
    switch (v) {
        case vU: return s->m * s->h;
        case vW: case vWd: return s->n * s->h;
        case vB: return s->h;
        default: return s->n;
    }
}

unsigned dense_blocks(int64_t count) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(8192, (count + 255) / 256)); }

int stamp(yue_ctx *c, yue_cdae *s, int phase) { return gcn::stamp(c, s->timer, phase); }

int cdae_ready(yue_ctx *c, yue_cdae **out, const char *who) {
    const std::string w(who);
    if (!c) return fail(YUE_ERR_ARG, w + ": null context");
    yue_cdae *s = c->cdae.get();
    if (!s || !s->have_data) return fail(YUE_ERR_ARG, w + ": call yue_cdae_set_data first");
    if (!s->have_params) return fail(YUE_ERR_ARG, w + ": call yue_cdae_set_params first");
    HIPCHK(hipSetDevice(c->device));
    s->timer.stamps = 0;
    *out = s;
    return YUE_OK;
}

yue::CdaeParts dev_parts(const yue_cdae *s, const PartsAt &a) {
    yue::CdaeParts p{};
    const int64_t *base = s->idx.p;
    p.seg = base + a.seg; p.beg = base + a.beg; p.end = base + a.end; p.out = base + a.out; p.parts = a.parts;
    p.hub_seg = base + a.hub_seg; p.hub_ptr = base + a.hub_ptr; p.H = a.H;
    p.partial = s->partial.p; p.partial_b = s->partial_b.p;
    return p;
}

// the batch's checks, then everything the kernels index with; nothing is launched before the last check
int prepare(yue_ctx *c, yue_cdae *s, const int32_t *users, int64_t B, const int64_t *sptr, const int32_t *sitems, const char *who) {
    const std::string w(who);
    if (B < 1 || B >= (1ll << 24) || !users || !sptr) return fail(YUE_ERR_ARG, w + ": needs 1 <= B < 2^24, the users and the sample pointers");
    for (int64_t b = 0; b < B; ++b)
        if (users[b] < 0 || users[b] >= s->m) return fail(YUE_ERR_ARG, w + ": slot " + std::to_string(b) + ": user out of range");
    const int64_t S = sptr[B];
    if (S >= (1ll << 31)) return fail(YUE_ERR_ARG, w + ": needs fewer than 2^31 sampled entries");
    int rc = check_rows(w + ": sample", sptr, B, sitems, s->n, yue_host::kNoTotal, Order::ascending);
    if (rc) return rc;
    const int64_t hub = c->opt_cdae_hub, n = s->n;
    s->B = B; s->S = S;
    // encoder rows and their input entries
    s->row_user.assign(users, users + B);
    s->in_ptr.assign((size_t)B + 1, 0);
    s->enc.clear();
    for (int64_t b = 0; b < B; ++b) {
        const int64_t ub = s->h_uptr[(size_t)users[b]], ue = s->h_uptr[(size_t)users[b] + 1];
        s->in_ptr[(size_t)b + 1] = s->in_ptr[(size_t)b] + (ue - ub);
        s->enc.add(b, ub, ue, hub, s->in_ptr[(size_t)b] - ub);
    }
    const int64_t Qin = s->in_ptr[(size_t)B];
    if (Qin >= (1ll << 31)) return fail(YUE_ERR_ARG, w + ": needs fewer than 2^31 input entries");
    s->Qin = Qin;
    // y_true's source per sampled entry: both lists ascend
    s->sptr64.assign(sptr, sptr + B + 1);
    s->sitems64.resize((size_t)S); s->ysrc.resize((size_t)S);
    for (int64_t b = 0; b < B; ++b) {
        int64_t q = s->h_uptr[(size_t)users[b]];
        const int64_t qe = s->h_uptr[(size_t)users[b] + 1], shift = s->in_ptr[(size_t)b] - q;
        for (int64_t p = sptr[b]; p < sptr[b + 1]; ++p) {
            s->sitems64[(size_t)p] = sitems[p];
            while (q < qe && s->h_uitems[(size_t)q] < sitems[p]) ++q;
            s->ysrc[(size_t)p] = q < qe && s->h_uitems[(size_t)q] == sitems[p] ? q + shift : -1;
        }
    }
    // the batch's items, ascending: compact rows of the item gradients
    if ((int64_t)s->h_imap.size() != n) s->h_imap.assign((size_t)n, -1);
    s->titems.clear();
    auto touch = [&](int64_t i) { if (s->h_imap[(size_t)i] < 0) { s->h_imap[(size_t)i] = 0; s->titems.push_back(i); } };
    for (int64_t p = 0; p < S; ++p) touch(sitems[p]);
    for (int64_t b = 0; b < B; ++b)
        for (int64_t q = s->h_uptr[(size_t)users[b]]; q < s->h_uptr[(size_t)users[b] + 1]; ++q) touch(s->h_uitems[(size_t)q]);
    std::sort(s->titems.begin(), s->titems.end());
    const int64_t T = (int64_t)s->titems.size();
    s->T = T;
    for (int64_t t = 0; t < T; ++t) s->h_imap[(size_t)s->titems[(size_t)t]] = (int32_t)t;
    // the two transposed patterns by a counting sort over the compact items, slots ascending within an item
    s->cnt_s.assign((size_t)T + 1, 0); s->cnt_i.assign((size_t)T + 1, 0);
    for (int64_t p = 0; p < S; ++p) s->cnt_s[(size_t)s->h_imap[(size_t)sitems[p]] + 1]++;
    for (int64_t b = 0; b < B; ++b)
        for (int64_t q = s->h_uptr[(size_t)users[b]]; q < s->h_uptr[(size_t)users[b] + 1]; ++q) s->cnt_i[(size_t)s->h_imap[(size_t)s->h_uitems[(size_t)q]] + 1]++;
    for (int64_t t = 0; t < T; ++t) { s->cnt_s[(size_t)t + 1] += s->cnt_s[(size_t)t]; s->cnt_i[(size_t)t + 1] += s->cnt_i[(size_t)t]; }
    s->src_dec.resize((size_t)S); s->row_dec.resize((size_t)S); s->src_enc.resize((size_t)Qin); s->row_enc.resize((size_t)Qin);
    s->at.assign(s->cnt_s.begin(), s->cnt_s.end() - 1);
    for (int64_t b = 0; b < B; ++b)
        for (int64_t p = sptr[b]; p < sptr[b + 1]; ++p) {
            const int64_t q = s->at[(size_t)s->h_imap[(size_t)sitems[p]]]++;
            s->src_dec[(size_t)q] = p; s->row_dec[(size_t)q] = b;
        }
    s->at.assign(s->cnt_i.begin(), s->cnt_i.end() - 1);
    for (int64_t b = 0; b < B; ++b) {
        const int64_t ub = s->h_uptr[(size_t)users[b]], ue = s->h_uptr[(size_t)users[b] + 1];
        for (int64_t q = ub; q < ue; ++q) {
            const int64_t at = s->at[(size_t)s->h_imap[(size_t)s->h_uitems[(size_t)q]]]++;
            s->src_enc[(size_t)at] = s->in_ptr[(size_t)b] + (q - ub); s->row_enc[(size_t)at] = b;
        }
    }
    s->seg_dec.clear(); s->seg_enc.clear();
    for (int64_t t = 0; t < T; ++t) {
        s->seg_dec.add(t, s->cnt_s[(size_t)t], s->cnt_s[(size_t)t + 1], hub);
        s->seg_enc.add(t, s->cnt_i[(size_t)t], s->cnt_i[(size_t)t + 1], hub);
    }
    for (int64_t t = 0; t < T; ++t) s->h_imap[(size_t)s->titems[(size_t)t]] = -1;
    // the slots of a user, ascending; all slots
    std::vector<std::pair<int64_t, int64_t>> us((size_t)B);
    for (int64_t b = 0; b < B; ++b) us[(size_t)b] = {users[b], b};
    std::sort(us.begin(), us.end());
    s->dusers.clear(); s->row_id.resize((size_t)(2 * B)); s->seg_usr.clear(); s->seg_all.clear();
    for (int64_t b = 0, first = 0; b < B; ++b) {
        s->row_id[(size_t)b] = us[(size_t)b].second;
        s->row_id[(size_t)(B + b)] = b;
        if (b + 1 == B || us[(size_t)b + 1].first != us[(size_t)b].first) {
            s->seg_usr.add((int64_t)s->dusers.size(), first, b + 1, hub);
            s->dusers.push_back(us[(size_t)b].first);
            first = b + 1;
        }
    }
    s->D = (int64_t)s->dusers.size();
    s->seg_all.add(0, B, 2 * B, hub);
    c->cdae_hubs = (int64_t)(s->enc.hub_seg.size() + s->seg_dec.hub_seg.size() + s->seg_enc.hub_seg.size() + s->seg_usr.hub_seg.size() + s->seg_all.hub_seg.size());
    c->cdae_parts = s->enc.partials + s->seg_dec.partials + s->seg_enc.partials + s->seg_usr.partials + s->seg_all.partials;
    // one upload
    Pack &pk = s->pk;
    pk.h.clear();
    s->o_row_user = pk.add(s->row_user); s->o_sptr = pk.add(s->sptr64); s->o_sitems = pk.add(s->sitems64); s->o_ysrc = pk.add(s->ysrc);
    s->o_src_dec = pk.add(s->src_dec); s->o_row_dec = pk.add(s->row_dec); s->o_src_enc = pk.add(s->src_enc); s->o_row_enc = pk.add(s->row_enc);
    s->o_row_id = pk.add(s->row_id); s->o_titems = pk.add(s->titems); s->o_dusers = pk.add(s->dusers);
    s->a_enc = pack_parts(pk, s->enc); s->a_dec = pack_parts(pk, s->seg_dec); s->a_ie = pack_parts(pk, s->seg_enc);
    s->a_usr = pack_parts(pk, s->seg_usr); s->a_all = pack_parts(pk, s->seg_all);
    HIPCHK(hipStreamSynchronize(c->stream));             // (the blocking upload below overwrites what an earlier call's kernels read)
    if ((rc = upload(s->idx, pk.h.data(), (int64_t)pk.h.size()))) return rc;
    const size_t h = (size_t)s->h, one = 1;
    const int64_t partials = std::max(std::max(s->enc.partials, s->seg_dec.partials), std::max(std::max(s->seg_enc.partials, s->seg_usr.partials), s->seg_all.partials));
    HIPCHK(s->xw.resize(std::max(one, (size_t)Qin))); HIPCHK(s->hid.resize((size_t)B * h)); HIPCHK(s->dz.resize((size_t)B * h));
    HIPCHK(s->logit.resize(std::max(one, (size_t)S))); HIPCHK(s->ypred.resize(std::max(one, (size_t)S))); HIPCHK(s->e.resize(std::max(one, (size_t)S)));
    HIPCHK(s->partial.resize(std::max(one, (size_t)partials * h))); HIPCHK(s->partial_b.resize(std::max(one, (size_t)partials)));
    HIPCHK(s->gWd.resize(std::max(one, (size_t)T * h))); HIPCHK(s->gBd.resize(std::max(one, (size_t)T))); HIPCHK(s->gWe.resize(std::max(one, (size_t)T * h)));
    HIPCHK(s->gU.resize((size_t)s->D * h)); HIPCHK(s->gB.resize(h));
    HIPCHK(s->usq.resize((size_t)B)); HIPCHK(s->loss.resize((size_t)B)); HIPCHK(s->sat.resize((size_t)B));
    return YUE_OK;
}

template <class K1, class K2, class A>
int launch_parts(yue_ctx *c, K1 parts_kernel, K2 combine_kernel, const A &a) {
    if (a.P.parts > 0) hipLaunchKernelGGL(parts_kernel, dim3((unsigned)((a.P.parts + 3) / 4)), dim3(256), 0, c->stream, a);
    if (a.P.H > 0) hipLaunchKernelGGL(combine_kernel, dim3((unsigned)((a.P.H + 3) / 4)), dim3(256), 0, c->stream, a);
    HIPCHK(hipGetLastError());
    return YUE_OK;
}

int launch_enc(yue_ctx *c, const yue::CdaeEncArgs &a) {
    return yue_host::with_kr(a.h, [&](auto kr) {
        constexpr int KR = kr() > 2 ? 2 : kr();
        return launch_parts(c, yue::k_cdae_enc_parts<KR>, yue::k_cdae_enc_combine<KR>, a);
    });
}

int launch_seg(yue_ctx *c, const yue::CdaeSegArgs &a) {
    return yue_host::with_kr(a.h, [&](auto kr) {
        constexpr int KR = kr() > 2 ? 2 : kr();
        return launch_parts(c, yue::k_cdae_seg_parts<KR>, yue::k_cdae_seg_combine<KR>, a);
    });
}

// the sums of squares of W, W'^T, b, b' before any update: one partial per workgroup, added on the host in ascending order
int sumsq_launch(yue_ctx *c, yue_cdae *s) {
    int64_t blocks = 0;
    for (int v = vW; v < kVars; ++v) { s->sq_blocks[v] = dense_blocks(var_count(s, v)); blocks += s->sq_blocks[v]; }
    HIPCHK(s->sq.resize((size_t)blocks));
    int64_t at = 0;
    for (int v = vW; v < kVars; ++v) {
        yue::CdaeDenseArgs a{};
        a.var = s->var[v].p; a.count = var_count(s, v); a.w = 1; a.partial = s->sq.p + at;
        hipLaunchKernelGGL(yue::k_cdae_dense<false>, dim3((unsigned)s->sq_blocks[v]), dim3(256), 0, c->stream, a);
        at += s->sq_blocks[v];
    }
    HIPCHK(hipGetLastError());
    return YUE_OK;
}

// encoder and sampled decoder of the prepared batch; the loss and the saturated entries come back to the host
int forward(yue_ctx *c, yue_cdae *s, double co, uint64_t seed, int64_t step, double reg, double *loss_out, int64_t *sat_out) {
    const int64_t *ix = s->idx.p;
    int rc;
    if ((rc = stamp(c, s, kEncode))) return rc;
    yue::CdaeEncArgs ea{};
    ea.P = dev_parts(s, s->a_enc); ea.off = ix + s->a_enc.off;
    ea.uptr = s->uptr.p; ea.uitems = s->uitems.p; ea.ucnt = s->ucnt.p; ea.row_user = ix + s->o_row_user;
    ea.W = s->var[vW].p; ea.b = s->var[vB].p; ea.U = s->var[vU].p; ea.h = s->h; ea.training = 1;
    ea.thr = (uint32_t)(co * 16777216.0); ea.seed = seed; ea.step = (uint64_t)step;
    ea.xw = s->xw.p; ea.hid = s->hid.p; ea.ld = s->h; ea.usq = s->usq.p;
    if ((rc = launch_enc(c, ea)) || (rc = stamp(c, s, kEncode))) return rc;
    yue::CdaeDecArgs da{};
    da.sptr = ix + s->o_sptr; da.sitems = ix + s->o_sitems; da.ysrc = ix + s->o_ysrc;
    da.xw = s->xw.p; da.hid = s->hid.p; da.WdT = s->var[vWd].p; da.bd = s->var[vBd].p; da.B = s->B; da.h = s->h;
    da.g0 = 1.0f / (float)(s->B * s->n);
    da.logit = s->logit.p; da.ypred = s->ypred.p; da.e = s->e.p; da.dz = s->dz.p; da.loss = s->loss.p; da.sat = s->sat.p;
    yue_host::with_kr(s->h, [&](auto kr) {
        constexpr int KR = kr() > 2 ? 2 : kr();
        hipLaunchKernelGGL(yue::k_cdae_dec<KR>, dim3((unsigned)((s->B + 3) / 4)), dim3(256), 0, c->stream, da);
    });
    HIPCHK(hipGetLastError());
    if ((rc = sumsq_launch(c, s)) || (rc = stamp(c, s, kDecode))) return rc;
    const size_t B = (size_t)s->B;
    s->h_loss.resize(B); s->h_usq.resize(B); s->h_sat.resize(B); s->h_sq.resize(s->sq.n);
    HIPCHK(hipMemcpyAsync(s->h_loss.data(), s->loss.p, B * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(s->h_usq.data(), s->usq.p, B * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(s->h_sat.data(), s->sat.p, B * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    int64_t blocks = 0;
    for (int v = vW; v < kVars; ++v) blocks += s->sq_blocks[v];
    HIPCHK(hipMemcpyAsync(s->h_sq.data(), s->sq.p, (size_t)blocks * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    double data = 0.0, l2 = 0.0;
    int64_t sat = 0;
    for (size_t b = 0; b < B; ++b) { data += s->h_loss[b]; sat += s->h_sat[b]; }          // slot order
    // an element outside `sample`: y_pred = max(1e-6, 0), y_true = 0, in float32
    const double unsampled = (double)(float)(-std::log((double)(1.0f - yue::kCdaeClamp)));
    const double count = (double)s->B * (double)s->n;
    data = (data + (count - (double)s->S) * unsampled) / count;
    for (int64_t t = 0; t < blocks; ++t) l2 += s->h_sq[(size_t)t];
    for (size_t b = 0; b < B; ++b) l2 += s->h_usq[b];
    c->cdae_saturated = sat;
    if (sat_out) *sat_out = sat;
    if (loss_out) *loss_out = sat > 0 ? std::numeric_limits<double>::infinity() : data + reg * (0.5 * l2);
    return YUE_OK;
}

// the four regroupings into the compact gradient rows
int regroup(yue_ctx *c, yue_cdae *s, double reg) {
    const int64_t *ix = s->idx.p;
    int rc;
    yue::CdaeSegArgs a{};
    a.h = s->h; a.reg = (float)reg;
    a.P = dev_parts(s, s->a_dec); a.src = ix + s->o_src_dec; a.row = ix + s->o_row_dec; a.C = s->e.p; a.X = s->hid.p; a.out = s->gWd.p; a.out_b = s->gBd.p;
    if ((rc = launch_seg(c, a))) return rc;
    a.P = dev_parts(s, s->a_ie); a.src = ix + s->o_src_enc; a.row = ix + s->o_row_enc; a.C = s->xw.p; a.X = s->dz.p; a.out = s->gWe.p; a.out_b = nullptr;
    if ((rc = launch_seg(c, a))) return rc;
    a.P = dev_parts(s, s->a_usr); a.src = nullptr; a.row = ix + s->o_row_id; a.C = nullptr; a.U = s->var[vU].p; a.seg_id = ix + s->o_dusers; a.out = s->gU.p;
    if ((rc = launch_seg(c, a))) return rc;
    a.P = dev_parts(s, s->a_all); a.U = nullptr; a.seg_id = nullptr; a.out = s->gB.p;
    if ((rc = launch_seg(c, a))) return rc;
    return stamp(c, s, kRegroup);
}

int adam(yue_ctx *c, yue_cdae *s, double lr, double reg, int64_t step) {
    const int64_t *ix = s->idx.p;
    HIPCHK(hipMemsetAsync(s->imap.p, 0xFF, (size_t)s->n * sizeof(int32_t), c->stream));
    HIPCHK(hipMemsetAsync(s->umap.p, 0xFF, (size_t)s->m * sizeof(int32_t), c->stream));
    if (s->T > 0) hipLaunchKernelGGL(yue::k_cdae_map, dim3((unsigned)((s->T + 255) / 256)), dim3(256), 0, c->stream, s->imap.p, ix + s->o_titems, s->T);
    hipLaunchKernelGGL(yue::k_cdae_map, dim3((unsigned)((s->D + 255) / 256)), dim3(256), 0, c->stream, s->umap.p, ix + s->o_dusers, s->D);
    const double b1 = 0.9, b2 = 0.999;
    const float lr_t = (float)(lr * std::sqrt(1.0 - std::pow(b2, (double)step)) / (1.0 - std::pow(b1, (double)step)));
    const float *grads[kVars] = {s->gU.p, s->gWe.p, s->gWd.p, s->gB.p, s->gBd.p};
    const int32_t *maps[kVars] = {s->umap.p, s->imap.p, s->imap.p, nullptr, s->imap.p};
    const int widths[kVars] = {s->h, s->h, s->h, s->h, 1};
    for (int v = 0; v < kVars; ++v) {
        yue::CdaeDenseArgs a{};
        a.var = s->var[v].p; a.m = s->mom[v].p; a.v = s->vel[v].p; a.count = var_count(s, v); a.w = widths[v]; a.map = maps[v]; a.G = grads[v];
        a.reg = v == vU ? 0.0f : (float)reg;             // (U's reg term is per slot, in its compact rows)
        a.lr_t = lr_t; a.beta1 = 0.9f; a.beta2 = 0.999f; a.eps = 1e-8f;
        hipLaunchKernelGGL(yue::k_cdae_dense<true>, dim3(dense_blocks(a.count)), dim3(256), 0, c->stream, a);
    }
    HIPCHK(hipGetLastError());
    return stamp(c, s, kAdam);
}

int finish(yue_ctx *c, yue_cdae *s) {
    HIPCHK(hipStreamSynchronize(c->stream));
    return gcn::read_times(s->timer, c->cdae_ns, kPhases);
}

}  // namespace

extern "C" {

int yue_cdae_set_data(yue_ctx *c, int64_t m, int64_t n, const int64_t *ptr, const int32_t *items, const int32_t *counts) {
    if (!c || !ptr) return fail(YUE_ERR_ARG, "yue_cdae_set_data: null argument");
    if (m <= 0 || n <= 0 || m >= (1ll << 31) || n >= (1ll << 31)) return fail(YUE_ERR_ARG, "yue_cdae_set_data: need 0 < m, n < 2^31");
    const int64_t nnz = ptr[m];
    if (nnz >= (1ll << 31)) return fail(YUE_ERR_ARG, "yue_cdae_set_data: needs fewer than 2^31 pairs");
    if (nnz > 0 && (!items || !counts)) return fail(YUE_ERR_ARG, "yue_cdae_set_data: null argument");
    int rc = check_rows("yue_cdae_set_data: user-major", ptr, m, items, n, yue_host::kNoTotal, Order::ascending, yue_host::kNoLimit,
                        [&](int64_t, int64_t p) { return counts[p] < 1 || counts[p] >= (1 << 24) ? "a count must be 1 .. 2^24 - 1" : nullptr; });
    if (rc) return rc;
    yue_cdae *s = nullptr;
    if ((rc = yue_host::state(c, c->cdae, &s))) return rc;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    s->have_data = false;
    if (s->have_params && (s->m != m || s->n != n)) s->have_params = false;          // parameters of another shape
    s->h_uptr.assign(ptr, ptr + m + 1);
    s->h_uitems.assign(items, items + nnz);
    if ((rc = upload(s->uptr, ptr, m + 1)) || (rc = upload(s->uitems, items, nnz)) || (rc = upload(s->ucnt, counts, nnz))) return rc;
    HIPCHK(s->imap.resize((size_t)n)); HIPCHK(s->umap.resize((size_t)m));
    s->h_imap.assign((size_t)n, -1);
    s->m = m; s->n = n;
    s->have_data = true;
    return YUE_OK;
}

int yue_cdae_set_params(yue_ctx *c, int h, const float *U, const float *W, const float *Wd, const float *b, const float *bd) {
    if (!c || !U || !W || !Wd || !b || !bd) return fail(YUE_ERR_ARG, "yue_cdae_set_params: null argument");
    if (h < 1 || h > yue::kCdaeMaxH) return fail(YUE_ERR_ARG, "yue_cdae_set_params: needs 1 <= h <= 128");
    yue_cdae *s = c->cdae.get();
    if (!s || !s->have_data) return fail(YUE_ERR_ARG, "yue_cdae_set_params: call yue_cdae_set_data first (m, n)");
    const int64_t m = s->m, n = s->n;
    const float *given[kVars] = {U, W, Wd, b, bd};
    const int64_t counts[kVars] = {m * h, n * h, n * h, h, n};
    for (int v = 0; v < kVars; ++v)
        for (int64_t t = 0; t < counts[v]; ++t)
            if (!std::isfinite(given[v][t])) return fail(YUE_ERR_ARG, "yue_cdae_set_params: parameter not finite");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    s->have_params = false;
    std::vector<float> WdT((size_t)(n * h));                   // the decoder is kept transposed: a column is a contiguous row
    for (int64_t e = 0; e < h; ++e)
        for (int64_t i = 0; i < n; ++i) WdT[(size_t)(i * h + e)] = Wd[e * n + i];
    given[vWd] = WdT.data();
    int rc;
    for (int v = 0; v < kVars; ++v) {
        if ((rc = upload(s->var[v], given[v], counts[v]))) return rc;
        HIPCHK(s->mom[v].resize((size_t)counts[v])); HIPCHK(s->vel[v].resize((size_t)counts[v]));
        HIPCHK(hipMemset(s->mom[v].p, 0, (size_t)counts[v] * sizeof(float)));
        HIPCHK(hipMemset(s->vel[v].p, 0, (size_t)counts[v] * sizeof(float)));
    }
    s->h = h;
    s->have_params = true;
    return YUE_OK;
}

// every pointer may be NULL; params, m_out and v_out each hold the five arrays in the order U, W, W' [h][n], b, b'
int yue_cdae_get_params(yue_ctx *c, float *const *params, float *const *m_out, float *const *v_out) {
    if (!c || !c->cdae || !c->cdae->have_params) return fail(YUE_ERR_ARG, "yue_cdae_get_params: call yue_cdae_set_params first");
    yue_cdae *s = c->cdae.get();
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    const int64_t n = s->n, h = s->h;
    std::vector<float> T((size_t)(n * h));
    float *const *sets[3] = {params, m_out, v_out};
    const DevBuf<float> *bufs[3] = {s->var, s->mom, s->vel};
    int rc;
    for (int k = 0; k < 3; ++k) {
        if (!sets[k]) continue;
        for (int v = 0; v < kVars; ++v) {
            if (!sets[k][v]) continue;
            if (v != vWd) { if ((rc = download(sets[k][v], bufs[k][v], (size_t)var_count(s, v)))) return rc; continue; }
            if ((rc = download(T.data(), bufs[k][v], (size_t)(n * h)))) return rc;
            for (int64_t i = 0; i < n; ++i)
                for (int64_t e = 0; e < h; ++e) sets[k][v][e * n + i] = T[(size_t)(i * h + e)];
        }
    }
    return YUE_OK;
}

int yue_cdae_forward(yue_ctx *c, const int32_t *users, int64_t B, const int64_t *sample_ptr, const int32_t *sample_items, double co, uint64_t seed,
                     int64_t step, double reg, float *hid_out, int32_t *kept_out, float *logit_out, float *ypred_out, double *loss_out) {
    yue_cdae *s = nullptr;
    int rc = cdae_ready(c, &s, "yue_cdae_forward");
    if (rc) return rc;
    if (!(co > 0.0 && co <= 1.0) || step < 0) return fail(YUE_ERR_ARG, "yue_cdae_forward: needs 0 < co <= 1 and step >= 0");
    if ((rc = prepare(c, s, users, B, sample_ptr, sample_items, "yue_cdae_forward"))) return rc;
    if ((rc = forward(c, s, co, seed, step, reg, loss_out, nullptr))) return rc;
    if ((rc = download(hid_out, s->hid, (size_t)(B * s->h))) || (rc = download(logit_out, s->logit, (size_t)s->S)) || (rc = download(ypred_out, s->ypred, (size_t)s->S)))
        return rc;
    if (kept_out && s->Qin > 0) {
        std::vector<float> xw((size_t)s->Qin);
        if ((rc = download(xw.data(), s->xw, (size_t)s->Qin))) return rc;
        for (int64_t q = 0; q < s->Qin; ++q) kept_out[q] = xw[(size_t)q] != 0.0f;
    }
    return finish(c, s);
}

int yue_cdae_grad(yue_ctx *c, const int32_t *users, int64_t B, const int64_t *sample_ptr, const int32_t *sample_items, double co, uint64_t seed,
                  int64_t step, double reg, double *loss_out, float *gU_out, float *gW_out, float *gWd_out, float *gb_out, float *gbd_out) {
    yue_cdae *s = nullptr;
    int rc = cdae_ready(c, &s, "yue_cdae_grad");
    if (rc) return rc;
    if (!(co > 0.0 && co <= 1.0) || step < 0) return fail(YUE_ERR_ARG, "yue_cdae_grad: needs 0 < co <= 1 and step >= 0");
    if ((rc = prepare(c, s, users, B, sample_ptr, sample_items, "yue_cdae_grad"))) return rc;
    if ((rc = forward(c, s, co, seed, step, reg, loss_out, nullptr)) || (rc = regroup(c, s, reg)) || (rc = finish(c, s))) return rc;
    // the dense gradients for tests, as k_cdae_dense forms them: the compact row (none: 0) + reg w, in float32
    const int64_t m = s->m, n = s->n, h = s->h;
    const float regf = (float)reg;
    std::vector<float> par, g;
    auto fill = [&](float *out, int v, const DevBuf<float> &compact, const std::vector<int64_t> &ids, int64_t rows, int64_t w, float r) -> int {
        if (!out) return YUE_OK;
        const int64_t count = rows * w;
        par.resize((size_t)count); g.resize((size_t)std::max<int64_t>(1, (int64_t)ids.size() * w));
        int rc2;
        if ((rc2 = download(par.data(), s->var[v], (size_t)count)) || (rc2 = download(g.data(), compact, ids.size() * (size_t)w))) return rc2;
        for (int64_t t = 0; t < count; ++t) out[t] = 0.0f;
        for (size_t k = 0; k < ids.size(); ++k)
            for (int64_t e = 0; e < w; ++e) out[ids[k] * w + e] = g[k * (size_t)w + (size_t)e];
        for (int64_t t = 0; t < count; ++t) out[t] = out[t] + r * par[(size_t)t];
        return YUE_OK;
    };
    if ((rc = fill(gU_out, vU, s->gU, s->dusers, m, h, 0.0f)) || (rc = fill(gW_out, vW, s->gWe, s->titems, n, h, regf)) ||
        (rc = fill(gbd_out, vBd, s->gBd, s->titems, n, 1, regf)) || (rc = fill(gb_out, vB, s->gB, std::vector<int64_t>{0}, 1, h, regf)))
        return rc;
    if (gWd_out) {
        std::vector<float> t((size_t)(n * h));
        if ((rc = fill(t.data(), vWd, s->gWd, s->titems, n, h, regf))) return rc;
        for (int64_t i = 0; i < n; ++i)
            for (int64_t e = 0; e < h; ++e) gWd_out[e * n + i] = t[(size_t)(i * h + e)];
    }
    return YUE_OK;
}

int yue_cdae_step(yue_ctx *c, const int32_t *users, int64_t B, const int64_t *sample_ptr, const int32_t *sample_items, double co, uint64_t seed,
                  double lr, double reg, int64_t step, double *loss_out) {
    yue_cdae *s = nullptr;
    int rc = cdae_ready(c, &s, "yue_cdae_step");
    if (rc) return rc;
    if (!(co > 0.0 && co <= 1.0) || step < 1) return fail(YUE_ERR_ARG, "yue_cdae_step: needs 0 < co <= 1 and step >= 1");
    if ((rc = prepare(c, s, users, B, sample_ptr, sample_items, "yue_cdae_step"))) return rc;
    int64_t sat = 0;
    if ((rc = forward(c, s, co, seed, step, reg, loss_out, &sat))) return rc;
    if (sat > 0) {
        if ((rc = finish(c, s))) return rc;
        return fail(YUE_ERR_SATURATED, "yue_cdae_step: " + std::to_string(sat) + " sampled outputs round to 1.0f, so that log(1 - y_pred) = -inf: the loss is inf and "
                                       "TensorFlow's gradients would be NaN; parameters and moments are left as they were");
    }
    if ((rc = regroup(c, s, reg)) || (rc = adam(c, s, lr, reg, step))) return rc;
    return finish(c, s);
}

int yue_cdae_load_factors(yue_ctx *c) {
    yue_cdae *s = nullptr;
    int rc = cdae_ready(c, &s, "yue_cdae_load_factors");
    if (rc) return rc;
    const int64_t m = s->m, n = s->n, k = s->h + 1;
    // the context's factor matrices as yue_set_factors leaves them, filled on the device
    if (c->have_inter && (m != c->m || n != c->n || k != c->k)) c->have_inter = false;
    if (k != c->k) c->opt_round_tpw = 0;
    c->have_factors = false;
    c->m = m; c->n = n; c->k = (int)k;
    HIPCHK(c->P.resize((size_t)(m * k))); HIPCHK(c->Q.resize((size_t)(n * k)));
    HIPCHK(c->dP.resize((size_t)(m * k))); HIPCHK(c->dQ.resize((size_t)(n * k)));
    HIPCHK(c->cnt0.resize((size_t)n)); HIPCHK(c->cnt1.resize((size_t)n)); HIPCHK(c->cntp0.resize((size_t)m)); HIPCHK(c->cntp1.resize((size_t)m));
    HIPCHK(hipMemsetAsync(c->dP.p, 0, (size_t)(m * k) * sizeof(float), c->stream));
    HIPCHK(hipMemsetAsync(c->dQ.p, 0, (size_t)(n * k) * sizeof(float), c->stream));
    HIPCHK(hipMemsetAsync(c->cntp0.p, 0, (size_t)m * sizeof(uint32_t), c->stream));
    HIPCHK(hipMemsetAsync(c->cntp1.p, 0, (size_t)m * sizeof(uint32_t), c->stream));
    HIPCHK(hipMemsetAsync(c->cnt0.p, 0, (size_t)n * sizeof(unsigned long long), c->stream));
    HIPCHK(hipMemsetAsync(c->cnt1.p, 0, (size_t)n * sizeof(unsigned long long), c->stream));
    // every user's uncorrupted row (a mask of ones)
    s->enc.clear();
    for (int64_t u = 0; u < m; ++u) s->enc.add(u, s->h_uptr[(size_t)u], s->h_uptr[(size_t)u + 1], c->opt_cdae_hub);
    c->cdae_hubs = (int64_t)s->enc.hub_seg.size(); c->cdae_parts = s->enc.partials;
    s->pk.h.clear();
    s->a_enc = pack_parts(s->pk, s->enc);
    HIPCHK(hipStreamSynchronize(c->stream));
    if ((rc = upload(s->idx, s->pk.h.data(), (int64_t)s->pk.h.size()))) return rc;
    HIPCHK(s->partial.resize(std::max<size_t>(1, (size_t)(s->enc.partials * s->h))));
    if ((rc = stamp(c, s, kEncode))) return rc;
    yue::CdaeEncArgs ea{};
    ea.P = dev_parts(s, s->a_enc); ea.off = s->idx.p + s->a_enc.off;
    ea.uptr = s->uptr.p; ea.uitems = s->uitems.p; ea.ucnt = s->ucnt.p;
    ea.W = s->var[vW].p; ea.b = s->var[vB].p; ea.U = s->var[vU].p; ea.h = s->h;
    ea.hid = c->P.p; ea.ld = k;
    if ((rc = launch_enc(c, ea))) return rc;
    hipLaunchKernelGGL(yue::k_cdae_pack_items, dim3((unsigned)((n * k + 255) / 256)), dim3(256), 0, c->stream, c->Q.p, s->var[vWd].p, s->var[vBd].p, n, s->h);
    HIPCHK(hipGetLastError());
    if ((rc = stamp(c, s, kEncode)) || (rc = finish(c, s))) return rc;
    c->have_factors = true;
    return YUE_OK;
}

int yue_cdae_times(yue_ctx *c, int64_t *ns_out) {
    if (!c || !ns_out) return fail(YUE_ERR_ARG, "yue_cdae_times: null argument");
    for (int p = 0; p < kPhases; ++p) ns_out[p] = c->cdae_ns[p];
    return YUE_OK;
}

}  // extern "C"
