// libyue_hip.so -- Song2vec's iteration (recommender/advanced/Song2vec.py:162-189): the rating steps and the similarity
// pairs with their dependency schedules (include/yue_hip.h).  Kernels: s2v_kernels.hpp.  The factors are the context's
// P (X, users) and Q (Y, items = tracks); the embedding and the similar tracks come from yue_cnet_* (cnet_host.hip).
#include "host_common.hpp"

#include "s2v_kernels.hpp"

#include <numeric>

using yue_host::fail;
using yue_host::upload;

namespace {

// steps (pairs) in level order; levels are built once and serve every iteration: no step is sampled
struct Schedule {
    int64_t count = 0, levels = 0;
    std::vector<int64_t> level_ptr;
    DevBuf<int32_t> a, b, order;
};

}  // namespace

struct yue_s2v {
    int64_t m = 0, n = 0;                // sizes the state, the steps and the pairs were checked against
    bool have_state = false;
    DevBuf<double> Bu, Bi, bu0, err2;
    Schedule steps, pairs;
    DevBuf<int32_t> cnt;
    DevBuf<float> sim32;
    Event ev[2];
};

namespace {

// the state for an entry point that takes the context's factors as X and Y
int s2v_state(yue_ctx *c, yue_s2v **out, const char *who) {
    if (!c->have_factors) return fail(YUE_ERR_ARG, std::string(who) + ": call yue_set_factors first (X, Y)");
    if (c->k > yue::kS2vMaxK) return fail(YUE_ERR_ARG, std::string(who) + ": needs k <= 128");
    yue_s2v *s = nullptr;
    const int rc = yue_host::state(c, c->s2v, &s);
    if (rc) return rc;
    if (s->m != c->m || s->n != c->n) {          // other factors: nothing uploaded for the old shape survives
        s->m = c->m; s->n = c->n;
        s->have_state = false; s->steps.count = 0; s->steps.levels = 0; s->pairs.count = 0; s->pairs.levels = 0;
    }
    *out = s;
    return YUE_OK;
}

// level(step) = 1 + max(level of the previous step with the same a, ... with the same b); `shared`: a and b name rows of
// ONE matrix (tracks), so a step depends on the previous step that touched either row in either place
int build_schedule(Schedule &s, const int32_t *a, const int32_t *b, int64_t count, int64_t na, int64_t nb, bool shared) {
    std::vector<int32_t> last_a((size_t)na, 0), last_b_own;
    if (!shared) last_b_own.assign((size_t)nb, 0);
    std::vector<int32_t> &last_b = shared ? last_a : last_b_own;
    std::vector<int32_t> level((size_t)count);
    int32_t levels = 0;
    for (int64_t t = 0; t < count; ++t) {
        const int32_t l = 1 + std::max(last_a[(size_t)a[t]], last_b[(size_t)b[t]]);
        last_a[(size_t)a[t]] = l; last_b[(size_t)b[t]] = l;
        level[(size_t)t] = l;
        levels = std::max(levels, l);
    }
    s.level_ptr.assign((size_t)levels + 1, 0);
    for (int64_t t = 0; t < count; ++t) s.level_ptr[(size_t)level[(size_t)t]]++;
    for (int32_t l = 0; l < levels; ++l) s.level_ptr[(size_t)l + 1] += s.level_ptr[(size_t)l];
    std::vector<int32_t> order((size_t)count);
    std::vector<int64_t> at(s.level_ptr.begin(), s.level_ptr.end());
    for (int64_t t = 0; t < count; ++t) order[(size_t)at[(size_t)level[(size_t)t] - 1]++] = (int32_t)t;
    int rc;
    if ((rc = upload(s.a, a, count)) || (rc = upload(s.b, b, count)) || (rc = upload(s.order, order.data(), count))) return rc;
    s.count = count; s.levels = levels;
    return YUE_OK;
}

template <bool PAIRS>
int run_pass(yue_ctx *c, const Schedule &sch, yue::S2vArgs a) {
    if (sch.count == 0) return YUE_OK;
    a.order = sch.order.p;
    if (c->opt_s2v_schedule == 0) {
        a.begin = 0; a.count = sch.count;
        yue_host::with_kr(c->k, [&](auto kr) {
            constexpr int KR = kr() > 2 ? 2 : kr();
            hipLaunchKernelGGL((yue::k_s2v_seq<KR, PAIRS>), dim3(1), dim3(64), 0, c->stream, a);
        });
    } else {
        for (int64_t l = 0; l < sch.levels; ++l) {
            a.begin = sch.level_ptr[(size_t)l]; a.count = sch.level_ptr[(size_t)l + 1] - a.begin;
            const unsigned blocks = (unsigned)((a.count + yue::kS2vWaves - 1) / yue::kS2vWaves);
            yue_host::with_kr(c->k, [&](auto kr) {
                constexpr int KR = kr() > 2 ? 2 : kr();
                hipLaunchKernelGGL((yue::k_s2v_level<KR, PAIRS>), dim3(blocks), dim3(64 * yue::kS2vWaves), 0, c->stream, a);
            });
        }
    }
    HIPCHK(hipGetLastError());
    return YUE_OK;
}

}  // namespace

namespace yue_host {

// which: 0 the rating steps' levels, 1 the similarity pairs'
int64_t s2v_levels(const yue_ctx *c, int which) { return !c->s2v ? 0 : which == 0 ? c->s2v->steps.levels : c->s2v->pairs.levels; }

}  // namespace yue_host

extern "C" {

int yue_s2v_set_state(yue_ctx *c, const double *Bu, const double *Bi) {
    if (!c || !Bu || !Bi) return fail(YUE_ERR_ARG, "yue_s2v_set_state: null argument");
    yue_s2v *s = nullptr;
    int rc = s2v_state(c, &s, "yue_s2v_set_state");
    if (rc) return rc;
    HIPCHK(hipSetDevice(c->device));
    s->have_state = false;
    if ((rc = upload(s->Bu, Bu, s->m)) || (rc = upload(s->Bi, Bi, s->n))) return rc;
    HIPCHK(s->bu0.resize((size_t)s->m));
    s->have_state = true;
    return YUE_OK;
}

int yue_s2v_get_state(yue_ctx *c, double *Bu, double *Bi) {
    if (!c) return fail(YUE_ERR_ARG, "yue_s2v_get_state: null context");
    yue_s2v *s = c->s2v.get();
    if (!s || !s->have_state || s->m != c->m || s->n != c->n) return fail(YUE_ERR_ARG, "yue_s2v_get_state: call yue_s2v_set_state first");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (Bu) HIPCHK(hipMemcpy(Bu, s->Bu.p, (size_t)s->m * sizeof(double), hipMemcpyDeviceToHost));
    if (Bi) HIPCHK(hipMemcpy(Bi, s->Bi.p, (size_t)s->n * sizeof(double), hipMemcpyDeviceToHost));
    return YUE_OK;
}

int yue_s2v_set_steps(yue_ctx *c, const int32_t *u, const int32_t *i, const int32_t *count, int64_t T) {
    if (!c || T < 0 || T >= INT32_MAX || (T > 0 && (!u || !i || !count))) return fail(YUE_ERR_ARG, "yue_s2v_set_steps: need 0 <= T < 2^31 - 1 and the three arrays");
    yue_s2v *s = nullptr;
    int rc = s2v_state(c, &s, "yue_s2v_set_steps");
    if (rc) return rc;
    std::vector<char> seen((size_t)s->m, 0);
    for (int64_t t = 0; t < T; ++t) {
        if (u[t] < 0 || u[t] >= s->m || i[t] < 0 || i[t] >= s->n) return fail(YUE_ERR_ARG, "yue_s2v_set_steps: id out of range at step " + std::to_string(t));
        if (t == 0 || u[t] != u[t - 1]) {
            if (seen[(size_t)u[t]])
                return fail(YUE_ERR_ARG, "yue_s2v_set_steps: the steps of user " + std::to_string(u[t]) + " are not contiguous (the stale bias is read once per user)");
            seen[(size_t)u[t]] = 1;
        }
    }
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    s->steps.count = 0; s->steps.levels = 0;
    if ((rc = upload(s->cnt, count, T))) return rc;
    return build_schedule(s->steps, u, i, T, s->m, s->n, false);
}

int yue_s2v_set_pairs(yue_ctx *c, const int32_t *t1, const int32_t *t2, const double *sim, int64_t Pn) {
    if (!c || Pn < 0 || Pn >= INT32_MAX || (Pn > 0 && (!t1 || !t2 || !sim))) return fail(YUE_ERR_ARG, "yue_s2v_set_pairs: need 0 <= Pn < 2^31 - 1 and the three arrays");
    yue_s2v *s = nullptr;
    int rc = s2v_state(c, &s, "yue_s2v_set_pairs");
    if (rc) return rc;
    std::vector<float> sim32((size_t)Pn);
    for (int64_t p = 0; p < Pn; ++p) {
        if (t1[p] < 0 || t1[p] >= s->n || t2[p] < 0 || t2[p] >= s->n) return fail(YUE_ERR_ARG, "yue_s2v_set_pairs: track id out of range at pair " + std::to_string(p));
        if (t1[p] == t2[p]) return fail(YUE_ERR_ARG, "yue_s2v_set_pairs: a track paired with itself at pair " + std::to_string(p));
        sim32[(size_t)p] = (float)sim[p];          // the Python float meets a float32 dot: NumPy rounds it to float32 first
    }
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    s->pairs.count = 0; s->pairs.levels = 0;
    if ((rc = upload(s->sim32, sim32.data(), Pn))) return rc;
    return build_schedule(s->pairs, t1, t2, Pn, s->n, s->n, true);
}

int yue_s2v_epoch(yue_ctx *c, double lr, double regU, double regI, double regB, double alpha, double globalMean, double *err2_steps,
                  double *err2_pairs) {
    if (!c) return fail(YUE_ERR_ARG, "yue_s2v_epoch: null context");
    yue_s2v *s = nullptr;
    int rc = s2v_state(c, &s, "yue_s2v_epoch");
    if (rc) return rc;
    if (!s->have_state) return fail(YUE_ERR_ARG, "yue_s2v_epoch: call yue_s2v_set_state first");
    HIPCHK(hipSetDevice(c->device));
    const int64_t T = s->steps.count, Pn = s->pairs.count;
    HIPCHK(s->err2.resize((size_t)std::max<int64_t>(T + Pn, 1)));
    yue::S2vArgs a{};
    a.X = c->P.p; a.Y = c->Q.p; a.Bu = s->Bu.p; a.Bi = s->Bi.p; a.bu0 = s->bu0.p; a.k = c->k;
    a.su = s->steps.a.p; a.si = s->steps.b.p; a.cnt = s->cnt.p;
    a.t1 = s->pairs.a.p; a.t2 = s->pairs.b.p; a.sim32 = s->sim32.p;
    a.lr = lr; a.regB = regB; a.ru = (float)regU; a.ri = (float)regI; a.gm32 = (float)globalMean;
    a.coef32 = (float)(0.5 * alpha * lr);
    HIPCHK(s->ev[0].record(c->stream));
    HIPCHK(hipMemcpyAsync(s->bu0.p, s->Bu.p, (size_t)s->m * sizeof(double), hipMemcpyDeviceToDevice, c->stream));
    a.err2 = s->err2.p;
    if ((rc = run_pass<false>(c, s->steps, a))) return rc;
    a.err2 = s->err2.p + T;
    if ((rc = run_pass<true>(c, s->pairs, a))) return rc;
    HIPCHK(s->ev[1].record(c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(yue_host::elapsed(s->ev[0], s->ev[1], &c->s2v_ns));
    if (err2_steps && T > 0) HIPCHK(hipMemcpy(err2_steps, s->err2.p, (size_t)T * sizeof(double), hipMemcpyDeviceToHost));
    if (err2_pairs && Pn > 0) HIPCHK(hipMemcpy(err2_pairs, s->err2.p + T, (size_t)Pn * sizeof(double), hipMemcpyDeviceToHost));
    return YUE_OK;
}

}  // extern "C"
