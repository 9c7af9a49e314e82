// APR kernels for gfx950 (reference recommender/advanced/APR.py): the pairwise minibatch gradient of
// BPR's live path with a perturbation D of the embeddings, in three forms that share one skeleton.  Everything float32 as
// TensorFlow computes it; loss terms in double.  No atomics: every output row has one writer and every sum a fixed order, so
// two runs on the same input give the same bits.
//
// Wave layout as in lgcn_kernels.hpp: lane l holds elements 64*r + l (r < KR) of a row, KR from with_kr, k <= 256.
//   k_apr_coef   one wave per triplet (u, i, j): x = U_u.V_i - U_u.V_j, a = -sigmoid(-x); with a perturbation also
//                x_adv = (U_u + D_u).(V_i + D_i) - (U_u + D_u).(V_j + D_j) and b = -(regA sigmoid(-x_adv)); the triplet's loss
//                terms as a double: softplus(-x) + reg (2 |U_u|^2 + |V_i|^2) / 2 (phase 1: the user rows are regularised
//                twice, the negative rows not at all, APR.py:61-67) or softplus(-x) + regA softplus(-x_adv)
//   k_apr_rows   one wave per distinct row of the batch, users first, then items.  The host sorted every row's (triplet, role)
//                entries by a stable counting sort, triplets ascending, the positive role before the negative one; the wave adds
//                their terms in that order and writes the row once with plain stores.  FORM:
//     kAprPre    user: (a V_i - a V_j) + 2 reg U_u; positive: a U_u + reg V_i; negative: -(a U_u)             -> gU / gV rows
//     kAprDelta  user: b Y_i - b Y_j; positive: b W_u; negative: -(b W_u), with W = U + D, Y = V + D at the OLD D.  The
//                epilogue is the normalisation: raw row out, ss = sum g^2 by a wave sum, D_new = (g * (1 / sqrt(max(ss, 1e-12))))
//                * eps (tf.nn.l2_normalize(g, 1) * eps: a zero row stays exactly 0)
//     kAprAdv    user: (a V_i - a V_j) + (b Y_i - b Y_j); positive: a U_u + b W_u; negative: its negation    -> gU / gV rows
// The perturbation is compact: dU / dV hold one row per distinct row of the batch that set them; a triplet finds its three
// rows through xu / xi / xj (-1: the row's perturbation is 0).
#pragma once
#include "bpr_device.hpp"

namespace yue {

constexpr int kAprMaxK = 256;
constexpr float kAprEps = 1e-12f;                    // tf.nn.l2_normalize's epsilon

enum { kAprPre = 0, kAprDelta = 1, kAprAdv = 2 };

struct AprArgs {
    const float *U, *V;
    int k;
    const int32_t *u, *i, *j;                        // [T]
    int64_t T;
    const float *dU, *dV;                            // the perturbation rows this launch reads (null: none, k_apr_coef only)
    const int32_t *xu, *xi, *xj;                     // [T] each triplet's rows in dU / dV, -1: zero
    float reg, regA, eps;
    float *a, *b;                                    // [T] coefficients
    double *loss;                                    // [T]
    // rows
    int64_t Du, Di;                                  // distinct users / items of the batch
    const int32_t *row_id;                           // [Du + Di] user ids ascending, then item ids ascending
    const int32_t *seg_ptr;                          // [Du + Di + 1] into ent
    const int32_t *ent;                              // [3 T] user rows: triplet; item rows: 2 * triplet + role (0 positive, 1 negative)
    float *gU, *gV;                                  // kAprPre / kAprAdv: [m, k] / [n, k], the batch's rows are written
    float *raw, *nU, *nV;                            // kAprDelta: raw gradient [Du + Di, k], the new perturbation [Du, k] / [Di, k]
};

__device__ __forceinline__ float apr_at(const float *base, int64_t row, int k, int el) { return el < k ? base[row * k + el] : 0.0f; }

template <int KR>
__global__ void __launch_bounds__(256) k_apr_coef(AprArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= a.T) return;
    const int k = a.k;
    const int64_t u = a.u[t], i = a.i[t], j = a.j[t];
    const bool adv = a.dU != nullptr;
    const int xu = adv ? a.xu[t] : -1, xi = adv ? a.xi[t] : -1, xj = adv ? a.xj[t] : -1;
    float di = 0.0f, dj = 0.0f, su = 0.0f, si = 0.0f, ei = 0.0f, ej = 0.0f;
#pragma unroll
    for (int r = 0; r < KR; ++r) {
        const int el = 64 * r + lane;
        const float pu = apr_at(a.U, u, k, el), vi = apr_at(a.V, i, k, el), vj = apr_at(a.V, j, k, el);
        di = __builtin_fmaf(pu, vi, di); dj = __builtin_fmaf(pu, vj, dj);
        su = __builtin_fmaf(pu, pu, su); si = __builtin_fmaf(vi, vi, si);
        if (adv) {
            const float w = xu >= 0 ? pu + apr_at(a.dU, xu, k, el) : pu;
            const float yi = xi >= 0 ? vi + apr_at(a.dV, xi, k, el) : vi, yj = xj >= 0 ? vj + apr_at(a.dV, xj, k, el) : vj;
            ei = __builtin_fmaf(w, yi, ei); ej = __builtin_fmaf(w, yj, ej);
        }
    }
    const float x = wave_sum(di) - wave_sum(dj);
    const float l2 = 2.0f * wave_sum(su) + wave_sum(si);
    const float xa = adv ? wave_sum(ei) - wave_sum(ej) : 0.0f;
    if (lane == 0) {
        a.a[t] = -1.0f / (1.0f + expf(x));
        const double xd = (double)x;
        double loss = fmax(-xd, 0.0) + log1p(exp(-fabs(xd)));
        if (adv) {
            a.b[t] = -(a.regA * (1.0f / (1.0f + expf(xa))));
            const double xad = (double)xa;
            loss += (double)a.regA * (fmax(-xad, 0.0) + log1p(exp(-fabs(xad))));
        } else {
            loss += (double)a.reg * (0.5 * (double)l2);
        }
        a.loss[t] = loss;
    }
}

template <int KR, int FORM>
__global__ void __launch_bounds__(256) k_apr_rows(AprArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t s = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= a.Du + a.Di) return;
    const int k = a.k;
    const bool user = s < a.Du;
    const int64_t row = a.row_id[s];
    float self[KR], acc[KR];
#pragma unroll
    for (int r = 0; r < KR; ++r) { self[r] = FORM == kAprPre ? apr_at(user ? a.U : a.V, row, k, 64 * r + lane) : 0.0f; acc[r] = 0.0f; }
    const float reg2 = 2.0f * a.reg;
    for (int p = a.seg_ptr[s]; p < a.seg_ptr[s + 1]; ++p) {
        const int32_t en = a.ent[p];
        if (user) {
            const int64_t t = en, i = a.i[t], j = a.j[t];
            const float ca = FORM == kAprDelta ? 0.0f : a.a[t], cb = FORM == kAprPre ? 0.0f : a.b[t];
            const int xi = FORM == kAprPre ? -1 : a.xi[t], xj = FORM == kAprPre ? -1 : a.xj[t];
#pragma unroll
            for (int r = 0; r < KR; ++r) {
                const int el = 64 * r + lane;
                const float vi = apr_at(a.V, i, k, el), vj = apr_at(a.V, j, k, el);
                float term;
                if (FORM == kAprPre) {
                    term = (ca * vi - ca * vj) + reg2 * self[r];
                } else {
                    const float yi = xi >= 0 ? vi + apr_at(a.dV, xi, k, el) : vi, yj = xj >= 0 ? vj + apr_at(a.dV, xj, k, el) : vj;
                    const float pert = cb * yi - cb * yj;
                    term = FORM == kAprDelta ? pert : (ca * vi - ca * vj) + pert;
                }
                acc[r] = acc[r] + term;
            }
        } else {
            const int64_t t = en >> 1, u = a.u[t];
            const bool neg = en & 1;
            const float ca = FORM == kAprDelta ? 0.0f : a.a[t], cb = FORM == kAprPre ? 0.0f : a.b[t];
            const int xu = FORM == kAprPre ? -1 : a.xu[t];
#pragma unroll
            for (int r = 0; r < KR; ++r) {
                const int el = 64 * r + lane;
                const float pu = apr_at(a.U, u, k, el);
                float term;
                if (FORM == kAprPre) {
                    term = neg ? -(ca * pu) : ca * pu + a.reg * self[r];
                } else {
                    const float w = xu >= 0 ? pu + apr_at(a.dU, xu, k, el) : pu;
                    const float v = FORM == kAprDelta ? cb * w : ca * pu + cb * w;
                    term = neg ? -v : v;
                }
                acc[r] = acc[r] + term;
            }
        }
    }
    if (FORM == kAprDelta) {
        float q = 0.0f;
#pragma unroll
        for (int r = 0; r < KR; ++r) q = __builtin_fmaf(acc[r], acc[r], q);          // (lanes past k hold 0)
        const float rinv = 1.0f / __builtin_sqrtf(fmaxf(wave_sum(q), kAprEps));
        float *dst = user ? a.nU + s * k : a.nV + (s - a.Du) * k;
#pragma unroll
        for (int r = 0; r < KR; ++r) {
            const int el = 64 * r + lane;
            if (el < k) { a.raw[s * k + el] = acc[r]; dst[el] = (acc[r] * rinv) * a.eps; }
        }
    } else {
        float *dst = user ? a.gU + row * k : a.gV + row * k;
#pragma unroll
        for (int r = 0; r < KR; ++r) {
            const int el = 64 * r + lane;
            if (el < k) dst[el] = acc[r];
        }
    }
}

}  // namespace yue
