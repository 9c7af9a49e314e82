// LightGCN kernels for gfx950 (reference recommender/advanced/LightGCN.py): the sparse-times-dense
// propagation over the (m + n)-row user-item graph with its fused epilogues, forward and backward, and the minibatch's
// loss / dF.  NGCF (ngcf_kernels.hpp) runs its products and its minibatch through the same kernels; the
// host side of both is gcn_host.hpp.  Everything float32 as TensorFlow computes it; loss partials in double.  No atomics:
// every output row has one writer and every sum a fixed order, so two runs on the same input give the same bits.
//
// Wave layout as in train_kernels.hpp: lane l holds elements 64*r + l (r < KR) of a row, k <= 128.
//   k_lgcn_rows   a wave takes `rpw` consecutive rows (many where the mean degree is small); per row it loads 64
//                 (neighbour, weight) pairs with one coalesced load, hands them out by readlane, keeps four neighbour rows in
//                 flight on four accumulators ((a0 + a1) + (a2 + a3) at the end), then runs the epilogue.  Rows above the hub
//                 threshold are left to:
//   k_lgcn_hub_parts / k_lgcn_hub_combine   a hub's neighbour list is cut into parts of `threshold` neighbours, one wave per
//                 part writes a partial row; one wave per hub adds the parts in ascending order and runs the epilogue.
// Epilogues (MODE):
//   kFwd   Y[row] = acc; ss[row] = sum acc^2; F[row] += acc * (1 / sqrt(max(ss, 1e-12)))              (LightGCN.py:40-45)
//   kBwd   out[row] = J(G[row]) + acc, J(g) = (g - nh (nh . g)) * rinv with nh = E[row] * rinv where ss >= 1e-12, g * 1e6 elsewhere
//          (the derivative of x * rsqrt(max(sum x^2, 1e-12))); `gather` = 0 for the last layer, which has no A . gE term
//   kPlain out[row] = (base ? base[row] : 0) + acc, rows below m to outU, the others to outV (out may be base).  LightGCN's
//          last backward product: base = G into the two gradient buffers; NGCF's S = A E (no base), its A^T gS added onto the
//          local part in place, and its last one into the two gradient buffers
#pragma once
#include "bpr_device.hpp"

namespace yue {

constexpr int kLgcnMaxK = 128;
constexpr float kLgcnEps = 1e-12f;                   // tf.nn.l2_normalize's epsilon

enum { kLgcnFwd = 0, kLgcnBwd = 1, kLgcnPlain = 2 };

struct LgcnArgs {
    const int64_t *ptr;                              // [N + 1] CSR of the graph (LightGCN: symmetric), N = m + n
    const int32_t *col;
    const float *w;
    const float *X;                                  // [N, k] the gathered matrix (E_{l-1} forward, gE_{l+1} backward)
    int64_t N, m;
    int k, rpw, gather;
    int64_t hub;                                     // rows with more neighbours than this are the hub kernels'
    // epilogue
    float *Y, *ss, *F;                               // kFwd: raw layer, its row sums of squares, the running sum of layers
    const float *G, *E, *ssr;                        // kBwd: dLoss / dF, the raw layer and its sums of squares
    float *out;                                      // kBwd: gE_l
    const float *base;                               // kPlain: [N, k] added to the product, or null
    float *outU, *outV;                              // kPlain: rows below m, the other rows (each from its first row)
    // hubs
    const int64_t *hub_row, *hub_part_ptr;           // [H] rows, [H + 1] first part of every hub
    const int64_t *part_beg, *part_end;              // [parts] neighbour ranges
    float *partial;                                  // [parts, k]
    int64_t H, parts;
};

__device__ __forceinline__ float lgcn_rdlane_f(float v, int l) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}

// acc += sum over the neighbours [b, e) of w * X[col], in the fixed order described above
template <int KR>
__device__ __forceinline__ void lgcn_gather(const LgcnArgs &a, int64_t b, int64_t e, int lane, float (&acc)[KR]) {
    const int k = a.k;
    float a0[KR], a1[KR], a2[KR], a3[KR];
#pragma unroll
    for (int r = 0; r < KR; ++r) { a0[r] = 0.0f; a1[r] = 0.0f; a2[r] = 0.0f; a3[r] = 0.0f; }
    for (int64_t base = b; base < e; base += 64) {
        const int cnt = (int)((e - base) < 64 ? (e - base) : 64);
        int cl = 0;
        float wl = 0.0f;
        if (lane < cnt) { cl = a.col[base + lane]; wl = a.w[base + lane]; }
        int t = 0;
        for (; t + 4 <= cnt; t += 4) {
            const int64_t c0 = __builtin_amdgcn_readlane(cl, t), c1 = __builtin_amdgcn_readlane(cl, t + 1);
            const int64_t c2 = __builtin_amdgcn_readlane(cl, t + 2), c3 = __builtin_amdgcn_readlane(cl, t + 3);
            const float w0 = lgcn_rdlane_f(wl, t), w1 = lgcn_rdlane_f(wl, t + 1), w2 = lgcn_rdlane_f(wl, t + 2), w3 = lgcn_rdlane_f(wl, t + 3);
            float x0[KR], x1[KR], x2[KR], x3[KR];
#pragma unroll
            for (int r = 0; r < KR; ++r) {
                const int el = 64 * r + lane;
                x0[r] = el < k ? a.X[c0 * k + el] : 0.0f;
                x1[r] = el < k ? a.X[c1 * k + el] : 0.0f;
                x2[r] = el < k ? a.X[c2 * k + el] : 0.0f;
                x3[r] = el < k ? a.X[c3 * k + el] : 0.0f;
            }
#pragma unroll
            for (int r = 0; r < KR; ++r) {
                a0[r] = __builtin_fmaf(w0, x0[r], a0[r]); a1[r] = __builtin_fmaf(w1, x1[r], a1[r]);
                a2[r] = __builtin_fmaf(w2, x2[r], a2[r]); a3[r] = __builtin_fmaf(w3, x3[r], a3[r]);
            }
        }
        for (; t < cnt; ++t) {
            const int64_t c0 = __builtin_amdgcn_readlane(cl, t);
            const float w0 = lgcn_rdlane_f(wl, t);
#pragma unroll
            for (int r = 0; r < KR; ++r) {
                const int el = 64 * r + lane;
                a0[r] = __builtin_fmaf(w0, el < k ? a.X[c0 * k + el] : 0.0f, a0[r]);
            }
        }
    }
#pragma unroll
    for (int r = 0; r < KR; ++r) acc[r] = acc[r] + ((a0[r] + a1[r]) + (a2[r] + a3[r]));
}

template <int KR, int MODE>
__device__ __forceinline__ void lgcn_epilogue(const LgcnArgs &a, int64_t row, int lane, const float (&acc)[KR]) {
    const int k = a.k;
    if (MODE == kLgcnFwd) {
        float q = 0.0f;
#pragma unroll
        for (int r = 0; r < KR; ++r) q = __builtin_fmaf(acc[r], acc[r], q);      // (lanes past k hold 0)
        const float ss = wave_sum(q);
        const float rinv = 1.0f / __builtin_sqrtf(fmaxf(ss, kLgcnEps));
        if (lane == 0) a.ss[row] = ss;
#pragma unroll
        for (int r = 0; r < KR; ++r) {
            const int el = 64 * r + lane;
            if (el < k) { a.Y[row * k + el] = acc[r]; a.F[row * k + el] = a.F[row * k + el] + acc[r] * rinv; }
        }
    } else if (MODE == kLgcnBwd) {
        float g[KR];
        bool any = false;
#pragma unroll
        for (int r = 0; r < KR; ++r) {
            const int el = 64 * r + lane;
            g[r] = el < k ? a.G[row * k + el] : 0.0f;
            any = any || g[r] != 0.0f;
        }
        float j[KR];
#pragma unroll
        for (int r = 0; r < KR; ++r) j[r] = 0.0f;
        if (__builtin_amdgcn_ballot_w64(any) != 0) {                 // (most rows of a step hold no dLoss / dF: E is not read)
            const float ss = a.ssr[row];
            if (ss >= kLgcnEps) {
                const float rinv = 1.0f / __builtin_sqrtf(ss);
                float nh[KR], d = 0.0f;
#pragma unroll
                for (int r = 0; r < KR; ++r) {
                    const int el = 64 * r + lane;
                    nh[r] = (el < k ? a.E[row * k + el] : 0.0f) * rinv;
                    d = __builtin_fmaf(nh[r], g[r], d);
                }
                const float dot = wave_sum(d);
#pragma unroll
                for (int r = 0; r < KR; ++r) j[r] = (g[r] - nh[r] * dot) * rinv;
            } else {
#pragma unroll
                for (int r = 0; r < KR; ++r) j[r] = g[r] * 1e6f;
            }
        }
#pragma unroll
        for (int r = 0; r < KR; ++r) {
            const int el = 64 * r + lane;
            if (el < k) a.out[row * k + el] = j[r] + acc[r];
        }
    } else {
        float *dst = row < a.m ? a.outU + row * k : a.outV + (row - a.m) * k;
#pragma unroll
        for (int r = 0; r < KR; ++r) {
            const int el = 64 * r + lane;
            if (el < k) dst[el] = (a.base ? a.base[row * k + el] : 0.0f) + acc[r];
        }
    }
}

template <int KR, int MODE>
__global__ void __launch_bounds__(256) k_lgcn_rows(LgcnArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t r0 = wave * a.rpw;
    const int64_t r1 = r0 + a.rpw < a.N ? r0 + a.rpw : a.N;
    for (int64_t row = r0; row < r1; ++row) {
        float acc[KR];
#pragma unroll
        for (int r = 0; r < KR; ++r) acc[r] = 0.0f;
        if (a.gather) {
            const int64_t b = a.ptr[row], e = a.ptr[row + 1];
            if (e - b > a.hub) continue;                             // k_lgcn_hub_parts / k_lgcn_hub_combine
            lgcn_gather<KR>(a, b, e, lane, acc);
        }
        lgcn_epilogue<KR, MODE>(a, row, lane, acc);
    }
}

template <int KR>
__global__ void __launch_bounds__(256) k_lgcn_hub_parts(LgcnArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= a.parts) return;
    float acc[KR];
#pragma unroll
    for (int r = 0; r < KR; ++r) acc[r] = 0.0f;
    lgcn_gather<KR>(a, a.part_beg[p], a.part_end[p], lane, acc);
#pragma unroll
    for (int r = 0; r < KR; ++r) {
        const int el = 64 * r + lane;
        if (el < a.k) a.partial[p * a.k + el] = acc[r];
    }
}

template <int KR, int MODE>
__global__ void __launch_bounds__(256) k_lgcn_hub_combine(LgcnArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t h = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (h >= a.H) return;
    float acc[KR];
#pragma unroll
    for (int r = 0; r < KR; ++r) acc[r] = 0.0f;
    for (int64_t p = a.hub_part_ptr[h]; p < a.hub_part_ptr[h + 1]; ++p) {
#pragma unroll
        for (int r = 0; r < KR; ++r) {
            const int el = 64 * r + lane;
            acc[r] = acc[r] + (el < a.k ? a.partial[p * a.k + el] : 0.0f);
        }
    }
    lgcn_epilogue<KR, MODE>(a, a.hub_row[h], lane, acc);
}

// ------------------------------------------------------------------------------------------
// The minibatch (LightGCN.py:83-88) on the gathered rows of F = [F_users; F_items].
//   k_lgcn_batch_y   one wave per triplet: y = F_u.F_i - F_u.F_j, c = d(-log sigmoid(y)) / dy = -1 / (1 + exp(y)), and
//                    the triplet's loss -log sigmoid(y) + reg (|F_u|^2 + |F_i|^2 + |F_j|^2) / 2 as a double
//   k_lgcn_batch_g   one wave per touched row of F: the host sorted the 3 T (row, triplet, role) entries by row, a row's
//                    entries in triplet order; the wave adds their terms in that order and writes G[row] (G was cleared)
//                    role 0 (u): c (F_i - F_j) + reg F_u    role 1 (i): c F_u + reg F_i    role 2 (j): -c F_u + reg F_j
// ------------------------------------------------------------------------------------------
struct LgcnBatchArgs {
    const float *F;
    float *G;
    int64_t m;
    int k;
    const int32_t *u, *i, *j;
    int64_t T, S;
    float reg;
    float *c;                                        // [T]
    double *loss;                                    // [T]
    const int64_t *seg_ptr;                          // [S + 1]
    const int64_t *seg_row;                          // [S] row of F
    const int32_t *ent;                              // [3 T] 4 * triplet + role
};

template <int KR>
__global__ void __launch_bounds__(256) k_lgcn_batch_y(LgcnBatchArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= a.T) return;
    const int k = a.k;
    const int64_t u = a.u[t], i = a.m + a.i[t], j = a.m + a.j[t];
    float di = 0.0f, dj = 0.0f, su = 0.0f, si = 0.0f, sj = 0.0f;
#pragma unroll
    for (int r = 0; r < KR; ++r) {
        const int el = 64 * r + lane;
        const float fu = el < k ? a.F[u * k + el] : 0.0f, fi = el < k ? a.F[i * k + el] : 0.0f, fj = el < k ? a.F[j * k + el] : 0.0f;
        di = __builtin_fmaf(fu, fi, di); dj = __builtin_fmaf(fu, fj, dj);
        su = __builtin_fmaf(fu, fu, su); si = __builtin_fmaf(fi, fi, si); sj = __builtin_fmaf(fj, fj, sj);
    }
    const float y = wave_sum(di) - wave_sum(dj);
    const float l2 = (wave_sum(su) + wave_sum(si)) + wave_sum(sj);
    if (lane == 0) {
        a.c[t] = -1.0f / (1.0f + expf(y));
        const double yd = (double)y;
        a.loss[t] = (fmax(-yd, 0.0) + log1p(exp(-fabs(yd)))) + (double)a.reg * (0.5 * (double)l2);
    }
}

template <int KR>
__global__ void __launch_bounds__(256) k_lgcn_batch_g(LgcnBatchArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t s = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= a.S) return;
    const int k = a.k;
    const int64_t row = a.seg_row[s];
    float acc[KR];
#pragma unroll
    for (int r = 0; r < KR; ++r) acc[r] = 0.0f;
    for (int64_t p = a.seg_ptr[s]; p < a.seg_ptr[s + 1]; ++p) {
        const int32_t en = a.ent[p];
        const int64_t t = en >> 2;
        const int role = en & 3;
        const float c = a.c[t];
        const int64_t u = a.u[t], i = a.m + a.i[t], j = a.m + a.j[t];
#pragma unroll
        for (int r = 0; r < KR; ++r) {
            const int el = 64 * r + lane;
            const float fu = el < k ? a.F[u * k + el] : 0.0f;
            float term;
            if (role == 0) {
                const float fi = el < k ? a.F[i * k + el] : 0.0f, fj = el < k ? a.F[j * k + el] : 0.0f;
                term = c * (fi - fj) + a.reg * fu;
            } else if (role == 1) {
                term = c * fu + a.reg * (el < k ? a.F[i * k + el] : 0.0f);
            } else {
                term = a.reg * (el < k ? a.F[j * k + el] : 0.0f) - c * fu;
            }
            acc[r] = acc[r] + term;
        }
    }
#pragma unroll
    for (int r = 0; r < KR; ++r) {
        const int el = 64 * r + lane;
        if (el < k) a.G[row * k + el] = acc[r];
    }
}

}  // namespace yue
