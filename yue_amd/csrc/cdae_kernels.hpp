// CDAE kernels for gfx950 (reference recommender/advanced/CDAE.py): the denoising autoencoder worked as
// sparse-in / sampled-out.  Everything float32 as TensorFlow computes it; loss terms and sums of squares in double.  No atomics:
// every output row has one writer and every sum a fixed order (items ascending, slots ascending), so two runs on the same input
// give the same bits.  Wave layout as in lgcn_kernels.hpp: lane l holds elements 64 r + l (r < KR) of a row, h <= 128.
//   k_cdae_enc_parts / k_cdae_enc_combine
//                 a wave takes one part of a row (a batch slot, or a user when all users are encoded): at most `cdae_hub` of the
//                 user's (item, count) entries.  It draws the entries' kept flags (the counter hash of (seed, step, slot, item)),
//                 stores xw = kept ? count : 0 per entry and adds xw W[item] in ascending item order.  A row of one part (also
//                 one with no entry at all) goes on to the epilogue hid = sigmoid((acc + b) + U[u]); the parts of a longer row
//                 are written out and added in ascending order by one wave per such row.
//   k_cdae_dec    a wave per slot walks the slot's sampled (item) entries: logit = hid . W'^T[item] + b'[item], y_pred, the
//                 loss term (double, added in entry order) and e = dLoss / dlogit in TensorFlow's decomposition; in the same
//                 pass g_hid += e W'^T[item] while the row is in registers, then dz = (g_hid hid) (1 - hid).
//   k_cdae_seg_parts / k_cdae_seg_combine
//                 the regroupings: out[segment] = sum over the segment's entries of C[src] X[row] (and the sum of C), entries in
//                 the host's order (slots ascending).  Segments are items (C = e, X = hid: dW'^T and db'; C = xw, X = dz: dW),
//                 users (X = dz, plus reg U[u] per slot: dU) or the whole batch (X = dz: db); parts as above.
//   k_cdae_dense  one pass over a parameter: the sum of its squares (double, one partial per workgroup) and, with UPDATE, Adam
//                 with the gradient G[map[row]] + reg w (map < 0: reg w alone), so that no [n, h] gradient array is cleared or
//                 filled.  TF-1 applies Adam to every row of every variable: moments decay and rows move with a zero gradient.
#pragma once
#include "bpr_device.hpp"
#include "counter_hash.hpp"

namespace yue {

constexpr int kCdaeMaxH = 128;
constexpr uint64_t kCdaeTagMask = 0x43444145ull;     // stream tag xor-ed into the seed
constexpr float kCdaeClamp = 1e-6f;                  // tf.maximum(1e-6, y_pred)

// input entry (slot, item) of `step` is kept when the hash's top 24 bits lie below thr = floor(co * 2^24)  (co = 1: every entry)
__host__ __device__ inline bool cdae_keep(uint64_t seed, uint64_t step, int64_t slot, int64_t item, uint32_t thr) {
    return (uint32_t)(cnet_hash(seed ^ kCdaeTagMask, step, (uint64_t)slot, (uint64_t)item, 0) >> 40) < thr;
}

__device__ __forceinline__ double cdae_wave_sum_d(double v) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) v = v + __shfl_xor(v, off, 64);
    return v;
}

__device__ __forceinline__ float cdae_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

// the parts of a set of rows / segments: part p covers entries [beg, end) of row seg[p]; out[p] < 0: the row's only part,
// else the row of `partial` it writes.  hub_seg / hub_ptr: the rows of several parts and their partial rows.
struct CdaeParts {
    const int64_t *seg, *beg, *end, *out;
    int64_t parts;
    const int64_t *hub_seg, *hub_ptr;
    int64_t H;
    float *partial, *partial_b;                      // [partial rows, h], [partial rows]
};

struct CdaeEncArgs {
    CdaeParts P;
    const int64_t *off;                              // [parts] index of an entry in xw = off + its index in the user CSR
    const int64_t *uptr;                             // user CSR: items ascending, counts
    const int32_t *uitems, *ucnt;
    const int64_t *row_user;                         // [rows] or null: row r is user r
    const float *W, *b, *U;
    int h, training;
    uint32_t thr;
    uint64_t seed, step;
    float *xw;                                       // [input entries] or null
    float *hid;                                      // [rows, ld]; with ld > h element h of a row is set to 1
    int64_t ld;
    double *usq;                                     // [rows] sum of U[u]^2, or null
};

template <int KR>
__device__ __forceinline__ void cdae_enc_epilogue(const CdaeEncArgs &a, int64_t row, int lane, const float (&acc)[KR]) {
    const int h = a.h;
    const int64_t u = a.row_user ? a.row_user[row] : row;
    double q = 0.0;
#pragma unroll
    for (int r = 0; r < KR; ++r) {
        const int el = 64 * r + lane;
        if (el < h) {
            const float uv = a.U[u * h + el];
            a.hid[row * a.ld + el] = cdae_sigmoid((acc[r] + a.b[el]) + uv);
            q += (double)uv * (double)uv;
        }
    }
    if (a.ld > h && lane == 0) a.hid[row * a.ld + h] = 1.0f;
    if (a.usq) {
        q = cdae_wave_sum_d(q);
        if (lane == 0) a.usq[row] = q;
    }
}

template <int KR>
__global__ void __launch_bounds__(256) k_cdae_enc_parts(CdaeEncArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= a.P.parts) return;
    const int h = a.h;
    const int64_t row = a.P.seg[p], b = a.P.beg[p], e = a.P.end[p];
    float acc[KR];
#pragma unroll
    for (int r = 0; r < KR; ++r) acc[r] = 0.0f;
    for (int64_t base = b; base < e; base += 64) {
        const int cnt = (int)((e - base) < 64 ? (e - base) : 64);
        int it = 0;
        float w = 0.0f;
        if (lane < cnt) {
            it = a.uitems[base + lane];
            const bool keep = !a.training || cdae_keep(a.seed, a.step, row, it, a.thr);
            w = keep ? (float)a.ucnt[base + lane] : 0.0f;
            if (a.xw) a.xw[a.off[p] + base + lane] = w;
        }
        for (int t = 0; t < cnt; ++t) {
            const float wt = rdlane(w, t);
            if (wt == 0.0f) continue;                                    // a dropped entry
            const int64_t i = __builtin_amdgcn_readlane(it, t);
#pragma unroll
            for (int r = 0; r < KR; ++r) {
                const int el = 64 * r + lane;
                acc[r] = acc[r] + wt * (el < h ? a.W[i * h + el] : 0.0f);
            }
        }
    }
    if (a.P.out[p] < 0) { cdae_enc_epilogue<KR>(a, row, lane, acc); return; }
#pragma unroll
    for (int r = 0; r < KR; ++r) {
        const int el = 64 * r + lane;
        if (el < h) a.P.partial[a.P.out[p] * h + el] = acc[r];
    }
}

template <int KR>
__global__ void __launch_bounds__(256) k_cdae_enc_combine(CdaeEncArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= a.P.H) return;
    float acc[KR];
#pragma unroll
    for (int r = 0; r < KR; ++r) acc[r] = 0.0f;
    for (int64_t p = a.P.hub_ptr[g]; p < a.P.hub_ptr[g + 1]; ++p) {
#pragma unroll
        for (int r = 0; r < KR; ++r) {
            const int el = 64 * r + lane;
            acc[r] = acc[r] + (el < a.h ? a.P.partial[p * a.h + el] : 0.0f);
        }
    }
    cdae_enc_epilogue<KR>(a, a.P.hub_seg[g], lane, acc);
}

struct CdaeDecArgs {
    const int64_t *sptr;                             // [B + 1] the batch's sampled entries by slot, items ascending and distinct
    const int64_t *sitems;
    const int64_t *ysrc;                             // [S] the entry of xw that holds y_true, or -1 (not one of the user's items)
    const float *xw, *hid, *WdT, *bd;                // hid [B, h], W'^T [n, h], b' [n]
    int64_t B;
    int h;
    float g0;                                        // 1 / (B n): the mean's share of an element
    float *logit, *ypred, *e;                        // [S]
    float *dz;                                       // [B, h]
    double *loss;                                    // [B] the slot's loss terms, added in entry order
    int32_t *sat;                                    // [B] entries with y_pred == 1
};

template <int KR>
__global__ void __launch_bounds__(256) k_cdae_dec(CdaeDecArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t s = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= a.B) return;
    const int h = a.h;
    float hv[KR], gh[KR];
#pragma unroll
    for (int r = 0; r < KR; ++r) {
        const int el = 64 * r + lane;
        hv[r] = el < h ? a.hid[s * h + el] : 0.0f;
        gh[r] = 0.0f;
    }
    double loss = 0.0;
    int sat = 0;
    const int64_t b = a.sptr[s], e = a.sptr[s + 1];
    for (int64_t base = b; base < e; base += 64) {
        const int cnt = (int)((e - base) < 64 ? (e - base) : 64);
        int it = 0;
        float yt = 0.0f, bias = 0.0f;
        if (lane < cnt) {
            it = (int)a.sitems[base + lane];
            const int64_t src = a.ysrc[base + lane];
            yt = src >= 0 ? a.xw[src] : 0.0f;
            bias = a.bd[it];
        }
        float my_logit = 0.0f, my_pred = 0.0f, my_e = 0.0f;
        for (int t = 0; t < cnt; ++t) {
            const int64_t i = __builtin_amdgcn_readlane(it, t);
            const float y = rdlane(yt, t), bi = rdlane(bias, t);
            float wr[KR], d = 0.0f;
#pragma unroll
            for (int r = 0; r < KR; ++r) {
                const int el = 64 * r + lane;
                wr[r] = el < h ? a.WdT[i * h + el] : 0.0f;
                d = __builtin_fmaf(hv[r], wr[r], d);
            }
            const float logit = wave_sum(d) + bi;
            const float dec = cdae_sigmoid(logit);
            const float pr = fmaxf(kCdaeClamp, dec);
            float ev = 0.0f;
            if (pr == 1.0f) {
                ++sat;                                                   // log(1 - y_pred) = -inf: the call reports the loss as inf
            } else {
                const double pd = (double)pr, yd = (double)y;
                loss += -yd * log(pd) - (1.0 - yd) * log(1.0 - pd);
                if (dec > kCdaeClamp) {                                  // tf.maximum passes the gradient to the larger argument
                    const float gp = ((-a.g0) * y) * (1.0f / pr) + (a.g0 * (1.0f - y)) * (1.0f / (1.0f - pr));
                    ev = (gp * dec) * (1.0f - dec);
                }
            }
#pragma unroll
            for (int r = 0; r < KR; ++r) gh[r] = gh[r] + ev * wr[r];
            if (lane == t) { my_logit = logit; my_pred = pr; my_e = ev; }
        }
        if (lane < cnt) { a.logit[base + lane] = my_logit; a.ypred[base + lane] = my_pred; a.e[base + lane] = my_e; }
    }
#pragma unroll
    for (int r = 0; r < KR; ++r) {
        const int el = 64 * r + lane;
        if (el < h) a.dz[s * h + el] = (gh[r] * hv[r]) * (1.0f - hv[r]);
    }
    if (lane == 0) { a.loss[s] = loss; a.sat[s] = sat; }
}

struct CdaeSegArgs {
    CdaeParts P;
    const int64_t *src, *row;                        // [entries] index into C, row of X
    const float *C;                                  // coefficients, or null: 1
    const float *X;                                  // [., h]
    const float *U;                                  // the user pattern: reg U[seg_id[segment]] is added per entry; else null
    const int64_t *seg_id;
    float reg;
    int h;
    float *out, *out_b;                              // [segments, h]; [segments] the coefficients' sum, or null
};

template <int KR>
__device__ __forceinline__ void cdae_seg_store(const CdaeSegArgs &a, int64_t seg, int lane, const float (&acc)[KR], float bsum) {
#pragma unroll
    for (int r = 0; r < KR; ++r) {
        const int el = 64 * r + lane;
        if (el < a.h) a.out[seg * a.h + el] = acc[r];
    }
    if (a.out_b && lane == 0) a.out_b[seg] = bsum;
}

template <int KR>
__global__ void __launch_bounds__(256) k_cdae_seg_parts(CdaeSegArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t p = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (p >= a.P.parts) return;
    const int h = a.h;
    const int64_t seg = a.P.seg[p];
    float acc[KR], ru[KR], bsum = 0.0f;
#pragma unroll
    for (int r = 0; r < KR; ++r) {
        const int el = 64 * r + lane;
        acc[r] = 0.0f;
        ru[r] = a.U && el < h ? a.reg * a.U[a.seg_id[seg] * h + el] : 0.0f;
    }
    for (int64_t q = a.P.beg[p]; q < a.P.end[p]; ++q) {
        const float c = a.C ? a.C[a.src[q]] : 1.0f;
        bsum = bsum + c;
        if (c == 0.0f) continue;
        const int64_t x = a.row[q];
#pragma unroll
        for (int r = 0; r < KR; ++r) {
            const int el = 64 * r + lane;
            const float xv = el < h ? a.X[x * h + el] : 0.0f;
            acc[r] = a.U ? acc[r] + (xv + ru[r]) : acc[r] + c * xv;
        }
    }
    if (a.P.out[p] < 0) { cdae_seg_store<KR>(a, seg, lane, acc, bsum); return; }
#pragma unroll
    for (int r = 0; r < KR; ++r) {
        const int el = 64 * r + lane;
        if (el < h) a.P.partial[a.P.out[p] * h + el] = acc[r];
    }
    if (lane == 0) a.P.partial_b[a.P.out[p]] = bsum;
}

template <int KR>
__global__ void __launch_bounds__(256) k_cdae_seg_combine(CdaeSegArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t g = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (g >= a.P.H) return;
    float acc[KR], bsum = 0.0f;
#pragma unroll
    for (int r = 0; r < KR; ++r) acc[r] = 0.0f;
    for (int64_t p = a.P.hub_ptr[g]; p < a.P.hub_ptr[g + 1]; ++p) {
#pragma unroll
        for (int r = 0; r < KR; ++r) {
            const int el = 64 * r + lane;
            acc[r] = acc[r] + (el < a.h ? a.P.partial[p * a.h + el] : 0.0f);
        }
        bsum = bsum + a.P.partial_b[p];
    }
    cdae_seg_store<KR>(a, a.P.hub_seg[g], lane, acc, bsum);
}

// map[ids[t]] = t: the compact gradient row of an item / a user of this batch (the host clears the map to -1 first)
__global__ void __launch_bounds__(256) k_cdae_map(int32_t *map, const int64_t *ids, int64_t T) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < T) map[ids[t]] = (int32_t)t;
}

struct CdaeDenseArgs {
    float *var, *m, *v;
    int64_t count;                                   // elements; rows of `w`
    int w;
    const int32_t *map;                              // [rows] compact row of G, -1: none; null: G is dense
    const float *G;
    float reg, lr_t, beta1, beta2, eps;
    double *partial;                                 // [workgroups] sum of var^2 before the update, or null
};

template <bool UPDATE>
__global__ void __launch_bounds__(256) k_cdae_dense(CdaeDenseArgs a) {
    __shared__ double red[256];
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    double q = 0.0;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < a.count; t += stride) {
        const float x = a.var[t];
        q += (double)x * (double)x;
        if (UPDATE) {
            float g = 0.0f;
            if (a.map) {
                const int64_t row = t / a.w;
                const int32_t cr = a.map[row];
                if (cr >= 0) g = a.G[(int64_t)cr * a.w + (t - row * a.w)];
            } else {
                g = a.G[t];
            }
            g = g + a.reg * x;
            const float m1 = a.beta1 * a.m[t] + (1.0f - a.beta1) * g;
            const float v1 = a.beta2 * a.v[t] + ((1.0f - a.beta2) * g) * g;
            a.m[t] = m1; a.v[t] = v1;
            a.var[t] = x - a.lr_t * m1 / (__builtin_sqrtf(v1) + a.eps);
        }
    }
    if (!a.partial) return;
    red[threadIdx.x] = q;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) a.partial[blockIdx.x] = red[0];
}

// Q[i] = [W'^T[i] | b'[i]]: the item factors of the ranking scan, width h + 1
__global__ void __launch_bounds__(256) k_cdae_pack_items(float *Q, const float *WdT, const float *bd, int64_t n, int h) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * (h + 1)) return;
    const int64_t i = t / (h + 1);
    const int el = (int)(t - i * (h + 1));
    Q[t] = el < h ? WdT[i * h + el] : bd[i];
}

}  // namespace yue
