// NGCF kernels for gfx950 (reference recommender/advanced/NGCF.py).  The sparse-times-dense products
// and the minibatch are lgcn_kernels.hpp's (k_lgcn_rows / k_lgcn_hub_parts / k_lgcn_hub_combine with the plain epilogue,
// k_lgcn_batch_y / k_lgcn_batch_g at width (layers + 1) k), launched through gcn_host.hpp; here is the dense half of a layer
// on v_mfma_f32_32x32x2_f32, forward and backward, and the weight gradients.  Everything float32; no atomics: every output
// element has one writer and every sum a fixed order, so two runs on the same input give the same bits.
//
//   k_ngcf_layer_fwd  a workgroup takes 32 rows: [S + E | E o S] (32 x 2 KP, KP = k rounded up to 32, zero padded) in LDS times
//                     [W_1; W_2] from global memory.  Z[row][c] is ONE chain of fused multiply-adds from 0: j = 0 .. k-1 over
//                     (S + E)[j] W_1[j][c], then j = 0 .. k-1 over (E o S)[j] W_2[j][c]  (the padded terms add 0 * 0).
//                     Epilogue: H = Z > 0 ? Z : 0.2 Z; D = training ? (kept ? H / keep : 0) : H; then, a wave per 8 rows,
//                     ss = sum D^2 and F's block = D * (1 / sqrt(max(ss, 1e-12))).
//   k_ngcf_layer_bwd  gD = gD_in + J(G block) (J: the derivative of l2_normalize, as lgcn_kernels.hpp's), gZ = gD * mask / keep *
//                     (Z > 0 ? 1 : 0.2) to LDS and global; gX1 = gZ W_1^T and gX2 = gZ W_2^T on the MFMA (chains over the
//                     output index j ascending); gS = gX1 + E o gX2 and the local part gX1 + S o gX2 (+ G's block 0 for the
//                     first layer) are written; the A^T gather then adds its part.
//   k_ngcf_wgrad      [S + E | E o S]^T gZ over a chunk of kNgcfWChunk rows, staged 32 rows at a time in LDS: 32 x 32 blocks of the
//                     2k x k result shared by the four waves, each a chain over the chunk's rows ascending; k_ngcf_wsum adds the chunks' partials in ascending order.
// The dropout mask is a pure function of (seed, step, layer, row, column): ngcf_keep, computed alike on host and device,
// recomputed in the backward pass and never stored.
#pragma once
#include "counter_hash.hpp"
#include "lgcn_kernels.hpp"

namespace yue {

constexpr int kNgcfMaxK = 128;
constexpr int kNgcfMaxWidth = 256;                   // (layers + 1) k: the minibatch kernels' KR = 4, and the scan's limit
constexpr int kNgcfTile = 32;
constexpr int kNgcfWChunk = 512;                     // rows per weight-gradient partial: a constant, so that no device changes the sums' order
constexpr float kNgcfSlope = 0.2f;                   // tf.nn.leaky_relu's default alpha
constexpr uint64_t kNgcfTagMask = 0x4E474346ull;     // stream tag xor-ed into the seed

// an element is kept when the hash's top 24 bits lie below thr = floor(keep * 2^24)  (keep = 1: every element)
__host__ __device__ inline bool ngcf_keep(uint64_t seed, uint64_t step, int layer, int64_t row, int col, uint32_t thr) {
    return (uint32_t)(cnet_hash(seed ^ kNgcfTagMask, step, (uint64_t)layer, (uint64_t)row, (uint64_t)col) >> 40) < thr;
}

typedef float ngcf_f32x16 __attribute__((ext_vector_type(16)));

// ---- the dense half of a layer ------------------------------------------------------------------------------------------
struct NgcfLayerArgs {
    const float *E, *S;                              // [N, k] the layer's input E_{l-1} and S = A E_{l-1}
    const float *W;                                  // [2][k][k] W_1 then W_2, input index major
    int64_t N;
    int k, ldF, layer, training;                     // ldF = (layers + 1) k: the row stride of F and G
    float keep;
    uint32_t thr;
    uint64_t seed, step;
    // forward
    float *Z, *D, *ss, *F;                           // [N, k], [N, k], [N]; F's block of this layer (row stride ldF)
    // backward
    const float *Zr, *Dr, *ssr;                      // what the forward pass kept
    const float *gD_in;                              // [N, k] gradient at E_l from the layer above (null for the last layer)
    const float *G, *G0;                             // dLoss / dF: this layer's block; block 0 for the first layer (else null)
    float *gZ, *gS, *loc;                            // [N, k] each; loc may alias gD_in (a tile reads its rows before it writes them)
};

__device__ __forceinline__ int ngcf_kp(int k) { return (k + 31) & ~31; }

__global__ void __launch_bounds__(256) k_ngcf_layer_fwd(NgcfLayerArgs a) {
    extern __shared__ __attribute__((aligned(16))) float ngcf_lds[];
    const int k = a.k, KP = ngcf_kp(k), ldx = 2 * KP + 1, ldd = KP + 1;
    float *X = ngcf_lds, *Dt = X + kNgcfTile * ldx;
    const int tid = (int)threadIdx.x, w = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int64_t row0 = (int64_t)blockIdx.x * kNgcfTile;
    for (int e = tid; e < kNgcfTile * KP; e += 256) {
        const int rr = e / KP, col = e - rr * KP;
        const int64_t row = row0 + rr;
        float ev = 0.0f, sv = 0.0f;
        if (row < a.N && col < k) { ev = a.E[row * k + col]; sv = a.S[row * k + col]; }
        X[rr * ldx + col] = sv + ev;
        X[rr * ldx + KP + col] = ev * sv;
    }
    __syncthreads();
    for (int cb = w; cb < KP / 32; cb += 4) {                        // (wave-uniform)
        const int col = cb * 32 + r;
        ngcf_f32x16 acc;
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[q] = 0.0f;
        for (int half = 0; half < 2; ++half) {
            const float *xa = X + r * ldx + half * KP, *wb = a.W + (int64_t)half * k * k;
            for (int j0 = 0; j0 < KP; j0 += 2) {
                const int j = j0 + h;
                const float bv = (j < k && col < k) ? wb[j * k + col] : 0.0f;
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[j], bv, acc, 0, 0, 0);
            }
        }
        // acc[q]: row (q & 3) + 8 (q >> 2) + 4 h of the tile, column col
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int i = (q & 3) + 8 * (q >> 2) + 4 * h;
            const int64_t row = row0 + i;
            float d = 0.0f;
            if (row < a.N && col < k) {
                const float z = acc[q];
                const float hv = z > 0.0f ? z : kNgcfSlope * z;
                d = hv;
                if (a.training) d = ngcf_keep(a.seed, a.step, a.layer, row, col, a.thr) ? hv / a.keep : 0.0f;
                a.Z[row * k + col] = z;
                a.D[row * k + col] = d;
            }
            Dt[i * ldd + col] = d;
        }
    }
    __syncthreads();
    for (int i = w * 8; i < w * 8 + 8; ++i) {
        const int64_t row = row0 + i;
        if (row >= a.N) break;                                       // (wave-uniform)
        float d[2], q = 0.0f;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int el = 64 * t + lane;
            d[t] = el < KP ? Dt[i * ldd + el] : 0.0f;
            q = __builtin_fmaf(d[t], d[t], q);
        }
        const float ss = wave_sum(q);
        const float rinv = 1.0f / __builtin_sqrtf(fmaxf(ss, kLgcnEps));
        if (lane == 0) a.ss[row] = ss;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int el = 64 * t + lane;
            if (el < k) a.F[row * a.ldF + el] = d[t] * rinv;
        }
    }
}

__global__ void __launch_bounds__(256) k_ngcf_layer_bwd(NgcfLayerArgs a) {
    extern __shared__ __attribute__((aligned(16))) float ngcf_lds[];
    const int k = a.k, KP = ngcf_kp(k), ldg = KP + 1;
    float *GZ = ngcf_lds;
    const int tid = (int)threadIdx.x, w = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int64_t row0 = (int64_t)blockIdx.x * kNgcfTile;
    for (int i = w * 8; i < w * 8 + 8; ++i) {
        const int64_t row = row0 + i;
        float gz[2] = {0.0f, 0.0f};
        if (row < a.N) {                                             // (wave-uniform)
            float g[2], d[2], dd = 0.0f;
            const float ss = a.ssr[row];
            const bool live = ss >= kLgcnEps;
            const float rinv = live ? 1.0f / __builtin_sqrtf(ss) : 1.0f;
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int el = 64 * t + lane;
                g[t] = el < k ? a.G[row * a.ldF + el] : 0.0f;
                d[t] = (el < k ? a.Dr[row * k + el] : 0.0f) * rinv;  // the normalised row where live
                dd = __builtin_fmaf(d[t], g[t], dd);
            }
            const float dot = wave_sum(dd);
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int el = 64 * t + lane;
                if (el < k) {
                    const float j = live ? (g[t] - d[t] * dot) * rinv : g[t] * 1e6f;
                    const float gd = (a.gD_in ? a.gD_in[row * k + el] : 0.0f) + j;
                    const float slope = a.Zr[row * k + el] > 0.0f ? 1.0f : kNgcfSlope;
                    float v = gd;
                    if (a.training) v = ngcf_keep(a.seed, a.step, a.layer, row, el, a.thr) ? gd / a.keep : 0.0f;
                    gz[t] = v * slope;
                    a.gZ[row * k + el] = gz[t];
                }
            }
        }
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            const int el = 64 * t + lane;
            if (el < KP) GZ[i * ldg + el] = gz[t];
        }
    }
    __syncthreads();
    for (int cb = w; cb < KP / 32; cb += 4) {                        // (wave-uniform)
        const int col = cb * 32 + r;                                 // the weights' input index
        ngcf_f32x16 acc1, acc2;
#pragma unroll
        for (int q = 0; q < 16; ++q) { acc1[q] = 0.0f; acc2[q] = 0.0f; }
        const float *ga = GZ + r * ldg, *w1 = a.W + (int64_t)col * k, *w2 = a.W + (int64_t)k * k + (int64_t)col * k;
        for (int j0 = 0; j0 < KP; j0 += 2) {
            const int j = j0 + h;
            const bool in = j < k && col < k;
            const float b1 = in ? w1[j] : 0.0f, b2 = in ? w2[j] : 0.0f;
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(ga[j], b1, acc1, 0, 0, 0);
            acc2 = __builtin_amdgcn_mfma_f32_32x32x2f32(ga[j], b2, acc2, 0, 0, 0);
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int i = (q & 3) + 8 * (q >> 2) + 4 * h;
            const int64_t row = row0 + i;
            if (row < a.N && col < k) {
                const float ev = a.E[row * k + col], sv = a.S[row * k + col];
                const float gx1 = acc1[q], gx2 = acc2[q];
                a.gS[row * k + col] = gx1 + ev * gx2;
                float lo = gx1 + sv * gx2;
                if (a.G0) lo = lo + a.G0[row * a.ldF + col];
                a.loc[row * k + col] = lo;
            }
        }
    }
}

// ---- weight gradients ---------------------------------------------------------------------------------------------------
struct NgcfWgradArgs {
    const float *E, *S, *gZ;                         // [N, k]
    int64_t N, chunks;
    int k;
    float *partial;                                  // [chunks][2][k][k]
    float *gW;                                       // [2][k][k]
};

// grid (chunks): the workgroup walks its chunk 32 rows at a time, stages [S + E | E o S] (32 x 2 KP) and gZ (32 x KP) in LDS
// (zero beyond the chunk and beyond k), and its four waves share the 2 NB x NB blocks of the result, NB = KP / 32, block
// w + 4 t to wave w.  Every block's chain runs over the chunk's rows ascending.
template <int NB>
__global__ void __launch_bounds__(256) k_ngcf_wgrad(NgcfWgradArgs a) {
    extern __shared__ __attribute__((aligned(16))) float ngcf_lds[];
    constexpr int KP = 32 * NB, ldx = 2 * KP, nblk = 2 * NB * NB, MAXT = (nblk + 3) / 4;
    const int k = a.k;
    float *X = ngcf_lds, *GZ = X + kNgcfTile * ldx;
    const int tid = (int)threadIdx.x, w = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int64_t c0 = (int64_t)blockIdx.x * kNgcfWChunk;
    const int64_t c1 = c0 + kNgcfWChunk < a.N ? c0 + kNgcfWChunk : a.N;
    ngcf_f32x16 acc[MAXT];
#pragma unroll
    for (int t = 0; t < MAXT; ++t)
#pragma unroll
        for (int q = 0; q < 16; ++q) acc[t][q] = 0.0f;
    for (int64_t s0 = c0; s0 < c1; s0 += kNgcfTile) {
        __syncthreads();                                             // the previous rows have been consumed
        for (int e = tid; e < kNgcfTile * KP; e += 256) {
            const int rr = e / KP, col = e - rr * KP;
            const int64_t row = s0 + rr;
            float ev = 0.0f, sv = 0.0f, gz = 0.0f;
            if (row < c1 && col < k) { ev = a.E[row * k + col]; sv = a.S[row * k + col]; gz = a.gZ[row * k + col]; }
            X[rr * ldx + col] = sv + ev;
            X[rr * ldx + KP + col] = ev * sv;
            GZ[rr * KP + col] = gz;
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < MAXT; ++t) {
            const int blk = w + 4 * t;
            if (blk < nblk) {                                        // (wave-uniform)
                const int rb = blk / NB, cb = blk - rb * NB;
                const float *xa = X + h * ldx + rb * 32 + r, *gb = GZ + h * KP + cb * 32 + r;
                for (int s = 0; s < kNgcfTile / 2; ++s)
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[2 * s * ldx], gb[2 * s * KP], acc[t], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int t = 0; t < MAXT; ++t) {
        const int blk = w + 4 * t;
        if (blk < nblk) {
            const int rb = blk / NB, cb = blk - rb * NB, half = rb / NB, jb = rb - half * NB, col = cb * 32 + r;
            float *dst = a.partial + ((int64_t)blockIdx.x * 2 + half) * k * k;
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int jr = jb * 32 + (q & 3) + 8 * (q >> 2) + 4 * h;
                if (jr < k && col < k) dst[jr * k + col] = acc[t][q];
            }
        }
    }
}

__global__ void __launch_bounds__(256) k_ngcf_wsum(NgcfWgradArgs a) {
    const int64_t count = 2ll * a.k * a.k;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= count) return;
    float sum = 0.0f;
    for (int64_t c = 0; c < a.chunks; ++c) sum = sum + a.partial[c * count + t];
    a.gW[t] = sum;
}

}  // namespace yue
