// ExpoMF (recommender/advanced/ExpoMF.py): exposure-weighted ALS.  One half-sweep solves every row r of one side from the
// other side's factors F and the row's own old value x_r:
//   s_j = x_r . f_j,  pEX_j = sqrt(lam_y pi / 2) exp(-lam_y s_j^2 / 2),  A~_j = (pEX_j + 1e-8) / (pEX_j + 1e-8 + (1 - mu) / mu)
//   B_r = sum over ALL j of A~_j f_j f_j^T  +  sum over the row's pairs of (1 - A~_j) f_j f_j^T  +  lam I,   a_r = sum r_j f_j
//   x_r = B_r^-1 a_r (fp64 Cholesky, als_tiles.hpp), rounded to fp32 once; rows without pairs become 0.
// The first sum is dense (nf columns per row, k(k+1) flop each) and runs on the matrix cores: k_expo_gram forms, for a tile of
// 32 rows and chunks of 128 columns in LDS, S = F_chunk X_tile^T (v_mfma_f32_32x32x2_f32), the posterior A~ in the accumulator
// registers, and then the GEMM A~ . Z with Z_j = (f_jp f_jq), p >= q, formed on the fly: M = 32 rows, N = k(k+1)/2 pairs in
// blocks of 32, K = columns.  Its result is the packed lower triangle of every row's Gram in fp32, [split][row][pair].  The
// second sum, lam I, a_r and the solve are fp64 (k_expo_chunk for the long rows, k_expo_solve).  The exposure prior
// (k_expo_asum, k_expo_mu) sums the posterior over all users per item the same way.
// Host side: expo_host.hip.  No float atomics: column chunks, splits and partials are summed in a fixed order that depends on
// the shapes only, so a half-sweep is bit-reproducible.
#pragma once
#include <hip/hip_runtime.h>

#include "als_tiles.hpp"

namespace yue {

constexpr int kExpoTile = 32;                 // rows per workgroup of the dense kernels (the M of the MFMA)
constexpr int kExpoFlush = 4;                 // chunks per inner accumulation of the Gram
constexpr int kExpoChunk = 128;               // columns staged in LDS per step: 32 per wave for S, all of them for the Gram

typedef float expo_f32x16 __attribute__((ext_vector_type(16)));

__host__ __device__ constexpr int expo_ld(int k) { return ((k + 3) & ~3) + 1; }          // LDS row stride (floats): odd, conflict-free column reads
// dynamic LDS of the dense kernels: F chunk [128][ld], old rows [32][ld], posterior [128][32], ratios [128]
__host__ __device__ constexpr int expo_dyn_lds(int k) { return (kExpoChunk * expo_ld(k) + kExpoTile * expo_ld(k) + kExpoChunk * kExpoTile + kExpoChunk) * 4; }

struct ExpoArgs {
    const float *F;          // fixed side [nf][k]
    int64_t nf;
    float *X;                // solved side [nr][k]: old rows read, new rows written in place
    int64_t nr;
    int k;
    const int64_t *ptr;      // pairs of the solved side's rows (the WRMF upload: wrmf_host.hip)
    const int32_t *idx;
    const int32_t *cnt;
    const int32_t *sched;    // solve order: rows longest first
    int64_t n_long;
    const int64_t *cptr;
    const int32_t *cpos;
    const int64_t *cbeg;
    const int64_t *cend;
    const float *mu;         // per column of the posterior (mu_per_column) or per solved row
    int mu_per_column;
    float *gws;              // dense Grams of the batch: [splits][pos1 - pos0][npairs] fp32
    double *ws;              // long rows' chunk partials [chunks][kWrmfWsStride]
    int64_t pos0, pos1;      // the batch: positions of sched
    int splits;              // column ranges summed separately (fixed by the shapes)
    int64_t cols_per_split;  // a multiple of kExpoChunk
    int npairs;              // k(k+1)/2
    double lam, c0, hl;      // ridge term; sqrt(lam_y pi / 2); lam_y / 2
    int *status;             // smallest row with a non-positive pivot (INT_MAX: none)
};

__device__ inline float expo_ratio32(float mu) { return (1.0f - mu) / mu; }
__device__ inline float expo_post32(float s, float ratio, float c0, float hl) {
    const float pex = c0 * expf(-hl * s * s) + 1e-8f;
    return pex / (pex + ratio);
}
__device__ inline double expo_post64(double s, double mu, double c0, double hl) {
    const double pex = c0 * exp(-hl * s * s) + 1e-8;
    return pex / (pex + (1.0 - mu) / mu);
}

// Stages rows [j0, j0 + rows) of F (or rows sched[j0 ..] when sched is given) as [rows][ld], zero beyond `limit` and beyond k.
__device__ inline void expo_stage(const float *__restrict__ F, const int32_t *__restrict__ sched, int64_t j0, int64_t limit, int k, int rows, float *dst) {
    const int KP = (k + 3) & ~3, ld = expo_ld(k);
    for (int e = (int)threadIdx.x; e < rows * KP; e += 256) {
        const int rr = e / KP, col = e - rr * KP;
        const int64_t j = j0 + rr;
        float v = 0.0f;
        if (j < limit && col < k) v = F[(sched ? (int64_t)sched[j] : j) * k + col];
        dst[rr * ld + col] = v;
    }
}

// S^T of 32 staged columns (rows of fc) against the 32 staged rows xo: acc[q] = f_i . x_r with i = (q&3) + 8(q>>2) + 4h, r = lane & 31.
__device__ inline expo_f32x16 expo_scores(const float *fc, const float *xo, int k) {
    const int lane = (int)threadIdx.x & 63, r = lane & 31, h = lane >> 5, ld = expo_ld(k), K2 = ((k + 3) & ~3) >> 1;
    expo_f32x16 acc;
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[q] = 0.0f;
    const float *pa = fc + r * ld + h, *pb = xo + r * ld + h;
    for (int s = 0; s < K2; ++s) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(pa[2 * s], pb[2 * s], acc, 0, 0, 0);
    return acc;
}

// ---- the dense Gram: grid (row tiles of the batch, groups of 4 * NB pair blocks, column splits) --------------------------------
template <int NB>
__global__ __launch_bounds__(256) void k_expo_gram(ExpoArgs a) {
    extern __shared__ __attribute__((aligned(16))) float expo_lds[];
    const int k = a.k, ld = expo_ld(k);
    float *fc = expo_lds, *xo = fc + kExpoChunk * ld, *at = xo + kExpoTile * ld, *ratio_c = at + kExpoChunk * kExpoTile;
    const int tid = (int)threadIdx.x, w = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int64_t tpos = a.pos0 + (int64_t)blockIdx.x * kExpoTile;
    const float c0 = (float)a.c0, hl = (float)a.hl;
    expo_stage(a.X, a.sched, tpos, a.pos1, k, kExpoTile, xo);
    float ratio_r = 1.0f;
    if (!a.mu_per_column && tpos + r < a.pos1) ratio_r = expo_ratio32(a.mu[a.sched[tpos + r]]);
    // this wave's pair blocks: lane n = r holds pair b * 32 + r = (p, q), p >= q
    int offp[NB], offq[NB];
    const int b0 = ((int)blockIdx.y * 4 + w) * NB;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        int pi = (b0 + j) * 32 + r;
        if (pi >= a.npairs) pi = 0;
        int p = (int)((sqrtf(8.0f * (float)pi + 1.0f) - 1.0f) * 0.5f);
        while (p * (p + 1) / 2 > pi) --p;
        while ((p + 1) * (p + 2) / 2 <= pi) ++p;
        offp[j] = h * ld + p;
        offq[j] = h * ld + (pi - p * (p + 1) / 2);
    }
    // two levels of fp32 accumulators: the MFMA chain runs over kExpoFlush chunks (512 columns), then joins the running sum, so
    // that the rounding of a long sum grows with the number of flushes and not with the number of columns
    expo_f32x16 acc[NB], tot[NB];
#pragma unroll
    for (int j = 0; j < NB; ++j)
#pragma unroll
        for (int q = 0; q < 16; ++q) { acc[j][q] = 0.0f; tot[j][q] = 0.0f; }
    int since = 0;
    const int64_t col0 = (int64_t)blockIdx.z * a.cols_per_split;
    const int64_t col1 = col0 + a.cols_per_split < a.nf ? col0 + a.cols_per_split : a.nf;
    for (int64_t c = col0; c < col1; c += kExpoChunk) {
        __syncthreads();                                              // the previous chunk has been consumed
        expo_stage(a.F, nullptr, c, col1, k, kExpoChunk, fc);
        if (tid < kExpoChunk) ratio_c[tid] = (c + tid < col1) ? (a.mu_per_column ? expo_ratio32(a.mu[c + tid]) : 0.0f) : 1.0f;
        __syncthreads();
        {   // posterior of this wave's 32 columns, for all 32 rows, to LDS as [column][row]
            const expo_f32x16 s = expo_scores(fc + w * 32 * ld, xo, k);
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int i = w * 32 + (q & 3) + 8 * (q >> 2) + 4 * h;
                at[i * kExpoTile + r] = expo_post32(s[q], a.mu_per_column ? ratio_c[i] : ratio_r, c0, hl);
            }
        }
        __syncthreads();
        // A~ . Z: K-step kk covers columns 2kk and 2kk + 1 (lane half h); padded columns have f = 0, so Z = 0
#pragma unroll 2
        for (int kk = 0; kk < kExpoChunk / 2; ++kk) {
            const float av = at[(2 * kk + h) * kExpoTile + r];
            const float *row = fc + 2 * kk * ld;
#pragma unroll
            for (int j = 0; j < NB; ++j)
                if ((b0 + j) * 32 < a.npairs)                          // wave-uniform
                    acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, row[offp[j]] * row[offq[j]], acc[j], 0, 0, 0);
        }
        if (++since == kExpoFlush || c + kExpoChunk >= col1) {
            since = 0;
#pragma unroll
            for (int j = 0; j < NB; ++j)
#pragma unroll
                for (int q = 0; q < 16; ++q) { tot[j][q] += acc[j][q]; acc[j][q] = 0.0f; }
        }
    }
    // acc[j][q]: row (q&3) + 8(q>>2) + 4h of the tile, pair (b0 + j) * 32 + r
    const int64_t rb = a.pos1 - a.pos0;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
        const int pi = (b0 + j) * 32 + r;
        if (pi < a.npairs) {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int64_t rr = (int64_t)blockIdx.x * kExpoTile + (q & 3) + 8 * (q >> 2) + 4 * h;
                if (rr < rb) a.gws[((int64_t)blockIdx.z * rb + rr) * a.npairs + pi] = tot[j][q];
            }
        }
    }
}

// ---- the pairs of one row: acc += sum (1 - A~_j) f_j f_j^T, bacc += sum r_j f_j (fp64) ------------------------------------------
__device__ inline void expo_pairs(const ExpoArgs &a, const WrmfTiles &t, int32_t row, int64_t p0, int64_t p1, float *stage, double *sw, double *sw1,
                                  const float *xo, double (&acc)[kWrmfTilesPerThread][4][4], double &bacc) {
    const int tid = (int)threadIdx.x, k = a.k;
    for (int64_t q0 = p0; q0 < p1; q0 += kWrmfStage) {
        const int cnt = (int)((p1 - q0) < kWrmfStage ? (p1 - q0) : kWrmfStage);
        __syncthreads();                                      // the previous stage has been consumed
        wrmf_stage(a.F, k, a.idx, q0, cnt, stage);
        __syncthreads();
        {
            const int r = tid >> 3, sub = tid & 7;
            double d = 0.0;
            for (int col = sub; col < k; col += 8) d = fma((double)xo[col], (double)stage[r * kWrmfMaxK + col], d);
            d += __shfl_xor(d, 1);
            d += __shfl_xor(d, 2);
            d += __shfl_xor(d, 4);
            if (sub == 0 && r < cnt) {
                const double mu = (double)a.mu[a.mu_per_column ? a.idx[q0 + r] : row];
                sw[r] = 1.0 - expo_post64(d, mu, a.c0, a.hl);
                sw1[r] = (double)a.cnt[q0 + r];
            }
        }
        __syncthreads();
        wrmf_tile_update(acc, t, stage, sw, cnt);
        if (tid < k)
            for (int j = 0; j < cnt; ++j) bacc = fma(sw1[j], (double)stage[j * kWrmfMaxK + tid], bacc);
    }
    __syncthreads();
}

// long rows: one workgroup per chunk of pairs writes its partial sums (the layout of k_wrmf_chunk)
__global__ __launch_bounds__(kWrmfThreads) void k_expo_chunk(ExpoArgs a) {
    __shared__ __attribute__((aligned(16))) float stage[kWrmfStage * kWrmfMaxK];
    __shared__ double sw[kWrmfStage], sw1[kWrmfStage];
    __shared__ float xo[kWrmfMaxK];
    const int tid = (int)threadIdx.x;
    const int64_t c = blockIdx.x;
    const int32_t row = a.sched[a.cpos[c]];
    if (tid < a.k) xo[tid] = a.X[(int64_t)row * a.k + tid];
    const WrmfTiles t = wrmf_tiles(a.k);
    double acc[kWrmfTilesPerThread][4][4] = {};
    double bacc = 0.0;
    expo_pairs(a, t, row, a.cbeg[c], a.cend[c], stage, sw, sw1, xo, acc, bacc);
    double *out = a.ws + c * kWrmfWsStride;
#pragma unroll
    for (int s = 0; s < kWrmfTilesPerThread; ++s)
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int q = 0; q < 4; ++q) out[(s * 16 + p * 4 + q) * kWrmfThreads + tid] = acc[s][p][q];
    if (tid < kWrmfMaxK) out[kWrmfSlots * kWrmfThreads + tid] = bacc;
}

// ---- the solve: one workgroup per row of the batch (in sched order) ---------------------------------------------------------
__global__ __launch_bounds__(kWrmfThreads, 2) void k_expo_solve(ExpoArgs a) {
    extern __shared__ __attribute__((aligned(16))) double lds_L[];   // wrmf_dyn_lds(k) bytes: staged rows, then packed L
    __shared__ double sw[kWrmfStage], sw1[kWrmfStage];
    __shared__ double colraw[kWrmfMaxK], colL[kWrmfMaxK], invd[kWrmfMaxK], bvec[kWrmfMaxK];
    __shared__ float xo[kWrmfMaxK];
    const int tid = (int)threadIdx.x, k = a.k;
    const int64_t pos = a.pos0 + blockIdx.x;
    const int32_t row = a.sched[pos];
    const int64_t p0 = a.ptr[row], p1 = a.ptr[row + 1];
    float *xrow = a.X + (int64_t)row * k;
    if (p1 == p0) {                                       // no pairs: a = 0, the row is exactly 0
        if (tid < k) xrow[tid] = 0.0f;
        return;
    }
    if (tid < k) xo[tid] = xrow[tid];
    const WrmfTiles t = wrmf_tiles(k);
    double acc[kWrmfTilesPerThread][4][4] = {};
    double bacc = 0.0;
    __syncthreads();                                      // xo visible
    if (pos < a.n_long) {                                 // long row: the chunks' partials, summed in chunk order
        for (int64_t c = a.cptr[pos]; c < a.cptr[pos + 1]; ++c) {
            const double *in = a.ws + c * kWrmfWsStride;
#pragma unroll
            for (int s = 0; s < kWrmfTilesPerThread; ++s)
#pragma unroll
                for (int p = 0; p < 4; ++p)
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[s][p][q] += in[(s * 16 + p * 4 + q) * kWrmfThreads + tid];
            if (tid < kWrmfMaxK) bacc += in[kWrmfSlots * kWrmfThreads + tid];
        }
    } else {
        expo_pairs(a, t, row, p0, p1, reinterpret_cast<float *>(lds_L), sw, sw1, xo, acc, bacc);
    }
    // B = (pairs' correction + the dense Gram's splits in order) + lam on the diagonal
    const int64_t rb = a.pos1 - a.pos0;
    const float *g = a.gws + (int64_t)blockIdx.x * a.npairs;
#pragma unroll
    for (int s = 0; s < kWrmfTilesPerThread; ++s) {
        if (!t.own[s]) continue;
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int i = 4 * t.ta[s] + p, j = 4 * t.tb[s] + q;
                const int hi = i > j ? i : j, lo = i > j ? j : i;
                if (hi < k) {
                    double v = 0.0;
                    for (int sp = 0; sp < a.splits; ++sp) v += (double)g[(int64_t)sp * rb * a.npairs + hi * (hi + 1) / 2 + lo];
                    acc[s][p][q] += v;
                }
                if (i == j) acc[s][p][q] += a.lam;
            }
    }
    if (tid < kWrmfMaxK) bvec[tid] = tid < k ? bacc : 0.0;
    __syncthreads();                                      // (the staged rows are dead from here on: lds_L becomes L)
    if (!als_cholesky_solve(acc, t, k, lds_L, colraw, colL, invd, bvec, xrow)) {
        if (tid == 0) atomicMin(a.status, row);
        return;
    }
}

// ---- exposure prior: A_sum[i] = sum over all users of A_ui --------------------------------------------------------------------
// grid (item tiles of 32, user splits): part[split][item] = sum over the split's users of A~_ui (fp64; the rows are items here)
__global__ __launch_bounds__(256) void k_expo_asum(ExpoArgs a, double *__restrict__ part) {
    extern __shared__ __attribute__((aligned(16))) float expo_lds[];
    __shared__ double red[4][kExpoTile];
    const int k = a.k, ld = expo_ld(k);
    float *fc = expo_lds, *xo = fc + kExpoChunk * ld;
    const int tid = (int)threadIdx.x, w = tid >> 6, lane = tid & 63, r = lane & 31, h = lane >> 5;
    const int64_t i0 = (int64_t)blockIdx.x * kExpoTile;
    const float c0 = (float)a.c0, hl = (float)a.hl;
    expo_stage(a.X, nullptr, i0, a.nr, k, kExpoTile, xo);
    const float ratio_r = i0 + r < a.nr ? expo_ratio32(a.mu[i0 + r]) : 1.0f;
    double sum = 0.0;
    const int64_t col0 = (int64_t)blockIdx.y * a.cols_per_split;
    const int64_t col1 = col0 + a.cols_per_split < a.nf ? col0 + a.cols_per_split : a.nf;
    for (int64_t c = col0; c < col1; c += kExpoChunk) {
        __syncthreads();
        expo_stage(a.F, nullptr, c, col1, k, kExpoChunk, fc);
        __syncthreads();
        const expo_f32x16 s = expo_scores(fc + w * 32 * ld, xo, k);
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            const int64_t u = c + w * 32 + (q & 3) + 8 * (q >> 2) + 4 * h;
            if (u < col1) sum += (double)expo_post32(s[q], ratio_r, c0, hl);
        }
    }
    sum += __shfl_xor(sum, 32);
    if (h == 0) red[w][r] = sum;
    __syncthreads();
    if (tid < kExpoTile && i0 + tid < a.nr) part[(int64_t)blockIdx.y * a.nr + i0 + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// one wave per item: A_sum = the splits in order + sum over the item's users of (1 - A~_ui); mu = (pa + A_sum - 1) / (pa + pb + m - 2)
__global__ __launch_bounds__(256) void k_expo_mu(ExpoArgs a, const double *__restrict__ part, int nsplit, double pa, double pb, float *mu_out) {
    const int lane = (int)threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= a.nr) return;
    const int k = a.k;
    const double mu = (double)a.mu[i];
    const float *x = a.X + i * k;
    double corr = 0.0;
    for (int64_t e = a.ptr[i] + lane; e < a.ptr[i + 1]; e += 64) {
        const float *f = a.F + (int64_t)a.idx[e] * k;
        double d = 0.0;
        for (int col = 0; col < k; ++col) d = fma((double)x[col], (double)f[col], d);
        corr += 1.0 - expo_post64(d, mu, a.c0, a.hl);
    }
    for (int o = 1; o < 64; o <<= 1) corr += __shfl_xor(corr, o);
    if (lane == 0) {
        double s = 0.0;
        for (int sp = 0; sp < nsplit; ++sp) s += part[(int64_t)sp * a.nr + i];
        mu_out[i] = (float)((pa + (s + corr) - 1.0) / (pa + pb + (double)a.nf - 2.0));
    }
}

}  // namespace yue
