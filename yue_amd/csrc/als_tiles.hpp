// Register-tile layout, staging, the pair sums and the fp64 Cholesky solve shared by the ALS solvers (WRMF: wrmf_kernels.hpp,
// ExpoMF: expo_kernels.hpp, CoFactor: cof_kernels.hpp).
//
// A workgroup of 256 threads holds a k x k symmetric matrix (k <= 128, padded to KP = k rounded up to 4) as the 4x4 tiles of
// its lower triangle, tile t = ta*(ta+1)/2 + tb (ta >= tb), thread `tid` owning tiles tid, tid + 256 and tid + 512 in
// registers (fp64).  Partial sums in global memory use the same slot-major layout, [slot][tid], slot = tile-of-thread * 16 +
// p * 4 + q.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

namespace yue {

constexpr int kWrmfThreads = 256;
constexpr int kWrmfMaxK = 128;
constexpr int kWrmfTilesPerThread = 3;                                    // ceil(528 / 256): 528 tiles of the lower triangle at k = 128
constexpr int kWrmfSlots = kWrmfTilesPerThread * 16;
constexpr int kWrmfStage = 32;                                            // gathered rows per LDS stage
constexpr int kWrmfWsStride = kWrmfSlots * kWrmfThreads + 2 * kWrmfMaxK;  // doubles per partial: slots, b[128], loss
constexpr int kWrmfGramBlocks = 512;                                      // fixed: the Gram's summation order does not depend on the device
// dynamic LDS of k_wrmf_solve: the packed lower triangle of L (fp64), which also hosts the staged rows before the factorisation
__host__ __device__ constexpr int wrmf_dyn_lds(int k) {
    return (k * (k + 1) / 2 * 8) > (kWrmfStage * kWrmfMaxK * 4) ? (k * (k + 1) / 2 * 8) : (kWrmfStage * kWrmfMaxK * 4);
}

// ---- per-thread tile bookkeeping ----------------------------------------------------------------------------------
struct WrmfTiles {
    int ta[kWrmfTilesPerThread], tb[kWrmfTilesPerThread];
    bool own[kWrmfTilesPerThread];
};

__device__ inline WrmfTiles wrmf_tiles(int k) {
    WrmfTiles t;
    const int T = (k + 3) >> 2, NT = T * (T + 1) / 2;
#pragma unroll
    for (int s = 0; s < kWrmfTilesPerThread; ++s) {
        const int tt = (int)threadIdx.x + s * kWrmfThreads;
        int a = (int)((sqrtf(8.0f * (float)tt + 1.0f) - 1.0f) * 0.5f);
        while (a * (a + 1) / 2 > tt) --a;
        while ((a + 1) * (a + 2) / 2 <= tt) ++a;
        t.ta[s] = a;
        t.tb[s] = tt - a * (a + 1) / 2;
        t.own[s] = tt < NT;
    }
    return t;
}

__device__ inline double wrmf_readlane(double v, int lane) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane);
    const int hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

// Stages up to kWrmfStage rows of F (rows idx[p0..p0+cnt), or r0.. when idx is null) as fp32 [kWrmfStage][128], zero-padded.
__device__ inline void wrmf_stage(const float *__restrict__ F, int k, const int32_t *__restrict__ idx, int64_t p0, int cnt, float *stage) {
    for (int e = (int)threadIdx.x; e < kWrmfStage * kWrmfMaxK; e += kWrmfThreads) {
        const int r = e >> 7, col = e & 127;
        float v = 0.0f;
        if (r < cnt && col < k) {
            const int64_t row = idx ? (int64_t)idx[p0 + r] : p0 + r;
            v = F[row * k + col];
        }
        stage[e] = v;
    }
}

// acc += sum over the staged rows of w_j f_j f_j^T (tiles of this thread); w = null: weight 1 (the Gram)
__device__ inline void wrmf_tile_update(double (&acc)[kWrmfTilesPerThread][4][4], const WrmfTiles &t, const float *stage, const double *w, int cnt) {
    for (int j = 0; j < cnt; ++j) {
        const float *f = stage + j * kWrmfMaxK;
        const double wj = w ? w[j] : 1.0;
#pragma unroll
        for (int s = 0; s < kWrmfTilesPerThread; ++s) {
            if (t.own[s]) {
                const float4 fa = *reinterpret_cast<const float4 *>(f + 4 * t.ta[s]);
                const float4 fb = *reinterpret_cast<const float4 *>(f + 4 * t.tb[s]);
                const double xa[4] = {wj * (double)fa.x, wj * (double)fa.y, wj * (double)fa.z, wj * (double)fa.w};
                const double yb[4] = {(double)fb.x, (double)fb.y, (double)fb.z, (double)fb.w};
#pragma unroll
                for (int p = 0; p < 4; ++p)
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[s][p][q] = fma(xa[p], yb[q], acc[s][p][q]);
            }
        }
    }
}

// Factorises the k x k matrix held in the register tiles (A = L L^T, right-looking, fp64), solves A x = bvec and writes x
// rounded to fp32 to xrow.  lds_L: k(k+1)/2 doubles (the packed factor); colraw, colL, invd, bvec: kWrmfMaxK doubles each.
// The block must be synchronised on entry (bvec visible).  Returns false, for every thread, at a non-positive pivot.
// Out: float (the factor rows) or double (CoFactor's context embeddings, which the reference holds in float64).
template <typename Out>
__device__ inline bool als_cholesky_solve(double (&acc)[kWrmfTilesPerThread][4][4], const WrmfTiles &t, int k, double *lds_L, double *colraw,
                                          double *colL, double *invd, const double *bvec, Out *xrow) {
    const int tid = (int)threadIdx.x;
    // right-looking Cholesky on the register tiles: column j goes out through LDS, every tile takes the rank-1 update
    for (int j = 0; j < k; ++j) {
        const int tj = j >> 2, qj = j & 3;
#pragma unroll
        for (int s = 0; s < kWrmfTilesPerThread; ++s) {
            if (t.own[s] && t.tb[s] == tj) {
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const int r = 4 * t.ta[s] + p;
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        if (q == qj && r >= j && r < k) colraw[r] = acc[s][p][q];
                }
            }
        }
        __syncthreads();
        const double piv = colraw[j];
        if (!(piv > 0.0)) {                               // uniform: every thread read the same word
            return false;
        }
        const double d = sqrt(piv), id = 1.0 / d;
        if (tid < kWrmfMaxK) {
            const double l = (tid > j && tid < k) ? colraw[tid] * id : 0.0;
            colL[tid] = l;
            if (tid > j && tid < k) lds_L[tid * (tid + 1) / 2 + j] = l;
        }
        if (tid == 0) { lds_L[j * (j + 1) / 2 + j] = d; invd[j] = id; }
        __syncthreads();
#pragma unroll
        for (int s = 0; s < kWrmfTilesPerThread; ++s) {
            if (t.own[s] && 4 * t.ta[s] + 3 > j) {
                double la[4], lb[4];
#pragma unroll
                for (int p = 0; p < 4; ++p) { la[p] = colL[4 * t.ta[s] + p]; lb[p] = colL[4 * t.tb[s] + p]; }
#pragma unroll
                for (int p = 0; p < 4; ++p)
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[s][p][q] = fma(-la[p], lb[q], acc[s][p][q]);
            }
        }
    }
    __syncthreads();
    // L z = b, then L^T x = z: one wave, rows lane and lane + 64 in registers, the pivot value by readlane
    if (tid < 64) {
        const int r0 = tid, r1 = tid + 64;
        double v0 = bvec[r0], v1 = bvec[r1];
        for (int j = 0; j < k; ++j) {
            const double z = wrmf_readlane(j < 64 ? v0 : v1, j & 63) * invd[j];
            if (r0 == j) v0 = z;
            else if (r0 > j && r0 < k) v0 = fma(-lds_L[r0 * (r0 + 1) / 2 + j], z, v0);
            if (r1 == j) v1 = z;
            else if (r1 > j && r1 < k) v1 = fma(-lds_L[r1 * (r1 + 1) / 2 + j], z, v1);
        }
        for (int j = k - 1; j >= 0; --j) {
            const double x = wrmf_readlane(j < 64 ? v0 : v1, j & 63) * invd[j];
            const int base = j * (j + 1) / 2;
            if (r0 == j) v0 = x;
            else if (r0 < j) v0 = fma(-lds_L[base + r0], x, v0);
            if (r1 == j) v1 = x;
            else if (r1 < j) v1 = fma(-lds_L[base + r1], x, v1);
        }
        if (r0 < k) xrow[r0] = (Out)v0;
        if (r1 < k) xrow[r1] = (Out)v1;
    }
    return true;
}

// ---- the pairs of one row (WRMF's sums; CoFactor's item sweep adds its context terms to them) -----------------------------
struct WrmfArgs {
    const float *F;          // fixed side [nf][k]
    int64_t nf;
    float *X;                // solved side [nr][k] (rows written in place)
    int64_t nr;
    int k;
    const int64_t *ptr;      // pairs of the solved side's rows: ptr[nr+1], idx / cnt (rows of F, counts >= 1)
    const int32_t *idx;
    const int32_t *cnt;
    const int32_t *sched;    // solve order: rows longest first
    int64_t n_long;          // the first n_long rows of sched are long: their sums come from chunk partials
    const int64_t *cptr;     // [n_long+1] chunk range of each long row
    const int32_t *cpos;     // per chunk: its long row's position in sched
    const int64_t *cbeg;     // per chunk: pair range [cbeg, cend)
    const int64_t *cend;
    const double *G;         // fp32-rounded F^T F, slot-major [kWrmfSlots][256]
    double *ws;              // chunk partials [chunks][kWrmfWsStride]
    double alpha, reg;
    int want_loss;           // side 0: sum (1 - x_old . y)^2 over the row's pairs
    double *row_loss;        // [nr] in sched order
    int *status;             // smallest row with a non-positive pivot (INT_MAX: none)
};

// Sums of the pairs [p0, p1) of one row: tiles (acc), b (thread t < k: bacc), and, with xo, the loss terms of the 32 rows
// of a stage (thread 8r: row r of each stage; lacc).  Leaves the block synchronised.
__device__ inline void wrmf_pairs(const WrmfArgs &a, const WrmfTiles &t, int64_t p0, int64_t p1, float *stage, double *sw, double *sw1,
                                  const float *xo, double (&acc)[kWrmfTilesPerThread][4][4], double &bacc, double &lacc) {
    const int tid = (int)threadIdx.x, k = a.k;
    for (int64_t q0 = p0; q0 < p1; q0 += kWrmfStage) {
        const int cnt = (int)((p1 - q0) < kWrmfStage ? (p1 - q0) : kWrmfStage);
        __syncthreads();                                      // the previous stage has been consumed
        wrmf_stage(a.F, k, a.idx, q0, cnt, stage);
        if (tid < cnt) {
            const double c = a.alpha * (double)a.cnt[q0 + tid];
            sw[tid] = c;
            sw1[tid] = 1.0 + c;
        }
        __syncthreads();
        wrmf_tile_update(acc, t, stage, sw, cnt);
        if (tid < k)
            for (int j = 0; j < cnt; ++j) bacc = fma(sw1[j], (double)stage[j * kWrmfMaxK + tid], bacc);
        if (xo) {                                              // (1 - x_old . y)^2, the dot rounded to fp32 once
            const int r = tid >> 3, sub = tid & 7;
            double d = 0.0;
            for (int col = sub; col < k; col += 8) d = fma((double)xo[col], (double)stage[r * kWrmfMaxK + col], d);
            d += __shfl_xor(d, 1);
            d += __shfl_xor(d, 2);
            d += __shfl_xor(d, 4);
            if (sub == 0 && r < cnt) {
                const double e = 1.0 - (double)(float)d;
                lacc = fma(e, e, lacc);
            }
        }
    }
    __syncthreads();
}

}  // namespace yue
