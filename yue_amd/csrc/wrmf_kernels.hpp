// WRMF (recommender/cf/WRMF.py): one ALS half-sweep = every row of one side solved from the other side's factors.
//   A_r = fp32(F^T F) + sum_j alpha*r_j f_j f_j^T + reg*I,  b_r = sum_j (1 + alpha*r_j) f_j,  x_r = A_r^-1 b_r (fp64 Cholesky)
// Host side: wrmf_host.hip.  No float atomics: every sum has one fixed order, so a half-sweep is bit-reproducible.
//
// Layout shared by the kernels: a workgroup of 256 threads holds a k x k symmetric matrix (k <= 128, padded to KP =
// k rounded up to 4) as the 4x4 tiles of its lower triangle, tile t = ta*(ta+1)/2 + tb (ta >= tb), thread `tid` owning
// tiles tid, tid + 256 and tid + 512 in registers (fp64).  Partial sums in global memory (Gram blocks, long-row chunks,
// the rounded Gram itself) use the same slot-major layout, [slot][tid], slot = tile-of-thread * 16 + p * 4 + q.
#pragma once
#include <hip/hip_runtime.h>

#include "als_tiles.hpp"

#include <climits>
#include <cstdint>

namespace yue {

// ---- F^T F: block partials over fixed row ranges, then one fixed-order sum rounded to fp32 ------------------------
__global__ __launch_bounds__(kWrmfThreads) void k_wrmf_gram_part(const float *__restrict__ F, int64_t nf, int k, int64_t rows_per_block, double *__restrict__ part) {
    __shared__ __attribute__((aligned(16))) float stage[kWrmfStage * kWrmfMaxK];
    const WrmfTiles t = wrmf_tiles(k);
    double acc[kWrmfTilesPerThread][4][4] = {};
    const int64_t r0 = (int64_t)blockIdx.x * rows_per_block;
    const int64_t r1 = r0 + rows_per_block < nf ? r0 + rows_per_block : nf;
    for (int64_t q0 = r0; q0 < r1; q0 += kWrmfStage) {
        const int cnt = (int)((r1 - q0) < kWrmfStage ? (r1 - q0) : kWrmfStage);
        __syncthreads();
        wrmf_stage(F, k, nullptr, q0, cnt, stage);
        __syncthreads();
        wrmf_tile_update(acc, t, stage, nullptr, cnt);
    }
    double *out = part + (int64_t)blockIdx.x * kWrmfWsStride;
#pragma unroll
    for (int s = 0; s < kWrmfTilesPerThread; ++s)
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int q = 0; q < 4; ++q) out[(s * 16 + p * 4 + q) * kWrmfThreads + threadIdx.x] = acc[s][p][q];
}

// grid kWrmfSlots x 256 threads: G[slot][tid] = fp32(sum over the blocks in order)
__global__ __launch_bounds__(kWrmfThreads) void k_wrmf_gram_sum(const double *__restrict__ part, int nblk, double *__restrict__ G) {
    const int64_t e = (int64_t)blockIdx.x * kWrmfThreads + threadIdx.x;
    double s = 0.0;
    for (int b = 0; b < nblk; ++b) s += part[(int64_t)b * kWrmfWsStride + e];
    G[e] = (double)(float)s;
}

// ---- long rows: one workgroup per chunk of pairs writes its partial sums ------------------------------------------
__global__ __launch_bounds__(kWrmfThreads) void k_wrmf_chunk(WrmfArgs a) {
    __shared__ __attribute__((aligned(16))) float stage[kWrmfStage * kWrmfMaxK];
    __shared__ double sw[kWrmfStage], sw1[kWrmfStage], red[kWrmfThreads];
    __shared__ float xo[kWrmfMaxK];
    const int tid = (int)threadIdx.x;
    const int64_t c = blockIdx.x;
    const int32_t row = a.sched[a.cpos[c]];
    if (a.want_loss && tid < a.k) xo[tid] = a.X[(int64_t)row * a.k + tid];
    const WrmfTiles t = wrmf_tiles(a.k);
    double acc[kWrmfTilesPerThread][4][4] = {};
    double bacc = 0.0, lacc = 0.0;
    wrmf_pairs(a, t, a.cbeg[c], a.cend[c], stage, sw, sw1, a.want_loss ? xo : nullptr, acc, bacc, lacc);
    double *out = a.ws + c * kWrmfWsStride;
#pragma unroll
    for (int s = 0; s < kWrmfTilesPerThread; ++s)
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int q = 0; q < 4; ++q) out[(s * 16 + p * 4 + q) * kWrmfThreads + tid] = acc[s][p][q];
    if (tid < kWrmfMaxK) out[kWrmfSlots * kWrmfThreads + tid] = bacc;
    red[tid] = lacc;
    __syncthreads();
    if (tid == 0) {
        double l = 0.0;
        for (int r = 0; r < kWrmfThreads; r += 8) l += red[r];
        out[kWrmfSlots * kWrmfThreads + kWrmfMaxK] = l;
    }
}

// ---- the solve: one workgroup per row (in sched order) -------------------------------------------------------------
__global__ __launch_bounds__(kWrmfThreads, 2) void k_wrmf_solve(WrmfArgs a) {
    extern __shared__ __attribute__((aligned(16))) double lds_L[];   // wrmf_dyn_lds(k) bytes: staged rows, then packed L
    __shared__ double sw[kWrmfStage], sw1[kWrmfStage], red[kWrmfThreads];
    __shared__ double colraw[kWrmfMaxK], colL[kWrmfMaxK], invd[kWrmfMaxK], bvec[kWrmfMaxK];
    __shared__ float xo[kWrmfMaxK];
    const int tid = (int)threadIdx.x, k = a.k;
    const int64_t pos = blockIdx.x;
    const int32_t row = a.sched[pos];
    const int64_t p0 = a.ptr[row], p1 = a.ptr[row + 1];
    float *xrow = a.X + (int64_t)row * k;
    if (p1 == p0) {                                       // no pairs: b = 0, the row is exactly 0
        if (tid < k) xrow[tid] = 0.0f;
        if (tid == 0 && a.want_loss) a.row_loss[pos] = 0.0;
        return;
    }
    if (a.want_loss && tid < k) xo[tid] = xrow[tid];
    const WrmfTiles t = wrmf_tiles(k);
    double acc[kWrmfTilesPerThread][4][4] = {};
    double bacc = 0.0, lacc = 0.0;
    if (pos < a.n_long) {                                 // long row: the chunks' partials, summed in chunk order
        __syncthreads();
        for (int64_t c = a.cptr[pos]; c < a.cptr[pos + 1]; ++c) {
            const double *in = a.ws + c * kWrmfWsStride;
#pragma unroll
            for (int s = 0; s < kWrmfTilesPerThread; ++s)
#pragma unroll
                for (int p = 0; p < 4; ++p)
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[s][p][q] += in[(s * 16 + p * 4 + q) * kWrmfThreads + tid];
            if (tid < kWrmfMaxK) bacc += in[kWrmfSlots * kWrmfThreads + tid];
            if (tid == 0) lacc += in[kWrmfSlots * kWrmfThreads + kWrmfMaxK];
        }
    } else {
        __syncthreads();                                  // xo visible
        wrmf_pairs(a, t, p0, p1, reinterpret_cast<float *>(lds_L), sw, sw1, a.want_loss ? xo : nullptr, acc, bacc, lacc);
    }
    // A = (sum + fp32 Gram) + reg on the diagonal
#pragma unroll
    for (int s = 0; s < kWrmfTilesPerThread; ++s)
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                acc[s][p][q] += a.G[(s * 16 + p * 4 + q) * kWrmfThreads + tid];
                if (p == q && t.ta[s] == t.tb[s]) acc[s][p][q] += a.reg;
            }
    if (tid < kWrmfMaxK) bvec[tid] = tid < k ? bacc : 0.0;
    red[tid] = lacc;
    __syncthreads();                                      // (the staged rows are dead from here on: lds_L becomes L)
    if (a.want_loss && tid == 0) {
        double l = 0.0;
        for (int r = 0; r < kWrmfThreads; r += 8) l += red[r];
        a.row_loss[pos] = l;
    }
    if (!als_cholesky_solve(acc, t, k, lds_L, colraw, colL, invd, bvec, xrow)) {
        if (tid == 0) atomicMin(a.status, row);
        return;
    }
}

// loss = sum of row_loss in a fixed order (one workgroup)
__global__ __launch_bounds__(kWrmfThreads) void k_wrmf_loss_sum(const double *__restrict__ row_loss, int64_t nr, double *__restrict__ out) {
    __shared__ double red[kWrmfThreads];
    double s = 0.0;
    for (int64_t r = threadIdx.x; r < nr; r += kWrmfThreads) s += row_loss[r];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = kWrmfThreads / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) *out = red[0];
}

}  // namespace yue
