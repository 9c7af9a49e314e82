// CoFactor (recommender/advanced/CoFactor.py): the item x item co-occurrence counts, and the item sweep of its ALS.
//   co-occurrence  count(i, j) = common users of items i and j, by posting-list counting: one workgroup per item i walks the
//                  item lists of i's users in passes over item ranges (integer LDS counters, no n x n array); items with
//                  fewer than f training events take no part, a pair is kept when count > f.  Count, then fill: ascending CSR.
//   item sweep     per item i with contexts S_i (its SPPMI row, values s_ij), every right-hand side before any write:
//                    Y[i] <- (fp32(X^T X) + sum_u alpha r x_u x_u^T + regU I + sum_j G_j G_j^T)^-1 (sum_u (1 + alpha r) x_u + sum_j (s_ij - w_i - c_j) G_j)
//                    G[i] <- (sum_j Y_j Y_j^T + regR I)^-1 sum_j (s_ij - w_j - c_i) Y_j,  w[i] <- mean_j (s_ij - Y_i.G_j - c_j),
//                    c[i] <- mean_j (s_ij - Y_j.G_i - w_j)   (the last three only where S_i is not empty)
//                  The reference sweeps the items in id order and reads the current rows of the contexts; the host launches
//                  the rows level by level (level(i) = 1 + max level of the contexts j < i), which reads and writes the same
//                  values.  Y is fp32 (rounded once), G, w, c are fp64 as in the reference.
// Host side: cof_host.hip.  Integer atomics only; every floating-point sum has one fixed order (contexts ascending).
#pragma once
#include <hip/hip_runtime.h>

#include "als_tiles.hpp"

#include <climits>
#include <cstdint>

namespace yue {

constexpr int kCofThreads = 256;
constexpr int kCofRange = 8192;        // items counted per pass of k_cof_cooccur (LDS counters)
constexpr int kCofStage = 16;          // fp64 context rows per LDS stage: the bytes of kWrmfStage fp32 rows

struct CofCoArgs {
    int64_t n;
    const int64_t *u_ptr;      // user-major pairs: items ascending
    const int32_t *u_items;
    const int64_t *i_ptr;      // item-major pairs: users ascending, with event counts
    const int32_t *i_users;
    const int32_t *i_counts;
    int64_t *cursor;           // [nnz] per (item, user) the next position in the user's item list
    int32_t *events;           // [n] training events of an item (sum of its counts, saturated)
    int filter;
    int range;                 // items per pass (<= kCofRange)
    int fill;                  // 0: count the kept entries of every row (row_nnz); 1: write them at ptr
    int64_t *row_nnz;          // [n]
    const int64_t *ptr;        // [n+1]
    int32_t *idx, *cnt;        // [nnz of the co-occurrence CSR]
};

__global__ __launch_bounds__(kCofThreads) void k_cof_events(CofCoArgs a) {
    const int64_t i = (int64_t)blockIdx.x * kCofThreads + threadIdx.x;
    if (i >= a.n) return;
    int64_t s = 0;
    for (int64_t e = a.i_ptr[i]; e < a.i_ptr[i + 1]; ++e) s += a.i_counts[e];
    a.events[i] = (int32_t)(s < INT_MAX ? s : INT_MAX);
}

// One workgroup per item i.  Per pass [lo, hi): every user of i adds 1 to the counters of the user's items inside the pass
// (cursor kept across passes); then the counters are read in item order, cleared, and the kept ones are numbered by a
// ballot prefix, so a row comes out ascending without a sort.
__global__ __launch_bounds__(kCofThreads) void k_cof_cooccur(CofCoArgs a) {
    __shared__ uint32_t cnt[kCofRange];
    __shared__ int wave_n[kCofThreads / 64];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t i = (int32_t)blockIdx.x;
    const int64_t rb = a.i_ptr[i], du = a.i_ptr[i + 1] - rb;
    if (du == 0 || a.events[i] < a.filter) {
        if (!a.fill && tid == 0) a.row_nnz[i] = 0;
        return;
    }
    for (int x = tid; x < a.range; x += kCofThreads) cnt[x] = 0u;
    for (int64_t j = tid; j < du; j += kCofThreads) a.cursor[rb + j] = a.u_ptr[a.i_users[rb + j]];
    __syncthreads();
    const int64_t row_end = a.fill ? a.ptr[i + 1] : 0;
    int64_t out = a.fill ? a.ptr[i] : 0;
    for (int64_t lo = 0; lo < a.n; lo += a.range) {
        const int64_t hi = lo + a.range < a.n ? lo + a.range : a.n;
        for (int64_t j = tid; j < du; j += kCofThreads) {       // the same thread owns cursor[rb + j] in every pass
            const int64_t end = a.u_ptr[a.i_users[rb + j] + 1];
            int64_t p = a.cursor[rb + j];
            while (p < end) {
                const int64_t it = a.u_items[p];
                if (it >= hi) break;
                atomicAdd(&cnt[it - lo], 1u);
                ++p;
            }
            a.cursor[rb + j] = p;
        }
        __syncthreads();
        const int width = (int)(hi - lo);
        for (int base = 0; base < width; base += kCofThreads) {
            const int x = base + tid;
            uint32_t c = 0u;
            bool keep = false;
            if (x < width) {
                c = cnt[x];
                cnt[x] = 0u;
                keep = (int64_t)c > (int64_t)a.filter && lo + x != i && a.events[lo + x] >= a.filter;
            }
            const unsigned long long b = __ballot(keep);
            if (lane == 0) wave_n[wave] = __popcll(b);
            __syncthreads();
            int before = 0, total = 0;
            for (int w = 0; w < kCofThreads / 64; ++w) {
                if (w < wave) before += wave_n[w];
                total += wave_n[w];
            }
            if (keep && a.fill) {
                const int64_t pos = out + before + __popcll(b & ((1ull << lane) - 1ull));
                if (pos < row_end) {
                    a.idx[pos] = (int32_t)(lo + x);
                    a.cnt[pos] = (int32_t)c;
                }
            }
            out += total;
            __syncthreads();
        }
    }
    if (!a.fill && tid == 0) a.row_nnz[i] = out;
}

struct CofArgs {
    WrmfArgs w;                // F = X (users), X = Y (item rows, written in place), the item-major pairs, the Gram, alpha, reg = regU;
                               // sched: the rows level by level; cptr / cbeg / cend: the chunks of the long rows; ws: their partials
                               // (n_long and cpos, WRMF's own long-row tables, are not used: lpos replaces them)
    const int32_t *lpos;       // per sched position: index of the row among the long rows, -1 for the others
    const int64_t *sp_ptr;     // SPPMI: symmetric CSR, ascending, no diagonal
    const int32_t *sp_idx;
    const double *sp_val;
    double *G, *wb, *cb;       // context embeddings [n][k], item bias [n], context bias [n]
    double regR;
    int64_t pos0;              // first sched position of the launch (a level)
};

// long rows: one workgroup per chunk of pairs writes its partial sums
__global__ __launch_bounds__(kWrmfThreads) void k_cof_chunk(CofArgs a) {
    __shared__ __attribute__((aligned(16))) float stage[kWrmfStage * kWrmfMaxK];
    __shared__ double sw[kWrmfStage], sw1[kWrmfStage];
    const int tid = (int)threadIdx.x;
    const int64_t c = blockIdx.x;
    const WrmfTiles t = wrmf_tiles(a.w.k);
    double acc[kWrmfTilesPerThread][4][4] = {};
    double bacc = 0.0, lacc = 0.0;
    wrmf_pairs(a.w, t, a.w.cbeg[c], a.w.cend[c], stage, sw, sw1, nullptr, acc, bacc, lacc);
    double *out = a.w.ws + c * kWrmfWsStride;
#pragma unroll
    for (int s = 0; s < kWrmfTilesPerThread; ++s)
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int q = 0; q < 4; ++q) out[(s * 16 + p * 4 + q) * kWrmfThreads + tid] = acc[s][p][q];
    if (tid < kWrmfMaxK) out[kWrmfSlots * kWrmfThreads + tid] = bacc;
}

// one workgroup per row of a level
__global__ __launch_bounds__(kWrmfThreads, 2) void k_cof_solve(CofArgs a) {
    extern __shared__ __attribute__((aligned(16))) double lds_L[];   // wrmf_dyn_lds(k) bytes: staged rows, then packed L
    __shared__ double sw[kWrmfStage], sw1[kWrmfStage], term[kWrmfStage];
    __shared__ double colraw[kWrmfMaxK], colL[kWrmfMaxK], invd[kWrmfMaxK], bvec[kWrmfMaxK];
    __shared__ double gi_old[kWrmfMaxK];
    __shared__ float yi_old[kWrmfMaxK];
    const int tid = (int)threadIdx.x, k = a.w.k;
    const int64_t pos = a.pos0 + blockIdx.x;
    const int32_t row = a.w.sched[pos];
    const int64_t p0 = a.w.ptr[row], p1 = a.w.ptr[row + 1];
    const int64_t q0 = a.sp_ptr[row], q1 = a.sp_ptr[row + 1];
    float *yrow = a.w.X + (int64_t)row * k;
    if (p1 == p0 && q1 == q0) {                           // no pairs, no contexts: b = 0, the row is exactly 0
        if (tid < k) yrow[tid] = 0.0f;
        return;
    }
    if (tid < kWrmfMaxK) {
        yi_old[tid] = tid < k ? yrow[tid] : 0.0f;
        gi_old[tid] = tid < k ? a.G[(int64_t)row * k + tid] : 0.0;
    }
    const double wi = a.wb[row], ci = a.cb[row];
    const WrmfTiles t = wrmf_tiles(k);
    double acc[kWrmfTilesPerThread][4][4] = {};
    double bacc = 0.0, lacc = 0.0;
    const int32_t lp = a.lpos[pos];
    if (lp >= 0) {                                        // long row: the chunks' partials, summed in chunk order
        for (int64_t c = a.w.cptr[lp]; c < a.w.cptr[lp + 1]; ++c) {
            const double *in = a.w.ws + c * kWrmfWsStride;
#pragma unroll
            for (int s = 0; s < kWrmfTilesPerThread; ++s)
#pragma unroll
                for (int p = 0; p < 4; ++p)
#pragma unroll
                    for (int q = 0; q < 4; ++q) acc[s][p][q] += in[(s * 16 + p * 4 + q) * kWrmfThreads + tid];
            if (tid < kWrmfMaxK) bacc += in[kWrmfSlots * kWrmfThreads + tid];
        }
    } else {
        wrmf_pairs(a.w, t, p0, p1, reinterpret_cast<float *>(lds_L), sw, sw1, nullptr, acc, bacc, lacc);
    }
    // the contexts' G rows: A += G_j G_j^T, m1 += (s - w_i - c_j) G_j, the terms of w[i] from the old Y[i]
    double m1 = 0.0, wsum = 0.0;
    for (int64_t e0 = q0; e0 < q1; e0 += kCofStage) {
        const int cnt = (int)((q1 - e0) < kCofStage ? (q1 - e0) : kCofStage);
        __syncthreads();                                  // the previous stage has been consumed (yi_old, gi_old visible)
        for (int e = tid; e < kCofStage * kWrmfMaxK; e += kWrmfThreads) {
            const int r = e >> 7, col = e & 127;
            lds_L[e] = (r < cnt && col < k) ? a.G[(int64_t)a.sp_idx[e0 + r] * k + col] : 0.0;
        }
        if (tid < cnt) sw[tid] = (a.sp_val[e0 + tid] - wi) - a.cb[a.sp_idx[e0 + tid]];
        __syncthreads();
        for (int j = 0; j < cnt; ++j) {
            const double *g = lds_L + j * kWrmfMaxK;
#pragma unroll
            for (int s = 0; s < kWrmfTilesPerThread; ++s) {
                if (t.own[s]) {
                    double xa[4], yb[4];
#pragma unroll
                    for (int p = 0; p < 4; ++p) { xa[p] = g[4 * t.ta[s] + p]; yb[p] = g[4 * t.tb[s] + p]; }
#pragma unroll
                    for (int p = 0; p < 4; ++p)
#pragma unroll
                        for (int q = 0; q < 4; ++q) acc[s][p][q] = fma(xa[p], yb[q], acc[s][p][q]);
                }
            }
        }
        if (tid < k)
            for (int j = 0; j < cnt; ++j) m1 = m1 + sw[j] * lds_L[j * kWrmfMaxK + tid];
        {   // Y_i(old) . G_j: 16 threads per staged row
            const int r = tid >> 4, sub = tid & 15;
            double d = 0.0;
            for (int col = sub; col < k; col += 16) d = fma((double)yi_old[col], lds_L[r * kWrmfMaxK + col], d);
            d += __shfl_xor(d, 1);
            d += __shfl_xor(d, 2);
            d += __shfl_xor(d, 4);
            d += __shfl_xor(d, 8);
            if (sub == 0 && r < cnt) term[r] = (a.sp_val[e0 + r] - d) - a.cb[a.sp_idx[e0 + r]];
        }
        __syncthreads();
        if (tid == 0)
            for (int r = 0; r < cnt; ++r) wsum += term[r];
    }
    // A = (sums + fp32 Gram) + regU on the diagonal
#pragma unroll
    for (int s = 0; s < kWrmfTilesPerThread; ++s)
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                acc[s][p][q] += a.w.G[(s * 16 + p * 4 + q) * kWrmfThreads + tid];
                if (p == q && t.ta[s] == t.tb[s]) acc[s][p][q] += a.w.reg;
            }
    __syncthreads();                                      // the staged rows are dead from here on: lds_L becomes L
    if (tid < kWrmfMaxK) bvec[tid] = tid < k ? bacc + m1 : 0.0;
    __syncthreads();
    if (!als_cholesky_solve(acc, t, k, lds_L, colraw, colL, invd, bvec, yrow)) {
        if (tid == 0) atomicMin(a.w.status, row);
        return;
    }
    if (q1 == q0) return;                                 // no contexts: G[i], w[i], c[i] stay
    // the contexts' Y rows: B = sum Y_j Y_j^T (fp32 products as the reference's float32 outer product, summed in fp64),
    // m2 = sum (s - w_j - c_i) Y_j, the terms of c[i] from the old G[i]
#pragma unroll
    for (int s = 0; s < kWrmfTilesPerThread; ++s)
#pragma unroll
        for (int p = 0; p < 4; ++p)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[s][p][q] = 0.0;
    float *stage = reinterpret_cast<float *>(lds_L);
    double m2 = 0.0, csum = 0.0;
    for (int64_t e0 = q0; e0 < q1; e0 += kWrmfStage) {
        const int cnt = (int)((q1 - e0) < kWrmfStage ? (q1 - e0) : kWrmfStage);
        __syncthreads();                                  // the solve / the previous stage is done with lds_L
        wrmf_stage(a.w.X, k, a.sp_idx, e0, cnt, stage);
        if (tid < cnt) sw[tid] = (a.sp_val[e0 + tid] - a.wb[a.sp_idx[e0 + tid]]) - ci;
        __syncthreads();
        for (int j = 0; j < cnt; ++j) {
            const float *f = stage + j * kWrmfMaxK;
#pragma unroll
            for (int s = 0; s < kWrmfTilesPerThread; ++s) {
                if (t.own[s]) {
                    const float4 fa = *reinterpret_cast<const float4 *>(f + 4 * t.ta[s]);
                    const float4 fb = *reinterpret_cast<const float4 *>(f + 4 * t.tb[s]);
                    const float xa[4] = {fa.x, fa.y, fa.z, fa.w}, yb[4] = {fb.x, fb.y, fb.z, fb.w};
#pragma unroll
                    for (int p = 0; p < 4; ++p)
#pragma unroll
                        for (int q = 0; q < 4; ++q) acc[s][p][q] = acc[s][p][q] + (double)(xa[p] * yb[q]);
                }
            }
        }
        if (tid < k)
            for (int j = 0; j < cnt; ++j) m2 = m2 + sw[j] * (double)stage[j * kWrmfMaxK + tid];
        {   // Y_j . G_i(old): 8 threads per staged row
            const int r = tid >> 3, sub = tid & 7;
            double d = 0.0;
            for (int col = sub; col < k; col += 8) d = fma((double)stage[r * kWrmfMaxK + col], gi_old[col], d);
            d += __shfl_xor(d, 1);
            d += __shfl_xor(d, 2);
            d += __shfl_xor(d, 4);
            if (sub == 0 && r < cnt) term[r] = (a.sp_val[e0 + r] - d) - a.wb[a.sp_idx[e0 + r]];
        }
        __syncthreads();
        if (tid == 0)
            for (int r = 0; r < cnt; ++r) csum += term[r];
    }
#pragma unroll
    for (int s = 0; s < kWrmfTilesPerThread; ++s)
#pragma unroll
        for (int p = 0; p < 4; ++p)
            if (t.ta[s] == t.tb[s]) acc[s][p][p] += a.regR;
    __syncthreads();
    if (tid < kWrmfMaxK) bvec[tid] = tid < k ? m2 : 0.0;
    __syncthreads();
    if (!als_cholesky_solve(acc, t, k, lds_L, colraw, colL, invd, bvec, a.G + (int64_t)row * k)) {
        if (tid == 0) atomicMin(a.w.status, row);
        return;
    }
    if (tid == 0) {
        const double cnt_all = (double)(q1 - q0);
        a.wb[row] = wsum / cnt_all;
        a.cb[row] = csum / cnt_all;
    }
}

}  // namespace yue
