// Song2vec's iteration (recommender/advanced/Song2vec.py:162-189): a biased matrix factorisation by sequential SGD over the
// (user, item, count) steps, then a similarity regulariser over the (track, similar track) pairs.  Host side: s2v_host.hip;
// contract in NumPy: tests/helpers/numpy_song2vec.py; DESIGN.md section 19.
//   step   one wave; lane l holds elements l and l + 64 of a row (k <= 128).  The arithmetic is NumPy's, call by call:
//          rating pass  dot = float32 butterfly of Y[i] * X[u]; rating = fp64(dot + fp32(globalMean)) + Bu[u] + Bi[i];
//                       error = count - rating (fp64); X[u] = fp32(fp64(X[u]) + lr (error fp64(Y[i]) - fp64(fp32(regU) X[u])));
//                       Y[i] likewise from the NEW X[u]; Bu[u] += lr (error - regB bu) with bu = Bu[u] as it was before the
//                       user's first step; Bi[i] += lr (error - regB Bi[i])
//          pair pass    all float32: error2 = fp32(sim) - dot(Y[t1], Y[t2]); c = fp32(0.5 alpha lr) error2;
//                       Y[t1] += c Y[t2]; Y[t2] += c Y[t1] (the new Y[t1])
//          Every product and sum is rounded separately (the library is built without contraction).
//   order  k_s2v_*_level runs the steps of one dependency level, one wave each: two steps of a level share no row, and every
//          step finds what the sequential loop would hand it.  k_s2v_*_seq is that loop: ONE wave walks all steps in order.
//          No atomics in either.
#pragma once
#include "bpr_device.hpp"

namespace yue {

constexpr int kS2vMaxK = 128;
constexpr int kS2vWaves = 4;               // waves (steps) per workgroup of a level launch

struct S2vArgs {
    float *X, *Y;              // [m][k], [n][k]
    double *Bu, *Bi;           // [m], [n]
    const double *bu0;         // [m] Bu as it was when the rating pass began (only a user's own steps change Bu[u])
    int k;
    // rating steps
    const int32_t *su, *si, *cnt;
    // pairs
    const int32_t *t1, *t2;
    const float *sim32;
    const int32_t *order;      // level launches: position -> step (pair); the sequential kernels walk 0 .. count - 1
    int64_t begin, count;
    double lr, regB;
    float ru, ri, gm32, coef32;    // fp32(regU), fp32(regI), fp32(globalMean), fp32(0.5 alpha lr)
    double *err2;              // per step (pair): the squared error
};

__device__ __forceinline__ double s2v_lane0(double v) { return __shfl(v, 0); }

template <int KR>
__device__ __forceinline__ void s2v_rate(const S2vArgs &a, int64_t t, int lane) {
    const int64_t u = a.su[t], i = a.si[t];
    const int k = a.k;
    float x[KR], y[KR];
#pragma unroll
    for (int r = 0; r < KR; ++r) {
        const int e = 64 * r + lane;
        x[r] = e < k ? a.X[u * k + e] : 0.0f;
        y[r] = e < k ? a.Y[i * k + e] : 0.0f;
    }
    float acc = 0.0f;
#pragma unroll
    for (int r = 0; r < KR; ++r) { const float m = y[r] * x[r]; acc = acc + m; }
    const float dot = wave_sum(acc);
    // lane 0 reads and writes the biases (one thread: its own stores are visible to its later loads), the others get copies
    double bu = 0.0, bi = 0.0, stale = 0.0;
    if (lane == 0) { bu = a.Bu[u]; bi = a.Bi[i]; stale = a.bu0[u]; }
    bu = s2v_lane0(bu); bi = s2v_lane0(bi); stale = s2v_lane0(stale);
    const float base = dot + a.gm32;
    const double r1 = (double)base + bu;
    const double rating = r1 + bi;
    const double err = (double)a.cnt[t] - rating;
#pragma unroll
    for (int r = 0; r < KR; ++r) {
        const float reg = a.ru * x[r];
        const double g = err * (double)y[r];
        const double d = g - (double)reg;
        const double step = a.lr * d;
        x[r] = (float)((double)x[r] + step);
    }
#pragma unroll
    for (int r = 0; r < KR; ++r) {
        const float reg = a.ri * y[r];
        const double g = err * (double)x[r];
        const double d = g - (double)reg;
        const double step = a.lr * d;
        y[r] = (float)((double)y[r] + step);
    }
#pragma unroll
    for (int r = 0; r < KR; ++r) {
        const int e = 64 * r + lane;
        if (e < k) { a.X[u * k + e] = x[r]; a.Y[i * k + e] = y[r]; }
    }
    if (lane == 0) {
        const double pu = a.regB * stale, du = err - pu, su = a.lr * du;
        const double pi = a.regB * bi, di = err - pi, si = a.lr * di;
        a.Bu[u] = bu + su;
        a.Bi[i] = bi + si;
        a.err2[t] = err * err;
    }
}

template <int KR>
__device__ __forceinline__ void s2v_pair(const S2vArgs &a, int64_t p, int lane) {
    const int64_t t1 = a.t1[p], t2 = a.t2[p];
    const int k = a.k;
    float y1[KR], y2[KR];
#pragma unroll
    for (int r = 0; r < KR; ++r) {
        const int e = 64 * r + lane;
        y1[r] = e < k ? a.Y[t1 * k + e] : 0.0f;
        y2[r] = e < k ? a.Y[t2 * k + e] : 0.0f;
    }
    float acc = 0.0f;
#pragma unroll
    for (int r = 0; r < KR; ++r) { const float m = y1[r] * y2[r]; acc = acc + m; }
    const float err = a.sim32[p] - wave_sum(acc);
    const float c = a.coef32 * err;
#pragma unroll
    for (int r = 0; r < KR; ++r) { const float d = c * y2[r]; y1[r] = y1[r] + d; }
#pragma unroll
    for (int r = 0; r < KR; ++r) { const float d = c * y1[r]; y2[r] = y2[r] + d; }
#pragma unroll
    for (int r = 0; r < KR; ++r) {
        const int e = 64 * r + lane;
        if (e < k) { a.Y[t1 * k + e] = y1[r]; a.Y[t2 * k + e] = y2[r]; }
    }
    if (lane == 0) { const float sq = err * err; a.err2[p] = (double)sq; }
}

template <int KR, bool PAIRS>
__global__ void __launch_bounds__(64 * kS2vWaves) k_s2v_level(S2vArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t x = (int64_t)blockIdx.x * kS2vWaves + (threadIdx.x >> 6);
    if (x >= a.count) return;              // whole waves leave: wave_sum below runs with all 64 lanes
    const int64_t t = a.order[a.begin + x];
    if (PAIRS) s2v_pair<KR>(a, t, lane); else s2v_rate<KR>(a, t, lane);
}

template <int KR, bool PAIRS>
__global__ void __launch_bounds__(64) k_s2v_seq(S2vArgs a) {
    const int lane = threadIdx.x;
    for (int64_t t = 0; t < a.count; ++t) {
        if (PAIRS) s2v_pair<KR>(a, t, lane); else s2v_rate<KR>(a, t, lane);
    }
}

}  // namespace yue
