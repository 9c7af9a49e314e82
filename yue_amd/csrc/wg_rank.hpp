// The workgroup machinery of the ranking kernels, written once: an inclusive scan and its segment lookup, a bitonic
// sort over LDS entries, the (score descending, key ascending) order, and the re-form step of a running top list.
// Device-only and stateless: every kernel keeps its own LDS arrays and hands in lambdas over flat indices.
//   k_knn_neighbors (knn_kernels.hpp)   wg_scan, wg_segment_of, wg_reform (order: knn_better, its own integer ratio)
//   k_knn_topn      (knn_kernels.hpp)   wg_scan, wg_segment_of, wg_pow2 + wg_bitonic (gather keys), wg_reform + wg_before (selection)
//   k_ipf_rank      (ipf_kernels.hpp)   wg_scan, wg_segment_of (both on int64_t), wg_reform + wg_before
//   k_cnet_friends  (cnet_kernels.hpp)  wg_bitonic over its eight lists at once, wg_before; it pads and truncates itself
// Every thread of the workgroup must reach wg_scan, wg_bitonic and wg_reform: they hold barriers.
#pragma once
#include <hip/hip_runtime.h>

namespace yue {

// inclusive scan of one value per thread over the workgroup; returns the total (all threads)
template <int THREADS, class T>
__device__ inline T wg_scan(T x, T *incl) {
    const int t = threadIdx.x;
    incl[t] = x;
    __syncthreads();
    for (int off = 1; off < THREADS; off <<= 1) {
        const T y = t >= off ? incl[t - off] : 0;
        __syncthreads();
        incl[t] += y;
        __syncthreads();
    }
    return incl[THREADS - 1];
}

// flattened position f of the concatenated segments -> segment index (smallest j with incl[j] > f)
template <int THREADS, class T>
__device__ inline int wg_segment_of(const T *incl, T f) {
    int lo = 0, hi = THREADS - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (incl[mid] > f) hi = mid; else lo = mid + 1;
    }
    return lo;
}

__device__ inline int wg_pow2(int x) {
    int p = 1;
    while (p < x) p <<= 1;
    return p;
}

// (score descending, key ascending): a strict total order where the keys are distinct.  Written without short circuit:
// with || and && the compiler loads the second key from LDS only after the scores have compared equal, a second round trip
// per compare-exchange on every tie -- and the sentinel tail of a padded list is all ties.
template <class Key>
__device__ inline bool wg_before(double s1, Key k1, double s2, Key k2) {
    return (s1 > s2) | ((s1 == s2) & (k1 < k2));
}

// bitonic sort of `lists` lists of P (a power of two) LDS entries each, stored back to back: every list on its own,
// ascending by less(x, y) over flat indices; ends with a barrier.  The xor partners stay inside a list (j < P), and the
// direction of a stage comes from the index inside the list: x & k alone would flip the last stage of every odd list.
template <int THREADS, class Less, class Swap>
__device__ inline void wg_bitonic(int lists, int P, Less less, Swap swap) {
    const int n = lists * P;
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int x = threadIdx.x; x < n; x += THREADS) {
                const int ixj = x ^ j;
                if (ixj > x) {
                    const bool up = ((x & (P - 1)) & k) == 0;
                    if (up ? less(ixj, x) : less(x, ixj)) swap(x, ixj);
                }
            }
            __syncthreads();
        }
}

// Re-forms a running top list: entries [0, nl) are the list, [nl, nl + nc) the block appended behind it.  Pads up to the
// next power of two with the caller's sentinel (pad(i): behind every entry by `less`), sorts, keeps the best K.  The caller
// re-forms before a batch of appends could pass its LDS capacity (capacity >= K + batch, a power of two) and once at the
// end; it appends an entry only while nl < K or the entry is before entry K - 1.  nl and nc live in LDS.
template <int THREADS, class Pad, class Less, class Swap>
__device__ inline void wg_reform(int &nl, int &nc, int K, Pad pad, Less less, Swap swap) {
    __syncthreads();
    const int tot = nl + nc;
    const int P = wg_pow2(tot);
    for (int i = tot + threadIdx.x; i < P; i += THREADS) pad(i);
    __syncthreads();
    wg_bitonic<THREADS>(1, P, less, swap);
    if (threadIdx.x == 0) { nl = tot < K ? tot : K; nc = 0; }
    __syncthreads();
}

}  // namespace yue
