// The counter hash shared by the user-network stage (cnet_kernels.hpp: walks, shuffle, init, sub-sampling, windows, negatives)
// and NGCF's dropout mask (ngcf_kernels.hpp): a pure function of a stream seed and four counters, the same on host and device.
// No kernel is defined here, so any translation unit may include it.
#pragma once
#include <cstdint>

#include <hip/hip_runtime.h>

namespace yue {

// 64 uniform bits for the counter (a, b, c, d) of stream `seed`: bpr_device.hpp's mix64, chained as ctr_draw chains it
__host__ __device__ inline uint64_t cnet_mix(uint64_t z) {
    z ^= z >> 30; z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27; z *= 0x94D049BB133111EBull;
    z ^= z >> 31; return z;
}
__host__ __device__ inline uint64_t cnet_hash(uint64_t seed, uint64_t a, uint64_t b, uint64_t c, uint64_t d) {
    uint64_t z = cnet_mix(seed + 0x9E3779B97F4A7C15ull * (a + 1));
    z = cnet_mix(z ^ (0xD1B54A32D192ED03ull * (b + 1) + 0x8CB92BA72F3D8DD7ull * c));
    return cnet_mix(z ^ (0xA0761D6478BD642Full * (d + 1)));
}

}  // namespace yue
