// wg_philox.h — the counter-based noise of include/walker_hip.h, one definition for every unit that draws it:
// es_hip.hip (the ES perturbation eps, counter domain WG_ES_TAG) and walker_hip.hip (the action noise aeps of
// wg_rollout_stochastic, counter domain WG_ACT_TAG).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

constexpr uint32_t WG_ES_TAG = 0x45530001u;    // counter word 3 of eps(seed, generation, j, k)
constexpr uint32_t WG_ACT_TAG = 0x41430001u;   // counter word 3 of aeps(seed, t, w, c)

// Philox4x32-10 on the counter (x, y, z, TAG) under the key (k0, k1) = (seed lo, seed hi); the eight 16-bit halves of the
// four output words added, centred and scaled to unit variance (Irwin-Hall(8)).
//   eps(seed, generation, j, k) = wg_eps<WG_ES_TAG>(k0, k1, generation, j, k)
//   aeps(seed, t, w, c)         = wg_eps<WG_ACT_TAG>(k0, k1, t, w, c)
template <uint32_t TAG>
__device__ __forceinline__ float wg_eps(uint32_t k0, uint32_t k1, uint32_t z, uint32_t y, uint32_t x) {
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
    uint32_t c0 = x, c1 = y, c2 = z, c3 = TAG;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t h0 = __umulhi(M0, c0), l0 = M0 * c0, h1 = __umulhi(M1, c2), l1 = M1 * c2;
        c0 = h1 ^ c1 ^ k0;
        c1 = l1;
        c2 = h0 ^ c3 ^ k1;
        c3 = l0;
        k0 += W0;
        k1 += W1;
    }
    const int32_t s = (int32_t)((c0 & 0xffffu) + (c0 >> 16) + (c1 & 0xffffu) + (c1 >> 16) + (c2 & 0xffffu) + (c2 >> 16) +
                                (c3 & 0xffffu) + (c3 >> 16));
    return __fmul_rn((float)(s - 262140), __uint_as_float(0x379CC471u));   // |s - 262140| < 2^24: the cast is exact
}
