// pg_hip.hip — policy-gradient support on the device: wg_gae of include/walker_hip.h.
//
// A translation unit of its own, linked into libwalker_hip.so beside walker_hip.hip and es_hip.hip with the same flags,
// so that the step kernels' register allocation does not depend on anything here.
//
//   gae_scan   one thread per walker, t descending.  A step's five loads (reward, value, next_value, term, cut) are
//              4-B / 1-B per lane and contiguous across the walkers of a wave; none depends on the chain (the carried
//              advantage), so the loads of the next GAE_U steps are issued before the chain runs over the GAE_U steps
//              already in registers: with vmcnt counting in order the chain waits for its own block only, and 5 * GAE_U
//              loads per lane stay in flight behind it.  Six dependent float32 operations per step, no FMA
//              (-ffp-contract=off, and the intrinsics round once each).  Every element offset is 64-bit.

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "walker_hip.h"
#include "walker_internal.h"   // wg_fail, wg_launched: the refusals here go to the library's one error message

namespace {

constexpr int GAE_THREADS = 64;   // one wave per workgroup: N = 4,096 walkers spread over 64 CUs, 65,536 over all
constexpr int GAE_U = 8;          // steps per block of loads

struct GaeIn {
    float r, v, nv;
    uint32_t tm, ct;
};

// Steps t_hi, t_hi - 1, ... of walker w into x[0..GAE_U); a step below 0 loads step 0 again (a valid address; unused).
template <bool TERM, bool CUT>
__device__ __forceinline__ void gae_load(GaeIn (&x)[GAE_U], const float *__restrict__ reward,
                                         const float *__restrict__ value, const float *__restrict__ next_value,
                                         const uint8_t *__restrict__ term, const uint8_t *__restrict__ cut, int t_hi,
                                         int64_t stride, int w) {
#pragma unroll
    for (int k = 0; k < GAE_U; k++) {
        const int t = t_hi - k > 0 ? t_hi - k : 0;
        const int64_t at = (int64_t)t * stride + w;
        x[k].r = reward[at];
        x[k].v = value[at];
        x[k].nv = next_value[at];
        x[k].tm = TERM ? term[at] : 0u;
        x[k].ct = CUT ? cut[at] : 0u;
    }
}

template <bool TERM, bool CUT>
__global__ __launch_bounds__(GAE_THREADS) void gae_scan(const float *__restrict__ reward, const float *__restrict__ value,
                                                        const float *__restrict__ next_value,
                                                        const uint8_t *__restrict__ term, const uint8_t *__restrict__ cut,
                                                        int n_steps, int N, int64_t stride, float gamma, float gl,
                                                        float *__restrict__ adv, float *__restrict__ ret) {
    const int w = (int)(blockIdx.x * GAE_THREADS + threadIdx.x);
    if (w >= N) return;
    GaeIn cur[GAE_U], nxt[GAE_U];
    float carry = 0.f;
    gae_load<TERM, CUT>(cur, reward, value, next_value, term, cut, n_steps - 1, stride, w);
    for (int t_hi = n_steps - 1; t_hi >= 0; t_hi -= GAE_U) {
        // (the next block's loads first; past the first step they reload step 0 and are dropped)
        gae_load<TERM, CUT>(nxt, reward, value, next_value, term, cut, t_hi - GAE_U, stride, w);
#pragma unroll
        for (int k = 0; k < GAE_U; k++) {
            const int t = t_hi - k;
            if (t < 0) break;
            const float nv = cur[k].tm ? 0.f : cur[k].nv;
            const float delta = __fsub_rn(__fadd_rn(cur[k].r, __fmul_rn(gamma, nv)), cur[k].v);
            const float c = cur[k].ct ? 0.f : carry;
            carry = __fadd_rn(delta, __fmul_rn(gl, c));
            const int64_t at = (int64_t)t * stride + w;
            adv[at] = carry;
            if (ret) ret[at] = __fadd_rn(carry, cur[k].v);
        }
#pragma unroll
        for (int k = 0; k < GAE_U; k++) cur[k] = nxt[k];
    }
}

// [p, p + bytes) of an array of `elem`-byte elements, [n_steps][N] with `stride` elements between steps
struct Span {
    uintptr_t lo, hi;
};
Span span_of(const void *p, int n_steps, int N, int64_t stride, int elem) {
    const uintptr_t lo = reinterpret_cast<uintptr_t>(p);
    return Span{lo, lo + (uintptr_t)(((int64_t)(n_steps - 1) * stride + N) * elem)};
}
bool overlap(const Span &a, const Span &b) { return a.lo < b.hi && b.lo < a.hi; }

}  // namespace

extern "C" {

int wg_gae(const float *reward, const float *value, const float *next_value, const uint8_t *term, const uint8_t *cut,
           int32_t n_steps, int32_t N, int64_t step_stride, float gamma, float lam, float *adv, float *ret,
           hipStream_t stream) {
    if (!reward) return wg_fail(WG_EINVAL, "wg_gae: null reward");
    if (!value) return wg_fail(WG_EINVAL, "wg_gae: null value");
    if (!next_value) return wg_fail(WG_EINVAL, "wg_gae: null next_value");
    if (!adv) return wg_fail(WG_EINVAL, "wg_gae: null adv");
    if (n_steps < 1) return wg_fail(WG_EINVAL, "wg_gae: n_steps %d < 1", n_steps);
    if (N < 1) return wg_fail(WG_EINVAL, "wg_gae: N %d < 1", N);
    if (step_stride < N) return wg_fail(WG_EINVAL, "wg_gae: step_stride %lld < N = %d", (long long)step_stride, N);
    if (!std::isfinite(gamma)) return wg_fail(WG_EINVAL, "wg_gae: gamma is not finite");
    if (!std::isfinite(lam)) return wg_fail(WG_EINVAL, "wg_gae: lam is not finite");
    const struct { const char *name; const void *p; int elem; } in[] = {
        {"reward", reward, 4}, {"value", value, 4}, {"next_value", next_value, 4}, {"term", term, 1}, {"cut", cut, 1}};
    const Span sa = span_of(adv, n_steps, N, step_stride, 4);
    for (const auto &i : in) {
        if (!i.p) continue;
        const Span si = span_of(i.p, n_steps, N, step_stride, i.elem);
        if (overlap(sa, si)) return wg_fail(WG_EINVAL, "wg_gae: adv aliases %s", i.name);
        if (ret && overlap(span_of(ret, n_steps, N, step_stride, 4), si))
            return wg_fail(WG_EINVAL, "wg_gae: ret aliases %s", i.name);
    }
    if (ret && overlap(sa, span_of(ret, n_steps, N, step_stride, 4)))
        return wg_fail(WG_EINVAL, "wg_gae: adv aliases ret");
    const float gl = gamma * lam;   // one float32 multiply (-ffp-contract=off)
    const dim3 grid((N + GAE_THREADS - 1) / GAE_THREADS);
    auto go = [&](auto kernel) {
        kernel<<<grid, GAE_THREADS, 0, stream>>>(reward, value, next_value, term, cut, n_steps, N, step_stride, gamma, gl,
                                                 adv, ret);
    };
    if (term && cut) go(gae_scan<true, true>);
    else if (term) go(gae_scan<true, false>);
    else if (cut) go(gae_scan<false, true>);
    else go(gae_scan<false, false>);
    return wg_launched("wg_gae: launch");
}

}  // extern "C"
