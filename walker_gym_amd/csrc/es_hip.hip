// es_hip.hip — evolution strategies on the device: wg_es_perturb and wg_es_update of include/walker_hip.h.
//
// A translation unit of its own, linked into libwalker_hip.so beside walker_hip.hip with the same flags, so that the
// step kernels' register allocation does not depend on anything here.
//
// The noise is never stored: eps(seed, generation, pair, k) is one Philox4x32-10 call, an integer function of its
// four arguments, so the update kernel regenerates what the perturb kernel added.  Both kernels are integer VALU work
// (about 90 instructions per Philox call); perturb also writes n_sets * K floats once.
//   es_perturb         one thread per (pair, k), k fastest (blockIdx.x the pairs, blockIdx.y blocks of 256 parameters):
//                      theta[k] +- RN32(sigma * eps) into sets 2j and 2j + 1 of the four weight tensors wg_policy
//                      reads (coalesced stores of 4 B per lane in each of the two sets)
//   es_update_partial  one thread per (chunk of 256 pairs, k): the chunk's float64 partial sum, pairs ascending
//   es_update_tail     one thread per k: the chunks' partials added in ascending order, scale, the float32 step
// The summation order is the contract (no atomics).  Every element offset is 64-bit.

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "walker_hip.h"
#include "walker_internal.h"   // wg_fail, wg_launched: the refusals here go to the library's one error message
#include "wg_philox.h"         // wg_eps: the one definition of the noise, shared with the action noise of walker_hip.hip

namespace {

constexpr int ES_THREADS = 256;
constexpr int ES_CHUNK = 256;             // pairs per float64 partial sum (the contract's chunk)
constexpr int64_t ES_MAX_K = (int64_t)1 << 23;   // parameters: blockIdx.y counts blocks of 256 of them (at most 65,535)

// The four segments of theta: element counts (0 for an absent one) and the candidate tensors.
struct EsLayout {
    int32_t n_w1, n_b1, n_w2, n_b2;
    float *w1, *b1, *w2, *b2;
};

// Pairs [first_pair, first_pair + n_pairs).  blockIdx.x is a row of ppb pairs, blockIdx.y a block of 256 values of k:
//   ppb == 1 (K >= 256): one pair per row
//   ppb  > 1 (K < 256):  a row covers ppb = 256 / K whole pairs, lane t holds (pair t / K, element t % K)
__global__ __launch_bounds__(ES_THREADS) void es_perturb(EsLayout lay, const float *__restrict__ theta, int32_t K,
                                                         int32_t ppb, uint32_t k0, uint32_t k1, uint32_t generation,
                                                         float sigma, int32_t first_pair, int32_t n_pairs) {
    int32_t pl = 0, k;
    if (ppb > 1) {
        pl = (int32_t)threadIdx.x / K;
        k = (int32_t)threadIdx.x - pl * K;
        if (pl >= ppb) return;
    } else {
        k = (int32_t)(blockIdx.y * ES_THREADS + threadIdx.x);
        if (k >= K) return;
    }
    const int32_t jl = (int32_t)blockIdx.x * ppb + pl;   // < n_pairs + ppb <= 2^30 + 256
    if (jl >= n_pairs) return;
    // the element's tensor, its offset inside a set and the set stride (k is fixed for the thread)
    float *dst;
    int64_t stride;
    int32_t off = k;
    if (off < lay.n_w1) {
        dst = lay.w1; stride = lay.n_w1;
    } else if ((off -= lay.n_w1) < lay.n_b1) {
        dst = lay.b1; stride = lay.n_b1;
    } else if ((off -= lay.n_b1) < lay.n_w2) {
        dst = lay.w2; stride = lay.n_w2;
    } else {
        off -= lay.n_w2;
        dst = lay.b2; stride = lay.n_b2;
    }
    dst += off;
    const int32_t j = first_pair + jl;
    const float th = theta[k];
    const float d = __fmul_rn(sigma, wg_eps<WG_ES_TAG>(k0, k1, generation, (uint32_t)j, (uint32_t)k));
    float *p = dst + 2 * (int64_t)j * stride;
    p[0] = __fadd_rn(th, d);
    p[stride] = __fsub_rn(th, d);
}

// partial[c][k] = sum over the chunk's pairs, ascending, of (double)d_j * (double)eps_j[k], d_j = RN32(util[2j] -
// util[2j + 1]).  The product of two float32 values is exact in float64; each addition rounds once.
__global__ __launch_bounds__(ES_THREADS) void es_update_partial(const float *__restrict__ util,
                                                                double *__restrict__ partial, int32_t K, uint32_t k0,
                                                                uint32_t k1, uint32_t generation, int32_t first_pair,
                                                                int32_t n_pairs) {
    const int32_t k = (int32_t)(blockIdx.y * ES_THREADS + threadIdx.x);
    if (k >= K) return;
    const int32_t c = (int32_t)blockIdx.x;   // the chunk: pairs [a, b) of the range
    const int32_t a = c * ES_CHUNK, b = (n_pairs - a < ES_CHUNK) ? n_pairs : a + ES_CHUNK;
    double acc = 0.0;
    for (int32_t jl = a; jl < b; ++jl) {
        const int64_t j = (int64_t)first_pair + jl;
        const float d = __fsub_rn(util[2 * j], util[2 * j + 1]);
        const float e = wg_eps<WG_ES_TAG>(k0, k1, generation, (uint32_t)j, (uint32_t)k);
        acc = __dadd_rn(acc, __dmul_rn((double)d, (double)e));
    }
    partial[(int64_t)c * K + k] = acc;
}

// S = the partials added in chunk order; grad = RN32(RN64(S * scale)); theta_out = RN32(theta + RN32(lr * grad)).
// theta_out may be theta: each thread reads its own element before it writes it.
__global__ __launch_bounds__(ES_THREADS) void es_update_tail(const double *__restrict__ partial, const float *theta,
                                                             float *grad, float *theta_out, int32_t K, int32_t n_chunks,
                                                             double scale, float lr) {
    const int32_t k = (int32_t)(blockIdx.x * ES_THREADS + threadIdx.x);
    if (k >= K) return;
    double s = 0.0;
    for (int32_t c = 0; c < n_chunks; ++c) s = __dadd_rn(s, partial[(int64_t)c * K + k]);
    const float g = (float)__dmul_rn(s, scale);
    if (grad) grad[k] = g;
    if (theta_out) theta_out[k] = __fadd_rn(theta[k], __fmul_rn(lr, g));
}

// The checks that wg_es_perturb and wg_es_update share; fills the layout and K.
int es_check(const wg_es *es, int32_t first_pair, int32_t n_pairs, const char *who, EsLayout *lay, int64_t *K) {
    if (!es) return wg_fail(WG_EINVAL, "%s: null es", who);
    if (!es->theta) return wg_fail(WG_EINVAL, "%s: null theta", who);
    if (es->obs_dim < 1) return wg_fail(WG_EINVAL, "%s: obs_dim %d < 1", who, es->obs_dim);
    if (es->act_dim < 1) return wg_fail(WG_EINVAL, "%s: act_dim %d < 1", who, es->act_dim);
    if (es->hidden < 0 || es->hidden > 256) return wg_fail(WG_EINVAL, "%s: hidden %d outside 0..256", who, es->hidden);
    if (es->hidden > 0 && !es->w1) return wg_fail(WG_EINVAL, "%s: hidden %d with a null w1", who, es->hidden);
    if (es->hidden == 0 && es->b1) return wg_fail(WG_EINVAL, "%s: b1 without a hidden layer", who);
    if (!es->w2) return wg_fail(WG_EINVAL, "%s: null w2", who);
    if (es->n_sets < 2 || (es->n_sets & 1))
        return wg_fail(WG_EINVAL, "%s: n_sets %d must be even and >= 2 (antithetic pairs)", who, es->n_sets);
    if (n_pairs < 1) return wg_fail(WG_EINVAL, "%s: n_pairs %d < 1", who, n_pairs);
    if (first_pair < 0 || first_pair > es->n_sets / 2 - n_pairs)
        return wg_fail(WG_EINVAL, "%s: pairs %d .. %lld outside 0 .. %d", who, first_pair,
                    (long long)first_pair + n_pairs, es->n_sets / 2);
    if (!std::isfinite(es->sigma) || !(es->sigma > 0.0f)) return wg_fail(WG_EINVAL, "%s: sigma must be finite and > 0", who);
    const int64_t H = es->hidden, D = es->obs_dim, C = es->act_dim;
    const int64_t n_w1 = D * H, n_b1 = es->b1 ? H : 0, n_w2 = (H > 0 ? H : D) * C, n_b2 = es->b2 ? C : 0;
    *K = n_w1 + n_b1 + n_w2 + n_b2;
    if (*K > ES_MAX_K) return wg_fail(WG_EINVAL, "%s: %lld parameters (at most 2^23)", who, (long long)*K);
    lay->n_w1 = (int32_t)n_w1; lay->n_b1 = (int32_t)n_b1; lay->n_w2 = (int32_t)n_w2; lay->n_b2 = (int32_t)n_b2;
    lay->w1 = es->w1; lay->b1 = es->b1; lay->w2 = es->w2; lay->b2 = es->b2;
    return 0;
}

}  // namespace

extern "C" {

int wg_es_perturb(const wg_es *es, int32_t first_pair, int32_t n_pairs, hipStream_t stream) {
    EsLayout lay;
    int64_t K64;
    if (const int rc = es_check(es, first_pair, n_pairs, "wg_es_perturb", &lay, &K64)) return rc;
    const int32_t K = (int32_t)K64;
    const int32_t ppb = K >= ES_THREADS ? 1 : ES_THREADS / K;
    const int32_t rows = (n_pairs + ppb - 1) / ppb;
    const dim3 grid(rows, ppb > 1 ? 1 : (K + ES_THREADS - 1) / ES_THREADS);
    es_perturb<<<grid, ES_THREADS, 0, stream>>>(lay, es->theta, K, ppb, (uint32_t)(es->seed & 0xffffffffu),
                                               (uint32_t)(es->seed >> 32), es->generation, es->sigma, first_pair,
                                               n_pairs);
    return wg_launched("wg_es_perturb: launch");
}

int wg_es_update(const wg_es *es, int32_t first_pair, int32_t n_pairs, const float *util, double scale, float lr,
                 double *workspace, float *grad, float *theta_out, hipStream_t stream) {
    EsLayout lay;
    int64_t K64;
    if (const int rc = es_check(es, first_pair, n_pairs, "wg_es_update", &lay, &K64)) return rc;
    if (!util) return wg_fail(WG_EINVAL, "wg_es_update: null util");
    if (!workspace) return wg_fail(WG_EINVAL, "wg_es_update: null workspace");
    if (!std::isfinite(scale)) return wg_fail(WG_EINVAL, "wg_es_update: scale is not finite");
    if (!std::isfinite(lr)) return wg_fail(WG_EINVAL, "wg_es_update: lr is not finite");
    if (!grad && !theta_out) return wg_fail(WG_EINVAL, "wg_es_update: grad and theta_out are both null");
    const int32_t K = (int32_t)K64;
    const int32_t n_chunks = (n_pairs + ES_CHUNK - 1) / ES_CHUNK, kb = (K + ES_THREADS - 1) / ES_THREADS;
    es_update_partial<<<dim3(n_chunks, kb), ES_THREADS, 0, stream>>>(
        util, workspace, K, (uint32_t)(es->seed & 0xffffffffu), (uint32_t)(es->seed >> 32), es->generation, first_pair,
        n_pairs);
    if (const int rc = wg_launched("wg_es_update (partial sums): launch")) return rc;
    es_update_tail<<<kb, ES_THREADS, 0, stream>>>(workspace, es->theta, grad, theta_out, K, n_chunks, scale, lr);
    return wg_launched("wg_es_update (tail): launch");
}

}  // extern "C"
