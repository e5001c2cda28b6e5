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
// and, with one standard deviation per parameter (wg_es_perturb_diag / wg_es_update_diag, PGPE with symmetric sampling):
//   es_perturb_diag    es_perturb's thread mapping with sigma[k] loaded beside theta[k]
//   es_diag_partial_spread  one workgroup per (chunk of 256 pairs, block of 32 parameters): four waves compute the
//                      chunk's terms (Philox, the products) into an LDS tile of 64 pairs while a fifth adds the previous
//                      tile's in pair order, lanes 0..31 the chain of the mean and lanes 32..63 the chain of sigma
//   es_diag_partial_thread  one thread per (chunk, k) walking both chains; the same bits (chosen for large launches)
//   es_diag_tail       one thread per k: both chunk-ordered sums, the scales, the division, the two steps, the clamp
// and for a policy with a second hidden layer (wg_es_mid: theta's six segments w1, b1, wm, bm, w2, b2):
//   es_perturb_deep, es_perturb_diag_deep  es_perturb's rows and lanes; es_deep_slot resolves the six segments for both
// The deep update entries launch the update kernels above: those depend on the layout through K alone.
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

// ---------------------------------------------------------------------------------------------- per-parameter sigma
// es_diag_partial has two forms with the same bits, chosen by the launch's size (wg_es_update_diag):
//   es_diag_partial_spread  a workgroup spreads a chunk's terms over four waves: small populations, where one thread
//                           per (chunk, k) leaves the chip idle behind 256 dependent Philox calls
//   es_diag_partial_thread  one thread per (chunk, k) walking both chains: once its grid has a workgroup for every CU
constexpr int DG_KB = 32;                      // parameters per workgroup of the spread form
constexpr int DG_TILE = 64;                    // pairs per LDS tile
constexpr int DG_FILL = 256;                   // threads that compute terms (four waves); one more wave adds them
constexpr int DG_THREADS = DG_FILL + 64;
constexpr int DG_AHEAD = 16;                   // rows the adding wave reads ahead of its chain
constexpr int DG_MAX_KBLOCKS = 65535;          // gridDim.y; a workgroup strides over the blocks of k beyond it
constexpr int64_t DG_THREAD_FORM_GROUPS = 256; // workgroups of the one-thread form (chunks x blocks of 256 k) from which
                                               // it is launched: one per CU (DESIGN 9g has the measurement)

// es_perturb with d = RN32(sigma[k] * eps): the same rows, the same lanes.
__global__ __launch_bounds__(ES_THREADS) void es_perturb_diag(EsLayout lay, const float *__restrict__ theta,
                                                              const float *__restrict__ sigma, int32_t K, int32_t ppb,
                                                              uint32_t k0, uint32_t k1, uint32_t generation,
                                                              int32_t first_pair, int32_t n_pairs) {
    int32_t pl = 0, k;
    if (ppb > 1) {
        pl = (int32_t)threadIdx.x / K;
        k = (int32_t)threadIdx.x - pl * K;
        if (pl >= ppb) return;
    } else {
        k = (int32_t)(blockIdx.y * ES_THREADS + threadIdx.x);
        if (k >= K) return;
    }
    const int32_t jl = (int32_t)blockIdx.x * ppb + pl;
    if (jl >= n_pairs) return;
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
    const float d = __fmul_rn(sigma[k], wg_eps<WG_ES_TAG>(k0, k1, generation, (uint32_t)j, (uint32_t)k));
    float *p = dst + 2 * (int64_t)j * stride;
    p[0] = __fadd_rn(th, d);
    p[stride] = __fsub_rn(th, d);
}

// The two terms of pair j at parameter k: tm = (double)dm_j * (double)d (exact), ts = RN64((double)ds_j * q),
// q = RN64((double)d * (double)d - ss), ss = (double)sigma[k] * (double)sigma[k] (both products exact).
__device__ __forceinline__ void es_diag_terms(const float *__restrict__ util, float base, int64_t j, float sg, double ss,
                                              uint32_t k0, uint32_t k1, uint32_t generation, int32_t k, double *tm,
                                              double *ts) {
    const float u0 = util[2 * j], u1 = util[2 * j + 1];
    const float dm = __fsub_rn(u0, u1);
    const float ds = __fsub_rn(__fmul_rn(__fadd_rn(u0, u1), 0.5f), base);
    const double d = (double)__fmul_rn(sg, wg_eps<WG_ES_TAG>(k0, k1, generation, (uint32_t)j, (uint32_t)k));
    *tm = __dmul_rn((double)dm, d);
    *ts = __dmul_rn((double)ds, __dsub_rn(__dmul_rn(d, d), ss));
}

// partial[0][c][k] and partial[1][c][k]: the chunk's ordered sums of tm and ts.  blockIdx.x is the chunk, blockIdx.y a
// block of 32 values of k.  Threads 0..255 (lane t & 31 the parameter, t >> 5 a row of eight) fill tile i of 64 pairs,
// [row][0..31] tm and [row][32..63] ts, while the fifth wave adds tile i - 1 row by row (a row is 64 consecutive
// doubles: conflict-free 8-byte reads); the two tiles alternate, one barrier per tile.
__global__ __launch_bounds__(DG_THREADS) void es_diag_partial_spread(const float *__restrict__ util,
                                                              const float *__restrict__ sigma,
                                                              double *__restrict__ partial, int32_t K, int32_t kblocks,
                                                              uint32_t k0, uint32_t k1, uint32_t generation,
                                                              int32_t first_pair, int32_t n_pairs, float base) {
    __shared__ double tile[2][DG_TILE][2 * DG_KB];
    const int32_t c = (int32_t)blockIdx.x, n_chunks = (int32_t)gridDim.x;
    const int32_t a = c * ES_CHUNK, n = (n_pairs - a < ES_CHUNK) ? n_pairs - a : ES_CHUNK;   // the chunk's pairs
    const int32_t n_tiles = (n + DG_TILE - 1) / DG_TILE;
    const int32_t t = (int32_t)threadIdx.x;
    const bool filler = t < DG_FILL;
    const int32_t lane = t & 63, kl = t & (DG_KB - 1), r0 = t >> 5;
    for (int32_t kb = (int32_t)blockIdx.y; kb < kblocks; kb += (int32_t)gridDim.y) {   // uniform in the workgroup
        const int32_t k = kb * DG_KB + kl;     // a filler's parameter, and the adder's (lanes 32..63: the same k)
        const bool live = k < K;
        float sg = 0.0f;
        double ss = 0.0, acc = 0.0;
        if (filler && live) {
            sg = sigma[k];
            ss = __dmul_rn((double)sg, (double)sg);
        }
        for (int32_t i = 0; i <= n_tiles; ++i) {
            if (filler) {
                if (i < n_tiles && live) {
                    const int32_t rows = (n - i * DG_TILE < DG_TILE) ? n - i * DG_TILE : DG_TILE;
#pragma unroll 4
                    for (int32_t r = r0; r < rows; r += DG_FILL / DG_KB) {
                        const int64_t j = (int64_t)first_pair + a + i * DG_TILE + r;
                        double tm, ts;
                        es_diag_terms(util, base, j, sg, ss, k0, k1, generation, k, &tm, &ts);
                        tile[i & 1][r][kl] = tm;
                        tile[i & 1][r][DG_KB + kl] = ts;
                    }
                }
            } else if (i > 0 && live) {
                const int32_t rows = (n - (i - 1) * DG_TILE < DG_TILE) ? n - (i - 1) * DG_TILE : DG_TILE;
                const double(*src)[2 * DG_KB] = tile[(i - 1) & 1];
                int32_t r = 0;
                for (; r + DG_AHEAD <= rows; r += DG_AHEAD) {   // the reads of 16 rows in flight, then the ordered adds
                    double v[DG_AHEAD];
#pragma unroll
                    for (int32_t u = 0; u < DG_AHEAD; ++u) v[u] = src[r + u][lane];
#pragma unroll
                    for (int32_t u = 0; u < DG_AHEAD; ++u) acc = __dadd_rn(acc, v[u]);
                }
                for (; r < rows; ++r) acc = __dadd_rn(acc, src[r][lane]);
            }
            __syncthreads();
        }
        if (!filler && live) partial[((int64_t)(lane >> 5) * n_chunks + c) * K + k] = acc;
    }
}

__global__ __launch_bounds__(ES_THREADS) void es_diag_partial_thread(const float *__restrict__ util,
                                                                     const float *__restrict__ sigma,
                                                                     double *__restrict__ partial, int32_t K,
                                                                     uint32_t k0, uint32_t k1, uint32_t generation,
                                                                     int32_t first_pair, int32_t n_pairs, float base) {
    const int32_t k = (int32_t)(blockIdx.y * ES_THREADS + threadIdx.x);
    if (k >= K) return;
    const int32_t c = (int32_t)blockIdx.x, n_chunks = (int32_t)gridDim.x;
    const int32_t a = c * ES_CHUNK, b = (n_pairs - a < ES_CHUNK) ? n_pairs : a + ES_CHUNK;
    const float sg = sigma[k];
    const double ss = __dmul_rn((double)sg, (double)sg);
    double pm = 0.0, ps = 0.0;
    for (int32_t jl = a; jl < b; ++jl) {
        double tm, ts;
        es_diag_terms(util, base, (int64_t)first_pair + jl, sg, ss, k0, k1, generation, k, &tm, &ts);
        pm = __dadd_rn(pm, tm);
        ps = __dadd_rn(ps, ts);
    }
    partial[(int64_t)c * K + k] = pm;
    partial[((int64_t)n_chunks + c) * K + k] = ps;
}

// The header's step 4 and 5.  theta_out may be theta and sigma_out sigma: a thread reads its own elements first.
__global__ __launch_bounds__(ES_THREADS) void es_diag_tail(const double *__restrict__ partial, const float *theta,
                                                           const float *sigma, float *g_theta, float *theta_out,
                                                           float *g_sigma, float *sigma_out, int32_t K,
                                                           int32_t n_chunks, wg_es_diag_step st) {
    const int32_t k = (int32_t)(blockIdx.x * ES_THREADS + threadIdx.x);
    if (k >= K) return;
    double sm = 0.0, ss = 0.0;
    for (int32_t c = 0; c < n_chunks; ++c) sm = __dadd_rn(sm, partial[(int64_t)c * K + k]);
    for (int32_t c = 0; c < n_chunks; ++c) ss = __dadd_rn(ss, partial[((int64_t)n_chunks + c) * K + k]);
    const float th = theta[k], sg = sigma[k];
    const float gt = (float)__dmul_rn(sm, st.scale_theta);
    const float gs = (float)__ddiv_rn(__dmul_rn(ss, st.scale_sigma), (double)sg);
    if (g_theta) g_theta[k] = gt;
    if (g_sigma) g_sigma[k] = gs;
    if (theta_out) theta_out[k] = __fadd_rn(th, __fmul_rn(st.lr_theta, gt));
    if (sigma_out) {
        const float s = __fadd_rn(sg, __fmul_rn(st.lr_sigma, gs));
        const float dn = __fmul_rn(sg, st.shrink), up = __fmul_rn(sg, st.grow);
        const float lo = dn > st.sigma_min ? dn : st.sigma_min, hi = up < st.sigma_max ? up : st.sigma_max;
        sigma_out[k] = (s < lo) ? lo : ((s > hi) ? hi : s);
    }
}

// ------------------------------------------------------------------------------------------- a second hidden layer
// The six segments of a deep theta in order (element counts, 0 for an absent one) and the candidate tensors.
struct EsDeepLayout {
    int32_t n_w1, n_b1, n_wm, n_bm, n_w2, n_b2;
    float *w1, *b1, *wm, *bm, *w2, *b2;
};

// A thread of the deep perturb kernels: its parameter k, its pair j and the address of element k in set 2j (set 2j + 1
// is *stride elements on).  es_perturb's mapping (rows of ppb pairs, blocks of 256 values of k); false for a thread
// beyond the launch's pairs or parameters.  A segment of no elements never takes an element: off >= 0 is not < 0, so
// the chain moves on with off unchanged.  The last branch is b2's: k < K leaves nothing else.
__device__ __forceinline__ bool es_deep_slot(const EsDeepLayout &lay, int32_t K, int32_t ppb, int32_t first_pair,
                                             int32_t n_pairs, int32_t *k_out, int32_t *j_out, float **p_out,
                                             int64_t *stride_out) {
    int32_t pl = 0, k;
    if (ppb > 1) {
        pl = (int32_t)threadIdx.x / K;
        k = (int32_t)threadIdx.x - pl * K;
        if (pl >= ppb) return false;
    } else {
        k = (int32_t)(blockIdx.y * ES_THREADS + threadIdx.x);
        if (k >= K) return false;
    }
    const int32_t jl = (int32_t)blockIdx.x * ppb + pl;   // < n_pairs + ppb <= 2^30 + 256
    if (jl >= n_pairs) return false;
    float *dst;
    int64_t stride;
    int32_t off = k;
    if (off < lay.n_w1) {
        dst = lay.w1; stride = lay.n_w1;
    } else if ((off -= lay.n_w1) < lay.n_b1) {
        dst = lay.b1; stride = lay.n_b1;
    } else if ((off -= lay.n_b1) < lay.n_wm) {
        dst = lay.wm; stride = lay.n_wm;
    } else if ((off -= lay.n_wm) < lay.n_bm) {
        dst = lay.bm; stride = lay.n_bm;
    } else if ((off -= lay.n_bm) < lay.n_w2) {
        dst = lay.w2; stride = lay.n_w2;
    } else {
        off -= lay.n_w2;
        dst = lay.b2; stride = lay.n_b2;
    }
    const int32_t j = first_pair + jl;
    *k_out = k;
    *j_out = j;
    *p_out = dst + off + 2 * (int64_t)j * stride;   // 64-bit: wm's set stride is up to 65,536 elements
    *stride_out = stride;
    return true;
}

// es_perturb over the six-segment theta: set 2j gets RN32(theta[k] + d), set 2j + 1 RN32(theta[k] - d), d = RN32(sigma *
// eps(seed, generation, j, k)) with k the index in the deep theta.
__global__ __launch_bounds__(ES_THREADS) void es_perturb_deep(EsDeepLayout lay, const float *__restrict__ theta, int32_t K,
                                                              int32_t ppb, uint32_t k0, uint32_t k1, uint32_t generation,
                                                              float sigma, int32_t first_pair, int32_t n_pairs) {
    int32_t k, j;
    float *p;
    int64_t stride;
    if (!es_deep_slot(lay, K, ppb, first_pair, n_pairs, &k, &j, &p, &stride)) return;
    const float th = theta[k];
    const float d = __fmul_rn(sigma, wg_eps<WG_ES_TAG>(k0, k1, generation, (uint32_t)j, (uint32_t)k));
    p[0] = __fadd_rn(th, d);
    p[stride] = __fsub_rn(th, d);
}

// The same with d = RN32(sigma[k] * eps), sigma [K] in the deep theta's order.
__global__ __launch_bounds__(ES_THREADS) void es_perturb_diag_deep(EsDeepLayout lay, const float *__restrict__ theta,
                                                                   const float *__restrict__ sigma, int32_t K,
                                                                   int32_t ppb, uint32_t k0, uint32_t k1,
                                                                   uint32_t generation, int32_t first_pair,
                                                                   int32_t n_pairs) {
    int32_t k, j;
    float *p;
    int64_t stride;
    if (!es_deep_slot(lay, K, ppb, first_pair, n_pairs, &k, &j, &p, &stride)) return;
    const float th = theta[k];
    const float d = __fmul_rn(sigma[k], wg_eps<WG_ES_TAG>(k0, k1, generation, (uint32_t)j, (uint32_t)k));
    p[0] = __fadd_rn(th, d);
    p[stride] = __fsub_rn(th, d);
}

// The checks that every call here shares, in the order the header lists them (scalar_sigma: also es->sigma, which
// the _diag calls do not read); everything but the parameter count, which depends on the layout.
int es_check_head(const wg_es *es, int32_t first_pair, int32_t n_pairs, const char *who, bool scalar_sigma) {
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
    if (scalar_sigma && (!std::isfinite(es->sigma) || !(es->sigma > 0.0f))) return wg_fail(WG_EINVAL, "%s: sigma must be finite and > 0", who);
    return 0;
}

// The four-segment entries: the shared checks, then the layout and K.
int es_check(const wg_es *es, int32_t first_pair, int32_t n_pairs, const char *who, EsLayout *lay, int64_t *K,
             bool scalar_sigma = true) {
    if (const int rc = es_check_head(es, first_pair, n_pairs, who, scalar_sigma)) return rc;
    const int64_t H = es->hidden, D = es->obs_dim, C = es->act_dim;
    const int64_t n_w1 = D * H, n_b1 = es->b1 ? H : 0, n_w2 = (H > 0 ? H : D) * C, n_b2 = es->b2 ? C : 0;
    *K = n_w1 + n_b1 + n_w2 + n_b2;
    if (*K > ES_MAX_K) return wg_fail(WG_EINVAL, "%s: %lld parameters (at most 2^23)", who, (long long)*K);
    lay->n_w1 = (int32_t)n_w1; lay->n_b1 = (int32_t)n_b1; lay->n_w2 = (int32_t)n_w2; lay->n_b2 = (int32_t)n_b2;
    lay->w1 = es->w1; lay->b1 = es->b1; lay->w2 = es->w2; lay->b2 = es->b2;
    return 0;
}

// The _deep entries: the shared checks in front, then the middle layer's, then K over the six segments.
int es_check_deep(const wg_es *es, const wg_es_mid *mid, int32_t first_pair, int32_t n_pairs, const char *who,
                  EsDeepLayout *lay, int64_t *K, bool scalar_sigma = true) {
    if (const int rc = es_check_head(es, first_pair, n_pairs, who, scalar_sigma)) return rc;
    if (!mid) return wg_fail(WG_EINVAL, "%s: null mid", who);
    if (mid->hidden2 < 1 || mid->hidden2 > 256)
        return wg_fail(WG_EINVAL, "%s: hidden2 %d outside 1..256", who, mid->hidden2);
    if (es->hidden == 0) return wg_fail(WG_EINVAL, "%s: a middle layer without a first hidden layer (hidden 0)", who);
    if (!mid->wm) return wg_fail(WG_EINVAL, "%s: null wm", who);
    const int64_t H = es->hidden, H2 = mid->hidden2, D = es->obs_dim, C = es->act_dim;
    const int64_t n_w1 = D * H, n_b1 = es->b1 ? H : 0, n_wm = H * H2, n_bm = mid->bm ? H2 : 0, n_w2 = H2 * C,
                  n_b2 = es->b2 ? C : 0;
    *K = n_w1 + n_b1 + n_wm + n_bm + n_w2 + n_b2;
    if (*K > ES_MAX_K) return wg_fail(WG_EINVAL, "%s: %lld parameters (at most 2^23)", who, (long long)*K);
    lay->n_w1 = (int32_t)n_w1; lay->n_b1 = (int32_t)n_b1; lay->n_wm = (int32_t)n_wm; lay->n_bm = (int32_t)n_bm;
    lay->n_w2 = (int32_t)n_w2; lay->n_b2 = (int32_t)n_b2;
    lay->w1 = es->w1; lay->b1 = es->b1; lay->wm = mid->wm; lay->bm = mid->bm; lay->w2 = es->w2; lay->b2 = es->b2;
    return 0;
}

// What follows the layout's checks in wg_es_update and wg_es_update_deep: the call's own refusals and the two launches
// (the kernels know the layout through K alone).
int es_update_run(const char *who, const wg_es *es, int32_t K, int32_t first_pair, int32_t n_pairs, const float *util,
                  double scale, float lr, double *workspace, float *grad, float *theta_out, hipStream_t stream) {
    if (!util) return wg_fail(WG_EINVAL, "%s: null util", who);
    if (!workspace) return wg_fail(WG_EINVAL, "%s: null workspace", who);
    if (!std::isfinite(scale)) return wg_fail(WG_EINVAL, "%s: scale is not finite", who);
    if (!std::isfinite(lr)) return wg_fail(WG_EINVAL, "%s: lr is not finite", who);
    if (!grad && !theta_out) return wg_fail(WG_EINVAL, "%s: grad and theta_out are both null", who);
    const int32_t n_chunks = (n_pairs + ES_CHUNK - 1) / ES_CHUNK, kb = (K + ES_THREADS - 1) / ES_THREADS;
    es_update_partial<<<dim3(n_chunks, kb), ES_THREADS, 0, stream>>>(
        util, workspace, K, (uint32_t)(es->seed & 0xffffffffu), (uint32_t)(es->seed >> 32), es->generation, first_pair,
        n_pairs);
    if (const int rc = wg_launched("wg_es_update (partial sums): launch")) return rc;
    es_update_tail<<<kb, ES_THREADS, 0, stream>>>(workspace, es->theta, grad, theta_out, K, n_chunks, scale, lr);
    return wg_launched("wg_es_update (tail): launch");
}

// The same for wg_es_update_diag and wg_es_update_diag_deep.
int es_update_diag_run(const char *who, const wg_es *es, int32_t K, const float *sigma, int32_t first_pair,
                       int32_t n_pairs, const float *util, const wg_es_diag_step *step, double *workspace,
                       float *g_theta, float *theta_out, float *g_sigma, float *sigma_out, hipStream_t stream) {
    if (!sigma) return wg_fail(WG_EINVAL, "%s: null sigma vector", who);
    if (!util) return wg_fail(WG_EINVAL, "%s: null util", who);
    if (!step) return wg_fail(WG_EINVAL, "%s: null step", who);
    if (!workspace) return wg_fail(WG_EINVAL, "%s: null workspace", who);
    if (!std::isfinite(step->base)) return wg_fail(WG_EINVAL, "%s: base is not finite", who);
    if (!std::isfinite(step->scale_theta)) return wg_fail(WG_EINVAL, "%s: scale_theta is not finite", who);
    if (!std::isfinite(step->scale_sigma)) return wg_fail(WG_EINVAL, "%s: scale_sigma is not finite", who);
    if (!std::isfinite(step->lr_theta)) return wg_fail(WG_EINVAL, "%s: lr_theta is not finite", who);
    if (!std::isfinite(step->lr_sigma)) return wg_fail(WG_EINVAL, "%s: lr_sigma is not finite", who);
    if (!(step->shrink > 0.0f && step->shrink <= 1.0f)) return wg_fail(WG_EINVAL, "%s: shrink outside (0, 1]", who);
    if (!std::isfinite(step->grow) || !(step->grow >= 1.0f)) return wg_fail(WG_EINVAL, "%s: grow must be finite and >= 1", who);
    if (!std::isfinite(step->sigma_min) || !(step->sigma_min > 0.0f))
        return wg_fail(WG_EINVAL, "%s: sigma_min must be finite and > 0", who);
    if (!(step->sigma_max >= step->sigma_min)) return wg_fail(WG_EINVAL, "%s: sigma_max below sigma_min (or NaN)", who);
    if (!g_theta && !theta_out && !g_sigma && !sigma_out) return wg_fail(WG_EINVAL, "%s: all four outputs are null", who);
    const int32_t n_chunks = (n_pairs + ES_CHUNK - 1) / ES_CHUNK;
    const uint32_t k0 = (uint32_t)(es->seed & 0xffffffffu), k1 = (uint32_t)(es->seed >> 32);
    const int32_t tblocks = (K + ES_THREADS - 1) / ES_THREADS;
    if ((int64_t)n_chunks * tblocks >= DG_THREAD_FORM_GROUPS) {
        es_diag_partial_thread<<<dim3(n_chunks, tblocks), ES_THREADS, 0, stream>>>(
            util, sigma, workspace, K, k0, k1, es->generation, first_pair, n_pairs, step->base);
    } else {
        const int32_t kblocks = (K + DG_KB - 1) / DG_KB;
        es_diag_partial_spread<<<dim3(n_chunks, kblocks < DG_MAX_KBLOCKS ? kblocks : DG_MAX_KBLOCKS), DG_THREADS, 0,
                                 stream>>>(util, sigma, workspace, K, kblocks, k0, k1, es->generation, first_pair,
                                           n_pairs, step->base);
    }
    if (const int rc = wg_launched("wg_es_update_diag (partial sums): launch")) return rc;
    es_diag_tail<<<(K + ES_THREADS - 1) / ES_THREADS, ES_THREADS, 0, stream>>>(workspace, es->theta, sigma, g_theta,
                                                                              theta_out, g_sigma, sigma_out, K,
                                                                              n_chunks, *step);
    return wg_launched("wg_es_update_diag (tail): launch");
}

// The grid of the perturb kernels: rows of ppb pairs by blocks of 256 parameters.
dim3 es_perturb_grid(int32_t K, int32_t n_pairs, int32_t *ppb) {
    *ppb = K >= ES_THREADS ? 1 : ES_THREADS / K;
    return dim3((n_pairs + *ppb - 1) / *ppb, *ppb > 1 ? 1 : (K + ES_THREADS - 1) / ES_THREADS);
}

}  // namespace

extern "C" {

int wg_es_perturb(const wg_es *es, int32_t first_pair, int32_t n_pairs, hipStream_t stream) {
    EsLayout lay;
    int64_t K64;
    if (const int rc = es_check(es, first_pair, n_pairs, "wg_es_perturb", &lay, &K64)) return rc;
    const int32_t K = (int32_t)K64;
    int32_t ppb;
    const dim3 grid = es_perturb_grid(K, n_pairs, &ppb);
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
    return es_update_run("wg_es_update", es, (int32_t)K64, first_pair, n_pairs, util, scale, lr, workspace, grad,
                         theta_out, stream);
}

int wg_es_perturb_diag(const wg_es *es, const float *sigma, int32_t first_pair, int32_t n_pairs, hipStream_t stream) {
    EsLayout lay;
    int64_t K64;
    if (const int rc = es_check(es, first_pair, n_pairs, "wg_es_perturb_diag", &lay, &K64, false)) return rc;
    if (!sigma) return wg_fail(WG_EINVAL, "wg_es_perturb_diag: null sigma vector");
    const int32_t K = (int32_t)K64;
    int32_t ppb;
    const dim3 grid = es_perturb_grid(K, n_pairs, &ppb);
    es_perturb_diag<<<grid, ES_THREADS, 0, stream>>>(lay, es->theta, sigma, K, ppb, (uint32_t)(es->seed & 0xffffffffu),
                                                    (uint32_t)(es->seed >> 32), es->generation, first_pair, n_pairs);
    return wg_launched("wg_es_perturb_diag: launch");
}

int wg_es_update_diag(const wg_es *es, const float *sigma, int32_t first_pair, int32_t n_pairs, const float *util,
                      const wg_es_diag_step *step, double *workspace, float *g_theta, float *theta_out, float *g_sigma,
                      float *sigma_out, hipStream_t stream) {
    EsLayout lay;
    int64_t K64;
    if (const int rc = es_check(es, first_pair, n_pairs, "wg_es_update_diag", &lay, &K64, false)) return rc;
    return es_update_diag_run("wg_es_update_diag", es, (int32_t)K64, sigma, first_pair, n_pairs, util, step, workspace,
                              g_theta, theta_out, g_sigma, sigma_out, stream);
}

int wg_es_perturb_deep(const wg_es *es, const wg_es_mid *mid, int32_t first_pair, int32_t n_pairs, hipStream_t stream) {
    EsDeepLayout lay;
    int64_t K64;
    if (const int rc = es_check_deep(es, mid, first_pair, n_pairs, "wg_es_perturb_deep", &lay, &K64)) return rc;
    const int32_t K = (int32_t)K64;
    int32_t ppb;
    const dim3 grid = es_perturb_grid(K, n_pairs, &ppb);
    es_perturb_deep<<<grid, ES_THREADS, 0, stream>>>(lay, es->theta, K, ppb, (uint32_t)(es->seed & 0xffffffffu),
                                                    (uint32_t)(es->seed >> 32), es->generation, es->sigma, first_pair,
                                                    n_pairs);
    return wg_launched("wg_es_perturb_deep: launch");
}

int wg_es_update_deep(const wg_es *es, const wg_es_mid *mid, int32_t first_pair, int32_t n_pairs, const float *util,
                      double scale, float lr, double *workspace, float *grad, float *theta_out, hipStream_t stream) {
    EsDeepLayout lay;
    int64_t K64;
    if (const int rc = es_check_deep(es, mid, first_pair, n_pairs, "wg_es_update_deep", &lay, &K64)) return rc;
    return es_update_run("wg_es_update_deep", es, (int32_t)K64, first_pair, n_pairs, util, scale, lr, workspace, grad,
                         theta_out, stream);
}

int wg_es_perturb_diag_deep(const wg_es *es, const wg_es_mid *mid, const float *sigma, int32_t first_pair,
                            int32_t n_pairs, hipStream_t stream) {
    EsDeepLayout lay;
    int64_t K64;
    if (const int rc = es_check_deep(es, mid, first_pair, n_pairs, "wg_es_perturb_diag_deep", &lay, &K64, false))
        return rc;
    if (!sigma) return wg_fail(WG_EINVAL, "wg_es_perturb_diag_deep: null sigma vector");
    const int32_t K = (int32_t)K64;
    int32_t ppb;
    const dim3 grid = es_perturb_grid(K, n_pairs, &ppb);
    es_perturb_diag_deep<<<grid, ES_THREADS, 0, stream>>>(lay, es->theta, sigma, K, ppb,
                                                         (uint32_t)(es->seed & 0xffffffffu), (uint32_t)(es->seed >> 32),
                                                         es->generation, first_pair, n_pairs);
    return wg_launched("wg_es_perturb_diag_deep: launch");
}

int wg_es_update_diag_deep(const wg_es *es, const wg_es_mid *mid, const float *sigma, int32_t first_pair,
                           int32_t n_pairs, const float *util, const wg_es_diag_step *step, double *workspace,
                           float *g_theta, float *theta_out, float *g_sigma, float *sigma_out, hipStream_t stream) {
    EsDeepLayout lay;
    int64_t K64;
    if (const int rc = es_check_deep(es, mid, first_pair, n_pairs, "wg_es_update_diag_deep", &lay, &K64, false))
        return rc;
    return es_update_diag_run("wg_es_update_diag_deep", es, (int32_t)K64, sigma, first_pair, n_pairs, util, step,
                              workspace, g_theta, theta_out, g_sigma, sigma_out, stream);
}

}  // extern "C"
