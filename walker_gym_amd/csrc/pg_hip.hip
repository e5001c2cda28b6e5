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
//   gae_held_scan  wg_gae_held: the same scan on wg_rollout_held's decision grid (a sixth load, `decided`, per step).
//
// and wg_policy_forward / wg_policy_backward: wg_policy's layers over recorded observation rows, and their gradient.
//
//   pr_forward       a workgroup takes tiles of up to 64 rows: the rows are copied to LDS once (coalesced; skipped rows
//                    are neither loaded nor stored), then one thread per (row, unit) runs the unit's chain, pr_chain,
//                    the one definition of the arithmetic here (x rows padded to an odd length: no bank conflicts).  A shared policy's weights (n_sets == 1) are staged in
//                    LDS when they fit PR_W_LDS bytes; otherwise they are read through L2.
//   pr_grad_partial  a workgroup owns one (set, chunk) and walks its rows in order, PR_BWD_ROWS at a time: x, dy in LDS,
//                    h recomputed by pr_chain, dh beside it.  The two outer products (x|1) (x) dh and (in|1) (x) dy (the
//                    appended 1 makes each bias one more row) are cut into 4 x 4 register blocks of float64
//                    accumulators, NT blocks per thread: a row costs a thread two 16-byte LDS reads per 16 fma.
//                    RN64(P + a * b) with an exact product is one float64 fma.  Blocks past the shapes compute on
//                    zero padding and are dropped.
//   pr_grad_tail     S = the chunks' partials added in order, g = RN32(S), one thread per element.
//
// The NM = PrNorm instances of pr_forward and pr_grad_partial (wg_policy_forward_normalized / _backward_normalized)
// normalise a row where it enters LDS, in pr_stage: the forward, the backward's recompute and both outer products then
// see xn.  The NM = PrNone instances are the kernels as they were; the normaliser is a trailing kernel argument.
//
// and wg_obs_moments: the float64 moments of recorded rows in a fixed order.
//
//   obs_moments_partial  a workgroup owns one chunk: its rows are staged in LDS tile by tile, a wave per row with the
//                        loads of OM_U rows issued before their LDS stores; each lane folds |x| < bound over its
//                        elements and the wave votes the row's used flag.  Then one thread per column walks the staged
//                        rows in ascending rho, its two float64 chains in registers (OM_NC columns per thread: 256 *
//                        OM_NC columns a pass; wider rows walk the chunk again for the next columns).
//   obs_moments_tail     one workgroup: a thread per column adds the chunks in order into the caller's state, then
//                        derives mean and scale.
//
// and wg_expf / wg_ppo_surrogate: the pinned exponential (wg_expf.h) and the clipped surrogate over recorded rows.
//
//   ppo_logp_rows     the density mode: a thread per row, the Gaussian log-density summed over c ascending.
//   ppo_rows_partial  a workgroup owns one (set, chunk): a thread per row of a tile (16-byte loads of y / u and stores of
//                     dy where act_dim % 4 == 0 and the addresses allow) computes the density, the ratio through
//                     wg_expf_scalar, the clip and the row's dy, and leaves its terms in LDS; then thread j < act_dim + 5
//                     adds the tile's rows in ascending rho, one float64 chain per element.
//   ppo_rows_tail     one workgroup: the chunks' partials added in order, then the sets' statistics.

#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>
#include <type_traits>

#include "walker_hip.h"
#include "walker_internal.h"   // wg_fail, wg_launched: the refusals here go to the library's one error message
#include "wg_expf.h"           // wg_expf_scalar: the pinned exponential of wg_expf and of the surrogate's ratio

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

// wg_gae_held: gae_scan on the decision grid of wg_rollout_held.  The same structure (one thread per walker, a step's
// seven loads contiguous across the wave, the next block's loads ahead of the chain); beside `carry` a thread carries
// the open hold's closing values (R, nv, cf) and whether the step above it decided (that step then closes a hold).
struct GaeHeldIn {
    float r, v, nv;
    uint32_t dc, tm, ct;
};
template <bool TERM, bool CUT>
__device__ __forceinline__ void gae_held_load(GaeHeldIn (&x)[GAE_U], const float *__restrict__ hold_reward,
                                              const float *__restrict__ value, const float *__restrict__ next_value,
                                              const uint8_t *__restrict__ decided, const uint8_t *__restrict__ term,
                                              const uint8_t *__restrict__ cut, int t_hi, int64_t stride, int w) {
#pragma unroll
    for (int k = 0; k < GAE_U; k++) {
        const int t = t_hi - k > 0 ? t_hi - k : 0;
        const int64_t at = (int64_t)t * stride + w;
        x[k].r = hold_reward[at];
        x[k].v = value[at];
        x[k].nv = next_value[at];
        x[k].dc = decided[at];
        x[k].tm = TERM ? term[at] : 0u;
        x[k].ct = CUT ? cut[at] : 0u;
    }
}

template <bool TERM, bool CUT>
__global__ __launch_bounds__(GAE_THREADS) void gae_held_scan(
    const float *__restrict__ hold_reward, const float *__restrict__ value, const float *__restrict__ next_value,
    const uint8_t *__restrict__ decided, const uint8_t *__restrict__ term, const uint8_t *__restrict__ cut, int n_steps,
    int N, int64_t stride, float gamma, float gl, float *__restrict__ adv, float *__restrict__ ret) {
    const int w = (int)(blockIdx.x * GAE_THREADS + threadIdx.x);
    if (w >= N) return;
    GaeHeldIn cur[GAE_U], nxt[GAE_U];
    float carry = 0.f, R = 0.f, nv = 0.f;
    uint32_t cf = 0u;
    bool closes = true;   // the call's last step closes the hold it is in
    gae_held_load<TERM, CUT>(cur, hold_reward, value, next_value, decided, term, cut, n_steps - 1, stride, w);
    for (int t_hi = n_steps - 1; t_hi >= 0; t_hi -= GAE_U) {
        gae_held_load<TERM, CUT>(nxt, hold_reward, value, next_value, decided, term, cut, t_hi - GAE_U, stride, w);
#pragma unroll
        for (int k = 0; k < GAE_U; k++) {
            const int t = t_hi - k;
            if (t < 0) break;
            if (closes) {
                R = cur[k].r;
                nv = cur[k].tm ? 0.f : cur[k].nv;
                cf = cur[k].ct;
            }
            closes = cur[k].dc != 0u;
            float a = 0.f, r = 0.f;
            if (closes) {   // the step decided
                const float delta = __fsub_rn(__fadd_rn(R, __fmul_rn(gamma, nv)), cur[k].v);
                const float c = cf ? 0.f : carry;
                a = carry = __fadd_rn(delta, __fmul_rn(gl, c));
                r = __fadd_rn(carry, cur[k].v);
            }
            const int64_t at = (int64_t)t * stride + w;
            adv[at] = a;
            if (ret) ret[at] = r;
        }
#pragma unroll
        for (int k = 0; k < GAE_U; k++) cur[k] = nxt[k];
    }
}

// ------------------------------------------------------------------------------------------------ policy rows
constexpr int PR_THREADS = 256;
constexpr int PR_LDS = 64 * 1024;    // dynamic LDS of a workgroup, at most
constexpr int PR_W_LDS = 32 * 1024;  // forward: a shared policy's weights are staged in LDS up to this size
constexpr int PR_FWD_ROWS = 64;      // rows per tile, at most
constexpr int PR_BWD_ROWS = 16;
constexpr int PR_MAX_NT = 4;         // 4 x 4 blocks per thread: WG_POLICY_GRAD_MAX_K / (16 * PR_THREADS)
static_assert(PR_MAX_NT * 16 * PR_THREADS == WG_POLICY_GRAD_MAX_K, "the header's limit is what the registers hold");

inline int up4(int v) { return (v + 3) & ~3; }

struct PrArgs {
    const float *x;
    const uint8_t *mask;
    const float *w1, *b1, *w2, *b2;
    int64_t x_step, mask_step;
    int32_t n_steps, N, n;          // n = N / n_sets walkers per set
    int32_t D, H, C, n2;            // n2 = H ? H : D inputs of the output layer
    int32_t Dp, Hq, Hp, Cp;         // LDS row lengths: up4(D + 1), up4(H + 1), up4(H), up4(C) (the forward: D | 1, H | 1)
    int32_t TR;                     // rows per tile
};
// wg_obs_norm as a kernel argument; PrNone in its place where nothing is normalised
struct PrNone {};
struct PrNorm {
    const float *mean, *scale;
    float clip;
};

// The unit's chain, acc = RN32(acc + RN32(in[i] * w[i * stride + off])) for i ascending, of NU units side by side:
// every unit's own operations are the contract's, in its order; NU independent chains share the loads of in[i].
// PR_NU = 4 was measured: the forward gained under 10 %, the backward's recompute lost a wave per SIMD to the extra
// registers and doubled its time at H = 32; one unit per thread it is.
constexpr int PR_NU = 1;
template <int NU>
__device__ __forceinline__ void pr_chain(float (&acc)[NU], const float *in, const float *w, int n, int stride,
                                         const int (&off)[NU]) {
#pragma unroll 4
    for (int i = 0; i < n; i++) {
        const float v = in[i];
        const float *wi = w + (int64_t)i * stride;
#pragma unroll
        for (int k = 0; k < NU; k++) acc[k] = __fadd_rn(acc[k], __fmul_rn(v, wi[off[k]]));
    }
}

// Rows rho0 .. rho0 + TR of a sequence numbered rho = t * n_seq + (w - w_base), those below rho_end: row r's (t, w) to
// rt / rw, whether it is evaluated to ok, its x (then 1.0f, then zeros up to Dp) to xs, and, with dy, its dy row (zeros
// up to Cp) to dys.  A wave per row, lanes along the row.  NM = PrNorm: the row's D values are normalised on their way in,
//   v = RN32(RN32(x[i] - mean[i]) * scale[i]);  xn[i] = (v < -clip) ? -clip : ((v > clip) ? clip : v)
template <class NM>
__device__ __forceinline__ void pr_stage(const PrArgs &a, int64_t rho0, int64_t rho_end, int n_seq, int w_base,
                                         const float *__restrict__ dy, int64_t dy_step, float *xs, float *dys, int *ok,
                                         int *rt, int *rw, const NM &nm) {
    const int lane = threadIdx.x & 63;
    for (int r = threadIdx.x >> 6; r < a.TR; r += PR_THREADS / 64) {
        const int64_t rho = rho0 + r;
        const bool in = rho < rho_end;
        const int t = in ? (int)(rho / n_seq) : 0, w = in ? w_base + (int)(rho % n_seq) : 0;
        const bool on = in && (!a.mask || a.mask[(int64_t)t * a.mask_step + w] != 0);
        if (lane == 0) {
            ok[r] = on;
            rt[r] = t;
            rw[r] = w;
        }
        if (!on) continue;
        const float *xr = a.x + (int64_t)t * a.x_step + (int64_t)w * a.D;
        if constexpr (std::is_same<NM, PrNorm>::value) {
            for (int i = lane; i < a.Dp; i += 64) {
                float v = i == a.D ? 1.0f : 0.0f;
                if (i < a.D) {
                    v = __fmul_rn(__fsub_rn(xr[i], nm.mean[i]), nm.scale[i]);
                    v = (v < -nm.clip) ? -nm.clip : ((v > nm.clip) ? nm.clip : v);   // (a NaN passes through)
                }
                xs[r * a.Dp + i] = v;
            }
        } else {
            for (int i = lane; i < a.Dp; i += 64) xs[r * a.Dp + i] = i < a.D ? xr[i] : (i == a.D ? 1.0f : 0.0f);
        }
        if (dy) {
            const float *dr = dy + (int64_t)t * dy_step + (int64_t)w * a.C;
            for (int c = lane; c < a.Cp; c += 64) dys[r * a.Cp + c] = c < a.C ? dr[c] : 0.0f;
        }
    }
}

// The hidden layer of the tile's rows: a thread takes a row and the PR_NU units j, j + JS, ... (JS = ceil(H / PR_NU):
// the lanes of a wave read consecutive weights; a unit past H repeats unit H - 1 and is dropped).  h to hs and, with DH,
// dh to dhs:
//   d = +0.0f; for c ascending: d = RN32(d + RN32(dy[c] * w2[j][c]));  dh[j] = (z[j] > 0) ? d : +0.0f   (h > 0 iff z > 0)
// lw1 / lb1: the set's weights in LDS (WLDS) -- otherwise each row's set is read through L2.
template <bool WLDS, bool DH>
__device__ __forceinline__ void pr_hidden(const PrArgs &a, const float *xs, const float *dys, const int *ok, const int *rw,
                                          const float *lw1, const float *lb1, float *hs, float *dhs) {
    const int JS = (a.H + PR_NU - 1) / PR_NU;
    for (int item = threadIdx.x; item < a.TR * JS; item += PR_THREADS) {
        const int r = item / JS, j = item - r * JS;
        if (!ok[r]) continue;
        const int64_t g = rw[r] / a.n;
        const float *w1 = WLDS ? lw1 : a.w1 + g * a.D * a.H;
        const float *b1 = WLDS ? lb1 : (a.b1 ? a.b1 + g * a.H : nullptr);
        int u[PR_NU];
        float z[PR_NU];
#pragma unroll
        for (int k = 0; k < PR_NU; k++) {
            u[k] = j + k * JS < a.H ? j + k * JS : a.H - 1;
            z[k] = b1 ? b1[u[k]] : 0.0f;
        }
        pr_chain<PR_NU>(z, xs + r * a.Dp, w1, a.D, a.H, u);
#pragma unroll
        for (int k = 0; k < PR_NU; k++) {
            if (j + k * JS >= a.H) continue;
            const float h = z[k] > 0.0f ? z[k] : 0.0f;
            hs[r * a.Hq + u[k]] = h;
            if (DH) {
                float d[1] = {0.0f};
                const int at[1] = {0};
                pr_chain<1>(d, dys + r * a.Cp, a.w2 + (g * a.H + u[k]) * a.C, a.C, 1, at);
                dhs[r * a.Hp + u[k]] = h > 0.0f ? d[0] : 0.0f;
            }
        }
    }
}

// LDS, in floats: [the weights (WLDS)] xs[TR][Dp] hs[TR][Hq] ok[TR] rt[TR] rw[TR]
template <bool WLDS, class NM = PrNone>
__global__ __launch_bounds__(PR_THREADS) void pr_forward(PrArgs a, int64_t n_tiles, int w_floats, float *__restrict__ y,
                                                         int64_t y_step, NM nm) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *lw1 = lds, *lb1 = lw1 + a.D * a.H, *lw2 = lb1 + (a.b1 ? a.H : 0), *lb2 = lw2 + a.n2 * a.C;
    float *xs = lds + w_floats, *hs = xs + a.TR * a.Dp;
    int *ok = reinterpret_cast<int *>(hs + (a.H ? a.TR * a.Hq : 0)), *rt = ok + a.TR, *rw = rt + a.TR;
    if (WLDS) {
        for (int i = threadIdx.x; i < a.D * a.H; i += PR_THREADS) lw1[i] = a.w1[i];
        for (int i = threadIdx.x; i < a.H && a.b1; i += PR_THREADS) lb1[i] = a.b1[i];
        for (int i = threadIdx.x; i < a.n2 * a.C; i += PR_THREADS) lw2[i] = a.w2[i];
        for (int i = threadIdx.x; i < a.C && a.b2; i += PR_THREADS) lb2[i] = a.b2[i];
    }
    const int64_t rows = (int64_t)a.n_steps * a.N;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        pr_stage(a, tile * a.TR, rows, a.N, 0, nullptr, 0, xs, nullptr, ok, rt, rw, nm);
        __syncthreads();
        if (a.H) {
            pr_hidden<WLDS, false>(a, xs, nullptr, ok, rw, lw1, a.b1 ? lb1 : nullptr, hs, nullptr);
            __syncthreads();
        }
        const int JS = (a.C + PR_NU - 1) / PR_NU;      // the output units likewise: c, c + JS, ...
        for (int item = threadIdx.x; item < a.TR * JS; item += PR_THREADS) {
            const int r = item / JS, c = item - r * JS;
            if (!ok[r]) continue;
            const int64_t g = rw[r] / a.n;
            const float *w2 = WLDS ? lw2 : a.w2 + g * a.n2 * a.C;
            const float *b2 = WLDS ? (a.b2 ? lb2 : nullptr) : (a.b2 ? a.b2 + g * a.C : nullptr);
            int u[PR_NU];
            float acc[PR_NU];
#pragma unroll
            for (int k = 0; k < PR_NU; k++) {
                u[k] = c + k * JS < a.C ? c + k * JS : a.C - 1;
                acc[k] = b2 ? b2[u[k]] : 0.0f;
            }
            pr_chain<PR_NU>(acc, a.H ? hs + r * a.Hq : xs + r * a.Dp, w2, a.n2, a.C, u);
            float *yr = y + (int64_t)rt[r] * y_step + (int64_t)rw[r] * a.C;
#pragma unroll
            for (int k = 0; k < PR_NU; k++)
                if (c + k * JS < a.C) yr[u[k]] = acc[k];
        }
        __syncthreads();
    }
}

// LDS, in floats: xs[TR][Dp] hs[TR][Hq] dhs[TR][Hp] dys[TR][Cp] ok[TR] rt[TR] rw[TR]
// Block q of the workgroup's list: q < T1 the layer-1 product (x|1) (x) dh, rows 4 * (q / JT1) .., columns 4 * (q % JT1)
// ..; then the T2 blocks of (in|1) (x) dy; thread tid owns blocks tid, tid + 256, ...
template <int NT, class NM = PrNone>
__global__ __launch_bounds__(PR_THREADS) void pr_grad_partial(PrArgs a, const float *__restrict__ dy, int64_t dy_step,
                                                              int32_t chunk_rows, int64_t n_chunks, int32_t T1,
                                                              double *__restrict__ ws, int32_t K, NM nm) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *xs = lds, *hs = xs + a.TR * a.Dp, *dhs = hs + (a.H ? a.TR * a.Hq : 0), *dys = dhs + (a.H ? a.TR * a.Hp : 0);
    int *ok = reinterpret_cast<int *>(dys + a.TR * a.Cp), *rt = ok + a.TR, *rw = rt + a.TR;
    const int g = (int)(blockIdx.x / n_chunks);
    const int64_t k = blockIdx.x - (int64_t)g * n_chunks;
    const int64_t lo = k * chunk_rows, set_rows = (int64_t)a.n_steps * a.n;
    const int64_t hi = set_rows - lo < chunk_rows ? set_rows : lo + chunk_rows;

    // the padding that no tile rewrites: hs[r][H] = 1 (the bias row), zeros behind it and behind dh
    if (a.H)
        for (int r = threadIdx.x; r < a.TR; r += PR_THREADS) {
            for (int j = a.H; j < a.Hq; j++) hs[r * a.Hq + j] = j == a.H ? 1.0f : 0.0f;
            for (int j = a.H; j < a.Hp; j++) dhs[r * a.Hp + j] = 0.0f;
        }

    const float *in2 = a.H ? hs : xs;
    const int s_in2 = a.H ? a.Hq : a.Dp, JT1 = a.Hp >> 2, JT2 = a.Cp >> 2, T2 = (s_in2 >> 2) * JT2;
    const float *pa[NT], *pb[NT];
    int sa[NT], sb[NT];
#pragma unroll
    for (int u = 0; u < NT; u++) {
        const int q = (int)threadIdx.x + u * PR_THREADS;
        if (q < T1) {
            pa[u] = xs + 4 * (q / JT1); sa[u] = a.Dp;
            pb[u] = dhs + 4 * (q % JT1); sb[u] = a.Hp;
        } else {
            const int q2 = q - T1 < T2 ? q - T1 : 0;      // a thread past the list repeats block 0 and drops it
            pa[u] = in2 + 4 * (q2 / JT2); sa[u] = s_in2;
            pb[u] = dys + 4 * (q2 % JT2); sb[u] = a.Cp;
        }
    }
    double acc[NT][4][4];
#pragma unroll
    for (int u = 0; u < NT; u++)
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j < 4; j++) acc[u][i][j] = 0.0;

    for (int64_t base = lo; base < hi; base += a.TR) {
        pr_stage(a, base, hi, a.n, g * a.n, dy, dy_step, xs, dys, ok, rt, rw, nm);
        __syncthreads();
        if (a.H) {
            if (T1) pr_hidden<false, true>(a, xs, dys, ok, rw, nullptr, nullptr, hs, dhs);
            else pr_hidden<false, false>(a, xs, dys, ok, rw, nullptr, nullptr, hs, dhs);
            __syncthreads();
        }
        for (int r = 0; r < a.TR; r++) {
            if (!ok[r]) continue;
#pragma unroll
            for (int u = 0; u < NT; u++) {
                const float4 va = *reinterpret_cast<const float4 *>(pa[u] + r * sa[u]);
                const float4 vb = *reinterpret_cast<const float4 *>(pb[u] + r * sb[u]);
                const double da[4] = {va.x, va.y, va.z, va.w}, db[4] = {vb.x, vb.y, vb.z, vb.w};
#pragma unroll
                for (int i = 0; i < 4; i++)
#pragma unroll
                    for (int j = 0; j < 4; j++) acc[u][i][j] = fma(da[i], db[j], acc[u][i][j]);
            }
        }
        __syncthreads();
    }

    // wg_es's segment order: w1 [D][H], b1 [H] (if set), w2 [n2][C], b2 [C] (if set)
    double *out = ws + ((int64_t)g * n_chunks + k) * K;
    const int base2 = a.D * a.H + (a.H && a.b1 ? a.H : 0);
#pragma unroll
    for (int u = 0; u < NT; u++) {
        const int q = (int)threadIdx.x + u * PR_THREADS;
        const bool l1 = q < T1;
        if (!l1 && q - T1 >= T2) continue;
        const int i0 = l1 ? 4 * (q / JT1) : 4 * ((q - T1) / JT2), j0 = l1 ? 4 * (q % JT1) : 4 * ((q - T1) % JT2);
        const int I = l1 ? a.D : a.n2, J = l1 ? a.H : a.C, off = l1 ? 0 : base2;
        const bool bias = l1 ? a.b1 != nullptr : a.b2 != nullptr;
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int ii = i0 + i, jj = j0 + j;
                if (jj < J && (ii < I || (ii == I && bias))) out[off + ii * J + jj] = acc[u][i][j];
            }
    }
}

struct PrGrads {
    float *g[4];        // w1, b1, w2, b2 (NULL: not wanted)
    int32_t end[4];     // the segments' ends in [0, K]
};

__global__ __launch_bounds__(PR_THREADS) void pr_grad_tail(const double *__restrict__ ws, PrGrads o, int32_t K,
                                                           int64_t n_chunks, int64_t total) {
    const int64_t idx = (int64_t)blockIdx.x * PR_THREADS + threadIdx.x;
    if (idx >= total) return;
    const int64_t g = idx / K;
    const int e = (int)(idx - g * K);
    float *dst;
    int lo, hi;
    if (e < o.end[0]) dst = o.g[0], lo = 0, hi = o.end[0];
    else if (e < o.end[1]) dst = o.g[1], lo = o.end[0], hi = o.end[1];
    else if (e < o.end[2]) dst = o.g[2], lo = o.end[1], hi = o.end[2];
    else dst = o.g[3], lo = o.end[2], hi = o.end[3];
    if (!dst) return;
    const double *p = ws + g * n_chunks * K + e;
    double S = 0.0;
    for (int64_t c = 0; c < n_chunks; c++) S = __dadd_rn(S, p[c * K]);
    dst[g * (hi - lo) + (e - lo)] = (float)S;
}

// ------------------------------------------------------------------------------------------------ deep policy rows
// wg_policy_mid as a kernel argument of the *_deep kernels (kernels of their own: the shallow ones above keep their
// arguments and their registers).  There a.H is H1, a.n2 = H2 and a.w2 is [H2][C].
struct PrMid {
    const float *wm, *bm;
    int32_t H2;
    int32_t Gq, Gp;                 // LDS row lengths of h2 | 1 and of dh2: up4(H2 + 1), up4(H2) (the forward: H2 | 1)
};

// The second hidden layer of the tile's rows, a thread per (row, unit k): h2 to h2s and, with dh2s,
//   d = +0.0f; for c ascending: d = RN32(d + RN32(dy[c] * w2[k][c]));  dh2[k] = (z2[k] > 0) ? d : +0.0f
template <bool WLDS>
__device__ __forceinline__ void pr_mid(const PrArgs &a, const PrMid &m, const float *hs, const float *dys, const int *ok,
                                       const int *rw, const float *lwm, const float *lbm, float *h2s, float *dh2s) {
    for (int item = threadIdx.x; item < a.TR * m.H2; item += PR_THREADS) {
        const int r = item / m.H2, k = item - r * m.H2;
        if (!ok[r]) continue;
        const int64_t g = rw[r] / a.n;
        const float *wm = WLDS ? lwm : m.wm + g * a.H * m.H2;
        const float *bm = WLDS ? lbm : (m.bm ? m.bm + g * m.H2 : nullptr);
        float z[1] = {bm ? bm[k] : 0.0f};
        const int at[1] = {k};
        pr_chain<1>(z, hs + r * a.Hq, wm, a.H, m.H2, at);
        const float h = z[0] > 0.0f ? z[0] : 0.0f;
        h2s[r * m.Gq + k] = h;
        if (dh2s) {
            float d[1] = {0.0f};
            const int at0[1] = {0};
            pr_chain<1>(d, dys + r * a.Cp, a.w2 + (g * m.H2 + k) * a.C, a.C, 1, at0);
            dh2s[r * m.Gp + k] = h > 0.0f ? d[0] : 0.0f;
        }
    }
}

// dh1 of the tile's rows, a thread per (row, unit j):
//   d = +0.0f; for k ascending: d = RN32(d + RN32(dh2[k] * wm[j][k]));  dh1[j] = (z1[j] > 0) ? d : +0.0f   (h1 > 0 iff z1 > 0)
__device__ __forceinline__ void pr_dh1(const PrArgs &a, const PrMid &m, const float *hs, const float *dh2s, const int *ok,
                                       const int *rw, float *dhs) {
    for (int item = threadIdx.x; item < a.TR * a.H; item += PR_THREADS) {
        const int r = item / a.H, j = item - r * a.H;
        if (!ok[r]) continue;
        const int64_t g = rw[r] / a.n;
        float d[1] = {0.0f};
        const int at0[1] = {0};
        pr_chain<1>(d, dh2s + r * m.Gp, m.wm + (g * a.H + j) * m.H2, m.H2, 1, at0);
        dhs[r * a.Hp + j] = hs[r * a.Hq + j] > 0.0f ? d[0] : 0.0f;
    }
}

// LDS, in floats: [the weights (WLDS): w1 b1 wm bm w2 b2] xs[TR][Dp] hs[TR][Hq] h2s[TR][Gq] ok[TR] rt[TR] rw[TR]
template <bool WLDS, class NM = PrNone>
__global__ __launch_bounds__(PR_THREADS) void pr_forward_deep(PrArgs a, PrMid m, int64_t n_tiles, int w_floats,
                                                              float *__restrict__ y, int64_t y_step, NM nm) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *lw1 = lds, *lb1 = lw1 + a.D * a.H, *lwm = lb1 + (a.b1 ? a.H : 0), *lbm = lwm + a.H * m.H2;
    float *lw2 = lbm + (m.bm ? m.H2 : 0), *lb2 = lw2 + m.H2 * a.C;
    float *xs = lds + w_floats, *hs = xs + a.TR * a.Dp, *h2s = hs + a.TR * a.Hq;
    int *ok = reinterpret_cast<int *>(h2s + a.TR * m.Gq), *rt = ok + a.TR, *rw = rt + a.TR;
    if (WLDS) {
        for (int i = threadIdx.x; i < a.D * a.H; i += PR_THREADS) lw1[i] = a.w1[i];
        for (int i = threadIdx.x; i < a.H && a.b1; i += PR_THREADS) lb1[i] = a.b1[i];
        for (int i = threadIdx.x; i < a.H * m.H2; i += PR_THREADS) lwm[i] = m.wm[i];
        for (int i = threadIdx.x; i < m.H2 && m.bm; i += PR_THREADS) lbm[i] = m.bm[i];
        for (int i = threadIdx.x; i < m.H2 * a.C; i += PR_THREADS) lw2[i] = a.w2[i];
        for (int i = threadIdx.x; i < a.C && a.b2; i += PR_THREADS) lb2[i] = a.b2[i];
    }
    const int64_t rows = (int64_t)a.n_steps * a.N;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        pr_stage(a, tile * a.TR, rows, a.N, 0, nullptr, 0, xs, nullptr, ok, rt, rw, nm);
        __syncthreads();
        pr_hidden<WLDS, false>(a, xs, nullptr, ok, rw, lw1, a.b1 ? lb1 : nullptr, hs, nullptr);
        __syncthreads();
        pr_mid<WLDS>(a, m, hs, nullptr, ok, rw, lwm, m.bm ? lbm : nullptr, h2s, nullptr);
        __syncthreads();
        for (int item = threadIdx.x; item < a.TR * a.C; item += PR_THREADS) {
            const int r = item / a.C, c = item - r * a.C;
            if (!ok[r]) continue;
            const int64_t g = rw[r] / a.n;
            const float *w2 = WLDS ? lw2 : a.w2 + g * m.H2 * a.C;
            const float *b2 = WLDS ? (a.b2 ? lb2 : nullptr) : (a.b2 ? a.b2 + g * a.C : nullptr);
            float acc[1] = {b2 ? b2[c] : 0.0f};
            const int at[1] = {c};
            pr_chain<1>(acc, h2s + r * m.Gq, w2, m.H2, a.C, at);
            y[(int64_t)rt[r] * y_step + (int64_t)rw[r] * a.C + c] = acc[0];
        }
        __syncthreads();
    }
}

// LDS, in floats: xs[TR][Dp] hs[TR][Hq] dhs[TR][Hp] h2s[TR][Gq] dh2s[TR][Gp] dys[TR][Cp] ok[TR] rt[TR] rw[TR]
// Block q of the workgroup's list: q < T1 the product (x|1) (x) dh1, then the Tm blocks of (h1|1) (x) dh2, then the T2
// blocks of (h2|1) (x) dy; rows 4 * (q' / JT) .., columns 4 * (q' % JT) .. of its product; thread tid owns blocks tid,
// tid + 256, ...  T1 == 0: dh1 is not formed; T1 == 0 and Tm == 0: neither is dh2.
template <int NT, class NM = PrNone>
__global__ __launch_bounds__(PR_THREADS) void pr_grad_partial_deep(PrArgs a, PrMid m, const float *__restrict__ dy,
                                                                   int64_t dy_step, int32_t chunk_rows, int64_t n_chunks,
                                                                   int32_t T1, int32_t Tm, double *__restrict__ ws,
                                                                   int32_t K, NM nm) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *xs = lds, *hs = xs + a.TR * a.Dp, *dhs = hs + a.TR * a.Hq, *h2s = dhs + a.TR * a.Hp;
    float *dh2s = h2s + a.TR * m.Gq, *dys = dh2s + a.TR * m.Gp;
    int *ok = reinterpret_cast<int *>(dys + a.TR * a.Cp), *rt = ok + a.TR, *rw = rt + a.TR;
    const int g = (int)(blockIdx.x / n_chunks);
    const int64_t k = blockIdx.x - (int64_t)g * n_chunks;
    const int64_t lo = k * chunk_rows, set_rows = (int64_t)a.n_steps * a.n;
    const int64_t hi = set_rows - lo < chunk_rows ? set_rows : lo + chunk_rows;

    // the padding that no tile rewrites: hs[r][H] = h2s[r][H2] = 1 (the bias rows), zeros behind them and behind dh1, dh2
    // (the whole dh rows: a product whose dh is not formed is not accumulated, but nothing is left unwritten)
    for (int r = threadIdx.x; r < a.TR; r += PR_THREADS) {
        for (int j = a.H; j < a.Hq; j++) hs[r * a.Hq + j] = j == a.H ? 1.0f : 0.0f;
        for (int j = 0; j < a.Hp; j++) dhs[r * a.Hp + j] = 0.0f;
        for (int j = m.H2; j < m.Gq; j++) h2s[r * m.Gq + j] = j == m.H2 ? 1.0f : 0.0f;
        for (int j = 0; j < m.Gp; j++) dh2s[r * m.Gp + j] = 0.0f;
    }

    const int JT1 = a.Hp >> 2, JTm = m.Gp >> 2, JT2 = a.Cp >> 2, T2 = (m.Gq >> 2) * JT2;
    const float *pa[NT], *pb[NT];
    int sa[NT], sb[NT];
#pragma unroll
    for (int u = 0; u < NT; u++) {
        const int q = (int)threadIdx.x + u * PR_THREADS;
        if (q < T1) {
            pa[u] = xs + 4 * (q / JT1); sa[u] = a.Dp;
            pb[u] = dhs + 4 * (q % JT1); sb[u] = a.Hp;
        } else if (q < T1 + Tm) {
            const int qm = q - T1;
            pa[u] = hs + 4 * (qm / JTm); sa[u] = a.Hq;
            pb[u] = dh2s + 4 * (qm % JTm); sb[u] = m.Gp;
        } else {
            const int q2 = q - T1 - Tm < T2 ? q - T1 - Tm : 0;      // a thread past the list repeats block 0 and drops it
            pa[u] = h2s + 4 * (q2 / JT2); sa[u] = m.Gq;
            pb[u] = dys + 4 * (q2 % JT2); sb[u] = a.Cp;
        }
    }
    double acc[NT][4][4];
#pragma unroll
    for (int u = 0; u < NT; u++)
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j < 4; j++) acc[u][i][j] = 0.0;

    for (int64_t base = lo; base < hi; base += a.TR) {
        pr_stage(a, base, hi, a.n, g * a.n, dy, dy_step, xs, dys, ok, rt, rw, nm);
        __syncthreads();
        pr_hidden<false, false>(a, xs, dys, ok, rw, nullptr, nullptr, hs, nullptr);
        __syncthreads();
        pr_mid<false>(a, m, hs, dys, ok, rw, nullptr, nullptr, h2s, (T1 || Tm) ? dh2s : nullptr);
        __syncthreads();
        if (T1) {
            pr_dh1(a, m, hs, dh2s, ok, rw, dhs);
            __syncthreads();
        }
        for (int r = 0; r < a.TR; r++) {
            if (!ok[r]) continue;
#pragma unroll
            for (int u = 0; u < NT; u++) {
                const float4 va = *reinterpret_cast<const float4 *>(pa[u] + r * sa[u]);
                const float4 vb = *reinterpret_cast<const float4 *>(pb[u] + r * sb[u]);
                const double da[4] = {va.x, va.y, va.z, va.w}, db[4] = {vb.x, vb.y, vb.z, vb.w};
#pragma unroll
                for (int i = 0; i < 4; i++)
#pragma unroll
                    for (int j = 0; j < 4; j++) acc[u][i][j] = fma(da[i], db[j], acc[u][i][j]);
            }
        }
        __syncthreads();
    }

    // the segment order: w1 [D][H], b1 [H] (if set), wm [H][H2], bm [H2] (if set), w2 [H2][C], b2 [C] (if set)
    double *out = ws + ((int64_t)g * n_chunks + k) * K;
    const int basem = a.D * a.H + (a.b1 ? a.H : 0);
    const int base2 = basem + a.H * m.H2 + (m.bm ? m.H2 : 0);
#pragma unroll
    for (int u = 0; u < NT; u++) {
        const int q = (int)threadIdx.x + u * PR_THREADS;
        int i0, j0, I, J, off;
        bool bias;
        if (q < T1) {
            i0 = 4 * (q / JT1); j0 = 4 * (q % JT1); I = a.D; J = a.H; off = 0; bias = a.b1 != nullptr;
        } else if (q < T1 + Tm) {
            const int qm = q - T1;
            i0 = 4 * (qm / JTm); j0 = 4 * (qm % JTm); I = a.H; J = m.H2; off = basem; bias = m.bm != nullptr;
        } else {
            const int q2 = q - T1 - Tm;
            if (q2 >= T2) continue;
            i0 = 4 * (q2 / JT2); j0 = 4 * (q2 % JT2); I = m.H2; J = a.C; off = base2; bias = a.b2 != nullptr;
        }
#pragma unroll
        for (int i = 0; i < 4; i++)
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int ii = i0 + i, jj = j0 + j;
                if (jj < J && (ii < I || (ii == I && bias))) out[off + ii * J + jj] = acc[u][i][j];
            }
    }
}

struct PrGrads6 {
    float *g[6];        // w1, b1, wm, bm, w2, b2 (NULL: not wanted)
    int32_t end[6];     // the segments' ends in [0, K]
};

__global__ __launch_bounds__(PR_THREADS) void pr_grad_tail_deep(const double *__restrict__ ws, PrGrads6 o, int32_t K,
                                                                int64_t n_chunks, int64_t total) {
    const int64_t idx = (int64_t)blockIdx.x * PR_THREADS + threadIdx.x;
    if (idx >= total) return;
    const int64_t g = idx / K;
    const int e = (int)(idx - g * K);
    float *dst = o.g[5];
    int lo = o.end[4], hi = o.end[5];
#pragma unroll
    for (int s = 4; s >= 0; s--)   // (the first segment that holds e; constant indices: the argument stays in SGPRs)
        if (e < o.end[s]) dst = o.g[s], lo = s ? o.end[s - 1] : 0, hi = o.end[s];
    if (!dst) return;
    const double *p = ws + g * n_chunks * K + e;
    double S = 0.0;
    for (int64_t c = 0; c < n_chunks; c++) S = __dadd_rn(S, p[c * K]);
    dst[g * (hi - lo) + (e - lo)] = (float)S;
}

// ------------------------------------------------------------------------------------------------ observation moments
constexpr int OM_ROWS = 64;  // rows per tile, at most
constexpr int OM_U = 4;       // rows whose loads a wave issues before their LDS stores
constexpr int OM_NC = 4;      // columns per thread and pass: two float64 chains each

struct OmArgs {
    const float *x;
    const uint8_t *mask;
    int64_t x_step, mask_step, rows;   // rows = n_steps * N
    int32_t N, D, TR, chunk_rows;
    float bound;
};

// LDS, in floats: xs[TR][D] used[TR]
__global__ __launch_bounds__(PR_THREADS) void obs_moments_partial(OmArgs a, double *__restrict__ ws) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *xs = lds;
    int *used = reinterpret_cast<int *>(xs + (size_t)a.TR * a.D);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t k = blockIdx.x, lo = k * a.chunk_rows;
    const int64_t hi = a.rows - lo < a.chunk_rows ? a.rows : lo + a.chunk_rows;
    double *out = ws + k * (1 + 2 * (int64_t)a.D);
    for (int cb = 0; cb < a.D; cb += PR_THREADS * OM_NC) {   // (one pass up to 1,024 columns)
        double p1[OM_NC], p2[OM_NC];
#pragma unroll
        for (int u = 0; u < OM_NC; u++) p1[u] = p2[u] = 0.0;
        double cnt = 0.0;
        for (int64_t base = lo; base < hi; base += a.TR) {
            // a wave takes OM_U rows at a time: rows wv * OM_U + u of each group of 4 * OM_U
            for (int r0 = wv * OM_U; r0 < a.TR; r0 += (PR_THREADS / 64) * OM_U) {
                const float *xr[OM_U];
                bool on[OM_U], fin[OM_U];
#pragma unroll
                for (int u = 0; u < OM_U; u++) {
                    const int64_t rho = base + r0 + u;
                    const bool in = r0 + u < a.TR && rho < hi;
                    const int64_t t = in ? rho / a.N : 0, w = in ? rho - t * a.N : 0;
                    on[u] = in && (!a.mask || a.mask[t * a.mask_step + w] != 0);   // (wave-uniform)
                    xr[u] = a.x + t * a.x_step + w * a.D;
                    fin[u] = true;
                }
                for (int i = lane; i < a.D; i += 64) {
                    float v[OM_U];
#pragma unroll
                    for (int u = 0; u < OM_U; u++) v[u] = on[u] ? xr[u][i] : 0.0f;
#pragma unroll
                    for (int u = 0; u < OM_U; u++) {
                        if (!on[u]) continue;
                        xs[(size_t)(r0 + u) * a.D + i] = v[u];
                        fin[u] = fin[u] && fabsf(v[u]) < a.bound;   // (a NaN compares false)
                    }
                }
#pragma unroll
                for (int u = 0; u < OM_U; u++) {
                    const bool all = __all(fin[u]) != 0;
                    if (lane == 0 && r0 + u < a.TR) used[r0 + u] = on[u] && all;
                }
            }
            __syncthreads();
            for (int r = 0; r < a.TR; r++) {
                if (!used[r]) continue;
                cnt += 1.0;
#pragma unroll
                for (int u = 0; u < OM_NC; u++) {
                    const int c = cb + (int)threadIdx.x + u * PR_THREADS;
                    if (c >= a.D) continue;
                    const double v = (double)xs[(size_t)r * a.D + c];
                    p1[u] = __dadd_rn(p1[u], v);
                    p2[u] = fma(v, v, p2[u]);
                }
            }
            __syncthreads();
        }
        if (cb == 0 && threadIdx.x == 0) out[0] = cnt;
#pragma unroll
        for (int u = 0; u < OM_NC; u++) {
            const int c = cb + (int)threadIdx.x + u * PR_THREADS;
            if (c >= a.D) continue;
            out[1 + c] = p1[u];
            out[1 + a.D + c] = p2[u];
        }
    }
}

// One workgroup.  state = n, S1[D], S2[D]; mean_out / scale_out NULL: the state alone.
__global__ __launch_bounds__(PR_THREADS) void obs_moments_tail(const double *__restrict__ ws, int64_t n_chunks, int32_t D,
                                                               double *__restrict__ state, double eps,
                                                               float *__restrict__ mean_out,
                                                               float *__restrict__ scale_out) {
    const int64_t W = 1 + 2 * (int64_t)D;
    double n = state[0];
    for (int64_t k = 0; k < n_chunks; k++) n = __dadd_rn(n, ws[k * W]);   // (every thread: the counts are exact)
    __syncthreads();   // every thread has read state[0]
    if (threadIdx.x == 0) state[0] = n;
    for (int c = threadIdx.x; c < D; c += PR_THREADS) {
        double s1 = state[1 + c], s2 = state[1 + D + c];
        for (int64_t k = 0; k < n_chunks; k++) {
            s1 = __dadd_rn(s1, ws[k * W + 1 + c]);
            s2 = __dadd_rn(s2, ws[k * W + 1 + D + c]);
        }
        state[1 + c] = s1;
        state[1 + D + c] = s2;
        if (n > 0.0 && mean_out) {
            const double m = __ddiv_rn(s1, n);
            double var = __dsub_rn(__ddiv_rn(s2, n), __dmul_rn(m, m));
            var = var > 0.0 ? var : 0.0;
            mean_out[c] = (float)m;
            scale_out[c] = (float)__ddiv_rn(1.0, __dsqrt_rn(__dadd_rn(var, eps)));
        }
    }
}

// ------------------------------------------------------------------------------------------------ PPO surrogate
constexpr int PPO_STATS = 5;   // rows, surrogate, log-ratio, clipped, value error: the elements behind the act_dim sums

struct PpoArgs {
    const float *y, *u, *sigma, *log_sigma;
    const uint8_t *mask;
    const float *old_logp, *adv, *value, *ret, *scale;
    float *logp_out, *dy, *dvalue;
    int64_t y_step, u_step, mask_step, row_step, dy_step;
    int32_t n_steps, N, n;          // n = N / n_sets walkers per set
    int32_t C, Cs, TR, chunk_rows;  // Cs = C | 1, the LDS row length (odd: the rows of a wave fall on distinct banks)
    float lo, hi;                   // RN32(1 - clip_eps), RN32(1 + clip_eps)
};

// The row's log-density, c ascending; with zs, z[c] is left in zs[c].  V4: act_dim % 4 == 0 and rows on 16-byte addresses.
template <bool V4>
__device__ __forceinline__ float ppo_logp(const float *__restrict__ yr, const float *__restrict__ ur,
                                          const float *__restrict__ sg, const float *__restrict__ ls, int C, float *zs) {
    const float K0 = __builtin_bit_cast(float, 0x3F6B3F8Eu);   // RN32(0.5 * ln(2 pi))
    float logp = 0.0f;
    auto unit = [&](int c, float y, float u) {
        const float z = __fdiv_rn(__fsub_rn(u, y), sg[c]);
        const float l = __fsub_rn(__fsub_rn(__fmul_rn(-0.5f, __fmul_rn(z, z)), ls[c]), K0);
        logp = __fadd_rn(logp, l);
        if (zs) zs[c] = z;
    };
    if (V4) {
        for (int c = 0; c < C; c += 4) {
            const float4 vy = *reinterpret_cast<const float4 *>(yr + c), vu = *reinterpret_cast<const float4 *>(ur + c);
            unit(c, vy.x, vu.x); unit(c + 1, vy.y, vu.y); unit(c + 2, vy.z, vu.z); unit(c + 3, vy.w, vu.w);
        }
    } else {
        for (int c = 0; c < C; c++) unit(c, yr[c], ur[c]);
    }
    return logp;
}

// wg_ppo_surrogate's density mode: a thread per row of the whole batch.
template <bool V4>
__global__ __launch_bounds__(PR_THREADS) void ppo_logp_rows(PpoArgs a, int64_t rows) {
    const int64_t idx = (int64_t)blockIdx.x * PR_THREADS + threadIdx.x;
    if (idx >= rows) return;
    const int64_t t = idx / a.N, w = idx - t * a.N;
    if (a.mask && a.mask[t * a.mask_step + w] == 0) return;   // (per lane: a skipped row is not loaded)
    const int64_t g = w / a.n;
    a.logp_out[t * a.row_step + w] = ppo_logp<V4>(a.y + t * a.y_step + w * a.C, a.u + t * a.u_step + w * a.C,
                                                  a.sigma + g * a.C, a.log_sigma + g * a.C, a.C, nullptr);
}

// Element j of a row's terms added to P: j < C the log-sigma term (an exact product: one float64 fma), then the five
// statistics.  f: bit 0 the row is unskipped, bit 1 it was clipped.
__device__ __forceinline__ double ppo_add(double P, int j, int C, int f, float wr, float qm1, float surr, float d,
                                          float ev) {
    if (j < C) return fma((double)wr, (double)qm1, P);
    switch (j - C) {
        case 0: return __dadd_rn(P, 1.0);
        case 1: return __dadd_rn(P, (double)surr);
        case 2: return __dadd_rn(P, (double)d);
        case 3: return __dadd_rn(P, (f & 2) ? 1.0 : 0.0);
        default: return fma((double)ev, (double)ev, P);
    }
}

// A workgroup owns one (set, chunk) and walks its rows in order, TR at a time: thread r takes row base + r (density,
// ratio, clip, dy; its z row, then q - 1, in LDS), then thread j < act_dim + 5 adds the tile's rows in ascending rho, one
// float64 chain per element (act_dim > 251: threads 0..4 carry a second chain, element 256 + j).
// LDS, in floats: zs[TR][Cs] wr[TR] surr[TR] d[TR] ev[TR] flag[TR]
template <bool V4>
__global__ __launch_bounds__(PR_THREADS) void ppo_rows_partial(PpoArgs a, int64_t n_chunks, double *__restrict__ ws) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float *zs = lds, *wrs = zs + a.TR * a.Cs, *surrs = wrs + a.TR, *dls = surrs + a.TR, *evs = dls + a.TR;
    int *flag = reinterpret_cast<int *>(evs + a.TR);
    const int g = (int)(blockIdx.x / n_chunks);
    const int64_t k = blockIdx.x - (int64_t)g * n_chunks;
    const int64_t lo = k * a.chunk_rows, set_rows = (int64_t)a.n_steps * a.n;
    const int64_t hi = set_rows - lo < a.chunk_rows ? set_rows : lo + a.chunk_rows;
    const float *sg = a.sigma + (int64_t)g * a.C, *ls = a.log_sigma + (int64_t)g * a.C;
    const float sc0 = a.scale[0], sc1 = a.value ? a.scale[1] : 0.0f;
    const int C = a.C, J = C + PPO_STATS, r = (int)threadIdx.x, j2 = r + PR_THREADS;
    double P = 0.0, P2 = 0.0;
    for (int64_t base = lo; base < hi; base += a.TR) {
        if (r < a.TR) {
            const int64_t rho = base + r;
            bool on = rho < hi;
            int64_t t = 0, w = 0;
            if (on) {
                t = rho / a.n;
                w = (int64_t)g * a.n + (rho - t * a.n);
                on = !a.mask || a.mask[t * a.mask_step + w] != 0;   // (per lane: a skipped row is not loaded)
            }
            int f = 0;
            if (on) {
                const int64_t at = t * a.row_step + w;
                float *z = zs + r * a.Cs;
                const float logp = ppo_logp<V4>(a.y + t * a.y_step + w * C, a.u + t * a.u_step + w * C, sg, ls, C, z);
                if (a.logp_out) a.logp_out[at] = logp;
                const float d = __fsub_rn(logp, a.old_logp[at]);
                const float rr = wg_expf_scalar(d), A = a.adv[at];
                const float s1 = __fmul_rn(rr, A);
                const float rc = (rr < a.lo) ? a.lo : ((rr > a.hi) ? a.hi : rr);
                const float s2 = __fmul_rn(rc, A);
                const bool take = s1 <= s2;                          // (a NaN compares false)
                const float wr = __fmul_rn(sc0, take ? s1 : 0.0f);
                float ev = 0.0f;
                if (a.value) {
                    ev = __fsub_rn(a.value[at], a.ret[at]);
                    if (a.dvalue) a.dvalue[at] = __fmul_rn(sc1, ev);
                }
                float *dr = a.dy ? a.dy + t * a.dy_step + w * C : nullptr;
                if (V4) {
                    for (int c = 0; c < C; c += 4) {
                        float4 v;
                        v.x = __fmul_rn(wr, __fdiv_rn(z[c], sg[c]));
                        v.y = __fmul_rn(wr, __fdiv_rn(z[c + 1], sg[c + 1]));
                        v.z = __fmul_rn(wr, __fdiv_rn(z[c + 2], sg[c + 2]));
                        v.w = __fmul_rn(wr, __fdiv_rn(z[c + 3], sg[c + 3]));
                        if (dr) *reinterpret_cast<float4 *>(dr + c) = v;
#pragma unroll
                        for (int i = 0; i < 4; i++) z[c + i] = __fsub_rn(__fmul_rn(z[c + i], z[c + i]), 1.0f);
                    }
                } else {
                    for (int c = 0; c < C; c++) {
                        const float zc = z[c];
                        if (dr) dr[c] = __fmul_rn(wr, __fdiv_rn(zc, sg[c]));
                        z[c] = __fsub_rn(__fmul_rn(zc, zc), 1.0f);
                    }
                }
                wrs[r] = wr;
                surrs[r] = take ? s1 : s2;
                dls[r] = d;
                evs[r] = ev;
                f = 1 | (rc != rr ? 2 : 0);
            }
            flag[r] = f;
        }
        __syncthreads();
        if (r < J) {
            for (int q = 0; q < a.TR; q++) {
                const int f = flag[q];
                if (!(f & 1)) continue;
                P = ppo_add(P, r, C, f, wrs[q], zs[q * a.Cs + (r < C ? r : 0)], surrs[q], dls[q], evs[q]);
                if (j2 < J) P2 = ppo_add(P2, j2, C, f, wrs[q], 0.0f, surrs[q], dls[q], evs[q]);   // (j2 >= 256 >= C)
            }
        }
        __syncthreads();
    }
    double *out = ws + ((int64_t)g * n_chunks + k) * J;
    if (r < J) out[r] = P;
    if (j2 < J) out[j2] = P2;
}

// One workgroup: S_g[j], the chunks' partials added in order; g_log_sigma[g][c] = RN32(S_g[c]); stats[j], the sets'
// S_g[act_dim + j] added in order.
__global__ __launch_bounds__(PR_THREADS) void ppo_rows_tail(const double *__restrict__ ws, int64_t n_chunks, int32_t G,
                                                            int32_t C, float *__restrict__ g_log_sigma,
                                                            double *__restrict__ stats) {
    const int J = C + PPO_STATS;
    if (g_log_sigma)
        for (int64_t i = threadIdx.x; i < (int64_t)G * C; i += PR_THREADS) {
            const int64_t g = i / C;
            const double *p = ws + g * n_chunks * J + (i - g * C);
            double S = 0.0;
            for (int64_t k = 0; k < n_chunks; k++) S = __dadd_rn(S, p[k * J]);
            g_log_sigma[i] = (float)S;
        }
    if (stats && threadIdx.x < PPO_STATS) {
        double st = 0.0;
        for (int64_t g = 0; g < G; g++) {
            const double *p = ws + g * n_chunks * J + C + threadIdx.x;
            double S = 0.0;
            for (int64_t k = 0; k < n_chunks; k++) S = __dadd_rn(S, p[k * J]);
            st = __dadd_rn(st, S);
        }
        stats[threadIdx.x] = st;
    }
}

// wg_expf: a thread per element, the grid striding past 2^31 elements.
__global__ __launch_bounds__(PR_THREADS) void expf_rows(const float *x, int64_t n, float *out) {
    for (int64_t i = (int64_t)blockIdx.x * PR_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * PR_THREADS)
        out[i] = wg_expf_scalar(x[i]);
}

// [p, p + bytes) of an array of `elem`-byte elements, [n_steps][N] with `stride` elements between steps
struct Span {
    uintptr_t lo, hi;
};
Span span_of(const void *p, int n_steps, int64_t N, int64_t stride, int elem) {
    const uintptr_t lo = reinterpret_cast<uintptr_t>(p);
    return Span{lo, lo + (uintptr_t)(((int64_t)(n_steps - 1) * stride + N) * elem)};
}
bool overlap(const Span &a, const Span &b) { return a.lo < b.hi && b.lo < a.hi; }

// ------------------------------------------------------------------------------------------------ policy rows: host
struct PrPlan {
    PrArgs a;
    int64_t K;            // parameters per set, wg_es's count
    int32_t end[4];       // the ends of w1, b1, w2, b2 in [0, K]
    int32_t T1, T2;       // 4 x 4 blocks of the two outer products
    int32_t n_sets;
};
struct PrBuf {
    const char *name;
    const void *p;
    Span s;
};

// What the three calls check alike; fills the plan (TR stays 0).
int pr_check(const wg_policy *pol, const wg_policy_rows *rows, const char *who, PrPlan *pl) {
    if (!pol) return wg_fail(WG_EINVAL, "%s: null policy", who);
    if (!rows) return wg_fail(WG_EINVAL, "%s: null rows", who);
    if (!pol->w2) return wg_fail(WG_EINVAL, "%s: null w2", who);
    if (pol->hidden < 0 || pol->hidden > 256) return wg_fail(WG_EINVAL, "%s: hidden %d outside 0..256", who, pol->hidden);
    if (pol->hidden > 0 && !pol->w1) return wg_fail(WG_EINVAL, "%s: hidden %d with a null w1", who, pol->hidden);
    if (pol->obs_dim < 1) return wg_fail(WG_EINVAL, "%s: obs_dim %d < 1", who, pol->obs_dim);
    if (pol->act_dim < 1) return wg_fail(WG_EINVAL, "%s: act_dim %d < 1", who, pol->act_dim);
    if (pol->action_out || pol->return_out || pol->length_out)
        return wg_fail(WG_EINVAL, "%s: action_out / return_out / length_out must be NULL", who);
    if (rows->n_steps < 1) return wg_fail(WG_EINVAL, "%s: n_steps %d < 1", who, rows->n_steps);
    if (rows->N < 1) return wg_fail(WG_EINVAL, "%s: N %d < 1", who, rows->N);
    if (pol->n_sets < 1 || rows->N % pol->n_sets != 0)
        return wg_fail(WG_EINVAL, "%s: n_sets %d does not divide N = %d", who, pol->n_sets, rows->N);
    const int64_t D = pol->obs_dim, H = pol->hidden, C = pol->act_dim, n2 = H ? H : D;
    if ((int64_t)rows->N * D > INT32_MAX || (int64_t)rows->N * C > INT32_MAX || D * (H ? H : C) > INT32_MAX)
        return wg_fail(WG_ERANGE, "%s: a step's rows or a layer pass 2^31 elements", who);
    if (!rows->x) return wg_fail(WG_EINVAL, "%s: null x", who);
    if (rows->x_step < rows->N * D)
        return wg_fail(WG_EINVAL, "%s: x_step %lld < N * obs_dim = %lld", who, (long long)rows->x_step,
                       (long long)(rows->N * D));
    if (rows->mask && rows->mask_step < rows->N)
        return wg_fail(WG_EINVAL, "%s: mask_step %lld < N = %d", who, (long long)rows->mask_step, rows->N);
    PrArgs &a = pl->a;
    a = PrArgs{};
    a.x = rows->x; a.mask = rows->mask; a.x_step = rows->x_step; a.mask_step = rows->mask_step;
    a.w1 = H ? pol->w1 : nullptr; a.b1 = H ? pol->b1 : nullptr; a.w2 = pol->w2; a.b2 = pol->b2;
    a.n_steps = rows->n_steps; a.N = rows->N; a.n = rows->N / pol->n_sets;
    a.D = (int32_t)D; a.H = (int32_t)H; a.C = (int32_t)C; a.n2 = (int32_t)n2;
    a.Dp = up4(a.D + 1); a.Hq = up4(a.H + 1); a.Hp = up4(a.H); a.Cp = up4(a.C);
    pl->n_sets = pol->n_sets;
    pl->K = D * H + (a.b1 ? H : 0) + n2 * C + (a.b2 ? C : 0);
    pl->end[0] = (int32_t)(D * H); pl->end[1] = pl->end[0] + (a.b1 ? a.H : 0);
    pl->end[2] = pl->end[1] + (int32_t)(n2 * C); pl->end[3] = (int32_t)pl->K;
    return 0;
}

// The inputs every call reads, for the aliasing checks.
int pr_inputs(const PrPlan &pl, PrBuf *in) {
    const PrArgs &a = pl.a;
    const int64_t G = pl.n_sets;
    int n = 0;
    in[n++] = {"x", a.x, span_of(a.x, a.n_steps, (int64_t)a.N * a.D, a.x_step, 4)};
    if (a.mask) in[n++] = {"mask", a.mask, span_of(a.mask, a.n_steps, a.N, a.mask_step, 1)};
    if (a.w1) in[n++] = {"w1", a.w1, span_of(a.w1, 1, G * a.D * a.H, 0, 4)};
    if (a.b1) in[n++] = {"b1", a.b1, span_of(a.b1, 1, G * a.H, 0, 4)};
    in[n++] = {"w2", a.w2, span_of(a.w2, 1, G * a.n2 * a.C, 0, 4)};
    if (a.b2) in[n++] = {"b2", a.b2, span_of(a.b2, 1, G * a.C, 0, 4)};
    return n;
}

// The backward's own limits: the 4 x 4 blocks in the registers of one workgroup, the rows of a tile in its LDS.
int pr_backward_plan(PrPlan *pl, int32_t chunk_rows, const char *who, int64_t *n_chunks) {
    if (chunk_rows < 1) return wg_fail(WG_EINVAL, "%s: chunk_rows %d < 1", who, chunk_rows);
    PrArgs &a = pl->a;
    const int64_t t1 = a.H ? (int64_t)(a.Dp / 4) * (a.Hp / 4) : 0, t2 = (int64_t)((a.H ? a.Hq : a.Dp) / 4) * (a.Cp / 4);
    if (pl->K > WG_POLICY_GRAD_MAX_K || 16 * (t1 + t2) > WG_POLICY_GRAD_MAX_K)
        return wg_fail(WG_ERANGE, "%s: %lld parameters per set, %lld in 4 x 4 blocks (at most WG_POLICY_GRAD_MAX_K = %d)",
                       who, (long long)pl->K, (long long)(16 * (t1 + t2)), WG_POLICY_GRAD_MAX_K);
    pl->T1 = (int32_t)t1; pl->T2 = (int32_t)t2;
    const int row = 4 * (a.Dp + (a.H ? a.Hq + a.Hp : 0) + a.Cp) + 12;
    a.TR = PR_LDS / row < PR_BWD_ROWS ? PR_LDS / row : PR_BWD_ROWS;
    if (a.TR < 1) return wg_fail(WG_ERANGE, "%s: one row needs %d B of LDS (> 64 KiB)", who, row);
    *n_chunks = ((int64_t)a.n_steps * a.n + chunk_rows - 1) / chunk_rows;
    if (*n_chunks * pl->n_sets > INT32_MAX)
        return wg_fail(WG_ERANGE, "%s: %lld chunks in %d sets pass 2^31 workgroups", who, (long long)*n_chunks, pl->n_sets);
    return 0;
}

// wg_obs_norm's own refusals; the normaliser's arrays join the inputs of the aliasing checks.
int pr_norm_check(const wg_obs_norm *nm, const PrPlan &pl, const char *who, PrBuf *in, int *n_in) {
    if (!nm) return wg_fail(WG_EINVAL, "%s: null obs norm", who);
    if (!nm->mean) return wg_fail(WG_EINVAL, "%s: null mean", who);
    if (!nm->scale) return wg_fail(WG_EINVAL, "%s: null scale", who);
    if (!(nm->clip > 0.f)) return wg_fail(WG_EINVAL, "%s: clip must be > 0 (+inf allowed)", who);
    in[(*n_in)++] = {"mean", nm->mean, span_of(nm->mean, 1, pl.a.D, 0, 4)};
    in[(*n_in)++] = {"scale", nm->scale, span_of(nm->scale, 1, pl.a.D, 0, 4)};
    return 0;
}

int policy_forward(const char *who, const wg_policy *pol, const wg_obs_norm *nm, bool norm, const wg_policy_rows *rows,
                   float *y, int64_t y_step, hipStream_t stream) {
    PrPlan pl;
    if (const int rc = pr_check(pol, rows, who, &pl)) return rc;
    PrArgs &a = pl.a;
    if (!y) return wg_fail(WG_EINVAL, "%s: null y", who);
    if (y_step < (int64_t)a.N * a.C)
        return wg_fail(WG_EINVAL, "%s: y_step %lld < N * act_dim = %lld", who, (long long)y_step, (long long)a.N * a.C);
    PrBuf in[8];
    int n_in = pr_inputs(pl, in);
    if (norm)
        if (const int rc = pr_norm_check(nm, pl, who, in, &n_in)) return rc;
    const Span sy = span_of(y, a.n_steps, (int64_t)a.N * a.C, y_step, 4);
    for (int i = 0; i < n_in; i++)
        if (overlap(sy, in[i].s)) return wg_fail(WG_EINVAL, "%s: y aliases %s", who, in[i].name);
    a.Dp = a.D | 1; a.Hq = a.H | 1;                  // odd row lengths: the rows of a wave fall on distinct LDS banks
    const bool stage = pl.n_sets == 1 && pl.K * 4 <= PR_W_LDS;
    const int w_floats = stage ? up4((int)pl.K) : 0;
    const int row = 4 * (a.Dp + (a.H ? a.Hq : 0)) + 12, room = PR_LDS - 4 * w_floats;
    a.TR = room / row < PR_FWD_ROWS ? room / row : PR_FWD_ROWS;
    if (a.TR < 1) return wg_fail(WG_ERANGE, "%s: one row needs %d B of LDS (> %d)", who, row, room);
    const int64_t n_tiles = ((int64_t)a.n_steps * a.N + a.TR - 1) / a.TR;
    const int64_t cap = stage ? 2048 : 1 << 20;     // staged weights are loaded once per workgroup: few, long-lived
    const dim3 grid((unsigned)(n_tiles < cap ? n_tiles : cap));
    const size_t lds = (size_t)4 * w_floats + (size_t)a.TR * row;
    if (norm) {
        const PrNorm kn{nm->mean, nm->scale, nm->clip};
        if (stage) pr_forward<true, PrNorm><<<grid, PR_THREADS, lds, stream>>>(a, n_tiles, w_floats, y, y_step, kn);
        else pr_forward<false, PrNorm><<<grid, PR_THREADS, lds, stream>>>(a, n_tiles, w_floats, y, y_step, kn);
    } else {
        if (stage) pr_forward<true><<<grid, PR_THREADS, lds, stream>>>(a, n_tiles, w_floats, y, y_step, PrNone{});
        else pr_forward<false><<<grid, PR_THREADS, lds, stream>>>(a, n_tiles, w_floats, y, y_step, PrNone{});
    }
    return wg_launched(norm ? "wg_policy_forward_normalized: launch" : "wg_policy_forward: launch");
}

int policy_backward(const char *who, const wg_policy *pol, const wg_obs_norm *nm, bool norm, const wg_policy_rows *rows,
                    const float *dy, int64_t dy_step, int32_t chunk_rows, double *workspace, float *g_w1, float *g_b1,
                    float *g_w2, float *g_b2, hipStream_t stream) {
    PrPlan pl;
    int64_t n_chunks;
    if (const int rc = pr_check(pol, rows, who, &pl)) return rc;
    PrArgs &a = pl.a;
    if (!dy) return wg_fail(WG_EINVAL, "%s: null dy", who);
    if (!workspace) return wg_fail(WG_EINVAL, "%s: null workspace", who);
    if (dy_step < (int64_t)a.N * a.C)
        return wg_fail(WG_EINVAL, "%s: dy_step %lld < N * act_dim = %lld", who, (long long)dy_step, (long long)a.N * a.C);
    if (!g_w1 && !g_b1 && !g_w2 && !g_b2) return wg_fail(WG_EINVAL, "%s: every gradient pointer is null", who);
    if (!a.H && (g_w1 || g_b1)) return wg_fail(WG_EINVAL, "%s: g_w1 / g_b1 without a hidden layer", who);
    if (g_b1 && !a.b1) return wg_fail(WG_EINVAL, "%s: g_b1 of a policy without b1", who);
    if (g_b2 && !a.b2) return wg_fail(WG_EINVAL, "%s: g_b2 of a policy without b2", who);
    if (const int rc = pr_backward_plan(&pl, chunk_rows, who, &n_chunks)) return rc;
    PrBuf in[9], out[5];
    int n_in = pr_inputs(pl, in), n_out = 0;
    in[n_in++] = {"dy", dy, span_of(dy, a.n_steps, (int64_t)a.N * a.C, dy_step, 4)};
    if (norm)
        if (const int rc = pr_norm_check(nm, pl, who, in, &n_in)) return rc;
    const int64_t G = pl.n_sets;
    out[n_out++] = {"workspace", workspace, span_of(workspace, 1, G * n_chunks * pl.K, 0, 8)};
    if (g_w1) out[n_out++] = {"g_w1", g_w1, span_of(g_w1, 1, G * a.D * a.H, 0, 4)};
    if (g_b1) out[n_out++] = {"g_b1", g_b1, span_of(g_b1, 1, G * a.H, 0, 4)};
    if (g_w2) out[n_out++] = {"g_w2", g_w2, span_of(g_w2, 1, G * a.n2 * a.C, 0, 4)};
    if (g_b2) out[n_out++] = {"g_b2", g_b2, span_of(g_b2, 1, G * a.C, 0, 4)};
    for (int o = 0; o < n_out; o++) {
        for (int i = 0; i < n_in; i++)
            if (overlap(out[o].s, in[i].s)) return wg_fail(WG_EINVAL, "%s: %s aliases %s", who, out[o].name, in[i].name);
        for (int p = 0; p < o; p++)
            if (overlap(out[o].s, out[p].s)) return wg_fail(WG_EINVAL, "%s: %s aliases %s", who, out[o].name, out[p].name);
    }
    const int32_t T1 = (g_w1 || g_b1) ? pl.T1 : 0;     // without them neither dh nor the layer-1 product is computed
    const int nt = (T1 + pl.T2 + PR_THREADS - 1) / PR_THREADS;
    const size_t lds = (size_t)a.TR * (4 * (a.Dp + (a.H ? a.Hq + a.Hp : 0) + a.Cp) + 12);
    const dim3 grid((unsigned)(n_chunks * G));
    const int32_t K = (int32_t)pl.K;
    auto go = [&](auto kernel, auto kn) {
        kernel<<<grid, PR_THREADS, lds, stream>>>(a, dy, dy_step, chunk_rows, n_chunks, T1, workspace, K, kn);
    };
    if (norm) {
        const PrNorm kn{nm->mean, nm->scale, nm->clip};
        if (nt <= 1) go(pr_grad_partial<1, PrNorm>, kn);
        else if (nt == 2) go(pr_grad_partial<2, PrNorm>, kn);
        else if (nt == 3) go(pr_grad_partial<3, PrNorm>, kn);
        else go(pr_grad_partial<4, PrNorm>, kn);
    } else {
        if (nt <= 1) go(pr_grad_partial<1>, PrNone{});
        else if (nt == 2) go(pr_grad_partial<2>, PrNone{});
        else if (nt == 3) go(pr_grad_partial<3>, PrNone{});
        else go(pr_grad_partial<4>, PrNone{});
    }
    if (const int rc = wg_launched(norm ? "wg_policy_backward_normalized (partial sums): launch"
                                        : "wg_policy_backward (partial sums): launch"))
        return rc;
    PrGrads o{{g_w1, g_b1, g_w2, g_b2}, {pl.end[0], pl.end[1], pl.end[2], pl.end[3]}};
    const int64_t total = G * K;
    pr_grad_tail<<<(unsigned)((total + PR_THREADS - 1) / PR_THREADS), PR_THREADS, 0, stream>>>(workspace, o, K, n_chunks,
                                                                                             total);
    return wg_launched(norm ? "wg_policy_backward_normalized (tail): launch" : "wg_policy_backward (tail): launch");
}

// ---- deep policy rows: host
struct PrPlanDeep {
    PrPlan p;             // a.H = H1, a.n2 = H2; K over the six segments; p.end unused
    PrMid m;
    int32_t end[6];       // the ends of w1, b1, wm, bm, w2, b2 in [0, K]
    int32_t T1, Tm, T2;   // 4 x 4 blocks of the three outer products
};

// pr_check and the middle layer's own refusals; fills the plan (TR stays 0).
int pr_check_deep(const wg_policy *pol, const wg_policy_mid *mid, const wg_policy_rows *rows, const char *who,
                  PrPlanDeep *pl) {
    if (const int rc = pr_check(pol, rows, who, &pl->p)) return rc;
    if (!mid) return wg_fail(WG_EINVAL, "%s: null middle layer", who);
    if (mid->hidden2 < 1 || mid->hidden2 > 256) return wg_fail(WG_EINVAL, "%s: hidden2 %d outside 1..256", who, mid->hidden2);
    if (!mid->wm) return wg_fail(WG_EINVAL, "%s: null wm", who);
    if (pol->hidden == 0) return wg_fail(WG_EINVAL, "%s: a middle layer needs hidden > 0", who);
    PrArgs &a = pl->p.a;
    const int32_t H2 = mid->hidden2;
    a.n2 = H2;
    pl->m = PrMid{mid->wm, mid->bm, H2, up4(H2 + 1), up4(H2)};
    const int32_t seg[6] = {a.D * a.H, a.b1 ? a.H : 0, a.H * H2, mid->bm ? H2 : 0, H2 * a.C, a.b2 ? a.C : 0};
    int32_t at = 0;
    for (int i = 0; i < 6; i++) pl->end[i] = (at += seg[i]);
    pl->p.K = at;
    return 0;
}

int pr_inputs_deep(const PrPlanDeep &pl, PrBuf *in) {
    const PrArgs &a = pl.p.a;
    const int64_t G = pl.p.n_sets;
    int n = pr_inputs(pl.p, in);      // (w2 over a.n2 = H2 inputs)
    in[n++] = {"wm", pl.m.wm, span_of(pl.m.wm, 1, G * a.H * pl.m.H2, 0, 4)};
    if (pl.m.bm) in[n++] = {"bm", pl.m.bm, span_of(pl.m.bm, 1, G * pl.m.H2, 0, 4)};
    return n;
}

int pr_backward_plan_deep(PrPlanDeep *pl, int32_t chunk_rows, const char *who, int64_t *n_chunks) {
    if (chunk_rows < 1) return wg_fail(WG_EINVAL, "%s: chunk_rows %d < 1", who, chunk_rows);
    PrArgs &a = pl->p.a;
    const PrMid &m = pl->m;
    const int64_t t1 = (int64_t)(a.Dp / 4) * (a.Hp / 4), tm = (int64_t)(a.Hq / 4) * (m.Gp / 4),
                  t2 = (int64_t)(m.Gq / 4) * (a.Cp / 4);
    if (pl->p.K > WG_POLICY_GRAD_MAX_K || 16 * (t1 + tm + t2) > WG_POLICY_GRAD_MAX_K)
        return wg_fail(WG_ERANGE, "%s: %lld parameters per set, %lld in 4 x 4 blocks (at most WG_POLICY_GRAD_MAX_K = %d)",
                       who, (long long)pl->p.K, (long long)(16 * (t1 + tm + t2)), WG_POLICY_GRAD_MAX_K);
    pl->T1 = (int32_t)t1; pl->Tm = (int32_t)tm; pl->T2 = (int32_t)t2;
    const int row = 4 * (a.Dp + a.Hq + a.Hp + m.Gq + m.Gp + a.Cp) + 12;
    a.TR = PR_LDS / row < PR_BWD_ROWS ? PR_LDS / row : PR_BWD_ROWS;
    if (a.TR < 1) return wg_fail(WG_ERANGE, "%s: one row needs %d B of LDS (> 64 KiB)", who, row);
    *n_chunks = ((int64_t)a.n_steps * a.n + chunk_rows - 1) / chunk_rows;
    if (*n_chunks * pl->p.n_sets > INT32_MAX)
        return wg_fail(WG_ERANGE, "%s: %lld chunks in %d sets pass 2^31 workgroups", who, (long long)*n_chunks,
                       pl->p.n_sets);
    return 0;
}

int policy_forward_deep(const char *who, const wg_policy *pol, const wg_policy_mid *mid, const wg_obs_norm *nm,
                        const wg_policy_rows *rows, float *y, int64_t y_step, hipStream_t stream) {
    PrPlanDeep pl;
    if (const int rc = pr_check_deep(pol, mid, rows, who, &pl)) return rc;
    PrArgs &a = pl.p.a;
    PrMid &m = pl.m;
    if (!y) return wg_fail(WG_EINVAL, "%s: null y", who);
    if (y_step < (int64_t)a.N * a.C)
        return wg_fail(WG_EINVAL, "%s: y_step %lld < N * act_dim = %lld", who, (long long)y_step, (long long)a.N * a.C);
    PrBuf in[10];
    int n_in = pr_inputs_deep(pl, in);
    if (nm)
        if (const int rc = pr_norm_check(nm, pl.p, who, in, &n_in)) return rc;
    const Span sy = span_of(y, a.n_steps, (int64_t)a.N * a.C, y_step, 4);
    for (int i = 0; i < n_in; i++)
        if (overlap(sy, in[i].s)) return wg_fail(WG_EINVAL, "%s: y aliases %s", who, in[i].name);
    a.Dp = a.D | 1; a.Hq = a.H | 1; m.Gq = m.H2 | 1;   // odd row lengths: the rows of a wave fall on distinct LDS banks
    const bool stage = pl.p.n_sets == 1 && pl.p.K * 4 <= PR_W_LDS;   // (the middle matrix counted)
    const int w_floats = stage ? up4((int)pl.p.K) : 0;
    const int row = 4 * (a.Dp + a.Hq + m.Gq) + 12, room = PR_LDS - 4 * w_floats;
    a.TR = room / row < PR_FWD_ROWS ? room / row : PR_FWD_ROWS;
    if (a.TR < 1) return wg_fail(WG_ERANGE, "%s: one row needs %d B of LDS (> %d)", who, row, room);
    const int64_t n_tiles = ((int64_t)a.n_steps * a.N + a.TR - 1) / a.TR;
    const int64_t cap = stage ? 2048 : 1 << 20;
    const dim3 grid((unsigned)(n_tiles < cap ? n_tiles : cap));
    const size_t lds = (size_t)4 * w_floats + (size_t)a.TR * row;
    if (nm) {
        const PrNorm kn{nm->mean, nm->scale, nm->clip};
        if (stage) pr_forward_deep<true, PrNorm><<<grid, PR_THREADS, lds, stream>>>(a, m, n_tiles, w_floats, y, y_step, kn);
        else pr_forward_deep<false, PrNorm><<<grid, PR_THREADS, lds, stream>>>(a, m, n_tiles, w_floats, y, y_step, kn);
    } else {
        if (stage) pr_forward_deep<true><<<grid, PR_THREADS, lds, stream>>>(a, m, n_tiles, w_floats, y, y_step, PrNone{});
        else pr_forward_deep<false><<<grid, PR_THREADS, lds, stream>>>(a, m, n_tiles, w_floats, y, y_step, PrNone{});
    }
    return wg_launched("wg_policy_forward_deep: launch");
}

int policy_backward_deep(const char *who, const wg_policy *pol, const wg_policy_mid *mid, const wg_obs_norm *nm,
                         const wg_policy_rows *rows, const float *dy, int64_t dy_step, int32_t chunk_rows,
                         double *workspace, float *g_w1, float *g_b1, float *g_wm, float *g_bm, float *g_w2, float *g_b2,
                         hipStream_t stream) {
    PrPlanDeep pl;
    int64_t n_chunks;
    if (const int rc = pr_check_deep(pol, mid, rows, who, &pl)) return rc;
    PrArgs &a = pl.p.a;
    const PrMid &m = pl.m;
    if (!dy) return wg_fail(WG_EINVAL, "%s: null dy", who);
    if (!workspace) return wg_fail(WG_EINVAL, "%s: null workspace", who);
    if (dy_step < (int64_t)a.N * a.C)
        return wg_fail(WG_EINVAL, "%s: dy_step %lld < N * act_dim = %lld", who, (long long)dy_step, (long long)a.N * a.C);
    if (!g_w1 && !g_b1 && !g_wm && !g_bm && !g_w2 && !g_b2)
        return wg_fail(WG_EINVAL, "%s: every gradient pointer is null", who);
    if (g_b1 && !a.b1) return wg_fail(WG_EINVAL, "%s: g_b1 of a policy without b1", who);
    if (g_bm && !m.bm) return wg_fail(WG_EINVAL, "%s: g_bm of a policy without bm", who);
    if (g_b2 && !a.b2) return wg_fail(WG_EINVAL, "%s: g_b2 of a policy without b2", who);
    if (const int rc = pr_backward_plan_deep(&pl, chunk_rows, who, &n_chunks)) return rc;
    PrBuf in[11], out[7];
    int n_in = pr_inputs_deep(pl, in), n_out = 0;
    in[n_in++] = {"dy", dy, span_of(dy, a.n_steps, (int64_t)a.N * a.C, dy_step, 4)};
    if (nm)
        if (const int rc = pr_norm_check(nm, pl.p, who, in, &n_in)) return rc;
    const int64_t G = pl.p.n_sets;
    out[n_out++] = {"workspace", workspace, span_of(workspace, 1, G * n_chunks * pl.p.K, 0, 8)};
    if (g_w1) out[n_out++] = {"g_w1", g_w1, span_of(g_w1, 1, G * a.D * a.H, 0, 4)};
    if (g_b1) out[n_out++] = {"g_b1", g_b1, span_of(g_b1, 1, G * a.H, 0, 4)};
    if (g_wm) out[n_out++] = {"g_wm", g_wm, span_of(g_wm, 1, G * a.H * m.H2, 0, 4)};
    if (g_bm) out[n_out++] = {"g_bm", g_bm, span_of(g_bm, 1, G * m.H2, 0, 4)};
    if (g_w2) out[n_out++] = {"g_w2", g_w2, span_of(g_w2, 1, G * m.H2 * a.C, 0, 4)};
    if (g_b2) out[n_out++] = {"g_b2", g_b2, span_of(g_b2, 1, G * a.C, 0, 4)};
    for (int o = 0; o < n_out; o++) {
        for (int i = 0; i < n_in; i++)
            if (overlap(out[o].s, in[i].s)) return wg_fail(WG_EINVAL, "%s: %s aliases %s", who, out[o].name, in[i].name);
        for (int p = 0; p < o; p++)
            if (overlap(out[o].s, out[p].s)) return wg_fail(WG_EINVAL, "%s: %s aliases %s", who, out[o].name, out[p].name);
    }
    // without g_w1 / g_b1 neither dh1 nor the first product is computed; without g_wm / g_bm too, neither is dh2
    const int32_t T1 = (g_w1 || g_b1) ? pl.T1 : 0, Tm = (g_wm || g_bm) ? pl.Tm : 0;
    const int nt = (T1 + Tm + pl.T2 + PR_THREADS - 1) / PR_THREADS;
    const size_t lds = (size_t)a.TR * (4 * (a.Dp + a.Hq + a.Hp + m.Gq + m.Gp + a.Cp) + 12);
    const dim3 grid((unsigned)(n_chunks * G));
    const int32_t K = (int32_t)pl.p.K;
    auto go = [&](auto kernel, auto kn) {
        kernel<<<grid, PR_THREADS, lds, stream>>>(a, m, dy, dy_step, chunk_rows, n_chunks, T1, Tm, workspace, K, kn);
    };
    if (nm) {
        const PrNorm kn{nm->mean, nm->scale, nm->clip};
        if (nt <= 1) go(pr_grad_partial_deep<1, PrNorm>, kn);
        else if (nt == 2) go(pr_grad_partial_deep<2, PrNorm>, kn);
        else if (nt == 3) go(pr_grad_partial_deep<3, PrNorm>, kn);
        else go(pr_grad_partial_deep<4, PrNorm>, kn);
    } else {
        if (nt <= 1) go(pr_grad_partial_deep<1>, PrNone{});
        else if (nt == 2) go(pr_grad_partial_deep<2>, PrNone{});
        else if (nt == 3) go(pr_grad_partial_deep<3>, PrNone{});
        else go(pr_grad_partial_deep<4>, PrNone{});
    }
    if (const int rc = wg_launched("wg_policy_backward_deep (partial sums): launch")) return rc;
    PrGrads6 o{{g_w1, g_b1, g_wm, g_bm, g_w2, g_b2},
               {pl.end[0], pl.end[1], pl.end[2], pl.end[3], pl.end[4], pl.end[5]}};
    const int64_t total = G * K;
    pr_grad_tail_deep<<<(unsigned)((total + PR_THREADS - 1) / PR_THREADS), PR_THREADS, 0, stream>>>(workspace, o, K,
                                                                                                  n_chunks, total);
    return wg_launched("wg_policy_backward_deep (tail): launch");
}

// wg_obs_moments' checks, shared with wg_obs_moments_workspace; fills the kernel's arguments and the chunk count.
int om_check(const wg_policy_rows *rows, int32_t obs_dim, int32_t chunk_rows, const char *who, OmArgs *a,
             int64_t *n_chunks) {
    if (!rows) return wg_fail(WG_EINVAL, "%s: null rows", who);
    if (!rows->x) return wg_fail(WG_EINVAL, "%s: null x", who);
    if (obs_dim < 1) return wg_fail(WG_EINVAL, "%s: obs_dim %d < 1", who, obs_dim);
    if (rows->n_steps < 1) return wg_fail(WG_EINVAL, "%s: n_steps %d < 1", who, rows->n_steps);
    if (rows->N < 1) return wg_fail(WG_EINVAL, "%s: N %d < 1", who, rows->N);
    if (chunk_rows < 1) return wg_fail(WG_EINVAL, "%s: chunk_rows %d < 1", who, chunk_rows);
    const int64_t D = obs_dim;
    if (rows->x_step < rows->N * D)
        return wg_fail(WG_EINVAL, "%s: x_step %lld < N * obs_dim = %lld", who, (long long)rows->x_step,
                       (long long)(rows->N * D));
    if (rows->mask && rows->mask_step < rows->N)
        return wg_fail(WG_EINVAL, "%s: mask_step %lld < N = %d", who, (long long)rows->mask_step, rows->N);
    if ((int64_t)rows->N * D > INT32_MAX) return wg_fail(WG_ERANGE, "%s: a step's rows pass 2^31 elements", who);
    *a = OmArgs{};
    a->x = rows->x; a->mask = rows->mask; a->x_step = rows->x_step; a->mask_step = rows->mask_step;
    a->rows = (int64_t)rows->n_steps * rows->N;
    a->N = rows->N; a->D = obs_dim; a->chunk_rows = chunk_rows;
    const int64_t row = 4 * D + 4;
    a->TR = (int32_t)(PR_LDS / row < OM_ROWS ? PR_LDS / row : OM_ROWS);
    if (a->TR < 1) return wg_fail(WG_ERANGE, "%s: one row needs %lld B of LDS (> 64 KiB)", who, (long long)row);
    *n_chunks = (a->rows + chunk_rows - 1) / chunk_rows;
    if (*n_chunks > INT32_MAX) return wg_fail(WG_ERANGE, "%s: %lld chunks pass 2^31 workgroups", who, (long long)*n_chunks);
    return 0;
}

// What wg_ppo_surrogate_workspace and wg_ppo_surrogate check alike, in the header's order; fills the rows' part of the
// kernel's arguments and the chunk count.
int ppo_check(const wg_ppo_rows *rows, int32_t chunk_rows, const char *who, PpoArgs *a, int64_t *n_chunks) {
    if (!rows) return wg_fail(WG_EINVAL, "%s: null rows", who);
    if (!rows->y) return wg_fail(WG_EINVAL, "%s: null y", who);
    if (!rows->u) return wg_fail(WG_EINVAL, "%s: null u", who);
    if (!rows->sigma) return wg_fail(WG_EINVAL, "%s: null sigma", who);
    if (!rows->log_sigma) return wg_fail(WG_EINVAL, "%s: null log_sigma", who);
    if (rows->act_dim < 1 || rows->act_dim > 256)
        return wg_fail(WG_EINVAL, "%s: act_dim %d outside 1..256", who, rows->act_dim);
    if (rows->n_steps < 1) return wg_fail(WG_EINVAL, "%s: n_steps %d < 1", who, rows->n_steps);
    if (rows->N < 1) return wg_fail(WG_EINVAL, "%s: N %d < 1", who, rows->N);
    if (rows->n_sets < 1 || rows->N % rows->n_sets != 0)
        return wg_fail(WG_EINVAL, "%s: n_sets %d does not divide N = %d", who, rows->n_sets, rows->N);
    const int64_t NC = (int64_t)rows->N * rows->act_dim;
    if (NC > INT32_MAX) return wg_fail(WG_ERANGE, "%s: a step's rows pass 2^31 elements", who);
    if (rows->y_step < NC)
        return wg_fail(WG_EINVAL, "%s: y_step %lld < N * act_dim = %lld", who, (long long)rows->y_step, (long long)NC);
    if (rows->u_step < NC)
        return wg_fail(WG_EINVAL, "%s: u_step %lld < N * act_dim = %lld", who, (long long)rows->u_step, (long long)NC);
    if (rows->mask && rows->mask_step < rows->N)
        return wg_fail(WG_EINVAL, "%s: mask_step %lld < N = %d", who, (long long)rows->mask_step, rows->N);
    if (chunk_rows < 1) return wg_fail(WG_EINVAL, "%s: chunk_rows %d < 1", who, chunk_rows);
    *a = PpoArgs{};
    a->y = rows->y; a->u = rows->u; a->sigma = rows->sigma; a->log_sigma = rows->log_sigma; a->mask = rows->mask;
    a->y_step = rows->y_step; a->u_step = rows->u_step; a->mask_step = rows->mask ? rows->mask_step : 0;
    a->n_steps = rows->n_steps; a->N = rows->N; a->n = rows->N / rows->n_sets;
    a->C = rows->act_dim; a->Cs = rows->act_dim | 1; a->chunk_rows = chunk_rows;
    const int row = 4 * (a->Cs + PPO_STATS);
    a->TR = PR_LDS / row < PR_THREADS ? PR_LDS / row : PR_THREADS;
    *n_chunks = ((int64_t)a->n_steps * a->n + chunk_rows - 1) / chunk_rows;
    if (*n_chunks * rows->n_sets > INT32_MAX)
        return wg_fail(WG_ERANGE, "%s: %lld chunks in %d sets pass 2^31 workgroups", who, (long long)*n_chunks,
                       rows->n_sets);
    return 0;
}

bool aligned16(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

}  // namespace

extern "C" {

int wg_expf(const float *x, int64_t n, float *out, hipStream_t stream) {
    if (!x) return wg_fail(WG_EINVAL, "wg_expf: null x");
    if (!out) return wg_fail(WG_EINVAL, "wg_expf: null out");
    if (n < 1) return wg_fail(WG_EINVAL, "wg_expf: n %lld < 1", (long long)n);
    if (x != out && overlap(span_of(x, 1, n, 0, 4), span_of(out, 1, n, 0, 4)))
        return wg_fail(WG_EINVAL, "wg_expf: out overlaps x without being x");
    const int64_t blocks = (n + PR_THREADS - 1) / PR_THREADS;
    expf_rows<<<(unsigned)(blocks < (1 << 20) ? blocks : (1 << 20)), PR_THREADS, 0, stream>>>(x, n, out);
    return wg_launched("wg_expf: launch");
}

int64_t wg_ppo_surrogate_workspace(const wg_ppo_rows *rows, int32_t chunk_rows) {
    PpoArgs a;
    int64_t n_chunks;
    if (const int rc = ppo_check(rows, chunk_rows, "wg_ppo_surrogate_workspace", &a, &n_chunks)) return rc;
    return (int64_t)rows->n_sets * n_chunks * (a.C + PPO_STATS);
}

int wg_ppo_surrogate(const wg_ppo_rows *rows, const float *old_logp, const float *adv, int64_t row_step,
                     const float *value, const float *ret, const float *scale, float clip_eps, int32_t chunk_rows,
                     double *workspace, float *logp_out, float *dy, int64_t dy_step, float *dvalue, float *g_log_sigma,
                     double *stats, hipStream_t stream) {
    const char *who = "wg_ppo_surrogate";
    PpoArgs a;
    int64_t n_chunks;
    if (const int rc = ppo_check(rows, chunk_rows, who, &a, &n_chunks)) return rc;
    if (row_step < a.N) return wg_fail(WG_EINVAL, "%s: row_step %lld < N = %d", who, (long long)row_step, a.N);
    const int64_t NC = (int64_t)a.N * a.C;
    if (dy && dy_step < NC)
        return wg_fail(WG_EINVAL, "%s: dy_step %lld < N * act_dim = %lld", who, (long long)dy_step, (long long)NC);
    const bool density = old_logp == nullptr;
    if (density) {
        if (adv || value || ret || scale || dy || dvalue || g_log_sigma || stats || workspace)
            return wg_fail(WG_EINVAL, "%s: without old_logp (the density alone) only logp_out may be set", who);
        if (!logp_out) return wg_fail(WG_EINVAL, "%s: without old_logp (the density alone) logp_out is required", who);
    } else {
        if (!adv) return wg_fail(WG_EINVAL, "%s: null adv", who);
        if (!scale) return wg_fail(WG_EINVAL, "%s: null scale", who);
        if (!workspace) return wg_fail(WG_EINVAL, "%s: null workspace", who);
    }
    if ((value == nullptr) != (ret == nullptr)) return wg_fail(WG_EINVAL, "%s: value and ret go together", who);
    if (dvalue && !value) return wg_fail(WG_EINVAL, "%s: dvalue without value", who);
    if (!(clip_eps >= 0.f) || !std::isfinite(clip_eps))
        return wg_fail(WG_EINVAL, "%s: clip_eps must be finite and >= 0", who);
    if (!logp_out && !dy && !dvalue && !g_log_sigma && !stats)
        return wg_fail(WG_EINVAL, "%s: every output pointer is null", who);
    const int64_t G = rows->n_sets, J = a.C + PPO_STATS;
    PrBuf in[10], out[6];
    int n_in = 0, n_out = 0;
    in[n_in++] = {"y", a.y, span_of(a.y, a.n_steps, NC, a.y_step, 4)};
    in[n_in++] = {"u", a.u, span_of(a.u, a.n_steps, NC, a.u_step, 4)};
    in[n_in++] = {"sigma", a.sigma, span_of(a.sigma, 1, G * a.C, 0, 4)};
    in[n_in++] = {"log_sigma", a.log_sigma, span_of(a.log_sigma, 1, G * a.C, 0, 4)};
    if (a.mask) in[n_in++] = {"mask", a.mask, span_of(a.mask, a.n_steps, a.N, a.mask_step, 1)};
    if (old_logp) in[n_in++] = {"old_logp", old_logp, span_of(old_logp, a.n_steps, a.N, row_step, 4)};
    if (adv) in[n_in++] = {"adv", adv, span_of(adv, a.n_steps, a.N, row_step, 4)};
    if (value) in[n_in++] = {"value", value, span_of(value, a.n_steps, a.N, row_step, 4)};
    if (ret) in[n_in++] = {"ret", ret, span_of(ret, a.n_steps, a.N, row_step, 4)};
    if (scale) in[n_in++] = {"scale", scale, span_of(scale, 1, 2, 0, 4)};
    if (workspace) out[n_out++] = {"workspace", workspace, span_of(workspace, 1, G * n_chunks * J, 0, 8)};
    if (logp_out) out[n_out++] = {"logp_out", logp_out, span_of(logp_out, a.n_steps, a.N, row_step, 4)};
    if (dy) out[n_out++] = {"dy", dy, span_of(dy, a.n_steps, NC, dy_step, 4)};
    if (dvalue) out[n_out++] = {"dvalue", dvalue, span_of(dvalue, a.n_steps, a.N, row_step, 4)};
    if (g_log_sigma) out[n_out++] = {"g_log_sigma", g_log_sigma, span_of(g_log_sigma, 1, G * a.C, 0, 4)};
    if (stats) out[n_out++] = {"stats", stats, span_of(stats, 1, PPO_STATS, 0, 8)};
    for (int o = 0; o < n_out; o++) {
        for (int i = 0; i < n_in; i++)
            if (overlap(out[o].s, in[i].s)) return wg_fail(WG_EINVAL, "%s: %s aliases %s", who, out[o].name, in[i].name);
        for (int p = 0; p < o; p++)
            if (overlap(out[o].s, out[p].s)) return wg_fail(WG_EINVAL, "%s: %s aliases %s", who, out[o].name, out[p].name);
    }
    a.old_logp = old_logp; a.adv = adv; a.value = value; a.ret = ret; a.scale = scale;
    a.logp_out = logp_out; a.dy = dy; a.dvalue = dvalue; a.row_step = row_step; a.dy_step = dy ? dy_step : 0;
    a.lo = 1.0f - clip_eps; a.hi = 1.0f + clip_eps;   // one float32 operation each (-ffp-contract=off)
    const bool v4 = a.C % 4 == 0 && a.y_step % 4 == 0 && a.u_step % 4 == 0 && a.dy_step % 4 == 0 && aligned16(a.y) &&
                    aligned16(a.u) && aligned16(dy);
    if (density) {
        const int64_t n_rows = (int64_t)a.n_steps * a.N, blocks = (n_rows + PR_THREADS - 1) / PR_THREADS;
        if (blocks > INT32_MAX) return wg_fail(WG_ERANGE, "%s: %lld rows pass 2^31 workgroups", who, (long long)n_rows);
        if (v4) ppo_logp_rows<true><<<(unsigned)blocks, PR_THREADS, 0, stream>>>(a, n_rows);
        else ppo_logp_rows<false><<<(unsigned)blocks, PR_THREADS, 0, stream>>>(a, n_rows);
        return wg_launched("wg_ppo_surrogate (density): launch");
    }
    const size_t lds = (size_t)a.TR * 4 * (a.Cs + PPO_STATS);
    const dim3 grid((unsigned)(n_chunks * G));
    if (v4) ppo_rows_partial<true><<<grid, PR_THREADS, lds, stream>>>(a, n_chunks, workspace);
    else ppo_rows_partial<false><<<grid, PR_THREADS, lds, stream>>>(a, n_chunks, workspace);
    if (const int rc = wg_launched("wg_ppo_surrogate (partial sums): launch")) return rc;
    if (!g_log_sigma && !stats) return 0;
    ppo_rows_tail<<<1, PR_THREADS, 0, stream>>>(workspace, n_chunks, (int32_t)G, a.C, g_log_sigma, stats);
    return wg_launched("wg_ppo_surrogate (tail): launch");
}

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

int wg_gae_held(const float *hold_reward, const float *value, const float *next_value, const uint8_t *decided,
                const uint8_t *term, const uint8_t *cut, int32_t n_steps, int32_t N, int64_t step_stride, float gamma,
                float lam, float *adv, float *ret, hipStream_t stream) {
    if (!hold_reward) return wg_fail(WG_EINVAL, "wg_gae_held: null hold_reward");
    if (!value) return wg_fail(WG_EINVAL, "wg_gae_held: null value");
    if (!next_value) return wg_fail(WG_EINVAL, "wg_gae_held: null next_value");
    if (!decided) return wg_fail(WG_EINVAL, "wg_gae_held: null decided");
    if (!adv) return wg_fail(WG_EINVAL, "wg_gae_held: null adv");
    if (n_steps < 1) return wg_fail(WG_EINVAL, "wg_gae_held: n_steps %d < 1", n_steps);
    if (N < 1) return wg_fail(WG_EINVAL, "wg_gae_held: N %d < 1", N);
    if (step_stride < N)
        return wg_fail(WG_EINVAL, "wg_gae_held: step_stride %lld < N = %d", (long long)step_stride, N);
    if (!std::isfinite(gamma)) return wg_fail(WG_EINVAL, "wg_gae_held: gamma is not finite");
    if (!std::isfinite(lam)) return wg_fail(WG_EINVAL, "wg_gae_held: lam is not finite");
    const struct { const char *name; const void *p; int elem; } in[] = {
        {"hold_reward", hold_reward, 4}, {"value", value, 4}, {"next_value", next_value, 4}, {"decided", decided, 1},
        {"term", term, 1}, {"cut", cut, 1}};
    const Span sa = span_of(adv, n_steps, N, step_stride, 4);
    for (const auto &i : in) {
        if (!i.p) continue;
        const Span si = span_of(i.p, n_steps, N, step_stride, i.elem);
        if (overlap(sa, si)) return wg_fail(WG_EINVAL, "wg_gae_held: adv aliases %s", i.name);
        if (ret && overlap(span_of(ret, n_steps, N, step_stride, 4), si))
            return wg_fail(WG_EINVAL, "wg_gae_held: ret aliases %s", i.name);
    }
    if (ret && overlap(sa, span_of(ret, n_steps, N, step_stride, 4)))
        return wg_fail(WG_EINVAL, "wg_gae_held: adv aliases ret");
    const float gl = gamma * lam;   // one float32 multiply (-ffp-contract=off)
    const dim3 grid((N + GAE_THREADS - 1) / GAE_THREADS);
    auto go = [&](auto kernel) {
        kernel<<<grid, GAE_THREADS, 0, stream>>>(hold_reward, value, next_value, decided, term, cut, n_steps, N,
                                                 step_stride, gamma, gl, adv, ret);
    };
    if (term && cut) go(gae_held_scan<true, true>);
    else if (term) go(gae_held_scan<true, false>);
    else if (cut) go(gae_held_scan<false, true>);
    else go(gae_held_scan<false, false>);
    return wg_launched("wg_gae_held: launch");
}

int wg_policy_forward(const wg_policy *pol, const wg_policy_rows *rows, float *y, int64_t y_step, hipStream_t stream) {
    return policy_forward("wg_policy_forward", pol, nullptr, false, rows, y, y_step, stream);
}

int wg_policy_forward_normalized(const wg_policy *pol, const wg_obs_norm *nm, const wg_policy_rows *rows, float *y,
                                 int64_t y_step, hipStream_t stream) {
    return policy_forward("wg_policy_forward_normalized", pol, nm, true, rows, y, y_step, stream);
}

int64_t wg_policy_backward_workspace(const wg_policy *pol, const wg_policy_rows *rows, int32_t chunk_rows) {
    PrPlan pl;
    int64_t n_chunks;
    if (const int rc = pr_check(pol, rows, "wg_policy_backward_workspace", &pl)) return rc;
    if (const int rc = pr_backward_plan(&pl, chunk_rows, "wg_policy_backward_workspace", &n_chunks)) return rc;
    return (int64_t)pl.n_sets * n_chunks * pl.K;
}

int wg_policy_backward(const wg_policy *pol, const wg_policy_rows *rows, const float *dy, int64_t dy_step,
                       int32_t chunk_rows, double *workspace, float *g_w1, float *g_b1, float *g_w2, float *g_b2,
                       hipStream_t stream) {
    return policy_backward("wg_policy_backward", pol, nullptr, false, rows, dy, dy_step, chunk_rows, workspace, g_w1, g_b1,
                           g_w2, g_b2, stream);
}

int wg_policy_backward_normalized(const wg_policy *pol, const wg_obs_norm *nm, const wg_policy_rows *rows,
                                  const float *dy, int64_t dy_step, int32_t chunk_rows, double *workspace, float *g_w1,
                                  float *g_b1, float *g_w2, float *g_b2, hipStream_t stream) {
    return policy_backward("wg_policy_backward_normalized", pol, nm, true, rows, dy, dy_step, chunk_rows, workspace, g_w1,
                           g_b1, g_w2, g_b2, stream);
}

int wg_policy_forward_deep(const wg_policy *pol, const wg_policy_mid *mid, const wg_obs_norm *nm,
                           const wg_policy_rows *rows, float *y, int64_t y_step, hipStream_t stream) {
    return policy_forward_deep("wg_policy_forward_deep", pol, mid, nm, rows, y, y_step, stream);
}

int64_t wg_policy_backward_deep_workspace(const wg_policy *pol, const wg_policy_mid *mid, const wg_policy_rows *rows,
                                          int32_t chunk_rows) {
    PrPlanDeep pl;
    int64_t n_chunks;
    if (const int rc = pr_check_deep(pol, mid, rows, "wg_policy_backward_deep_workspace", &pl)) return rc;
    if (const int rc = pr_backward_plan_deep(&pl, chunk_rows, "wg_policy_backward_deep_workspace", &n_chunks)) return rc;
    return (int64_t)pl.p.n_sets * n_chunks * pl.p.K;
}

int wg_policy_backward_deep(const wg_policy *pol, const wg_policy_mid *mid, const wg_obs_norm *nm,
                            const wg_policy_rows *rows, const float *dy, int64_t dy_step, int32_t chunk_rows,
                            double *workspace, float *g_w1, float *g_b1, float *g_wm, float *g_bm, float *g_w2,
                            float *g_b2, hipStream_t stream) {
    return policy_backward_deep("wg_policy_backward_deep", pol, mid, nm, rows, dy, dy_step, chunk_rows, workspace, g_w1,
                                g_b1, g_wm, g_bm, g_w2, g_b2, stream);
}

int64_t wg_obs_moments_workspace(const wg_policy_rows *rows, int32_t obs_dim, int32_t chunk_rows) {
    OmArgs a;
    int64_t n_chunks;
    if (const int rc = om_check(rows, obs_dim, chunk_rows, "wg_obs_moments_workspace", &a, &n_chunks)) return rc;
    return n_chunks * (1 + 2 * (int64_t)obs_dim);
}

int wg_obs_moments(const wg_policy_rows *rows, int32_t obs_dim, float bound, int32_t chunk_rows, double *workspace,
                   double *state, double eps, float *mean_out, float *scale_out, hipStream_t stream) {
    const char *who = "wg_obs_moments";
    OmArgs a;
    int64_t n_chunks;
    if (const int rc = om_check(rows, obs_dim, chunk_rows, who, &a, &n_chunks)) return rc;
    if (!workspace) return wg_fail(WG_EINVAL, "%s: null workspace", who);
    if (!state) return wg_fail(WG_EINVAL, "%s: null state", who);
    if (!(bound > 0.f)) return wg_fail(WG_EINVAL, "%s: bound must be > 0 (+inf allowed)", who);
    if (!(eps >= 0.0)) return wg_fail(WG_EINVAL, "%s: eps must be >= 0", who);
    if ((mean_out == nullptr) != (scale_out == nullptr))
        return wg_fail(WG_EINVAL, "%s: mean_out and scale_out go together", who);
    const int64_t W = 1 + 2 * (int64_t)a.D;
    PrBuf in[2], out[4];
    int n_in = 0, n_out = 0;
    in[n_in++] = {"x", a.x, span_of(a.x, rows->n_steps, (int64_t)a.N * a.D, a.x_step, 4)};
    if (a.mask) in[n_in++] = {"mask", a.mask, span_of(a.mask, rows->n_steps, a.N, a.mask_step, 1)};
    out[n_out++] = {"workspace", workspace, span_of(workspace, 1, n_chunks * W, 0, 8)};
    out[n_out++] = {"state", state, span_of(state, 1, W, 0, 8)};
    if (mean_out) out[n_out++] = {"mean_out", mean_out, span_of(mean_out, 1, a.D, 0, 4)};
    if (scale_out) out[n_out++] = {"scale_out", scale_out, span_of(scale_out, 1, a.D, 0, 4)};
    for (int o = 0; o < n_out; o++) {
        for (int i = 0; i < n_in; i++)
            if (overlap(out[o].s, in[i].s)) return wg_fail(WG_EINVAL, "%s: %s aliases %s", who, out[o].name, in[i].name);
        for (int p = 0; p < o; p++)
            if (overlap(out[o].s, out[p].s)) return wg_fail(WG_EINVAL, "%s: %s aliases %s", who, out[o].name, out[p].name);
    }
    a.bound = bound;
    const size_t lds = (size_t)a.TR * (4 * (size_t)a.D + 4);
    obs_moments_partial<<<(unsigned)n_chunks, PR_THREADS, lds, stream>>>(a, workspace);
    if (const int rc = wg_launched("wg_obs_moments (partial sums): launch")) return rc;
    obs_moments_tail<<<1, PR_THREADS, 0, stream>>>(workspace, n_chunks, a.D, state, eps, mean_out, scale_out);
    return wg_launched("wg_obs_moments (tail): launch");
}

}  // extern "C"
