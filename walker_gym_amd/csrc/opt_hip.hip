// opt_hip.hip — the device optimiser of libwalker_hip.so: wg_adam_step, a global-norm clip and Adam / AdamW over up to
// WG_OPT_MAX_SEGMENTS float32 tensors in one call (include/walker_hip.h, "Device optimiser", has the contract; DESIGN.md
// §9m the reasons).  A unit of its own beside es_hip.hip and pg_hip.hip: the same flags, the same library.
//
// The segment table travels by value in the kernel arguments (32 x 40 B and the 33 element offsets: 1.6 KB of the 4 KB a
// dispatch carries), so the call allocates nothing and copies nothing.  Every kernel walks the table with a loop whose
// index is uniform over the workgroup (scalar loads from the argument segment, no private copy of the table): a chunk
// or an apply range is cut at the segment edges, and the lanes share each piece.
//
//   adam_sq_partial  one workgroup per chunk of L = 4,096 elements: 256 float64 chains, a fixed LDS tree, P_k
//   adam_tail        one workgroup: S = the P_k in order, then the step's scalars and state (wg_adam.h)
//   adam_apply       elementwise, 1,024 elements per workgroup: 16-byte loads and stores where the four pointers of a
//                    segment agree modulo 16, 4-byte ones at a piece's unaligned ends and otherwise; the same bits
//   adam_fused       the three phases in one workgroup of 1,024 threads (four chunks in flight), the same chunks in the
//                    same order, for E <= WG_ADAM_FUSED_MAX
// Only plain vector stores, no atomics, no inline assembly.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdlib>

#include "walker_hip.h"
#include "walker_internal.h"   // wg_fail, wg_launched
#include "wg_adam.h"           // wg_adam_scalars, wg_adam_element: the arithmetic, shared with host probes

namespace {

constexpr int AD_LANES = 256;          // the chains of a chunk
constexpr int AD_L = 4096;             // elements per chunk: the contract's L
constexpr int AD_APPLY = 1024;         // elements per workgroup of adam_apply
constexpr int AD_FUSED_THREADS = 1024; // adam_fused: four chunks at a time
constexpr int64_t AD_FUSED_MAX_DEFAULT = 24576;   // where the one launch and the three cross

struct AdTable {
    wg_opt_segment seg[WG_OPT_MAX_SEGMENTS];
    int64_t start[WG_OPT_MAX_SEGMENTS + 1];   // start[s] = the global number of segment s's first element; start[n] = E
    int32_t n;
};

struct AdCfg {
    float lr, beta1, beta2, eps, weight_decay, max_norm;
    int32_t maximize;
};

// Lane j's chain over the chunk [lo, hi): elements lo + j, lo + j + 256, ... ascending, across the segment edges.
__device__ __forceinline__ double ad_chain(const AdTable &t, int64_t lo, int64_t hi, int j) {
    double q = 0.0;
    for (int s = 0; s < t.n; s++) {   // (uniform)
        const int64_t a = t.start[s], b = t.start[s + 1];
        if (b <= lo) continue;
        if (a >= hi) break;
        const int64_t from = a > lo ? a : lo, to = b < hi ? b : hi;
        const int64_t off = from - lo;   // 0 .. L - 1
        const int64_t i0 = off <= j ? 0 : (off - j + AD_LANES - 1) / AD_LANES;
        const float *g = t.seg[s].grad;
        for (int64_t e = lo + j + i0 * AD_LANES; e < to; e += AD_LANES) {
            const double v = (double)g[e - a];
            q = fma(v, v, q);   // the product of two float32 values is exact in float64: one rounding
        }
    }
    return q;
}

// The fixed tree over 256 chains held in q[0..255].  Every thread of the workgroup calls it (the barriers are the
// workgroup's); P = q[0] once the last barrier has passed.
__device__ __forceinline__ void ad_tree(double *q, int j) {
    for (int s = AD_LANES / 2; s >= 1; s >>= 1) {
        __syncthreads();
        if (j < s) q[j] = __dadd_rn(q[j], q[j + s]);
    }
    __syncthreads();
}

__device__ __forceinline__ void ad_fixed(const AdCfg &c, wg_adam_consts *k) {
    wg_adam_fixed(c.lr, c.beta1, c.beta2, c.eps, c.weight_decay, c.maximize, k);
}

// The elements [lo, hi) by `threads` threads, this one `tid`.  A segment's piece is split into a head of at most three
// elements, whole 16-byte groups, and a tail of at most three when p, grad, m and v sit alike modulo 16.
__device__ __forceinline__ void ad_apply(const AdTable &t, const wg_adam_consts &k, int64_t lo, int64_t hi, int tid,
                                         int threads) {
    for (int s = 0; s < t.n; s++) {   // (uniform)
        const int64_t a = t.start[s], b = t.start[s + 1];
        if (b <= lo) continue;
        if (a >= hi) break;
        const int64_t from = (a > lo ? a : lo) - a, to = (b < hi ? b : hi) - a;   // within the segment
        float *p = t.seg[s].param, *m = t.seg[s].m, *v = t.seg[s].v;
        const float *g = t.seg[s].grad;
        const unsigned rp = (unsigned)(reinterpret_cast<uintptr_t>(p) >> 2) & 3u;
        const bool alike = rp == ((unsigned)(reinterpret_cast<uintptr_t>(g) >> 2) & 3u) &&
                           rp == ((unsigned)(reinterpret_cast<uintptr_t>(m) >> 2) & 3u) &&
                           rp == ((unsigned)(reinterpret_cast<uintptr_t>(v) >> 2) & 3u) &&
                           (reinterpret_cast<uintptr_t>(p) & 3u) == 0;
        int64_t v0 = to, v1 = to;   // [v0, v1): the 16-byte groups
        if (alike) {
            v0 = from + ((4 - ((from + rp) & 3)) & 3);
            v1 = v0 <= to ? v0 + ((to - v0) & ~(int64_t)3) : to;
            if (v0 > to) v0 = to;
        }
        for (int64_t i = v0 + 4 * (int64_t)tid; i < v1; i += 4 * (int64_t)threads) {
            float4 P = *reinterpret_cast<float4 *>(p + i), M = *reinterpret_cast<float4 *>(m + i);
            float4 V = *reinterpret_cast<float4 *>(v + i);
            const float4 G = *reinterpret_cast<const float4 *>(g + i);
            wg_adam_element(&k, G.x, &P.x, &M.x, &V.x);
            wg_adam_element(&k, G.y, &P.y, &M.y, &V.y);
            wg_adam_element(&k, G.z, &P.z, &M.z, &V.z);
            wg_adam_element(&k, G.w, &P.w, &M.w, &V.w);
            *reinterpret_cast<float4 *>(p + i) = P;
            *reinterpret_cast<float4 *>(m + i) = M;
            *reinterpret_cast<float4 *>(v + i) = V;
        }
        // the ends (everything, when the pointers disagree): [from, v0) and [v1, to)
        const int64_t n_head = v0 - from, n_ends = n_head + (to - v1);
        for (int64_t r = tid; r < n_ends; r += threads) {
            const int64_t i = r < n_head ? from + r : v1 + (r - n_head);
            float P = p[i], M = m[i], V = v[i];
            wg_adam_element(&k, g[i], &P, &M, &V);
            p[i] = P;
            m[i] = M;
            v[i] = V;
        }
    }
}

__global__ __launch_bounds__(AD_LANES) void adam_sq_partial(AdTable t, double *__restrict__ ws) {
    __shared__ double q[AD_LANES];
    const int j = threadIdx.x;
    const int64_t E = t.start[t.n], lo = (int64_t)blockIdx.x * AD_L, hi = E - lo < AD_L ? E : lo + AD_L;
    q[j] = ad_chain(t, lo, hi, j);
    ad_tree(q, j);
    if (j == 0) ws[blockIdx.x] = q[0];
}

// S over the chunk sums in order: the sums are fetched 256 at a time, thread 0 adds them one by one.
__device__ __forceinline__ double ad_chunk_sum(const double *ws, int64_t n_chunks, double *q, int tid) {
    double S = 0.0;
    for (int64_t base = 0; base < n_chunks; base += AD_LANES) {
        __syncthreads();
        if (tid < AD_LANES && base + tid < n_chunks) q[tid] = ws[base + tid];
        __syncthreads();
        if (tid == 0) {
            const int n = n_chunks - base < AD_LANES ? (int)(n_chunks - base) : AD_LANES;
            for (int i = 0; i < n; i++) S = __dadd_rn(S, q[i]);
        }
    }
    return S;   // (thread 0's)
}

__global__ __launch_bounds__(AD_LANES) void adam_tail(const double *__restrict__ ws, int64_t n_chunks, AdCfg c,
                                                      double *__restrict__ state) {
    __shared__ double q[AD_LANES];
    const double S = ad_chunk_sum(ws, n_chunks, q, threadIdx.x);
    if (threadIdx.x == 0) {
        wg_adam_consts k;
        wg_adam_scalars(S, state, c.lr, c.beta1, c.beta2, c.max_norm, &k);
    }
}

// What adam_tail left in state gives the step's scalars back: a finite norm (no skip), the advanced powers, cf.
__global__ __launch_bounds__(AD_LANES) void adam_apply(AdTable t, AdCfg c, const double *__restrict__ state) {
    const double norm = state[3];
    if (!(norm - norm == 0.0)) return;   // skipped: nothing is written (uniform)
    wg_adam_consts k;
    ad_fixed(c, &k);
    wg_adam_rates(state[1], state[2], c.lr, &k.a, &k.r2);
    k.cf = (float)state[4];
    k.skip = 0;
    const int64_t E = t.start[t.n], lo = (int64_t)blockIdx.x * AD_APPLY, hi = E - lo < AD_APPLY ? E : lo + AD_APPLY;
    ad_apply(t, k, lo, hi, threadIdx.x, AD_LANES);
}

__global__ __launch_bounds__(AD_FUSED_THREADS) void adam_fused(AdTable t, AdCfg c, double *ws, double *state) {
    constexpr int GROUPS = AD_FUSED_THREADS / AD_LANES;
    __shared__ double q[GROUPS][AD_LANES];
    __shared__ wg_adam_consts ks;
    const int tid = threadIdx.x, grp = tid / AD_LANES, j = tid % AD_LANES;
    const int64_t E = t.start[t.n], n_chunks = (E + AD_L - 1) / AD_L;
    for (int64_t k0 = 0; k0 < n_chunks; k0 += GROUPS) {   // (uniform: every thread meets every barrier)
        const int64_t kc = k0 + grp, lo = kc * AD_L, hi = E - lo < AD_L ? E : lo + AD_L;
        q[grp][j] = kc < n_chunks ? ad_chain(t, lo, hi, j) : 0.0;
        ad_tree(q[grp], j);
        if (j == 0 && kc < n_chunks) ws[kc] = q[grp][0];
        __syncthreads();
    }
    const double S = ad_chunk_sum(ws, n_chunks, q[0], tid);   // (its first barrier orders the stores to ws above)
    if (tid == 0) {
        wg_adam_consts k;
        ad_fixed(c, &k);
        wg_adam_scalars(S, state, c.lr, c.beta1, c.beta2, c.max_norm, &k);
        ks = k;
    }
    __syncthreads();
    const wg_adam_consts k = ks;
    if (k.skip) return;
    ad_apply(t, k, 0, E, tid, AD_FUSED_THREADS);
}

struct AdSpan {
    uintptr_t lo, hi;
    const char *name;
    int seg;
};
bool ad_overlap(const AdSpan &a, const AdSpan &b) { return a.lo < b.hi && b.lo < a.hi; }
AdSpan ad_span(const void *p, int64_t n, int elem, const char *name, int seg) {
    const uintptr_t lo = reinterpret_cast<uintptr_t>(p);
    return AdSpan{lo, lo + (uintptr_t)n * (uintptr_t)elem, name, seg};
}

// NULL table, count and segments: what the workspace query and the step check alike.  E may pass 2^31 here.
int ad_table(const wg_opt_segment *seg, int32_t n_segments, const char *who, bool pointers, AdTable *t) {
    if (!seg) return wg_fail(WG_EINVAL, "%s: null segment table", who);
    if (n_segments < 1 || n_segments > WG_OPT_MAX_SEGMENTS)
        return wg_fail(WG_EINVAL, "%s: n_segments %d outside 1..%d", who, n_segments, WG_OPT_MAX_SEGMENTS);
    t->n = n_segments;
    t->start[0] = 0;
    for (int s = 0; s < n_segments; s++) {
        if (pointers && (!seg[s].param || !seg[s].grad || !seg[s].m || !seg[s].v))
            return wg_fail(WG_EINVAL, "%s: segment %d has a null pointer", who, s);
        if (seg[s].n < 1) return wg_fail(WG_EINVAL, "%s: segment %d: n %lld < 1", who, s, (long long)seg[s].n);
        t->seg[s] = seg[s];
        const int64_t cap = (int64_t)1 << 32;   // (a count past 2^31 is refused later; the sum must not wrap before that)
        t->start[s + 1] = t->start[s] + (seg[s].n < cap ? seg[s].n : cap);
    }
    for (int s = n_segments; s < WG_OPT_MAX_SEGMENTS; s++) {
        t->seg[s] = wg_opt_segment{nullptr, nullptr, nullptr, nullptr, 0};
        t->start[s + 1] = t->start[n_segments];
    }
    return 0;
}

int64_t ad_fused_max() {   // WG_ADAM_FUSED_MAX, read on every call; 0 never fuses
    const char *e = std::getenv("WG_ADAM_FUSED_MAX");
    if (!e || !*e) return AD_FUSED_MAX_DEFAULT;
    char *end = nullptr;
    const long long v = std::strtoll(e, &end, 10);
    return end == e || v < 0 ? AD_FUSED_MAX_DEFAULT : (int64_t)v;
}

}   // namespace

extern "C" {

int64_t wg_adam_workspace(const wg_opt_segment *seg, int32_t n_segments) {
    AdTable t;
    if (const int rc = ad_table(seg, n_segments, "wg_adam_workspace", false, &t)) return rc;
    const int64_t E = t.start[t.n];
    if (E > INT32_MAX) return wg_fail(WG_ERANGE, "wg_adam_workspace: %lld elements pass 2^31", (long long)E);
    return (E + AD_L - 1) / AD_L;
}

int wg_adam_step(const wg_opt_segment *seg, int32_t n_segments, const wg_adam *cfg, double *workspace, double *state,
                 hipStream_t stream) {
    const char *who = "wg_adam_step";
    if (!seg) return wg_fail(WG_EINVAL, "%s: null segment table", who);
    if (!cfg) return wg_fail(WG_EINVAL, "%s: null cfg", who);
    if (!workspace) return wg_fail(WG_EINVAL, "%s: null workspace", who);
    if (!state) return wg_fail(WG_EINVAL, "%s: null state", who);
    AdTable t;
    if (const int rc = ad_table(seg, n_segments, who, true, &t)) return rc;
    if (!std::isfinite(cfg->lr)) return wg_fail(WG_EINVAL, "%s: lr must be finite", who);
    if (!(cfg->beta1 >= 0.f && cfg->beta1 < 1.f)) return wg_fail(WG_EINVAL, "%s: beta1 outside [0, 1)", who);
    if (!(cfg->beta2 >= 0.f && cfg->beta2 < 1.f)) return wg_fail(WG_EINVAL, "%s: beta2 outside [0, 1)", who);
    if (!(cfg->eps > 0.f) || !std::isfinite(cfg->eps)) return wg_fail(WG_EINVAL, "%s: eps must be finite and > 0", who);
    if (!(cfg->weight_decay >= 0.f) || !std::isfinite(cfg->weight_decay))
        return wg_fail(WG_EINVAL, "%s: weight_decay must be finite and >= 0", who);
    if (!(cfg->max_norm > 0.f)) return wg_fail(WG_EINVAL, "%s: max_norm must be > 0 (+inf allowed)", who);
    const int64_t E = t.start[t.n];
    if (E > INT32_MAX) return wg_fail(WG_ERANGE, "%s: %lld elements pass 2^31", who, (long long)E);
    const int64_t n_chunks = (E + AD_L - 1) / AD_L;
    // every output range against every other output, every grad, the workspace and the state
    static const char *const names[4] = {"param", "m", "v", "grad"};
    AdSpan out[3 * WG_OPT_MAX_SEGMENTS], in[WG_OPT_MAX_SEGMENTS + 2];
    int n_out = 0, n_in = 0;
    for (int s = 0; s < t.n; s++) {
        out[n_out++] = ad_span(seg[s].param, seg[s].n, 4, names[0], s);
        out[n_out++] = ad_span(seg[s].m, seg[s].n, 4, names[1], s);
        out[n_out++] = ad_span(seg[s].v, seg[s].n, 4, names[2], s);
        in[n_in++] = ad_span(seg[s].grad, seg[s].n, 4, names[3], s);
    }
    in[n_in++] = ad_span(workspace, n_chunks, 8, "workspace", -1);
    in[n_in++] = ad_span(state, 8, 8, "state", -1);
    for (int o = 0; o < n_out; o++) {
        for (int p = 0; p < o; p++)
            if (ad_overlap(out[o], out[p]))
                return wg_fail(WG_EINVAL, "%s: %s of segment %d overlaps %s of segment %d", who, out[o].name, out[o].seg,
                               out[p].name, out[p].seg);
        for (int i = 0; i < n_in; i++)
            if (ad_overlap(out[o], in[i]))
                return wg_fail(WG_EINVAL, "%s: %s of segment %d overlaps %s (segment %d)", who, out[o].name, out[o].seg,
                               in[i].name, in[i].seg);
    }
    if (ad_overlap(in[n_in - 2], in[n_in - 1])) return wg_fail(WG_EINVAL, "%s: workspace overlaps state", who);
    const AdCfg c{cfg->lr, cfg->beta1, cfg->beta2, cfg->eps, cfg->weight_decay, cfg->max_norm, cfg->maximize};
    if (E <= ad_fused_max()) {
        adam_fused<<<1, AD_FUSED_THREADS, 0, stream>>>(t, c, workspace, state);
        return wg_launched("wg_adam_step (fused): launch");
    }
    adam_sq_partial<<<(unsigned)n_chunks, AD_LANES, 0, stream>>>(t, workspace);
    if (const int rc = wg_launched("wg_adam_step (squares): launch")) return rc;
    adam_tail<<<1, AD_LANES, 0, stream>>>(workspace, n_chunks, c, state);
    if (const int rc = wg_launched("wg_adam_step (tail): launch")) return rc;
    adam_apply<<<(unsigned)((E + AD_APPLY - 1) / AD_APPLY), AD_LANES, 0, stream>>>(t, c, state);
    return wg_launched("wg_adam_step (apply): launch");
}

}   // extern "C"
