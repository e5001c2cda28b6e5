// wg_host.h — the host side of the C ABI: argument checks, launch geometry, instance selection, the launchers, run(),
// rollout_policy() and the planners' packer.
// Included by walker_hip.hip inside its anonymous namespace, after every kernel.
#pragma once

// ------------------------------------------------------------------ host side
// An integer knob of the environment (WG_LEAN, WG_XCD, ...): read on every call, so one process can A/B them.
int env_int(const char *name, int dflt) {
    const char *e = getenv(name);
    return (e && *e) ? atoi(e) : dflt;
}

KParams make_kparams(const wg_params &p) {
    KParams k;
    k.neg_g = (float)(-p.g);
    k.neg_dampk = (float)(-p.dampk);
    k.ground = (float)p.ground;
    k.neg_groundk = (float)(-p.groundk);
    k.neg_grounddamp = (float)(-p.grounddamp);
    k.friction = (float)p.friction;
    k.dt = (float)p.dt;
    k.pk = (float)p.pk; k.vk = (float)p.vk; k.ak = (float)p.ak; k.mk = (float)p.mk;
    k.done_y = (float)(p.ground - 50.0);
    k.g = p.g;
    k.max_steps = p.max_steps; k.midform = p.midform; k.conmid = p.conmid;
    k.spring_mode = p.spring_mode; k.action_mode = p.action_mode;
    k.integrator = p.integrator;
    k.pair_mode = p.pair_mode;
    k.pair_g = p.pair_g;
    k.pair_k = p.pair_k;
    k.pair_e = p.pair_e;
    k.bounce_kh = (float)(p.bounce_k / 2);
    for (int i = 0; i < 3; i++) k.g3g[i] = (float)p.g3_gravity[i];
    k.g3_damp = (float)p.g3_damping;
    k.g3_dragc = (float)(-0.5 * p.g3_air);
    k.g3_level = (float)p.g3_ground_level;
    k.g3_rest = (float)p.g3_restitution;
    k.g3_fric = (float)p.g3_friction;
    k.g3_ground = p.g3_ground;
    k.friction_mode = p.friction_mode;
    k.prio = env_int("WG_LEAN_PRIO", 1);
    k.xcd = env_int("WG_XCD", 3);   // both kernels (profiles/r03e_ab_canon.json, r03d_ab_ragged_window_xcd.json)
    k.keep_aux = 1;

    k.dt2 = (float)(p.dt * p.dt);
    return k;
}

constexpr int RAG_P = 256, RAG_E = 512, RAG_U = 256, RAG_W = 64;
constexpr int LDS_LIMIT = 160 * 1024;

// Spring passes of a ragged wave tile (wg_batch.ragged = 2) from the batch maxima: enough for the longest walker, and
// for 64 masses of the densest one (K / M springs per mass), rounded up to an instantiated NE (1, 2, 3, 4, 8); 0 = not
// eligible.
int wave_passes(int M, int K) {
    if (M < 1 || M > 64 || K < 0) return 0;
    int ne = std::max((K + 63) / 64, (K + M - 1) / M);
    ne = std::max(ne, 1);
    if (ne > 8) return 0;
    return ne <= 4 ? ne : 8;
}

int validate(const wg_batch *b) {
    if (!b) return wg_fail(WG_EINVAL, "null batch");
    if (b->N < 0 || b->M < 1 || b->K < 0 || b->A < 0 || b->A > b->K)
        return wg_fail(WG_EINVAL, "bad sizes N=%d M=%d K=%d A=%d", b->N, b->M, b->K, b->A);
    if (2 * b->K > 65535) return wg_fail(WG_ERANGE, "K=%d exceeds the u16 incidence encoding", b->K);
    if (b->M > WG_MAX_M) return wg_fail(WG_ERANGE, "M=%d > %d masses per walker", b->M, WG_MAX_M);
    if (!b->pos || !b->vel || !b->acc || !b->mass || !b->steps || !b->muscle_x)
        return wg_fail(WG_EINVAL, "missing state pointer");
    if (b->K > 0 && (!b->edges || !b->inc || !b->inc_off)) return wg_fail(WG_EINVAL, "missing edge pointer");
    if (b->M > 32767) return wg_fail(WG_ERANGE, "M=%d exceeds the 15-bit edge endpoint encoding", b->M);
    if (!b->inc_off) return wg_fail(WG_EINVAL, "missing inc_off");
    if (b->ragged < 0 || b->ragged > 2) return wg_fail(WG_EINVAL, "ragged must be 0, 1 or 2");
    if (b->ragged && (!b->mass_off || !b->edge_off || !b->muscle_off))
        return wg_fail(WG_EINVAL, "ragged batch without offsets");
    if (!b->ragged && b->row) return wg_fail(WG_EINVAL, "row (a walker permutation) is for ragged batches only");
    if (b->ragged == 2 && !wave_passes(b->M, b->K))
        return wg_fail(WG_EINVAL, "ragged = 2 (wave tiles) needs M <= 64 and at most 8 spring passes (M=%d K=%d)", b->M, b->K);
    return 0;
}

Geo uniform_geo(const wg_batch *b, int obs_stride, bool no_lite = false) {
    Geo g{};
    // walkers per workgroup: fill the 256 mass lanes, keep edges within EPL registers per lane,
    // and make sure the grid has >= 512 workgroups when the batch allows it.
    int W = std::max(1, NTHREADS / b->M);
    if (b->M > 64 && env_int("WG_WIDE", 1)) {
        // M > 64: the workgroup size (256..512 threads) that leaves the fewest idle lanes; 100-mass chains run
        // 5 walkers on 512 threads (98 % of the lanes busy) instead of 2 on 256 (78 %)
        int best = 0, bestT = NTHREADS;
        for (int T = NTHREADS; T <= MAXT; T += 64) {
            const int w = T / b->M;
            if (w >= 1 && (int64_t)w * b->M * bestT > (int64_t)best * T) { best = w * b->M; bestT = T; W = w; }
        }
    }
    if (b->K > 0) W = std::max(1, std::min(W, EPL * MAXT / std::max(1, b->K)));
    while (W > 1 && (b->N + W - 1) / W < 512) W = std::max(1, W / 2);
    g.W = W;
    const bool shfl_shape = b->M <= 64 && (64 % b->M) == 0 && !(WG_ABLATE & 64);
    for (;;) {
        g.Pcap = g.W * b->M; g.Ecap = g.W * b->K; g.Ucap = g.W * b->A;
        g.tbytes = std::max(g.Ecap * 3 * 8, g.W * std::max(0, obs_stride) * 4);
        g.lite = (shfl_shape && g.W * b->M <= MAXT && !no_lite) ? 1 : 0;   // pair passes need the LDS copies
        g.threads = std::min(MAXT, std::max(64, ((g.W * b->M + 63) / 64) * 64));
        if (b->K > 0 && g.W * b->K > EPL * g.threads) g.threads = MAXT;
        g.lds = carve_bytes(g);
        if (g.lds <= 64 * 1024 || g.W == 1) break;
        g.W = std::max(1, g.W / 2);
    }
    g.invM = 1.f / (float)b->M;
    g.invK = 1.f / (float)std::max(1, b->K);
    g.invA = 1.f / (float)std::max(1, b->A);
    return g;
}

Geo ragged_geo(const wg_batch *b) {
    Geo g{};
    g.threads = NTHREADS;
    g.W = RAG_W;
    g.Pcap = std::max(RAG_P, b->M);
    g.Ecap = std::max(RAG_E, b->K);
    g.Ucap = std::max(RAG_U, b->A);
    g.tbytes = g.Ecap * 3 * 8;
    g.lite = 0;
    g.lds = carve_bytes(g);
    g.invM = g.invK = g.invA = 0.f;
    return g;
}

template <bool STEP, bool RAGGED, bool IN3D, int PWD, bool SHFL>
int launch(const wg_batch *b, const KParams &kp, const float *action, int cols, int astride,
           const wg_outputs &o, const int32_t *plan, int blocks, const Geo &g, hipStream_t stream) {
    // (+ the static 512 B of the powf tables in LDS)
    const int lds_static = (int)(sizeof(s_pw_log2) + sizeof(s_pw_exp2));
    if (g.lds + lds_static > LDS_LIMIT)
        return wg_fail(WG_ERANGE, "workgroup needs %d B of LDS (> 160 KiB)", g.lds + lds_static);
    WG_KLAUNCH((walker_step_kernel<STEP, RAGGED, IN3D, PWD, SHFL>), dim3(blocks), dim3(g.threads), (uint32_t)g.lds, stream,
               *b, kp, action, cols, astride, kout(o), plan, g);
    return wg_launched("launch");
}

// register (shuffle) reductions: every walker's masses are adjacent lanes of one wave
bool shfl_ok(const wg_batch *b, const Geo &g) { return !b->ragged && g.lite; }

template <bool STEP, int PWD>
int dispatch2(const wg_batch *b, const KParams &kp, bool in3d, const float *a, int cols, int astride,
              const wg_outputs &o, const int32_t *plan, int blocks, const Geo &g, hipStream_t st) {
    if (b->ragged) {
        return in3d ? launch<STEP, true, true, PWD, false>(b, kp, a, cols, astride, o, plan, blocks, g, st)
                    : launch<STEP, true, false, PWD, false>(b, kp, a, cols, astride, o, plan, blocks, g, st);
    }
    if (PWD == 0 && shfl_ok(b, g)) {
        return in3d ? launch<STEP, false, true, 0, true>(b, kp, a, cols, astride, o, plan, blocks, g, st)
                    : launch<STEP, false, false, 0, true>(b, kp, a, cols, astride, o, plan, blocks, g, st);
    }
    return in3d ? launch<STEP, false, true, PWD, false>(b, kp, a, cols, astride, o, plan, blocks, g, st)
                : launch<STEP, false, false, PWD, false>(b, kp, a, cols, astride, o, plan, blocks, g, st);
}
// ---- lean kernel selection: uniform batch, M | 64 with M >= 4, the wave's edges in <= 8 register
// passes, its muscles in one pass, and a workgroup LDS footprint that keeps >= 2 workgroups per CU.
// Knobs (env_int): WG_LEAN=0 selects the barrier kernels; WG_LEAN_WAVES 1/2/4 waves per workgroup; WG_LEAN_PRIO 0/1
// load-phase priority.
bool lean_enabled() { return env_int("WG_LEAN", 1) != 0; }

// The compact spring records (wg_batch.edges8, ABI 15) are addressed by tile-relative lane roles: a lean launch reads
// them only with the standard tile of 64 / M walkers per wave (small batches whose tiles lean_geo halves, and WG_LEAN_WPW,
// keep the 16-B records).  WG_EDGE8=0 (read on every launch, like WG_LEAN) forces the 16-B records.
bool use_edge8(const wg_batch *b, const LeanGeo &g) {
    return b->edges8 != nullptr && g.wpw * b->M == 64 && env_int("WG_EDGE8", 1) != 0;
}

// The barrier-free kernels address their loads as SGPR base + 32-bit byte offset (at_u32): every array of the batch
// must then span less than 4 GiB (positions 12 B and spring records 16 B per element dominate; M, K are maxima).
bool u32_bytes(const wg_batch *b) {
    const int64_t lim = 1ll << 32;
    return (int64_t)b->N * b->M * 12 < lim && (int64_t)b->N * b->K * 16 < lim && (int64_t)b->N * b->A * 8 < lim &&
           (int64_t)b->N * (b->M + 1) * 2 < lim;
}
// and their observation rows as 32-bit byte offsets (WG_ST)
bool obs_u32(const wg_batch *b, int obs_stride) { return (int64_t)b->N * std::max(obs_stride, 1) * 4 < (1ll << 32); }

// spring passes of a lean wave tile: ceil(wpw * K / 64), at most 8 (lean_geo)
int lean_passes(const LeanGeo &g, const wg_batch *b) { return (g.wpw * b->K + 63) / 64; }

bool lean_geo(const wg_batch *b, int obs_stride, LeanGeo *out, int spring_mode = 0) {
    const int M = b->M;
    if (b->ragged || M < 4 || M > 64 || (64 % M) != 0 || b->K < 1 || !lean_enabled() || (WG_ABLATE & 128)) return false;
    if (spring_mode != 0) return false;          // the G2-compat element runs on the workgroup kernel
    // 32-bit element offsets inside the kernel, 32-bit byte offsets for its loads (at_u32)
    if ((int64_t)b->N * b->M * 3 >= (1ll << 31) || (int64_t)b->N * b->K * 4 >= (1ll << 31) ||
        !obs_u32(b, obs_stride) || !u32_bytes(b))
        return false;
    LeanGeo g{};
    g.wpw = 64 / M;
    // small batches: fewer walkers per wave until there are 512 wave tiles (two per CU), so a latency-bound step
    // spreads over more waves (4,096 Balance-v0 walkers: 16 -> 8 walkers per wave, 6.40 -> 5.97 us per step,
    // profiles/r02_ab_balance4096_wpw.json); WG_LEAN_WPW (experiment) caps the count
    while (g.wpw > 1 && (b->N + g.wpw - 1) / g.wpw < 512) g.wpw >>= 1;
    const int wcap = env_int("WG_LEAN_WPW", 0);
    if (wcap > 0 && wcap < g.wpw) g.wpw = wcap;
    g.lgM = 0;
    while ((1 << g.lgM) < M) g.lgM++;
    if (lean_passes(g, b) > 8 || g.wpw * b->A > 64) return false;
    // waves per workgroup: 4 (one workgroup per four tiles) unless the batch has no more tiles than the chip has SIMDs,
    // where one wave per workgroup spreads the latency-bound step over twice the CUs (4,096 Balance-v0 walkers: 5.45
    // against 5.60 us, 65,536 canonical: 44.31 against 44.01; profiles/r04m_ab_*_wpb.json); WG_LEAN_WAVES overrides
    const int wpb = env_int("WG_LEAN_WAVES", 0);
    g.wpb = (wpb == 1 || wpb == 2 || wpb == 4) ? wpb : ((b->N + g.wpw - 1) / g.wpw <= 1024 ? 1 : 4);
    const int ew = g.wpw * b->K;                          // springs of a full wave tile
    g.pl = (ew + 3) & ~3;                                 // spring-term slots: 16-B aligned regions
    // t (f64 x3) | df (f32 x3) | incidence words | x (observation rows go from registers to HBM, no LDS tile)
    g.off_df = align16(g.pl * 24);
    g.off_inc = g.off_df + align16(g.pl * 12);
    g.off_x = g.off_inc + align16(ew * 4 + 4);              // + the zero word after the last list (mass_accumulate_v2)
    g.slice = g.off_x + align16(std::max(1, g.wpw * b->A) * 4);
    if (4 * g.slice > 80 * 1024) return false;
    g.invK = 1.f / (float)b->K;
    g.invA = 1.f / (float)std::max(1, b->A);
    g.invM = 1.f / (float)M;
    g.nblk = (b->N + g.wpb * g.wpw - 1) / (g.wpb * g.wpw);   // the grid of a lean launch: one tile per wave
    *out = g;
    return true;
}

// walker_step_lean1's preloaded word: bits 0..29 the workgroup count, bit 30 the XCD-order flag (WG_XCD bit 1), bit 31
// the load-phase priority flag (WG_LEAN_PRIO)
int lean1_nblkx(const LeanGeo &g, const KParams &kp) {
    return (int)((unsigned)g.nblk | ((unsigned)(kp.xcd & 2) << 29) | ((unsigned)(kp.prio != 0) << 31));
}

// ---- instance selection: the runtime (in3d, passes, compact records) of a launch as compile-time tags, in one place.
// A launch site is one call whose generic lambda names its kernel with the tags' values; `if constexpr` in the lambda
// keeps the instances nobody launches (NE 1 of walker_step_lean, FIX outside E8 and NE 1-4) uninstantiated.
template <class F>
void with_flag(bool v, F &&f) {
    if (v) f(std::true_type{});
    else f(std::false_type{});
}
// the pass count rounded up to an instantiated NE: 1, 2, 3, 4, 8
template <class F>
void with_passes(int ne, F &&f) {
    if (ne <= 1) f(std::integral_constant<int, 1>{});
    else if (ne == 2) f(std::integral_constant<int, 2>{});
    else if (ne == 3) f(std::integral_constant<int, 3>{});
    else if (ne == 4) f(std::integral_constant<int, 4>{});
    else f(std::integral_constant<int, 8>{});
}
template <class F>
void with_instance(bool in3d, int ne, F &&f) {   // f(IN3D, NE)
    with_flag(in3d, [&](auto d3) { with_passes(ne, [&](auto n) { f(d3, n); }); });
}
template <class F>
void with_instance(bool in3d, int ne, bool e8, F &&f) {   // f(IN3D, NE, E8)
    with_instance(in3d, ne, [&](auto d3, auto n) { with_flag(e8, [&](auto c8) { f(d3, n, c8); }); });
}

// The caller's actions: cols values in row w of step s at ptr[s * step + w * stride]; ptr NULL = none
struct Actions {
    const float *ptr;
    int32_t cols, stride;
    int64_t step;
    Actions at(int s) const { return Actions{ptr ? ptr + s * step : nullptr, cols, stride, step}; }
};

// The fixed-parameter instance (FIX) runs a launch whose every tile is full and whose batch, parameters, actions and
// outputs are the default path's: compact records in 1..4 passes, no auto-reset, continuous actions for every muscle,
// no pair passes, pins or radii, run1, midform 1 without conmid, unit observation scales (by bit pattern), every
// per-step output but the optional steps asked for.  Anything else takes the generic instance, as a whole launch (a
// partial last tile too).  WG_FIX=0 (read on every launch, like WG_EDGE8) forces the generic instance: the control arm
// and the tests' cross-check.
bool lean_fix_ok(const wg_batch *b, const KParams &kp, const Actions &a, const wg_outputs &o, const LeanGeo &g, bool e8,
                 int ne, int ar_mode) {
#ifdef WG_STAMPS
    return false;
#endif
    if (WG_ABLATE != 0 || env_int("WG_FIX", 1) == 0) return false;
    auto one = [](float f) {
        uint32_t u;
        memcpy(&u, &f, sizeof u);
        return u == 0x3f800000u;
    };
    return e8 && ne >= 1 && ne <= 4 && ar_mode == 0 && b->N % g.wpw == 0 && g.wpw * b->M == 64 &&
           b->A >= 1 && a.ptr != nullptr && a.cols >= b->A && a.stride >= b->A && kp.action_mode == 0 &&
           kp.pair_mode == 0 && !b->pinned && !b->radius && kp.integrator != 2 && kp.midform == 1 && kp.conmid == 0 &&
           one(kp.pk) && one(kp.vk) && one(kp.ak) && one(kp.mk) &&
           o.obs && o.reward && o.done && o.centroid && o.energy;
}
// launches that took the fixed-parameter instance, this process (wg_fix_launches: the tests read which instance ran)
std::atomic<long long> g_fix_launches{0};

// The FIX instances' tile epilogue through LDS (lean_tile_image: pos, vel and the observation rows as the tile's HBM
// image, stored 16 B per lane, write-through).  A FIX launch takes it, as a whole launch, when the observation rows are
// contiguous (no padding; FIX has no conmid column), pos / vel / obs start on 16-B boundaries, a tile's row block is a
// multiple of 16 B (pos and vel are 768 B each: wpw * M == 64) and the image fits the spring terms' area of the wave's
// slice.  A one-pass tile (walker_step_lean1) never qualifies: its terms' area is at most 64 x 36 = 2,304 B, and pos and
// vel alone are 1,536 B of the image.  WG_WT=0 (read on every launch, like WG_FIX) forces today's epilogue: the control
// arm and the tests' cross-check.
bool lean_wt_ok(const wg_batch *b, bool in3d, const wg_outputs &o, const LeanGeo &g, bool fix) {
    if (!fix || env_int("WG_WT", 1) == 0 || lean_passes(g, b) < 2) return false;
    const int row = 3 * (in3d ? 3 : 2) * b->M + b->A;
    const int64_t rows_b = (int64_t)g.wpw * row * 4;
    auto al16 = [](const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; };
    static_assert(64 * 12 % 16 == 0, "a tile's pos / vel block");
    return o.obs_stride == row && al16(b->pos) && al16(b->vel) && al16(o.obs) && rows_b % 16 == 0 &&
           2 * 768 + rows_b <= g.off_inc;
}
// launches that took that epilogue, this process (wg_wt_launches)
std::atomic<long long> g_wt_launches{0};

// One step of a uniform batch on the lean kernels.  ar_mode (wg_params.auto_reset) != 0: the AR instances (the auto-reset
// tail, ABI 16); a launch that lean_fix_ok admits: the FIX instances.  One spring pass is walker_step_lean1's, with its
// leading arguments preloaded (the compact records take the spring records' slot).
int launch_lean(const wg_batch *b, const KParams &kp, bool in3d, const Actions &a, const wg_outputs &o, const LeanGeo &g,
                hipStream_t st, int ar_mode = 0) {
    const int ne = lean_passes(g, b);
    // WG_LDS_PAD (diagnostic): extra LDS bytes per workgroup, to measure the kernel at lower occupancy
    const uint32_t lds = (uint32_t)(g.wpb * g.slice + std::max(0, env_int("WG_LDS_PAD", 0)));
    const bool e8 = use_edge8(b, g);
    const bool fix = lean_fix_ok(b, kp, a, o, g, e8, ne, ar_mode);   // (E8, 1..4 passes, no auto-reset)
    const bool wt = lean_wt_ok(b, in3d, o, g, fix);
    const dim3 grid(g.nblk), block(64 * g.wpb);
    with_instance(in3d, ne, e8, [&](auto d3, auto n, auto c8) {
        constexpr bool D3 = decltype(d3)::value, E8 = decltype(c8)::value;
        constexpr int NE = decltype(n)::value;
        if constexpr (NE == 1) {
            const void *recs = E8 ? static_cast<const void *>(b->edges8) : static_cast<const void *>(b->edges);
            auto go = [&](auto kernel, auto reset) {
                WG_KLAUNCH(kernel, grid, block, lds, st, b->pos, b->vel, recs, b->inc, b->N, b->M, b->K, g.wpw, g.wpb,
                           lean1_nblkx(g, kp), *b, kp, a.ptr, a.cols, a.stride, kout(o), g, reset);
            };
            if constexpr (E8) {
                if (fix) return go(walker_step_lean1<D3, true, false, true>, KNoReset{});
            }
            if (ar_mode) go(walker_step_lean1<D3, E8, true>, kreset(o, ar_mode));
            else go(walker_step_lean1<D3, E8>, KNoReset{});
        } else {
            auto go = [&](auto kernel, const auto &batch, auto reset) {
                WG_KLAUNCH(kernel, grid, block, lds, st, batch, kp, a.ptr, a.cols, a.stride, kout(o), g, reset);
            };
            if constexpr (E8 && NE <= 4) {
                if (wt) return go(walker_step_lean<D3, NE, true, false, true, true>, kbatch15(b), KNoReset{});
                if (fix) return go(walker_step_lean<D3, NE, true, false, true>, kbatch15(b), KNoReset{});
            }
            if (ar_mode) go(walker_step_lean<D3, NE, E8, true>, *b, kreset(o, ar_mode));
            else go(walker_step_lean<D3, NE, E8>, kbatch15(b), KNoReset{});
        }
    });
    if (const int rc = wg_launched("launch")) return rc;
    if (fix) g_fix_launches.fetch_add(1, std::memory_order_relaxed);
    if (wt) g_wt_launches.fetch_add(1, std::memory_order_relaxed);
    return 0;
}

// n_steps steps of a uniform batch in one launch, the state in registers between them.  ar_mode != 0: the AR twin, one
// LDS word per walker (its episode count) behind each wave's slice.  (A plain launch: wg_time_step never comes here.)
int launch_lean_rollout(const wg_batch *b, const KParams &kp, bool in3d, const Actions &a, const wg_outputs &o,
                        int n_steps, const LeanGeo &g0, hipStream_t st, int ar_mode = 0) {
    LeanGeo g = g0;
    const KResetRes ar{kreset(o, ar_mode), g.slice};
    if (ar_mode) g.slice += align16(g.wpw * 4);
    const dim3 grid(g.nblk), block(64 * g.wpb);
    const int lds = g.wpb * g.slice;
    with_instance(in3d, lean_passes(g, b), use_edge8(b, g), [&](auto d3, auto n, auto c8) {
        constexpr bool D3 = decltype(d3)::value, E8 = decltype(c8)::value;
        constexpr int NE = decltype(n)::value;
        if (ar_mode)
            hipLaunchKernelGGL((walker_rollout_lean<D3, NE, E8, true>), grid, block, lds, st, *b, kp, a.ptr, a.cols,
                               a.stride, a.step, kout(o), n_steps, g, ar);
        else
            hipLaunchKernelGGL((walker_rollout_lean<D3, NE, E8>), grid, block, lds, st, *b, kp, a.ptr, a.cols, a.stride,
                               a.step, kout(o), n_steps, g, KNoReset{});
    });
    return wg_launched("launch");
}

// ---- argument checks that run() and rollout_policy() share: 0, or the refusal.  Each entry calls them in the order its
// callers have always seen (the first of several refusals is part of the contract: tests/test_refusal_order_cpu.py).
// auto-reset (ABI 16): everything the reset tail reads
int check_auto_reset(const wg_batch *b, int ar_mode) {
    if (ar_mode & ~3) return wg_fail(WG_EINVAL, "auto_reset %d: bits 1 (done) and 2 (non-finite) only", ar_mode);
    if (!b->init_pos || !b->init_vel || !b->init_acc || !b->init_muscle_x)
        return wg_fail(WG_EINVAL, "auto_reset needs the snapshot (init_pos, init_vel, init_acc, init_muscle_x)");
    if (!b->episodes) return wg_fail(WG_EINVAL, "auto_reset needs the episodes array");
    if (b->reset_noise && b->reset_noise_rows < 1)
        return wg_fail(WG_EINVAL, "auto_reset: reset_noise with reset_noise_rows %d < 1", b->reset_noise_rows);
    if (b->reset_noise && b->reset_noise_stride < 3ll * b->N * b->M)
        return wg_fail(WG_EINVAL, "auto_reset: reset_noise_stride %lld < 3 * P = %lld",
                       (long long)b->reset_noise_stride, 3ll * b->N * b->M);
    return 0;
}
int check_integrator(const wg_params *p) {
    return p->integrator < 0 || p->integrator > 2 ? wg_fail(WG_EINVAL, "integrator must be 0/1 (run1) or 2 (run2)") : 0;
}
int check_muscle_bounds(const wg_batch *b) {
    return b->muscle_bounds ? 0 : wg_fail(WG_EINVAL, "actions need muscle_bounds");
}
int check_discrete(const wg_batch *b, const wg_params *p) {
    return p->action_mode == 1 && !b->muscle_stride ? wg_fail(WG_EINVAL, "discrete actions need muscle_stride") : 0;
}

// a batch's observation row length under p: Creature.getstat's list (gym/optimized_walker.py:129-162)
int obs_row_len(const wg_batch *b, const wg_params *p) {
    return 3 * (p->in3d ? 3 : 2) * b->M + (p->conmid ? 3 : 0) + b->A;
}

// [p, p + bytes) of a caller's buffer: wg_rollout_held's test of `held` against the call's other outputs
struct HostSpan {
    const char *name;
    const void *p;
    int64_t bytes;
};
bool host_overlap(const HostSpan &a, const HostSpan &c) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a.p), c0 = reinterpret_cast<uintptr_t>(c.p);
    return a.p && c.p && a.bytes > 0 && c.bytes > 0 && a0 < c0 + (uintptr_t)c.bytes && c0 < a0 + (uintptr_t)a.bytes;
}

// wg_rollout_policy: every argument checked, then one walker_rollout_policy launch.  The wave's LDS slice is the lean
// kernel's plus the walkers' observation rows, hidden vectors and actions.
// episodes (wg_rollout_episodes): the AR instances, with auto-reset's own checks in place of the auto_reset refusal, the
// accounting of `st`, and eight words per walker in the slice instead of four.
// stochastic (wg_rollout_stochastic): either mode, chosen by p->auto_reset, with the NZ instances and the checks of `nz`.
// normalized (wg_rollout_normalized): either mode likewise, with or without the noise, the ON instances and the checks of
// `nm`.
// held (wg_rollout_held): the mode and the form by p->auto_reset, nz and nm as above, the HOLD instances (which carry the
// noise and the normaliser as runtime options), the checks of `hold`, and one more word per walker in the slice.
// deep (wg_rollout_deep): held with the middle layer of `mid`: the DEEP instances, the checks of `mid`, hidden2 more words
// per walker in the slice (the second hidden vector), and the middle matrix among a shared policy's staged weights.
int rollout_policy(const wg_batch *b, const wg_params *p, const wg_policy *pol, const wg_outputs *o, int32_t n_steps,
                   hipStream_t stream, bool episodes = false, const wg_episode_stats *st = nullptr,
                   bool stochastic = false, const wg_action_noise *nz = nullptr, bool normalized = false,
                   const wg_obs_norm *nm = nullptr, bool held = false, const wg_action_hold *hold = nullptr,
                   bool deep = false, const wg_policy_mid *mid = nullptr) {
    const char *fn = deep ? "wg_rollout_deep" : held ? "wg_rollout_held" : normalized ? "wg_rollout_normalized"
                     : stochastic ? "wg_rollout_stochastic" : episodes ? "wg_rollout_episodes" : "wg_rollout_policy";
    int rc = validate(b);
    if (rc) return rc;
    if (!p) return wg_fail(WG_EINVAL, "null params");
    if ((stochastic || normalized || held) && !episodes && st)
        return wg_fail(WG_EINVAL, "%s: episode stats with auto_reset 0 (st must be NULL without episode roll-over)", fn);
    if (!pol) return wg_fail(WG_EINVAL, "%s: null policy", fn);
    if (!pol->w2) return wg_fail(WG_EINVAL, "%s: null w2", fn);
    if (n_steps < 1) return wg_fail(WG_EINVAL, "%s: n_steps %d < 1", fn, n_steps);
    if (pol->hidden < 0 || pol->hidden > 256)
        return wg_fail(WG_EINVAL, "%s: hidden %d outside 0..256", fn, pol->hidden);
    if (pol->hidden > 0 && !pol->w1) return wg_fail(WG_EINVAL, "%s: hidden %d with a null w1", fn, pol->hidden);
    if (deep) {
        if (!mid) return wg_fail(WG_EINVAL, "%s: null middle layer", fn);
        if (mid->hidden2 < 1 || mid->hidden2 > 256)
            return wg_fail(WG_EINVAL, "%s: hidden2 %d outside 1..256", fn, mid->hidden2);
        if (!mid->wm) return wg_fail(WG_EINVAL, "%s: null wm", fn);
        if (pol->hidden == 0) return wg_fail(WG_EINVAL, "%s: a middle layer needs hidden > 0", fn);
    }
    if (pol->act_dim < 1 || pol->act_dim > b->A)
        return wg_fail(WG_EINVAL, "%s: act_dim %d outside 1..A = %d", fn, pol->act_dim, b->A);
    if (pol->obs_dim != obs_row_len(b, p))
        return wg_fail(WG_EINVAL, "%s: obs_dim %d, the batch's rows have %d values", fn, pol->obs_dim,
                    obs_row_len(b, p));
    if (pol->n_sets < 1 || b->N % pol->n_sets != 0)
        return wg_fail(WG_EINVAL, "%s: n_sets %d does not divide N = %d", fn, pol->n_sets, b->N);
    if (!(pol->act_limit > 0.f)) return wg_fail(WG_EINVAL, "%s: act_limit must be > 0 (+inf allowed)", fn);
    if (!episodes && p->auto_reset != 0)
        return wg_fail(WG_EINVAL, "%s: auto_reset %d (the resident loop has no reset tail)", fn, p->auto_reset);
    if (episodes) {
        if (p->auto_reset == 0)
            return wg_fail(WG_EINVAL, "%s: auto_reset is 0 (without episode roll-over use wg_rollout_policy)", fn);
        if ((rc = check_auto_reset(b, p->auto_reset))) return rc;   // (auto-reset's own checks, as wg_step makes them)
        if (!st) return wg_fail(WG_EINVAL, "%s: null episode stats", fn);
        if (st->ep_slots < 0) return wg_fail(WG_EINVAL, "%s: ep_slots %d < 0", fn, st->ep_slots);
        if ((st->ep_return || st->ep_length) && st->ep_slots == 0)
            return wg_fail(WG_EINVAL, "%s: ep_return / ep_length with ep_slots 0", fn);
        if (pol->return_out || pol->length_out)
            return wg_fail(WG_EINVAL, "%s: return_out / length_out are defined by the first done (wg_rollout_policy); "
                                   "the episode stats replace them", fn);
    }
    if (stochastic) {
        if (!nz) return wg_fail(WG_EINVAL, "%s: null action noise", fn);
        if (!nz->sigma) return wg_fail(WG_EINVAL, "%s: null sigma", fn);
        const int64_t row = (int64_t)b->N * pol->act_dim;
        if (nz->raw_out && nz->raw_out_step < row)
            return wg_fail(WG_EINVAL, "%s: raw_out_step %lld < N * act_dim = %lld", fn, (long long)nz->raw_out_step,
                           (long long)row);
        if (nz->eps_out && nz->eps_out_step < row)
            return wg_fail(WG_EINVAL, "%s: eps_out_step %lld < N * act_dim = %lld", fn, (long long)nz->eps_out_step,
                           (long long)row);
        // the counters are 32-bit words: no step or walker of the call may wrap
        if ((uint64_t)nz->step_base + (uint64_t)n_steps > (1ull << 32))
            return wg_fail(WG_EINVAL, "%s: step_base %u + n_steps %d passes 2^32", fn, nz->step_base, n_steps);
        if ((uint64_t)nz->walker_base + (uint64_t)b->N > (1ull << 32))
            return wg_fail(WG_EINVAL, "%s: walker_base %u + N %d passes 2^32", fn, nz->walker_base, b->N);
    }
    if (normalized) {
        if (!nm) return wg_fail(WG_EINVAL, "%s: null obs norm", fn);
        if (!nm->mean) return wg_fail(WG_EINVAL, "%s: null mean", fn);
        if (!nm->scale) return wg_fail(WG_EINVAL, "%s: null scale", fn);
        if (!(nm->clip > 0.f)) return wg_fail(WG_EINVAL, "%s: clip must be > 0 (+inf allowed)", fn);
    }
    if (held) {
        if (!hold) return wg_fail(WG_EINVAL, "%s: null action hold", fn);
        if (hold->every < 1) return wg_fail(WG_EINVAL, "%s: every %d < 1", fn, hold->every);
        if (hold->decided_out && hold->decided_out_step < b->N)
            return wg_fail(WG_EINVAL, "%s: decided_out_step %lld < N = %d", fn, (long long)hold->decided_out_step, b->N);
        if (hold->hold_reward_out && hold->hold_reward_out_step < b->N)
            return wg_fail(WG_EINVAL, "%s: hold_reward_out_step %lld < N = %d", fn,
                           (long long)hold->hold_reward_out_step, b->N);
        if (hold->held) {   // in and out: no other output of the call may lie in it
            const int64_t N = b->N, C = pol->act_dim, T = n_steps, slots = st ? st->ep_slots : 0;
            const auto steps = [&](int64_t step, int64_t row, int elem) { return ((T - 1) * step + row) * elem; };
            const wg_outputs oo = o ? *o : wg_outputs{};
            const int64_t orow = (N - 1) * (int64_t)oo.obs_stride + pol->obs_dim;
            const HostSpan hs{"held", hold->held, N * (C + 1) * 4};
            const HostSpan outs[] = {
                {"action_out", pol->action_out, steps(pol->action_out_step, N * C, 4)},
                {"return_out", pol->return_out, N * 4}, {"length_out", pol->length_out, N * 4},
                {"raw_out", nz ? nz->raw_out : nullptr, nz ? steps(nz->raw_out_step, N * C, 4) : 0},
                {"eps_out", nz ? nz->eps_out : nullptr, nz ? steps(nz->eps_out_step, N * C, 4) : 0},
                {"decided_out", hold->decided_out, steps(hold->decided_out_step, N, 1)},
                {"hold_reward_out", hold->hold_reward_out, steps(hold->hold_reward_out_step, N, 4)},
                {"obs", oo.obs, steps(oo.obs_step, orow, 4)}, {"final_obs", oo.final_obs, steps(oo.obs_step, orow, 4)},
                {"reward", oo.reward, steps(oo.out_step, N, 4)}, {"done", oo.done, steps(oo.out_step, N, 1)},
                {"centroid", oo.centroid, steps(3 * oo.out_step, 3 * N, 4)},
                {"energy", oo.energy, steps(oo.out_step, N, 4)}, {"steps", oo.steps, steps(oo.out_step, N, 4)},
                {"reset", oo.reset, steps(oo.out_step, N, 1)},
                {"return_sum", st ? st->return_sum : nullptr, N * 4}, {"length_sum", st ? st->length_sum : nullptr, N * 4},
                {"episodes_done", st ? st->episodes_done : nullptr, N * 4},
                {"tail_return", st ? st->tail_return : nullptr, N * 4},
                {"tail_length", st ? st->tail_length : nullptr, N * 4},
                {"ep_return", st ? st->ep_return : nullptr, N * slots * 4},
                {"ep_length", st ? st->ep_length : nullptr, N * slots * 4}};
            for (const HostSpan &x : outs)
                if (host_overlap(hs, x)) return wg_fail(WG_EINVAL, "%s: held aliases %s", fn, x.name);
        }
    }
    if ((rc = check_integrator(p)) || (rc = check_muscle_bounds(b)) || (rc = check_discrete(b, p))) return rc;
    wg_outputs out = o ? *o : wg_outputs{};
    if ((out.obs || (episodes && out.final_obs)) && out.obs_stride < pol->obs_dim)
        return wg_fail(WG_EINVAL, "%s: obs_stride %d < obs_dim %d", fn, out.obs_stride, pol->obs_dim);
    if (episodes && (out.nonfinite || out.momentum))
        return wg_fail(WG_EINVAL, "%s: nonfinite / momentum are not produced here", fn);
    if (!episodes && (out.nonfinite || out.momentum || out.reset || out.final_obs))
        return wg_fail(WG_EINVAL, "%s: nonfinite / momentum / reset / final_obs are not produced here", fn);
    LeanGeo lg{};
    if (b->ragged || p->spring_mode != 0 || p->pair_mode != 0 ||
        !lean_geo(b, (out.obs || (episodes && out.final_obs)) ? out.obs_stride : 0, &lg, p->spring_mode))
        return wg_fail(WG_EINVAL, "%s needs a batch the resident lean kernel takes (uniform, M dividing 64, "
                               "spring_mode 0, pair_mode 0, WG_LEAN not 0)", fn);
    if (b->N == 0) return 0;
    const KParams kp = make_kparams(*p);
    KPolicy kpol{};
    kpol.w1 = pol->hidden > 0 ? pol->w1 : nullptr; kpol.b1 = pol->hidden > 0 ? pol->b1 : nullptr;
    kpol.w2 = pol->w2; kpol.b2 = pol->b2;
    kpol.action_out = pol->action_out; kpol.return_out = pol->return_out; kpol.length_out = pol->length_out;
    kpol.action_out_step = pol->action_out_step;
    kpol.act_limit = pol->act_limit;
    kpol.D = pol->obs_dim; kpol.H = pol->hidden; kpol.C = pol->act_dim;
    kpol.wps = b->N / pol->n_sets;
    kpol.off_row = lg.slice;
    kpol.off_h = kpol.off_row + align16(lg.wpw * kpol.D * 4);
    kpol.off_a = kpol.off_h + align16(std::max(1, lg.wpw * kpol.H) * 4);
    kpol.off_w = kpol.off_a + align16(lg.wpw * kpol.C * 4);
    lg.slice = kpol.off_w + lg.wpw * (episodes ? 32 : 16);
    KHold kh{};
    if (held) {   // one more float per walker: the open hold's reward
        kh = KHold{hold->held, hold->decided_out, hold->hold_reward_out, hold->decided_out_step,
                   hold->hold_reward_out_step, hold->every, lg.slice};
        lg.slice += align16(lg.wpw * 4);
    }
    KDeep kd{};
    if (deep) {   // hidden2 more floats per walker: the second hidden vector
        kd = KDeep{mid->wm, mid->bm, mid->hidden2, lg.slice};
        lg.slice += align16(lg.wpw * mid->hidden2 * 4);
    }
    int lds = lg.wpb * lg.slice;
    if (lds > 80 * 1024) return wg_fail(WG_ERANGE, "%s: workgroup needs %d B of LDS (> 80 KiB)", fn, lds);
    // a shared policy's weights staged in LDS where that costs no resident wave: as many workgroups per CU (160 KiB of
    // LDS, the kernel's register budget of 4 waves per SIMD, 3 at NE 8) with the weights as without.  (Staged at the
    // price of occupancy the canonical batch ran 90.6 us per step with H = 32 against 73.8 through L2; the one-wave
    // workgroups of a small batch keep their occupancy and run 7.96 against 9.03: profiles/r08_policy_rollout_ab.json.)
    // WG_POLICY_STAGE (read on every call, like WG_LEAN): 0 never, 2 whenever the workgroup stays within 80 KiB
    const int wbytes = deep ? 4 * (kpol.D * kpol.H + kpol.H * kd.H2 + kd.H2 * kpol.C)
                            : 4 * (kpol.D * kpol.H + (kpol.H > 0 ? kpol.H : kpol.D) * kpol.C);
    const int ne = lean_passes(lg, b);
    const int cap = std::max(1, (ne > 4 ? 12 : 16) / lg.wpb);
    const int stage = env_int("WG_POLICY_STAGE", 1);
    const bool free_stage = std::min(cap, LDS_LIMIT / lds) == std::min(cap, LDS_LIMIT / (lds + wbytes));
    kpol.off_wts = -1;
    if (pol->n_sets == 1 && lds + wbytes <= 80 * 1024 && (stage == 2 || (stage == 1 && free_stage))) {
        kpol.off_wts = lds;
        lds += wbytes;
    }
    const dim3 grid(lg.nblk), block(64 * lg.wpb);
    const KReset ar = kreset(out, p->auto_reset);
    KNoise kn{};
    if (stochastic)
        kn = KNoise{nz->sigma, nz->raw_out, nz->eps_out, nz->raw_out_step, nz->eps_out_step,
                    (uint32_t)(nz->seed & 0xffffffffu), (uint32_t)(nz->seed >> 32), nz->step_base, nz->walker_base};
    const KObsNorm kon = normalized ? KObsNorm{nm->mean, nm->scale, nm->clip} : KObsNorm{};   // (held: a null mean = off)
    with_instance(p->in3d != 0, ne, use_edge8(b, lg), [&](auto d3, auto n, auto c8) {
        constexpr bool D3 = decltype(d3)::value, E8 = decltype(c8)::value;
        constexpr int NE = decltype(n)::value;
        auto go = [&](auto kernel, const auto &reset, const auto &stats, const auto &noise, const auto &norm) {
            hipLaunchKernelGGL(kernel, grid, block, lds, stream, *b, kp, kpol, kout(out), n_steps, lg, reset, stats, noise,
                               norm, KNoReset{}, KNoReset{});
        };
        if (deep) {   // (held, with the middle layer)
            if (episodes)
                hipLaunchKernelGGL((walker_rollout_policy<D3, NE, E8, true, true, true, true, true>), grid, block, lds,
                                   stream, *b, kp, kpol, kout(out), n_steps, lg, ar, *st, kn, kon, kh, kd);
            else
                hipLaunchKernelGGL((walker_rollout_policy<D3, NE, E8, false, true, true, true, true>), grid, block, lds,
                                   stream, *b, kp, kpol, kout(out), n_steps, lg, KNoReset{}, KNoReset{}, kn, kon, kh, kd);
        } else if (held) {   // (kn with a null sigma, kon with a null mean: that option is off)
            if (episodes)
                hipLaunchKernelGGL((walker_rollout_policy<D3, NE, E8, true, true, true, true>), grid, block, lds, stream, *b,
                                   kp, kpol, kout(out), n_steps, lg, ar, *st, kn, kon, kh, KNoReset{});
            else
                hipLaunchKernelGGL((walker_rollout_policy<D3, NE, E8, false, true, true, true>), grid, block, lds, stream,
                                   *b, kp, kpol, kout(out), n_steps, lg, KNoReset{}, KNoReset{}, kn, kon, kh, KNoReset{});
        } else if (normalized) {
            if (stochastic) {
                if (episodes) go(walker_rollout_policy<D3, NE, E8, true, true, true>, ar, *st, kn, kon);
                else go(walker_rollout_policy<D3, NE, E8, false, true, true>, KNoReset{}, KNoReset{}, kn, kon);
            } else {
                if (episodes) go(walker_rollout_policy<D3, NE, E8, true, false, true>, ar, *st, KNoReset{}, kon);
                else go(walker_rollout_policy<D3, NE, E8, false, false, true>, KNoReset{}, KNoReset{}, KNoReset{}, kon);
            }
        } else if (stochastic) {
            if (episodes) go(walker_rollout_policy<D3, NE, E8, true, true>, ar, *st, kn, KNoReset{});
            else go(walker_rollout_policy<D3, NE, E8, false, true>, KNoReset{}, KNoReset{}, kn, KNoReset{});
        } else {
            if (episodes) go(walker_rollout_policy<D3, NE, E8, true>, ar, *st, KNoReset{}, KNoReset{});
            else go(walker_rollout_policy<D3, NE, E8>, KNoReset{}, KNoReset{}, KNoReset{}, KNoReset{});
        }
    });
    return wg_launched("launch");
}

// ---- ragged wave kernel (wg_batch.ragged = 2): geometry, launch (its spring passes: wave_passes, above)
bool rag_geo(const wg_batch *b, int obs_stride, RagGeo *out) {
    const int ne = wave_passes(b->M, b->K);
    if (b->ragged != 2 || ne == 0 || b->A > 64 || !u32_bytes(b) || !obs_u32(b, obs_stride)) return false;
    RagGeo g{};
    const int wpb = env_int("WG_LEAN_WAVES", 4);
    g.wpb = (wpb == 1 || wpb == 2) ? wpb : 4;
    const int ec = 64 * ne;                                      // spring slots of a tile
    // spring terms t (f64 x3), later the per-mass reduction terms | damping forces df, later the walker partials |
    // incidence words | muscle x | walker offsets and rows
    g.off_df = align16(std::max(ec * 24, 4 * 64 * 6));
    g.off_inc = g.off_df + align16(std::max(ec * 12, 4 * RW_MAXW * 8));
    g.off_x = g.off_inc + align16(ec * 4 + 4);                   // + the read-ahead pad word (mass_accumulate_v2)
    g.off_wo = g.off_x + align16(64 * 4);
    g.slice = g.off_wo + align16(4 * (RW_MAXW + 1) * 3 + 4 * RW_MAXW + 12 * RW_MAXW);   // + the walkers' means
    *out = g;
    return true;
}

int launch_waves(const wg_batch *b, const KParams &kp, bool in3d, const Actions &a, const wg_outputs &o,
                 const int32_t *plan, int ntiles, const RagGeo &g, hipStream_t st) {
    const dim3 grid((ntiles + g.wpb - 1) / g.wpb), block(64 * g.wpb);
    const uint32_t lds = (uint32_t)(g.wpb * g.slice);
    with_instance(in3d, wave_passes(b->M, b->K), [&](auto d3, auto n) {
        WG_KLAUNCH((walker_step_waves<decltype(d3)::value, decltype(n)::value>), grid, block, lds, st, *b, kp, a.ptr,
                   a.cols, a.stride, kout(o), plan, ntiles, g);
    });
    return wg_launched("launch");
}

int reset_impl(const wg_batch *b, const float *noise, const uint8_t *mask, int zmode, hipStream_t stream) {
    int rc = validate(b);
    if (rc) return rc;
    if (b->N == 0) return 0;
    const long P = b->ragged ? -1 : (long)b->N * b->M;
    const int blocks = P > 0 ? (int)std::min<long>((P + 255) / 256, 4096) : 1024;
    hipLaunchKernelGGL(walker_reset_kernel, dim3(blocks), dim3(256), 0, stream, *b, noise, mask, zmode);
    return wg_launched("reset launch");
}

template <bool STEP>
int dispatch(const wg_batch *b, const KParams &kp, bool in3d, const float *a, int cols, int astride,
             const wg_outputs &o, const int32_t *plan, int blocks, const Geo &g, hipStream_t st) {
    return b->M <= 128 ? dispatch2<STEP, 0>(b, kp, in3d, a, cols, astride, o, plan, blocks, g, st)
                       : dispatch2<STEP, 3>(b, kp, in3d, a, cols, astride, o, plan, blocks, g, st);
}

// the outputs of step s of a call (rows out_step / obs_step apart; the three-component ones 3 * out_step)
wg_outputs outputs_at(const wg_outputs &o, int s) {
    wg_outputs os = o;
    if (os.obs) os.obs += s * os.obs_step;
    if (os.reward) os.reward += s * os.out_step;
    if (os.done) os.done += s * os.out_step;
    if (os.energy) os.energy += s * os.out_step;
    if (os.centroid) os.centroid += 3 * s * os.out_step;
    if (os.steps) os.steps += s * os.out_step;
    if (os.nonfinite) os.nonfinite += s * os.out_step;
    if (os.momentum) os.momentum += 3 * s * os.out_step;
    if (os.reset) os.reset += s * os.out_step;
    if (os.final_obs) os.final_obs += s * os.obs_step;
    return os;
}

// What a run() call is, beside the batch, parameters, outputs and plan.  Every entry fills it by field name.
struct RunCall {
    bool step;         // env steps; false: the outputs of the state as it is (wg_observe), one launch
    bool resident;     // every step in one launch where the batch allows it (wg_rollout); false: a launch per step
    bool check_only;   // check every argument, launch nothing (wg_run_ranges, wg_time_step: before their first launch)
    int s_first;       // the index of this call's first step in the caller's whole call (its outputs and actions)
    int s_total;       // the steps of that whole call when this is one slice of it: 0 = s_first + n_steps, < 0 = every
                       // step keeps its acc / contact stores (wg_time_step)
    Actions act;
};

int run(const wg_batch *b, const wg_params *p, const wg_outputs *o, int32_t n_steps, const int32_t *plan,
        int32_t plan_blocks, hipStream_t stream, const RunCall &c) {
    const bool step = c.step;
    Actions act = c.act;
    if (!act.ptr) act.step = 0;
    int rc = validate(b);
    if (rc) return rc;
    if (!p) return wg_fail(WG_EINVAL, "null params");
    if (b->N == 0 || n_steps <= 0) return 0;
    if (act.ptr && (act.cols < 0 || act.stride < act.cols)) return wg_fail(WG_EINVAL, "bad action stride");
    if (act.ptr && (rc = check_discrete(b, p))) return rc;
    if ((rc = check_integrator(p))) return rc;
    if (act.ptr && (rc = check_muscle_bounds(b))) return rc;
    if (b->ragged && (!plan || plan_blocks <= 0)) return wg_fail(WG_EINVAL, "ragged batch needs a plan");
    wg_outputs out = o ? *o : wg_outputs{};
    if (out.obs && out.obs_stride <= 0) return wg_fail(WG_EINVAL, "obs_stride must be > 0");
    KParams kp = make_kparams(*p);
    const Geo g = b->ragged ? ragged_geo(b) : uniform_geo(b, out.obs ? out.obs_stride : 0, step && p->pair_mode != 0);
    if (g.W > g.threads) return wg_fail(WG_ERANGE, "more than %d walkers per workgroup", g.threads);
    const int blocks = b->ragged ? plan_blocks : (b->N + g.W - 1) / g.W;
    LeanGeo lg{};
    const bool act_u32 = !act.ptr || (int64_t)b->N * act.stride * 4 < (1ll << 32);   // at_u32 action offsets
    const bool use_lean = step && act_u32 && lean_geo(b, out.obs ? out.obs_stride : 0, &lg, p->spring_mode);
    RagGeo rgeo{};
    const bool use_waves = step && act_u32 && p->spring_mode == 0 && p->pair_mode == 0 && lean_enabled() &&
                           rag_geo(b, out.obs ? out.obs_stride : 0, &rgeo);
    if (p->spring_mode < 0 || p->spring_mode > 2)
        return wg_fail(WG_EINVAL, "spring_mode %d: 0 (engine.py), 1 (G2 element), 2 (G3 engine) only", p->spring_mode);
    if (step && (p->pair_mode & ~31))
        return wg_fail(WG_EINVAL, "pair_mode %d: bits 1 (gravity), 2 (coulomb), 4 (bounce), 8 (G2 gravity_vec), "
                                  "16 (electrostatic) only", p->pair_mode);
    if (step && p->pair_mode != 0 && p->spring_mode != 0)
        return wg_fail(WG_EINVAL, "pair_mode %d needs spring_mode 0", p->pair_mode);
    if (step && (p->pair_mode & 4) && !b->radius)
        return wg_fail(WG_EINVAL, "pair_mode 4 (bounce) needs the radius array");
    // auto-reset (ABI 16): fused into the lean step kernels only; everything it reads checked here
    const int ar_mode = step ? p->auto_reset : 0;
    if (ar_mode) {
        if ((rc = check_auto_reset(b, ar_mode))) return rc;
        if (p->pair_mode != 0) return wg_fail(WG_EINVAL, "auto_reset needs pair_mode 0 (pair_mode %d)", p->pair_mode);
        if (!use_lean)
            return wg_fail(WG_EINVAL, "auto_reset needs a batch the lean kernel takes (uniform, M dividing 64, "
                                      "spring_mode 0, pair_mode 0, WG_LEAN not 0): the ragged wave kernel and the "
                                      "workgroup kernel have no auto-reset");
    }
    if (c.check_only) return 0;
    const bool in3d = p->in3d != 0;
    const bool extras = out.nonfinite || out.momentum;   // opt-in per-walker info after each step (ABI 10)
    auto info_pass = [&](const wg_outputs &os) -> int {
        if (!(os.nonfinite || os.momentum)) return 0;
        hipLaunchKernelGGL(walker_info_kernel, dim3((b->N + 255) / 256), dim3(256), 0, stream, *b, os.nonfinite,
                           os.momentum, b->ragged ? plan : nullptr, plan_blocks);
        return wg_launched("info launch");
    };
    // (the resident rollout keeps the state in registers between steps: with the per-step info extras requested the
    // steps run as per-step launches instead, bit-identical)
    // (with auto-reset: the resident kernel's AR twin, the reset tail in its loop, where its episode counts fit beside
    // the slices in the lean kernel's 80 KiB)
    const bool ar_fits = !ar_mode || lg.wpb * (lg.slice + align16(lg.wpw * 4)) <= 80 * 1024;
    if (c.resident && use_lean && p->pair_mode == 0 && !extras && ar_fits)   // one launch for every step
        return launch_lean_rollout(b, kp, in3d, act, out, n_steps, lg, stream, ar_mode);
    // acc and contact are read by nothing on the step path and overwritten by the next step: only the call's last step
    // stores them (the info kernel reads acc: with its outputs requested every step does)
    const int s_last = (c.s_total > 0 ? c.s_total : c.s_first + n_steps) - 1;
    for (int s = c.s_first; s < c.s_first + n_steps; s++) {
        kp.keep_aux = (c.s_total < 0 || s >= s_last || extras) ? 1 : 0;
        const wg_outputs os = outputs_at(out, s);
        const Actions a = act.at(s);
        if (use_lean) rc = launch_lean(b, kp, in3d, a, os, lg, stream, ar_mode);
        else if (use_waves) rc = launch_waves(b, kp, in3d, a, os, plan, plan_blocks, rgeo, stream);
        else rc = step ? dispatch<true>(b, kp, in3d, a.ptr, a.cols, a.stride, os, plan, blocks, g, stream)
                       : dispatch<false>(b, kp, in3d, nullptr, 0, 0, os, plan, blocks, g, stream);
        if (rc) return rc;
        if (extras && (rc = info_pass(os))) return rc;
    }
    return 0;
}

// The greedy packer of wg_plan_waves and wg_plan_ragged: consecutive walkers join a group (a wave tile, a workgroup)
// while its masses, springs, muscles and walkers stay within the caps; plan[i] .. plan[i + 1] are group i's walkers.
// A walker over a cap by itself: refused where the group cannot hold it (strict: a wave tile), a group of its own
// otherwise (the ragged workgroup kernel sizes its LDS from the batch maxima).
struct PackCaps { int P, E, U, W; };
int pack_plan(const int32_t *mass_off, const int32_t *edge_off, const int32_t *muscle_off, int N, int32_t *plan,
              int max_groups, const PackCaps &c, bool strict, const char *unit) {
    int groups = 0, w = 0;
    plan[0] = 0;
    while (w < N) {
        int P = 0, E = 0, U = 0, n = 0;
        while (w < N) {
            const int m = mass_off[w + 1] - mass_off[w], k = edge_off[w + 1] - edge_off[w],
                      a = muscle_off[w + 1] - muscle_off[w];
            if (strict && (m > c.P || a > c.U || k > c.E)) return wg_fail(WG_EINVAL, "walker %d does not fit one wave", w);
            if (n > 0 && (P + m > c.P || E + k > c.E || U + a > c.U || n + 1 > c.W)) break;
            P += m; E += k; U += a; n++; w++;
        }
        if (groups + 1 > max_groups) return wg_fail(WG_ERANGE, "plan needs more than %d %s", max_groups, unit);
        plan[++groups] = w;
    }
    return groups;
}
