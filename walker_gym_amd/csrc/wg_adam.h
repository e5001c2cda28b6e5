/* wg_adam.h — the scalar arithmetic of wg_adam_step (include/walker_hip.h), one definition for the kernels (HIP device
 * code) and for host probes (HIP host code or plain C), as wg_expf.h is for the exponential.
 *
 * Two pieces: the per-step scalars (float64, one thread) and the element update (float32).  Every operation is rounded
 * by itself: no FMA, no reassociation.  Multiply, add, subtract, divide and square root are correctly rounded in both
 * worlds (the device build passes -fhip-fp32-correctly-rounded-divide-sqrt and keeps denormals), so the bits agree.
 *
 * The float32 square root is sqrtf under that flag, not __fsqrt_rn: HIP's __fsqrt_rn is the native approximation
 * (1 ulp) unless OCML's rounded operations are switched on, and the contract needs RN32(sqrt(v)). */
#pragma once

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define WA_FN __host__ __device__ __forceinline__
#else
#include <math.h>
#define WA_FN static inline
#endif

#if defined(__HIP_DEVICE_COMPILE__) && __HIP_DEVICE_COMPILE__
#define WA_FMUL(a, b) __fmul_rn((a), (b))
#define WA_FADD(a, b) __fadd_rn((a), (b))
#define WA_FSUB(a, b) __fsub_rn((a), (b))
#define WA_FDIV(a, b) __fdiv_rn((a), (b))
#define WA_DMUL(a, b) __dmul_rn((a), (b))
#define WA_DADD(a, b) __dadd_rn((a), (b))
#define WA_DSUB(a, b) __dsub_rn((a), (b))
#define WA_DDIV(a, b) __ddiv_rn((a), (b))
#define WA_DSQRT(a) __dsqrt_rn((a))
#else
/* the host: a volatile result keeps a compiler from contracting a product into the sum that follows it, and from
 * carrying a float32 intermediate in a wider register */
static inline float wa_fmul_host(float a, float b) { volatile float v = a * b; return v; }
static inline float wa_fadd_host(float a, float b) { volatile float v = a + b; return v; }
static inline float wa_fsub_host(float a, float b) { volatile float v = a - b; return v; }
static inline float wa_fdiv_host(float a, float b) { volatile float v = a / b; return v; }
static inline double wa_dmul_host(double a, double b) { volatile double v = a * b; return v; }
static inline double wa_dadd_host(double a, double b) { volatile double v = a + b; return v; }
static inline double wa_dsub_host(double a, double b) { volatile double v = a - b; return v; }
static inline double wa_ddiv_host(double a, double b) { volatile double v = a / b; return v; }
#define WA_FMUL(a, b) wa_fmul_host((a), (b))
#define WA_FADD(a, b) wa_fadd_host((a), (b))
#define WA_FSUB(a, b) wa_fsub_host((a), (b))
#define WA_FDIV(a, b) wa_fdiv_host((a), (b))
#define WA_DMUL(a, b) wa_dmul_host((a), (b))
#define WA_DADD(a, b) wa_dadd_host((a), (b))
#define WA_DSUB(a, b) wa_dsub_host((a), (b))
#define WA_DDIV(a, b) wa_ddiv_host((a), (b))
#define WA_DSQRT(a) sqrt((a))
#endif

/* What a step's elements share.  skip != 0: the squared norm was not finite and nothing is to be written. */
typedef struct wg_adam_consts {
    float lr, beta1, beta2, omb1, omb2, eps, lrwd; /* omb = RN32(1 - beta); lrwd = RN32(lr * weight_decay) */
    float a, r2, cf;                               /* RN32(lr / c1), RN32(sqrt(c2)), the clip coefficient */
    int decay, flip, skip;                         /* weight_decay != 0; maximize != 0 */
} wg_adam_consts;

/* a and r2 from the advanced powers b1p' = beta1^t', b2p' = beta2^t' (the values a step leaves in state[1], state[2]). */
WA_FN void wg_adam_rates(double b1p, double b2p, float lr, float *a, float *r2) {
    const double c1 = WA_DSUB(1.0, b1p), c2 = WA_DSUB(1.0, b2p);
    *a = (float)WA_DDIV((double)lr, c1);
    *r2 = (float)WA_DSQRT(c2);
}

/* The constants that do not depend on the step's norm or count. */
WA_FN void wg_adam_fixed(float lr, float beta1, float beta2, float eps, float weight_decay, int maximize,
                         wg_adam_consts *k) {
    k->lr = lr;
    k->beta1 = beta1;
    k->beta2 = beta2;
    k->omb1 = WA_FSUB(1.0f, beta1);
    k->omb2 = WA_FSUB(1.0f, beta2);
    k->eps = eps;
    k->lrwd = WA_FMUL(lr, weight_decay);
    k->decay = weight_decay != 0.0f;
    k->flip = maximize != 0;
}

/* One step's scalars from S, the ordered float64 sum of the squared gradients.  state is wg_adam_step's [8]: t, b1p,
 * b2p, norm, cf, skipped, and two slots left alone.  Writes state and fills k->a, k->r2, k->cf, k->skip. */
WA_FN void wg_adam_scalars(double S, double *state, float lr, float beta1, float beta2, float max_norm,
                           wg_adam_consts *k) {
    const double norm = WA_DSQRT(S);
    state[3] = norm;
    if (!(S - S == 0.0)) { /* inf or NaN: the step is skipped */
        state[4] = 0.0;
        state[5] = WA_DADD(state[5], 1.0);
        k->a = k->r2 = k->cf = 0.0f;
        k->skip = 1;
        return;
    }
    const double t = state[0];
    const double b1p = WA_DMUL(t == 0.0 ? 1.0 : state[1], (double)beta1);
    const double b2p = WA_DMUL(t == 0.0 ? 1.0 : state[2], (double)beta2);
    double c = WA_DDIV((double)max_norm, WA_DADD(norm, 1e-6));
    c = c < 1.0 ? c : 1.0;
    k->cf = (float)c;
    wg_adam_rates(b1p, b2p, lr, &k->a, &k->r2);
    k->skip = 0;
    state[0] = WA_DADD(t, 1.0);
    state[1] = b1p;
    state[2] = b2p;
    state[4] = (double)k->cf;
}

/* One element: g its gradient as stored; p, m, v updated in place. */
WA_FN void wg_adam_element(const wg_adam_consts *k, float g, float *p, float *m, float *v) {
    const float gs = k->flip ? -g : g;
    const float gc = WA_FMUL(gs, k->cf);
    const float m1 = WA_FADD(WA_FMUL(k->beta1, *m), WA_FMUL(k->omb1, gc));
    const float v1 = WA_FADD(WA_FMUL(k->beta2, *v), WA_FMUL(k->omb2, WA_FMUL(gc, gc)));
    const float den = WA_FADD(WA_FDIV(sqrtf(v1), k->r2), k->eps);
    const float upd = WA_FMUL(k->a, WA_FDIV(m1, den));
    const float p0 = *p;
    const float p1 = k->decay ? WA_FSUB(p0, WA_FMUL(k->lrwd, p0)) : p0;
    *p = WA_FSUB(p1, upd);
    *m = m1;
    *v = v1;
}
