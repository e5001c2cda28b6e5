/* wg_expf.h — the library's own float32 exponential, one definition for the kernels (HIP device code) and for host
 * probes (HIP host code or plain C).  `exp` has no cross-platform bit-exact definition; this one is pinned operation by
 * operation (include/walker_hip.h, wg_expf), as powf2.h pins `** 2`.
 *
 * For a float32 x:  a NaN returns x.  Otherwise xd = (double)x clamped to [-150, 150] (so +-inf follow the clamp),
 *   k = rint(RN64(xd * LOG2E))                                  ties to even; |k| <= 217
 *   r = RN64(RN64(xd - RN64(k * LN2_HI)) - RN64(k * LN2_LO))    k * LN2_HI is exact: LN2_HI has 21 trailing zero bits
 *   p = C13;  for n = 12 .. 0:  p = RN64(RN64(p * r) + Cn)      Cn = RN64(1 / n!)
 *   result = RN32(ldexp(p, k))                                  ldexp is exact in float64; one double -> float rounding
 * |r| stays near ln2 / 2, where the degree-13 Taylor remainder is below 2^-56 of the sum: p carries a few float64 ulps
 * of error into a single rounding to float32 (tests/test_ppo_cpu.py compares against RN32 of a float64 exp).  Overflow
 * gives +inf (x >= 88.72284), float32 subnormals are rounded once (x = -103.9 gives 1e-45), x <= -104 gives +0, and
 * exp(+-0) = 1 exactly (k = 0, r = +-0, every Horner step adds a positive constant).  No FMA anywhere: every operation
 * is rounded by itself. */
#ifndef WALKER_WG_EXPF_H
#define WALKER_WG_EXPF_H

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define WE_FN __host__ __device__ __forceinline__
#else
#include <math.h>
#define WE_FN static inline
#endif

#if defined(__HIP_DEVICE_COMPILE__) && __HIP_DEVICE_COMPILE__
#define WE_MUL(a, b) __dmul_rn((a), (b))
#define WE_ADD(a, b) __dadd_rn((a), (b))
#define WE_SUB(a, b) __dsub_rn((a), (b))
#else
/* the host: a volatile result keeps a compiler from contracting a product into the sum that follows it */
static inline double we_mul_host(double a, double b) { volatile double v = a * b; return v; }
static inline double we_add_host(double a, double b) { volatile double v = a + b; return v; }
static inline double we_sub_host(double a, double b) { volatile double v = a - b; return v; }
#define WE_MUL(a, b) we_mul_host((a), (b))
#define WE_ADD(a, b) we_add_host((a), (b))
#define WE_SUB(a, b) we_sub_host((a), (b))
#endif

#define WE_LOG2E 0x1.71547652b82fep+0
#define WE_LN2_HI 0x1.62e42fee00000p-1
#define WE_LN2_LO 0x1.a39ef35793c76p-33

WE_FN float wg_expf_scalar(float x) {
    if (x != x) return x;
    double xd = (double)x;
    xd = xd < -150.0 ? -150.0 : (xd > 150.0 ? 150.0 : xd);
    const double k = rint(WE_MUL(xd, WE_LOG2E));
    const double r = WE_SUB(WE_SUB(xd, WE_MUL(k, WE_LN2_HI)), WE_MUL(k, WE_LN2_LO));
    /* Cn = RN64(1 / n!): n! is exact in float64 up to 13!, and the division of two constants is folded correctly rounded */
    double p = 1.0 / 6227020800.0;
    p = WE_ADD(WE_MUL(p, r), 1.0 / 479001600.0);
    p = WE_ADD(WE_MUL(p, r), 1.0 / 39916800.0);
    p = WE_ADD(WE_MUL(p, r), 1.0 / 3628800.0);
    p = WE_ADD(WE_MUL(p, r), 1.0 / 362880.0);
    p = WE_ADD(WE_MUL(p, r), 1.0 / 40320.0);
    p = WE_ADD(WE_MUL(p, r), 1.0 / 5040.0);
    p = WE_ADD(WE_MUL(p, r), 1.0 / 720.0);
    p = WE_ADD(WE_MUL(p, r), 1.0 / 120.0);
    p = WE_ADD(WE_MUL(p, r), 1.0 / 24.0);
    p = WE_ADD(WE_MUL(p, r), 1.0 / 6.0);
    p = WE_ADD(WE_MUL(p, r), 0.5);
    p = WE_ADD(WE_MUL(p, r), 1.0);
    p = WE_ADD(WE_MUL(p, r), 1.0);
    return (float)ldexp(p, (int)k);
}

#endif /* WALKER_WG_EXPF_H */
