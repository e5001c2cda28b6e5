// walker_internal.h — what libwalker_hip.so's translation units (walker_hip.hip, es_hip.hip, pg_hip.hip) share and do not export.
#pragma once

#include <hip/hip_runtime.h>

#include "walker_hip.h"

// Formats the calling thread's wg_last_error() text (512 bytes, owned by walker_hip.hip) and returns `code`.
__attribute__((visibility("hidden"), format(printf, 2, 3))) int wg_fail(int code, const char *fmt, ...);

// After a kernel launch: 0, or WG_EHIP with "<what> failed: <the runtime's error>".
static inline int wg_launched(const char *what) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : wg_fail(WG_EHIP, "%s failed: %s", what, hipGetErrorString(e));
}
