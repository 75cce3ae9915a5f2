// rowlist.h — the host checks that the stages for finished rows share (shortcut.hip, timing.hip, blend.hip, sdf.hip's repair): the
// per-joint limits and the row list of a call, each refusal spelled once with `what` naming the entry point; and the list's way to the
// device and back for the calls that do not keep a block for it.
#pragma once
#include <cmath>

#include "common.h"

namespace edmp {

// a per-joint limit array of a call: seven finite values > 0
inline int check_limits(const char* what, const char* name, const double* v) {
    EDMP_REQUIRE(v, "%s: %s is a null pointer", what, name);
    for (int j = 0; j < 7; ++j) EDMP_REQUIRE(std::isfinite(v[j]) && v[j] > 0.0, "%s: %s[%d] = %g must be finite and > 0", what, name, j, v[j]);
    return EDMP_OK;
}

// the row list of a call over n rows, checked on the host (nullptr = every row): two workgroups on one row would write the same outputs
inline int check_rows(const char* what, const int32_t* rows_host, int n_rows, int n) {
    if (!rows_host) return EDMP_OK;
    EDMP_REQUIRE(n_rows >= 1 && n_rows <= n, "%s: %d listed rows outside 1..%d", what, n_rows, n);
    std::vector<char> seen((size_t)n, 0);
    for (int i = 0; i < n_rows; ++i) {
        EDMP_REQUIRE(rows_host[i] >= 0 && rows_host[i] < n, "%s: rows[%d] = %d outside 0..%d", what, i, (int)rows_host[i], n - 1);
        EDMP_REQUIRE(!seen[rows_host[i]], "%s: rows[%d] = %d is listed twice", what, i, (int)rows_host[i]);
        seen[rows_host[i]] = 1;
    }
    return EDMP_OK;
}

// the checked list in a block of the call's own from the context's pool (nullptr stays nullptr): nothing of the guide, the sampler or a
// segmented run is replaced.  Called behind every refusal of the entry point; rows_call_end gives the block back
inline int rows_upload(edmp_ctx* ctx, const int32_t* rows_host, int n_rows, int32_t** rows_dev) {
    *rows_dev = nullptr;
    if (!rows_host) return EDMP_OK;
    if (int rc = ctx_alloc(ctx, (void**)rows_dev, (size_t)n_rows * sizeof(int32_t))) return rc;
    const hipError_t e = hipMemcpyAsync(*rows_dev, rows_host, (size_t)n_rows * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream);
    if (e != hipSuccess) {
        ctx_release(ctx, *rows_dev);
        *rows_dev = nullptr;
        EDMP_HIP_CHECK(e);
    }
    return EDMP_OK;
}

// right behind the launch that reads rows_upload's block: the launch's error, the call's synchronise (the list lives in the caller's
// array), and only then the block goes back to the pool - on the error paths too
inline int rows_call_end(edmp_ctx* ctx, int32_t* rows_dev) {
    const hipError_t e = hipGetLastError();
    const hipError_t w = hipStreamSynchronize(ctx->stream);
    if (rows_dev) ctx_release(ctx, rows_dev);
    EDMP_HIP_CHECK(w);
    EDMP_HIP_CHECK(e);
    return EDMP_OK;
}

}  // namespace edmp
