// The operand contract of the rows-family entry points (robust.hip, pairdist.hip,
// gram.hip, weiszfeld.hip), host only: K selected rows of an fp32 matrix at pitch ldu,
// read over their first P elements as 16-byte vectors.  An entry point makes the
// checks in this order: the head (non-null pointers, then 1 <= K <= DLS_ROBUST_MAX_K),
// its rule's own scalar (at the entry point), the layout (P >= 0, P and the pitches
// multiples of 4 and >= P, the alignment); then P == 0 ends the call early.
#pragma once

#include "dls_common.h"

namespace dls {

inline int check_count(const char *fn, const char *name, int32_t K) {
    DLS_REQUIRE(K >= 1 && K <= DLS_ROBUST_MAX_K, DLS_EINVAL, "%s: %s=%d (1..DLS_ROBUST_MAX_K=%d)",
                fn, name, K, DLS_ROBUST_MAX_K);
    return DLS_OK;
}

inline int check_head(const char *fn, bool nonnull, const char *name, int32_t K) {
    DLS_REQUIRE(nonnull, DLS_EINVAL, "%s: null pointer", fn);
    return check_count(fn, name, K);
}

// `aligned`: the entry point's own alignment test; `which`: what its message says
// after "16-byte alignment", e.g. " (U, workspace), 8-byte (D)"; `ldh`: the second
// pitch of a call on two matrices (gram.hip), named in the message beside ldu.
inline int check_layout(const char *fn, int64_t ldu, int64_t P, bool aligned,
                        const char *which = "", const int64_t *ldh = nullptr) {
    DLS_REQUIRE(P >= 0, DLS_EINVAL, "%s: P=%lld", fn, (long long)P);
    if (ldh) {
        DLS_REQUIRE(P % 4 == 0 && ldu % 4 == 0 && ldu >= P && *ldh % 4 == 0 && *ldh >= P,
                    DLS_ELAYOUT,
                    "%s: P=%lld, ldu=%lld and ldh=%lld must be multiples of 4, ldu and ldh >= P",
                    fn, (long long)P, (long long)ldu, (long long)*ldh);
    } else {
        DLS_REQUIRE(P % 4 == 0 && ldu % 4 == 0 && ldu >= P, DLS_ELAYOUT,
                    "%s: P=%lld and ldu=%lld must be multiples of 4, ldu >= P", fn, (long long)P,
                    (long long)ldu);
    }
    DLS_REQUIRE(aligned, DLS_ELAYOUT, "%s: 16-byte alignment%s", fn, which);
    return DLS_OK;
}

inline bool aligned_to(const void *p, uintptr_t bytes) {
    return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0;
}

// A dls_*_workspace query: the bytes of `part_doubles` doubles for each of the nW()
// waves of the launch plan, which is made once K and P are known to be in range.
template <typename Waves>
int64_t workspace_query(const char *fn, int32_t K, int64_t P, Waves nW, int part_doubles) {
    const int rc = check_count(fn, "K", K);
    if (rc != DLS_OK) return rc;
    DLS_REQUIRE(P >= 0, DLS_EINVAL, "%s: P=%lld", fn, (long long)P);
    return (int64_t)nW() * part_doubles * (int64_t)sizeof(double);
}

// The P == 0 exit of an entry point with an fp64 result: n zeros, in stream order.
inline int zero_f64(const char *fn, double *out, size_t n, hipStream_t st) {
    const hipError_t e = hipMemsetAsync(out, 0, n * sizeof(double), st);
    DLS_REQUIRE(e == hipSuccess, (int)e, "%s: %s", fn, hipGetErrorString(e));
    return DLS_OK;
}

}  // namespace dls
