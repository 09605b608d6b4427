// Fused server-optimizer step for gfx950: what turns a round's aggregate into the next
// global model when FedServer runs with server_optimizer (FedAvgM, Hsu et al. 2019;
// FedAdagrad / FedAdam / FedYogi, Reddi et al. 2021).  The pseudo-gradient d = agg - x,
// the moment updates and the model update are one pass over P:
//
//   SGD:      m' = fl(fl(beta1*m) + d);                 out = fl(x + fl(lr*m'))
//   adaptive: m' = fl(fl(beta1*m) + fl(omb1*d));  v' by kind from d2 = fl(d*d);
//             out = fl(x + div_ieee(fl(lr*m'), fl(sqrt_ieee(v') + tau)))
//
// (include/dls_hip.h has the contract: every operation rounded once, never fused, so
// numpy float32 reproduces the bits.)  Traffic: agg, x, m, v read once, m, v, out
// written once: 7 * 4 * P bytes (5 * 4 * P for SGD with momentum, 3 * 4 * P without).
//
// Pure streaming: 256-thread blocks, at most DLS_SERVER_OPT_MAX_BLOCKS of them, each
// block walking chunks of 256 * DLS_SERVER_OPT_UNROLL vectors grid-strided; a thread
// issues every load of its DLS_SERVER_OPT_UNROLL vectors (up to 8 x 16 bytes) before
// the first use.  A coordinate is read and written by one thread alone, so out may be
// x itself.  Where the operands do not share one 16-byte phase the same kernel runs
// with one element per "vector"; where they do, up to 3 leading and 3 trailing
// elements are stepped by single lanes of block 0.  The element arithmetic is the same
// inlined function on every path, so the bits do not depend on the alignment.
#include <algorithm>
#include <cmath>

#include "dls_common.h"

namespace dls {
namespace {

constexpr int kBlock = DLS_SERVER_OPT_BLOCK;
constexpr int kMaxBlocks = DLS_SERVER_OPT_MAX_BLOCKS;
constexpr int kUnroll = DLS_SERVER_OPT_UNROLL;

// One coordinate.  HAS_M: SGD with a momentum buffer (the adaptive kinds always have one).
template <int KIND, bool HAS_M>
__device__ __forceinline__ void step_one(float a, float x, float &m, float &v, float &out,
                                         float lr, float beta1, float omb1, float beta2,
                                         float omb2, float tau) {
    const float d = a - x;
    if constexpr (KIND == DLS_SERVER_OPT_SGD) {
        if constexpr (HAS_M) m = beta1 * m + d;
        else m = d;
        out = x + lr * m;
    } else {
        m = beta1 * m + omb1 * d;
        const float d2 = d * d;
        if constexpr (KIND == DLS_SERVER_OPT_ADAGRAD) {
            v = v + d2;
        } else if constexpr (KIND == DLS_SERVER_OPT_ADAM) {
            v = beta2 * v + omb2 * d2;
        } else {
            const float t = v - d2;
            const float s = (float)((t > 0.f) - (t < 0.f));
            v = v - (omb2 * d2) * s;
        }
        out = x + div_ieee(lr * m, sqrt_ieee(v) + tau);
    }
}

template <int W> struct vec_of { typedef f32x4 type; };
template <> struct vec_of<1> { typedef float type; };

template <int W>
__device__ __forceinline__ float get(const typename vec_of<W>::type &q, int j) {
    if constexpr (W == 1) return q;
    else return q[j];
}

template <int W>
__device__ __forceinline__ void put(typename vec_of<W>::type &q, int j, float val) {
    if constexpr (W == 1) q = val;
    else q[j] = val;
}

// W = 4: the operands, advanced by `head` elements, are 16-byte aligned and hold nvec
// whole vectors followed by `tail` elements; W = 1: head = tail = 0, nvec = P.
template <int KIND, bool HAS_M, int W>
__global__ __launch_bounds__(kBlock) void k_server_opt(const float *agg, const float *x, float *m,
                                                       float *v, float *out, int head,
                                                       int64_t nvec, int tail, float lr,
                                                       float beta1, float omb1, float beta2,
                                                       float omb2, float tau) {
    using vec = typename vec_of<W>::type;
    constexpr bool ADAPTIVE = KIND != DLS_SERVER_OPT_SGD;
    const vec *av = reinterpret_cast<const vec *>(agg + head);
    const vec *xv = reinterpret_cast<const vec *>(x + head);
    vec *mv = HAS_M ? reinterpret_cast<vec *>(m + head) : nullptr;
    vec *vv = ADAPTIVE ? reinterpret_cast<vec *>(v + head) : nullptr;
    vec *ov = reinterpret_cast<vec *>(out + head);
    constexpr int64_t chunk = (int64_t)kBlock * kUnroll;
    for (int64_t c = blockIdx.x; c * chunk < nvec; c += gridDim.x) {
        vec qa[kUnroll], qx[kUnroll], qm[kUnroll], qv[kUnroll], qo[kUnroll];
        int64_t i[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            i[u] = c * chunk + (int64_t)u * kBlock + threadIdx.x;
            if (i[u] < nvec) {
                qa[u] = __builtin_nontemporal_load(av + i[u]);
                qx[u] = __builtin_nontemporal_load(xv + i[u]);
                if constexpr (HAS_M) qm[u] = __builtin_nontemporal_load(mv + i[u]);
                if constexpr (ADAPTIVE) qv[u] = __builtin_nontemporal_load(vv + i[u]);
            }
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            if (i[u] < nvec) {
#pragma unroll
                for (int j = 0; j < W; ++j) {
                    float em = 0.f, ev = 0.f, eo;
                    if constexpr (HAS_M) em = get<W>(qm[u], j);
                    if constexpr (ADAPTIVE) ev = get<W>(qv[u], j);
                    step_one<KIND, HAS_M>(get<W>(qa[u], j), get<W>(qx[u], j), em, ev, eo, lr, beta1,
                                          omb1, beta2, omb2, tau);
                    put<W>(qo[u], j, eo);
                    if constexpr (HAS_M) put<W>(qm[u], j, em);
                    if constexpr (ADAPTIVE) put<W>(qv[u], j, ev);
                }
                ov[i[u]] = qo[u];
                if constexpr (HAS_M) mv[i[u]] = qm[u];
                if constexpr (ADAPTIVE) vv[i[u]] = qv[u];
            }
        }
    }
    if constexpr (W == 4) {
        // the elements before and after the aligned body: lanes 0..2 and 4..6 of block 0
        if (blockIdx.x == 0 && threadIdx.x < 8) {
            const int t = threadIdx.x & 3;
            const bool front = threadIdx.x < 4;
            if (t < (front ? head : tail)) {
                const int64_t e = front ? t : head + 4 * nvec + t;
                float em = 0.f, ev = 0.f, eo;
                if constexpr (HAS_M) em = m[e];
                if constexpr (ADAPTIVE) ev = v[e];
                step_one<KIND, HAS_M>(agg[e], x[e], em, ev, eo, lr, beta1, omb1, beta2, omb2, tau);
                out[e] = eo;
                if constexpr (HAS_M) m[e] = em;
                if constexpr (ADAPTIVE) v[e] = ev;
            }
        }
    }
}

template <int KIND, bool HAS_M>
void launch(const float *agg, const float *x, float *m, float *v, float *out, int64_t P, float lr,
            float beta1, float omb1, float beta2, float omb2, float tau, hipStream_t st) {
    // one 16-byte phase for every operand in use, or one element at a time
    const uintptr_t ph = reinterpret_cast<uintptr_t>(agg) & 15u;
    bool same = (reinterpret_cast<uintptr_t>(x) & 15u) == ph &&
                (reinterpret_cast<uintptr_t>(out) & 15u) == ph;
    if (HAS_M) same = same && (reinterpret_cast<uintptr_t>(m) & 15u) == ph;
    if (KIND != DLS_SERVER_OPT_SGD) same = same && (reinterpret_cast<uintptr_t>(v) & 15u) == ph;
    const int64_t chunk = (int64_t)kBlock * kUnroll;
    if (same) {
        const int head = (int)std::min<int64_t>(P, (int64_t)((16u - ph) & 15u) / 4);
        const int64_t nvec = (P - head) / 4;
        const int tail = (int)(P - head - 4 * nvec);
        const int64_t blocks = std::max<int64_t>(1, std::min<int64_t>(kMaxBlocks, (nvec + chunk - 1) / chunk));
        hipLaunchKernelGGL((k_server_opt<KIND, HAS_M, 4>), dim3((unsigned)blocks), dim3(kBlock), 0,
                           st, agg, x, m, v, out, head, nvec, tail, lr, beta1, omb1, beta2, omb2,
                           tau);
    } else {
        const int64_t blocks = std::min<int64_t>(kMaxBlocks, (P + chunk - 1) / chunk);
        hipLaunchKernelGGL((k_server_opt<KIND, HAS_M, 1>), dim3((unsigned)blocks), dim3(kBlock), 0,
                           st, agg, x, m, v, out, 0, P, 0, lr, beta1, omb1, beta2, omb2, tau);
    }
}

// [a, a + n) and [b, b + n) floats share a byte
inline bool overlap(const float *a, const float *b, int64_t n) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    const uintptr_t len = (uintptr_t)n * sizeof(float);
    return a0 < b0 + len && b0 < a0 + len;
}

}  // namespace
}  // namespace dls

using namespace dls;

extern "C" int dls_server_opt_step_f32(int32_t kind, const float *agg, const float *x, float *m,
                                       float *v, float *out, int64_t P, float lr, float beta1,
                                       float omb1, float beta2, float omb2, float tau,
                                       dls_stream_t stream) {
    const char *fn = "dls_server_opt_step_f32";
    DLS_REQUIRE(kind >= DLS_SERVER_OPT_SGD && kind <= DLS_SERVER_OPT_YOGI, DLS_EINVAL,
                "%s: kind=%d (DLS_SERVER_OPT_SGD=0 .. DLS_SERVER_OPT_YOGI=3)", fn, kind);
    DLS_REQUIRE(P >= 0, DLS_EINVAL, "%s: P=%lld", fn, (long long)P);
    DLS_REQUIRE(agg && x && out, DLS_EINVAL, "%s: null pointer (agg, x, out)", fn);
    const bool sgd = kind == DLS_SERVER_OPT_SGD;
    DLS_REQUIRE(!(sgd && v), DLS_EINVAL, "%s: v must be null for DLS_SERVER_OPT_SGD", fn);
    DLS_REQUIRE(sgd || v, DLS_EINVAL, "%s: null pointer (v, kind=%d)", fn, kind);
    const float coef[6] = {lr, beta1, omb1, beta2, omb2, tau};
    for (float c : coef)
        DLS_REQUIRE(std::isfinite(c), DLS_EINVAL,
                    "%s: non-finite coefficient (lr=%g beta1=%g omb1=%g beta2=%g omb2=%g tau=%g)",
                    fn, lr, beta1, omb1, beta2, omb2, tau);
    DLS_REQUIRE(m || (sgd && beta1 == 0.f), DLS_EINVAL,
                "%s: null pointer (m may be null for DLS_SERVER_OPT_SGD with beta1 == 0 alone)", fn);
    const float *ops[5] = {agg, x, m, v, out};
    for (const float *p : ops)
        DLS_REQUIRE((reinterpret_cast<uintptr_t>(p) & 3u) == 0, DLS_ELAYOUT,
                    "%s: 4-byte alignment of every operand", fn);
    for (int a = 0; a < 5; ++a)
        for (int b = a + 1; b < 5; ++b) {
            if (!ops[a] || !ops[b] || (a == 1 && b == 4 && x == out)) continue;  // out is x itself
            DLS_REQUIRE(!overlap(ops[a], ops[b], P), DLS_EINVAL,
                        "%s: operands overlap (out may be x itself, nothing else)", fn);
        }
    if (P == 0) return DLS_OK;
    hipStream_t st = as_stream(stream);
#define DLS_GO(K_, M_) launch<K_, M_>(agg, x, m, v, out, P, lr, beta1, omb1, beta2, omb2, tau, st)
    switch (kind) {
        case DLS_SERVER_OPT_SGD:
            if (m) DLS_GO(DLS_SERVER_OPT_SGD, true);
            else DLS_GO(DLS_SERVER_OPT_SGD, false);
            break;
        case DLS_SERVER_OPT_ADAGRAD: DLS_GO(DLS_SERVER_OPT_ADAGRAD, true); break;
        case DLS_SERVER_OPT_ADAM: DLS_GO(DLS_SERVER_OPT_ADAM, true); break;
        default: DLS_GO(DLS_SERVER_OPT_YOGI, true); break;
    }
#undef DLS_GO
    return check_launch(fn);
}
