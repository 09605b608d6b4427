// SCAFFOLD control variates and the FedProx proximal term (Karimireddy et al. 2020,
// "SCAFFOLD: stochastic controlled averaging for federated learning"; Li et al. 2020,
// "Federated optimization in heterogeneous networks") for gfx950: three streaming kernels,
// every fp32 operation rounded once and never fused (include/dls_hip.h has the contracts;
// tests/scaffold_ref.py restates them in numpy float32).
//
// k_local_step: the client's optimizer step over up to 32 parameter tensors per launch.
// The segment table {p, g, flat offset, n} and the running count of 256-element tiles are
// kernel arguments, so nothing is uploaded.  A wave owns one tile: it counts the table's
// tile ends at or below its tile number (32 scalar compares on SGPRs, no LDS, no global
// table), reads its segment's four words with scalar loads and steps 4 consecutive elements
// per lane, 16-byte accesses where p, g and the flat offset allow them, one element per
// access otherwise and in a segment's last, partial vector.  Traffic: 12 bytes per element
// (+ 4 each for x and corr where mu != 0 / control is on).  What bounds it on a model of
// many small tensors is the launch count: 2 launches for ResNet-18's 62 tensors.
//
// k_finish: the round-end pass, delta = y - x and c_i updated in place from one read of
// each vector: 16 (12 without control) bytes read and 8 (4) written per coordinate,
// grid-strided 16-byte lanes; the non-finite deltas are counted per lane, summed over the
// wave and the block, and meet in the stream's ticket cell (one integer atomic per block,
// as in drive.hip).
//
// k_server_step: FedAvg's exact chain and SCAFFOLD's control chain over the K client rows
// in one read: (K + 2) * 4P bytes read, 8P written.  The per-client coefficients {n_k, b_k,
// row offset} are staged once per block in LDS (16 KiB at K = 1024) and read back at
// wave-uniform addresses; a lane owns 4 coordinates, carries both chains in registers and
// keeps kRowUnroll non-temporal 16-byte row loads in flight.  HBM-bound like dls_fedavg_f32;
// per row and coordinate it issues FedAvg's multiply, quotient and add plus one multiply and
// one add.
#include <algorithm>
#include <cmath>

#include "rows_common.h"

namespace dls {
namespace {

constexpr int kBlock = 256;
constexpr int kTile = DLS_SCAFFOLD_TILE;       // elements a wave steps: 64 lanes x 4
constexpr int kSegs = DLS_SCAFFOLD_MAX_SEGS;   // segments per launch
constexpr int kMaxBlocks = 2048;               // grid cap of the two flat-vector kernels
constexpr int kRowUnroll = 8;

struct Seg {
    float *p;
    const float *g;
    int64_t off;  // flat index of element 0 (x and corr are indexed by it)
    int64_t n;
};

struct SegTable {
    Seg seg[kSegs];
    int32_t tile_end[kSegs];  // tiles of segments 0..i; unused entries hold the total
};

template <bool WD, bool MU, bool CTRL>
__device__ __forceinline__ float step_one(float p, float g, float x, float c, float lr, float wd,
                                          float mu) {
    float d = g;
    if constexpr (WD) d = d + wd * p;
    if constexpr (MU) d = d + mu * (p - x);
    if constexpr (CTRL) d = d + c;
    return p - lr * d;
}

template <bool WD, bool MU, bool CTRL>
__global__ __launch_bounds__(kBlock) void k_local_step(SegTable tab, int32_t tiles,
                                                       const float *__restrict__ x,
                                                       const float *__restrict__ corr, float lr,
                                                       float wd, float mu) {
    const int lane = __lane_id();
    const int tile = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6)));
    if (tile >= tiles) return;  // wave-uniform
    int s = 0;
#pragma unroll
    for (int i = 0; i < kSegs - 1; ++i) s += tile >= tab.tile_end[i] ? 1 : 0;
    const int first = s == 0 ? 0 : tab.tile_end[s - 1];
    float *p = tab.seg[s].p;
    const float *g = tab.seg[s].g;
    const int64_t off = tab.seg[s].off, n = tab.seg[s].n;
    const float *xs = MU ? x + off : nullptr;
    const float *cs = CTRL ? corr + off : nullptr;
    uintptr_t bits = reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(g);
    if constexpr (MU) bits |= reinterpret_cast<uintptr_t>(xs);
    if constexpr (CTRL) bits |= reinterpret_cast<uintptr_t>(cs);
    const int64_t e0 = (int64_t)(tile - first) * kTile;
    if ((bits & 15u) == 0) {  // wave-uniform: 16-byte lanes
        const int64_t e = e0 + 4 * lane;
        if (e + 4 <= n) {
            f32x4 qp = *reinterpret_cast<const f32x4 *>(p + e);
            const f32x4 qg = *reinterpret_cast<const f32x4 *>(g + e);
            f32x4 qx = f32x4{0.f, 0.f, 0.f, 0.f}, qc = qx;
            if constexpr (MU) qx = *reinterpret_cast<const f32x4 *>(xs + e);
            if constexpr (CTRL) qc = *reinterpret_cast<const f32x4 *>(cs + e);
#pragma unroll
            for (int j = 0; j < 4; ++j) qp[j] = step_one<WD, MU, CTRL>(qp[j], qg[j], qx[j], qc[j], lr, wd, mu);
            *reinterpret_cast<f32x4 *>(p + e) = qp;
        } else {  // the segment's last, partial vector
            for (int64_t i = e; i < n; ++i)
                p[i] = step_one<WD, MU, CTRL>(p[i], g[i], MU ? xs[i] : 0.f, CTRL ? cs[i] : 0.f, lr, wd, mu);
        }
    } else {  // one element per access, consecutive lanes on consecutive elements
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t i = e0 + 64 * j + lane;
            if (i < n)
                p[i] = step_one<WD, MU, CTRL>(p[i], g[i], MU ? xs[i] : 0.f, CTRL ? cs[i] : 0.f, lr, wd, mu);
        }
    }
}

template <bool CTRL>
__global__ __launch_bounds__(kBlock) void k_finish(const f32x4 *__restrict__ y,
                                                   const f32x4 *__restrict__ x,
                                                   const f32x4 *__restrict__ c, f32x4 *ci,
                                                   f32x4 *__restrict__ delta, int64_t P4, float a,
                                                   int32_t *__restrict__ stats,
                                                   unsigned long long *cell) {
    __shared__ uint32_t wbad[kBlock / 64];
    uint32_t bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < P4; i += (int64_t)gridDim.x * kBlock) {
        const f32x4 qy = y[i], qx = x[i];
        f32x4 d, qc, qi;
        if constexpr (CTRL) {
            qc = c[i];
            qi = ci[i];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            d[j] = qy[j] - qx[j];
            bad += (__float_as_uint(d[j]) & 0x7f800000u) == 0x7f800000u ? 1u : 0u;
            if constexpr (CTRL) qi[j] = (qi[j] - qc[j]) - a * d[j];
        }
        delta[i] = d;
        if constexpr (CTRL) ci[i] = qi;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o);
    if ((threadIdx.x & 63) == 0) wbad[threadIdx.x >> 6] = bad;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t nbad = 0;
#pragma unroll
        for (int w = 0; w < kBlock / 64; ++w) nbad += wbad[w];
        const unsigned long long before = atomicAdd(cell, (1ull << 32) | nbad);
        if ((before >> 32) == gridDim.x - 1) {  // every other block's count is in `before`
            stats[0] = (int32_t)((uint32_t)before + nbad);
            atomicExch(cell, 0ull);
        }
    }
}

// fl(fl(x * w) / N), the exact division of DLS_FEDAVG_EXACT (dls_common.h)
__device__ __forceinline__ float avg_term(float x, float w, const FastDiv &d) {
    return div_exact(x * w, d);
}

template <bool CTRL>
__global__ __launch_bounds__(kBlock) void k_server_step(
    const f32x4 *__restrict__ Uv, int64_t ldu4, const int32_t *__restrict__ rows,
    const float *__restrict__ weight, const float *__restrict__ b, int K, FastDiv dv, int64_t P4,
    float eta_g, float f, const f32x4 *x, const f32x4 *c, f32x4 *x_out, f32x4 *c_out) {
    __shared__ int64_t s_row[DLS_SCAFFOLD_MAX_K];
    __shared__ float s_n[DLS_SCAFFOLD_MAX_K];
    __shared__ float s_b[DLS_SCAFFOLD_MAX_K];
    for (int k = threadIdx.x; k < K; k += kBlock) {
        s_row[k] = (int64_t)rows[k] * ldu4;
        s_n[k] = weight[k];
        if constexpr (CTRL) s_b[k] = b[k];
    }
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < P4; i += (int64_t)gridDim.x * kBlock) {
        const f32x4 *col = Uv + i;
        // -0 + t == t for every fp32 t: "the first row assigns, the rest add"
        f32x4 acc = f32x4{-0.f, -0.f, -0.f, -0.f}, s = acc;
        auto consume = [&](f32x4 q, int k) {
            const float nk = s_n[k];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = acc[j] + avg_term(q[j], nk, dv);
            if constexpr (CTRL) {
                const float bk = s_b[k];
#pragma unroll
                for (int j = 0; j < 4; ++j) s[j] = s[j] + bk * q[j];
            }
        };
        int k = 0;
        for (; k + kRowUnroll <= K; k += kRowUnroll) {
            f32x4 q[kRowUnroll];
#pragma unroll
            for (int u = 0; u < kRowUnroll; ++u) q[u] = __builtin_nontemporal_load(col + s_row[k + u]);
#pragma unroll
            for (int u = 0; u < kRowUnroll; ++u) consume(q[u], k + u);
        }
        for (; k < K; ++k) consume(__builtin_nontemporal_load(col + s_row[k]), k);
        const f32x4 qx = x[i];
        f32x4 ox;
#pragma unroll
        for (int j = 0; j < 4; ++j) ox[j] = qx[j] + eta_g * acc[j];
        x_out[i] = ox;
        if constexpr (CTRL) {
            const f32x4 qc = c[i];
            f32x4 oc;
#pragma unroll
            for (int j = 0; j < 4; ++j) oc[j] = (qc[j] - f * qc[j]) - s[j];
            c_out[i] = oc;
        }
    }
}

// [a, a + n) and [b, b + n) floats share a byte
inline bool overlap(const float *a, const float *b, int64_t n) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    const uintptr_t len = (uintptr_t)n * sizeof(float);
    return a0 < b0 + len && b0 < a0 + len;
}

inline unsigned flat_grid(int64_t P4) {
    const int64_t blocks = (P4 + kBlock - 1) / kBlock;
    return (unsigned)(blocks < kMaxBlocks ? blocks : kMaxBlocks);
}

}  // namespace
}  // namespace dls

using namespace dls;

extern "C" int dls_scaffold_local_step_f32(float *const *p, const float *const *g,
                                           const int64_t *off, const int64_t *n, int32_t T,
                                           const float *x, const float *corr, int64_t P, float lr,
                                           float wd, float mu, int32_t control,
                                           dls_stream_t stream) {
    const char *fn = "dls_scaffold_local_step_f32";
    DLS_REQUIRE(p && g && off && n, DLS_EINVAL, "%s: null pointer (p, g, off, n)", fn);
    DLS_REQUIRE(T >= 0 && P >= 0, DLS_EINVAL, "%s: T=%d P=%lld", fn, T, (long long)P);
    DLS_REQUIRE(control == 0 || control == 1, DLS_EINVAL, "%s: control=%d (0 or 1)", fn, control);
    DLS_REQUIRE(std::isfinite(lr) && std::isfinite(wd) && std::isfinite(mu), DLS_EINVAL,
                "%s: non-finite coefficient (lr=%g wd=%g mu=%g)", fn, lr, wd, mu);
    const bool use_x = mu != 0.f, use_c = control != 0;
    DLS_REQUIRE(!use_x || x, DLS_EINVAL, "%s: null pointer (x, mu=%g)", fn, mu);
    DLS_REQUIRE(!use_c || corr, DLS_EINVAL, "%s: null pointer (corr, control=1)", fn);
    DLS_REQUIRE((reinterpret_cast<uintptr_t>(x) & 3u) == 0 && (reinterpret_cast<uintptr_t>(corr) & 3u) == 0,
                DLS_ELAYOUT, "%s: 4-byte alignment of x and corr", fn);
    for (int32_t t = 0; t < T; ++t) {
        DLS_REQUIRE(p[t] && g[t], DLS_EINVAL, "%s: null pointer (segment %d)", fn, t);
        DLS_REQUIRE(n[t] >= 0 && n[t] < ((int64_t)1 << 31) * kTile / kSegs, DLS_EINVAL,
                    "%s: segment %d has n=%lld", fn, t, (long long)n[t]);
        DLS_REQUIRE(!(use_x || use_c) || (off[t] >= 0 && off[t] <= P && n[t] <= P - off[t]), DLS_EINVAL,
                    "%s: segment %d [%lld, %lld + %lld) leaves the flat vector of P=%lld", fn, t,
                    (long long)off[t], (long long)off[t], (long long)n[t], (long long)P);
        DLS_REQUIRE(((reinterpret_cast<uintptr_t>(p[t]) | reinterpret_cast<uintptr_t>(g[t])) & 3u) == 0,
                    DLS_ELAYOUT, "%s: 4-byte alignment of segment %d", fn, t);
        DLS_REQUIRE(!overlap(p[t], g[t], n[t]), DLS_EINVAL, "%s: p and g of segment %d overlap", fn, t);
    }
    hipStream_t st = as_stream(stream);
    int32_t t = 0;
    while (t < T) {  // launches of at most kSegs non-empty segments
        SegTable tab;
        int m = 0;
        int64_t tiles = 0;
        for (; t < T && m < kSegs; ++t) {
            if (n[t] == 0) continue;
            tab.seg[m] = Seg{p[t], g[t], off[t], n[t]};
            tiles += (n[t] + kTile - 1) / kTile;
            tab.tile_end[m++] = (int32_t)tiles;
        }
        if (m == 0) break;
        for (int i = m; i < kSegs; ++i) {
            tab.seg[i] = tab.seg[m - 1];
            tab.tile_end[i] = (int32_t)tiles;
        }
        const dim3 grid((unsigned)((tiles + kBlock / 64 - 1) / (kBlock / 64)));
#define DLS_GO(WD_, MU_, C_)                                                                      \
    hipLaunchKernelGGL((k_local_step<WD_, MU_, C_>), grid, dim3(kBlock), 0, st, tab, (int32_t)tiles, \
                       x, corr, lr, wd, mu)
        switch ((wd != 0.f ? 4 : 0) | (use_x ? 2 : 0) | (use_c ? 1 : 0)) {
            case 0: DLS_GO(false, false, false); break;
            case 1: DLS_GO(false, false, true); break;
            case 2: DLS_GO(false, true, false); break;
            case 3: DLS_GO(false, true, true); break;
            case 4: DLS_GO(true, false, false); break;
            case 5: DLS_GO(true, false, true); break;
            case 6: DLS_GO(true, true, false); break;
            default: DLS_GO(true, true, true); break;
        }
#undef DLS_GO
        const int rc = check_launch(fn);
        if (rc != DLS_OK) return rc;
    }
    return DLS_OK;
}

extern "C" int dls_scaffold_finish_f32(const float *y, const float *x, const float *c, float *ci,
                                       float *delta, int64_t P, float a, int32_t control,
                                       int32_t *stats, dls_stream_t stream) {
    const char *fn = "dls_scaffold_finish_f32";
    DLS_REQUIRE(y && x && delta && stats, DLS_EINVAL, "%s: null pointer (y, x, delta, stats)", fn);
    DLS_REQUIRE(control == 0 || control == 1, DLS_EINVAL, "%s: control=%d (0 or 1)", fn, control);
    DLS_REQUIRE(!control || (c && ci), DLS_EINVAL, "%s: null pointer (c, ci, control=1)", fn);
    DLS_REQUIRE(!control || std::isfinite(a), DLS_EINVAL, "%s: non-finite a=%g", fn, a);
    DLS_REQUIRE(P >= 4 && P % 4 == 0, DLS_EINVAL, "%s: P=%lld must be a positive multiple of 4", fn,
                (long long)P);
    DLS_REQUIRE(aligned16(y) && aligned16(x) && aligned16(delta) && (!control || (aligned16(c) && aligned16(ci))),
                DLS_ELAYOUT, "%s: 16-byte alignment of y, x, c, ci and delta", fn);
    DLS_REQUIRE((reinterpret_cast<uintptr_t>(stats) & 3u) == 0, DLS_ELAYOUT, "%s: 4-byte alignment of stats", fn);
    const float *in[5] = {y, x, control ? c : nullptr, control ? ci : nullptr, delta};
    for (const float *q : in) {
        const uintptr_t q0 = reinterpret_cast<uintptr_t>(q), s0 = reinterpret_cast<uintptr_t>(stats);
        DLS_REQUIRE(!q || ((q == delta || !overlap(delta, q, P)) && (s0 + 4 <= q0 || s0 >= q0 + 4 * (uintptr_t)P)),
                    DLS_EINVAL, "%s: delta and stats must not overlap an input or each other", fn);
    }
    DLS_REQUIRE(!control || (!overlap(ci, y, P) && !overlap(ci, x, P) && !overlap(ci, c, P)), DLS_EINVAL,
                "%s: ci must not overlap y, x or c", fn);
    unsigned long long *cell = stream_cell(as_stream(stream));
    DLS_REQUIRE(cell, DLS_EINVAL, "%s: no device memory for the stream's counter cell", fn);
    const int64_t P4 = P / 4;
    auto go = [&](auto kern) {
        hipLaunchKernelGGL(kern, dim3(flat_grid(P4)), dim3(kBlock), 0, as_stream(stream),
                           reinterpret_cast<const f32x4 *>(y), reinterpret_cast<const f32x4 *>(x),
                           reinterpret_cast<const f32x4 *>(c), reinterpret_cast<f32x4 *>(ci),
                           reinterpret_cast<f32x4 *>(delta), P4, a, stats, cell);
    };
    if (control) go(k_finish<true>);
    else go(k_finish<false>);
    return check_launch(fn);
}

extern "C" int dls_scaffold_server_step_f32(const float *U, int64_t ldu, const int32_t *rows,
                                            const float *weight, const float *b, int32_t K,
                                            float total, int64_t P, float eta_g, float f,
                                            const float *x, const float *c, float *x_out,
                                            float *c_out, int32_t control, dls_stream_t stream) {
    const char *fn = "dls_scaffold_server_step_f32";
    DLS_REQUIRE(U && rows && weight && x && x_out, DLS_EINVAL, "%s: null pointer", fn);
    DLS_REQUIRE(control == 0 || control == 1, DLS_EINVAL, "%s: control=%d (0 or 1)", fn, control);
    DLS_REQUIRE(!control || (b && c && c_out), DLS_EINVAL, "%s: null pointer (b, c, c_out, control=1)", fn);
    DLS_REQUIRE(K >= 1 && K <= DLS_SCAFFOLD_MAX_K, DLS_EINVAL, "%s: K=%d (1..DLS_SCAFFOLD_MAX_K=%d)", fn, K,
                DLS_SCAFFOLD_MAX_K);
    DLS_REQUIRE(std::isfinite(eta_g) && std::isfinite(f) && total > 0.f && std::isfinite(total), DLS_EINVAL,
                "%s: eta_g=%g and f=%g must be finite, total=%g finite and positive", fn, eta_g, f, total);
    const bool aligned = aligned16(U) && aligned16(x) && aligned16(x_out) &&
                         (!control || (aligned16(c) && aligned16(c_out)));
    const int rc = check_layout(fn, ldu, P, aligned, " (U, x, c, x_out, c_out)");
    if (rc != DLS_OK) return rc;
    // an output is its own input or disjoint from every vector (the rows are checked by the caller)
    const float *vec[4] = {x, control ? c : nullptr, x_out, control ? c_out : nullptr};
    for (int i = 0; i < 4; ++i)
        for (int j = std::max(i + 1, 2); j < 4; ++j) {
            if (!vec[i] || !vec[j] || (j == i + 2 && vec[i] == vec[j])) continue;
            DLS_REQUIRE(!overlap(vec[i], vec[j], P), DLS_EINVAL,
                        "%s: operands overlap (x_out may be x itself and c_out c itself, nothing else)", fn);
        }
    if (P == 0) return DLS_OK;
    const FastDiv dv = make_fastdiv(total);
    const int64_t P4 = P / 4;
    auto go = [&](auto kern) {
        const int64_t resident = resident_blocks(reinterpret_cast<const void *>(kern), kBlock, 0);
        const int64_t blocks = (P4 + kBlock - 1) / kBlock;
        hipLaunchKernelGGL(kern, dim3((unsigned)std::max<int64_t>(1, std::min(blocks, resident))), dim3(kBlock), 0,
                           as_stream(stream), reinterpret_cast<const f32x4 *>(U), ldu / 4, rows, weight, b,
                           (int)K, dv, P4, eta_g, f, reinterpret_cast<const f32x4 *>(x),
                           reinterpret_cast<const f32x4 *>(c), reinterpret_cast<f32x4 *>(x_out),
                           reinterpret_cast<f32x4 *>(c_out));
    };
    if (control) go(k_server_step<true>);
    else go(k_server_step<false>);
    return check_launch(fn);
}
