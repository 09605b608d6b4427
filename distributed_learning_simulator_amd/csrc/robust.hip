// Coordinate-wise trimmed mean / median, the mean around the median (second part of
// this file) and the crafted Byzantine rows they are measured against (third part),
// over K client rows for gfx950: the robust counterparts of the FedAvg hook
// (servers/fed_server.py:44-66).
//
// Per flat coordinate, independently (include/dls_hip.h has the contract):
//   sort the K values ascending (-0 below +0, every NaN above +inf), drop the
//   `trim` lowest and highest, acc = v[trim]; acc = fl(acc + v[i]) ascending;
//   out = fl(acc / fl32(m)), m = K - 2 trim; any NaN result is 0x7fc00000.
// The result is a function of the column's multiset: the same bits for any
// order of `rows`.
//
// One pass over the rows, FedAvg's traffic (K*P*4 read, P*4 written): a lane owns
// 4 consecutive coordinates (one 16-byte load per row), the row indices reach the
// wave through a per-lane table and v_readlane, and a lane's K x 4 values are
// sorted in registers as order-preserving uint32 keys by a fully unrolled Batcher
// odd-even merge network (v_min_u32 / v_max_u32 per comparator and coordinate),
// instantiated for KP = 1, 2, 4, ..., 64 wires; wires K..KP-1 hold the top key.
// Every register index is a compile-time constant (no scratch, no LDS), and one
// lane produces each output (no atomics, no split reduction).
#include <cmath>
#include <utility>

#include "dls_common.h"

namespace dls {
namespace {

constexpr int kRobustBlock = 256;
constexpr uint32_t kTopKey = 0xffffffffu;  // the canonical NaN's key; pads wires >= K

// ------------------------------------------------- the comparator network
// Batcher's odd-even merge sort of N = 2^t wires as a compile-time list of
// (a < b) comparators: 1, 3, 9, 25, 63 (N = 16), 191, 543 (N = 64) of them.
struct Cmp {
    unsigned char a, b;
};

template <typename F>
constexpr void batcher(int n, F &&f) {
    for (int p = 1; p < n; p *= 2)
        for (int k = p; k >= 1; k /= 2)
            for (int j = k % p; j + k < n; j += 2 * k)
                for (int i = 0; i < k && i + j + k < n; ++i)
                    if ((i + j) / (2 * p) == (i + j + k) / (2 * p)) f(i + j, i + j + k);
}

template <int N>
constexpr int net_count() {
    int c = 0;
    batcher(N, [&](int, int) { ++c; });
    return c;
}

template <int N>
struct NetTab {
    Cmp c[net_count<N>() + 1];
};

template <int N>
constexpr NetTab<N> make_net() {
    NetTab<N> t{};
    int c = 0;
    batcher(N, [&](int a, int b) {
        t.c[c].a = (unsigned char)a;
        t.c[c].b = (unsigned char)b;
        ++c;
    });
    return t;
}

template <int N>
struct Net {
    static constexpr int count = net_count<N>();
    static constexpr NetTab<N> tab = make_net<N>();
};

// W coordinates' keys go through the network side by side: v[w][wire]
template <int N, int W, int I>
__device__ __forceinline__ void net_step(uint32_t (&v)[W][N]) {
    if constexpr (I < Net<N>::count) {
        constexpr int a = Net<N>::tab.c[I].a, b = Net<N>::tab.c[I].b;
        static_assert(a < b && b < N, "comparator wires");
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const uint32_t lo = min(v[w][a], v[w][b]);
            v[w][b] = max(v[w][a], v[w][b]);
            v[w][a] = lo;
        }
    }
}

template <int N, int W, int I0, int... Is>
__device__ __forceinline__ void net_chunk(uint32_t (&v)[W][N], std::integer_sequence<int, Is...>) {
    (net_step<N, W, I0 + Is>(v), ...);
}

// comparators I0, I0 + 1, ... in chunks of 32 (a fold over all 543 would pass the
// compiler's expression nesting limit)
template <int N, int W, int I0 = 0>
__device__ __forceinline__ void net_sort(uint32_t (&v)[W][N]) {
    if constexpr (I0 < Net<N>::count) {
        net_chunk<N, W, I0>(v, std::make_integer_sequence<int, 32>{});
        net_sort<N, W, I0 + 32>(v);
    }
}

// ------------------------------------------------------------------- keys
// fp32 bits -> uint32 whose unsigned order is the contract's total order: the
// sign-flip map (negative: all bits inverted; else the sign bit set), every NaN
// on the top key.
__device__ __forceinline__ uint32_t to_key(uint32_t u) {
    const uint32_t k = u ^ ((uint32_t)((int32_t)u >> 31) | 0x80000000u);
    return (u & 0x7fffffffu) > 0x7f800000u ? kTopKey : k;
}

__device__ __forceinline__ float from_key(uint32_t k) {
    return __uint_as_float(k ^ ((uint32_t)((int32_t)~k >> 31) | 0x80000000u));
}

__device__ __forceinline__ float quiet(float x) {
    return (__float_as_uint(x) & 0x7fffffffu) > 0x7f800000u ? __uint_as_float(0x7fc00000u) : x;
}

// ----------------------------------------------------------------- kernel
// Coordinates C0 .. C0 + W - 1 of the lane's four: keys, network, trim, sum, division.
template <int KP, int W, int C0>
__device__ __forceinline__ void reduce_coords(const f32x4 (&x)[KP], int K, int trim, f32x4 &res) {
    uint32_t v[W][KP];
#pragma unroll
    for (int j = 0; j < KP; ++j)
#pragma unroll
        for (int w = 0; w < W; ++w)
            v[w][j] = j < K ? to_key(__float_as_uint(x[j][C0 + w])) : kTopKey;  // wave-uniform
    net_sort<KP, W>(v);
    // -0 + t == t for every fp32 t (-0 and NaN included), so starting from -0
    // makes v[trim] the first term with its own bits, and m == 1 adds nothing else
    const int lo = trim, hi = K - 1 - trim;
    float acc[W];
#pragma unroll
    for (int w = 0; w < W; ++w) acc[w] = -0.f;
#pragma unroll
    for (int j = 0; j < KP; ++j) {
        const bool kept = j >= lo && j <= hi;  // wave-uniform; t + -0 == t as well
#pragma unroll
        for (int w = 0; w < W; ++w) acc[w] = acc[w] + (kept ? from_key(v[w][j]) : -0.f);
    }
    const int m = hi - lo + 1;
    if (m > 1) {
        const float fm = (float)m;
#pragma unroll
        for (int w = 0; w < W; ++w) acc[w] = div_ieee(acc[w], fm);
    }
#pragma unroll
    for (int w = 0; w < W; ++w) res[C0 + w] = quiet(acc[w]);
}

// KP wires (a power of two >= K); W of the lane's 4 coordinates are sorted at a
// time (KP = 64: two at a time, so that the 256 loaded values and the 128 keys in
// work fit the register file without scratch).  All KP loads are unconditional and
// issued together: lane j >= K of the row table holds the last row, so a wire
// past K re-reads that row's 16 bytes (a cache hit) and its key is replaced by
// the top key; no branch touches a load or an element of the register arrays.
template <int KP, int W>
__global__ __launch_bounds__(kRobustBlock) void k_trimmed_mean(const f32x4 *__restrict__ Uv,
                                                               int64_t ldu4,
                                                               const int32_t *__restrict__ rows,
                                                               int K, int trim, int64_t P4,
                                                               f32x4 *__restrict__ out) {
    const int lane = __lane_id();
    const int64_t i0 = ((int64_t)blockIdx.x * (kRobustBlock / 64) + (threadIdx.x >> 6)) * 64 + lane;
    const int64_t iq = i0 < P4 ? i0 : P4 - 1;  // every lane stays: the table needs all 64
    const int tr = rows[min(lane, K - 1)];
    f32x4 x[KP];
#pragma unroll
    for (int j = 0; j < KP; ++j) {
        const int64_t r = __builtin_amdgcn_readlane(tr, j);
        x[j] = __builtin_nontemporal_load(Uv + r * ldu4 + iq);
    }
    f32x4 res;
    if constexpr (W == 4) {
        reduce_coords<KP, 4, 0>(x, K, trim, res);
    } else {
        static_assert(W == 2, "coordinates per pass");
        reduce_coords<KP, 2, 0>(x, K, trim, res);
        __builtin_amdgcn_sched_barrier(0);  // one pass's keys in registers at a time
        reduce_coords<KP, 2, 2>(x, K, trim, res);
    }
    if (i0 < P4) out[i0] = res;
}

template <int KP, int W = 4>
void launch(const float *U, int64_t ldu, const int32_t *rows, int K, int trim, int64_t P4,
            float *out, hipStream_t st) {
    const dim3 grid((unsigned)((P4 + kRobustBlock - 1) / kRobustBlock));
    hipLaunchKernelGGL((k_trimmed_mean<KP, W>), grid, dim3(kRobustBlock), 0, st,
                       reinterpret_cast<const f32x4 *>(U), ldu / 4, rows, K, trim, P4,
                       reinterpret_cast<f32x4 *>(out));
}

// ------------------------------------------- mean around the median (MeaMed)
// dls_mean_around_median_f32: the `keep` consecutive sorted values closest to the
// median, summed ascending.  Same loads, keys and network as k_trimmed_mean; after
// the network, per coordinate:
//   f[j]  = the sorted values (wires >= K decode to a NaN);
//   med   = f[(K-1)/2], or fl(fl(f[K/2-1] + f[K/2]) / 2) for an even K, picked by
//           wave-uniform selects over the wires that can hold it (j <= KP/2);
//   h[i]  = f[i + keep], a NaN past the last wire: `keep` is wave-uniform, so the
//           array is moved down by its set bits, one power of two per stage, every
//           stage a select between two compile-time wires;
//   s     = the number of wires with fl(med - f[i]) > fl(h[i] - med).  The true
//           comparisons are a prefix of i = 0, 1, ... (both sides are monotone in
//           i and the NaNs sit on top, where every comparison is false), so the
//           count is the first false index, and a wire i >= K - keep compares
//           with a NaN and never counts;
//   sum   = the ascending sum of k_trimmed_mean with kept = s <= j < s + keep, a
//           per-lane select (each of the lane's coordinates has its own s).
template <int KP>
constexpr int shift_stages() {
    int n = 0;
    while ((1 << n) <= KP) ++n;  // keep <= KP: bits 0 .. log2(KP)
    return n;
}

template <int KP, int W, int C0>
__device__ __forceinline__ void window_coords(const f32x4 (&x)[KP], int K, int keep, f32x4 &res) {
    uint32_t v[W][KP];
#pragma unroll
    for (int j = 0; j < KP; ++j)
#pragma unroll
        for (int w = 0; w < W; ++w)
            v[w][j] = j < K ? to_key(__float_as_uint(x[j][C0 + w])) : kTopKey;  // wave-uniform
    net_sort<KP, W>(v);
    float f[W][KP], h[W][KP];
#pragma unroll
    for (int j = 0; j < KP; ++j)
#pragma unroll
        for (int w = 0; w < W; ++w) h[w][j] = f[w][j] = from_key(v[w][j]);
    // K > KP / 2 for KP >= 2, so the middle wires are among 0 .. KP/2
    const int mlo = (K - 1) >> 1, mhi = K >> 1;
    constexpr int kMid = KP > 1 ? KP / 2 : 0;
    float med[W];
#pragma unroll
    for (int w = 0; w < W; ++w) {
        float lo = f[w][0], hi = f[w][0];
#pragma unroll
        for (int j = 1; j <= kMid; ++j) {
            lo = j == mlo ? f[w][j] : lo;  // wave-uniform
            hi = j == mhi ? f[w][j] : hi;
        }
        med[w] = mlo == mhi ? lo : div_ieee(lo + hi, 2.f);
    }
    const float nan = __uint_as_float(0x7fc00000u);
#pragma unroll
    for (int b = 0; b < shift_stages<KP>(); ++b) {
        const bool on = (keep >> b) & 1;  // wave-uniform
#pragma unroll
        for (int i = 0; i < KP; ++i)  // ascending: wire i + 2^b is still this stage's input
#pragma unroll
            for (int w = 0; w < W; ++w) {
                const int src = i + (1 << b);
                const float moved = src < KP ? h[w][src < KP ? src : i] : nan;
                h[w][i] = on ? moved : h[w][i];
            }
    }
    int s[W];
#pragma unroll
    for (int w = 0; w < W; ++w) s[w] = 0;
#pragma unroll
    for (int i = 0; i + 1 < KP; ++i)  // h[KP - 1] is a NaN for every keep >= 1
#pragma unroll
        for (int w = 0; w < W; ++w) s[w] += (med[w] - f[w][i]) > (h[w][i] - med[w]) ? 1 : 0;
    float acc[W];
#pragma unroll
    for (int w = 0; w < W; ++w) acc[w] = -0.f;
#pragma unroll
    for (int j = 0; j < KP; ++j)
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const bool kept = (uint32_t)(j - s[w]) < (uint32_t)keep;  // s <= j < s + keep
            acc[w] = acc[w] + (kept ? f[w][j] : -0.f);
        }
    if (keep > 1) {
        const float fk = (float)keep;
#pragma unroll
        for (int w = 0; w < W; ++w) acc[w] = div_ieee(acc[w], fk);
    }
#pragma unroll
    for (int w = 0; w < W; ++w) res[C0 + w] = quiet(acc[w]);
}

// The loads of k_trimmed_mean; W of the lane's 4 coordinates go through the network
// and the window at a time.  KP = 64 takes one at a time: beside the parked loads a
// pass holds the sorted values and their moved copy, and two coordinates per pass
// spilled 60 bytes per lane to scratch.
template <int KP, int W>
__global__ __launch_bounds__(kRobustBlock) void k_mean_around_median(
    const f32x4 *__restrict__ Uv, int64_t ldu4, const int32_t *__restrict__ rows, int K, int keep,
    int64_t P4, f32x4 *__restrict__ out) {
    const int lane = __lane_id();
    const int64_t i0 = ((int64_t)blockIdx.x * (kRobustBlock / 64) + (threadIdx.x >> 6)) * 64 + lane;
    const int64_t iq = i0 < P4 ? i0 : P4 - 1;  // every lane stays: the table needs all 64
    const int tr = rows[min(lane, K - 1)];
    f32x4 x[KP];
#pragma unroll
    for (int j = 0; j < KP; ++j) {
        const int64_t r = __builtin_amdgcn_readlane(tr, j);
        x[j] = __builtin_nontemporal_load(Uv + r * ldu4 + iq);
    }
    f32x4 res;
    if constexpr (W == 4) {
        window_coords<KP, 4, 0>(x, K, keep, res);
    } else if constexpr (W == 2) {
        window_coords<KP, 2, 0>(x, K, keep, res);
        __builtin_amdgcn_sched_barrier(0);  // one pass's keys in registers at a time
        window_coords<KP, 2, 2>(x, K, keep, res);
    } else {
        static_assert(W == 1, "coordinates per pass");
        window_coords<KP, 1, 0>(x, K, keep, res);
        __builtin_amdgcn_sched_barrier(0);
        window_coords<KP, 1, 1>(x, K, keep, res);
        __builtin_amdgcn_sched_barrier(0);
        window_coords<KP, 1, 2>(x, K, keep, res);
        __builtin_amdgcn_sched_barrier(0);
        window_coords<KP, 1, 3>(x, K, keep, res);
    }
    if (i0 < P4) out[i0] = res;
}

template <int KP, int W = 4>
void launch_window(const float *U, int64_t ldu, const int32_t *rows, int K, int keep, int64_t P4,
                   float *out, hipStream_t st) {
    const dim3 grid((unsigned)((P4 + kRobustBlock - 1) / kRobustBlock));
    hipLaunchKernelGGL((k_mean_around_median<KP, W>), grid, dim3(kRobustBlock), 0, st,
                       reinterpret_cast<const f32x4 *>(U), ldu / 4, rows, K, keep, P4,
                       reinterpret_cast<f32x4 *>(out));
}

// ------------------------------------------- crafted Byzantine rows (ALIE, IPM)
// dls_craft_rows_f32: out = base + a * (mu - base) + b * sigma per coordinate, mu and
// sigma the ascending mean and the population standard deviation of the Kh honest
// values, written into every attacker row.  Same loads, keys and network as
// k_trimmed_mean.  The sorted keys stay in registers and are decoded twice: once for
// the ascending sum, and, when b != 0 (wave-uniform), once more for the deviations
//   d = fl(v[j] - mu); s = fmaf(d, d, s),
// where a wire >= Kh (a NaN) is masked out by a wave-uniform select.  Nothing beside
// that fmaf is contracted (the library is built with -ffp-contract=off).
template <int KP, int W, int C0>
__device__ __forceinline__ void craft_coords(const f32x4 (&x)[KP], int K, float a, float b,
                                             bool has_base, const f32x4 &bs, f32x4 &res) {
    uint32_t v[W][KP];
#pragma unroll
    for (int j = 0; j < KP; ++j)
#pragma unroll
        for (int w = 0; w < W; ++w)
            v[w][j] = j < K ? to_key(__float_as_uint(x[j][C0 + w])) : kTopKey;  // wave-uniform
    net_sort<KP, W>(v);
    // the sum of reduce_coords with trim 0: from -0, so that v[0] keeps its own bits
    float mu[W], sg[W];
#pragma unroll
    for (int w = 0; w < W; ++w) mu[w] = -0.f;
#pragma unroll
    for (int j = 0; j < KP; ++j) {
        const bool kept = j < K;  // wave-uniform; t + -0 == t
#pragma unroll
        for (int w = 0; w < W; ++w) mu[w] = mu[w] + (kept ? from_key(v[w][j]) : -0.f);
    }
    const float fk = (float)K;
    if (K > 1) {
#pragma unroll
        for (int w = 0; w < W; ++w) mu[w] = div_ieee(mu[w], fk);
    }
    const bool use_b = b != 0.f;  // wave-uniform
#pragma unroll
    for (int w = 0; w < W; ++w) sg[w] = 0.f;
    if (use_b) {
        float s[W];
#pragma unroll
        for (int w = 0; w < W; ++w) s[w] = 0.f;
#pragma unroll
        for (int j = 0; j < KP; ++j) {
            const bool kept = j < K;
#pragma unroll
            for (int w = 0; w < W; ++w) {
                const float d = from_key(v[w][j]) - mu[w];
                const float q = __builtin_fmaf(d, d, s[w]);
                s[w] = kept ? q : s[w];
            }
        }
        if (K > 1) {
#pragma unroll
            for (int w = 0; w < W; ++w) s[w] = div_ieee(s[w], fk);
        }
#pragma unroll
        for (int w = 0; w < W; ++w) sg[w] = sqrt_ieee(s[w]);
    }
#pragma unroll
    for (int w = 0; w < W; ++w) {
        const float z = bs[C0 + w];
        const float t = has_base ? mu[w] - z : mu[w];
        float r = a * t;
        const float e = b * sg[w];
        r = use_b ? r + e : r;
        res[C0 + w] = quiet(has_base ? z + r : r);
    }
}

// The loads of k_trimmed_mean over the honest rows; the attacker rows reach the wave
// the same way (a per-lane table and v_readlane) and take one 16-byte store each.
template <int KP, int W>
__global__ __launch_bounds__(kRobustBlock) void k_craft_rows(
    f32x4 *Uv, int64_t ldu4, const int32_t *__restrict__ hrows, int K,
    const int32_t *__restrict__ arows, int Ka, float a, float b, const f32x4 *base, int64_t P4) {
    const int lane = __lane_id();
    const int64_t i0 = ((int64_t)blockIdx.x * (kRobustBlock / 64) + (threadIdx.x >> 6)) * 64 + lane;
    const int64_t iq = i0 < P4 ? i0 : P4 - 1;  // every lane stays: the tables need all 64
    const int tr = hrows[min(lane, K - 1)];
    const int ta = arows[min(lane, Ka - 1)];
    f32x4 x[KP];
#pragma unroll
    for (int j = 0; j < KP; ++j) {
        const int64_t r = __builtin_amdgcn_readlane(tr, j);
        x[j] = __builtin_nontemporal_load(Uv + r * ldu4 + iq);
    }
    const bool has_base = base != nullptr;  // wave-uniform
    f32x4 bs = {0.f, 0.f, 0.f, 0.f};
    if (has_base) bs = base[iq];
    f32x4 res;
    if constexpr (W == 4) {
        craft_coords<KP, 4, 0>(x, K, a, b, has_base, bs, res);
    } else if constexpr (W == 2) {
        craft_coords<KP, 2, 0>(x, K, a, b, has_base, bs, res);
        __builtin_amdgcn_sched_barrier(0);  // one pass's keys in registers at a time
        craft_coords<KP, 2, 2>(x, K, a, b, has_base, bs, res);
    } else {
        static_assert(W == 1, "coordinates per pass");
        craft_coords<KP, 1, 0>(x, K, a, b, has_base, bs, res);
        __builtin_amdgcn_sched_barrier(0);
        craft_coords<KP, 1, 1>(x, K, a, b, has_base, bs, res);
        __builtin_amdgcn_sched_barrier(0);
        craft_coords<KP, 1, 2>(x, K, a, b, has_base, bs, res);
        __builtin_amdgcn_sched_barrier(0);
        craft_coords<KP, 1, 3>(x, K, a, b, has_base, bs, res);
    }
    for (int j = 0; j < Ka; ++j) {  // wave-uniform trip count and row
        const int64_t r = __builtin_amdgcn_readlane(ta, j);
        if (i0 < P4) Uv[r * ldu4 + i0] = res;
    }
}

template <int KP, int W = 4>
void launch_craft(float *U, int64_t ldu, const int32_t *hrows, int K, const int32_t *arows, int Ka,
                  float a, float b, const float *base, int64_t P4, hipStream_t st) {
    const dim3 grid((unsigned)((P4 + kRobustBlock - 1) / kRobustBlock));
    hipLaunchKernelGGL((k_craft_rows<KP, W>), grid, dim3(kRobustBlock), 0, st,
                       reinterpret_cast<f32x4 *>(U), ldu / 4, hrows, K, arows, Ka, a, b,
                       reinterpret_cast<const f32x4 *>(base), P4);
}

}  // namespace
}  // namespace dls

using namespace dls;

extern "C" int dls_trimmed_mean_f32(const float *U, int64_t ldu, const int32_t *rows, int32_t K,
                                    int32_t trim, int64_t P, float *out, dls_stream_t stream) {
    DLS_REQUIRE(U && rows && out, DLS_EINVAL, "dls_trimmed_mean_f32: null pointer");
    DLS_REQUIRE(K >= 1 && K <= DLS_ROBUST_MAX_K, DLS_EINVAL,
                "dls_trimmed_mean_f32: K=%d (1..DLS_ROBUST_MAX_K=%d)", K, DLS_ROBUST_MAX_K);
    DLS_REQUIRE(trim >= 0 && 2 * (int64_t)trim < K, DLS_EINVAL,
                "dls_trimmed_mean_f32: trim=%d (0 <= 2*trim < K=%d)", trim, K);
    DLS_REQUIRE(P >= 0, DLS_EINVAL, "dls_trimmed_mean_f32: P=%lld", (long long)P);
    DLS_REQUIRE(P % 4 == 0 && ldu % 4 == 0 && ldu >= P, DLS_ELAYOUT,
                "dls_trimmed_mean_f32: P=%lld and ldu=%lld must be multiples of 4, ldu >= P",
                (long long)P, (long long)ldu);
    DLS_REQUIRE(aligned16(U) && aligned16(out), DLS_ELAYOUT,
                "dls_trimmed_mean_f32: 16-byte alignment");
    if (P == 0) return DLS_OK;
    const int64_t P4 = P / 4;
    DLS_REQUIRE((P4 + kRobustBlock - 1) / kRobustBlock < (int64_t)1 << 31, DLS_EINVAL,
                "dls_trimmed_mean_f32: grid too large");
    hipStream_t st = as_stream(stream);
    if (K == 1)
        launch<1>(U, ldu, rows, K, trim, P4, out, st);
    else if (K == 2)
        launch<2>(U, ldu, rows, K, trim, P4, out, st);
    else if (K <= 4)
        launch<4>(U, ldu, rows, K, trim, P4, out, st);
    else if (K <= 8)
        launch<8>(U, ldu, rows, K, trim, P4, out, st);
    else if (K <= 16)
        launch<16>(U, ldu, rows, K, trim, P4, out, st);
    else if (K <= 32)
        launch<32>(U, ldu, rows, K, trim, P4, out, st);
    else
        launch<64, 2>(U, ldu, rows, K, trim, P4, out, st);
    return check_launch("dls_trimmed_mean_f32");
}

extern "C" int dls_mean_around_median_f32(const float *U, int64_t ldu, const int32_t *rows,
                                          int32_t K, int32_t keep, int64_t P, float *out,
                                          dls_stream_t stream) {
    DLS_REQUIRE(U && rows && out, DLS_EINVAL, "dls_mean_around_median_f32: null pointer");
    DLS_REQUIRE(K >= 1 && K <= DLS_ROBUST_MAX_K, DLS_EINVAL,
                "dls_mean_around_median_f32: K=%d (1..DLS_ROBUST_MAX_K=%d)", K, DLS_ROBUST_MAX_K);
    DLS_REQUIRE(keep >= 1 && keep <= K, DLS_EINVAL,
                "dls_mean_around_median_f32: keep=%d (1 <= keep <= K=%d)", keep, K);
    DLS_REQUIRE(P >= 0, DLS_EINVAL, "dls_mean_around_median_f32: P=%lld", (long long)P);
    DLS_REQUIRE(P % 4 == 0 && ldu % 4 == 0 && ldu >= P, DLS_ELAYOUT,
                "dls_mean_around_median_f32: P=%lld and ldu=%lld must be multiples of 4, ldu >= P",
                (long long)P, (long long)ldu);
    DLS_REQUIRE(aligned16(U) && aligned16(out), DLS_ELAYOUT,
                "dls_mean_around_median_f32: 16-byte alignment");
    if (P == 0) return DLS_OK;
    const int64_t P4 = P / 4;
    DLS_REQUIRE((P4 + kRobustBlock - 1) / kRobustBlock < (int64_t)1 << 31, DLS_EINVAL,
                "dls_mean_around_median_f32: grid too large");
    hipStream_t st = as_stream(stream);
    if (K == 1)
        launch_window<1>(U, ldu, rows, K, keep, P4, out, st);
    else if (K == 2)
        launch_window<2>(U, ldu, rows, K, keep, P4, out, st);
    else if (K <= 4)
        launch_window<4>(U, ldu, rows, K, keep, P4, out, st);
    else if (K <= 8)
        launch_window<8>(U, ldu, rows, K, keep, P4, out, st);
    else if (K <= 16)
        launch_window<16>(U, ldu, rows, K, keep, P4, out, st);
    else if (K <= 32)
        launch_window<32>(U, ldu, rows, K, keep, P4, out, st);
    else
        launch_window<64, 1>(U, ldu, rows, K, keep, P4, out, st);
    return check_launch("dls_mean_around_median_f32");
}

extern "C" int dls_craft_rows_f32(float *U, int64_t ldu, const int32_t *hrows, int32_t Kh,
                                  const int32_t *arows, int32_t Ka, float a, float b,
                                  const float *base, int64_t P, dls_stream_t stream) {
    DLS_REQUIRE(U && hrows && arows, DLS_EINVAL, "dls_craft_rows_f32: null pointer");
    DLS_REQUIRE(Kh >= 1 && Kh <= DLS_ROBUST_MAX_K, DLS_EINVAL,
                "dls_craft_rows_f32: Kh=%d (1..DLS_ROBUST_MAX_K=%d)", Kh, DLS_ROBUST_MAX_K);
    DLS_REQUIRE(Ka >= 1 && Ka <= DLS_ROBUST_MAX_K, DLS_EINVAL,
                "dls_craft_rows_f32: Ka=%d (1..DLS_ROBUST_MAX_K=%d)", Ka, DLS_ROBUST_MAX_K);
    DLS_REQUIRE(std::isfinite(a) && std::isfinite(b), DLS_EINVAL,
                "dls_craft_rows_f32: a=%g and b=%g must be finite", (double)a, (double)b);
    DLS_REQUIRE(P >= 0, DLS_EINVAL, "dls_craft_rows_f32: P=%lld", (long long)P);
    DLS_REQUIRE(P % 4 == 0 && ldu % 4 == 0 && ldu >= P, DLS_ELAYOUT,
                "dls_craft_rows_f32: P=%lld and ldu=%lld must be multiples of 4, ldu >= P",
                (long long)P, (long long)ldu);
    DLS_REQUIRE(aligned16(U) && aligned16(base), DLS_ELAYOUT,
                "dls_craft_rows_f32: 16-byte alignment");
    if (P == 0) return DLS_OK;
    const int64_t P4 = P / 4;
    DLS_REQUIRE((P4 + kRobustBlock - 1) / kRobustBlock < (int64_t)1 << 31, DLS_EINVAL,
                "dls_craft_rows_f32: grid too large");
    hipStream_t st = as_stream(stream);
    if (Kh == 1)
        launch_craft<1>(U, ldu, hrows, Kh, arows, Ka, a, b, base, P4, st);
    else if (Kh == 2)
        launch_craft<2>(U, ldu, hrows, Kh, arows, Ka, a, b, base, P4, st);
    else if (Kh <= 4)
        launch_craft<4>(U, ldu, hrows, Kh, arows, Ka, a, b, base, P4, st);
    else if (Kh <= 8)
        launch_craft<8>(U, ldu, hrows, Kh, arows, Ka, a, b, base, P4, st);
    else if (Kh <= 16)
        launch_craft<16>(U, ldu, hrows, Kh, arows, Ka, a, b, base, P4, st);
    else if (Kh <= 32)
        launch_craft<32>(U, ldu, hrows, Kh, arows, Ka, a, b, base, P4, st);
    else
        launch_craft<64, 2>(U, ldu, hrows, Kh, arows, Ka, a, b, base, P4, st);
    return check_launch("dls_craft_rows_f32");
}
