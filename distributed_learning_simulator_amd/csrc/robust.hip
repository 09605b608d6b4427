// Coordinate-wise rules over the sorted column of K client rows for gfx950: the
// trimmed mean / median, the mean around the median and the crafted Byzantine rows
// they are measured against, the robust counterparts of the FedAvg hook
// (servers/fed_server.py:44-66).  include/dls_hip.h has each rule's contract.
//
// One skeleton (k_sorted_columns and the helpers before it), written once:
//   load     a lane owns 4 consecutive coordinates (one 16-byte load per row), the
//            row indices reach the wave through a per-lane table and v_readlane;
//            one pass over the rows, FedAvg's traffic (K*P*4 read);
//   sort     a lane's K x 4 values become order-preserving uint32 keys (-0 below
//            +0, every NaN above +inf) and are sorted in registers by a fully
//            unrolled Batcher odd-even merge network (v_min_u32 / v_max_u32 per
//            comparator and coordinate), instantiated for KP = 1, 2, 4, ..., 64
//            wires; wires K..KP-1 hold the top key;
//   passes   W of the lane's 4 coordinates go through sort and rule at a time.
// Each rule keeps its own ascending sum from -0 (a shared one with a kept(j, w)
// functor cost the trimmed mean at KP = 16 two of its seven waves per SIMD).
// A rule (the last part of this file) is a small struct of its scalar parameters
// with the per-coordinate body after the sort and the output step.  Every register
// index is a compile-time constant (no scratch, no LDS), one lane produces each
// output (no atomics, no split reduction), and the result is a function of the
// column's multiset: the same bits for any order of the rows.
#include <cmath>
#include <utility>

#include "rows_common.h"

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

// ------------------------------------------------------------ the skeleton
// The lane's columns: x[j] = the lane's 4 coordinates of row rows[j], KP wires (a
// power of two >= K).  All KP loads are unconditional and issued together: lane
// j >= K of the row table holds the last row, so a wire past K re-reads that row's
// 16 bytes (a cache hit) and its key is replaced by the top key; no branch touches a
// load or an element of the register arrays.
struct Place {
    int64_t i0;  // the lane's index into the P4 vectors of a row
    int64_t iq;  // i0 clamped into the row
};

template <int KP>
__device__ __forceinline__ Place load_columns(const f32x4 *Uv, int64_t ldu4, const int32_t *rows,
                                              int K, int64_t P4, f32x4 (&x)[KP]) {
    const int lane = __lane_id();
    const int64_t i0 = ((int64_t)blockIdx.x * (kRobustBlock / 64) + (threadIdx.x >> 6)) * 64 + lane;
    const int64_t iq = i0 < P4 ? i0 : P4 - 1;  // every lane stays: the table needs all 64
    const int tr = rows[min(lane, K - 1)];
#pragma unroll
    for (int j = 0; j < KP; ++j) {
        const int64_t r = __builtin_amdgcn_readlane(tr, j);
        x[j] = __builtin_nontemporal_load(Uv + r * ldu4 + iq);
    }
    return {i0, iq};
}

// The sorted keys of coordinates C0 .. C0 + W - 1 of the lane's four.
template <int KP, int W, int C0>
__device__ __forceinline__ void sorted_keys(const f32x4 (&x)[KP], int K, uint32_t (&v)[W][KP]) {
#pragma unroll
    for (int j = 0; j < KP; ++j)
#pragma unroll
        for (int w = 0; w < W; ++w)
            v[w][j] = j < K ? to_key(__float_as_uint(x[j][C0 + w])) : kTopKey;  // wave-uniform
    net_sort<KP, W>(v);
}

// acc / fl32(n), correctly rounded; n == 1 keeps acc's own bits (n is wave-uniform)
template <int W>
__device__ __forceinline__ void divide_by_count(float (&acc)[W], int n) {
    if (n > 1) {
        const float fn = (float)n;
#pragma unroll
        for (int w = 0; w < W; ++w) acc[w] = div_ieee(acc[w], fn);
    }
}

// The rule's body over the lane's four coordinates, W at a time, one pass's keys in
// registers at a time.  KP <= 32 takes all four at once; KP = 64 holds 256 loaded
// values per lane and takes the rule's kW64 (below), the others parked meanwhile.
template <int KP, int W, int C0 = 0, typename Rule>
__device__ __forceinline__ void for_each_pass(const Rule &rule, const f32x4 (&x)[KP], int K,
                                              const typename Rule::Lane &ln, f32x4 &res) {
    static_assert(W == 4 || W == 2 || W == 1, "coordinates per pass");
    rule.template coords<KP, W, C0>(x, K, ln, res);
    if constexpr (C0 + W < 4) {
        __builtin_amdgcn_sched_barrier(0);
        for_each_pass<KP, W, C0 + W>(rule, x, K, ln, res);
    }
}

template <typename Rule, int KP, int W>
__global__ __launch_bounds__(kRobustBlock) void k_sorted_columns(
    typename Rule::Rows Uv, int64_t ldu4, const int32_t *__restrict__ rows, int K, Rule rule,
    int64_t P4, typename Rule::Out out) {
    f32x4 x[KP];
    const Place at = load_columns<KP>(Uv, ldu4, rows, K, P4, x);
    const typename Rule::Lane ln = rule.prepare(at.iq);
    f32x4 res;
    for_each_pass<KP, W>(rule, x, K, ln, res);
    rule.store(ln, res, Uv, ldu4, at.i0, P4, out);
}

template <typename Rule, int KP, int W>
void launch(typename Rule::Rows Uv, int64_t ldu4, const int32_t *rows, int K, const Rule &rule,
            int64_t P4, typename Rule::Out out, hipStream_t st) {
    const dim3 grid((unsigned)((P4 + kRobustBlock - 1) / kRobustBlock));
    hipLaunchKernelGGL((k_sorted_columns<Rule, KP, W>), grid, dim3(kRobustBlock), 0, st, Uv, ldu4,
                       rows, K, rule, P4, out);
}

inline const f32x4 *vec4(const float *p) { return reinterpret_cast<const f32x4 *>(p); }
inline f32x4 *vec4(float *p) { return reinterpret_cast<f32x4 *>(p); }

// The operands are checked (rows_common.h); `fn` names the entry point.
template <typename Rule>
int dispatch(const char *fn, typename Rule::Rows Uv, int64_t ldu, const int32_t *rows, int K,
             const Rule &rule, int64_t P, typename Rule::Out out, hipStream_t st) {
    if (P == 0) return DLS_OK;
    const int64_t P4 = P / 4, ldu4 = ldu / 4;
    DLS_REQUIRE((P4 + kRobustBlock - 1) / kRobustBlock < (int64_t)1 << 31, DLS_EINVAL,
                "%s: grid too large", fn);
    if (K == 1)
        launch<Rule, 1, 4>(Uv, ldu4, rows, K, rule, P4, out, st);
    else if (K == 2)
        launch<Rule, 2, 4>(Uv, ldu4, rows, K, rule, P4, out, st);
    else if (K <= 4)
        launch<Rule, 4, 4>(Uv, ldu4, rows, K, rule, P4, out, st);
    else if (K <= 8)
        launch<Rule, 8, 4>(Uv, ldu4, rows, K, rule, P4, out, st);
    else if (K <= 16)
        launch<Rule, 16, 4>(Uv, ldu4, rows, K, rule, P4, out, st);
    else if (K <= 32)
        launch<Rule, 32, 4>(Uv, ldu4, rows, K, rule, P4, out, st);
    else
        launch<Rule, 64, Rule::kW64>(Uv, ldu4, rows, K, rule, P4, out, st);
    return check_launch(fn);
}

// ---------------------------------------------------------------- the rules
// A rule carries its scalar parameters as a kernel argument and provides
//   Rows, Out   the types of the kernel's row pointer and of its last argument;
//   kW64        the coordinates per pass at KP = 64 that fit the register file
//               without scratch;
//   Lane        what a lane holds across the passes, made by prepare(iq);
//   coords      coordinates C0 .. C0 + W - 1: from the loaded values to res;
//   store       the lane's four results to where they go.

// Rules that reduce the K rows to one: res goes to out[i0].
struct ToOneRow {
    using Rows = const f32x4 *__restrict__;
    using Out = f32x4 *__restrict__;
    struct Lane {};
    __device__ __forceinline__ Lane prepare(int64_t) const { return {}; }
    __device__ __forceinline__ void store(const Lane &, const f32x4 &res, Rows, int64_t,
                                          int64_t i0, int64_t P4, Out out) const {
        if (i0 < P4) out[i0] = res;
    }
};

// dls_trimmed_mean_f32: drop the `trim` lowest and highest of the sorted values,
// acc = v[trim]; acc = fl(acc + v[i]) ascending; out = fl(acc / fl32(m)), m = K - 2
// trim; any NaN result is 0x7fc00000.  The kept wires are wave-uniform.
struct TrimmedMean : ToOneRow {
    int trim;
    // two at a time: 128 keys in work beside the 256 loaded values
    static constexpr int kW64 = 2;

    template <int KP, int W, int C0>
    __device__ __forceinline__ void coords(const f32x4 (&x)[KP], int K, const Lane &,
                                           f32x4 &res) const {
        uint32_t v[W][KP];
        sorted_keys<KP, W, C0>(x, K, v);
        const int lo = trim, hi = K - 1 - trim;
        float acc[W];
        // -0 + t == t for every fp32 t (-0 and NaN included), so starting from -0
        // makes v[trim] the first term with its own bits, and m == 1 adds nothing else
#pragma unroll
        for (int w = 0; w < W; ++w) acc[w] = -0.f;
#pragma unroll
        for (int j = 0; j < KP; ++j) {
            const bool kept = j >= lo && j <= hi;  // wave-uniform; t + -0 == t as well
#pragma unroll
            for (int w = 0; w < W; ++w) acc[w] = acc[w] + (kept ? from_key(v[w][j]) : -0.f);
        }
        divide_by_count<W>(acc, hi - lo + 1);
#pragma unroll
        for (int w = 0; w < W; ++w) res[C0 + w] = quiet(acc[w]);
    }
};

// dls_mean_around_median_f32 (MeaMed): the `keep` consecutive sorted values closest
// to the median, summed ascending.  After the sort, per coordinate:
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
//   sum   = the ascending sum with kept = s <= j < s + keep, a per-lane select
//           (each of the lane's coordinates has its own s).
template <int KP>
constexpr int shift_stages() {
    int n = 0;
    while ((1 << n) <= KP) ++n;  // keep <= KP: bits 0 .. log2(KP)
    return n;
}

struct MeanAroundMedian : ToOneRow {
    int keep;
    // one at a time: beside the parked loads a pass holds the sorted values and their
    // moved copy, and two coordinates per pass spilled 60 bytes per lane to scratch
    static constexpr int kW64 = 1;

    template <int KP, int W, int C0>
    __device__ __forceinline__ void coords(const f32x4 (&x)[KP], int K, const Lane &,
                                           f32x4 &res) const {
        uint32_t v[W][KP];
        sorted_keys<KP, W, C0>(x, K, v);
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
        divide_by_count<W>(acc, keep);
#pragma unroll
        for (int w = 0; w < W; ++w) res[C0 + w] = quiet(acc[w]);
    }
};

// dls_craft_rows_f32 (ALIE, IPM): out = base + a * (mu - base) + b * sigma per
// coordinate, mu and sigma the ascending mean and the population standard deviation
// of the K honest values, written into every attacker row.  The sorted keys stay in
// registers and are decoded twice: once for the ascending sum over the wires < K
// (the trimmed mean's with trim 0), and, when b != 0 (wave-uniform), once more for
// the deviations
//   d = fl(v[j] - mu); s = fmaf(d, d, s),
// where a wire >= K (a NaN) is masked out by a wave-uniform select.  Nothing beside
// that fmaf is contracted (the library is built with -ffp-contract=off).  The
// attacker rows reach the wave as the honest ones do (a per-lane table and
// v_readlane) and take one 16-byte store each.
struct InPlace {};  // the results go into rows of U itself

struct CraftRows {
    using Rows = f32x4 *;
    using Out = InPlace;
    const int32_t *arows;
    int Ka;
    float a, b;
    const f32x4 *base;
    static constexpr int kW64 = 2;  // nothing but the keys is live across the two sums

    struct Lane {
        int ta;  // the lane's entry of the attacker table
        bool has_base;
        f32x4 bs;
    };
    __device__ __forceinline__ Lane prepare(int64_t iq) const {
        Lane ln;
        ln.ta = arows[min((int)__lane_id(), Ka - 1)];
        ln.has_base = base != nullptr;  // wave-uniform
        ln.bs = (f32x4){0.f, 0.f, 0.f, 0.f};
        if (ln.has_base) ln.bs = base[iq];
        return ln;
    }

    template <int KP, int W, int C0>
    __device__ __forceinline__ void coords(const f32x4 (&x)[KP], int K, const Lane &ln,
                                           f32x4 &res) const {
        uint32_t v[W][KP];
        sorted_keys<KP, W, C0>(x, K, v);
        float mu[W], sg[W];
        // the trimmed mean's sum with trim 0: from -0, so that v[0] keeps its own bits
#pragma unroll
        for (int w = 0; w < W; ++w) mu[w] = -0.f;
#pragma unroll
        for (int j = 0; j < KP; ++j) {
            const bool kept = j < K;  // wave-uniform; t + -0 == t
#pragma unroll
            for (int w = 0; w < W; ++w) mu[w] = mu[w] + (kept ? from_key(v[w][j]) : -0.f);
        }
        divide_by_count<W>(mu, K);
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
            divide_by_count<W>(s, K);
#pragma unroll
            for (int w = 0; w < W; ++w) sg[w] = sqrt_ieee(s[w]);
        }
#pragma unroll
        for (int w = 0; w < W; ++w) {
            const float z = ln.bs[C0 + w];
            const float t = ln.has_base ? mu[w] - z : mu[w];
            float r = a * t;
            const float e = b * sg[w];
            r = use_b ? r + e : r;
            res[C0 + w] = quiet(ln.has_base ? z + r : r);
        }
    }

    __device__ __forceinline__ void store(const Lane &ln, const f32x4 &res, Rows Uv, int64_t ldu4,
                                          int64_t i0, int64_t P4, Out) const {
        for (int j = 0; j < Ka; ++j) {  // wave-uniform trip count and row
            const int64_t r = __builtin_amdgcn_readlane(ln.ta, j);
            if (i0 < P4) Uv[r * ldu4 + i0] = res;
        }
    }
};

}  // namespace
}  // namespace dls

using namespace dls;

extern "C" int dls_trimmed_mean_f32(const float *U, int64_t ldu, const int32_t *rows, int32_t K,
                                    int32_t trim, int64_t P, float *out, dls_stream_t stream) {
    const char *fn = "dls_trimmed_mean_f32";
    int rc = check_head(fn, U && rows && out, "K", K);
    if (rc != DLS_OK) return rc;
    DLS_REQUIRE(trim >= 0 && 2 * (int64_t)trim < K, DLS_EINVAL,
                "%s: trim=%d (0 <= 2*trim < K=%d)", fn, trim, K);
    rc = check_layout(fn, ldu, P, aligned16(U) && aligned16(out));
    if (rc != DLS_OK) return rc;
    return dispatch(fn, vec4(U), ldu, rows, K, TrimmedMean{{}, trim}, P, vec4(out),
                    as_stream(stream));
}

extern "C" int dls_mean_around_median_f32(const float *U, int64_t ldu, const int32_t *rows,
                                          int32_t K, int32_t keep, int64_t P, float *out,
                                          dls_stream_t stream) {
    const char *fn = "dls_mean_around_median_f32";
    int rc = check_head(fn, U && rows && out, "K", K);
    if (rc != DLS_OK) return rc;
    DLS_REQUIRE(keep >= 1 && keep <= K, DLS_EINVAL, "%s: keep=%d (1 <= keep <= K=%d)", fn, keep,
                K);
    rc = check_layout(fn, ldu, P, aligned16(U) && aligned16(out));
    if (rc != DLS_OK) return rc;
    return dispatch(fn, vec4(U), ldu, rows, K, MeanAroundMedian{{}, keep}, P, vec4(out),
                    as_stream(stream));
}

extern "C" int dls_craft_rows_f32(float *U, int64_t ldu, const int32_t *hrows, int32_t Kh,
                                  const int32_t *arows, int32_t Ka, float a, float b,
                                  const float *base, int64_t P, dls_stream_t stream) {
    const char *fn = "dls_craft_rows_f32";
    int rc = check_head(fn, U && hrows && arows, "Kh", Kh);
    if (rc == DLS_OK) rc = check_count(fn, "Ka", Ka);
    if (rc != DLS_OK) return rc;
    DLS_REQUIRE(std::isfinite(a) && std::isfinite(b), DLS_EINVAL,
                "%s: a=%g and b=%g must be finite", fn, (double)a, (double)b);
    rc = check_layout(fn, ldu, P, aligned16(U) && aligned16(base));
    if (rc != DLS_OK) return rc;
    return dispatch(fn, vec4(U), ldu, hrows, Kh, CraftRows{arows, Ka, a, b, vec4(base)}, P,
                    InPlace{}, as_stream(stream));
}
