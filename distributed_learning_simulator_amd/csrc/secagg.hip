// Secure aggregation in the ring Z_2^32 on pairwise Philox masks for gfx950 (Bonawitz et
// al. 2017; FedSecAggServer / FedSecAggWorker): the client's fused encode + mask and the
// server's fused sum + mask recovery + decode.
//
//   mask:    y[p] = q(w[p] - base[p]) * weight + sum_{t in add} m_t[p] - sum_{t in sub} m_t[p]
//   unmask:  S[p] = sum_k Y[rows[k]][p] + sum_{t in add} m_t[p] - sum_{t in sub} m_t[p]
//            out[p] = fl32(base[p] + (float)((double)(int32)S[p] * 2^-f / total))
// with m_t[p] the word of coordinate p of the library's stream under (seed, stream t) and
// all integer arithmetic mod 2^32 (include/dls_hip.h has the contract).  Every value is
// an integer until the decode, so the bits depend on nothing below.
//
// Both kernels follow k_dp_clip_noise (dpnoise.hip): 256-thread blocks of four
// independent waves, no LDS, no barrier; a lane owns four consecutive coordinates of a
// tile of 256, which is exactly one Philox block; tile n belongs to wave n % nW as its
// visit n / nW; 16-byte non-temporal loads and stores.  The stream ids are wave-uniform:
// they come through the scalar cache, and the ten rounds of a block are two dependent
// chains of v_mul_hi_u32 / v_mul_lo_u32, so four streams are in flight per iteration.
//
// The mask kernel counts through wave ballots and adds its two counters with one integer
// atomicAdd per wave and counter (an order-independent sum).  The unmask kernel takes the
// row table through per-lane registers and v_readlane; integer addition is associative, so
// K > 32 rows are summed as a chunk of 32 and a chunk of the rest, with the same bits;
// the correction streams run after the last chunk's loads have been issued, on registers
// the rows do not hold, and a lane past P stores nothing.
//
// Cost per lane and tile (four coordinates): mask 2 loads + 1 store of 16 bytes and
// n_add + n_sub Philox blocks; unmask K + 1 loads, 1 (2 with sum_out) stores and
// n_add + n_sub blocks; a block compiles to 36 v_mul_hi_u32 / v_mul_lo_u32 and about 40
// other integer VALU instructions (DESIGN.md has the model and the measurement).
#include <cmath>

#include "philox_common.h"
#include "rows_common.h"

namespace dls {
namespace {

constexpr int kBlock = 256;      // 4 waves; no wave waits on another
constexpr int kMaxWaves = 2048;  // 256 CUs x 8 resident waves
constexpr int kTile = 256;       // coordinates per wave and visit: 64 lanes x 4
constexpr int kChunk = 32;       // rows summed per visit of the row table

struct Plan {
    int64_t tiles;  // of kTile coordinates
    int64_t tpw;    // tiles per wave
    int nW;         // waves
};

// Tile n belongs to wave n % nW as its visit n / nW (a function of P alone).
inline Plan make_plan(int64_t P) {
    Plan p;
    p.tiles = (P + kTile - 1) / kTile;
    p.tpw = (p.tiles + kMaxWaves - 1) / kMaxWaves;
    p.nW = (int)((p.tiles + p.tpw - 1) / p.tpw);
    return p;
}

inline unsigned blocks_of(const Plan &pl) {
    return (unsigned)((pl.nW + kBlock / 64 - 1) / (kBlock / 64));
}

// The sum over the n streams of the words of block b, mod 2^32; `streams` and n are
// wave-uniform.
__device__ __forceinline__ u32x4 mask_sum(const uint64_t *__restrict__ streams, int n, uint64_t b,
                                          uint64_t seed) {
    u32x4 acc = (u32x4)(0u);
    int t = 0;
    for (; t + 4 <= n; t += 4) {
        const u32x4 m0 = philox_block(b, make_key(seed, streams[t]));
        const u32x4 m1 = philox_block(b, make_key(seed, streams[t + 1]));
        const u32x4 m2 = philox_block(b, make_key(seed, streams[t + 2]));
        const u32x4 m3 = philox_block(b, make_key(seed, streams[t + 3]));
        acc += (m0 + m1) + (m2 + m3);
    }
    for (; t < n; ++t) acc += philox_block(b, make_key(seed, streams[t]));
    return acc;
}

// q * weight mod 2^32 of one coordinate; sat / bad: what the two counters count.
__device__ __forceinline__ uint32_t encode(float w, float base, float scale, float limit, int32_t L,
                                           uint32_t weight, bool &sat, bool &bad) {
    const float d = w - base;
    const float r = __builtin_rintf(d * scale);  // ties to even; inf when the product overflows
    bad = !(__builtin_fabsf(d) <= 3.402823466e+38f);  // inf or NaN
    // r is an integer or an infinity here: |r| > L is |r| >= L + 1 = limit, exact in fp32
    sat = !bad && __builtin_fabsf(r) >= limit;
    int32_t q = sat ? (r > 0.f ? L : -L) : (int32_t)r;
    if (bad) q = 0;
    return (uint32_t)q * weight;
}

__global__ __launch_bounds__(kBlock) void k_secagg_mask(
    const float *__restrict__ w, const float *__restrict__ base, int64_t P, int64_t tiles,
    int64_t tpw, int nW, float scale, float limit, int32_t L, uint32_t weight,
    const uint64_t *__restrict__ add, int n_add, const uint64_t *__restrict__ sub, int n_sub,
    uint64_t seed, uint32_t *__restrict__ y, int32_t *stats) {
    const int lane = __lane_id();
    const int wv = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (wv >= nW) return;  // the whole wave
    const int64_t PV = P / 4;
    int n_sat = 0, n_bad = 0;  // wave-uniform

    for (int64_t it = 0; it < tpw; ++it) {
        const int64_t t = it * nW + wv;
        if (t >= tiles) break;  // wave-uniform
        const int64_t i0 = t * 64 + lane;
        const bool in = i0 < PV;
        const int64_t iq = in ? i0 : PV - 1;  // every lane stays: the ballots want all 64
        const f32x4 wq = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(w) + iq);
        const f32x4 bq = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(base) + iq);
        u32x4 acc;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            bool sat, bad;
            acc[j] = encode(wq[j], bq[j], scale, limit, L, weight, sat, bad);
            n_sat += __popcll(__ballot(in && sat));
            n_bad += __popcll(__ballot(in && bad));
        }
        acc += mask_sum(add, n_add, (uint64_t)iq, seed);
        acc -= mask_sum(sub, n_sub, (uint64_t)iq, seed);
        if (in) __builtin_nontemporal_store(acc, reinterpret_cast<u32x4 *>(y) + i0);
    }
    if (lane == 0) {
        if (n_sat) atomicAdd(stats, n_sat);
        if (n_bad) atomicAdd(stats + 1, n_bad);
    }
}

// KP wires (a power of two >= the rows of the last chunk); FULL: a chunk of kChunk rows
// comes first (K > kChunk).
template <int KP, bool FULL>
__global__ __launch_bounds__(kBlock) void k_secagg_unmask(
    const uint32_t *__restrict__ Y, int64_t ldy, const int32_t *__restrict__ rows, int K, int64_t P,
    int64_t tiles, int64_t tpw, int nW, const uint64_t *__restrict__ add, int n_add,
    const uint64_t *__restrict__ sub, int n_sub, uint64_t seed, const float *base, double scale,
    double total, float *out, uint32_t *sum_out) {
    const int lane = __lane_id();
    const int wv = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (wv >= nW) return;  // the whole wave
    const int tr = rows[min(lane, K - 1)];
    const int first = FULL ? kChunk : 0;  // the last chunk's first wire
    const int64_t PV = P / 4;

    for (int64_t it = 0; it < tpw; ++it) {
        const int64_t t = it * nW + wv;
        if (t >= tiles) break;  // wave-uniform
        const int64_t i0 = t * 64 + lane;
        const bool in = i0 < PV;
        const int64_t iq = in ? i0 : PV - 1;  // every lane stays: the table needs all 64
        u32x4 S = (u32x4)(0u);
        if constexpr (FULL) {
            u32x4 x[kChunk];
#pragma unroll
            for (int j = 0; j < kChunk; ++j) {
                const int64_t r = __builtin_amdgcn_readlane(tr, j);
                x[j] = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(Y + r * ldy) + iq);
            }
            __builtin_amdgcn_sched_barrier(0);  // every load of the chunk before the first use
#pragma unroll
            for (int j = 0; j < kChunk; ++j) S += x[j];
        }
        // the last chunk: every load is unconditional (a wire past K re-reads the last row
        // and adds nothing)
        u32x4 x[KP];
#pragma unroll
        for (int j = 0; j < KP; ++j) {
            const int64_t r = __builtin_amdgcn_readlane(tr, min(first + j, K - 1));
            x[j] = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(Y + r * ldy) + iq);
        }
        // The old out may be base itself: an ordinary load (this lane stores to the same
        // address and nobody else reads it).  A lane past P re-reads index PV - 1, which
        // its owner in this wave may already have rewritten: such a lane stores nothing.
        const f32x4 bq = reinterpret_cast<const f32x4 *>(base)[iq];
        __builtin_amdgcn_sched_barrier(0);
        // the masks to take off, while the loads are in flight
        S += mask_sum(add, n_add, (uint64_t)iq, seed);
        S -= mask_sum(sub, n_sub, (uint64_t)iq, seed);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < KP; ++j)
            if (first + j < K) S += x[j];  // wave-uniform
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            // exact product, one rounding in the IEEE fp64 division, one in the cast
            const double dl = ((double)(int32_t)S[j] * scale) / total;
            o[j] = bq[j] + (float)dl;
        }
        if (in) {
            __builtin_nontemporal_store(o, reinterpret_cast<f32x4 *>(out) + i0);
            if (sum_out) __builtin_nontemporal_store(S, reinterpret_cast<u32x4 *>(sum_out) + i0);
        }
    }
}

template <int KP, bool FULL>
void launch_unmask(const uint32_t *Y, int64_t ldy, const int32_t *rows, int K, int64_t P,
                   const uint64_t *add, int n_add, const uint64_t *sub, int n_sub, uint64_t seed,
                   const float *base, double scale, double total, float *out, uint32_t *sum_out,
                   hipStream_t st) {
    const Plan pl = make_plan(P);
    hipLaunchKernelGGL((k_secagg_unmask<KP, FULL>), dim3(blocks_of(pl)), dim3(kBlock), 0, st, Y, ldy,
                       rows, K, P, pl.tiles, pl.tpw, pl.nW, add, n_add, sub, n_sub, seed, base,
                       scale, total, out, sum_out);
}

template <bool FULL, typename... Args>
void launch_unmask_last(int last, Args... args) {
    if (last <= 4)
        launch_unmask<4, FULL>(args...);
    else if (last <= 8)
        launch_unmask<8, FULL>(args...);
    else if (last <= 16)
        launch_unmask<16, FULL>(args...);
    else
        launch_unmask<32, FULL>(args...);
}

// The checks the two entry points share after their heads, in their order: the fixed-point
// format, the stream counts, the tables' presence.
int check_format(const char *fn, int32_t frac_bits, const void *add, int32_t n_add, const void *sub,
                 int32_t n_sub) {
    DLS_REQUIRE(frac_bits >= 0 && frac_bits <= 126, DLS_EINVAL, "%s: frac_bits=%d (0..126)", fn,
                frac_bits);
    DLS_REQUIRE(n_add >= 0 && n_sub >= 0 && (int64_t)n_add + n_sub <= DLS_SECAGG_MAX_STREAMS,
                DLS_EINVAL,
                "%s: n_add=%d and n_sub=%d must be non-negative, n_add + n_sub <= "
                "DLS_SECAGG_MAX_STREAMS=%d",
                fn, n_add, n_sub, DLS_SECAGG_MAX_STREAMS);
    DLS_REQUIRE((add || n_add == 0) && (sub || n_sub == 0), DLS_EINVAL,
                "%s: null stream table with a non-zero count", fn);
    return DLS_OK;
}

}  // namespace
}  // namespace dls

using namespace dls;

extern "C" int dls_secagg_mask_f32(const float *w, const float *base, int64_t P, int32_t frac_bits,
                                   int32_t bits, uint32_t weight, const uint64_t *add_streams,
                                   int32_t n_add, const uint64_t *sub_streams, int32_t n_sub,
                                   uint64_t seed, uint32_t *y, int32_t *stats, dls_stream_t stream) {
    const char *fn = "dls_secagg_mask_f32";
    DLS_REQUIRE(w && base && y && stats, DLS_EINVAL, "%s: null pointer", fn);
    DLS_REQUIRE(bits >= 2 && bits <= 31, DLS_EINVAL, "%s: bits=%d (2..31)", fn, bits);
    DLS_REQUIRE(weight >= 1, DLS_EINVAL, "%s: weight=%u must be at least 1", fn, weight);
    int rc = check_format(fn, frac_bits, add_streams, n_add, sub_streams, n_sub);
    if (rc != DLS_OK) return rc;
    rc = check_layout(fn, P, P,
                      aligned16(w) && aligned16(base) && aligned16(y) && aligned_to(stats, 4) &&
                          aligned_to(add_streams, 8) && aligned_to(sub_streams, 8),
                      " (w, base, y), 8-byte (stream tables), 4-byte (stats)");
    if (rc != DLS_OK || P == 0) return rc;
    const Plan pl = make_plan(P);
    const int32_t L = (int32_t)((1u << (bits - 1)) - 1u);
    hipLaunchKernelGGL(k_secagg_mask, dim3(blocks_of(pl)), dim3(kBlock), 0, as_stream(stream), w,
                       base, P, pl.tiles, pl.tpw, pl.nW, std::ldexp(1.0f, frac_bits),
                       std::ldexp(1.0f, bits - 1), L, weight, add_streams, n_add, sub_streams,
                       n_sub, seed, y, stats);
    return check_launch(fn);
}

extern "C" int dls_secagg_unmask_f32(const uint32_t *Y, int64_t ldy, const int32_t *rows, int32_t K,
                                     const uint64_t *add_streams, int32_t n_add,
                                     const uint64_t *sub_streams, int32_t n_sub, uint64_t seed,
                                     const float *base, int32_t frac_bits, double total, int64_t P,
                                     float *out, uint32_t *sum_out, dls_stream_t stream) {
    const char *fn = "dls_secagg_unmask_f32";
    int rc = check_head(fn, Y && rows && base && out, "K", K);
    if (rc != DLS_OK) return rc;
    rc = check_format(fn, frac_bits, add_streams, n_add, sub_streams, n_sub);
    if (rc != DLS_OK) return rc;
    DLS_REQUIRE(std::isfinite(total) && total >= 1.0, DLS_EINVAL,
                "%s: total=%g must be finite and >= 1", fn, total);
    rc = check_layout(fn, ldy, P,
                      aligned16(Y) && aligned16(base) && aligned16(out) && aligned16(sum_out) &&
                          aligned_to(rows, 4) && aligned_to(add_streams, 8) &&
                          aligned_to(sub_streams, 8),
                      " (Y, base, out, sum_out), 8-byte (stream tables), 4-byte (rows)");
    if (rc != DLS_OK || P == 0) return rc;
    const double scale = std::ldexp(1.0, -frac_bits);
    hipStream_t st = as_stream(stream);
    if (K <= kChunk)
        launch_unmask_last<false>(K, Y, ldy, rows, K, P, add_streams, n_add, sub_streams, n_sub,
                                  seed, base, scale, total, out, sum_out, st);
    else
        launch_unmask_last<true>(K - kChunk, Y, ldy, rows, K, P, add_streams, n_add, sub_streams,
                                 n_sub, seed, base, scale, total, out, sum_out, st);
    return check_launch(fn);
}
