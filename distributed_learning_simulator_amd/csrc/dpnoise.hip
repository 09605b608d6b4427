// The library's random stream and the client-level DP-FedAvg step on it for gfx950
// (McMahan et al. 2018; FedServer dp_clip): the clipped mean of the clients' updates
// plus Gaussian noise, in one read of the rows.
//
//   stream:  Philox4x32-10 on (seed, stream_id, coordinate / 4); word coordinate % 4
//   normal:  Box-Muller on the word pairs (0, 1) and (2, 3) of a block
//   step:    z[p] = fl32(fl32(z[p] + sum_k fl32(c[k] * fl32(U[rows[k]][p] - z[p])))
//                        + fl32(sigma * g_p))
// (include/dls_hip.h has the contract.)  A value is a function of (seed, stream_id,
// coordinate) alone, so the bits do not depend on anything below.
//
// The step streams the rows the way k_weiszfeld's clip mode does (weiszfeld.hip): lanes
// across coordinates, a lane owns VW consecutive coordinates of a tile of 64 VW (VW = 4
// for K <= 32, 2 above), the row indices and coefficients reach the wave through
// per-lane tables and v_readlane, every load is unconditional (a wire past K re-reads
// the last row; its term is replaced by -0) and non-temporal.  There are no distances,
// so no chains, no butterfly and no second launch.
//
// The generator runs after the K loads of a tile have been issued and their values
// summed, on registers the rows no longer need.  One Philox call makes the four words of
// a block of four coordinates: with VW = 4 that is exactly the lane's vector.  With
// VW = 2 a lane owns half a block; the two lanes of a block each compute the whole block
// and keep their own word pair (no cross-lane traffic; the Box-Muller transform is per
// word pair and is not repeated).  That doubles the integer work per coordinate, about 70
// extra VALU instructions per lane and tile, where K > 32 rows make a tile at least 33
// eight-byte loads per lane: the step stays bound by its loads there.  Per block the
// generator issues about 20 v_mul_hi_u32 / v_mul_lo_u32 pairs, two logf, two square
// roots and two cospif / sinpif pairs, a few hundred VALU instructions against (K + 2)
// 16-byte accesses per lane; no LDS, no atomics.
#include <cmath>
#include <type_traits>

#include "philox_common.h"
#include "rows_common.h"

namespace dls {
namespace {

constexpr int kBlock = 256;        // 4 waves; no wave waits on another
constexpr int kMaxWaves = 2048;    // 256 CUs x 8 resident waves
constexpr int kMaxBlocks = 4096;   // of the generator-only kernels (grid-strided)

// u = ((w >> 9) + 0.5) * 2^-23: every step exact in fp32
__device__ __forceinline__ float uniform_of(uint32_t w) {
    return ((float)(w >> 9) + 0.5f) * 0x1p-23f;
}

// Box-Muller on one word pair; each operation rounded once (-ffp-contract=off)
__device__ __forceinline__ f32x2 normal_pair(uint32_t wa, uint32_t wb) {
    const float r = sqrt_ieee(-2.0f * logf(uniform_of(wa)));
    const float a = 2.0f * uniform_of(wb);
    return (f32x2){r * cospif(a), r * sinpif(a)};
}

// ------------------------------------------------------------ the stream alone
// Thread per block of four coordinates, from the block that holds `first`; a thread
// stores the words (NORMAL: the normals) of its coordinates inside [first, first + n).
template <bool NORMAL>
__global__ __launch_bounds__(kBlock) void k_philox(uint32_t *__restrict__ out, int64_t n,
                                                   int64_t first, int64_t nblocks,
                                                   PhiloxKey key) {
    const int64_t b0 = first >> 2;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < nblocks;
         i += (int64_t)gridDim.x * kBlock) {
        u32x4 w = philox_block((uint64_t)(b0 + i), key);
        if constexpr (NORMAL) {
            const f32x2 g0 = normal_pair(w[0], w[1]), g1 = normal_pair(w[2], w[3]);
            w = (u32x4){__float_as_uint(g0[0]), __float_as_uint(g0[1]), __float_as_uint(g1[0]),
                        __float_as_uint(g1[1])};
        }
        const int64_t o = (b0 + i) * 4 - first;  // where the block's word 0 would go
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (o + j >= 0 && o + j < n) out[o + j] = w[j];
    }
}

// Thread per word pair.
__global__ __launch_bounds__(kBlock) void k_normal_from_bits(const uint32_t *bits, int64_t pairs,
                                                             float *out) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < pairs;
         i += (int64_t)gridDim.x * kBlock) {
        const f32x2 g = normal_pair(bits[2 * i], bits[2 * i + 1]);
        out[2 * i] = g[0];
        out[2 * i + 1] = g[1];
    }
}

inline unsigned grid_for(int64_t threads) {
    const int64_t blocks = (threads + kBlock - 1) / kBlock;
    return (unsigned)(blocks < kMaxBlocks ? blocks : kMaxBlocks);
}

// ------------------------------------------------------------------- the step
inline int vw_of(int K) { return K <= 32 ? 4 : 2; }

struct StepPlan {
    int64_t tiles;  // of 64 * VW coordinates
    int64_t tpw;    // tiles per wave
    int nW;         // waves
};

// Tile n belongs to wave n % nW as its visit n / nW (a function of P and K alone).
inline StepPlan make_plan(int K, int64_t P) {
    StepPlan p;
    const int64_t tc = 64 * vw_of(K);
    p.tiles = (P + tc - 1) / tc;
    p.tpw = (p.tiles + kMaxWaves - 1) / kMaxWaves;
    p.nW = (int)((p.tiles + p.tpw - 1) / p.tpw);
    return p;
}

// KP wires (a power of two >= K), VW coordinates per lane; NOISE: sigma > 0.
template <int KP, int VW, bool NOISE>
__global__ __launch_bounds__(kBlock) void k_dp_clip_noise(const float *__restrict__ U, int64_t ldu,
                                                          const int32_t *__restrict__ rows, int K,
                                                          const float *__restrict__ c, int64_t P,
                                                          int64_t tiles, int64_t tpw, int nW,
                                                          float *z, float sigma, PhiloxKey key) {
    using vec = std::conditional_t<VW == 4, f32x4, f32x2>;
    static_assert(VW == 4 || VW == 2, "coordinates per lane");
    const int lane = __lane_id();
    const int wv = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (wv >= nW) return;  // the whole wave
    const int tr = rows[min(lane, K - 1)];
    const int tw = __float_as_int(c[min(lane, K - 1)]);
    const int64_t PV = P / VW;
    vec *zv = reinterpret_cast<vec *>(z);

    for (int64_t it = 0; it < tpw; ++it) {
        const int64_t t = it * nW + wv;
        if (t >= tiles) break;  // wave-uniform
        const int64_t i0 = t * 64 + lane;
        const bool in = i0 < PV;
        const int64_t iq = in ? i0 : PV - 1;  // every lane stays: the tables need all 64
        vec x[KP];
#pragma unroll
        for (int j = 0; j < KP; ++j) {
            const int64_t r = __builtin_amdgcn_readlane(tr, j);
            x[j] = __builtin_nontemporal_load(reinterpret_cast<const vec *>(U + r * ldu) + iq);
        }
        // The old z: an ordinary load (this lane stores z' to the same address and nobody
        // else reads it).  A lane past P re-reads index PV - 1, which its owner in this
        // wave may already have rewritten: such a lane stores nothing.
        const vec zo = zv[iq];
        // Every load of the tile is issued before the first use: without the distances
        // nothing keeps the K values live, and the scheduler would otherwise sink each load
        // to its use, one load in flight per wave.
        __builtin_amdgcn_sched_barrier(0);
        // t_k = fl32(c_k * fl32(x_k - z)); acc = t_0; acc = fl32(acc + t_k);
        // y = fl32(z + acc): no fma (-ffp-contract=off), a wire past K adds -0
        vec acc;
#pragma unroll
        for (int j = 0; j < KP; ++j) {
            const float cj = __int_as_float(__builtin_amdgcn_readlane(tw, j));
            vec tk = (x[j] - zo) * cj;
            if (j == 0) {
                acc = tk;
            } else {
                if (j >= K) tk = (vec)(-0.f);  // wave-uniform
                acc = acc + tk;
            }
        }
        vec zq = zo + acc;
        if constexpr (NOISE) {
            // the lane's coordinates are iq * VW ..: block iq (VW = 4) or half iq & 1 of
            // block iq >> 1 (VW = 2: both lanes of the block compute it)
            vec g;
            if constexpr (VW == 4) {
                const u32x4 w = philox_block((uint64_t)iq, key);
                const f32x2 g0 = normal_pair(w[0], w[1]), g1 = normal_pair(w[2], w[3]);
                g = (vec){g0[0], g0[1], g1[0], g1[1]};
            } else {
                const u32x4 w = philox_block((uint64_t)(iq >> 1), key);
                const bool hi = (iq & 1) != 0;
                g = normal_pair(hi ? w[2] : w[0], hi ? w[3] : w[1]);
            }
            zq = zq + g * sigma;  // fl32(y + fl32(sigma * g))
        }
        if (in) zv[i0] = zq;
    }
}

template <int KP, int VW>
void launch(const float *U, int64_t ldu, const int32_t *rows, int K, const float *c, int64_t P,
            float *z, float sigma, PhiloxKey key, hipStream_t st) {
    const StepPlan pl = make_plan(K, P);
    const unsigned blocks = (unsigned)((pl.nW + kBlock / 64 - 1) / (kBlock / 64));
    if (sigma > 0.f)
        hipLaunchKernelGGL((k_dp_clip_noise<KP, VW, true>), dim3(blocks), dim3(kBlock), 0, st, U,
                           ldu, rows, K, c, P, pl.tiles, pl.tpw, pl.nW, z, sigma, key);
    else
        hipLaunchKernelGGL((k_dp_clip_noise<KP, VW, false>), dim3(blocks), dim3(kBlock), 0, st, U,
                           ldu, rows, K, c, P, pl.tiles, pl.tpw, pl.nW, z, sigma, key);
}

// The checks the generator-only entry points share, in their order.
int check_stream_call(const char *fn, bool nonnull, bool aligned, int64_t n, int64_t first) {
    DLS_REQUIRE(nonnull, DLS_EINVAL, "%s: null pointer", fn);
    DLS_REQUIRE(n >= 0, DLS_EINVAL, "%s: n=%lld", fn, (long long)n);
    DLS_REQUIRE(first >= 0 && first <= INT64_MAX - n, DLS_EINVAL,
                "%s: first=%lld (first >= 0, first + n <= 2^63 - 1)", fn, (long long)first);
    DLS_REQUIRE(aligned, DLS_ELAYOUT, "%s: 4-byte alignment", fn);
    return DLS_OK;
}

template <bool NORMAL>
int run_philox(const char *fn, void *out, int64_t n, uint64_t seed, uint64_t stream_id,
               int64_t first, dls_stream_t stream) {
    const int rc = check_stream_call(fn, out != nullptr, aligned_to(out, 4), n, first);
    if (rc != DLS_OK || n == 0) return rc;
    const int64_t nblocks = ((first + n - 1) >> 2) - (first >> 2) + 1;
    hipLaunchKernelGGL(k_philox<NORMAL>, dim3(grid_for(nblocks)), dim3(kBlock), 0,
                       as_stream(stream), static_cast<uint32_t *>(out), n, first, nblocks,
                       make_key(seed, stream_id));
    return check_launch(fn);
}

}  // namespace
}  // namespace dls

using namespace dls;

extern "C" int dls_philox_u32(uint32_t *out, int64_t n, uint64_t seed, uint64_t stream_id,
                              int64_t first, dls_stream_t stream) {
    return run_philox<false>("dls_philox_u32", out, n, seed, stream_id, first, stream);
}

extern "C" int dls_philox_normal_f32(float *out, int64_t n, uint64_t seed, uint64_t stream_id,
                                     int64_t first, dls_stream_t stream) {
    return run_philox<true>("dls_philox_normal_f32", out, n, seed, stream_id, first, stream);
}

extern "C" int dls_normal_from_bits_f32(const uint32_t *bits, int64_t n, float *out,
                                        dls_stream_t stream) {
    const char *fn = "dls_normal_from_bits_f32";
    const int rc = check_stream_call(fn, bits && out, aligned_to(bits, 4) && aligned_to(out, 4), n, 0);
    if (rc != DLS_OK) return rc;
    DLS_REQUIRE(n % 2 == 0, DLS_EINVAL, "%s: n=%lld must be even (word pairs)", fn, (long long)n);
    if (n == 0) return DLS_OK;
    hipLaunchKernelGGL(k_normal_from_bits, dim3(grid_for(n / 2)), dim3(kBlock), 0,
                       as_stream(stream), bits, n / 2, out);
    return check_launch(fn);
}

extern "C" int dls_dp_clip_noise_step_f32(const float *U, int64_t ldu, const int32_t *rows,
                                          int32_t K, const float *c, int64_t P, float *z,
                                          float sigma, uint64_t seed, uint64_t stream_id,
                                          dls_stream_t stream) {
    const char *fn = "dls_dp_clip_noise_step_f32";
    int rc = check_head(fn, U && rows && c && z, "K", K);
    if (rc != DLS_OK) return rc;
    DLS_REQUIRE(std::isfinite(sigma) && sigma >= 0.f, DLS_EINVAL,
                "%s: sigma=%g must be finite and >= 0", fn, (double)sigma);
    rc = check_layout(fn, ldu, P, aligned16(U) && aligned16(z) && aligned_to(c, 4), " (U, z)");
    if (rc != DLS_OK || P == 0) return rc;
    hipStream_t st = as_stream(stream);
    const PhiloxKey key = make_key(seed, stream_id);
    if (K <= 4)
        launch<4, 4>(U, ldu, rows, K, c, P, z, sigma, key, st);
    else if (K <= 8)
        launch<8, 4>(U, ldu, rows, K, c, P, z, sigma, key, st);
    else if (K <= 16)
        launch<16, 4>(U, ldu, rows, K, c, P, z, sigma, key, st);
    else if (K <= 32)
        launch<32, 4>(U, ldu, rows, K, c, P, z, sigma, key, st);
    else
        launch<64, 2>(U, ldu, rows, K, c, P, z, sigma, key, st);
    return check_launch(fn);
}
