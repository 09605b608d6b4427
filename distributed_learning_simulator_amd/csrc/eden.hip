// Multi-bit rotated compression for gfx950 (Vargaftik et al. 2022, "EDEN: communication-
// efficient and robust distributed mean estimation for federated learning"): drive.hip's
// rotation, then per coordinate the nearest level of the Lloyd-Max quantizer of the normal
// distribution at 2 or 4 bits, scaled by the block's root mean square, and one scale per block
// that makes the decode unbiased.  include/dls_hip.h has the contract.
//
// Both kernels give a 256-thread workgroup one block of 4096 coordinates in the register
// ownership of hadamard_common.h: the thread (wave v, lane l) holds the coordinates 1024 v +
// 64 r + l, r = 0..15.  The code row is laid out for that ownership: a thread's 16 fields are
// BITS / 2 whole words, word h of them at (v BITS / 2 + h) 64 + l of the block's 128 BITS words,
// so a wave stores or loads 256 contiguous bytes per word and no field crosses a thread.
//
// The compressor.  The thresholds need the block's sum of squares, so the block meets twice
// in LDS: once for sq (every thread then forms rms and the M - 1 thresholds itself), once for
// dot, qq and the non-finite count behind the code stores.  The magnitude index is the last
// threshold the value exceeds (the thresholds ascend), and the centroid follows through the
// same compares: 2 (M - 1) selects per coordinate, nothing indexed.  The three sums are fp64
// in the order of dls_drive_compress_f32, and the non-finite count goes through its per-stream
// ticket cell (drive.hip has the protocol): no fence.
//
// The server.  Per client and rotated coordinate the chain adds t[i][f], one of 2^BITS
// values that are fixed per client and block.  A tile's tables are built once per block in
// LDS (64 clients x 2^BITS floats, 4 KB at 4 bits, beside the rotation's 16 KB): four threads
// per client form c[i] and a quarter of its row each.  The client loop then costs, per
// coordinate, three VALU operations for the address (the field's shift and mask and the add of
// the row's base), one ds_read_b32 and the chain's add; a wave's 64 reads touch at most 2^BITS consecutive dwords, so they never conflict.  The next
// kAhead clients' code words are loaded while the current ones are looked up.  DESIGN.md
// ("Multi-bit rotated compression") has the timings of this form and of the table kept across
// lanes behind ds_bpermute_b32, which was not kept.  The accumulator starts as -0.0 (fl(-0.0
// + t) has t's bits for every t), so "the first assigns" costs no select.
#include "hadamard_common.h"

namespace dls {
namespace {

constexpr int kTileK = DLS_EDEN_CLIENT_TILE;  // clients per table in LDS
constexpr int kAhead = 4;                     // clients whose code words are in flight
static_assert(kTileK * 4 == kBlock, "four threads build a client's table row");

// cent_b[m] and bound_b[m]; m is a constant after unrolling everywhere but in the server's
// table build
template <int BITS>
__device__ __forceinline__ float centroid(int m) {
    if constexpr (BITS == 2) {
        const float c[2] = DLS_EDEN_CENT2;
        return c[m];
    } else {
        const float c[8] = DLS_EDEN_CENT4;
        return c[m];
    }
}

template <int BITS>
__device__ __forceinline__ float boundary(int m) {
    if constexpr (BITS == 2) {
        const float t[1] = DLS_EDEN_BOUND2;
        return t[m];
    } else {
        const float t[7] = DLS_EDEN_BOUND4;
        return t[m];
    }
}

// the words of a block's code row before those of thread (wave, lane = 0)
template <int BITS>
__device__ __forceinline__ int64_t first_word(int64_t B, int wave) {
    return B * (kD * BITS / 32) + wave * (BITS / 2) * 64;
}

template <int BITS>
__global__ __launch_bounds__(kBlock) void k_eden_compress(
    const float *__restrict__ w, const float *__restrict__ base, int64_t P, PhiloxKey key,
    int scale_mode, uint32_t *__restrict__ codes, float *__restrict__ scales,
    int32_t *__restrict__ stats, unsigned long long *cell) {
    constexpr int kM = 1 << (BITS - 1), kFpw = 32 / BITS, kCw = BITS / 2;
    __shared__ f32x4 xch[kD / 4];
    __shared__ double lsq[kWaves], ldot[kWaves], lqq[kWaves];
    __shared__ uint32_t lbad[kWaves];
    const int64_t B = blockIdx.x;
    const int wave = uniform(threadIdx.x >> 6), lane = lane_id();
    const int64_t j = first_coordinate(B, wave, lane);
    uint64_t m[kRegs];
    sign_masks(m, B, wave, lane, key);
    float v[kRegs], vb[kRegs];
#pragma unroll
    for (int r = 0; r < kRegs; ++r) {
        const bool in = j + 64 * r < P;
        v[r] = in ? ldg_nt(w + j + 64 * r) : 0.f;
        vb[r] = in ? ldg_nt(base + j + 64 * r) : 0.f;
    }
    uint32_t nbad = 0;
#pragma unroll
    for (int r = 0; r < kRegs; ++r) {
        v[r] = v[r] - vb[r];
        nbad += (__float_as_uint(v[r]) & 0x7fffffffu) >= 0x7f800000u;
    }
    apply_signs(v, m);
    hadamard(v, xch, wave, lane);
    scale_down(v);
    double sq = 0.0;
#pragma unroll
    for (int r = 0; r < kRegs; ++r) {
        const double y = (double)v[r];
        sq += y * y;
    }
    sq = wave_tree(sq);
    if (lane == 0) lsq[wave] = sq;
    __syncthreads();
    sq = ((lsq[0] + lsq[1]) + lsq[2]) + lsq[3];
    const float rms = (float)__builtin_sqrt(sq / (double)kD);
    float thr[kM - 1];
#pragma unroll
    for (int k = 0; k < kM - 1; ++k) thr[k] = boundary<BITS>(k) * rms;
    double dot = 0.0, qq = 0.0;
    uint32_t word[kCw];
#pragma unroll
    for (int h = 0; h < kCw; ++h) word[h] = 0;
#pragma unroll
    for (int r = 0; r < kRegs; ++r) {
        const float a = __builtin_fabsf(v[r]);
        uint32_t idx = 0;
        float c = centroid<BITS>(0);
#pragma unroll
        for (int k = 0; k < kM - 1; ++k) {  // ascending thresholds: the last one exceeded counts
            const bool over = a > thr[k];
            idx = over ? (uint32_t)(k + 1) : idx;
            c = over ? centroid<BITS>(k + 1) : c;
        }
        const double cd = (double)c;
        dot += (double)a * cd;
        qq += cd * cd;
        const uint32_t field = idx | (v[r] < 0.f ? (uint32_t)kM : 0u);
        word[r / kFpw] |= field << ((r % kFpw) * BITS);
    }
    uint32_t *row = codes + first_word<BITS>(B, wave) + lane;
#pragma unroll
    for (int h = 0; h < kCw; ++h) row[h * 64] = word[h];
    dot = wave_tree(dot);
    qq = wave_tree(qq);
    nbad = wave_sum(nbad);
    if (lane == 0) {
        ldot[wave] = dot;
        lqq[wave] = qq;
        lbad[wave] = nbad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        dot = ((ldot[0] + ldot[1]) + ldot[2]) + ldot[3];
        qq = ((lqq[0] + lqq[1]) + lqq[2]) + lqq[3];
        nbad = lbad[0] + lbad[1] + lbad[2] + lbad[3];
        scales[B] = dot == 0.0 ? 0.f : (float)(scale_mode == DLS_EDEN_UNBIASED ? sq / dot : dot / qq);
        const unsigned long long before = atomicAdd(cell, (1ull << 32) | nbad);
        if ((before >> 32) == gridDim.x - 1) {  // every other block's count is in `before`
            stats[0] = (int32_t)((uint32_t)before + nbad);
            atomicExch(cell, 0ull);
        }
    }
}

// a thread's 16 fields of one client
template <int BITS>
struct Words {
    uint32_t w[BITS / 2];
};

// client i of the tile whose rows start at `tile` (this thread's first word of each); a client
// past the tile's last (a wave-uniform test) is not loaded and never applied
template <int BITS>
__device__ __forceinline__ Words<BITS> load_words(const uint32_t *tile, int64_t ldc, int i, int nb) {
    Words<BITS> x;
#pragma unroll
    for (int h = 0; h < BITS / 2; ++h) x.w[h] = i < nb ? ldg_nt(tile + (int64_t)i * ldc + h * 64) : 0u;
    return x;
}

// z[r] = fl(z[r] + t[f_r]), t the client's table row in LDS
template <int BITS>
__device__ __forceinline__ void add_client(float (&z)[kRegs], const Words<BITS> &x, const float *t) {
    constexpr int kFpw = 32 / BITS;
#pragma unroll
    for (int r = 0; r < kRegs; ++r)
        z[r] = z[r] + t[(x.w[r / kFpw] >> ((r % kFpw) * BITS)) & ((1u << BITS) - 1u)];
}

template <int BITS>
__global__ __launch_bounds__(kBlock) void k_eden_fedavg(
    const float *__restrict__ base, const uint32_t *__restrict__ codes, int64_t ldc,
    const float *__restrict__ scales, int64_t lds, const float *__restrict__ weight, FastDiv d,
    int K, int64_t P, PhiloxKey key, float *__restrict__ out) {
    constexpr int kLevels = 1 << BITS, kM = kLevels / 2, kEach = kLevels / 4;
    __shared__ f32x4 xch[kD / 4];
    __shared__ float tab[kTileK * kLevels];  // t[i][f] of the tile's clients
    const int64_t B = blockIdx.x;
    const int wave = uniform(threadIdx.x >> 6), lane = lane_id();
    float z[kRegs];
#pragma unroll
    for (int r = 0; r < kRegs; ++r) z[r] = -0.f;
    const uint32_t *mine = codes + first_word<BITS>(B, wave) + lane;
    for (int k0 = 0; k0 < K; k0 += kTileK) {
        __syncthreads();  // the previous tile has been applied
        const int nb = K - k0 < kTileK ? K - k0 : kTileK;
        const int i = threadIdx.x >> 2, f0 = (threadIdx.x & 3) * kEach;
        if (i < nb) {
            const float c = div_exact(scales[(int64_t)(k0 + i) * lds + B] * weight[k0 + i], d);
#pragma unroll
            for (int e = 0; e < kEach; ++e) {
                const int f = f0 + e;
                const float t = c * centroid<BITS>(f & (kM - 1));
                tab[i * kLevels + f] = (f & kM) ? __uint_as_float(__float_as_uint(t) | 0x80000000u) : t;
            }
        }
        __syncthreads();
        const uint32_t *tile = mine + (int64_t)k0 * ldc;
        Words<BITS> cur[kAhead], nxt[kAhead];
#pragma unroll
        for (int a = 0; a < kAhead; ++a) cur[a] = load_words<BITS>(tile, ldc, a, nb);
        for (int i0 = 0; i0 < nb; i0 += kAhead) {
#pragma unroll
            for (int a = 0; a < kAhead; ++a) nxt[a] = load_words<BITS>(tile, ldc, i0 + kAhead + a, nb);
#pragma unroll
            for (int a = 0; a < kAhead; ++a) {
                if (i0 + a < nb) add_client<BITS>(z, cur[a], tab + (i0 + a) * kLevels);
                cur[a] = nxt[a];
            }
        }
    }
    const int64_t j = first_coordinate(B, wave, lane);
    float vb[kRegs];
#pragma unroll
    for (int r = 0; r < kRegs; ++r) vb[r] = j + 64 * r < P ? ldg_nt(base + j + 64 * r) : 0.f;
    uint64_t m[kRegs];
    sign_masks(m, B, wave, lane, key);
    hadamard(z, xch, wave, lane);
    scale_down(z);
    apply_signs(z, m);
#pragma unroll
    for (int r = 0; r < kRegs; ++r)
        if (j + 64 * r < P) out[j + 64 * r] = vb[r] + z[r];
}

}  // namespace
}  // namespace dls

using namespace dls;

extern "C" int dls_eden_compress_f32(const float *w, const float *base, int64_t P, int32_t bits,
                                     uint64_t seed, uint64_t stream_id, int32_t scale_mode,
                                     uint32_t *codes, float *scales, int32_t *stats,
                                     dls_stream_t stream) {
    const char *fn = "dls_eden_compress_f32";
    DLS_REQUIRE(w && base && codes && scales && stats, DLS_EINVAL,
                "%s: null pointer (w, base, codes, scales, stats)", fn);
    DLS_REQUIRE(bits == 2 || bits == 4, DLS_EINVAL, "%s: bits=%d (2 or 4)", fn, bits);
    DLS_REQUIRE(scale_mode == DLS_EDEN_UNBIASED || scale_mode == DLS_EDEN_MSE, DLS_EINVAL,
                "%s: scale_mode=%d (DLS_EDEN_UNBIASED or DLS_EDEN_MSE)", fn, scale_mode);
    const int rc = check_extent(fn, P);
    if (rc != DLS_OK) return rc;
    DLS_REQUIRE(aligned16(w) && aligned16(base) && aligned16(codes) && aligned16(scales) &&
                    aligned16(stats),
                DLS_ELAYOUT, "%s: 16-byte alignment of w, base, codes, scales and stats", fn);
    const int64_t NB = blocks_of(P), cb = NB * kD * bits / 8;  // the code row's bytes
    DLS_REQUIRE(!overlap(codes, cb, w, 4 * P) && !overlap(codes, cb, base, 4 * P) &&
                    !overlap(scales, 4 * NB, w, 4 * P) && !overlap(scales, 4 * NB, base, 4 * P) &&
                    !overlap(stats, 4, w, 4 * P) && !overlap(stats, 4, base, 4 * P),
                DLS_EINVAL, "%s: codes, scales and stats must not alias w or base", fn);
    unsigned long long *cell = stream_cell(as_stream(stream));
    DLS_REQUIRE(cell, DLS_EINVAL, "%s: no device memory for the stream's counter cell", fn);
    const PhiloxKey key = make_key(seed, stream_id);
    if (bits == 2)
        hipLaunchKernelGGL(k_eden_compress<2>, dim3((unsigned)NB), dim3(kBlock), 0, as_stream(stream),
                           w, base, P, key, (int)scale_mode, codes, scales, stats, cell);
    else
        hipLaunchKernelGGL(k_eden_compress<4>, dim3((unsigned)NB), dim3(kBlock), 0, as_stream(stream),
                           w, base, P, key, (int)scale_mode, codes, scales, stats, cell);
    return check_launch(fn);
}

extern "C" int dls_eden_fedavg_f32(const float *base, const uint32_t *codes, int64_t ldc,
                                   const float *scales, int64_t lds, const float *weight,
                                   float total, int32_t K, int64_t P, int32_t bits, uint64_t seed,
                                   uint64_t stream_id, float *out, dls_stream_t stream) {
    const char *fn = "dls_eden_fedavg_f32";
    DLS_REQUIRE(base && codes && scales && weight && out, DLS_EINVAL,
                "%s: null pointer (base, codes, scales, weight, out)", fn);
    DLS_REQUIRE(bits == 2 || bits == 4, DLS_EINVAL, "%s: bits=%d (2 or 4)", fn, bits);
    DLS_REQUIRE(K >= 1, DLS_EINVAL, "%s: K=%d (K >= 1)", fn, K);
    const int rc = check_extent(fn, P);
    if (rc != DLS_OK) return rc;
    const int64_t NB = blocks_of(P), words = NB * kD * bits / 32;
    DLS_REQUIRE(ldc >= words && lds >= NB, DLS_ELAYOUT,
                "%s: ldc=%lld and lds=%lld must be at least 128 bits NB = %lld and NB = %lld", fn,
                (long long)ldc, (long long)lds, (long long)words, (long long)NB);
    DLS_REQUIRE(aligned16(base) && aligned16(codes) && aligned16(scales) && aligned16(weight) &&
                    aligned16(out),
                DLS_ELAYOUT, "%s: 16-byte alignment of base, codes, scales, weight and out", fn);
    DLS_REQUIRE(!overlap(out, 4 * P, base, 4 * P), DLS_EINVAL, "%s: out must not alias base", fn);
    const FastDiv d = make_fastdiv(total);
    const PhiloxKey key = make_key(seed, stream_id);
    if (bits == 2)
        hipLaunchKernelGGL(k_eden_fedavg<2>, dim3((unsigned)NB), dim3(kBlock), 0, as_stream(stream),
                           base, codes, ldc, scales, lds, weight, d, (int)K, P, key, out);
    else
        hipLaunchKernelGGL(k_eden_fedavg<4>, dim3((unsigned)NB), dim3(kBlock), 0, as_stream(stream),
                           base, codes, ldc, scales, lds, weight, d, (int)K, P, key, out);
    return check_launch(fn);
}
