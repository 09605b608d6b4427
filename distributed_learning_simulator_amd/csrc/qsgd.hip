// Stochastic quantization for gfx950 (Alistarh et al. 2017, "QSGD: communication-efficient SGD
// via gradient quantization and encoding"; Wen et al. 2017, "TernGrad", its one-level max-norm
// case): the client's compressor and the server's FedAvg over packed 2-, 4- and 8-bit codes.
// include/dls_hip.h has the contract.
//
// Both kernels give one wave to one bucket of 512 coordinates and four buckets to a
// 256-thread workgroup; a lane owns the 8 consecutive coordinates 8 g .. 8 g + 7 of its global
// lane index g = 64 bucket + lane.  So
//   - w and base come as two 16-byte loads each, a wave reads 2 KB of either contiguously;
//   - the lane's Philox words are the blocks 2 g and 2 g + 1 whole;
//   - the lane's eight b-bit fields are 8 b contiguous bits of the code row: one uint32 at
//     b = 4 (a wave stores or loads 256 contiguous bytes), two at b = 8 (one 8-byte access),
//     and 16 bits at b = 2, where the compressor's odd lane hands its half to the even one
//     with one DPP move (quad_perm [1,0,3,2]) and the even lane stores, and the server loads
//     16 bits per lane.
// Nothing passes between a bucket's lanes but the norm (the compressor's wave reduction over
// __shfl_xor: the integer max of the |u| patterns, or the fp64 butterfly 32, 16, .., 1) and
// the server's c[i], which lane i forms once per tile of 64 clients and the client loop reads
// with v_readlane: wave-uniform, no per-lane divide.  The server keeps kAhead clients' code
// loads in flight ahead of the chain; fields leave a word through v_bfe_i32, and the chain
// per client and coordinate is one convert, one multiply and one add on the scalar-per-lane
// VALU forms (the Makefile builds this file without the packed fp32 forms, like efsign.hip).
// The accumulator starts as -0.0: fl(-0.0 + p) has p's bits for every p, so "the first
// assigns" costs no select.
//
// The compressor's count of non-finite coordinates goes through the per-stream cell of
// dls_drive_compress_f32 (drive.hip has the protocol): the four waves of a workgroup put
// their counts into 16 bytes of LDS, and after the one barrier, behind every store of the
// workgroup, thread 0 takes the ticket with one integer atomic.  The kernels have no other
// LDS and no other barrier.
#include "philox_common.h"

namespace dls {
namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kBucket = DLS_QSGD_BUCKET;       // coordinates per bucket, 8 per lane
constexpr int kTileK = DLS_QSGD_CLIENT_TILE;   // clients per c table (one per lane)
constexpr int kAhead = 8;                      // clients whose code loads are in flight
constexpr int64_t kMaxP = (int64_t)1 << 31;
static_assert(kBucket == 512 && kTileK == 64, "a lane owns 8 coordinates and one client's c");

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t o = __shfl_xor(v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}

template <int B, int NORM>
__global__ __launch_bounds__(kBlock) void k_qsgd_compress(
    const float *__restrict__ w, const float *__restrict__ base, int64_t P, int64_t NB,
    PhiloxKey key, uint32_t *__restrict__ codes, float *__restrict__ scales,
    int32_t *__restrict__ stats, unsigned long long *cell) {
    __shared__ uint32_t lbad[kWaves];
    constexpr int kS = (1 << (B - 1)) - 1;
    constexpr float fS = (float)kS;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = lane_id();
    const int64_t bucket = (int64_t)blockIdx.x * kWaves + wave;
    uint32_t nbad = 0;
    if (bucket < NB) {
        const int64_t g = bucket * 64 + lane, j = 8 * g;
        float u[8];
        if (j < P) {  // P is a multiple of 64: a lane's eight lie inside the row together
            const f32x4 w0 = ldg_nt((const f32x4 *)(w + j)), w1 = ldg_nt((const f32x4 *)(w + j + 4));
            const f32x4 b0 = ldg_nt((const f32x4 *)(base + j)),
                        b1 = ldg_nt((const f32x4 *)(base + j + 4));
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                u[k] = w0[k] - b0[k];
                u[4 + k] = w1[k] - b1[k];
            }
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) u[k] = 0.f;
        }
        float n;
        if constexpr (NORM == DLS_QSGD_MAX) {
            uint32_t m = 0;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const uint32_t a = __float_as_uint(u[k]) & 0x7fffffffu;
                nbad += a >= 0x7f800000u;
                m = a > m ? a : m;
            }
            n = __uint_as_float(wave_max(m));
        } else {
            double sq = 0.0;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                nbad += (__float_as_uint(u[k]) & 0x7fffffffu) >= 0x7f800000u;
                const double y = (double)u[k];
                sq += y * y;
            }
            n = (float)__builtin_sqrt(wave_sum(sq));
        }
        const float r = div_ieee(fS, n), d = div_ieee(n, fS);
        // 0 < n < inf: the bucket carries codes
        const bool coded = (__float_as_uint(n) - 1u) < 0x7f7fffffu;
        const u32x4 x0 = philox_block(2 * (uint64_t)g, key), x1 = philox_block(2 * (uint64_t)g + 1, key);
        uint32_t lo = 0, hi = 0;  // fields 0-3 and 4-7 at B = 8; all eight in lo below that
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint32_t word = k < 4 ? x0[k & 3] : x1[k & 3];
            const float xi = (float)(word >> 8) * 0x1p-24f;
            const float t = __builtin_fabsf(u[k]) * r;
            const float l0 = __builtin_floorf(t);
            const float f = t - l0;
            float l = l0 + (xi < f ? 1.f : 0.f);
            l = l < fS ? l : fS;
            const int li = (int)l;
            const uint32_t field = (uint32_t)(u[k] < 0.f ? -li : li) & ((1u << B) - 1u);
            if (B == 8 && k >= 4)
                hi |= field << (B * (k - 4));
            else
                lo |= field << (B * k);
        }
        if (!coded) lo = hi = 0;
        if constexpr (B == 8) {
            typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
            *(u32x2 *)(codes + 2 * g) = (u32x2){lo, hi};
        } else if constexpr (B == 4) {
            codes[g] = lo;
        } else {
            const uint32_t other = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)lo, 0xB1, 0xf, 0xf,
                                                                         false);  // lane ^ 1
            if (!(lane & 1)) codes[g >> 1] = lo | (other << 16);
        }
        if (lane == 0) scales[bucket] = d;
        nbad = wave_sum(nbad);
    }
    if (lane == 0) lbad[wave] = nbad;
    __syncthreads();
    if (threadIdx.x == 0) {
        nbad = lbad[0] + lbad[1] + lbad[2] + lbad[3];
        const unsigned long long before = atomicAdd(cell, (1ull << 32) | nbad);
        if ((before >> 32) == gridDim.x - 1) {  // every other workgroup's count is in `before`
            stats[0] = (int32_t)((uint32_t)before + nbad);
            atomicExch(cell, 0ull);
        }
    }
}

// the 8 B bits of a lane's eight fields of one client's code row
template <int B>
struct Fields {
    uint32_t lo, hi;
};

// client i of the tile that starts at `tile`; a client past the tile's last (a wave-uniform
// test) is not loaded and never applied
template <int B>
__device__ __forceinline__ Fields<B> load_fields(const uint32_t *tile, int64_t ldc, int i, int nb,
                                                 int64_t g) {
    Fields<B> v{0, 0};
    if (i >= nb) return v;
    const uint32_t *row = tile + (int64_t)i * ldc;
    if constexpr (B == 8) {
        typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
        const u32x2 p = ldg_nt((const u32x2 *)(row + 2 * g));
        v.lo = p[0];
        v.hi = p[1];
    } else if constexpr (B == 4) {
        v.lo = ldg_nt(row + g);
    } else {
        v.lo = ldg_nt((const uint16_t *)row + g);
    }
    return v;
}

// acc[k] = fl(acc[k] + fl((float)q[k] * c))
template <int B>
__device__ __forceinline__ void add_client(float (&acc)[8], const Fields<B> &v, float c) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const uint32_t word = (B == 8 && k >= 4) ? v.hi : v.lo;
        const int q = __builtin_amdgcn_sbfe((int)word, (B * k) & 31, B);  // v_bfe_i32
        acc[k] = acc[k] + (float)q * c;
    }
}

template <int B>
__global__ __launch_bounds__(kBlock) void k_qsgd_fedavg(
    const float *__restrict__ base, const uint32_t *__restrict__ codes, int64_t ldc,
    const float *__restrict__ scales, int64_t lds, const float *__restrict__ weight, FastDiv d,
    int K, int64_t P, int64_t NB, float *__restrict__ out) {
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = lane_id();
    const int64_t bucket = (int64_t)blockIdx.x * kWaves + wave;
    if (bucket >= NB) return;
    const int64_t g = bucket * 64 + lane, j = 8 * g;
    float acc[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = -0.f;
    for (int k0 = 0; k0 < K; k0 += kTileK) {
        const int nb = K - k0 < kTileK ? K - k0 : kTileK;
        float c = 0.f;  // lane i: c[k0 + i][bucket]
        if (lane < nb)
            c = div_exact(scales[(int64_t)(k0 + lane) * lds + bucket] * weight[k0 + lane], d);
        const uint32_t *row = codes + (int64_t)k0 * ldc;
        Fields<B> cur[kAhead], nxt[kAhead];
#pragma unroll
        for (int a = 0; a < kAhead; ++a) cur[a] = load_fields<B>(row, ldc, a, nb, g);
        for (int i0 = 0; i0 < nb; i0 += kAhead) {
#pragma unroll
            for (int a = 0; a < kAhead; ++a) nxt[a] = load_fields<B>(row, ldc, i0 + kAhead + a, nb, g);
#pragma unroll
            for (int a = 0; a < kAhead; ++a) {
                if (i0 + a < nb)
                    add_client<B>(acc, cur[a], __int_as_float(__builtin_amdgcn_readlane(
                                                   __float_as_int(c), i0 + a)));
                cur[a] = nxt[a];
            }
        }
    }
    if (j < P) {
        const f32x4 b0 = ldg_nt((const f32x4 *)(base + j)), b1 = ldg_nt((const f32x4 *)(base + j + 4));
        f32x4 o0, o1;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            o0[k] = b0[k] + acc[k];
            o1[k] = b1[k] + acc[4 + k];
        }
        *(f32x4 *)(out + j) = o0;
        *(f32x4 *)(out + j + 4) = o1;
    }
}

// [a, a + na) and [b, b + nb) bytes intersect
inline bool overlap(const void *a, int64_t na, const void *b, int64_t nb) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + (uintptr_t)nb && b0 < a0 + (uintptr_t)na;
}

inline int64_t buckets_of(int64_t P) { return (P + kBucket - 1) / kBucket; }

template <int B>
void launch_compress(int norm, unsigned grid, hipStream_t st, const float *w, const float *base,
                     int64_t P, int64_t NB, PhiloxKey key, uint32_t *codes, float *scales,
                     int32_t *stats, unsigned long long *cell) {
    if (norm == DLS_QSGD_MAX)
        hipLaunchKernelGGL((k_qsgd_compress<B, DLS_QSGD_MAX>), dim3(grid), dim3(kBlock), 0, st, w,
                           base, P, NB, key, codes, scales, stats, cell);
    else
        hipLaunchKernelGGL((k_qsgd_compress<B, DLS_QSGD_L2>), dim3(grid), dim3(kBlock), 0, st, w,
                           base, P, NB, key, codes, scales, stats, cell);
}

}  // namespace
}  // namespace dls

using namespace dls;

extern "C" int dls_qsgd_compress_f32(const float *w, const float *base, int64_t P, int32_t bits,
                                     int32_t norm, uint64_t seed, uint64_t stream_id,
                                     uint32_t *codes, float *scales, int32_t *stats,
                                     dls_stream_t stream) {
    const char *fn = "dls_qsgd_compress_f32";
    DLS_REQUIRE(w && base && codes && scales && stats, DLS_EINVAL,
                "%s: null pointer (w, base, codes, scales, stats)", fn);
    DLS_REQUIRE(bits == 2 || bits == 4 || bits == 8, DLS_EINVAL, "%s: bits=%d (2, 4 or 8)", fn, bits);
    DLS_REQUIRE(norm == DLS_QSGD_MAX || norm == DLS_QSGD_L2, DLS_EINVAL,
                "%s: norm=%d (DLS_QSGD_MAX or DLS_QSGD_L2)", fn, norm);
    DLS_REQUIRE(P >= 64 && P < kMaxP, DLS_EINVAL, "%s: P=%lld (64 <= P < 2^31)", fn, (long long)P);
    DLS_REQUIRE(P % 64 == 0, DLS_ELAYOUT, "%s: P=%lld must be a multiple of 64", fn, (long long)P);
    DLS_REQUIRE(aligned16(w) && aligned16(base) && aligned16(codes) && aligned16(scales) &&
                    aligned16(stats),
                DLS_ELAYOUT, "%s: 16-byte alignment of w, base, codes, scales and stats", fn);
    const int64_t NB = buckets_of(P), cb = NB * 64 * bits;  // the code row's bytes
    DLS_REQUIRE(!overlap(codes, cb, w, 4 * P) && !overlap(codes, cb, base, 4 * P) &&
                    !overlap(scales, 4 * NB, w, 4 * P) && !overlap(scales, 4 * NB, base, 4 * P) &&
                    !overlap(stats, 4, w, 4 * P) && !overlap(stats, 4, base, 4 * P),
                DLS_EINVAL, "%s: codes, scales and stats must not alias w or base", fn);
    unsigned long long *cell = stream_cell(as_stream(stream));
    DLS_REQUIRE(cell, DLS_EINVAL, "%s: no device memory for the stream's counter cell", fn);
    const unsigned grid = (unsigned)((NB + kWaves - 1) / kWaves);
    const PhiloxKey key = make_key(seed, stream_id);
    if (bits == 2)
        launch_compress<2>(norm, grid, as_stream(stream), w, base, P, NB, key, codes, scales, stats, cell);
    else if (bits == 4)
        launch_compress<4>(norm, grid, as_stream(stream), w, base, P, NB, key, codes, scales, stats, cell);
    else
        launch_compress<8>(norm, grid, as_stream(stream), w, base, P, NB, key, codes, scales, stats, cell);
    return check_launch(fn);
}

extern "C" int dls_qsgd_fedavg_f32(const float *base, const uint32_t *codes, int64_t ldc,
                                   const float *scales, int64_t lds, const float *weight,
                                   float total, int32_t K, int64_t P, int32_t bits, float *out,
                                   dls_stream_t stream) {
    const char *fn = "dls_qsgd_fedavg_f32";
    DLS_REQUIRE(base && codes && scales && weight && out, DLS_EINVAL,
                "%s: null pointer (base, codes, scales, weight, out)", fn);
    DLS_REQUIRE(bits == 2 || bits == 4 || bits == 8, DLS_EINVAL, "%s: bits=%d (2, 4 or 8)", fn, bits);
    DLS_REQUIRE(K >= 1, DLS_EINVAL, "%s: K=%d (K >= 1)", fn, K);
    DLS_REQUIRE(P >= 64 && P < kMaxP, DLS_EINVAL, "%s: P=%lld (64 <= P < 2^31)", fn, (long long)P);
    DLS_REQUIRE(P % 64 == 0, DLS_ELAYOUT, "%s: P=%lld must be a multiple of 64", fn, (long long)P);
    const int64_t NB = buckets_of(P);
    DLS_REQUIRE(ldc >= NB * 16 * bits && ldc % 4 == 0 && lds >= NB, DLS_ELAYOUT,
                "%s: ldc=%lld must be a multiple of 4, at least 16 bits NB = %lld, and lds=%lld at "
                "least NB = %lld",
                fn, (long long)ldc, (long long)(NB * 16 * bits), (long long)lds, (long long)NB);
    DLS_REQUIRE(aligned16(base) && aligned16(codes) && aligned16(scales) && aligned16(weight) &&
                    aligned16(out),
                DLS_ELAYOUT, "%s: 16-byte alignment of base, codes, scales, weight and out", fn);
    DLS_REQUIRE(!overlap(out, 4 * P, base, 4 * P), DLS_EINVAL, "%s: out must not alias base", fn);
    const dim3 grid((unsigned)((NB + kWaves - 1) / kWaves));
    const FastDiv d = make_fastdiv(total);
    if (bits == 2)
        hipLaunchKernelGGL(k_qsgd_fedavg<2>, grid, dim3(kBlock), 0, as_stream(stream), base, codes,
                           ldc, scales, lds, weight, d, (int)K, P, NB, out);
    else if (bits == 4)
        hipLaunchKernelGGL(k_qsgd_fedavg<4>, grid, dim3(kBlock), 0, as_stream(stream), base, codes,
                           ldc, scales, lds, weight, d, (int)K, P, NB, out);
    else
        hipLaunchKernelGGL(k_qsgd_fedavg<8>, grid, dim3(kBlock), 0, as_stream(stream), base, codes,
                           ldc, scales, lds, weight, d, (int)K, P, NB, out);
    return check_launch(fn);
}
