// OCP Microscaling update compression for gfx950 (Rouhani et al. 2023, "Microscaling Data
// Formats for Deep Learning"; the OCP MX v1.0 specification): the client's compressor and the
// server's FedAvg over FP8 (E4M3, E5M2) and FP4 (E2M1) codes with one power-of-two scale per
// block of 32 coordinates.  include/dls_hip.h has the contract.
//
// Both kernels give one wave to one group of 512 coordinates and four groups to a 256-thread
// workgroup; a lane owns the 8 consecutive coordinates 8 g .. 8 g + 7 of its global lane index
// g = 64 group + lane, as in qsgd.hip.  So
//   - w, base and the residual come as two 16-byte loads each;
//   - a block of 32 coordinates is one aligned quad of lanes: the block's largest |u| pattern is
//     an integer max over two DPP quad permutes, and lane 0 of the quad stores the scale byte;
//   - the lane's Philox words are the blocks 2 g and 2 g + 1 whole (stochastic rounding only);
//   - the lane's eight codes are one uint32 at FP4 and two at FP8.
//
// The compressor's encode is integer arithmetic on the fp32 pattern of |u|: the significand is
// shifted right by the distance between its own last place and the element grid's step at t =
// |u| 2^-e, the bits shifted out are the fraction f exactly, and the code is (exponent field <<
// M) + quotient + round-up, which carries into the next binade by itself.  No float operation
// rounds on the way, so the rule of the contract holds for denormal inputs and for every scale.
// The hardware encodes (v_cvt_scalef32_pk_fp8_f32, .._pk_fp4_f32 and their sr forms) are not
// used: their saturation and the sr forms' random-bit convention are not established against
// the contract, and the encode does not bound the kernel.
//
// The server decodes with the hardware conversions v_cvt_scalef32_pk_f32_fp8 / _bf8 / _fp4: two
// fp32 values from two codes with the block's scale applied, exact for every scale byte 0..254
// and every code the compressor emits, denormal results included.  The scale operand is an fp32
// whose exponent field is the E8M0 byte: byte << 23.  Lane i of a tile of 64 clients loads
// client i's 16 scale bytes of the wave's group with one 16-byte load and forms c[i]; the client
// loop reads both back with v_readlane, each lane picks its block's byte.  kAhead clients' code
// loads are in flight ahead of the chain.  The accumulator starts as -0.0 (qsgd.hip).
//
// The compressor's count of non-finite coordinates goes through the per-stream cell of
// dls_drive_compress_f32 (drive.hip has the protocol); its 16 bytes of LDS and the one barrier
// before the ticket are the only ones here.
#include "philox_common.h"

namespace dls {
namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kGroup = DLS_MX_GROUP;          // coordinates per wave, 8 per lane
constexpr int kTileK = DLS_MX_CLIENT_TILE;    // clients per scale and c table (one per lane)
constexpr int kAhead = 8;                     // clients whose code loads are in flight
constexpr int64_t kMaxP = (int64_t)1 << 31;
static_assert(kGroup == 512 && kTileK == 64 && DLS_MX_BLOCK == 32,
              "a lane owns 8 coordinates, a quad one block, a lane one client's scales");

typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// M mantissa bits, the exponents of the largest and the least normal, the mantissa field of
// fmax as an fp32, the code's width
template <int FMT>
struct Format;
template <>
struct Format<DLS_MX_E4M3> {
    static constexpr int M = 3, EMAX = 8, EMIN = -6, BITS = 8;
    static constexpr uint32_t MF = 0x600000u;  // 448 = 1.75 * 2^8
};
template <>
struct Format<DLS_MX_E5M2> {
    static constexpr int M = 2, EMAX = 15, EMIN = -14, BITS = 8;
    static constexpr uint32_t MF = 0x600000u;  // 57344 = 1.75 * 2^15
};
template <>
struct Format<DLS_MX_E2M1> {
    static constexpr int M = 1, EMAX = 2, EMIN = 0, BITS = 4;
    static constexpr uint32_t MF = 0x400000u;  // 6 = 1.5 * 2^2
};

__device__ __forceinline__ uint32_t quad_max(uint32_t v) {
    uint32_t o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xf, 0xf, false);  // lane ^ 1
    v = o > v ? o : v;
    o = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xf, 0xf, false);  // lane ^ 2
    return o > v ? o : v;
}

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// The code of u under the block exponent e, and its exact decode.  With |u| = sig 2^ex (sig the
// 24-bit significand, top bit tb) the element grid's step at t = |u| 2^-e is 2^(sh + ex - e):
// sig >> sh is the grid index, the bits below it are f.
template <int FMT, int ROUND>
__device__ __forceinline__ uint32_t encode(float u, int e, uint32_t word, float &dec) {
    typedef Format<FMT> F;
    const uint32_t bits = __float_as_uint(u), a = bits & 0x7fffffffu;
    const int E = (int)(a >> 23);
    const uint32_t sig = E ? (a & 0x7fffffu) | 0x800000u : a;
    const int ex = (E ? E : 1) - 150;
    const int tb = 31 - (int)__builtin_clz(sig | 1u) - (sig ? 0 : 1);
    const int te = tb + ex - e;  // floor(log2 t)
    const int lo = F::EMIN - F::M + e - ex;
    const int sh = tb - F::M > lo ? tb - F::M : lo;  // >= 6
    const int eb = te > F::EMIN ? te - F::EMIN : 0;
    uint32_t n, up;
    if constexpr (ROUND == DLS_MX_NEAREST) {
        const int sn = sh < 25 ? sh : 25;  // sig < 2^24: from 25 on the quotient is 0, rounded down
        n = sig >> sn;
        const uint32_t rem = sig & ((1u << sn) - 1u), half = 1u << (sn - 1);
        up = (rem > half || (rem == half && (n & 1u))) ? 1u : 0u;
    } else {
        const int s1 = sh < 24 ? sh : 24;
        n = sig >> s1;
        const uint32_t rem = sig & ((1u << s1) - 1u);
        int k = sh - 24;  // f = rem 2^-sh: xi < f  <=>  (word >> 8) < ceil(rem 2^(24 - sh))
        k = k < 0 ? 0 : (k > 31 ? 31 : k);
        const uint32_t T = ((rem + ((1u << k) - 1u)) >> k) << (24 - s1);
        up = (word >> 8) < T ? 1u : 0u;
    }
    const uint32_t nn = n + up;
    dec = __uint_as_float(__float_as_uint(__builtin_ldexpf((float)nn, sh + ex)) | (bits & 0x80000000u));
    return ((bits >> 31) << (F::BITS - 1)) | (((uint32_t)eb << F::M) + nn);
}

template <int FMT, int ROUND>
__global__ __launch_bounds__(kBlock) void k_mx_compress(
    const float *__restrict__ w, const float *__restrict__ base, float *residual, int64_t P,
    int64_t NG, PhiloxKey key, uint32_t *__restrict__ codes, uint8_t *__restrict__ scales,
    int32_t *__restrict__ stats, unsigned long long *cell) {
    typedef Format<FMT> F;
    __shared__ uint32_t lbad[kWaves];
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = lane_id();
    const int64_t group = (int64_t)blockIdx.x * kWaves + wave;
    uint32_t nbad = 0;
    if (group < NG) {
        const int64_t g = group * 64 + lane, j = 8 * g;
        const bool live = j < P;  // P is a multiple of 64: a lane's eight lie inside together
        float u[8];
        if (live) {
            const f32x4 w0 = ldg_nt((const f32x4 *)(w + j)), w1 = ldg_nt((const f32x4 *)(w + j + 4));
            const f32x4 b0 = ldg_nt((const f32x4 *)(base + j)),
                        b1 = ldg_nt((const f32x4 *)(base + j + 4));
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                u[k] = w0[k] - b0[k];
                u[4 + k] = w1[k] - b1[k];
            }
            if (residual) {
                const f32x4 r0 = *(const f32x4 *)(residual + j), r1 = *(const f32x4 *)(residual + j + 4);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    u[k] = u[k] + r0[k];
                    u[4 + k] = u[4 + k] + r1[k];
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < 8; ++k) u[k] = 0.f;
        }
        uint32_t m = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint32_t a = __float_as_uint(u[k]) & 0x7fffffffu;
            nbad += a >= 0x7f800000u;
            m = a > m ? a : m;
        }
        m = quad_max(m);
        const bool finite = m < 0x7f800000u;
        int e = (int)(m >> 23) - 127 - F::EMAX + ((m & 0x7fffffu) > F::MF ? 1 : 0);
        e = e < -127 ? -127 : e;
        u32x4 x0 = {0, 0, 0, 0}, x1 = {0, 0, 0, 0};
        if constexpr (ROUND == DLS_MX_STOCHASTIC) {
            x0 = philox_block(2 * (uint64_t)g, key);
            x1 = philox_block(2 * (uint64_t)g + 1, key);
        }
        uint32_t lo = 0, hi = 0;  // codes 0-3 and 4-7 at 8 bits; all eight in lo at 4
        float d[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const uint32_t code = encode<FMT, ROUND>(u[k], e, k < 4 ? x0[k & 3] : x1[k & 3], d[k]);
            if (F::BITS == 8 && k >= 4)
                hi |= code << (8 * (k - 4));
            else
                lo |= code << (F::BITS * k);
        }
        if (!finite) {
            lo = hi = 0;
#pragma unroll
            for (int k = 0; k < 8; ++k) d[k] = 0.f;
        }
        if constexpr (F::BITS == 8)
            *(u32x2 *)(codes + 2 * g) = (u32x2){lo, hi};
        else
            codes[g] = lo;
        if (!(lane & 3)) scales[group * 16 + (lane >> 2)] = finite ? (uint8_t)(e + 127) : (uint8_t)255;
        if (live && residual) {
            f32x4 r0, r1;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                r0[k] = finite ? u[k] - d[k] : u[k];
                r1[k] = finite ? u[4 + k] - d[4 + k] : u[4 + k];
            }
            *(f32x4 *)(residual + j) = r0;
            *(f32x4 *)(residual + j + 4) = r1;
        }
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

// a lane's eight codes of one client's code row
struct Codes {
    uint32_t lo, hi;
};

// client i of the tile that starts at `tile`; a client past the tile's last (a wave-uniform
// test) is not loaded and never applied
template <int BITS>
__device__ __forceinline__ Codes load_codes(const uint32_t *tile, int64_t ldc, int i, int nb,
                                            int64_t g) {
    Codes v{0, 0};
    if (i >= nb) return v;
    const uint32_t *row = tile + (int64_t)i * ldc;
    if constexpr (BITS == 8) {
        const u32x2 p = ldg_nt((const u32x2 *)(row + 2 * g));
        v.lo = p[0];
        v.hi = p[1];
    } else {
        v.lo = ldg_nt(row + g);
    }
    return v;
}

// the lane's eight exact decodes code * 2^e; `scale` holds the E8M0 byte in its exponent field
template <int FMT>
__device__ __forceinline__ void decode8(const Codes &v, float scale, float (&x)[8]) {
    f32x2 p[4];
    if constexpr (FMT == DLS_MX_E4M3) {
        p[0] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8((int)v.lo, scale, false);
        p[1] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8((int)v.lo, scale, true);
        p[2] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8((int)v.hi, scale, false);
        p[3] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8((int)v.hi, scale, true);
    } else if constexpr (FMT == DLS_MX_E5M2) {
        p[0] = __builtin_amdgcn_cvt_scalef32_pk_f32_bf8((int)v.lo, scale, false);
        p[1] = __builtin_amdgcn_cvt_scalef32_pk_f32_bf8((int)v.lo, scale, true);
        p[2] = __builtin_amdgcn_cvt_scalef32_pk_f32_bf8((int)v.hi, scale, false);
        p[3] = __builtin_amdgcn_cvt_scalef32_pk_f32_bf8((int)v.hi, scale, true);
    } else {
        p[0] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(v.lo, scale, 0);
        p[1] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(v.lo, scale, 1);
        p[2] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(v.lo, scale, 2);
        p[3] = __builtin_amdgcn_cvt_scalef32_pk_f32_fp4(v.lo, scale, 3);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        x[2 * k] = p[k][0];
        x[2 * k + 1] = p[k][1];
    }
}

__device__ __forceinline__ uint32_t readlane(uint32_t v, int i) {
    return (uint32_t)__builtin_amdgcn_readlane((int)v, i);
}

template <int FMT>
__global__ __launch_bounds__(kBlock) void k_mx_fedavg(
    const float *__restrict__ base, const uint32_t *__restrict__ codes, int64_t ldc,
    const uint8_t *__restrict__ scales, int64_t lds, const float *__restrict__ weight, FastDiv d,
    int K, int64_t P, int64_t NG, float *__restrict__ out) {
    constexpr int BITS = Format<FMT>::BITS;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = lane_id();
    const int64_t group = (int64_t)blockIdx.x * kWaves + wave;
    if (group >= NG) return;
    const int64_t g = group * 64 + lane, j = 8 * g;
    const int dword = lane >> 4, shift = 8 * ((lane >> 2) & 3);  // the block's byte of 16
    float acc[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = -0.f;
    for (int k0 = 0; k0 < K; k0 += kTileK) {
        const int nb = K - k0 < kTileK ? K - k0 : kTileK;
        float c = 0.f;               // lane i: c[k0 + i]
        u32x4 sc = {0, 0, 0, 0};     // lane i: client k0 + i's 16 scale bytes of this group
        if (lane < nb) {
            c = div_exact(weight[k0 + lane], d);
            sc = *(const u32x4 *)(scales + (int64_t)(k0 + lane) * lds + group * 16);
        }
        const uint32_t *row = codes + (int64_t)k0 * ldc;
        Codes cur[kAhead], nxt[kAhead];
#pragma unroll
        for (int a = 0; a < kAhead; ++a) cur[a] = load_codes<BITS>(row, ldc, a, nb, g);
        for (int i0 = 0; i0 < nb; i0 += kAhead) {
#pragma unroll
            for (int a = 0; a < kAhead; ++a) nxt[a] = load_codes<BITS>(row, ldc, i0 + kAhead + a, nb, g);
#pragma unroll
            for (int a = 0; a < kAhead; ++a) {
                if (i0 + a < nb) {
                    const int i = i0 + a;
                    const uint32_t s0 = readlane(sc[0], i), s1 = readlane(sc[1], i),
                                   s2 = readlane(sc[2], i), s3 = readlane(sc[3], i);
                    const uint32_t dw = dword == 0 ? s0 : dword == 1 ? s1 : dword == 2 ? s2 : s3;
                    const float scale = __uint_as_float(((dw >> shift) & 0xffu) << 23);
                    const float ci = __uint_as_float(readlane(__float_as_uint(c), i));
                    float x[8];
                    decode8<FMT>(cur[a], scale, x);
#pragma unroll
                    for (int k = 0; k < 8; ++k) acc[k] = acc[k] + x[k] * ci;
                }
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

inline int64_t groups_of(int64_t P) { return (P + kGroup - 1) / kGroup; }
inline bool format_ok(int32_t f) { return f == DLS_MX_E4M3 || f == DLS_MX_E5M2 || f == DLS_MX_E2M1; }
inline int code_bits(int32_t f) { return f == DLS_MX_E2M1 ? 4 : 8; }

template <int FMT>
void launch_compress(int rounding, unsigned grid, hipStream_t st, const float *w, const float *base,
                     float *residual, int64_t P, int64_t NG, PhiloxKey key, uint32_t *codes,
                     uint8_t *scales, int32_t *stats, unsigned long long *cell) {
    if (rounding == DLS_MX_NEAREST)
        hipLaunchKernelGGL((k_mx_compress<FMT, DLS_MX_NEAREST>), dim3(grid), dim3(kBlock), 0, st, w,
                           base, residual, P, NG, key, codes, scales, stats, cell);
    else
        hipLaunchKernelGGL((k_mx_compress<FMT, DLS_MX_STOCHASTIC>), dim3(grid), dim3(kBlock), 0, st,
                           w, base, residual, P, NG, key, codes, scales, stats, cell);
}

}  // namespace
}  // namespace dls

using namespace dls;

extern "C" int dls_mx_compress_f32(const float *w, const float *base, float *residual, int64_t P,
                                   int32_t format, int32_t rounding, uint64_t seed,
                                   uint64_t stream_id, uint32_t *codes, uint8_t *scales,
                                   int32_t *stats, dls_stream_t stream) {
    const char *fn = "dls_mx_compress_f32";
    DLS_REQUIRE(w && base && codes && scales && stats, DLS_EINVAL,
                "%s: null pointer (w, base, codes, scales, stats)", fn);
    DLS_REQUIRE(format_ok(format), DLS_EINVAL,
                "%s: format=%d (DLS_MX_E4M3, DLS_MX_E5M2 or DLS_MX_E2M1)", fn, format);
    DLS_REQUIRE(rounding == DLS_MX_NEAREST || rounding == DLS_MX_STOCHASTIC, DLS_EINVAL,
                "%s: rounding=%d (DLS_MX_NEAREST or DLS_MX_STOCHASTIC)", fn, rounding);
    DLS_REQUIRE(P >= 64 && P < kMaxP, DLS_EINVAL, "%s: P=%lld (64 <= P < 2^31)", fn, (long long)P);
    DLS_REQUIRE(P % 64 == 0, DLS_ELAYOUT, "%s: P=%lld must be a multiple of 64", fn, (long long)P);
    DLS_REQUIRE(aligned16(w) && aligned16(base) && aligned16(residual) && aligned16(codes) &&
                    aligned16(scales) && aligned16(stats),
                DLS_ELAYOUT, "%s: 16-byte alignment of w, base, residual, codes, scales and stats",
                fn);
    const int64_t NG = groups_of(P), cb = NG * 64 * code_bits(format), sb = NG * 16;
    const void *in[3] = {w, base, residual};
    for (int i = 0; i < (residual ? 3 : 2); ++i)
        DLS_REQUIRE(!overlap(codes, cb, in[i], 4 * P) && !overlap(scales, sb, in[i], 4 * P) &&
                        !overlap(stats, 4, in[i], 4 * P),
                    DLS_EINVAL, "%s: codes, scales and stats must not alias w, base or residual", fn);
    DLS_REQUIRE(!residual || (!overlap(residual, 4 * P, w, 4 * P) &&
                              !overlap(residual, 4 * P, base, 4 * P)),
                DLS_EINVAL, "%s: residual must not alias w or base", fn);
    unsigned long long *cell = stream_cell(as_stream(stream));
    DLS_REQUIRE(cell, DLS_EINVAL, "%s: no device memory for the stream's counter cell", fn);
    const unsigned grid = (unsigned)((NG + kWaves - 1) / kWaves);
    const PhiloxKey key = make_key(seed, stream_id);
    hipStream_t st = as_stream(stream);
    if (format == DLS_MX_E4M3)
        launch_compress<DLS_MX_E4M3>(rounding, grid, st, w, base, residual, P, NG, key, codes, scales, stats, cell);
    else if (format == DLS_MX_E5M2)
        launch_compress<DLS_MX_E5M2>(rounding, grid, st, w, base, residual, P, NG, key, codes, scales, stats, cell);
    else
        launch_compress<DLS_MX_E2M1>(rounding, grid, st, w, base, residual, P, NG, key, codes, scales, stats, cell);
    return check_launch(fn);
}

extern "C" int dls_mx_fedavg_f32(const float *base, const uint32_t *codes, int64_t ldc,
                                 const uint8_t *scales, int64_t lds, const float *weight,
                                 float total, int32_t K, int64_t P, int32_t format, float *out,
                                 dls_stream_t stream) {
    const char *fn = "dls_mx_fedavg_f32";
    DLS_REQUIRE(base && codes && scales && weight && out, DLS_EINVAL,
                "%s: null pointer (base, codes, scales, weight, out)", fn);
    DLS_REQUIRE(format_ok(format), DLS_EINVAL,
                "%s: format=%d (DLS_MX_E4M3, DLS_MX_E5M2 or DLS_MX_E2M1)", fn, format);
    DLS_REQUIRE(K >= 1, DLS_EINVAL, "%s: K=%d (K >= 1)", fn, K);
    DLS_REQUIRE(P >= 64 && P < kMaxP, DLS_EINVAL, "%s: P=%lld (64 <= P < 2^31)", fn, (long long)P);
    DLS_REQUIRE(P % 64 == 0, DLS_ELAYOUT, "%s: P=%lld must be a multiple of 64", fn, (long long)P);
    const int64_t NG = groups_of(P), words = NG * 16 * code_bits(format);
    DLS_REQUIRE(ldc >= words && ldc % 4 == 0 && lds >= NG * 16 && lds % 16 == 0, DLS_ELAYOUT,
                "%s: ldc=%lld must be a multiple of 4 words, at least %lld, and lds=%lld a multiple "
                "of 16 bytes, at least %lld",
                fn, (long long)ldc, (long long)words, (long long)lds, (long long)(NG * 16));
    DLS_REQUIRE(aligned16(base) && aligned16(codes) && aligned16(scales) && aligned16(weight) &&
                    aligned16(out),
                DLS_ELAYOUT, "%s: 16-byte alignment of base, codes, scales, weight and out", fn);
    DLS_REQUIRE(!overlap(out, 4 * P, base, 4 * P), DLS_EINVAL, "%s: out must not alias base", fn);
    const dim3 grid((unsigned)((NG + kWaves - 1) / kWaves));
    const FastDiv d = make_fastdiv(total);
    hipStream_t st = as_stream(stream);
    if (format == DLS_MX_E4M3)
        hipLaunchKernelGGL(k_mx_fedavg<DLS_MX_E4M3>, grid, dim3(kBlock), 0, st, base, codes, ldc,
                           scales, lds, weight, d, (int)K, P, NG, out);
    else if (format == DLS_MX_E5M2)
        hipLaunchKernelGGL(k_mx_fedavg<DLS_MX_E5M2>, grid, dim3(kBlock), 0, st, base, codes, ldc,
                           scales, lds, weight, d, (int)K, P, NG, out);
    else
        hipLaunchKernelGGL(k_mx_fedavg<DLS_MX_E2M1>, grid, dim3(kBlock), 0, st, base, codes, ldc,
                           scales, lds, weight, d, (int)K, P, NG, out);
    return check_launch(fn);
}
