// Rotated one-bit compression for gfx950 (Suresh, Yu, Kumar & McMahan 2017, "Distributed
// mean estimation with limited communication"; Vargaftik et al. 2021, "DRIVE: one-bit
// distributed mean estimation"): a randomised Walsh-Hadamard rotation over blocks of 4096
// coordinates, the client's compressor and the server's FedAvg over bit rows in the
// rotated domain.  include/dls_hip.h has the contract.
//
// One transform device function, hadamard(), serves the three entry points.  A 256-thread
// block owns one block of 4096 coordinates and holds it in registers: of the index
//   bits 0-5   the lane,
//   bits 6-9   the thread's register r (0..15),
//   bits 10-11 the wave,
// so a wave's register r is the 64 coordinates of bit word 16 wave + r of the block: in
// the compressor the word is the wave's ballot, in the FedAvg a client's word is the wave's
// lane mask (k_efsign_fedavg's walk), and the 64 signs of the word are two Philox words
// that one lane draws and the wave reads as a lane mask.  The stages in ascending order:
//   h = 1, 2, 4, 8   across lanes: the partner's value comes by DPP (quad_perm for 1 and 2,
//                    two bank-masked row shifts for 4, row_ror:8 for 8), the own value has
//                    its sign flipped where the lane is the upper of its pair, one v_add
//   h = 16, 32       v_permlane16_swap / v_permlane32_swap on register pairs: a swap puts
//                    both halves of two butterflies into the same lanes of two registers,
//                    one v_add and one v_sub, and a second swap puts them back
//   h = 64 .. 512    between the thread's own registers
//   h = 1024, 2048   one exchange between the four waves through 16 KB of LDS: every thread
//                    stores its 16 values as four 16-byte vectors, reads the four waves'
//                    values of its (register, lane) and keeps its wave's output of both
//                    stages
// DLS_DRIVE_XLANE=0 builds the cross-lane stages on __shfl_xor (ds_bpermute) instead; DESIGN.md
// has both timings.  x - y is computed as x + (-y) wherever that saves a select: the same
// bits for every finite result.
//
// dls_drive_compress_f32's count of non-finite coordinates is the one number of the call
// that blocks share.  They meet in one 64-bit cell that the library keeps per HIP stream
// (calls on one stream are ordered): a block adds (1 << 32) + its count with one integer
// atomic, tickets in the high word and the count in the low one (it stays below 2^31), and
// the block that finds gridDim.x - 1 tickets taken stores the sum to stats[0] and leaves
// the cell zero for the next call.  Nothing else passes between blocks, so there is no fence
// (on a multi-die part a device-scope release writes the die's L2 back: with a fence per
// block the compressor took 128 us on the ResNet-18 row instead of 48).
#include "philox_common.h"

#ifndef DLS_DRIVE_XLANE
#define DLS_DRIVE_XLANE 1
#endif

namespace dls {
namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kD = DLS_DRIVE_BLOCK;             // coordinates per rotation block
constexpr int kWords = kD / 64;                 // bit words per block
constexpr int kRegs = kD / kBlock;              // 16 coordinates (registers) per thread
constexpr int kTileK = DLS_DRIVE_CLIENT_TILE;   // clients per c table in LDS
constexpr int64_t kMaxP = (int64_t)1 << 31;
static_assert(kD == 4096 && kRegs == 16, "the ownership above and the exact 2^-6");

__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

__device__ __forceinline__ float flip(float v, uint32_t signbit) {
    return __uint_as_float(__float_as_uint(v) ^ signbit);
}

#if DLS_DRIVE_XLANE
template <int CTRL, int BANKS>
__device__ __forceinline__ float dpp(float old, float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(old), __float_as_int(v), CTRL,
                                                      0xf, BANKS, false));
}
#endif

// the value lane ^ H holds of v, H = 1, 2, 4, 8
template <int H>
__device__ __forceinline__ float partner(float v) {
#if DLS_DRIVE_XLANE
    if constexpr (H == 1) return dpp<0xB1, 0xf>(v, v);  // quad_perm:[1,0,3,2]
    if constexpr (H == 2) return dpp<0x4E, 0xf>(v, v);  // quad_perm:[2,3,0,1]
    if constexpr (H == 4)  // row_shl:4 into the banks 0 and 2, row_shr:4 into 1 and 3
        return dpp<0x114, 0xA>(dpp<0x104, 0x5>(v, v), v);
    if constexpr (H == 8) return dpp<0x128, 0xf>(v, v);  // row_ror:8
#else
    return __shfl_xor(v, H, 64);
#endif
}

// (a, b) -> (fl(a + b), fl(a - b)) on the lane pairs (l, l ^ H) of every register
template <int H>
__device__ __forceinline__ void lane_stage(float (&v)[kRegs], int lane) {
    const uint32_t upper = (lane & H) ? 0x80000000u : 0u;  // the upper lane keeps fl(p - v)
#pragma unroll
    for (int r = 0; r < kRegs; ++r) v[r] = flip(v[r], upper) + partner<H>(v[r]);
}

// the same across the 16-lane rows (H = 16) or the wave's halves (H = 32)
template <int H>
__device__ __forceinline__ void row_stage(float (&v)[kRegs], int lane) {
#if DLS_DRIVE_XLANE && defined(__HIP_DEVICE_COMPILE__)
    typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
#pragma unroll
    for (int r = 0; r < kRegs; r += 2) {
        // after the swap the lower lanes of every pair hold register r's (a, b) in (p[0],
        // p[1]) and the upper lanes register r + 1's
        u32x2 p, q;
        if constexpr (H == 16)
            p = __builtin_amdgcn_permlane16_swap(__float_as_uint(v[r]), __float_as_uint(v[r + 1]),
                                                 false, false);
        else
            p = __builtin_amdgcn_permlane32_swap(__float_as_uint(v[r]), __float_as_uint(v[r + 1]),
                                                 false, false);
        const float a = __uint_as_float(p[0]), b = __uint_as_float(p[1]);
        const float s = a + b, d = a - b;
        if constexpr (H == 16)
            q = __builtin_amdgcn_permlane16_swap(__float_as_uint(s), __float_as_uint(d), false,
                                                 false);
        else
            q = __builtin_amdgcn_permlane32_swap(__float_as_uint(s), __float_as_uint(d), false,
                                                 false);
        v[r] = __uint_as_float(q[0]);
        v[r + 1] = __uint_as_float(q[1]);
    }
#else
    const uint32_t upper = (lane & H) ? 0x80000000u : 0u;
#pragma unroll
    for (int r = 0; r < kRegs; ++r) v[r] = flip(v[r], upper) + __shfl_xor(v[r], H, 64);
#endif
}

// H of include/dls_hip.h on the block the workgroup holds, without the final 2^-6: the
// stages h = 1 .. 2048 in ascending order.  xch: 16 KB of LDS, free on entry; the caller
// synchronises before it uses xch again.
__device__ __forceinline__ void hadamard(float (&v)[kRegs], f32x4 *xch, int wave, int lane) {
    lane_stage<1>(v, lane);
    lane_stage<2>(v, lane);
    lane_stage<4>(v, lane);
    lane_stage<8>(v, lane);
    row_stage<16>(v, lane);
    row_stage<32>(v, lane);
#pragma unroll
    for (int h = 1; h < kRegs; h <<= 1) {
#pragma unroll
        for (int r = 0; r < kRegs; ++r) {
            if (r & h) continue;
            const float a = v[r], b = v[r + h];
            v[r] = a + b;
            v[r + h] = a - b;
        }
    }
    // vector (wave, r / 4, lane): consecutive lanes 16 bytes apart
#pragma unroll
    for (int g = 0; g < kRegs / 4; ++g)
        xch[(wave * (kRegs / 4) + g) * 64 + lane] =
            f32x4{v[4 * g], v[4 * g + 1], v[4 * g + 2], v[4 * g + 3]};
    __syncthreads();
    const uint32_t odd = (wave & 1) ? 0x80000000u : 0u;   // h = 1024: the waves 1, 3 subtract
    const uint32_t high = (wave & 2) ? 0x80000000u : 0u;  // h = 2048: the waves 2, 3
#pragma unroll
    for (int g = 0; g < kRegs / 4; ++g) {
        f32x4 a[kWaves];
#pragma unroll
        for (int w = 0; w < kWaves; ++w) a[w] = xch[(w * (kRegs / 4) + g) * 64 + lane];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float lo = a[0][k] + flip(a[1][k], odd);
            const float hi = a[2][k] + flip(a[3][k], odd);
            v[4 * g + k] = lo + flip(hi, high);
        }
    }
}

// sigma of the wave's 16 words as lane masks: word r is the Philox words of the
// coordinates 2 W and 2 W + 1, W = 64 B + 16 wave + r, i.e. half of Philox block W / 2;
// the lanes 0..7 of the wave hold the wave's eight blocks
__device__ __forceinline__ void sign_masks(uint64_t (&m)[kRegs], int64_t B, int wave, int lane,
                                           const PhiloxKey &key) {
    const u32x4 blk = philox_block((uint64_t)B * (kWords / 2) + wave * (kRegs / 2) + (lane & 7), key);
#pragma unroll
    for (int r = 0; r < kRegs; ++r) {
        const uint32_t lo = __builtin_amdgcn_readlane(blk[2 * (r & 1)], r >> 1);
        const uint32_t hi = __builtin_amdgcn_readlane(blk[2 * (r & 1) + 1], r >> 1);
        m[r] = ((uint64_t)hi << 32) | lo;
    }
}

__device__ __forceinline__ void apply_signs(float (&v)[kRegs], const uint64_t (&m)[kRegs]) {
#pragma unroll
    for (int r = 0; r < kRegs; ++r) v[r] = __builtin_amdgcn_inverse_ballot_w64(m[r]) ? -v[r] : v[r];
}

__device__ __forceinline__ void scale_down(float (&v)[kRegs]) {
#pragma unroll
    for (int r = 0; r < kRegs; ++r) v[r] = v[r] * 0x1p-6f;
}

__device__ __forceinline__ double wave_tree(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// the coordinate of register r = 0 of this thread; register r is 64 r further on, and a
// register's 64 coordinates lie inside the row together (P is a multiple of 64)
__device__ __forceinline__ int64_t first_coordinate(int64_t B, int wave, int lane) {
    return B * kD + wave * (kD / kWaves) + lane;
}

template <bool INVERSE>
__global__ __launch_bounds__(kBlock) void k_hadamard_rotate(const float *__restrict__ x, int64_t P,
                                                            PhiloxKey key, float *__restrict__ out) {
    __shared__ f32x4 xch[kD / 4];
    const int64_t B = blockIdx.x;
    const int wave = uniform(threadIdx.x >> 6), lane = lane_id();
    const int64_t j = first_coordinate(B, wave, lane);
    uint64_t m[kRegs];
    sign_masks(m, B, wave, lane, key);
    float v[kRegs];
#pragma unroll
    for (int r = 0; r < kRegs; ++r) v[r] = (INVERSE || j + 64 * r < P) ? ldg_nt(x + j + 64 * r) : 0.f;
    if constexpr (!INVERSE) apply_signs(v, m);
    hadamard(v, xch, wave, lane);
    scale_down(v);
    if constexpr (INVERSE) apply_signs(v, m);
#pragma unroll
    for (int r = 0; r < kRegs; ++r)
        if (!INVERSE || j + 64 * r < P) out[j + 64 * r] = v[r];
}

__global__ __launch_bounds__(kBlock) void k_drive_compress(
    const float *__restrict__ w, const float *__restrict__ base, int64_t P, PhiloxKey key,
    int scale_mode, uint64_t *__restrict__ bits, float *__restrict__ scales,
    int32_t *__restrict__ stats, unsigned long long *cell) {
    __shared__ f32x4 xch[kD / 4];
    __shared__ double lsq[kWaves], ll1[kWaves];
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
    double sq = 0.0, l1 = 0.0;
    uint64_t word = 0;
#pragma unroll
    for (int r = 0; r < kRegs; ++r) {
        const double y = (double)v[r];
        sq += y * y;
        l1 += __builtin_fabs(y);
        const uint64_t ballot = __ballot(v[r] < 0.f);
        if (lane == r) word = ballot;
    }
    if (lane < kRegs) bits[B * kWords + wave * kRegs + lane] = word;
    sq = wave_tree(sq);
    l1 = wave_tree(l1);
    nbad = wave_sum(nbad);
    if (lane == 0) {
        lsq[wave] = sq;
        ll1[wave] = l1;
        lbad[wave] = nbad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        sq = ((lsq[0] + lsq[1]) + lsq[2]) + lsq[3];
        l1 = ((ll1[0] + ll1[1]) + ll1[2]) + ll1[3];
        nbad = lbad[0] + lbad[1] + lbad[2] + lbad[3];
        scales[B] = l1 == 0.0 ? 0.f : (float)(scale_mode == 0 ? sq / l1 : l1 / (double)kD);
        const unsigned long long before = atomicAdd(cell, (1ull << 32) | nbad);
        if ((before >> 32) == gridDim.x - 1) {  // every other block's count is in `before`
            stats[0] = (int32_t)((uint32_t)before + nbad);
            atomicExch(cell, 0ull);
        }
    }
}

__global__ __launch_bounds__(kBlock) void k_drive_fedavg(
    const float *__restrict__ base, const uint64_t *__restrict__ bits, int64_t ldb,
    const float *__restrict__ scales, int64_t lds, const float *__restrict__ weight, FastDiv d,
    int K, int64_t P, PhiloxKey key, float *__restrict__ out) {
    __shared__ f32x4 xch[kD / 4];
    __shared__ float ctab[kTileK];  // c[i][B] of the tile's clients
    const int64_t B = blockIdx.x;
    const int wave = uniform(threadIdx.x >> 6), lane = lane_id();
    float z[kRegs];
#pragma unroll
    for (int r = 0; r < kRegs; ++r) z[r] = 0.f;
    for (int k0 = 0; k0 < K; k0 += kTileK) {
        __syncthreads();  // the previous tile has been applied
        const int nb = K - k0 < kTileK ? K - k0 : kTileK;
        if ((int)threadIdx.x < nb)
            ctab[threadIdx.x] = div_exact(
                scales[(int64_t)(k0 + threadIdx.x) * lds + B] * weight[k0 + threadIdx.x], d);
        __syncthreads();
        const uint64_t *row = bits + (int64_t)k0 * ldb + B * kWords + wave * kRegs;
        for (int i = 0; i < nb; ++i, row += ldb) {
            uint64_t m[kRegs];
#pragma unroll
            for (int r = 0; r < kRegs; ++r) m[r] = row[r];  // wave-uniform: the scalar cache
            const float c = ctab[i], n = -c;
            if (k0 + i == 0) {
#pragma unroll
                for (int r = 0; r < kRegs; ++r)
                    z[r] = __builtin_amdgcn_inverse_ballot_w64(m[r]) ? n : c;
            } else {
#pragma unroll
                for (int r = 0; r < kRegs; ++r)
                    z[r] = z[r] + (__builtin_amdgcn_inverse_ballot_w64(m[r]) ? n : c);
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

// [a, a + na) and [b, b + nb) bytes intersect
inline bool overlap(const void *a, int64_t na, const void *b, int64_t nb) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + (uintptr_t)nb && b0 < a0 + (uintptr_t)na;
}

inline int check_extent(const char *fn, int64_t P) {
    DLS_REQUIRE(P >= 64 && P < kMaxP, DLS_EINVAL, "%s: P=%lld (64 <= P < 2^31)", fn, (long long)P);
    DLS_REQUIRE(P % 64 == 0, DLS_ELAYOUT, "%s: P=%lld must be a multiple of 64", fn, (long long)P);
    return DLS_OK;
}

inline int64_t blocks_of(int64_t P) { return (P + kD - 1) / kD; }

}  // namespace
}  // namespace dls

using namespace dls;

extern "C" int dls_hadamard_rotate_f32(const float *x, int64_t P, uint64_t seed,
                                       uint64_t stream_id, int32_t inverse, float *out,
                                       dls_stream_t stream) {
    const char *fn = "dls_hadamard_rotate_f32";
    DLS_REQUIRE(x && out, DLS_EINVAL, "%s: null pointer (x, out)", fn);
    DLS_REQUIRE(inverse == 0 || inverse == 1, DLS_EINVAL, "%s: inverse=%d (0 or 1)", fn, inverse);
    const int rc = check_extent(fn, P);
    if (rc != DLS_OK) return rc;
    DLS_REQUIRE(aligned16(x) && aligned16(out), DLS_ELAYOUT, "%s: 16-byte alignment of x and out",
                fn);
    const int64_t NB = blocks_of(P), Pd = NB * kD;
    DLS_REQUIRE(!overlap(out, 4 * (inverse ? P : Pd), x, 4 * (inverse ? Pd : P)), DLS_EINVAL,
                "%s: out must not alias x", fn);
    const PhiloxKey key = make_key(seed, stream_id);
    if (inverse)
        hipLaunchKernelGGL(k_hadamard_rotate<true>, dim3((unsigned)NB), dim3(kBlock), 0,
                           as_stream(stream), x, P, key, out);
    else
        hipLaunchKernelGGL(k_hadamard_rotate<false>, dim3((unsigned)NB), dim3(kBlock), 0,
                           as_stream(stream), x, P, key, out);
    return check_launch(fn);
}

extern "C" int dls_drive_compress_f32(const float *w, const float *base, int64_t P, uint64_t seed,
                                      uint64_t stream_id, int32_t scale_mode, uint64_t *bits,
                                      float *scales, int32_t *stats, dls_stream_t stream) {
    const char *fn = "dls_drive_compress_f32";
    DLS_REQUIRE(w && base && bits && scales && stats, DLS_EINVAL,
                "%s: null pointer (w, base, bits, scales, stats)", fn);
    DLS_REQUIRE(scale_mode == DLS_DRIVE_UNBIASED || scale_mode == DLS_DRIVE_MSE, DLS_EINVAL,
                "%s: scale_mode=%d (DLS_DRIVE_UNBIASED or DLS_DRIVE_MSE)", fn, scale_mode);
    const int rc = check_extent(fn, P);
    if (rc != DLS_OK) return rc;
    DLS_REQUIRE(aligned16(w) && aligned16(base) && aligned16(bits) && aligned16(scales) &&
                    aligned16(stats),
                DLS_ELAYOUT, "%s: 16-byte alignment of w, base, bits, scales and stats", fn);
    const int64_t NB = blocks_of(P);
    DLS_REQUIRE(!overlap(bits, NB * kD / 8, w, 4 * P) && !overlap(bits, NB * kD / 8, base, 4 * P) &&
                    !overlap(scales, 4 * NB, w, 4 * P) && !overlap(scales, 4 * NB, base, 4 * P) &&
                    !overlap(stats, 4, w, 4 * P) && !overlap(stats, 4, base, 4 * P),
                DLS_EINVAL, "%s: bits, scales and stats must not alias w or base", fn);
    unsigned long long *cell = stream_cell(as_stream(stream));
    DLS_REQUIRE(cell, DLS_EINVAL, "%s: no device memory for the stream's counter cell", fn);
    hipLaunchKernelGGL(k_drive_compress, dim3((unsigned)NB), dim3(kBlock), 0, as_stream(stream), w,
                       base, P, make_key(seed, stream_id), (int)scale_mode, bits, scales, stats,
                       cell);
    return check_launch(fn);
}

extern "C" int dls_drive_fedavg_f32(const float *base, const uint64_t *bits, int64_t ldb,
                                    const float *scales, int64_t lds, const float *weight,
                                    float total, int32_t K, int64_t P, uint64_t seed,
                                    uint64_t stream_id, float *out, dls_stream_t stream) {
    const char *fn = "dls_drive_fedavg_f32";
    DLS_REQUIRE(base && bits && scales && weight && out, DLS_EINVAL,
                "%s: null pointer (base, bits, scales, weight, out)", fn);
    DLS_REQUIRE(K >= 1, DLS_EINVAL, "%s: K=%d (K >= 1)", fn, K);
    const int rc = check_extent(fn, P);
    if (rc != DLS_OK) return rc;
    const int64_t NB = blocks_of(P);
    DLS_REQUIRE(ldb >= NB * kWords && lds >= NB, DLS_ELAYOUT,
                "%s: ldb=%lld and lds=%lld must be at least Pd / 64 = %lld and NB = %lld", fn,
                (long long)ldb, (long long)lds, (long long)(NB * kWords), (long long)NB);
    DLS_REQUIRE(aligned16(base) && aligned16(bits) && aligned16(scales) && aligned16(weight) &&
                    aligned16(out),
                DLS_ELAYOUT, "%s: 16-byte alignment of base, bits, scales, weight and out", fn);
    DLS_REQUIRE(!overlap(out, 4 * P, base, 4 * P), DLS_EINVAL, "%s: out must not alias base", fn);
    hipLaunchKernelGGL(k_drive_fedavg, dim3((unsigned)NB), dim3(kBlock), 0, as_stream(stream), base,
                       bits, ldb, scales, lds, weight, make_fastdiv(total), (int)K, P,
                       make_key(seed, stream_id), out);
    return check_launch(fn);
}
