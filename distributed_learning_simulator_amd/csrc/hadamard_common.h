// The randomised Walsh-Hadamard rotation over blocks of 4096 coordinates that the rotated
// compressors share (drive.hip, eden.hip); include/dls_hip.h has its contract.
//
// One transform device function, hadamard().  A 256-thread block owns one block of 4096
// coordinates and holds it in registers: of the index
//   bits 0-5   the lane,
//   bits 6-9   the thread's register r (0..15),
//   bits 10-11 the wave,
// so a wave's register r is the 64 coordinates of bit word 16 wave + r of the block, and the
// 64 signs of the word are two Philox words that one lane draws and the wave reads as a lane
// mask.  The stages in ascending order:
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
#pragma once

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

// [a, a + na) and [b, b + nb) bytes intersect
inline bool overlap(const void *a, int64_t na, const void *b, int64_t nb) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + (uintptr_t)nb && b0 < a0 + (uintptr_t)na;
}

// the extent every entry point over the rotation's blocks takes
inline int check_extent(const char *fn, int64_t P) {
    DLS_REQUIRE(P >= 64 && P < ((int64_t)1 << 31), DLS_EINVAL, "%s: P=%lld (64 <= P < 2^31)", fn,
                (long long)P);
    DLS_REQUIRE(P % 64 == 0, DLS_ELAYOUT, "%s: P=%lld must be a multiple of 64", fn, (long long)P);
    return DLS_OK;
}

inline int64_t blocks_of(int64_t P) { return (P + kD - 1) / kD; }

}  // namespace
}  // namespace dls
