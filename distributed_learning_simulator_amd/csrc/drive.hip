// Rotated one-bit compression for gfx950 (Suresh, Yu, Kumar & McMahan 2017, "Distributed
// mean estimation with limited communication"; Vargaftik et al. 2021, "DRIVE: one-bit
// distributed mean estimation"): a randomised Walsh-Hadamard rotation over blocks of 4096
// coordinates, the client's compressor and the server's FedAvg over bit rows in the
// rotated domain.  include/dls_hip.h has the contract.
//
// One transform device function, hadamard() of hadamard_common.h, serves the three entry
// points.  A 256-thread block owns one block of 4096 coordinates and holds it in registers
// in that header's ownership, so a wave's register r is the 64 coordinates of bit word 16
// wave + r of the block: in the compressor the word is the wave's ballot, in the FedAvg a
// client's word is the wave's lane mask (k_efsign_fedavg's walk).
//
// dls_drive_compress_f32's count of non-finite coordinates is the one number of the call
// that blocks share.  They meet in one 64-bit cell that the library keeps per HIP stream
// (calls on one stream are ordered): a block adds (1 << 32) + its count with one integer
// atomic, tickets in the high word and the count in the low one (it stays below 2^31), and
// the block that finds gridDim.x - 1 tickets taken stores the sum to stats[0] and leaves
// the cell zero for the next call.  Nothing else passes between blocks, so there is no fence
// (on a multi-die part a device-scope release writes the die's L2 back: with a fence per
// block the compressor took 128 us on the ResNet-18 row instead of 48).
#include "hadamard_common.h"

namespace dls {
namespace {

constexpr int kTileK = DLS_DRIVE_CLIENT_TILE;   // clients per c table in LDS

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
