// Scaled-sign compression with error feedback for gfx950 (Karimireddy, Rebjock, Stich &
// Jaggi 2019, "Error feedback fixes SignSGD"; the compressor of 1-bit SGD / 1-bit Adam):
// the client's compressor and the server's FedAvg over bit rows.  include/dls_hip.h has
// the contract.
//
// dls_efsign_compress_f32: u = fl(fl(w - base) + e); per tensor t the scale s[t] =
// fl32(sum |u| / count[t]); one bit per coordinate (u < 0); e <- u -+ s[t].  Four launches
// on one stream, nothing leaving the device:
//
//   k_plan    one block: first[t], the number of kChunk-sized chunks of the tensors before
//             t (an exclusive scan of ceil(count / kChunk)); stats[0] <- 0
//   k_form    one block per chunk (chunk c of tensor t: its real elements c * kChunk ..):
//             u -> e, the chunk's fp64 sum of |u| and its non-finite count.  A thread adds
//             its 16 elements in ascending order, a wave combines its lanes by a fixed
//             xor tree, the block's four wave sums are added in wave order
//   k_scale   one wave per tensor: lane l adds the chunk sums l, l + 64, ... in ascending
//             order, the same xor tree combines the lanes; s[t] = (float)(sum / count[t])
//   k_pack    one block per 4096 coordinates of the row: the bits, and e <- u -+ s[t] on the
//             real slots, +0.0 on the padding
//
// Chunks are cut relative to the tensor's own start, so every step of the sum's order is
// a function of count[t] alone.  The only atomic is the integer add of the non-finite
// counts.  k_pack has two forms (DLS_EFSIGN_PACK_VEC): 1, lane l of a wave holds coordinate
// 64 w + l and the word is the wave's ballot; 4, a lane loads 16 bytes and the four ballots
// of 256 coordinates are bit-interleaved into four words.  DESIGN.md has both timings.
//
// dls_efsign_fedavg_f32: one launch.  A block owns 64 words (4096 coordinates), a wave 16
// of them, lane l of the wave coordinate 64 w + l of each: a client's word is then the
// wave's lane mask, and the client costs one v_cndmask (+c or -c) and one v_add per
// coordinate.  Clients go in tiles of kTileK; per tile the block computes c[i][t] =
// fl(fl(s[i][t] * n_i) / N) for the tensors it touches into LDS.  The masks reach the wave
// through the scalar data cache (uniform loads of the client's 16 words), or, with
// DLS_EFSIGN_DECODE_LDS, through an LDS tile [clients x words] that lanes over clients
// stage.  No atomics; a coordinate's chain is walked in client order by one lane.
#include <algorithm>

#include "rows_common.h"

#ifndef DLS_EFSIGN_PACK_VEC
#define DLS_EFSIGN_PACK_VEC 4
#endif
#ifndef DLS_EFSIGN_DECODE_LDS
#define DLS_EFSIGN_DECODE_LDS 0
#endif

namespace dls {
namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kChunk = DLS_EFSIGN_CHUNK;         // real elements of one tensor per k_form block
constexpr int kPlanBlock = 1024;
constexpr int kTileK = DLS_EFSIGN_CLIENT_TILE;   // clients per c table in LDS
constexpr int kRun = 4096;                       // coordinates per k_pack / k_fedavg block
constexpr int kRunWords = kRun / 64;
constexpr int kWaveWords = kRunWords / kWaves;   // 16 words per wave
static_assert(kChunk == kBlock * 16, "a k_form thread owns four 16-byte vectors");
constexpr int64_t kMaxP = (int64_t)1 << 31;

// workspace: int32 first[first_words(T)], double part[slots], uint32 bad[slots]
inline int64_t slots_of(int64_t P, int64_t T) { return P / kChunk + T; }  // >= sum ceil(count / kChunk)
inline int64_t first_words(int64_t T) { return (T + 2) & ~(int64_t)1; }   // >= T + 1, even

__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }

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

// the last t in [lo, hi] with a[t] <= j (lo when there is none)
template <typename T>
__device__ __forceinline__ int last_le(const T *a, int lo, int hi, int64_t j) {
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((int64_t)a[mid] <= j) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

__device__ __forceinline__ uint32_t chunks_in(int64_t n, int64_t P) {
    n = n < 0 ? 0 : (n > P ? P : n);
    return (uint32_t)((n + kChunk - 1) / kChunk);
}

__global__ __launch_bounds__(kPlanBlock) void k_efsign_plan(const int64_t *count, int T, int64_t P,
                                                            int32_t *first, int32_t *stats) {
    __shared__ uint32_t lds[kPlanBlock / 64];
    const int per = (T + kPlanBlock - 1) / kPlanBlock;
    const int64_t a64 = (int64_t)threadIdx.x * per;
    const int a = a64 < T ? (int)a64 : T, b = a + per < T ? a + per : T;
    uint32_t sum = 0;
    for (int t = a; t < b; ++t) sum += chunks_in(count[t], P);
    uint32_t incl = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(incl, d, 64);
        if (lane_id() >= d) incl += o;
    }
    const int wave = threadIdx.x >> 6;
    if (lane_id() == 63) lds[wave] = incl;
    __syncthreads();
    uint32_t run = incl - sum, total = 0;
    for (int w = 0; w < kPlanBlock / 64; ++w) {
        if (w < wave) run += lds[w];
        total += lds[w];
    }
    for (int t = a; t < b; ++t) {
        first[t] = (int32_t)run;
        run += chunks_in(count[t], P);
    }
    if (threadIdx.x == 0) {
        first[T] = (int32_t)total;
        stats[0] = 0;
    }
}

__global__ __launch_bounds__(kBlock) void k_efsign_form(const float *w, const float *base, float *e,
                                                        int64_t P, const int64_t *bounds,
                                                        const int64_t *count, int T,
                                                        const int32_t *first, double *part,
                                                        uint32_t *bad) {
    __shared__ double lsum[kWaves];
    __shared__ uint32_t lbad[kWaves];
    const int64_t b = blockIdx.x;
    if (b >= first[T]) return;
    const int t = last_le(first, 0, T - 1, b);
    const int64_t start = bounds[t] + (b - first[t]) * kChunk;
    // the chunk's real elements; clipped to the row whatever the segment arrays hold
    int64_t n = bounds[t] + count[t] - start;
    n = n < kChunk ? n : kChunk;
    if (start < 0 || (start & 3) != 0) n = 0;
    n = n < P - start ? n : P - start;
    const f32x4 *wv = reinterpret_cast<const f32x4 *>(w + start);
    const f32x4 *bv = reinterpret_cast<const f32x4 *>(base + start);
    f32x4 *ev = reinterpret_cast<f32x4 *>(e + start);
    f32x4 qw[4], qb[4], qe[4];
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        const int q = v * kBlock + threadIdx.x;
        if (4 * q < n) {
            qw[v] = ldg_nt(wv + q);
            qb[v] = ldg_nt(bv + q);
            qe[v] = ev[q];
        }
    }
    double acc = 0.0;
    uint32_t nbad = 0;
#pragma unroll
    for (int v = 0; v < 4; ++v) {
        const int q = v * kBlock + threadIdx.x;
        if (4 * q < n) {
            f32x4 u;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                u[j] = (qw[v][j] - qb[v][j]) + qe[v][j];
                if (4 * q + j < n) {
                    acc += __builtin_fabs((double)u[j]);
                    nbad += (__float_as_uint(u[j]) & 0x7fffffffu) >= 0x7f800000u;
                }
            }
            ev[q] = u;  // the padding lanes of the last vector are rewritten by k_pack
        }
    }
    acc = wave_tree(acc);
    nbad = wave_sum(nbad);
    if (lane_id() == 0) {
        lsum[threadIdx.x >> 6] = acc;
        lbad[threadIdx.x >> 6] = nbad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        part[b] = ((lsum[0] + lsum[1]) + lsum[2]) + lsum[3];
        bad[b] = lbad[0] + lbad[1] + lbad[2] + lbad[3];
    }
}

__global__ __launch_bounds__(kBlock) void k_efsign_scale(const int64_t *count, int T, int64_t slots,
                                                         const int32_t *first, const double *part,
                                                         const uint32_t *bad, float *scales,
                                                         int32_t *stats) {
    const int t = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (t >= T) return;
    int64_t f0 = first[t], f1 = first[t + 1];
    f0 = f0 < 0 ? 0 : (f0 > slots ? slots : f0);
    f1 = f1 < f0 ? f0 : (f1 > slots ? slots : f1);
    double acc = 0.0;
    uint32_t nbad = 0;
    for (int64_t c = f0 + lane_id(); c < f1; c += 64) {
        acc += part[c];
        nbad += bad[c];
    }
    acc = wave_tree(acc);
    nbad = wave_sum(nbad);
    if (lane_id() == 0) {
        scales[t] = (float)(acc / (double)count[t]);
        if (nbad) atomicAdd(stats, (int32_t)nbad);
    }
}

// bits 0..15 of x to the bit positions 0, 4, 8, ..., 60
__device__ __forceinline__ uint64_t spread4(uint64_t x) {
    x = (x | (x << 24)) & 0x000000ff000000ffull;
    x = (x | (x << 12)) & 0x000f000f000f000full;
    x = (x | (x << 6)) & 0x0303030303030303ull;
    x = (x | (x << 3)) & 0x1111111111111111ull;
    return x;
}

template <int VEC>
__global__ __launch_bounds__(kBlock) void k_efsign_pack(float *e, int64_t P, const int64_t *bounds,
                                                        const int64_t *count, int T,
                                                        const float *scales, uint64_t *bits) {
    const int64_t c0 = (int64_t)blockIdx.x * kRun;
    const int64_t c1 = c0 + kRun < P ? c0 + kRun : P;
    const int t_lo = last_le(bounds, 0, T - 1, c0);
    const int t_hi = last_le(bounds, t_lo, T - 1, c1 - 1);
    const int wave = uniform(threadIdx.x >> 6), lane = lane_id();
    if constexpr (VEC == 1) {
        float u[kWaveWords];
#pragma unroll
        for (int q = 0; q < kWaveWords; ++q) {
            const int64_t j = c0 + 64 * (wave * kWaveWords + q) + lane;
            u[q] = j < P ? e[j] : 0.f;
        }
#pragma unroll
        for (int q = 0; q < kWaveWords; ++q) {
            const int64_t j0 = c0 + 64 * (wave * kWaveWords + q), j = j0 + lane;
            const bool valid = j0 < P;  // wave-uniform: P is a multiple of 64
            const int t = last_le(bounds, t_lo, t_hi, j0);
            const float s = scales[t];
            const bool real = valid && j < bounds[t] + count[t];
            const bool neg = real && u[q] < 0.f;
            const uint64_t word = __ballot(neg);
            if (valid) {
                e[j] = real ? (neg ? u[q] + s : u[q] - s) : 0.f;
                if (lane == 0) bits[j0 >> 6] = word;
            }
        }
    } else {
        constexpr int kGroups = kRun / 256 / kWaves;  // 256-coordinate groups per wave
        f32x4 u[kGroups];
#pragma unroll
        for (int r = 0; r < kGroups; ++r) {
            const int64_t j = c0 + 256 * (wave + kWaves * r) + 4 * lane;
            u[r] = j < P ? *reinterpret_cast<const f32x4 *>(e + j) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
#pragma unroll
        for (int r = 0; r < kGroups; ++r) {
            const int64_t g0 = c0 + 256 * (wave + kWaves * r), j = g0 + 4 * lane;
            const bool valid = j < P;
            const int t = last_le(bounds, t_lo, t_hi, valid ? j : c0);
            const float s = scales[t];
            const int64_t lim = bounds[t] + count[t];
            uint64_t bal[4];
            f32x4 r4;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool real = valid && j + k < lim;
                const bool neg = real && u[r][k] < 0.f;
                bal[k] = __ballot(neg);
                r4[k] = real ? (neg ? u[r][k] + s : u[r][k] - s) : 0.f;
            }
            if (valid) *reinterpret_cast<f32x4 *>(e + j) = r4;
            // word m of the group: bit i is coordinate 64 m + i = lane 16 m + i / 4, element i % 4
            const int m = lane & 3;
            uint64_t word = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) word |= spread4((bal[k] >> (16 * m)) & 0xffffull) << k;
            if (lane < 4 && g0 + 64 * lane < P) bits[(g0 >> 6) + lane] = word;
        }
    }
}

// ---------------------------------------------------------------- FedAvg over bit rows
template <bool LDSMASK>
__device__ __forceinline__ uint64_t client_word(const uint64_t *row, const uint64_t *tile, int q,
                                                bool inside) {
    if constexpr (LDSMASK) {
        const uint64_t v = tile[q];
        const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
        const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
        return ((uint64_t)hi << 32) | lo;
    } else {
        return inside ? row[q] : 0ull;
    }
}

// client i of the tile onto the wave's 16 accumulators
template <bool FIRST, bool LDSMASK>
__device__ __forceinline__ void apply_client(float (&acc)[kWaveWords], const uint64_t *row,
                                             const uint64_t *tile, const float *crow, const int *wt,
                                             bool same, int words) {
    uint64_t m[kWaveWords];
    if (words >= kWaveWords) {
#pragma unroll
        for (int q = 0; q < kWaveWords; ++q) m[q] = client_word<LDSMASK>(row, tile, q, true);
    } else {
#pragma unroll
        for (int q = 0; q < kWaveWords; ++q) m[q] = client_word<LDSMASK>(row, tile, q, q < words);
    }
    if (same) {
        const float c = crow[wt[0]], n = -c;
#pragma unroll
        for (int q = 0; q < kWaveWords; ++q) {
            const float term = __builtin_amdgcn_inverse_ballot_w64(m[q]) ? n : c;
            acc[q] = FIRST ? term : acc[q] + term;
        }
    } else {
#pragma unroll
        for (int q = 0; q < kWaveWords; ++q) {
            const float c = crow[wt[q]];
            const float term = __builtin_amdgcn_inverse_ballot_w64(m[q]) ? -c : c;
            acc[q] = FIRST ? term : acc[q] + term;
        }
    }
}

template <bool LDSMASK>
__global__ __launch_bounds__(kBlock) void k_efsign_fedavg(
    const float *__restrict__ base, const uint64_t *__restrict__ bits, int64_t ldb,
    const float *__restrict__ scales, int64_t lds, const int64_t *__restrict__ bounds,
    const int64_t *__restrict__ count, int T, const float *__restrict__ weight, FastDiv d, int K,
    int64_t P, float *__restrict__ out) {
    __shared__ float ctab[kTileK * kRunWords];  // [client of the tile][tensor - t_lo]
    __shared__ int wt[kRunWords];               // word of the run -> tensor - t_lo
    __shared__ int wreal[kRunWords];            // word of the run -> its real coordinates, 0..64
    __shared__ uint64_t mtile[LDSMASK ? kTileK * kRunWords : 1];
    const int64_t w0 = (int64_t)blockIdx.x * kRunWords;
    const int64_t left = P / 64 - w0;
    const int nwords = left < kRunWords ? (int)left : kRunWords;
    const int t_lo = last_le(bounds, 0, T - 1, 64 * w0);
    const int t_hi = last_le(bounds, t_lo, T - 1, 64 * (w0 + nwords) - 1);
    const int nt = t_hi - t_lo < kRunWords ? t_hi - t_lo + 1 : kRunWords;
    if (threadIdx.x < kRunWords) {  // the tensor of a word: found once per word
        const int q = (int)threadIdx.x < nwords ? threadIdx.x : nwords - 1;
        const int64_t j0 = 64 * (w0 + q);
        const int t = last_le(bounds, t_lo, t_hi, j0);
        const int64_t r = bounds[t] + count[t] - j0;
        wt[threadIdx.x] = t - t_lo < kRunWords ? t - t_lo : kRunWords - 1;
        wreal[threadIdx.x] = (int)threadIdx.x < nwords ? (int)(r < 0 ? 0 : (r > 64 ? 64 : r)) : 0;
    }
    const int wave = uniform(threadIdx.x >> 6), lane = lane_id();
    const int q0 = wave * kWaveWords;
    const int words = nwords - q0 < kWaveWords ? (nwords - q0 < 0 ? 0 : nwords - q0) : kWaveWords;
    const float *bp = base + 64 * (w0 + q0) + lane;
    float bv[kWaveWords], acc[kWaveWords];
#pragma unroll
    for (int q = 0; q < kWaveWords; ++q) {
        bv[q] = q < words ? ldg_nt(bp + 64 * q) : 0.f;
        acc[q] = 0.f;
    }
    for (int k0 = 0; k0 < K; k0 += kTileK) {
        __syncthreads();  // the previous tile has been applied; wt / wreal are written
        const int nb = K - k0 < kTileK ? K - k0 : kTileK;
        for (int x = threadIdx.x; x < nb * nt; x += kBlock) {
            const int i = x / nt, tt = x - i * nt;
            ctab[i * kRunWords + tt] =
                div_exact(scales[(int64_t)(k0 + i) * lds + t_lo + tt] * weight[k0 + i], d);
        }
        if constexpr (LDSMASK) {  // thread = (client, quarter of the run): 16 contiguous words
            const int i = threadIdx.x >> 2, p = (threadIdx.x & 3) * kWaveWords;
            const uint64_t *src = bits + (int64_t)(k0 + i) * ldb + w0 + p;
#pragma unroll
            for (int x = 0; x < kWaveWords; ++x)
                mtile[i * kRunWords + p + x] = (i < nb && p + x < nwords) ? src[x] : 0ull;
        }
        __syncthreads();
        const bool same = wt[q0] == wt[q0 + kWaveWords - 1];
        const uint64_t *row = bits + (int64_t)k0 * ldb + w0 + q0;
        int i = 0;
        if (k0 == 0) {
            apply_client<true, LDSMASK>(acc, row, mtile + q0, ctab, wt + q0, same, words);
            i = 1;
        }
        for (; i < nb; ++i)
            apply_client<false, LDSMASK>(acc, row + (int64_t)i * ldb, mtile + i * kRunWords + q0,
                                         ctab + i * kRunWords, wt + q0, same, words);
    }
    float *op = out + 64 * (w0 + q0) + lane;
#pragma unroll
    for (int q = 0; q < kWaveWords; ++q)
        if (q < words) op[64 * q] = lane < wreal[q0 + q] ? bv[q] + acc[q] : bv[q];
}

// [a, a + na) and [b, b + nb) bytes intersect
inline bool overlap(const void *a, int64_t na, const void *b, int64_t nb) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + (uintptr_t)nb && b0 < a0 + (uintptr_t)na;
}

// the extent of a bit row: P coordinates in whole words, T tensors of at least one word
inline int check_extent(const char *fn, int64_t P, int64_t T) {
    DLS_REQUIRE(P >= 64 && P < kMaxP, DLS_EINVAL, "%s: P=%lld (64 <= P < 2^31)", fn, (long long)P);
    DLS_REQUIRE(P % 64 == 0, DLS_ELAYOUT, "%s: P=%lld must be a multiple of 64", fn, (long long)P);
    DLS_REQUIRE(T >= 1 && T <= P / 64, DLS_EINVAL, "%s: T=%lld (1 <= T <= P / 64 = %lld)", fn,
                (long long)T, (long long)(P / 64));
    return DLS_OK;
}

}  // namespace
}  // namespace dls

using namespace dls;

extern "C" int64_t dls_efsign_workspace(int64_t P, int64_t T) {
    const int rc = check_extent("dls_efsign_workspace", P, T);
    if (rc != DLS_OK) return rc;
    return 4 * first_words(T) + 12 * slots_of(P, T);
}

extern "C" int dls_efsign_compress_f32(const float *w, const float *base, float *e, int64_t P,
                                       const int64_t *bounds, const int64_t *count, int32_t T,
                                       uint64_t *bits, float *scales, int32_t *stats,
                                       void *workspace, dls_stream_t stream) {
    const char *fn = "dls_efsign_compress_f32";
    DLS_REQUIRE(w && base && e && bounds && count && bits && scales && stats && workspace,
                DLS_EINVAL,
                "%s: null pointer (w, base, e, bounds, count, bits, scales, stats, workspace)", fn);
    const int rc = check_extent(fn, P, T);
    if (rc != DLS_OK) return rc;
    DLS_REQUIRE(aligned16(w) && aligned16(base) && aligned16(e) && aligned16(bounds) &&
                    aligned16(count) && aligned16(bits) && aligned16(scales) && aligned16(stats) &&
                    aligned16(workspace),
                DLS_ELAYOUT,
                "%s: 16-byte alignment of w, base, e, bounds, count, bits, scales, stats and "
                "workspace", fn);
    DLS_REQUIRE(!overlap(e, 4 * P, w, 4 * P) && !overlap(e, 4 * P, base, 4 * P), DLS_EINVAL,
                "%s: e must not alias w or base", fn);
    hipStream_t st = as_stream(stream);
    const int64_t slots = slots_of(P, T);
    int32_t *first = static_cast<int32_t *>(workspace);
    double *part = reinterpret_cast<double *>(first + first_words(T));
    uint32_t *bad = reinterpret_cast<uint32_t *>(part + slots);
    hipLaunchKernelGGL(k_efsign_plan, dim3(1), dim3(kPlanBlock), 0, st, count, (int)T, P, first,
                       stats);
    hipLaunchKernelGGL(k_efsign_form, dim3((unsigned)slots), dim3(kBlock), 0, st, w, base, e, P,
                       bounds, count, (int)T, first, part, bad);
    hipLaunchKernelGGL(k_efsign_scale, dim3((unsigned)((T + kWaves - 1) / kWaves)), dim3(kBlock), 0,
                       st, count, (int)T, slots, first, part, bad, scales, stats);
    hipLaunchKernelGGL(k_efsign_pack<DLS_EFSIGN_PACK_VEC>, dim3((unsigned)((P + kRun - 1) / kRun)),
                       dim3(kBlock), 0, st, e, P, bounds, count, (int)T, scales, bits);
    return check_launch(fn);
}

extern "C" int dls_efsign_fedavg_f32(const float *base, const uint64_t *bits, int64_t ldb,
                                     const float *scales, int64_t lds, const int64_t *bounds,
                                     const int64_t *count, int32_t T, const float *weight,
                                     float total, int32_t K, int64_t P, float *out,
                                     dls_stream_t stream) {
    const char *fn = "dls_efsign_fedavg_f32";
    DLS_REQUIRE(base && bits && scales && bounds && count && weight && out, DLS_EINVAL,
                "%s: null pointer (base, bits, scales, bounds, count, weight, out)", fn);
    DLS_REQUIRE(K >= 1, DLS_EINVAL, "%s: K=%d (K >= 1)", fn, K);
    const int rc = check_extent(fn, P, T);
    if (rc != DLS_OK) return rc;
    DLS_REQUIRE(ldb >= P / 64 && lds >= T, DLS_ELAYOUT,
                "%s: ldb=%lld and lds=%lld must be at least P / 64 = %lld and T = %d", fn,
                (long long)ldb, (long long)lds, (long long)(P / 64), T);
    DLS_REQUIRE(aligned16(base) && aligned16(bits) && aligned16(scales) && aligned16(bounds) &&
                    aligned16(count) && aligned16(weight) && aligned16(out),
                DLS_ELAYOUT,
                "%s: 16-byte alignment of base, bits, scales, bounds, count, weight and out", fn);
    DLS_REQUIRE(!overlap(out, 4 * P, base, 4 * P), DLS_EINVAL, "%s: out must not alias base", fn);
    hipLaunchKernelGGL(k_efsign_fedavg<DLS_EFSIGN_DECODE_LDS != 0>,
                       dim3((unsigned)((P / 64 + kRunWords - 1) / kRunWords)), dim3(kBlock), 0,
                       as_stream(stream), base, bits, ldb, scales, lds, bounds, count, (int)T, weight,
                       make_fastdiv(total), (int)K, P, out);
    return check_launch(fn);
}
