// Top-k sparsified FedAvg with error feedback for gfx950 ("sparsified SGD with memory",
// Stich, Cordonnier & Jaggi 2018; Aji & Heafield 2017; Lin et al. 2018): the client's
// compressor and the server's sparse aggregation.  include/dls_hip.h has the contract.
//
// dls_topk_compress_f32: u = fl(fl(w - base) + e), the k coordinates with the largest
// key = bits(u) & 0x7fffffff (ties: lowest index first) go out as (idx ascending, val),
// the rest stays in e.  A radix select on the 31-bit key, digits of 11 + 10 + 10 bits,
// all on one stream, the threshold never leaving the device:
//
//   memset     the three digit histograms and the select state (the workspace may hold
//              anything on entry)
//   k_form     u -> e, histogram of key >> 20, count of non-finite u      (pass 1: 16 P bytes)
//   k_pick     one block: the digit the k-th largest key falls in, how many are still wanted
//   k_refine   histogram of the next 10 bits among the keys that share the prefix (pass 2)
//   k_pick
//   k_refine   ... of the last 10 bits                                             (pass 3)
//   k_pick     -> the threshold key T and `need`, how many keys == T are selected
//   k_count    per chunk of kChunk coordinates: #{key > T}, #{key == T}            (pass 4)
//   k_scan     one block: exclusive scan of both counts over the chunks; stats
//   k_write    per chunk: coordinate j is selected when key > T, or key == T and fewer
//              than `need` equal keys precede it; its output slot is
//              G(j) + min(E(j), need), G / E the numbers of larger / equal keys before j
//              (chunk prefix + an in-block scan): idx ascending by construction; e <- +0
//              there                                                                (pass 5)
//
// Histogram counts are integer LDS atomics flushed with one global integer atomic per
// (block, non-empty bin): sums of integers, so no result depends on their order.  Every
// output position comes from the scans.  No floating-point atomics.
//
// dls_sparse_fedavg_f32: one wave owns a tile of kTile coordinates in LDS.  For every
// batch of 64 clients each lane binary-searches one client's ascending indices for the
// tile's range; then the clients are applied in order (within a client the coordinates
// are distinct, so its entries go in parallel; a barrier separates clients), the first
// sender of a coordinate assigning fl(fl(v * n_i) / N) and the later ones adding theirs;
// out = fl(base + acc) where someone sent the coordinate and base's own bits elsewhere.
#include <algorithm>

#include "dls_common.h"

namespace dls {
namespace {

constexpr int kBlock = 256;
constexpr int kVecs = 4;                          // 16-byte vectors per thread and chunk
constexpr int kChunk = DLS_TOPK_CHUNK;            // 4096 coordinates
constexpr int kHistBlocks = DLS_TOPK_HIST_BLOCKS; // grid-strided histogram passes
constexpr int kBins = 2048;                       // 11-bit first digit; the others use 1024
constexpr int kScanBlock = DLS_TOPK_SCAN_BLOCK;
static_assert(kChunk == kBlock * kVecs * 4, "a block covers one chunk per trip");
constexpr uint32_t kAbs = 0x7fffffffu;
constexpr uint32_t kInfKey = 0x7f800000u;

// workspace, in 32-bit words: [0, 3 * kBins) the histograms of the three digits;
// kState + 0 the key prefix chosen so far (after the third pick: T), + 1 the number still
// wanted among the keys that share it (after the third pick: need), + 2 the non-finite
// count; from kCounts on: gt[nchunks + 1], then eq[nchunks + 1]
constexpr int kState = 3 * kBins;
constexpr int kCounts = kState + 16;

inline int64_t chunks_of(int64_t P) { return (P + kChunk - 1) / kChunk; }

__device__ __forceinline__ uint32_t key_of(float u) { return __float_as_uint(u) & kAbs; }

// inclusive scan over a wave64
__device__ __forceinline__ uint32_t wave_scan_incl(uint32_t v) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(v, d, 64);
        if (lane_id() >= d) v += o;
    }
    return v;
}

// exclusive scan of v over a block of NT threads (lds: NT / 64 words); total: the block's sum
template <int NT>
__device__ __forceinline__ uint32_t block_scan_excl(uint32_t v, uint32_t *lds, uint32_t &total) {
    constexpr int NW = NT / 64;
    const int wave = threadIdx.x >> 6;
    const uint32_t incl = wave_scan_incl(v);
    __syncthreads();  // lds may still be read from an earlier call
    if (lane_id() == 63) lds[wave] = incl;
    __syncthreads();
    uint32_t before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) {
        const uint32_t t = lds[w];
        if (w < wave) before += t;
        total += t;
    }
    return before + incl - v;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__device__ __forceinline__ void flush_hist(const uint32_t *lh, uint32_t *gh, int bins) {
    for (int b = threadIdx.x; b < bins; b += kBlock) {
        const uint32_t c = lh[b];
        if (c) atomicAdd(gh + b, c);
    }
}

// pass 1: e <- u, first-digit histogram, non-finite count
__global__ __launch_bounds__(kBlock) void k_topk_form(const f32x4 *w, const f32x4 *base, f32x4 *e,
                                                      int64_t nvec, uint32_t *ws) {
    __shared__ uint32_t lh[kBins];
    for (int b = threadIdx.x; b < kBins; b += kBlock) lh[b] = 0;
    __syncthreads();
    uint32_t bad = 0;
    constexpr int64_t step = (int64_t)kBlock * kVecs;
    for (int64_t c = blockIdx.x; c * step < nvec; c += gridDim.x) {
        f32x4 qw[kVecs], qb[kVecs], qe[kVecs];
        int64_t i[kVecs];
#pragma unroll
        for (int v = 0; v < kVecs; ++v) {
            i[v] = c * step + (int64_t)v * kBlock + threadIdx.x;
            if (i[v] < nvec) {
                qw[v] = ldg_nt(w + i[v]);
                qb[v] = ldg_nt(base + i[v]);
                qe[v] = e[i[v]];
            }
        }
#pragma unroll
        for (int v = 0; v < kVecs; ++v) {
            if (i[v] < nvec) {
                f32x4 u;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    u[j] = (qw[v][j] - qb[v][j]) + qe[v][j];
                    const uint32_t key = key_of(u[j]);
                    bad += key >= kInfKey;
                    atomicAdd(&lh[key >> 20], 1u);
                }
                e[i[v]] = u;
            }
        }
    }
    __syncthreads();
    flush_hist(lh, ws, kBins);
    bad = wave_sum(bad);
    if (lane_id() == 0 && bad) atomicAdd(ws + kState + 2, bad);
}

// passes 2 and 3: the next 10 bits of the keys that share the chosen prefix
template <int PASS>  // 1: key >> 20 == prefix, digit bits 19..10; 2: key >> 10 == prefix, bits 9..0
__global__ __launch_bounds__(kBlock) void k_topk_refine(const f32x4 *e, int64_t nvec, uint32_t *ws) {
    __shared__ uint32_t lh[1024];
    for (int b = threadIdx.x; b < 1024; b += kBlock) lh[b] = 0;
    __syncthreads();
    const uint32_t prefix = ws[kState];
    constexpr int hi = PASS == 1 ? 20 : 10, lo = hi - 10;
    constexpr int64_t step = (int64_t)kBlock * kVecs;
    for (int64_t c = blockIdx.x; c * step < nvec; c += gridDim.x) {
        f32x4 q[kVecs];
        int64_t i[kVecs];
#pragma unroll
        for (int v = 0; v < kVecs; ++v) {
            i[v] = c * step + (int64_t)v * kBlock + threadIdx.x;
            if (i[v] < nvec) q[v] = e[i[v]];
        }
#pragma unroll
        for (int v = 0; v < kVecs; ++v) {
            if (i[v] < nvec) {
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint32_t key = key_of(q[v][j]);
                    if ((key >> hi) == prefix) atomicAdd(&lh[(key >> lo) & 1023u], 1u);
                }
            }
        }
    }
    __syncthreads();
    flush_hist(lh, ws + PASS * kBins, 1024);
}

// One block: walk the histogram from its highest bin down to the bin in which the
// `want`-th largest of the counted keys lies; extend the prefix by that digit and leave
// in want how many of that bin's keys are still wanted (1 .. its count).
__global__ __launch_bounds__(kBlock) void k_topk_pick(uint32_t *ws, int pass, int bins,
                                                      uint32_t first_want) {
    __shared__ uint32_t lds[kBlock / 64];
    const uint32_t *hist = ws + pass * kBins;
    const uint32_t want = pass == 0 ? first_want : ws[kState + 1];
    const uint32_t prefix = pass == 0 ? 0u : ws[kState];
    const int per = bins / kBlock;  // 8 or 4 bins per thread, thread 0 the highest ones
    uint32_t h[kBins / kBlock];
    uint32_t sum = 0;
    for (int j = 0; j < per; ++j) {
        h[j] = hist[bins - 1 - (threadIdx.x * per + j)];
        sum += h[j];
    }
    uint32_t total;
    uint32_t above = block_scan_excl<kBlock>(sum, lds, total);  // keys in higher bins
    if (above < want && want <= above + sum) {                 // exactly one thread
        for (int j = 0; j < per; ++j) {
            if (want <= above + h[j]) {
                const uint32_t digit = (uint32_t)(bins - 1 - (threadIdx.x * per + j));
                ws[kState] = pass == 0 ? digit : ((prefix << 10) | digit);
                ws[kState + 1] = want - above;
                break;
            }
            above += h[j];
        }
    }
}

// pass 4: chunk c's numbers of keys above and equal to the threshold
__global__ __launch_bounds__(kBlock) void k_topk_count(const f32x4 *e, int64_t nvec, int64_t nchunks,
                                                       uint32_t *ws) {
    __shared__ uint32_t lds[kBlock / 64];
    const uint32_t T = ws[kState];
    const int64_t v0 = (int64_t)blockIdx.x * (kBlock * kVecs);
    uint32_t packed = 0;  // gt in the low half, eq in the high half (each <= kChunk)
    f32x4 q[kVecs];
#pragma unroll
    for (int v = 0; v < kVecs; ++v) {
        const int64_t i = v0 + (int64_t)v * kBlock + threadIdx.x;
        if (i < nvec) q[v] = e[i];
    }
#pragma unroll
    for (int v = 0; v < kVecs; ++v) {
        const int64_t i = v0 + (int64_t)v * kBlock + threadIdx.x;
        if (i < nvec) {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t key = key_of(q[v][j]);
                packed += (key > T ? 1u : 0u) + (key == T ? 0x10000u : 0u);
            }
        }
    }
    packed = wave_sum(packed);
    if (lane_id() == 0) lds[threadIdx.x >> 6] = packed;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t s = 0;
        for (int wv = 0; wv < kBlock / 64; ++wv) s += lds[wv];
        ws[kCounts + blockIdx.x] = s & 0xffffu;
        ws[kCounts + (nchunks + 1) + blockIdx.x] = s >> 16;
    }
}

// One block: both count arrays become exclusive prefixes, entry nchunks the totals.
__global__ __launch_bounds__(kScanBlock) void k_topk_scan(uint32_t *ws, int64_t nchunks, int32_t k,
                                                          int32_t *stats) {
    __shared__ uint32_t lds[kScanBlock / 64];
    const int64_t per = (nchunks + kScanBlock - 1) / kScanBlock;
    const int64_t a = (int64_t)threadIdx.x * per < nchunks ? (int64_t)threadIdx.x * per : nchunks;
    const int64_t b = a + per < nchunks ? a + per : nchunks;
    for (int arr = 0; arr < 2; ++arr) {
        uint32_t *cnt = ws + kCounts + arr * (nchunks + 1);
        uint32_t sum = 0;
        for (int64_t c = a; c < b; ++c) sum += cnt[c];
        uint32_t total;
        uint32_t run = block_scan_excl<kScanBlock>(sum, lds, total);
        for (int64_t c = a; c < b; ++c) {
            const uint32_t own = cnt[c];
            cnt[c] = run;
            run += own;
        }
        if (threadIdx.x == 0) cnt[nchunks] = total;
    }
    if (threadIdx.x == 0) {
        stats[0] = k;
        stats[1] = (int32_t)ws[kState + 2];
    }
}

// pass 5: thread t of chunk c owns the 16 consecutive coordinates from c * kChunk + 16 t
__global__ __launch_bounds__(kBlock) void k_topk_write(f32x4 *e, int64_t nvec, int64_t nchunks,
                                                       const uint32_t *ws, int64_t k, int32_t *idx,
                                                       float *val) {
    __shared__ uint32_t lds[kBlock / 64];
    const uint32_t T = ws[kState], need = ws[kState + 1];
    const uint32_t *gt = ws + kCounts, *eq = gt + (nchunks + 1);
    const uint32_t G0 = gt[blockIdx.x], E0 = eq[blockIdx.x];
    // nothing of this chunk is selected: no larger key, and no equal one early enough
    if (gt[blockIdx.x + 1] == G0 && (eq[blockIdx.x + 1] == E0 || E0 >= need)) return;
    const int64_t v0 = (int64_t)blockIdx.x * (kBlock * kVecs) + (int64_t)threadIdx.x * kVecs;
    f32x4 q[kVecs];
    uint32_t packed = 0;
#pragma unroll
    for (int v = 0; v < kVecs; ++v) {
        if (v0 + v < nvec) {
            q[v] = e[v0 + v];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t key = key_of(q[v][j]);
                packed += (key > T ? 1u : 0u) + (key == T ? 0x10000u : 0u);
            }
        }
    }
    uint32_t total;
    const uint32_t before = block_scan_excl<kBlock>(packed, lds, total);
    uint32_t G = G0 + (before & 0xffffu), E = E0 + (before >> 16);
#pragma unroll
    for (int v = 0; v < kVecs; ++v) {
        if (v0 + v < nvec) {
            bool any = false;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t key = key_of(q[v][j]);
                const bool above = key > T, equal = key == T;
                if (above || (equal && E < need)) {
                    const int64_t pos = (int64_t)G + (E < need ? E : need);
                    if (pos < k) {  // always, when the histograms are the keys' own
                        idx[pos] = (int32_t)((v0 + v) * 4 + j);
                        val[pos] = q[v][j];
                    }
                    q[v][j] = 0.f;
                    any = true;
                }
                G += above;
                E += equal;
            }
            if (any) e[v0 + v] = q[v];
        }
    }
}

// ---------------------------------------------------------------- sparse FedAvg
constexpr int kTile = 2048;  // coordinates per wave
constexpr int kWave = 64;

// first position in [lo, hi) whose index is >= c
__device__ __forceinline__ int64_t lower_bound(const int32_t *idx, int64_t lo, int64_t hi, int64_t c) {
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if ((int64_t)idx[mid] < c) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kWave) void k_sparse_fedavg(const float *base, const int32_t *idx,
                                                         const float *val, const int64_t *off,
                                                         const float *weight, int K, FastDiv d,
                                                         int64_t P, float *out) {
    __shared__ float acc[kTile];
    __shared__ uint8_t has[kTile];
    __shared__ int64_t seg_lo[kWave], seg_hi[kWave];
    __shared__ float seg_w[kWave];
    const int lane = threadIdx.x;
    const int64_t c0 = (int64_t)blockIdx.x * kTile;
    const int64_t c1 = c0 + kTile < P ? c0 + kTile : P;
    for (int t = lane; t < kTile; t += kWave) has[t] = 0;
    for (int k0 = 0; k0 < K; k0 += kWave) {
        __syncthreads();  // the previous batch's table has been read; has[] is cleared
        const int nb = K - k0 < kWave ? K - k0 : kWave;
        if (lane < nb) {
            const int64_t a = off[k0 + lane], b = off[k0 + lane + 1];
            const int64_t lo = lower_bound(idx, a, b, c0);
            seg_lo[lane] = lo;
            seg_hi[lane] = lower_bound(idx, lo, b, c1);
            seg_w[lane] = weight[k0 + lane];
        }
        __syncthreads();
        for (int i = 0; i < nb; ++i) {
            const int64_t lo = seg_lo[i], hi = seg_hi[i];
            const float n = seg_w[i];
            for (int64_t p = lo + lane; p < hi; p += kWave) {
                const uint32_t t = (uint32_t)((int64_t)idx[p] - c0);
                if (t < (uint32_t)kTile) {  // always, for ascending in-range indices
                    const float term = div_exact(val[p] * n, d);
                    acc[t] = has[t] ? acc[t] + term : term;
                    has[t] = 1;
                }
            }
            __syncthreads();  // client i is applied before client i + 1 reads acc
        }
    }
    const f32x4 *bv = reinterpret_cast<const f32x4 *>(base + c0);
    f32x4 *ov = reinterpret_cast<f32x4 *>(out + c0);
    const int nv = (int)((c1 - c0) / 4);
    for (int v = lane; v < nv; v += kWave) {
        f32x4 q = ldg_nt(bv + v);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (has[4 * v + j]) q[j] = q[j] + acc[4 * v + j];
        ov[v] = q;
    }
}

// [a, a + na) and [b, b + nb) bytes intersect
inline bool overlap(const void *a, int64_t na, const void *b, int64_t nb) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + (uintptr_t)nb && b0 < a0 + (uintptr_t)na;
}

constexpr int64_t kMaxP = (int64_t)1 << 31;

}  // namespace
}  // namespace dls

using namespace dls;

extern "C" int64_t dls_topk_workspace(int64_t P) {
    DLS_REQUIRE(P >= 1 && P < kMaxP, DLS_EINVAL, "dls_topk_workspace: P=%lld (1 <= P < 2^31)",
                (long long)P);
    return (int64_t)sizeof(uint32_t) * (kCounts + 2 * (chunks_of(P) + 1));
}

extern "C" int dls_topk_compress_f32(const float *w, const float *base, float *e, int64_t P,
                                     int64_t k, int32_t *idx, float *val, int32_t *stats,
                                     void *workspace, dls_stream_t stream) {
    const char *fn = "dls_topk_compress_f32";
    DLS_REQUIRE(w && base && e && idx && val && stats && workspace, DLS_EINVAL,
                "%s: null pointer (w, base, e, idx, val, stats, workspace)", fn);
    DLS_REQUIRE(P >= 1 && P < kMaxP, DLS_EINVAL, "%s: P=%lld (1 <= P < 2^31)", fn, (long long)P);
    DLS_REQUIRE(k >= 1 && k <= P, DLS_EINVAL, "%s: k=%lld (1 <= k <= P=%lld)", fn, (long long)k,
                (long long)P);
    DLS_REQUIRE(P % 4 == 0, DLS_ELAYOUT, "%s: P=%lld must be a multiple of 4", fn, (long long)P);
    DLS_REQUIRE(aligned16(w) && aligned16(base) && aligned16(e) && aligned16(val) && aligned16(idx) &&
                    aligned16(workspace),
                DLS_ELAYOUT, "%s: 16-byte alignment of w, base, e, val, idx and workspace", fn);
    DLS_REQUIRE((reinterpret_cast<uintptr_t>(stats) & 3u) == 0, DLS_ELAYOUT,
                "%s: 4-byte alignment of stats", fn);
    DLS_REQUIRE(!overlap(e, 4 * P, w, 4 * P) && !overlap(e, 4 * P, base, 4 * P), DLS_EINVAL,
                "%s: e must not alias w or base", fn);
    hipStream_t st = as_stream(stream);
    uint32_t *ws = static_cast<uint32_t *>(workspace);
    const int64_t nvec = P / 4, nchunks = chunks_of(P);
    const unsigned hist_grid = (unsigned)std::min<int64_t>(nchunks, kHistBlocks);
    const f32x4 *ev = reinterpret_cast<const f32x4 *>(e);
    const hipError_t me = hipMemsetAsync(ws, 0, sizeof(uint32_t) * kCounts, st);
    DLS_REQUIRE(me == hipSuccess, (int)me, "%s: %s", fn, hipGetErrorString(me));
    hipLaunchKernelGGL(k_topk_form, dim3(hist_grid), dim3(kBlock), 0, st,
                       reinterpret_cast<const f32x4 *>(w), reinterpret_cast<const f32x4 *>(base),
                       reinterpret_cast<f32x4 *>(e), nvec, ws);
    hipLaunchKernelGGL(k_topk_pick, dim3(1), dim3(kBlock), 0, st, ws, 0, kBins, (uint32_t)k);
    hipLaunchKernelGGL(k_topk_refine<1>, dim3(hist_grid), dim3(kBlock), 0, st, ev, nvec, ws);
    hipLaunchKernelGGL(k_topk_pick, dim3(1), dim3(kBlock), 0, st, ws, 1, 1024, 0u);
    hipLaunchKernelGGL(k_topk_refine<2>, dim3(hist_grid), dim3(kBlock), 0, st, ev, nvec, ws);
    hipLaunchKernelGGL(k_topk_pick, dim3(1), dim3(kBlock), 0, st, ws, 2, 1024, 0u);
    hipLaunchKernelGGL(k_topk_count, dim3((unsigned)nchunks), dim3(kBlock), 0, st, ev, nvec, nchunks,
                       ws);
    hipLaunchKernelGGL(k_topk_scan, dim3(1), dim3(kScanBlock), 0, st, ws, nchunks, (int32_t)k, stats);
    hipLaunchKernelGGL(k_topk_write, dim3((unsigned)nchunks), dim3(kBlock), 0, st,
                       reinterpret_cast<f32x4 *>(e), nvec, nchunks, ws, k, idx, val);
    return check_launch(fn);
}

extern "C" int dls_sparse_fedavg_f32(const float *base, const int32_t *idx, const float *val,
                                     const int64_t *off, const float *weight, int32_t K,
                                     float total, int64_t P, float *out, dls_stream_t stream) {
    const char *fn = "dls_sparse_fedavg_f32";
    // idx and val may both be null when every segment is empty: they are then never read
    DLS_REQUIRE(base && off && weight && out && (idx != nullptr) == (val != nullptr), DLS_EINVAL,
                "%s: null pointer (base, off, weight, out; idx and val only together)", fn);
    DLS_REQUIRE(K >= 1, DLS_EINVAL, "%s: K=%d (K >= 1)", fn, K);
    DLS_REQUIRE(P >= 1 && P < kMaxP, DLS_EINVAL, "%s: P=%lld (1 <= P < 2^31)", fn, (long long)P);
    DLS_REQUIRE(P % 4 == 0, DLS_ELAYOUT, "%s: P=%lld must be a multiple of 4", fn, (long long)P);
    DLS_REQUIRE(aligned16(base) && aligned16(out), DLS_ELAYOUT,
                "%s: 16-byte alignment of base and out", fn);
    DLS_REQUIRE(!overlap(out, 4 * P, base, 4 * P), DLS_EINVAL, "%s: out must not alias base", fn);
    hipLaunchKernelGGL(k_sparse_fedavg, dim3((unsigned)((P + kTile - 1) / kTile)), dim3(kWave), 0,
                       as_stream(stream), base, idx, val, off, weight, (int)K, make_fastdiv(total), P,
                       out);
    return check_launch(fn);
}
