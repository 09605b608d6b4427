// FetchSGD's Count Sketch for gfx950 (Rothchild et al. 2020, "FetchSGD: Communication-
// Efficient Federated Learning with Sketching"; Charikar, Chen & Farach-Colton 2002): the
// client's sketch and the server's median-of-rows inverse.  include/dls_hip.h has the
// contract.
//
// A textbook Count Sketch is a scatter with floating-point atomics.  Here the hash of
// coordinate j = q C + t in row r is t ^ m_r(q), one mask per block of C coordinates and row,
// so bucket b of row r receives exactly the coordinate q C + (b ^ m_r(q)) of every block q:
// the sketch is a gather whose sum has a stated order, and the inverse reads one bucket per
// row.
//
// k_sketch.  A 256-thread workgroup owns the aligned tile of 1024 buckets `tile` of one row
// and a range of segments of DLS_SKETCH_QSEG = 32 blocks; a thread owns 4 consecutive
// buckets in 4 registers.  With m = m_r(q), of the mask's bits
//   10..     the tile's sources in block q are the aligned 1024-coordinate tile tile ^ (m >> 10),
//   2..9     the thread reads that tile's quad tid ^ ((m >> 2) & 255) as one 16-byte load: the
//            bits 8-9 pick which wave's 1 KB span a wave reads, the bits 2-7 permute its lanes
//            inside the span, so every wave load is one full aligned 1 KB line set,
//   0..1     the four components are swapped in registers.
// m is uniform in the workgroup.  Per segment every lane of a wave makes two Philox calls:
// lane l draws m of the segment's block l / 2 (the wave reads step i's mask from lane 2 i with
// v_readlane) and then half l % 2 of the 256 sign bits of the span its wave reads in that
// block, 64 calls for the 32 steps of the wave, kept in 1 KB of LDS per wave; at step i a lane
// picks its word, one of 8, with one LDS read (the 64 lanes read 8 addresses: a broadcast).
// Steps are walked four at a time so that four (with base: eight) loads are in flight per
// lane.  Segment partials and their sum follow the contract's order; with few tiles the
// segments are spread over workgroups, the partials go through the workspace and k_combine
// adds them in segment order: the same bits either way.
//
// The row-0 workgroups see every coordinate exactly once and count the non-finite ones; the
// counts meet in the stream's cell as in dls_drive_compress_f32 (one integer atomic per
// workgroup, no fence).
//
// k_unsketch.  A workgroup owns 1024 consecutive coordinates (one block q, since C >= 1024),
// a thread 4.  The first wave draws the 8 R sign blocks of the span, the second the R masks;
// then per row one 16-byte load of the table quad ((j % C) ^ m) & ~3, the same component
// swap, the signs, and the median on integer keys: v_med3_i32 for R = 3, med3 of the two
// middle candidates for 5, a compare-exchange network for 7.
#include "philox_common.h"

namespace dls {
namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kTile = 4 * kBlock;          // buckets (sketch) or coordinates (unsketch) per workgroup
constexpr int kQSeg = DLS_SKETCH_QSEG;     // blocks per segment
constexpr int kMaxRows = DLS_SKETCH_MAX_ROWS;
constexpr int kMinC = 1024, kMaxLogC = 24;
constexpr int64_t kMaxP = (int64_t)1 << 31;
constexpr int64_t kSpreadBelow = 1024;     // fewer single-pass workgroups than this: spread segments
constexpr uint64_t kSignBlock0 = (uint64_t)1 << 30;  // Philox block of coordinate 2^32
static_assert(kTile == kMinC && kQSeg == 32, "a wave's 64 lanes draw the 2 x 32 sign blocks of a segment");

__device__ __forceinline__ uint32_t uniform(uint32_t v) { return __builtin_amdgcn_readfirstlane(v); }

__device__ __forceinline__ uint32_t word_of(const u32x4 &b, int k) {  // k uniform
    return k == 0 ? b[0] : k == 1 ? b[1] : k == 2 ? b[2] : b[3];
}

// m_r(q)
__device__ __forceinline__ uint32_t mask_of(int64_t q, int r, uint32_t cmask, const PhiloxKey &key) {
    return word_of(philox_block((uint64_t)(2 * q + (r >> 2)), key), r & 3) & cmask;
}

// the 128 sign bits of the coordinates 128 g .. 128 g + 127 in row r
__device__ __forceinline__ u32x4 sign_block(int64_t g, int r, const PhiloxKey &key) {
    return philox_block(kSignBlock0 + ((uint64_t)r << 24) + (uint64_t)g, key);
}

// component c of the result is component c ^ x of v (x uniform, 0..3)
__device__ __forceinline__ f32x4 swap_components(f32x4 v, uint32_t x) {
    if (x & 1) v = f32x4{v[1], v[0], v[3], v[2]};
    if (x & 2) v = f32x4{v[2], v[3], v[0], v[1]};
    return v;
}

// bit k of nib flips the sign of component k
__device__ __forceinline__ f32x4 apply_signs(f32x4 v, uint32_t nib) {
#pragma unroll
    for (int k = 0; k < 4; ++k)
        v[k] = __uint_as_float(__float_as_uint(v[k]) ^ (((nib >> k) & 1u) << 31));
    return v;
}

__device__ __forceinline__ uint32_t nonfinite(f32x4 v) {
    uint32_t n = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) n += (__float_as_uint(v[k]) & 0x7fffffffu) >= 0x7f800000u;
    return n;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

struct SketchShape {
    int64_t P, NQ;   // coordinates, blocks
    int R, logC;
    int nseg, segs_per;  // segments in all and per workgroup
};

// grid: ((segment range z * R + r) * tiles + tile); out: the table (segs_per == nseg) or the
// workspace's partials [z][r][C]
template <bool HAS_BASE>
__global__ __launch_bounds__(kBlock) void k_sketch(const float *__restrict__ w,
                                                   const float *__restrict__ base, SketchShape sh,
                                                   PhiloxKey key, float *__restrict__ out,
                                                   int32_t *__restrict__ stats,
                                                   unsigned long long *cell) {
    __shared__ u32x4 sgn[kWaves][2 * kQSeg];
    __shared__ uint32_t lbad[kWaves];
    const int tid = threadIdx.x, lane = lane_id();
    const int wave = uniform(tid >> 6);
    const uint32_t ntiles = 1u << (sh.logC - 10), cmask = (1u << sh.logC) - 1u;
    const uint32_t tile = blockIdx.x & (ntiles - 1), zr = blockIdx.x >> (sh.logC - 10);
    const int z = zr / (uint32_t)sh.R, r = zr - z * sh.R;
    const int s0 = z * sh.segs_per, s1 = s0 + sh.segs_per < sh.nseg ? s0 + sh.segs_per : sh.nseg;
    const uint32_t *words = reinterpret_cast<const uint32_t *>(&sgn[wave][0]);
    f32x4 tot = {0.f, 0.f, 0.f, 0.f};
    uint32_t nbad = 0;
    for (int s = s0; s < s1; ++s) {
        const int64_t q0 = (int64_t)s * kQSeg;
        const int nq = sh.NQ - q0 < kQSeg ? (int)(sh.NQ - q0) : kQSeg;
        // the lane's two draws: the mask of block q0 + lane / 2 and half lane % 2 of the sign
        // bits of the 256 coordinates this wave reads there (a block past NQ: never used)
        const int64_t ql = q0 + (lane >> 1);
        const uint32_t mv = mask_of(ql, r, cmask, key);
        const int64_t span = (ql << sh.logC) + ((int64_t)(tile ^ (mv >> 10)) << 10) +
                             ((wave ^ ((mv >> 8) & 3u)) << 8);
        __syncthreads();  // the previous segment's words have been read
        sgn[wave][lane] = sign_block((span >> 7) + (lane & 1), r, key);
        __syncthreads();
        f32x4 seg = {0.f, 0.f, 0.f, 0.f};
        for (int i0 = 0; i0 < nq; i0 += 4) {
            uint32_t m[4];
            bool in[4];
            f32x4 v[4], vb[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) {  // steps past nq load coordinate 0 and are dropped
                m[a] = __builtin_amdgcn_readlane(mv, 2 * ((i0 + a) & (kQSeg - 1)));
                const int64_t j = ((q0 + i0 + a) << sh.logC) + ((int64_t)(tile ^ (m[a] >> 10)) << 10) +
                                  ((tid ^ ((m[a] >> 2) & 255u)) << 2);
                in[a] = i0 + a < nq && j < sh.P;
                const int64_t js = in[a] ? j : 0;
                v[a] = *reinterpret_cast<const f32x4 *>(w + js);
                if constexpr (HAS_BASE) vb[a] = *reinterpret_cast<const f32x4 *>(base + js);
            }
#pragma unroll
            for (int a = 0; a < 4; ++a) {
                if (i0 + a >= nq) break;
                f32x4 u = v[a];
                if constexpr (HAS_BASE) u = u - vb[a];
                if (!in[a]) u = f32x4{0.f, 0.f, 0.f, 0.f};  // j >= P: +0.0, no sign
                nbad += nonfinite(u);
                const uint32_t qd = lane ^ ((m[a] >> 2) & 63u);  // the lane's quad in the span
                const uint32_t word = words[8 * (i0 + a) + (qd >> 3)];
                u = apply_signs(u, in[a] ? (word >> ((qd & 7u) * 4)) & 15u : 0u);
                u = swap_components(u, m[a] & 3u);
                seg = i0 + a == 0 ? u : seg + u;
            }
        }
        tot = s == s0 ? seg : tot + seg;
    }
    *reinterpret_cast<f32x4 *>(out + (((int64_t)zr << sh.logC) + ((int64_t)tile << 10) + 4 * tid)) = tot;
    if (r != 0) return;
    nbad = wave_sum(nbad);
    if (lane == 0) lbad[wave] = nbad;
    __syncthreads();
    if (tid == 0) {
        nbad = lbad[0] + lbad[1] + lbad[2] + lbad[3];
        const uint32_t tickets = ntiles * (uint32_t)((sh.nseg + sh.segs_per - 1) / sh.segs_per);
        const unsigned long long before = atomicAdd(cell, (1ull << 32) | nbad);
        if ((before >> 32) == tickets - 1) {  // every other row-0 workgroup's count is in `before`
            stats[0] = (int32_t)((uint32_t)before + nbad);
            atomicExch(cell, 0ull);
        }
    }
}

// table[i] = the partials part[s][i], s ascending, the first assigning; n4 quads per partial
__global__ __launch_bounds__(kBlock) void k_combine(const f32x4 *__restrict__ part, int nseg,
                                                    int64_t n4, f32x4 *__restrict__ table) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n4) return;
    f32x4 acc = part[i];
#pragma unroll 8
    for (int s = 1; s < nseg; ++s) acc = acc + part[s * n4 + i];
    table[i] = acc;
}

// the total order on bit patterns: an involution
__device__ __forceinline__ int32_t to_key(int32_t b) { return b >= 0 ? b : b ^ 0x7fffffff; }

__device__ __forceinline__ void order(int32_t &a, int32_t &b) {
    const int32_t lo = min(a, b), hi = max(a, b);
    a = lo;
    b = hi;
}

__device__ __forceinline__ int32_t med3(int32_t a, int32_t b, int32_t c) {
    return max(min(a, b), min(max(a, b), c));  // v_med3_i32
}

template <int R>
__device__ __forceinline__ int32_t median(int32_t (&k)[R]) {
    if constexpr (R == 1) return k[0];
    if constexpr (R == 3) return med3(k[0], k[1], k[2]);
    if constexpr (R == 5)  // the median is neither below two pair minima nor above two pair maxima
        return med3(k[4], max(min(k[0], k[1]), min(k[2], k[3])), min(max(k[0], k[1]), max(k[2], k[3])));
    if constexpr (R == 7) {  // odd-even transposition sort, 7 rounds; the dead exchanges fold away
#pragma unroll
        for (int round = 0; round < R; ++round)
#pragma unroll
            for (int i = round & 1; i + 1 < R; i += 2) order(k[i], k[i + 1]);
        return k[R / 2];
    }
}

template <int R>
__global__ __launch_bounds__(kBlock) void k_unsketch(const float *__restrict__ table, int64_t P,
                                                     int logC, PhiloxKey key,
                                                     float *__restrict__ est) {
    __shared__ u32x4 sgn[R][8];
    __shared__ uint32_t ms[R];
    const int tid = threadIdx.x;
    const int64_t j0 = (int64_t)blockIdx.x * kTile;
    const uint32_t cmask = (1u << logC) - 1u;
    if (tid < 8 * R) sgn[tid >> 3][tid & 7] = sign_block((j0 >> 7) + (tid & 7), tid >> 3, key);
    if (tid >= 64 && tid < 64 + R) ms[tid - 64] = mask_of(j0 >> logC, tid - 64, cmask, key);
    __syncthreads();
    const int64_t j = j0 + 4 * tid;
    if (j >= P) return;
    const uint32_t t = ((uint32_t)j0 & cmask) + 4 * tid;
    int32_t k[4][R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const uint32_t m = uniform(ms[r]);
        f32x4 e = *reinterpret_cast<const f32x4 *>(table + (((int64_t)r << logC) + ((t ^ m) & ~3u)));
        e = swap_components(e, m & 3u);
        const uint32_t word = reinterpret_cast<const uint32_t *>(&sgn[r][0])[tid >> 3];
        e = apply_signs(e, (word >> ((tid & 7) * 4)) & 15u);
#pragma unroll
        for (int c = 0; c < 4; ++c) k[c][r] = to_key(__float_as_int(e[c]));
    }
    f32x4 o;
#pragma unroll
    for (int c = 0; c < 4; ++c) o[c] = __int_as_float(to_key(median<R>(k[c])));
    *reinterpret_cast<f32x4 *>(est + j) = o;
}

// [a, a + na) and [b, b + nb) bytes intersect
inline bool overlap(const void *a, int64_t na, const void *b, int64_t nb) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + (uintptr_t)nb && b0 < a0 + (uintptr_t)na;
}

inline int log2_of(int64_t C) {
    int l = 0;
    while (((int64_t)1 << l) < C) ++l;
    return l;
}

inline int check_shape(const char *fn, int64_t P, int32_t R, int64_t C) {
    DLS_REQUIRE(R >= 1 && R <= kMaxRows && (R & 1), DLS_EINVAL, "%s: R=%d (1, 3, 5 or 7)", fn, R);
    DLS_REQUIRE(C >= kMinC && C <= ((int64_t)1 << kMaxLogC) && (C & (C - 1)) == 0, DLS_EINVAL,
                "%s: C=%lld (a power of two in 1024..2^24)", fn, (long long)C);
    DLS_REQUIRE(P >= 4 && P < kMaxP, DLS_EINVAL, "%s: P=%lld (4 <= P < 2^31)", fn, (long long)P);
    return DLS_OK;
}

inline int check_layout(const char *fn, int64_t P) {
    DLS_REQUIRE(P % 4 == 0, DLS_ELAYOUT, "%s: P=%lld must be a multiple of 4", fn, (long long)P);
    return DLS_OK;
}

// how dls_sketch_f32 splits the work: a function of (P, R, C) alone
inline SketchShape shape_of(int64_t P, int32_t R, int64_t C) {
    SketchShape sh;
    sh.P = P;
    sh.R = R;
    sh.logC = log2_of(C);
    sh.NQ = (P + C - 1) >> sh.logC;
    sh.nseg = (int)((sh.NQ + kQSeg - 1) / kQSeg);
    const bool spread = sh.nseg > 1 && (C / kTile) * R < kSpreadBelow;
    sh.segs_per = spread ? 1 : sh.nseg;
    return sh;
}

}  // namespace
}  // namespace dls

using namespace dls;

extern "C" int64_t dls_sketch_workspace(int64_t P, int32_t R, int64_t C) {
    const char *fn = "dls_sketch_workspace";
    int rc = check_shape(fn, P, R, C);
    if (rc == DLS_OK) rc = check_layout(fn, P);
    if (rc != DLS_OK) return rc;
    const SketchShape sh = shape_of(P, R, C);
    return sh.segs_per == sh.nseg ? 16 : (int64_t)sh.nseg * R * C * 4;
}

extern "C" int dls_sketch_f32(const float *w, const float *base, int64_t P, int32_t R, int64_t C,
                              uint64_t seed, uint64_t stream_id, float *table, int32_t *stats,
                              void *workspace, dls_stream_t stream) {
    const char *fn = "dls_sketch_f32";
    DLS_REQUIRE(w && table && stats && workspace, DLS_EINVAL,
                "%s: null pointer (w, table, stats, workspace; base may be null)", fn);
    int rc = check_shape(fn, P, R, C);
    if (rc == DLS_OK) rc = check_layout(fn, P);
    if (rc != DLS_OK) return rc;
    DLS_REQUIRE(aligned16(w) && aligned16(base) && aligned16(table) && aligned16(stats) &&
                    aligned16(workspace),
                DLS_ELAYOUT, "%s: 16-byte alignment of w, base, table, stats and workspace", fn);
    const SketchShape sh = shape_of(P, R, C);
    const bool spread = sh.segs_per != sh.nseg;
    const int64_t nt = (int64_t)R * C * 4, nws = spread ? nt * sh.nseg : 16;
    const float *in[2] = {w, base};
    for (const float *x : in)
        DLS_REQUIRE(!x || (!overlap(table, nt, x, 4 * P) && !overlap(stats, 4, x, 4 * P) &&
                           !overlap(workspace, nws, x, 4 * P)),
                    DLS_EINVAL, "%s: table, stats and workspace must not alias w or base", fn);
    DLS_REQUIRE(!overlap(table, nt, stats, 4) && !overlap(table, nt, workspace, nws) &&
                    !overlap(workspace, nws, stats, 4),
                DLS_EINVAL, "%s: table, stats and workspace must not alias each other", fn);
    hipStream_t st = as_stream(stream);
    unsigned long long *cell = stream_cell(st);
    DLS_REQUIRE(cell, DLS_EINVAL, "%s: no device memory for the stream's counter cell", fn);
    const int64_t groups = (sh.nseg + sh.segs_per - 1) / sh.segs_per;
    const dim3 grid((unsigned)(groups * R * (C / kTile)));
    float *out = spread ? static_cast<float *>(workspace) : table;
    const PhiloxKey key = make_key(seed, stream_id);
    if (base)
        hipLaunchKernelGGL(k_sketch<true>, grid, dim3(kBlock), 0, st, w, base, sh, key, out, stats, cell);
    else
        hipLaunchKernelGGL(k_sketch<false>, grid, dim3(kBlock), 0, st, w, base, sh, key, out, stats, cell);
    if (spread) {
        rc = check_launch(fn);
        if (rc != DLS_OK) return rc;
        const int64_t n4 = (int64_t)R * C / 4;
        hipLaunchKernelGGL(k_combine, dim3((unsigned)((n4 + kBlock - 1) / kBlock)), dim3(kBlock), 0, st,
                           static_cast<const f32x4 *>(workspace), sh.nseg, n4,
                           reinterpret_cast<f32x4 *>(table));
    }
    return check_launch(fn);
}

extern "C" int dls_unsketch_f32(const float *table, int64_t P, int32_t R, int64_t C, uint64_t seed,
                                uint64_t stream_id, float *est, dls_stream_t stream) {
    const char *fn = "dls_unsketch_f32";
    DLS_REQUIRE(table && est, DLS_EINVAL, "%s: null pointer (table, est)", fn);
    int rc = check_shape(fn, P, R, C);
    if (rc == DLS_OK) rc = check_layout(fn, P);
    if (rc != DLS_OK) return rc;
    DLS_REQUIRE(aligned16(table) && aligned16(est), DLS_ELAYOUT,
                "%s: 16-byte alignment of table and est", fn);
    DLS_REQUIRE(!overlap(est, 4 * P, table, (int64_t)R * C * 4), DLS_EINVAL,
                "%s: est must not alias table", fn);
    const dim3 grid((unsigned)((P + kTile - 1) / kTile));
    const int logC = log2_of(C);
    const PhiloxKey key = make_key(seed, stream_id);
    hipStream_t st = as_stream(stream);
    switch (R) {
        case 1: hipLaunchKernelGGL(k_unsketch<1>, grid, dim3(kBlock), 0, st, table, P, logC, key, est); break;
        case 3: hipLaunchKernelGGL(k_unsketch<3>, grid, dim3(kBlock), 0, st, table, P, logC, key, est); break;
        case 5: hipLaunchKernelGGL(k_unsketch<5>, grid, dim3(kBlock), 0, st, table, P, logC, key, est); break;
        default: hipLaunchKernelGGL(k_unsketch<7>, grid, dim3(kBlock), 0, st, table, P, logC, key, est); break;
    }
    return check_launch(fn);
}
