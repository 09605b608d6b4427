// Width-heterogeneous FedAvg (HeteroFL, Diao, Ding & Tarokh 2021; FedRolex, Alam et al. 2022)
// for gfx950: the server's round and the downlink, one launch each, over clients whose rows have
// different lengths.  Every parameter tensor is an [O, I, R] array; a width level holds a
// (rolled) window of O_l x I_l of its first two dimensions as its own compact tensor
// (include/dls_hip.h has the plan's encoding and the contracts; tests/hetero_ref.py restates
// them in numpy float32).
//
// How the work is split.  A tile is DLS_HETERO_TILE = 1024 consecutive elements of one global
// tensor (its 64-element padding included), a block of 256 threads walks tiles blockIdx.x,
// blockIdx.x + gridDim.x, ... and a lane owns 4 consecutive elements, so `prev` is read and
// `out` written as 16-byte vectors whatever the tensor.  The tile finds its tensor by a
// binary search of the plan's tile prefix (wave-uniform loads), then the block stages the
// tensor's record (12 words and 8 per level) in LDS; the per-client {level, weight, row start}
// were staged once per block (16 KiB at K = 1024).  Both are read back at wave-uniform
// addresses and moved to SGPRs, so a client's row base is a scalar.
//
// Where a lane's elements live in a level's compact row depends on the lane and the level, not
// on the client, so it is computed once per tile: (o, i, r) by multiply-high division with the
// plan's constants for I*R and R (no integer divide on the device), then per level the window
// test and the compact index, kept in LDS as s_idx[level][lane] (32 KiB; a register array
// indexed by a client's level would live in scratch).  The client loop then costs one LDS read,
// the row load and the arithmetic.  A level whose window misses the tile's whole o-range is
// skipped wave-uniformly before the LDS read: the rows of narrow clients are only read where
// they exist, sum_k 4 P_k + 8 P bytes in all.
//
// Two paths with the same bits.  Vector path (shift 0, I*R and every I_l*R multiples of 4): a
// lane's 4 elements are wholly held or wholly absent and consecutive in the compact row: one
// index, one non-temporal 16-byte load per client, kRowUnroll clients in flight.  Element path
// (rolled windows, odd row lengths): 4 indices per lane and level, 4-byte loads, 2 clients in
// flight.  Both add fl(w * u) in ascending client order from -0 ("the first member assigns":
// -0 + t == t for every t), sum the members' weights the same way and divide once, IEEE.
//
// k_extract walks the same tiles, reads the global row once and scatters every element to
// each level that holds it (16-byte stores on the vector path); tile 0 of a tensor also zeroes
// the levels' padding.  No atomics anywhere; nothing depends on the grid size.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "rows_common.h"

namespace dls {
namespace {

constexpr int kBlock = 256;
constexpr int kTile = DLS_HETERO_TILE;
constexpr int kL = DLS_HETERO_MAX_LEVELS;
constexpr int kHdr = DLS_HETERO_HEADER_WORDS;
constexpr int kHead = DLS_HETERO_TENSOR_WORDS;
constexpr int kLev = DLS_HETERO_LEVEL_WORDS;
constexpr int kRec = kHead + kL * kLev;  // words of one tensor's record
constexpr int kRowUnroll = 8;
static_assert(kTile == 4 * kBlock, "a lane owns 4 elements of the tile");

// word numbers of a tensor record's head and of a level record (include/dls_hip.h)
enum { H_GOFF, H_O, H_I, H_R, H_MIR, H_SIR, H_MR, H_SR, H_FAST, H_NUMEL, H_IR, H_PAD };
enum { V_OFF, V_O, V_I, V_SHO, V_SHI, V_IR, V_LEN, V_RES };

// floor(n / d) for n < 2^31 from the plan's (m, s) of d: m = floor(2^(31 + l) / d) + 1 and
// s = l - 1 with l = ceil(log2 d); m = 0 stands for d = 1.  With err = m d - 2^(31 + l) in
// (0, d] the quotient's excess n err / (d 2^(31 + l)) stays below 1 / d, so the floor is exact.
__device__ __forceinline__ int mdiv(int n, uint32_t m, uint32_t s) {
    return m ? (int)(__umulhi((uint32_t)n, m) >> s) : n;
}

inline void make_magic(uint32_t d, uint32_t *m, uint32_t *s) {
    if (d == 1) {
        *m = *s = 0;
        return;
    }
    int l = 0;
    while ((1ull << l) < d) ++l;
    *m = (uint32_t)((1ull << (31 + l)) / d + 1);
    *s = (uint32_t)(l - 1);
}

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

// The tile's tensor: the first t with tile < tile_end[t].
__device__ __forceinline__ int find_tensor(const int32_t *tile_end, int T, int tile) {
    int lo = 0, hi = T - 1;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (tile >= tile_end[mid]) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

struct Head {
    int goff, O, I, R, fast, numel, IR, pad;
    uint32_t mIR, sIR, mR, sR;
};

__device__ __forceinline__ Head load_head(const int32_t *s_rec) {
    Head h;
    h.goff = uni(s_rec[H_GOFF]);
    h.O = uni(s_rec[H_O]);
    h.I = uni(s_rec[H_I]);
    h.R = uni(s_rec[H_R]);
    h.mIR = (uint32_t)uni(s_rec[H_MIR]);
    h.sIR = (uint32_t)uni(s_rec[H_SIR]);
    h.mR = (uint32_t)uni(s_rec[H_MR]);
    h.sR = (uint32_t)uni(s_rec[H_SR]);
    h.fast = uni(s_rec[H_FAST]);
    h.numel = uni(s_rec[H_NUMEL]);
    h.IR = uni(s_rec[H_IR]);
    h.pad = uni(s_rec[H_PAD]);
    return h;
}

// Vector path: the compact index of the 4 elements from (o, rem = e - o I R), or -1.
__device__ __forceinline__ int vec_index(const int32_t *lev, int o, int rem) {
    const int IlR = uni(lev[V_IR]);
    return (o < uni(lev[V_O]) && rem < IlR) ? uni(lev[V_OFF]) + o * IlR + rem : -1;
}

// Element path: the compact index of element (o, i, r), or -1.
__device__ __forceinline__ int elem_index(const int32_t *lev, const Head &h, int o, int i, int r) {
    int jo = o - uni(lev[V_SHO]), ji = i - uni(lev[V_SHI]);
    jo += jo < 0 ? h.O : 0;
    ji += ji < 0 ? h.I : 0;
    const int Il = uni(lev[V_I]);
    return (jo < uni(lev[V_O]) && ji < Il) ? uni(lev[V_OFF]) + (jo * Il + ji) * h.R + r : -1;
}

__global__ __launch_bounds__(kBlock) void k_fedavg(const int32_t *__restrict__ plan,
                                                   const int4 *__restrict__ clients, int K,
                                                   const float *__restrict__ ragged,
                                                   const uint32_t *prev, uint32_t *out) {
    __shared__ int4 s_cli[DLS_HETERO_MAX_K];  // {level, weight bits, row start lo, hi}
    __shared__ int32_t s_rec[kRec];
    __shared__ int32_t s_idx[kL * kTile];
    const int tid = threadIdx.x;
    for (int k = tid; k < K; k += kBlock) s_cli[k] = clients[k];
    const int T = plan[1], L = plan[2], tiles = plan[3];
    const int32_t *tile_end = plan + kHdr, *recs = tile_end + T;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int t = find_tensor(tile_end, T, tile);
        const int first = t ? tile_end[t - 1] : 0;
        __syncthreads();  // the tile before is done with s_rec (the first time: s_cli is staged)
        if (tid < kHead + L * kLev) s_rec[tid] = recs[(int64_t)t * kRec + tid];
        __syncthreads();
        const Head h = load_head(s_rec);
        const int e0 = (tile - first) * kTile, e = e0 + 4 * tid;
        if (e >= h.pad) continue;  // past the tensor's padded end (no barrier below)
        // levels whose window meets the tile's o-range [o0, o1]
        const int o0 = mdiv(e0, h.mIR, h.sIR);
        const int o1 = mdiv(min(e0 + kTile, h.numel) - 1, h.mIR, h.sIR);
        uint32_t mask = 0;
        for (int l = 0; l < L; ++l) {
            const int32_t *lev = s_rec + kHead + l * kLev;
            int a = o0 - uni(lev[V_SHO]);
            a += a < 0 ? h.O : 0;  // o0's place in the window's own order
            if (a < uni(lev[V_O]) || o0 + (h.O - a) <= o1) mask |= 1u << l;
        }
        float acc[4] = {-0.f, -0.f, -0.f, -0.f}, den[4] = {0.f, 0.f, 0.f, 0.f};
        if (h.fast) {
            int32_t *my = s_idx + tid;  // [level][lane]
            const int o = mdiv(e, h.mIR, h.sIR), rem = e - o * h.IR;
            for (int l = 0; l < L; ++l)
                my[l * kBlock] = e < h.numel ? vec_index(s_rec + kHead + l * kLev, o, rem) : -1;
            auto fetch = [&](int k, int &ix, float &w, f32x4 &q) {
                const int4 c = s_cli[k];
                const int lvl = uni(c.x);
                w = __int_as_float(uni(c.y));
                ix = -1;
                q = f32x4{0.f, 0.f, 0.f, 0.f};
                if (!((mask >> lvl) & 1u)) return;  // wave-uniform
                ix = my[lvl * kBlock];
                const float *row = ragged + (((int64_t)uni(c.w) << 32) | (uint32_t)uni(c.z));
                if (ix >= 0) q = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(row + ix));
            };
            auto eat = [&](int ix, float w, f32x4 q) {
                if (ix < 0) return;
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = acc[j] + w * q[j];
                den[0] = den[0] + w;
            };
            int k = 0;
            for (; k + kRowUnroll <= K; k += kRowUnroll) {
                int ix[kRowUnroll];
                float w[kRowUnroll];
                f32x4 q[kRowUnroll];
#pragma unroll
                for (int u = 0; u < kRowUnroll; ++u) fetch(k + u, ix[u], w[u], q[u]);
#pragma unroll
                for (int u = 0; u < kRowUnroll; ++u) eat(ix[u], w[u], q[u]);
            }
            for (; k < K; ++k) {
                int ix;
                float w;
                f32x4 q;
                fetch(k, ix, w, q);
                eat(ix, w, q);
            }
            den[1] = den[2] = den[3] = den[0];
        } else {
            int4 *my = reinterpret_cast<int4 *>(s_idx) + tid;  // [level][lane] x 4 elements
            int4 mine[kL];
#pragma unroll
            for (int l = 0; l < kL; ++l) mine[l] = int4{-1, -1, -1, -1};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (e + j >= h.numel) continue;
                const int o = mdiv(e + j, h.mIR, h.sIR), rem = e + j - o * h.IR;
                const int i = mdiv(rem, h.mR, h.sR), r = rem - i * h.R;
#pragma unroll
                for (int l = 0; l < kL; ++l)
                    if (l < L) (&mine[l].x)[j] = elem_index(s_rec + kHead + l * kLev, h, o, i, r);
            }
#pragma unroll
            for (int l = 0; l < kL; ++l)
                if (l < L) my[l * kBlock] = mine[l];
            auto fetch = [&](int k, int4 &ix, float &w, float *q) {
                const int4 c = s_cli[k];
                const int lvl = uni(c.x);
                w = __int_as_float(uni(c.y));
                ix = int4{-1, -1, -1, -1};
                q[0] = q[1] = q[2] = q[3] = 0.f;
                if (!((mask >> lvl) & 1u)) return;  // wave-uniform
                ix = my[lvl * kBlock];
                const float *row = ragged + (((int64_t)uni(c.w) << 32) | (uint32_t)uni(c.z));
                if (ix.x >= 0) q[0] = row[ix.x];
                if (ix.y >= 0) q[1] = row[ix.y];
                if (ix.z >= 0) q[2] = row[ix.z];
                if (ix.w >= 0) q[3] = row[ix.w];
            };
            auto eat = [&](const int4 &ix, float w, const float *q) {
                const int held[4] = {ix.x, ix.y, ix.z, ix.w};
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (held[j] >= 0) {
                        acc[j] = acc[j] + w * q[j];
                        den[j] = den[j] + w;
                    }
            };
            int k = 0;
            for (; k + 2 <= K; k += 2) {
                int4 ix[2];
                float w[2], q[2][4];
#pragma unroll
                for (int u = 0; u < 2; ++u) fetch(k + u, ix[u], w[u], q[u]);
#pragma unroll
                for (int u = 0; u < 2; ++u) eat(ix[u], w[u], q[u]);
            }
            if (k < K) {
                int4 ix;
                float w, q[4];
                fetch(k, ix, w, q);
                eat(ix, w, q);
            }
        }
        const int64_t at = (int64_t)h.goff + e;
        const u32x4 pv = *reinterpret_cast<const u32x4 *>(prev + at);
        u32x4 ov;
#pragma unroll
        for (int j = 0; j < 4; ++j)  // nobody holds it: prev's bits; the padding: zero
            ov[j] = e + j >= h.numel ? 0u : den[j] > 0.f ? __float_as_uint(acc[j] / den[j]) : pv[j];
        *reinterpret_cast<u32x4 *>(out + at) = ov;
    }
}

__global__ __launch_bounds__(kBlock) void k_extract(const int32_t *__restrict__ plan,
                                                    const uint32_t *__restrict__ global,
                                                    uint32_t *__restrict__ dst) {
    __shared__ int32_t s_rec[kRec];
    const int tid = threadIdx.x;
    const int T = plan[1], L = plan[2], tiles = plan[3];
    const int32_t *tile_end = plan + kHdr, *recs = tile_end + T;
    int64_t row[kL];  // level l's row in dst: the levels' rows follow each other
    {
        int64_t at = 0;
#pragma unroll
        for (int l = 0; l < kL; ++l) {
            row[l] = at;
            at += plan[8 + l];
        }
    }
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int t = find_tensor(tile_end, T, tile);
        const int first = t ? tile_end[t - 1] : 0;
        __syncthreads();
        if (tid < kHead + L * kLev) s_rec[tid] = recs[(int64_t)t * kRec + tid];
        __syncthreads();
        const Head h = load_head(s_rec);
        const int e = (tile - first) * kTile + 4 * tid;
        if (tile == first && tid < 64) {  // the levels' padding, fewer than 64 elements each
#pragma unroll
            for (int l = 0; l < kL; ++l) {
                if (l >= L) continue;
                const int32_t *lev = s_rec + kHead + l * kLev;
                const int len = uni(lev[V_LEN]);
                if (len + tid < ((len + 63) & ~63)) dst[row[l] + uni(lev[V_OFF]) + len + tid] = 0u;
            }
        }
        if (e >= h.numel) continue;
        const u32x4 v = *reinterpret_cast<const u32x4 *>(global + (int64_t)h.goff + e);
        if (h.fast) {
            const int o = mdiv(e, h.mIR, h.sIR), rem = e - o * h.IR;
#pragma unroll
            for (int l = 0; l < kL; ++l) {
                if (l >= L) continue;
                const int ix = vec_index(s_rec + kHead + l * kLev, o, rem);
                if (ix >= 0) *reinterpret_cast<u32x4 *>(dst + row[l] + ix) = v;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (e + j >= h.numel) continue;
                const int o = mdiv(e + j, h.mIR, h.sIR), rem = e + j - o * h.IR;
                const int i = mdiv(rem, h.mR, h.sR), r = rem - i * h.R;
#pragma unroll
                for (int l = 0; l < kL; ++l) {
                    if (l >= L) continue;
                    const int ix = elem_index(s_rec + kHead + l * kLev, h, o, i, r);
                    if (ix >= 0) dst[row[l] + ix] = v[j];
                }
            }
        }
    }
}

struct PlanInfo {
    int32_t T, L, tiles;
    int64_t P, Pl[kL], rows;  // rows: the levels' rows together
};

inline int64_t pad64(int64_t n) { return (n + 63) / 64 * 64; }

// Every word of a host plan is what include/dls_hip.h says it is: the kernels index with them.
int check_plan(const char *fn, const int32_t *plan, int64_t words, PlanInfo *info) {
    DLS_REQUIRE(plan, DLS_EINVAL, "%s: null pointer (plan)", fn);
    DLS_REQUIRE(words >= kHdr && plan[0] == DLS_HETERO_MAGIC, DLS_EINVAL,
                "%s: not a plan (%lld words, first word 0x%x)", fn, (long long)words,
                words >= 1 ? (unsigned)plan[0] : 0u);
    const int32_t T = plan[1], L = plan[2];
    DLS_REQUIRE(L >= 1 && L <= kL, DLS_EINVAL, "%s: L=%d levels (1..DLS_HETERO_MAX_LEVELS=%d)", fn, L, kL);
    DLS_REQUIRE(T >= 1 && T <= DLS_HETERO_MAX_TENSORS, DLS_EINVAL,
                "%s: T=%d tensors (1..DLS_HETERO_MAX_TENSORS=%d)", fn, T, DLS_HETERO_MAX_TENSORS);
    DLS_REQUIRE(words == kHdr + (int64_t)T * (1 + kRec), DLS_EINVAL,
                "%s: a plan of T=%d tensors has %lld words, not %lld", fn, T,
                (long long)(kHdr + (int64_t)T * (1 + kRec)), (long long)words);
    const int32_t *tile_end = plan + kHdr, *recs = tile_end + T;
    int64_t goff = 0, loff[kL] = {0}, tiles = 0;
    for (int32_t t = 0; t < T; ++t) {
        const int32_t *h = recs + (int64_t)t * kRec;
        const int64_t O = h[H_O], I = h[H_I], R = h[H_R], numel = O * I * R;
        DLS_REQUIRE(O >= 1 && I >= 1 && R >= 1 && O <= (1 << 30) && I <= (1 << 30) && R <= (1 << 30) &&
                        I * R <= (1 << 30) && numel <= (1 << 30),
                    DLS_EINVAL, "%s: tensor %d is [%lld, %lld, %lld] (1..2^30 elements)", fn, t,
                    (long long)O, (long long)I, (long long)R);
        uint32_t mIR, sIR, mR, sR;
        make_magic((uint32_t)(I * R), &mIR, &sIR);
        make_magic((uint32_t)R, &mR, &sR);
        bool fast = (I * R) % 4 == 0;
        for (int l = 0; l < L; ++l) {
            const int32_t *v = h + kHead + l * kLev;
            const int64_t Ol = v[V_O], Il = v[V_I], len = Ol * Il * R;
            DLS_REQUIRE(Ol >= 1 && Ol <= O && Il >= 1 && Il <= I && v[V_SHO] >= 0 && v[V_SHO] < O &&
                            v[V_SHI] >= 0 && v[V_SHI] < I,
                        DLS_EINVAL, "%s: tensor %d level %d holds [%lld, %lld] at shifts (%d, %d) of [%lld, %lld]",
                        fn, t, l, (long long)Ol, (long long)Il, v[V_SHO], v[V_SHI], (long long)O, (long long)I);
            DLS_REQUIRE(v[V_OFF] == loff[l] && v[V_IR] == Il * R && v[V_LEN] == len && v[V_RES] == 0,
                        DLS_EINVAL, "%s: tensor %d level %d: offset, row length or size do not follow", fn, t, l);
            loff[l] += pad64(len);
            DLS_REQUIRE(loff[l] < ((int64_t)1 << 31), DLS_EINVAL, "%s: level %d is longer than 2^31 - 1", fn, l);
            fast = fast && v[V_SHO] == 0 && v[V_SHI] == 0 && (Il * R) % 4 == 0;
        }
        DLS_REQUIRE(h[H_GOFF] == goff && (uint32_t)h[H_MIR] == mIR && (uint32_t)h[H_SIR] == sIR &&
                        (uint32_t)h[H_MR] == mR && (uint32_t)h[H_SR] == sR && h[H_FAST] == (fast ? 1 : 0) &&
                        h[H_NUMEL] == numel && h[H_IR] == I * R && h[H_PAD] == pad64(numel),
                    DLS_EINVAL, "%s: tensor %d: offset, division constants, path or sizes do not follow", fn, t);
        goff += pad64(numel);
        tiles += (pad64(numel) + kTile - 1) / kTile;
        DLS_REQUIRE(goff < ((int64_t)1 << 31) && tile_end[t] == tiles, DLS_EINVAL,
                    "%s: tensor %d: the row is longer than 2^31 - 1 or the tile prefix does not follow", fn, t);
    }
    DLS_REQUIRE(plan[3] == tiles && plan[4] == goff && plan[5] == 0 && plan[6] == 0 && plan[7] == 0,
                DLS_EINVAL, "%s: the header's tiles=%d and P=%d do not follow (%lld, %lld)", fn, plan[3],
                plan[4], (long long)tiles, (long long)goff);
    info->T = T;
    info->L = L;
    info->tiles = (int32_t)tiles;
    info->P = goff;
    info->rows = 0;
    for (int l = 0; l < kL; ++l) {
        DLS_REQUIRE(plan[8 + l] == (l < L ? loff[l] : 0), DLS_EINVAL, "%s: the header's length of level %d", fn, l);
        info->Pl[l] = plan[8 + l];
        info->rows += plan[8 + l];
    }
    return DLS_OK;
}

// [a, a + n) and [b, b + m) floats share a byte
inline bool overlap(const void *a, int64_t n, const void *b, int64_t m) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + (uintptr_t)m * 4 && b0 < a0 + (uintptr_t)n * 4;
}

template <typename Kernel>
unsigned tile_grid(Kernel kern, int32_t tiles) {
    const int64_t resident = resident_blocks(reinterpret_cast<const void *>(kern), kBlock, 0);
    return (unsigned)std::max<int64_t>(1, std::min<int64_t>(tiles, resident));
}

}  // namespace
}  // namespace dls

using namespace dls;

extern "C" int dls_hetero_fedavg_f32(const int32_t *plan, const int32_t *plan_dev, int64_t plan_words,
                                     const int32_t *clients, const int32_t *clients_dev, int32_t K,
                                     const float *ragged, int64_t ragged_len, const float *prev,
                                     float *out, dls_stream_t stream) {
    const char *fn = "dls_hetero_fedavg_f32";
    PlanInfo info;
    const int rc = check_plan(fn, plan, plan_words, &info);
    if (rc != DLS_OK) return rc;
    DLS_REQUIRE(plan_dev && clients && clients_dev && ragged && prev && out, DLS_EINVAL, "%s: null pointer", fn);
    DLS_REQUIRE(K >= 1 && K <= DLS_HETERO_MAX_K, DLS_EINVAL, "%s: K=%d (1..DLS_HETERO_MAX_K=%d)", fn, K,
                DLS_HETERO_MAX_K);
    DLS_REQUIRE(ragged_len >= 0, DLS_EINVAL, "%s: ragged_len=%lld", fn, (long long)ragged_len);
    for (int32_t k = 0; k < K; ++k) {
        const int32_t *c = clients + 4 * (int64_t)k;
        DLS_REQUIRE(c[0] >= 0 && c[0] < info.L, DLS_EINVAL, "%s: client %d has level %d of %d", fn, k, c[0], info.L);
        float w;
        memcpy(&w, c + 1, sizeof w);
        DLS_REQUIRE(std::isfinite(w) && w > 0.f, DLS_EINVAL, "%s: client %d has weight %g (finite and > 0)", fn, k, w);
        const int64_t start = ((int64_t)c[3] << 32) | (uint32_t)c[2];
        DLS_REQUIRE(start >= 0 && start % 4 == 0 && start <= ragged_len && info.Pl[c[0]] <= ragged_len - start,
                    DLS_EINVAL, "%s: client %d's row [%lld, %lld + %lld) of level %d leaves the %lld elements "
                    "of ragged or starts off a 16-byte boundary", fn, k, (long long)start, (long long)start,
                    (long long)info.Pl[c[0]], c[0], (long long)ragged_len);
    }
    DLS_REQUIRE(aligned16(ragged) && aligned16(prev) && aligned16(out) && aligned16(plan_dev) && aligned16(clients_dev),
                DLS_ELAYOUT, "%s: 16-byte alignment (plan_dev, clients_dev, ragged, prev, out)", fn);
    DLS_REQUIRE((out == prev || !overlap(out, info.P, prev, info.P)) && !overlap(out, info.P, ragged, ragged_len) &&
                    !overlap(out, info.P, plan_dev, plan_words) && !overlap(out, info.P, clients_dev, 4 * (int64_t)K),
                DLS_EINVAL, "%s: out may be prev itself and overlaps nothing else", fn);
    hipLaunchKernelGGL(k_fedavg, dim3(tile_grid(k_fedavg, info.tiles)), dim3(kBlock), 0, as_stream(stream), plan_dev,
                       reinterpret_cast<const int4 *>(clients_dev), (int)K, ragged,
                       reinterpret_cast<const uint32_t *>(prev), reinterpret_cast<uint32_t *>(out));
    return check_launch(fn);
}

extern "C" int dls_hetero_extract_f32(const int32_t *plan, const int32_t *plan_dev, int64_t plan_words,
                                      const float *global, float *rows, int64_t rows_len,
                                      dls_stream_t stream) {
    const char *fn = "dls_hetero_extract_f32";
    PlanInfo info;
    const int rc = check_plan(fn, plan, plan_words, &info);
    if (rc != DLS_OK) return rc;
    DLS_REQUIRE(plan_dev && global && rows, DLS_EINVAL, "%s: null pointer", fn);
    DLS_REQUIRE(rows_len >= info.rows, DLS_EINVAL, "%s: rows holds %lld elements, the levels need %lld", fn,
                (long long)rows_len, (long long)info.rows);
    DLS_REQUIRE(aligned16(global) && aligned16(rows) && aligned16(plan_dev), DLS_ELAYOUT,
                "%s: 16-byte alignment (plan_dev, global, rows)", fn);
    DLS_REQUIRE(!overlap(rows, info.rows, global, info.P) && !overlap(rows, info.rows, plan_dev, plan_words),
                DLS_EINVAL, "%s: rows overlaps an input", fn);
    hipLaunchKernelGGL(k_extract, dim3(tile_grid(k_extract, info.tiles)), dim3(kBlock), 0, as_stream(stream), plan_dev,
                       reinterpret_cast<const uint32_t *>(global), reinterpret_cast<uint32_t *>(rows));
    return check_launch(fn);
}
