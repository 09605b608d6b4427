// Low-rank update compression for gfx950 (Vogels, Karimireddy & Jaggi 2019, "PowerSGD"): one
// power-iteration step per weight matrix with error feedback on the client, and the server's
// FedAvg over the clients' factors.  include/dls_hip.h has the contract.
//
// Every matrix product goes through v_mfma_f32_16x16x4_f32 with the rank padded to the 16-wide
// side, so a lane supplies one operand element per instruction and no reduction crosses lanes.
// Operand layout of the instruction (wave of 64, lane l): A[i][k] sits in lane 16 k + i,
// B[k][j] in lane 16 k + j, D[i][j] in register i % 4 of lane 16 (i / 4) + j.
//
// The unit of work is a WAVE item, found by a binary search of the plan's prefix counts; a
// workgroup is four consecutive items, so LeNet-5's 6 x 25 and 16 x 150 share a workgroup
// with their neighbours instead of costing one each.  Grids are capped and stride over the
// items; an item's arithmetic never depends on which wave runs it.
//
// dls_powersgd_compress_f32, three launches:
//   k_psgd_form   item = (tensor, 16 rows, kChunk columns): u = fl(fl(w - base) + e) -> e, and
//                 the chunk's partial of P = U Q0 into the workspace (A = U, B = Q0; a lane
//                 loads 16 bytes of a row and feeds them to four instructions).  Dense tensors:
//                 item = 1024 elements, w -> payload, +0.0 -> e.  Each item leaves its count
//                 of non-finite u in the workspace.
//   k_psgd_gs     one workgroup per compressed tensor: P = the chunk partials added in chunk
//                 order in fp64, modified Gram-Schmidt in fp64 on [n][16] in the workspace,
//                 P^ rounded once to fp32 into the payload.  Thread i owns the rows i, i +
//                 256, ..; a sum runs over a thread's rows ascending, the wave's xor butterfly
//                 (32, 16, .., 1) and the four waves in order.  One more workgroup adds the
//                 non-finite counts in item order into stats[0].
//   k_psgd_resid  item = (tensor, 16 columns): sweep 1, Q = U^T P^ over all n rows (A = U^T,
//                 B = P^), stored to the payload and, through 1 KB of LDS per wave, turned
//                 into the A operand of sweep 2, R^T = Q P^^T, whose D registers are four
//                 consecutive columns of a row: e = fl(u - R) with 16-byte accesses where m
//                 is a multiple of 4.  The strip is read from HBM in sweep 1 and from the L2
//                 in sweep 2.
//
// dls_powersgd_fedavg_f32, one launch: item = (tensor, 32 rows, 64 columns): eight D tiles,
// A = Q_i, B = fl(c_i P^_i), the K r contraction flattened (client, then q) and walked four
// slots per instruction; c_i sits in LDS per tile of kTileK clients, the accumulators stay in
// registers from tile to tile.  Dense tensors: item = 1024 elements, the exact FedAvg chain.
#include <algorithm>

#include "rows_common.h"

namespace dls {
namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kChunk = DLS_POWERSGD_CHUNK;      // columns of one pass-A item
constexpr int kTileK = DLS_POWERSGD_CLIENT_TILE;
constexpr int kDense = 1024;                    // elements of one dense item
constexpr int kPW = DLS_POWERSGD_PLAN_WORDS;
constexpr int64_t kMaxP = (int64_t)1 << 31;
enum { kOff = 0, kN, kM, kKind, kPoff, kQoff, kWs, kFirstA, kFirstB, kFirstS };

__device__ __forceinline__ int uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ int64_t uniform64(int64_t v) {
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)((uint64_t)v >> 32));
    return (int64_t)(((uint64_t)hi << 32) | lo);
}

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

inline __host__ __device__ int64_t ru64(int64_t x) { return (x + 63) & ~(int64_t)63; }
inline __host__ __device__ int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
inline __host__ __device__ bool compressed_shape(int64_t n, int64_t m, int64_t r) {
    return r <= (n < m ? n : m) && (n + m) * r < n * m;
}

// One tensor of the plan, every field checked against what the kernel may touch: P (the
// row), L (a payload), W (the workspace's bytes; negative: the kernel has no workspace).
// ok == false: the tensor is skipped.
struct Seg {
    int64_t off, ext, n, m, poff, qoff, ws;
    int kind;
    bool ok;
};

__device__ __forceinline__ Seg load_seg(const int64_t *plan, int t, int r, int64_t P, int64_t L,
                                        int64_t W) {
    const int64_t *p = plan + (int64_t)t * kPW;
    Seg s;
    s.off = p[kOff];
    s.ext = p[kPW + kOff] - s.off;
    s.n = p[kN];
    s.m = p[kM];
    s.kind = (int)p[kKind];
    s.poff = p[kPoff];
    s.qoff = p[kQoff];
    s.ws = p[kWs];
    bool ok = s.off >= 0 && (s.off & 63) == 0 && s.ext >= 64 && (s.ext & 63) == 0 &&
              s.ext <= P - s.off && s.off <= P && s.n >= 1 && s.m >= 1 && s.n < kMaxP &&
              s.m < kMaxP && s.n * s.m <= s.ext && s.poff >= 0 && (s.poff & 63) == 0;
    if (ok && s.kind == 1) {
        ok = s.qoff >= 0 && (s.qoff & 63) == 0 && s.poff + s.n * r <= L && s.qoff + s.m * r <= L &&
             (W < 0 || (s.ws >= 0 && (s.ws & 15) == 0 &&
                        s.ws + s.n * 128 + cdiv(s.m, kChunk) * s.n * 64 <= W));
    } else if (ok) {
        ok = s.kind == 0 && s.poff + ru64(s.n * s.m) <= L;
    }
    s.ok = ok;
    return s;
}

// the last t in [0, T) whose prefix count plan[t][col] is <= item
__device__ __forceinline__ int find_tensor(const int64_t *plan, int col, int T, int64_t item) {
    int lo = 0, hi = T - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (plan[(int64_t)mid * kPW + col] <= item) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}

// four consecutive floats from p[0..4), element k read only where k < valid; one 16-byte
// access where the caller knows the address to be 16-byte aligned
__device__ __forceinline__ f32x4 load4(const float *p, int valid, bool vec) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (vec && valid >= 4) return *reinterpret_cast<const f32x4 *>(p);
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k < valid) v[k] = p[k];
    return v;
}

__device__ __forceinline__ void store4(float *p, f32x4 v, int valid, bool vec) {
    if (vec && valid >= 4) {
        *reinterpret_cast<f32x4 *>(p) = v;
        return;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k < valid) p[k] = v[k];
}

__device__ __forceinline__ uint32_t nonfinite(float v) {
    return (__float_as_uint(v) & 0x7fffffffu) >= 0x7f800000u;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

__device__ __forceinline__ double wave_tree(double v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// ------------------------------------------------------------------ pass A: u and P = U Q0
__global__ __launch_bounds__(kBlock) void k_psgd_form(const float *w, const float *base, float *e,
                                                      int64_t P, const int64_t *plan, int T, int r,
                                                      const float *q0, float *payload, int64_t L,
                                                      char *ws, int64_t W, int64_t bad_slots) {
    const int wave = uniform(threadIdx.x >> 6), lane = lane_id();
    uint32_t *bad = reinterpret_cast<uint32_t *>(ws);
    const int64_t total = plan[(int64_t)T * kPW + kFirstA];
    const int64_t limit = total < bad_slots ? total : bad_slots;
    for (int64_t item = (int64_t)blockIdx.x * kWaves + wave; item < limit;
         item += (int64_t)gridDim.x * kWaves) {
        const int t = find_tensor(plan, kFirstA, T, item);
        const Seg s = load_seg(plan, t, r, P, L, W);
        const int64_t local = item - plan[(int64_t)t * kPW + kFirstA];
        uint32_t nbad = 0;
        if (s.ok && s.kind == 0 && local >= 0 && local < cdiv(s.ext, kDense)) {
            const int64_t count = s.n * s.m, sent = ru64(count);
#pragma unroll
            for (int it = 0; it < kDense / 256; ++it) {
                const int64_t j = local * kDense + it * 256 + 4 * lane;
                if (j >= s.ext) continue;
                const int valid = count - j > 4 ? 4 : (count - j < 0 ? 0 : (int)(count - j));
                const f32x4 vw = load4(w + s.off + j, valid, true);
                const f32x4 vb = load4(base + s.off + j, valid, true);
                f32x4 ve = {0.f, 0.f, 0.f, 0.f};
                if (e) ve = load4(e + s.off + j, valid, true);
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k < valid) nbad += nonfinite((vw[k] - vb[k]) + ve[k]);
                if (j < sent) *reinterpret_cast<f32x4 *>(payload + s.poff + j) = vw;
                if (e) *reinterpret_cast<f32x4 *>(e + s.off + j) = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        } else if (s.ok && s.kind == 1) {
            const int64_t nrb = cdiv(s.n, 16), nch = cdiv(s.m, kChunk);
            if (local >= 0 && local < nrb * nch) {
                const int64_t ch = local / nrb, rb = local - ch * nrb;  // row blocks run fastest
                const int64_t a = rb * 16 + (lane & 15);
                const int g = lane >> 4, q = lane & 15;
                const bool vec = (s.m & 3) == 0;
                const int64_t c_end = (ch + 1) * kChunk < s.m ? (ch + 1) * kChunk : s.m;
                const float *wr = w + s.off + a * s.m, *br = base + s.off + a * s.m;
                float *er = e ? e + s.off + a * s.m : nullptr;
                const float *qp = q0 + s.qoff;
                f32x4 acc = {0.f, 0.f, 0.f, 0.f};
                for (int64_t cc = ch * kChunk; cc < c_end; cc += 64) {
                    f32x4 u[4];
                    float bq[4][4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const int64_t col = cc + 16 * j + 4 * g;
                        int valid = 0;
                        if (a < s.n && col < c_end) valid = c_end - col > 4 ? 4 : (int)(c_end - col);
                        const f32x4 vw = load4(wr + col, valid, vec), vb = load4(br + col, valid, vec);
                        f32x4 ve = {0.f, 0.f, 0.f, 0.f};
                        if (er) ve = load4(er + col, valid, vec);
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            u[j][k] = k < valid ? (vw[k] - vb[k]) + ve[k] : 0.f;
                            nbad += k < valid ? nonfinite(u[j][k]) : 0u;
                            // the B operand's slot is this lane's g too: the same column
                            bq[j][k] = (q < r && col + k < c_end) ? qp[(col + k) * r + q] : 0.f;
                        }
                        if (er) store4(er + col, u[j], valid, vec);
                    }
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int k = 0; k < 4; ++k) acc = mfma4(u[j][k], bq[j][k], acc);
                }
                float *part = reinterpret_cast<float *>(ws + s.ws + s.n * 128) + ch * s.n * 16;
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int64_t row = rb * 16 + 4 * g + v;
                    if (row < s.n) part[row * 16 + q] = acc[v];
                }
                if (local == 0 && e)  // the tensor's padding slots
                    for (int64_t j = s.n * s.m + lane; j < s.ext; j += 64) e[s.off + j] = 0.f;
            }
        }
        nbad = wave_sum(nbad);
        if (lane == 0) bad[item] = nbad;
    }
}

// ------------------------------------------------------------------ Gram-Schmidt on P
// the 16 sums of the workgroup, every thread receiving them
__device__ __forceinline__ void block_sum16(double (&d)[16], double (*lds)[16]) {
    const int wave = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < 16; ++j) d[j] = wave_tree(d[j]);
    __syncthreads();
    if (lane_id() == 0) {
#pragma unroll
        for (int j = 0; j < 16; ++j) lds[wave][j] = d[j];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 16; ++j) d[j] = ((lds[0][j] + lds[1][j]) + lds[2][j]) + lds[3][j];
}

__global__ __launch_bounds__(kBlock) void k_psgd_gs(const int64_t *plan, int T, int r, int64_t P,
                                                    float *payload, int64_t L, char *ws, int64_t W,
                                                    int64_t bad_slots, int32_t *stats) {
    __shared__ double lds[kWaves][16];
    if ((int)blockIdx.x == T) {  // the non-finite counts, in item order
        const uint32_t *bad = reinterpret_cast<const uint32_t *>(ws);
        int64_t total = plan[(int64_t)T * kPW + kFirstA];
        total = total < bad_slots ? total : bad_slots;
        uint32_t sum = 0;
        for (int64_t i = threadIdx.x; i < total; i += kBlock) sum += bad[i];
        sum = wave_sum(sum);
        uint32_t *l32 = reinterpret_cast<uint32_t *>(&lds[0][0]);
        if (lane_id() == 0) l32[threadIdx.x >> 6] = sum;
        __syncthreads();
        if (threadIdx.x == 0) stats[0] = (int32_t)(l32[0] + l32[1] + l32[2] + l32[3]);
        return;
    }
    const Seg s = load_seg(plan, blockIdx.x, r, P, L, W);
    if (!s.ok || s.kind != 1) return;
    double *Pd = reinterpret_cast<double *>(ws + s.ws);
    const float *part = reinterpret_cast<const float *>(ws + s.ws + s.n * 128);
    const int64_t nch = cdiv(s.m, kChunk);
    float *ph = payload + s.poff;
    for (int64_t a = threadIdx.x; a < s.n; a += kBlock)
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            double sum = 0.0;
            for (int64_t ch = 0; ch < nch; ++ch) sum += (double)part[(ch * s.n + a) * 16 + q];
            Pd[a * 16 + q] = q < r ? sum : 0.0;
        }
    for (int64_t j = s.n * r + threadIdx.x; j < ru64(s.n * r); j += kBlock) ph[j] = 0.f;
    float *qh = payload + s.qoff;
    for (int64_t j = s.m * r + threadIdx.x; j < ru64(s.m * r); j += kBlock) qh[j] = 0.f;
    for (int q = 0; q < r; ++q) {
        double d[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) d[j] = 0.0;
        for (int64_t a = threadIdx.x; a < s.n; a += kBlock) {
            const double v = Pd[a * 16 + q];
            d[0] += v * v;
        }
        block_sum16(d, lds);
        const double norm2 = d[0];
        const bool zero = !(norm2 > 0.0 && norm2 < __builtin_inf());
        const double norm = zero ? 1.0 : __builtin_sqrt(norm2);
#pragma unroll
        for (int j = 0; j < 16; ++j) d[j] = 0.0;
        for (int64_t a = threadIdx.x; a < s.n; a += kBlock) {
            const double v = zero ? 0.0 : Pd[a * 16 + q] / norm;
            Pd[a * 16 + q] = v;
            ph[a * r + q] = (float)v;
            if (!zero) {
#pragma unroll
                for (int j = 0; j < 16; ++j) d[j] += v * Pd[a * 16 + j];
            }
        }
        if (q + 1 == r) break;
        block_sum16(d, lds);
        if (!zero) {
            for (int64_t a = threadIdx.x; a < s.n; a += kBlock) {
                const double v = Pd[a * 16 + q];
#pragma unroll
                for (int j = 0; j < 16; ++j)
                    if (j > q && j < r) Pd[a * 16 + j] -= d[j] * v;
            }
        }
    }
}

// ------------------------------------------------------------------ pass B: Q and the residual
__global__ __launch_bounds__(kBlock) void k_psgd_resid(const float *w, const float *base, float *e,
                                                       int64_t P, const int64_t *plan, int T, int r,
                                                       float *payload, int64_t L, int64_t W) {
    __shared__ float qt[kWaves][16][17];
    const int wave = uniform(threadIdx.x >> 6), lane = lane_id();
    const int g = lane >> 4, x = lane & 15;
    const int64_t total = plan[(int64_t)T * kPW + kFirstB];
    for (int64_t grp = blockIdx.x; grp * kWaves < total; grp += gridDim.x) {
        const int64_t item = grp * kWaves + wave;
        Seg s;
        s.ok = false;
        int64_t b0 = 0;
        if (item < total) {
            const int t = find_tensor(plan, kFirstB, T, item);
            s = load_seg(plan, t, r, P, L, W);
            const int64_t local = item - plan[(int64_t)t * kPW + kFirstB];
            s.ok = s.ok && s.kind == 1 && local >= 0 && local < cdiv(s.m, 16);
            b0 = local * 16;
        }
        const float *ph = payload + (s.ok ? s.poff : 0);
        const float *src = e ? e : w;  // pass A left u in e; without e it is formed again
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if (s.ok) {
            const int64_t col = b0 + x;
            for (int64_t a0 = 0; a0 < s.n; a0 += 16) {
                float uv[4], pv[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int64_t row = a0 + 4 * k + g;
                    const bool in = row < s.n && col < s.m;
                    const int64_t j = s.off + row * s.m + col;
                    uv[k] = in ? src[j] : 0.f;
                    if (!e && in) uv[k] = uv[k] - base[j];
                    pv[k] = (row < s.n && x < r) ? ph[row * r + x] : 0.f;
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) acc = mfma4(uv[k], pv[k], acc);
            }
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int64_t b = b0 + 4 * g + v;
                if (b < s.m && x < r) payload[s.qoff + b * r + x] = acc[v];
            }
        }
#pragma unroll
        for (int v = 0; v < 4; ++v) qt[wave][4 * g + v][x] = acc[v];
        __syncthreads();
        if (s.ok && e) {
            const bool vec = (s.m & 3) == 0;
            const int64_t col = b0 + 4 * g;
            const int valid = col < s.m ? (s.m - col > 4 ? 4 : (int)(s.m - col)) : 0;
            const int steps = (r + 3) >> 2;
            float qa[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) qa[k] = qt[wave][x][4 * k + g];
            for (int64_t a0 = 0; a0 < s.n; a0 += 16) {
                const int64_t row = a0 + x;
                float *ep = e + s.off + row * s.m + col;
                const int vrow = row < s.n ? valid : 0;
                const f32x4 u = load4(ep, vrow, vec);
                f32x4 rr = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (k < steps) {
                        const int q = 4 * k + g;
                        const float pb = (row < s.n && q < r) ? ph[row * r + q] : 0.f;
                        rr = mfma4(qa[k], pb, rr);
                    }
                }
                f32x4 out;
#pragma unroll
                for (int k = 0; k < 4; ++k) out[k] = u[k] - rr[k];
                store4(ep, out, vrow, vec);
            }
        }
    }
}

// ------------------------------------------------------------------ the server
__global__ __launch_bounds__(kBlock) void k_psgd_fedavg(const float *__restrict__ base,
                                                        const float *__restrict__ pay, int64_t ldp,
                                                        const int64_t *__restrict__ plan, int T,
                                                        int r, const float *__restrict__ weight,
                                                        float total_w, FastDiv d, int K, int64_t P,
                                                        int64_t L, float *__restrict__ out) {
    __shared__ float ctab[kTileK];
    const int wave = uniform(threadIdx.x >> 6), lane = lane_id();
    const int g = lane >> 4, x = lane & 15;
    const int64_t total = plan[(int64_t)T * kPW + kFirstS];
    for (int64_t grp = blockIdx.x; grp * kWaves < total; grp += gridDim.x) {
        const int64_t item = grp * kWaves + wave;
        Seg s;
        s.ok = false;
        int64_t local = 0, a0 = 0, b0 = 0;
        if (item < total) {
            const int t = find_tensor(plan, kFirstS, T, item);
            s = load_seg(plan, t, r, P, L, -1);
            local = item - plan[(int64_t)t * kPW + kFirstS];
            if (s.kind == 1) {
                const int64_t ncb = cdiv(s.m, 64);
                s.ok = s.ok && local >= 0 && local < cdiv(s.n, 32) * ncb;
                a0 = (local / ncb) * 32;
                b0 = (local % ncb) * 64;
            } else {
                s.ok = s.ok && local >= 0 && local < cdiv(s.ext, kDense);
            }
        }
        const bool lowrank = s.ok && s.kind == 1, dense = s.ok && s.kind == 0;
        f32x4 acc[4][2], dacc[kDense / 256];
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i][0] = acc[i][1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < kDense / 256; ++i) dacc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        const int64_t count = s.ok ? s.n * s.m : 0;
        for (int k0 = 0; k0 < K; k0 += kTileK) {
            const int nb = K - k0 < kTileK ? K - k0 : kTileK;
            __syncthreads();  // the previous tile's coefficients have been used
            if ((int)threadIdx.x < nb) ctab[threadIdx.x] = weight[k0 + threadIdx.x] / total_w;
            __syncthreads();
            if (lowrank) {
                const int slots = nb * r;  // kTileK * r is a multiple of 4: whole instructions
                for (int k4 = 0; k4 < slots; k4 += 4) {
                    const int kk = k4 + g;
                    const bool in = kk < slots;
                    const int i = in ? kk / r : 0, q = in ? kk - i * r : 0;
                    const float *row = pay + (int64_t)(k0 + i) * ldp;
                    const float c = ctab[i];
                    float qa[4], pb[2];
#pragma unroll
                    for (int mt = 0; mt < 4; ++mt) {
                        const int64_t b = b0 + 16 * mt + x;
                        qa[mt] = (in && b < s.m) ? row[s.qoff + b * r + q] : 0.f;
                    }
#pragma unroll
                    for (int nt = 0; nt < 2; ++nt) {
                        const int64_t a = a0 + 16 * nt + x;
                        pb[nt] = (in && a < s.n) ? c * row[s.poff + a * r + q] : 0.f;
                    }
#pragma unroll
                    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                        for (int nt = 0; nt < 2; ++nt)
                            acc[mt][nt] = mfma4(qa[mt], pb[nt], acc[mt][nt]);
                }
            } else if (dense) {
                for (int i = 0; i < nb; ++i) {
                    const float wi = weight[k0 + i];
                    const float *row = pay + (int64_t)(k0 + i) * ldp + s.poff;
#pragma unroll
                    for (int it = 0; it < kDense / 256; ++it) {
                        const int64_t j = local * kDense + it * 256 + 4 * lane;
                        if (j >= count) continue;
                        const f32x4 v = *reinterpret_cast<const f32x4 *>(row + j);
#pragma unroll
                        for (int k = 0; k < 4; ++k) {
                            const float term = div_exact(v[k] * wi, d);
                            dacc[it][k] = (k0 + i == 0) ? term : dacc[it][k] + term;
                        }
                    }
                }
            }
        }
        if (lowrank) {
            const bool vec = (s.m & 3) == 0;
#pragma unroll
            for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                for (int nt = 0; nt < 2; ++nt) {
                    const int64_t a = a0 + 16 * nt + x, b = b0 + 16 * mt + 4 * g;
                    const int valid = (a < s.n && b < s.m) ? (s.m - b > 4 ? 4 : (int)(s.m - b)) : 0;
                    const int64_t j = s.off + a * s.m + b;
                    const f32x4 bv = load4(base + j, valid, vec);
                    f32x4 o;
#pragma unroll
                    for (int k = 0; k < 4; ++k) o[k] = bv[k] + acc[mt][nt][k];
                    store4(out + j, o, valid, vec);
                }
            if (local == 0)  // the tensor's padding slots keep base's bits
                for (int64_t j = count + lane; j < s.ext; j += 64) out[s.off + j] = base[s.off + j];
        } else if (dense) {
#pragma unroll
            for (int it = 0; it < kDense / 256; ++it) {
                const int64_t j = local * kDense + it * 256 + 4 * lane;
                if (j >= s.ext) continue;
                f32x4 o = *reinterpret_cast<const f32x4 *>(base + s.off + j);
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (j + k < count) o[k] = dacc[it][k];
                *reinterpret_cast<f32x4 *>(out + s.off + j) = o;
            }
        }
    }
}

// [a, a + na) and [b, b + nb) bytes intersect
inline bool overlap(const void *a, int64_t na, const void *b, int64_t nb) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + (uintptr_t)nb && b0 < a0 + (uintptr_t)na;
}

inline int check_extent(const char *fn, int64_t P, int64_t T, int64_t r) {
    DLS_REQUIRE(P >= 64 && P < kMaxP, DLS_EINVAL, "%s: P=%lld (64 <= P < 2^31)", fn, (long long)P);
    DLS_REQUIRE(T >= 1 && T <= P / 64, DLS_EINVAL, "%s: T=%lld (1 <= T <= P / 64 = %lld)", fn,
                (long long)T, (long long)(P / 64));
    DLS_REQUIRE(r >= 1 && r <= DLS_POWERSGD_MAX_RANK, DLS_EINVAL, "%s: r=%lld (1..%d)", fn,
                (long long)r, DLS_POWERSGD_MAX_RANK);
    return DLS_OK;
}

// the (n, m) pairs of a size query: host memory
inline int check_dims(const char *fn, const int64_t *dims, int64_t T, int64_t r) {
    DLS_REQUIRE(dims, DLS_EINVAL, "%s: null pointer (dims)", fn);
    DLS_REQUIRE(T >= 1 && T < kMaxP / 64, DLS_EINVAL, "%s: T=%lld (1 <= T < 2^25)", fn, (long long)T);
    DLS_REQUIRE(r >= 1 && r <= DLS_POWERSGD_MAX_RANK, DLS_EINVAL, "%s: r=%lld (1..%d)", fn,
                (long long)r, DLS_POWERSGD_MAX_RANK);
    for (int64_t t = 0; t < T; ++t) {
        const int64_t n = dims[2 * t], m = dims[2 * t + 1];
        DLS_REQUIRE(n >= 1 && m >= 1 && n < kMaxP && m < kMaxP && n * m < kMaxP, DLS_EINVAL,
                    "%s: tensor %lld is %lld x %lld (n, m >= 1, n m < 2^31)", fn, (long long)t,
                    (long long)n, (long long)m);
    }
    return DLS_OK;
}

inline int64_t item_bound(int64_t P, int64_t T) { return P / 16 + T; }
inline int64_t bad_bytes(int64_t P, int64_t T) { return (4 * item_bound(P, T) + 15) & ~(int64_t)15; }

inline unsigned grid_for(int64_t P, int64_t T) {
    const int64_t want = (item_bound(P, T) + kWaves - 1) / kWaves;
    const int64_t cap = (int64_t)std::max(device_cus(), 1) * 8;
    return (unsigned)std::min(want, cap);
}

}  // namespace
}  // namespace dls

using namespace dls;

extern "C" int64_t dls_powersgd_payload_len(const int64_t *dims, int64_t T, int32_t r) {
    const int rc = check_dims("dls_powersgd_payload_len", dims, T, r);
    if (rc != DLS_OK) return rc;
    int64_t len = 0;
    for (int64_t t = 0; t < T; ++t) {
        const int64_t n = dims[2 * t], m = dims[2 * t + 1];
        len += compressed_shape(n, m, r) ? ru64(n * r) + ru64(m * r) : ru64(n * m);
    }
    return len;
}

extern "C" int64_t dls_powersgd_workspace(const int64_t *dims, int64_t T, int32_t r, int64_t P) {
    const char *fn = "dls_powersgd_workspace";
    int rc = check_dims(fn, dims, T, r);
    if (rc != DLS_OK) return rc;
    rc = check_extent(fn, P, T, r);
    if (rc != DLS_OK) return rc;
    DLS_REQUIRE(P % 64 == 0, DLS_ELAYOUT, "%s: P=%lld must be a multiple of 64", fn, (long long)P);
    int64_t bytes = bad_bytes(P, T);
    for (int64_t t = 0; t < T; ++t) {
        const int64_t n = dims[2 * t], m = dims[2 * t + 1];
        if (compressed_shape(n, m, r)) bytes += n * 128 + cdiv(m, kChunk) * n * 64;
    }
    return bytes;
}

extern "C" int dls_powersgd_compress_f32(const float *w, const float *base, float *e, int64_t P,
                                         const int64_t *plan, int32_t T, int32_t r, const float *q0,
                                         float *payload, int64_t L, int32_t *stats, void *workspace,
                                         int64_t workspace_bytes, dls_stream_t stream) {
    const char *fn = "dls_powersgd_compress_f32";
    DLS_REQUIRE(w && base && plan && q0 && payload && stats && workspace, DLS_EINVAL,
                "%s: null pointer (w, base, plan, q0, payload, stats, workspace)", fn);
    const int rc = check_extent(fn, P, T, r);
    if (rc != DLS_OK) return rc;
    DLS_REQUIRE(L >= 64 && L < kMaxP && workspace_bytes >= bad_bytes(P, T), DLS_EINVAL,
                "%s: L=%lld (64 <= L < 2^31), workspace_bytes=%lld (>= %lld)", fn, (long long)L,
                (long long)workspace_bytes, (long long)bad_bytes(P, T));
    DLS_REQUIRE(!e || (!overlap(e, 4 * P, w, 4 * P) && !overlap(e, 4 * P, base, 4 * P)), DLS_EINVAL,
                "%s: e must not alias w or base", fn);
    DLS_REQUIRE(!overlap(payload, 4 * L, q0, 4 * L), DLS_EINVAL, "%s: payload must not alias q0", fn);
    DLS_REQUIRE(P % 64 == 0 && L % 64 == 0, DLS_ELAYOUT,
                "%s: P=%lld and L=%lld must be multiples of 64", fn, (long long)P, (long long)L);
    DLS_REQUIRE(aligned16(w) && aligned16(base) && aligned16(e) && aligned16(plan) &&
                    aligned16(q0) && aligned16(payload) && aligned16(stats) && aligned16(workspace),
                DLS_ELAYOUT,
                "%s: 16-byte alignment of w, base, e, plan, q0, payload, stats and workspace", fn);
    hipStream_t st = as_stream(stream);
    char *ws = static_cast<char *>(workspace);
    const unsigned grid = grid_for(P, T);
    hipLaunchKernelGGL(k_psgd_form, dim3(grid), dim3(kBlock), 0, st, w, base, e, P, plan, (int)T,
                       (int)r, q0, payload, L, ws, workspace_bytes, item_bound(P, T));
    hipLaunchKernelGGL(k_psgd_gs, dim3((unsigned)T + 1), dim3(kBlock), 0, st, plan, (int)T, (int)r, P,
                       payload, L, ws, workspace_bytes, item_bound(P, T), stats);
    hipLaunchKernelGGL(k_psgd_resid, dim3(grid), dim3(kBlock), 0, st, w, base, e, P, plan, (int)T,
                       (int)r, payload, L, workspace_bytes);
    return check_launch(fn);
}

extern "C" int dls_powersgd_fedavg_f32(const float *base, const float *payloads, int64_t ldp,
                                       int64_t L, const int64_t *plan, int32_t T, int32_t r,
                                       const float *weight, float total, int32_t K, int64_t P,
                                       float *out, dls_stream_t stream) {
    const char *fn = "dls_powersgd_fedavg_f32";
    DLS_REQUIRE(base && payloads && plan && weight && out, DLS_EINVAL,
                "%s: null pointer (base, payloads, plan, weight, out)", fn);
    DLS_REQUIRE(K >= 1, DLS_EINVAL, "%s: K=%d (K >= 1)", fn, K);
    const int rc = check_extent(fn, P, T, r);
    if (rc != DLS_OK) return rc;
    DLS_REQUIRE(L >= 64 && L < kMaxP, DLS_EINVAL, "%s: L=%lld (64 <= L < 2^31)", fn, (long long)L);
    DLS_REQUIRE(total > 0.f && total < __builtin_inff(), DLS_EINVAL,
                "%s: total=%g must be positive and finite", fn, (double)total);
    DLS_REQUIRE(!overlap(out, 4 * P, base, 4 * P), DLS_EINVAL, "%s: out must not alias base", fn);
    DLS_REQUIRE(P % 64 == 0 && L % 64 == 0 && ldp >= L && ldp % 4 == 0, DLS_ELAYOUT,
                "%s: P=%lld and L=%lld must be multiples of 64, ldp=%lld a multiple of 4 and at "
                "least L", fn, (long long)P, (long long)L, (long long)ldp);
    DLS_REQUIRE(aligned16(base) && aligned16(payloads) && aligned16(plan) && aligned16(weight) &&
                    aligned16(out),
                DLS_ELAYOUT, "%s: 16-byte alignment of base, payloads, plan, weight and out", fn);
    hipLaunchKernelGGL(k_psgd_fedavg, dim3(grid_for(P, T)), dim3(kBlock), 0, as_stream(stream), base,
                       payloads, ldp, plan, (int)T, (int)r, weight, total, make_fastdiv(total),
                       (int)K, P, L, out);
    return check_launch(fn);
}
