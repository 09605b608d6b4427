// Fused Weiszfeld step, centered-clipping step and row-to-point squared distances for
// gfx950: the hot path of the geometric-median rule (RFA, Pillutla et al.; FedServer
// aggregation_rule="geometric_median"), of centered clipping (Karimireddy et al.;
// aggregation_rule="centered_clip") and of "how far is every client from the
// aggregate".
//
//   step:      z[p]     = sum_k fl32(w[k] * U[rows[k]][p])     (mul, then add, in row order)
//   clip step: z[p]     = fl32(z[p] + sum_k fl32(c[k] * fl32(U[rows[k]][p] - z[p])))
//   distances: dist2[k] ~ sum_p (U[rows[k]][p] - z[p])^2       (include/dls_hip.h)
// One kernel template with a mode: z read (dls_rows_sqdist_to_f32), z computed from
// the K values the lane already holds and written (dls_weiszfeld_step_f32), or z read,
// moved by the clipped differences to those K values and written back
// (dls_centered_clip_step_f32), so a step reads the rows from HBM once: FedAvg's
// traffic (the clip step adds one read of z).
//
// Lanes run across coordinates as in k_trimmed_mean: a lane owns VW consecutive
// coordinates of a tile of 64 VW (VW = 4, one 16-byte load per row, for K <= 32;
// VW = 2, 8-byte loads, for K > 32, so that the KP x VW values and the KP chains
// leave room for two waves per SIMD), the row indices and weights reach the wave
// through per-lane tables and v_readlane, every load is unconditional (a wire past K
// re-reads the last row; its results are dropped) and non-temporal.  Per row the
// lane keeps fp32 chains acc = fmaf(d, d, acc), d = fl32(x - z), across the tiles it
// visits: two terms per tile and chain.  After kFlushTiles tiles (8 terms; the
// contract allows 120) the chains are converted to fp64 and reduced across the 64
// lanes by a fixed transposing butterfly that leaves row r's sum on lane r (64 / KP
// lanes per row), where one fp64 register accumulates it.  No atomics: a wave stores
// its 64 sums once and k_weiszfeld_finish adds the waves in ascending order.
//
// Work split (a function of P and K alone, not of the device): tile n belongs to wave
// n % nW as its visit n / nW, nW = ceil(tiles / ceil(tiles / kMaxWaves)).
#include <type_traits>

#include "rows_common.h"

namespace dls {
namespace {

constexpr int kBlock = 256;         // 4 waves; no wave waits on another
constexpr int kMaxWaves = 2048;     // 256 CUs x 8 resident waves
constexpr int kFlushTiles = 4;      // tiles per flush: chains of 2 * 4 = 8 terms
constexpr int kPartDoubles = 64;    // per wave in the workspace: one sum per row
constexpr int kFinishPhases = 16;
static_assert(2 * kFlushTiles <= 120, "fp32 chains of at most 120 terms");

inline int vw_of(int K) { return K <= 32 ? 4 : 2; }

struct StepPlan {
    int64_t tiles;  // of 64 * VW coordinates
    int64_t tpw;    // tiles per wave
    int nW;         // waves
};

inline StepPlan make_plan(int K, int64_t P) {
    StepPlan p;
    const int64_t tc = 64 * vw_of(K);
    p.tiles = P > 0 ? (P + tc - 1) / tc : 1;
    p.tpw = (p.tiles + kMaxWaves - 1) / kMaxWaves;
    p.nW = (int)((p.tiles + p.tpw - 1) / p.tpw);
    return p;
}

// Sums v[r] over the 64 lanes, r = 0 .. N - 1 (N = 2^t): stage M = 32, 16, ... keeps
// the half of the rows the lane's bit M selects, hands the other half to lane ^ M and
// adds what it receives; once one row is left, the remaining lane bits are a plain
// butterfly (a + b on one side, b + a on the other: the same bits).  Lane l returns
// the sum of row l >> (6 - t); the order is fixed by N alone.
template <int N, int M>
__device__ __forceinline__ double reduce_rows(const double (&v)[N], int lane) {
    if constexpr (N == 1) {
        double t = v[0];
#pragma unroll
        for (int m = M; m >= 1; m >>= 1) t += __shfl_xor(t, m);
        return t;
    } else {
        const bool up = (lane & M) != 0;
        double h[N / 2];
#pragma unroll
        for (int i = 0; i < N / 2; ++i) {
            const double keep = up ? v[i + N / 2] : v[i];
            const double send = up ? v[i] : v[i + N / 2];
            h[i] = keep + __shfl_xor(send, M);
        }
        return reduce_rows<N / 2, M / 2>(h, lane);
    }
}

enum Mode { kRead, kStep, kClip };  // what happens to z before the distances

// KP wires (a power of two >= K), VW coordinates per lane; kRead: z is read; kStep: z
// is computed from the rows and written; kClip: z is read, stepped and written back.
template <int KP, int VW, Mode MODE>
__global__ __launch_bounds__(kBlock) void k_weiszfeld(const float *__restrict__ U, int64_t ldu,
                                                      const int32_t *__restrict__ rows, int K,
                                                      const float *__restrict__ w, int64_t P,
                                                      int64_t tiles, int64_t tpw, int nW,
                                                      float *z, double *__restrict__ part) {
    using vec = std::conditional_t<VW == 4, f32x4, f32x2>;
    static_assert(VW == 4 || VW == 2, "coordinates per lane");
    const int lane = __lane_id();
    const int wv = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (wv >= nW) return;  // the whole wave
    const int tr = rows[min(lane, K - 1)];
    int tw = 0;
    if constexpr (MODE != kRead) tw = __float_as_int(w[min(lane, K - 1)]);
    const int64_t PV = P / VW;
    vec *zv = reinterpret_cast<vec *>(z);

    f32x2 chain[KP];  // VW == 2 uses element 0 alone
    double mysum = 0.0;
    for (int64_t it = 0; it < tpw; ++it) {
        const int64_t t = it * nW + wv;
        if (t >= tiles) break;  // wave-uniform
        if (it % kFlushTiles == 0) {
#pragma unroll
            for (int j = 0; j < KP; ++j) chain[j] = (f32x2){0.f, 0.f};
        }
        const int64_t i0 = t * 64 + lane;
        const bool in = i0 < PV;
        const int64_t iq = in ? i0 : PV - 1;  // every lane stays: the tables need all 64
        vec x[KP];
#pragma unroll
        for (int j = 0; j < KP; ++j) {
            const int64_t r = __builtin_amdgcn_readlane(tr, j);
            x[j] = __builtin_nontemporal_load(reinterpret_cast<const vec *>(U + r * ldu) + iq);
        }
        vec zq;
        if constexpr (MODE == kStep) {
            // t_k = fl32(w_k * x_k); acc = t_0; acc = fl32(acc + t_k): -0 + t == t for
            // every t, so a wire past K adds -0
#pragma unroll
            for (int j = 0; j < KP; ++j) {
                const float wj = __int_as_float(__builtin_amdgcn_readlane(tw, j));
                vec tk = x[j] * wj;
                if (j == 0) {
                    zq = tk;
                } else {
                    if (j >= K) tk = (vec)(-0.f);  // wave-uniform
                    zq = zq + tk;
                }
            }
            if (in) zv[i0] = zq;
        } else if constexpr (MODE == kClip) {
            // The old z: an ordinary load (this lane stores z' to the same address and
            // nobody else reads it).  A lane past P re-reads index PV - 1, which its
            // owner in this wave may already have rewritten: whatever it gets is
            // harmless, because such a lane stores nothing and its d below is forced
            // to 0.
            const vec zo = zv[iq];
            // t_k = fl32(c_k * fl32(x_k - z)); acc = t_0; acc = fl32(acc + t_k);
            // z' = fl32(z + acc): no fma (-ffp-contract=off), a wire past K adds -0
            vec acc;
#pragma unroll
            for (int j = 0; j < KP; ++j) {
                const float cj = __int_as_float(__builtin_amdgcn_readlane(tw, j));
                vec tk = (x[j] - zo) * cj;
                if (j == 0) {
                    acc = tk;
                } else {
                    if (j >= K) tk = (vec)(-0.f);  // wave-uniform
                    acc = acc + tk;
                }
            }
            zq = zo + acc;
            if (in) zv[i0] = zq;
        } else {
            zq = reinterpret_cast<const vec *>(z)[iq];
        }
#pragma unroll
        for (int j = 0; j < KP; ++j) {
            vec d = x[j] - zq;  // fl32(x - z)
            if (!in) d = (vec)(0.f);  // a coordinate past P adds nothing
            if constexpr (VW == 4) {
                const f32x2 d0 = {d[0], d[1]}, d1 = {d[2], d[3]};
                chain[j] = __builtin_elementwise_fma(d0, d0, chain[j]);
                chain[j] = __builtin_elementwise_fma(d1, d1, chain[j]);
            } else {
                chain[j][0] = __builtin_fmaf(d[0], d[0], chain[j][0]);
                chain[j][0] = __builtin_fmaf(d[1], d[1], chain[j][0]);
            }
        }
        // flush at the end of a period and of the wave's share
        if (it % kFlushTiles == kFlushTiles - 1 || it + 1 == tpw || t + nW >= tiles) {
            double v[KP];
#pragma unroll
            for (int j = 0; j < KP; ++j) {
                if constexpr (VW == 4)
                    v[j] = (double)chain[j][0] + (double)chain[j][1];
                else
                    v[j] = (double)chain[j][0];
            }
            mysum += reduce_rows<KP, 32>(v, lane);
        }
    }
    constexpr int LPR = 64 / KP;  // lanes per row
    if (lane % LPR == 0) part[(int64_t)wv * kPartDoubles + lane / LPR] = mysum;
}

// Thread (phase, row) adds the waves phase, phase + 16, ... ascending, then the 16
// phases ascending: the order is a function of nW alone.
__global__ __launch_bounds__(64 * kFinishPhases) void k_weiszfeld_finish(
    const double *__restrict__ part, int nW, int K, double *__restrict__ dist2) {
    __shared__ double sm[kFinishPhases][64];
    const int row = threadIdx.x & 63, ph = threadIdx.x >> 6;
    double t = 0.0;
    if (row < K)
        for (int w = ph; w < nW; w += kFinishPhases) t += part[(int64_t)w * kPartDoubles + row];
    sm[ph][row] = t;
    __syncthreads();
    if (ph == 0 && row < K) {
        t = 0.0;
#pragma unroll
        for (int q = 0; q < kFinishPhases; ++q) t += sm[q][row];
        dist2[row] = t;
    }
}

template <int KP, int VW, Mode MODE>
void launch(const float *U, int64_t ldu, const int32_t *rows, int K, const float *w, int64_t P,
            float *z, double *dist2, double *part, hipStream_t st) {
    const StepPlan pl = make_plan(K, P);
    const unsigned blocks = (unsigned)((pl.nW + kBlock / 64 - 1) / (kBlock / 64));
    hipLaunchKernelGGL((k_weiszfeld<KP, VW, MODE>), dim3(blocks), dim3(kBlock), 0, st, U, ldu, rows,
                       K, w, P, pl.tiles, pl.tpw, pl.nW, z, part);
    hipLaunchKernelGGL(k_weiszfeld_finish, dim3(1), dim3(64 * kFinishPhases), 0, st,
                       (const double *)part, pl.nW, K, dist2);
}

template <Mode MODE>
void dispatch(const float *U, int64_t ldu, const int32_t *rows, int K, const float *w, int64_t P,
              float *z, double *dist2, double *part, hipStream_t st) {
    if (K <= 4)
        launch<4, 4, MODE>(U, ldu, rows, K, w, P, z, dist2, part, st);
    else if (K <= 8)
        launch<8, 4, MODE>(U, ldu, rows, K, w, P, z, dist2, part, st);
    else if (K <= 16)
        launch<16, 4, MODE>(U, ldu, rows, K, w, P, z, dist2, part, st);
    else if (K <= 32)
        launch<32, 4, MODE>(U, ldu, rows, K, w, P, z, dist2, part, st);
    else
        launch<64, 2, MODE>(U, ldu, rows, K, w, P, z, dist2, part, st);
}

// The checks the entry points share (rows_common.h; nonnull: the entry point's own
// pointers; w: the step's coefficients, null for the read-only call), then the launches.
template <Mode MODE>
int run_step(const char *fn, bool nonnull, const float *U, int64_t ldu, const int32_t *rows,
             int32_t K, const float *w, int64_t P, float *z, double *dist2, void *workspace,
             dls_stream_t stream) {
    int rc = check_head(fn, nonnull, "K", K);
    if (rc == DLS_OK)
        rc = check_layout(fn, ldu, P,
                          aligned16(U) && aligned16(z) && aligned16(workspace) &&
                              aligned_to(dist2, 8) && aligned_to(w, 4),
                          " (U, z, workspace), 8-byte (dist2)");
    if (rc != DLS_OK) return rc;
    hipStream_t st = as_stream(stream);
    if (P == 0) return zero_f64(fn, dist2, K, st);
    dispatch<MODE>(U, ldu, rows, K, w, P, z, dist2, static_cast<double *>(workspace), st);
    return check_launch(fn);
}

}  // namespace
}  // namespace dls

using namespace dls;

extern "C" int64_t dls_weiszfeld_workspace(int32_t K, int64_t P) {
    return workspace_query("dls_weiszfeld_workspace", K, P, [&] { return make_plan(K, P).nW; },
                           kPartDoubles);
}

extern "C" int dls_rows_sqdist_to_f32(const float *U, int64_t ldu, const int32_t *rows, int32_t K,
                                      int64_t P, const float *z, double *dist2, void *workspace,
                                      dls_stream_t stream) {
    return run_step<kRead>("dls_rows_sqdist_to_f32", U && rows && z && dist2 && workspace, U, ldu,
                           rows, K, nullptr, P, const_cast<float *>(z), dist2, workspace, stream);
}

extern "C" int dls_weiszfeld_step_f32(const float *U, int64_t ldu, const int32_t *rows, int32_t K,
                                      const float *w, int64_t P, float *z, double *dist2,
                                      void *workspace, dls_stream_t stream) {
    return run_step<kStep>("dls_weiszfeld_step_f32", U && rows && z && dist2 && workspace && w, U,
                           ldu, rows, K, w, P, z, dist2, workspace, stream);
}

extern "C" int dls_centered_clip_step_f32(const float *U, int64_t ldu, const int32_t *rows,
                                          int32_t K, const float *c, int64_t P, float *z,
                                          double *dist2, void *workspace, dls_stream_t stream) {
    return run_step<kClip>("dls_centered_clip_step_f32", U && rows && z && dist2 && workspace && c,
                           U, ldu, rows, K, c, P, z, dist2, workspace, stream);
}
