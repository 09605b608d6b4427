// Pairwise squared distances between K client rows for gfx950: the hot path of the
// distance-based robust rules (multi-Krum, FedServer aggregation_rule="multi_krum")
// and of client similarity / clustering.
//
//   D[a][b] = sum_p (U[rows[a]][p] - U[rows[b]][p])^2      (include/dls_hip.h)
// formed term by term from the difference: d = fl32(x - y), acc = fmaf(d, d, acc) in
// fp32 chains of at most 120 terms, everything above the chains in fp64 in a fixed
// order.  No Gram-matrix form (|x|^2 + |y|^2 - 2 x.y cancels catastrophically for
// honest clients, which differ in the 3rd or 4th digit).
//
// Lanes run across PAIRS, not across coordinates.  The KP = 8 G padded rows form a
// G x G grid of 8 x 8 row blocks; a lane owns one block (i, j) - 64 pairs, 64 fp32
// chain accumulators and their 64 fp64 sums in registers - and one of SL = 64 / G^2
// coordinate slots, so a wave holds the whole KP x KP matrix SL times.  A wave is
// its own workgroup: it streams tiles of TW = 2048 / KP coordinates of all KP rows
// (eight 16-byte loads per lane, 128 contiguous bytes per row and instruction),
// transposes them through LDS to [coordinate][row], and per step every lane reads
// its 8 + 8 row values of one coordinate as four 16-byte LDS loads (lanes of a grid
// row / column read the same address: a broadcast) and issues 32 packed subtractions
// and 32 packed fmas.  A pair's chain is a function of the coordinate alone: the same
// for every pair and position, so permuting `rows` permutes D bit for bit, and
// (x - y)^2 == (y - x)^2 makes D symmetric.  The next tile's loads are in flight
// while a tile is computed.  No cross-lane reduction, no atomics: a wave stores its
// fp64 sums once (32 KiB), and k_pairdist_finish adds the waves' and slots' partials
// in ascending order.
//
// Work split (a function of P and K alone, not of the device): a period is FLT
// tiles (one flush: <= 120 steps); period n belongs to wave n % nW, nW =
// ceil(periods / ceil(periods / kMaxWaves)).
#include "rows_common.h"

namespace dls {
namespace {

constexpr int kMaxWaves = DLS_PAIRDIST_MAX_WAVES;  // 256 CUs x 8 resident waves
constexpr int kPartDoubles = 4096; // per wave: 64 pairs x 64 lanes
constexpr int kFinishPhases = 16;

template <int G_>
struct PairCfg {
    static constexpr int G = G_;
    static constexpr int KP = 8 * G;           // padded rows
    static constexpr int SL = 64 / (G * G);    // coordinate slots per wave
    static constexpr int NL = 8;               // 16-byte loads per lane and tile
    static constexpr int TW = 256 * NL / KP;   // coordinates per tile: 32, 64, 128, 256
    static constexpr int STEPS = TW / SL;      // chain terms per tile: 32, 16, 8, 4
    static constexpr int S = KP + 4;           // LDS floats per coordinate (16-byte multiple)
    static constexpr int FLT = 120 / STEPS;    // tiles per flush: 3, 7, 15, 30
    static constexpr int64_t PERIOD = (int64_t)FLT * TW;
    static_assert(FLT * STEPS <= 120, "fp32 chains of at most 120 terms");
    static_assert(G * G * SL == 64 && TW % SL == 0 && (TW / 4) % 8 == 0, "lane maps");
};

struct PairPlan {
    int64_t periods;
    int ppw;  // periods per wave
    int nW;   // waves
};

template <typename C>
PairPlan make_plan(int64_t P) {
    PairPlan p;
    p.periods = P > 0 ? (P + C::PERIOD - 1) / C::PERIOD : 1;
    p.ppw = (int)((p.periods + kMaxWaves - 1) / kMaxWaves);
    p.nW = (int)((p.periods + p.ppw - 1) / p.ppw);
    return p;
}

inline int grid_of(int K) { return K <= 8 ? 1 : K <= 16 ? 2 : K <= 32 ? 4 : 8; }

inline PairPlan plan_for(int K, int64_t P) {
    switch (grid_of(K)) {
        case 1: return make_plan<PairCfg<1>>(P);
        case 2: return make_plan<PairCfg<2>>(P);
        case 4: return make_plan<PairCfg<4>>(P);
        default: return make_plan<PairCfg<8>>(P);
    }
}

// One tile's loads: load m covers rows 8 (m % G) + lane % 8, quad 8 (m / G) + lane / 8.
// A quad at or past P reads the row's last quad instead; store_tile makes it 0.
template <typename C>
__device__ __forceinline__ void load_tile(f32x4 (&buf)[C::NL], const float *__restrict__ U,
                                          int64_t ldu, const int (&rid)[C::G], int64_t tbase,
                                          int64_t P, int lq) {
#pragma unroll
    for (int m = 0; m < C::NL; ++m) {
        const int64_t c = tbase + 4 * (8 * (m / C::G) + lq);
        const int64_t cc = c < P ? c : P - 4;
        buf[m] = __builtin_nontemporal_load(
            reinterpret_cast<const f32x4 *>(U + (int64_t)rid[m % C::G] * ldu + cc));
    }
}

// The loaded tile into LDS as [coordinate][row]; coordinates at or past P become 0
// (d = 0 adds nothing to a chain).  The values are first touched here, so the loads
// stay in flight through the previous tile's steps.
template <typename C>
__device__ __forceinline__ void store_tile(float *tile, const f32x4 (&buf)[C::NL], int64_t tbase,
                                           int64_t P, int lr, int lq) {
#pragma unroll
    for (int m = 0; m < C::NL; ++m) {
        const int row = 8 * (m % C::G) + lr;
        const int c0 = 4 * (8 * (m / C::G) + lq);
        const bool in = tbase + c0 < P;
#pragma unroll
        for (int k = 0; k < 4; ++k) tile[(c0 + k) * C::S + row] = in ? buf[m][k] : 0.f;
    }
}

struct PairOperands {
    f32x4 x0, x1, y0, y1;
};

__device__ __forceinline__ PairOperands read_step(const float *px, const float *py, int off) {
    PairOperands o;
    o.x0 = *reinterpret_cast<const f32x4 *>(px + off);
    o.x1 = *reinterpret_cast<const f32x4 *>(px + off + 4);
    o.y0 = *reinterpret_cast<const f32x4 *>(py + off);
    o.y1 = *reinterpret_cast<const f32x4 *>(py + off + 4);
    return o;
}

template <int G>
__global__ __launch_bounds__(64) void k_pairdist(const float *__restrict__ U, int64_t ldu,
                                                 const int32_t *__restrict__ rows, int K,
                                                 int64_t P, int64_t periods, int ppw, int nW,
                                                 double *__restrict__ part) {
    using C = PairCfg<G>;
    __shared__ __attribute__((aligned(16))) float tile[C::TW * C::S];
    const int lane = threadIdx.x;
    const int w = blockIdx.x;
    const int lr = lane & 7, lq = lane >> 3;  // load map: row within a group of 8, quad
    const int ij = lane / C::SL, s = lane % C::SL;
    const int bi = ij / G, bj = ij % G;       // the lane's 8 x 8 block of pairs
    int rid[G];
#pragma unroll
    for (int g = 0; g < G; ++g) rid[g] = rows[min(8 * g + lr, K - 1)];  // pad: the last row

    f32x2 acc[8][4];
    double sum[8][8];
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int b = 0; b < 8; ++b) sum[a][b] = 0.0;

    const float *px = tile + s * C::S + 8 * bi;
    const float *py = tile + s * C::S + 8 * bj;
    f32x4 buf[C::NL];

    // tile n of this wave: tile n % FLT of its period n / FLT (period it * nW + w);
    // -1 past the wave's share or past P (then every later tile is, too)
    auto tile_base = [&](int n) -> int64_t {
        const int it = n / C::FLT;
        const int64_t pidx = (int64_t)it * nW + w;
        if (it >= ppw || pidx >= periods) return -1;
        const int64_t tb = pidx * C::PERIOD + (int64_t)(n % C::FLT) * C::TW;
        return tb < P ? tb : -1;
    };
    int64_t tbase = tile_base(0);
    if (tbase >= 0) load_tile<C>(buf, U, ldu, rid, tbase, P, lq);
    for (int n = 0; tbase >= 0; ++n) {
        if (n % C::FLT == 0) {
#pragma unroll
            for (int a = 0; a < 8; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[a][b] = (f32x2){0.f, 0.f};
        }
        {
            __syncthreads();  // the previous tile's reads are done
            store_tile<C>(tile, buf, tbase, P, lr, lq);
            __syncthreads();
            const int64_t nbase = tile_base(n + 1);  // in flight during the steps below
            if (nbase >= 0) load_tile<C>(buf, U, ldu, rid, nbase, P, lq);
            tbase = nbase;
            PairOperands cur = read_step(px, py, 0);
#pragma unroll 2
            for (int t = 0; t < C::STEPS; ++t) {
                // the next step's operands are read while this step computes (the
                // last step re-reads itself)
                const PairOperands nxt =
                    read_step(px, py, (t + 1 < C::STEPS ? t + 1 : t) * C::SL * C::S);
                const float x[8] = {cur.x0[0], cur.x0[1], cur.x0[2], cur.x0[3],
                                    cur.x1[0], cur.x1[1], cur.x1[2], cur.x1[3]};
                const f32x2 y[4] = {{cur.y0[0], cur.y0[1]}, {cur.y0[2], cur.y0[3]},
                                    {cur.y1[0], cur.y1[1]}, {cur.y1[2], cur.y1[3]}};
#pragma unroll
                for (int a = 0; a < 8; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b) {
                        const f32x2 d = (f32x2){x[a], x[a]} - y[b];  // fl32(x - y)
                        acc[a][b] = __builtin_elementwise_fma(d, d, acc[a][b]);
                    }
                cur = nxt;
            }
        }
        // flush at the end of a period (<= 120 terms per chain) and of the wave's
        // share: every chain joins its fp64 sum
        if (n % C::FLT == C::FLT - 1 || tbase < 0) {
#pragma unroll
            for (int a = 0; a < 8; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    sum[a][2 * b] += (double)acc[a][b][0];
                    sum[a][2 * b + 1] += (double)acc[a][b][1];
                }
        }
    }
    // canonical pairs only (block above the diagonal, or on it with ka < kb)
    double *out = part + (int64_t)w * kPartDoubles + lane;
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int b = 0; b < 8; ++b)
            if (bi < bj || (bi == bj && a < b)) out[(a * 8 + b) * 64] = sum[a][b];
}

// Block p = ka * 8 + kb adds, per lane, the waves' partials: thread (phase, lane)
// takes waves phase, phase + 16, ... ascending; then the 16 phases ascending; then
// the lane's SL slots ascending.  The order is a function of nW and G alone.
template <int G>
__global__ __launch_bounds__(64 * kFinishPhases) void k_pairdist_finish(
    const double *__restrict__ part, int nW, int K, double *__restrict__ D) {
    using C = PairCfg<G>;
    __shared__ double sm[kFinishPhases][64];
    __shared__ double sl[64];
    const int p = blockIdx.x, ka = p >> 3, kb = p & 7;
    const int lane = threadIdx.x & 63, ph = threadIdx.x >> 6;
    {
        const int ij = lane / C::SL, bi = ij / G, bj = ij % G;
        const bool canon = (bi < bj || (bi == bj && ka < kb)) && 8 * bj + kb < K;
        double t = 0.0;
        if (canon)
            for (int w = ph; w < nW; w += kFinishPhases)
                t += part[((int64_t)w * 64 + p) * 64 + lane];
        sm[ph][lane] = t;
    }
    __syncthreads();
    if (ph == 0) {
        double t = 0.0;
#pragma unroll
        for (int q = 0; q < kFinishPhases; ++q) t += sm[q][lane];
        sl[lane] = t;
    }
    __syncthreads();
    if (threadIdx.x < G * G) {
        const int ij = threadIdx.x, bi = ij / G, bj = ij % G;
        const int a = 8 * bi + ka, b = 8 * bj + kb;
        if (b < K && a < K) {
            if (a == b) {
                D[(int64_t)a * K + a] = 0.0;
            } else if (bi < bj || (bi == bj && ka < kb)) {
                double t = 0.0;
                for (int q = 0; q < C::SL; ++q) t += sl[ij * C::SL + q];
                D[(int64_t)a * K + b] = t;
                D[(int64_t)b * K + a] = t;
            }
        }
    }
}

template <int G>
void launch(const float *U, int64_t ldu, const int32_t *rows, int K, int64_t P, double *D,
            double *part, hipStream_t st) {
    const PairPlan pl = make_plan<PairCfg<G>>(P);
    hipLaunchKernelGGL((k_pairdist<G>), dim3((unsigned)pl.nW), dim3(64), 0, st, U, ldu, rows, K,
                       P, pl.periods, pl.ppw, pl.nW, part);
    hipLaunchKernelGGL((k_pairdist_finish<G>), dim3(64), dim3(64 * kFinishPhases), 0, st,
                       (const double *)part, pl.nW, K, D);
}

}  // namespace
}  // namespace dls

using namespace dls;

extern "C" int64_t dls_pairwise_sqdist_workspace(int32_t K, int64_t P) {
    return workspace_query("dls_pairwise_sqdist_workspace", K, P,
                           [&] { return plan_for(K, P).nW; }, kPartDoubles);
}

extern "C" int dls_pairwise_sqdist_f32(const float *U, int64_t ldu, const int32_t *rows, int32_t K,
                                       int64_t P, double *D, void *workspace,
                                       dls_stream_t stream) {
    const char *fn = "dls_pairwise_sqdist_f32";
    int rc = check_head(fn, U && rows && D && workspace, "K", K);
    if (rc == DLS_OK)
        rc = check_layout(fn, ldu, P, aligned16(U) && aligned16(workspace) && aligned_to(D, 8),
                          " (U, workspace), 8-byte (D)");
    if (rc != DLS_OK) return rc;
    hipStream_t st = as_stream(stream);
    if (P == 0) return zero_f64(fn, D, (size_t)K * K, st);
    double *part = static_cast<double *>(workspace);
    switch (grid_of(K)) {
        case 1: launch<1>(U, ldu, rows, K, P, D, part, st); break;
        case 2: launch<2>(U, ldu, rows, K, P, D, part, st); break;
        case 4: launch<4>(U, ldu, rows, K, P, D, part, st); break;
        default: launch<8>(U, ldu, rows, K, P, D, part, st); break;
    }
    return check_launch(fn);
}
