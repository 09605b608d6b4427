// Gram matrix (inner products) of K client rows for gfx950, read-only and fused with
// the in-place fold of the rows into a per-client history: the hot path of the
// direction-based robust rules (FoolsGold, FedServer aggregation_rule="foolsgold") and
// the base of cosine similarity, trust scores and spectral filtering.
//
//   h_k[p] = base ? fl32(U[rows[k]][p] - base[p]) : U[rows[k]][p]
//   dls_rows_gram_f32:     G[a][b] ~ sum_p h_a[p] * h_b[p]
//   dls_history_gram_f32:  H'[hrows[k]][p] = fl32(H[hrows[k]][p] + h_k[p]), stored in
//                          place, and G is the Gram matrix of the rows of H'
// (include/dls_hip.h).  The arithmetic is pairdist.hip's with the subtraction removed:
// acc = fmaf(h_a, h_b, acc) in fp32 chains of at most 120 terms, everything above the
// chains in fp64 in a fixed order.  The terms are signed, so the error bound is
// relative to sum_p |h_a h_b|, not to the result.
//
// The structure is k_pairdist's.  Lanes run across PAIRS: the KP = 8 G padded rows
// form a G x G grid of 8 x 8 row blocks; a lane owns one block (i, j) - 64 fp32 chain
// accumulators and their 64 fp64 sums in registers - and one of SL = 64 / G^2
// coordinate slots.  A wave is its own workgroup: it streams tiles of TW = 2048 / KP
// coordinates of all KP rows (eight 16-byte loads per lane and operand), transposes
// them through LDS to [coordinate][row], and per step every lane reads its 8 + 8 row
// values of one coordinate as four 16-byte LDS loads and issues 32 packed fmas.  A
// pair's chain is a function of the coordinate alone, and a * b == b * a, so G is
// symmetric in bits, permuting `rows` permutes G bit for bit, and rows of equal
// contents give G[a][b] == G[a][a] == G[b][b]: the same chain of the same operands.
// The next tile's loads are in flight while a tile is computed.  No cross-lane
// reduction, no atomics: a wave stores its fp64 sums once, and k_gram_finish adds the
// waves' and slots' partials in ascending order.
//
// What differs from k_pairdist, because of the in-place fold:
//   * a (row, quad) of a tile belongs to exactly one lane of exactly one wave (the load
//     map is a bijection, the tiles partition 0..P), and only that lane reads and
//     writes H there: H is read once and written once with no ordering between lanes;
//   * rows K..KP-1 are padding.  k_pairdist re-reads the last row for them; here a
//     padding lane loads nothing, stores nothing and contributes zeros (its pairs are
//     never output), so the last client is not folded twice;
//   * a quad at or past P is not redirected to the row's last quad: it is neither
//     loaded nor stored and contributes zeros.
//
// Work split (a function of P and K alone, not of the device): a period is FLT tiles
// (one flush: <= 120 steps); period n belongs to wave n % nW, nW = ceil(periods /
// ceil(periods / kMaxWaves)): pairdist.hip's plan with half its waves.  The kernels
// take 256 VGPRs, so one wave per SIMD is resident: 1024 waves fill the device in one
// round, and every wave costs 32 KiB of partials written and read back.
#include "rows_common.h"

namespace dls {
namespace {

constexpr int kMaxWaves = 1024;    // 256 CUs x 4 SIMDs, one resident wave each
constexpr int kPartDoubles = 4096; // per wave: 64 pairs x 64 lanes
constexpr int kFinishPhases = 16;

template <int G_>
struct GramCfg {
    static constexpr int G = G_;
    static constexpr int KP = 8 * G;           // padded rows
    static constexpr int SL = 64 / (G * G);    // coordinate slots per wave
    static constexpr int NL = 8;               // 16-byte loads per lane, operand and tile
    static constexpr int TW = 256 * NL / KP;   // coordinates per tile: 32, 64, 128, 256
    static constexpr int STEPS = TW / SL;      // chain terms per tile: 32, 16, 8, 4
    static constexpr int S = KP + 4;           // LDS floats per coordinate (16-byte multiple)
    static constexpr int FLT = 120 / STEPS;    // tiles per flush: 3, 7, 15, 30
    static constexpr int64_t PERIOD = (int64_t)FLT * TW;
    static_assert(FLT * STEPS <= 120, "fp32 chains of at most 120 terms");
    static_assert(G * G * SL == 64 && TW % SL == 0 && (TW / 4) % 8 == 0, "lane maps");
};

struct GramPlan {
    int64_t periods;
    int ppw;  // periods per wave
    int nW;   // waves
};

template <typename C>
GramPlan make_plan(int64_t P) {
    GramPlan p;
    p.periods = P > 0 ? (P + C::PERIOD - 1) / C::PERIOD : 1;
    p.ppw = (int)((p.periods + kMaxWaves - 1) / kMaxWaves);
    p.nW = (int)((p.periods + p.ppw - 1) / p.ppw);
    return p;
}

inline int grid_of(int K) { return K <= 8 ? 1 : K <= 16 ? 2 : K <= 32 ? 4 : 8; }

inline GramPlan plan_for(int K, int64_t P) {
    switch (grid_of(K)) {
        case 1: return make_plan<GramCfg<1>>(P);
        case 2: return make_plan<GramCfg<2>>(P);
        case 4: return make_plan<GramCfg<4>>(P);
        default: return make_plan<GramCfg<8>>(P);
    }
}

// One tile's operands as loaded: the row of U, of base and (the fold) of H.
template <typename C>
struct GramTile {
    f32x4 u[C::NL], b[C::NL], h[C::NL];
};

// One tile's loads: load m covers row 8 (m % G) + lane % 8, quad 8 (m / G) + lane / 8.
// A padding row (real[] false) and a quad at or past P load nothing.
template <typename C, bool FOLD>
__device__ __forceinline__ void load_tile(GramTile<C> &t, const float *__restrict__ U,
                                          const float *H, const float *__restrict__ base,
                                          const int64_t (&uoff)[C::G], const int64_t (&hoff)[C::G],
                                          const bool (&real)[C::G], int64_t tbase, int64_t P,
                                          int lq) {
#pragma unroll
    for (int m = 0; m < C::NL; ++m) {
        const int g = m % C::G;
        const int64_t c = tbase + 4 * (8 * (m / C::G) + lq);
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        t.u[m] = t.b[m] = t.h[m] = zero;
        if (real[g] && c < P) {
            t.u[m] = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(U + uoff[g] + c));
            if (base) t.b[m] = *reinterpret_cast<const f32x4 *>(base + c);
            if (FOLD) t.h[m] = *reinterpret_cast<const f32x4 *>(H + hoff[g] + c);
        }
    }
}

// The loaded tile into LDS as [coordinate][row], the fold's H' stored on the way:
// d = fl32(u - base), h' = fl32(h + d), each rounded once (-ffp-contract=off, and a
// subtraction followed by an addition has no fused form).  The lane that loaded a
// quad is the only one that stores it; padding rows and quads at or past P store
// nothing and put zeros into LDS (a zero adds nothing to a chain).  The values are
// first touched here, so the loads stay in flight through the previous tile's steps.
template <typename C, bool FOLD>
__device__ __forceinline__ void store_tile(float *tile, const GramTile<C> &t, float *H,
                                           const float *__restrict__ base,
                                           const int64_t (&hoff)[C::G], const bool (&real)[C::G],
                                           int64_t tbase, int64_t P, int lr, int lq) {
#pragma unroll
    for (int m = 0; m < C::NL; ++m) {
        const int g = m % C::G;
        const int row = 8 * g + lr;
        const int c0 = 4 * (8 * (m / C::G) + lq);
        const bool in = real[g] && tbase + c0 < P;
        f32x4 v = t.u[m];
        if (base) v = v - t.b[m];
        if (FOLD) {
            v = t.h[m] + v;
            if (in) *reinterpret_cast<f32x4 *>(H + hoff[g] + tbase + c0) = v;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) tile[(c0 + k) * C::S + row] = in ? v[k] : 0.f;
    }
}

struct GramOperands {
    f32x4 x0, x1, y0, y1;
};

__device__ __forceinline__ GramOperands read_step(const float *px, const float *py, int off) {
    GramOperands o;
    o.x0 = *reinterpret_cast<const f32x4 *>(px + off);
    o.x1 = *reinterpret_cast<const f32x4 *>(px + off + 4);
    o.y0 = *reinterpret_cast<const f32x4 *>(py + off);
    o.y1 = *reinterpret_cast<const f32x4 *>(py + off + 4);
    return o;
}

template <int G, bool FOLD>
__global__ __launch_bounds__(64) void k_gram(const float *__restrict__ U, int64_t ldu,
                                             const int32_t *__restrict__ rows, float *H,
                                             int64_t ldh, const int32_t *__restrict__ hrows, int K,
                                             int64_t P, const float *__restrict__ base,
                                             int64_t periods, int ppw, int nW,
                                             double *__restrict__ part) {
    using C = GramCfg<G>;
    __shared__ __attribute__((aligned(16))) float tile[C::TW * C::S];
    const int lane = threadIdx.x;
    const int w = blockIdx.x;
    const int lr = lane & 7, lq = lane >> 3;  // load map: row within a group of 8, quad
    const int ij = lane / C::SL, s = lane % C::SL;
    const int bi = ij / G, bj = ij % G;       // the lane's 8 x 8 block of pairs
    int64_t uoff[G], hoff[G];
    bool real[G];
#pragma unroll
    for (int g = 0; g < G; ++g) {
        real[g] = 8 * g + lr < K;  // rows K .. KP-1 are padding: never loaded or stored
        const int k = min(8 * g + lr, K - 1);
        uoff[g] = (int64_t)rows[k] * ldu;
        hoff[g] = FOLD ? (int64_t)hrows[k] * ldh : 0;
    }

    f32x2 acc[8][4];
    double sum[8][8];
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int b = 0; b < 8; ++b) sum[a][b] = 0.0;

    const float *px = tile + s * C::S + 8 * bi;
    const float *py = tile + s * C::S + 8 * bj;
    GramTile<C> buf;

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
    if (tbase >= 0) load_tile<C, FOLD>(buf, U, H, base, uoff, hoff, real, tbase, P, lq);
    for (int n = 0; tbase >= 0; ++n) {
        if (n % C::FLT == 0) {
#pragma unroll
            for (int a = 0; a < 8; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) acc[a][b] = (f32x2){0.f, 0.f};
        }
        {
            __syncthreads();  // the previous tile's reads are done
            store_tile<C, FOLD>(tile, buf, H, base, hoff, real, tbase, P, lr, lq);
            __syncthreads();
            const int64_t nbase = tile_base(n + 1);  // in flight during the steps below
            if (nbase >= 0) load_tile<C, FOLD>(buf, U, H, base, uoff, hoff, real, nbase, P, lq);
            tbase = nbase;
            GramOperands cur = read_step(px, py, 0);
#pragma unroll 2
            for (int t = 0; t < C::STEPS; ++t) {
                // the next step's operands are read while this step computes (the
                // last step re-reads itself)
                const GramOperands nxt =
                    read_step(px, py, (t + 1 < C::STEPS ? t + 1 : t) * C::SL * C::S);
                const float x[8] = {cur.x0[0], cur.x0[1], cur.x0[2], cur.x0[3],
                                    cur.x1[0], cur.x1[1], cur.x1[2], cur.x1[3]};
                const f32x2 y[4] = {{cur.y0[0], cur.y0[1]}, {cur.y0[2], cur.y0[3]},
                                    {cur.y1[0], cur.y1[1]}, {cur.y1[2], cur.y1[3]}};
#pragma unroll
                for (int a = 0; a < 8; ++a)
#pragma unroll
                    for (int b = 0; b < 4; ++b)
                        acc[a][b] =
                            __builtin_elementwise_fma((f32x2){x[a], x[a]}, y[b], acc[a][b]);
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
    // canonical pairs only (block above the diagonal, or on it with ka <= kb)
    double *out = part + (int64_t)w * kPartDoubles + lane;
#pragma unroll
    for (int a = 0; a < 8; ++a)
#pragma unroll
        for (int b = 0; b < 8; ++b)
            if (bi < bj || (bi == bj && a <= b)) out[(a * 8 + b) * 64] = sum[a][b];
}

// Block p = ka * 8 + kb adds, per lane, the waves' partials: thread (phase, lane)
// takes waves phase, phase + 16, ... ascending; then the 16 phases ascending; then
// the lane's SL slots ascending.  The order is a function of nW and G alone.
template <int G>
__global__ __launch_bounds__(64 * kFinishPhases) void k_gram_finish(
    const double *__restrict__ part, int nW, int K, double *__restrict__ Gm) {
    using C = GramCfg<G>;
    __shared__ double sm[kFinishPhases][64];
    __shared__ double sl[64];
    const int p = blockIdx.x, ka = p >> 3, kb = p & 7;
    const int lane = threadIdx.x & 63, ph = threadIdx.x >> 6;
    {
        const int ij = lane / C::SL, bi = ij / G, bj = ij % G;
        const bool canon = (bi < bj || (bi == bj && ka <= kb)) && 8 * bj + kb < K;
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
        if (b < K && a < K && (bi < bj || (bi == bj && ka <= kb))) {
            double t = 0.0;
            for (int q = 0; q < C::SL; ++q) t += sl[ij * C::SL + q];
            Gm[(int64_t)a * K + b] = t;
            Gm[(int64_t)b * K + a] = t;
        }
    }
}

template <int G>
void launch(const float *U, int64_t ldu, const int32_t *rows, float *H, int64_t ldh,
            const int32_t *hrows, int K, int64_t P, const float *base, double *Gm, double *part,
            hipStream_t st) {
    const GramPlan pl = make_plan<GramCfg<G>>(P);
    if (H)
        hipLaunchKernelGGL((k_gram<G, true>), dim3((unsigned)pl.nW), dim3(64), 0, st, U, ldu, rows,
                           H, ldh, hrows, K, P, base, pl.periods, pl.ppw, pl.nW, part);
    else
        hipLaunchKernelGGL((k_gram<G, false>), dim3((unsigned)pl.nW), dim3(64), 0, st, U, ldu,
                           rows, H, ldh, hrows, K, P, base, pl.periods, pl.ppw, pl.nW, part);
    hipLaunchKernelGGL((k_gram_finish<G>), dim3(64), dim3(64 * kFinishPhases), 0, st,
                       (const double *)part, pl.nW, K, Gm);
}

// The checks both entry points share (rows_common.h; nonnull: the entry point's own
// pointers; H == nullptr: the read-only call), then the launches.
int run_gram(const char *fn, bool nonnull, const float *U, int64_t ldu, const int32_t *rows,
             float *H, int64_t ldh, const int32_t *hrows, int32_t K, int64_t P, const float *base,
             double *Gm, void *workspace, dls_stream_t stream) {
    int rc = check_head(fn, nonnull, "K", K);
    if (rc == DLS_OK)
        rc = check_layout(fn, ldu, P,
                          aligned16(U) && aligned16(H) && aligned16(base) &&
                              aligned16(workspace) && aligned_to(Gm, 8),
                          " (U, H, base, workspace), 8-byte (G)", &ldh);
    if (rc != DLS_OK) return rc;
    hipStream_t st = as_stream(stream);
    if (P == 0) return zero_f64(fn, Gm, (size_t)K * K, st);
    double *part = static_cast<double *>(workspace);
    switch (grid_of(K)) {
        case 1: launch<1>(U, ldu, rows, H, ldh, hrows, K, P, base, Gm, part, st); break;
        case 2: launch<2>(U, ldu, rows, H, ldh, hrows, K, P, base, Gm, part, st); break;
        case 4: launch<4>(U, ldu, rows, H, ldh, hrows, K, P, base, Gm, part, st); break;
        default: launch<8>(U, ldu, rows, H, ldh, hrows, K, P, base, Gm, part, st); break;
    }
    return check_launch(fn);
}

}  // namespace
}  // namespace dls

using namespace dls;

extern "C" int64_t dls_rows_gram_workspace(int32_t K, int64_t P) {
    return workspace_query("dls_rows_gram_workspace", K, P, [&] { return plan_for(K, P).nW; },
                           kPartDoubles);
}

extern "C" int dls_rows_gram_f32(const float *U, int64_t ldu, const int32_t *rows, int32_t K,
                                 int64_t P, const float *base, double *G, void *workspace,
                                 dls_stream_t stream) {
    return run_gram("dls_rows_gram_f32", U && rows && G && workspace, U, ldu, rows, nullptr, ldu,
                    nullptr, K, P, base, G, workspace, stream);
}

extern "C" int dls_history_gram_f32(const float *U, int64_t ldu, const int32_t *rows, float *H,
                                    int64_t ldh, const int32_t *hrows, int32_t K, int64_t P,
                                    const float *base, double *G, void *workspace,
                                    dls_stream_t stream) {
    return run_gram("dls_history_gram_f32", U && rows && H && hrows && G && workspace, U, ldu,
                    rows, H, ldh, hrows, K, P, base, G, workspace, stream);
}
