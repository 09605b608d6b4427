/*
 * dls_hip.h — C-ABI of libdls_hip.so, the MI355X (gfx950) implementation of the
 * server-side aggregation hot path of chen-zichen/distributed_learning_simulator.
 *
 * Every entry point replaces one reference hook (file:line in the reference
 * repository) and is called from the Python host layer
 * (distributed_learning_simulator_amd/_native.py, via ctypes).
 *
 * Contract:
 *   - plain pointers and sizes; every array argument is DEVICE memory owned by
 *     the caller (allocated by torch); nothing is retained after return;
 *   - `stream` is a hipStream_t passed as void*; every launch is asynchronous on
 *     it; no entry point synchronises, allocates or frees (graph-capturable);
 *   - return 0 on success, a negative DLS_E* code for a bad argument, or a
 *     positive hipError_t; dls_last_error() then describes it (thread-local);
 *   - all entry points are re-entrant; nothing throws across the ABI.
 *
 * Flattened parameter layout ("flat rows"): a client's parameter dict is one row
 * of a client-major matrix, tensors concatenated in dict (named_parameters)
 * order, each tensor starting at a multiple of 64 elements; `ld*` is the row
 * stride in elements.
 */
#ifndef DLS_HIP_H
#define DLS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DLS_ABI_VERSION 2

#define DLS_OK 0
#define DLS_EINVAL (-1)     /* bad size / null pointer / unsupported mode */
#define DLS_ELAYOUT (-2)    /* misaligned pointer or leading dimension */

/* FedAvg modes */
#define DLS_FEDAVG_EXACT 0  /* reference op order: acc (+)= fl(fl(x*n_i)/N) in client order; bit-exact */
#define DLS_FEDAVG_FMA 1    /* acc = fma(x, w_i, acc) with w_i = fl(n_i/N); normwise ~1e-7 */

/* Sign planes: parameters are grouped by 64; group g is two uint64 words,
 * word 2g = "positive" plane, word 2g+1 = "negative" plane, bit j of either
 * is parameter 64*g + j.  NaN sets both bits; parameters past P are 0.
 * A client row holds DLS_SIGN_WORDS(P) words (padded to whole 256-param
 * tiles, 8 words per tile). */
#define DLS_SIGN_TILE 256
#define DLS_SIGN_WORDS(P) ((((P) + 255) / 256) * 8)
/* Vote counts: #pos - #neg, plus DLS_SIGN_NAN_MARK if any counted client sent
 * NaN for that parameter; a count >= DLS_SIGN_NAN_MARK/2 decodes as "poisoned"
 * (vote 0), which survives an int32 sum over up to 127 ranks. */
#define DLS_SIGN_NAN_MARK (1 << 24)

typedef void *dls_stream_t;

const char *dls_last_error(void);
int dls_abi_version(void);
/* First 16 hex digits of the SHA-256 of the library's sources and headers
 * (the csrc .hip sources, csrc/dls_common.h, csrc/quant_common.h, include/dls_hip.h, concatenated in build
 * order), fixed at build time: ties a loaded library to its source tree. */
const char *dls_source_hash(void);
int dls_device_count(void);
/* 1 if the dequant kernels divide by `divisor` (= fl32(N), fed_server.py:60)
 * with the two-constant method q = fma(a, yh, RN(a*yl)) — proven correctly
 * rounded for this divisor by an exhaustive host-side mantissa check, cached —
 * and 0 if they use the 3-op Markstein correction.  Host only; no GPU needed. */
int dls_two_constant_division(float divisor);

/* ------------------------------------------------------------------ FedAvg
 * Replaces FedServer.get_subset_model (servers/fed_server.py:44-66) for a
 * non-empty subset.
 *   U      fp32 [*, ldu]    client rows (flat parameter layout)
 *   rows   int32 [K]        row of U for each client, in the reference's
 *                           iteration order (dict key order / subset tuple)
 *   weight fp32 [K]         fl32(n_i): the Python int sample counts as torch
 *                           converts them (fed_server.py:59)
 *   total  fl32(sum n_i)    (fed_server.py:51-53,60)
 *   out    fp32 [P]         out = first term, then += (fed_server.py:62-65)
 * P, ldu multiples of 4; U and out 16-byte aligned. */
int dls_fedavg_f32(const float *U, int64_t ldu, const int32_t *rows, const float *weight,
                   int32_t K, float total, int64_t P, int32_t mode, float *out,
                   dls_stream_t stream);

/* Batched subset aggregation in reference order: S subsets at once.
 * Subset s lists sub_rows[sub_off[s] .. sub_off[s+1]) with matching
 * sub_weight[], divisor sub_total[s]; result row s of out [S, ldo].
 * Replaces the get_subset_model calls of the Shapley servers
 * (servers/GTG_shapley_value_server.py:56, multiround_shapley_value_server.py:37). */
int dls_subset_fedavg_f32(const float *U, int64_t ldu, const int32_t *sub_off,
                          const int32_t *sub_rows, const float *sub_weight,
                          const float *sub_total, int32_t S, int64_t P, float *out,
                          int64_t ldo, dls_stream_t stream);

/* The same batch, reading each client row ONCE (the Shapley servers' default
 * path: servers/GTG_shapley_value_server.py:56 and
 * servers/multiround_shapley_value_server.py:37 call get_subset_model,
 * servers/fed_server.py:44-66, once per coalition; a batch's coalitions share
 * their clients).
 *   urows   int32 [Ku]   row of U of each client of the batch's union
 *   uweight fp32  [Ku]   fl32(n_j)
 *   member  uint64 [Ku]  bit s set iff client j belongs to coalition s
 *   sub_total fp32 [S]   fl32(N_s) of coalition s, a HOST array (the library
 *                        derives each coalition's division constants on the
 *                        host, cf. dls_two_constant_division); S <= DLS_SUBSET_UNION_MAX
 * Row s of out [S, ldo] is coalition s's weighted mean, its members summed in
 * union order: bit-exact with the reference when every coalition lists its
 * clients in the union's order (the caller orders the union so — sorted
 * worker-id tuples, as the Shapley servers pass them, always are).  A coalition
 * without members leaves its row undefined. */
#define DLS_SUBSET_UNION_MAX 64
int dls_subset_fedavg_union_f32(const float *U, int64_t ldu, const int32_t *urows,
                                const float *uweight, const uint64_t *member, int32_t Ku,
                                const float *sub_total, int32_t S, int64_t P, float *out,
                                int64_t ldo, dls_stream_t stream);

/* Robust coordinate-wise aggregation: the trimmed mean (Yin et al. 2018) and, as
 * its case trim = (K-1)/2, the median of K client rows.  Generalises the hook
 * FedServer.get_subset_model (servers/fed_server.py:44-66) replaces by a
 * weighted mean: same operands and layout rules as dls_fedavg_f32 (rows device
 * int32 [K]; P, ldu multiples of 4, ldu >= P; U and out 16-byte aligned), but the
 * client weights n_i play no part.  Per flat coordinate, independently:
 *   1. order the K values ascending by IEEE value, -0.0 below +0.0 and every
 *      NaN (any sign or payload) above +inf: a total order, values with equal
 *      bits are interchangeable;
 *   2. drop the `trim` lowest and the `trim` highest: v[trim] .. v[K-1-trim],
 *      m = K - 2*trim >= 1 values, are kept;
 *   3. acc = v[trim]; acc = fl32(acc + v[i]) for i ascending (one rounding
 *      each); out = fl32(acc / fl32(m)), correctly rounded.  m == 1: out is
 *      v[trim]'s own bits (no addition, no division: -0.0 stays -0.0).
 * A NaN result — a kept NaN, or inf + -inf inside the sum — is the canonical
 * quiet NaN 0x7fc00000.  The median of an even K is fl32(fl32(lo + hi) / 2);
 * trim = 0 is the unweighted mean summed in ascending order (not FedAvg's
 * arithmetic).  The result depends only on the multiset of each column: the
 * same bits for any permutation of `rows`.
 * 1 <= K <= DLS_ROBUST_MAX_K and 0 <= 2*trim < K, checked (with the null
 * pointers) before any device call; P == 0 returns 0 without a launch. */
#define DLS_ROBUST_MAX_K 64
int dls_trimmed_mean_f32(const float *U, int64_t ldu, const int32_t *rows, int32_t K,
                         int32_t trim, int64_t P, float *out, dls_stream_t stream);

/* Mean around the median (MeaMed, Xie, Koyejo & Gupta 2018), which is also stage 2
 * of Bulyan (El Mhamdi, Guerraoui & Rouault 2018): per coordinate the mean of the
 * `keep` values closest to the median.  Unlike the trimmed mean the kept window
 * is not centred in the sorted order: it slides, per coordinate, to where the
 * values cluster.  Operands, layout rules and checks of dls_trimmed_mean_f32 (rows
 * device int32 [K], 1 <= K <= DLS_ROBUST_MAX_K; P, ldu multiples of 4, ldu >= P; U
 * and out 16-byte aligned; every check, the null pointers included, before any
 * device call; P == 0 returns 0 without a launch), with 1 <= keep <= K in place of
 * trim.  Per flat coordinate, independently:
 *   1. order the K values ascending in the total order of dls_trimmed_mean_f32
 *      (-0.0 below +0.0, every NaN above +inf): v[0] .. v[K-1];
 *   2. the median: med = v[(K-1)/2]'s own bits for an odd K,
 *      med = fl32(fl32(v[K/2-1] + v[K/2]) / 2) for an even K;
 *   3. the window start s: the first i in 0 .. K-keep-1 for which
 *      fl32(med - v[i]) > fl32(v[i+keep] - med) is false, s = K-keep if there is
 *      none; a comparison with a NaN is false.  In words: a window of `keep`
 *      consecutive sorted values slides upwards while the value leaving at the
 *      bottom is strictly farther from the median than the value entering at the
 *      top; an exact tie keeps the lower value.  (The true comparisons always form
 *      a prefix of i = 0, 1, ..., so s is also their count.)
 *   4. acc = v[s]; acc = fl32(acc + v[i]) for i = s+1 .. s+keep-1 ascending (one
 *      rounding each); out = fl32(acc / fl32(keep)), correctly rounded.
 *      keep == 1: out is v[s]'s own bits.  A NaN result is 0x7fc00000.
 * Consequences: the result depends only on the multiset of each column (the same
 * bits for any permutation of `rows`); keep == K gives the bits of
 * dls_trimmed_mean_f32 with trim 0; as long as at most K-keep values of a column
 * are NaN and its median is not NaN, no NaN is kept; keep == 1 with an odd K gives
 * the bits of the median whenever the median is finite and not a zero (the steps
 * decide elsewhere: {-0, +0, +0} gives -0, the tie keeps the lower value; with an
 * infinite or NaN median the comparisons against it are false where they would
 * meet inf - inf or the NaN, e.g. {1, inf, inf} gives 1). */
int dls_mean_around_median_f32(const float *U, int64_t ldu, const int32_t *rows, int32_t K,
                               int32_t keep, int64_t P, float *out, dls_stream_t stream);

/* Byzantine client updates crafted from the honest clients' rows, in place: the
 * omniscient coordinate-wise attacks the robust rules above are measured against.
 * Per coordinate out = base + a * (mean - base) + b * sigma over the Kh honest rows,
 * written into each of the Ka attacker rows of the same store.  "A little is enough"
 * (Baruch, Baruch & Goldberg 2019) is a = 1, b = -z, no base (mean - z * std); inner
 * product manipulation (Xie, Koyejo & Gupta 2019) is a = -eps, b = 0 with the
 * previous global model as base (-eps times the honest mean update).
 * hrows / arows are device int32 [Kh] / [Ka] tables of row indices of U, 1 <= Kh, Ka <=
 * DLS_ROBUST_MAX_K; they must not share a row (a precondition: the tables live on
 * the device and are not checked; rows in neither table are not touched).  a and b
 * are finite; base is NULL or P device floats (16-byte aligned); P, ldu multiples of
 * 4, ldu >= P; U 16-byte aligned.  Every check, the null pointers included, runs
 * before any device call; P == 0 returns 0 without a launch.
 * Per flat coordinate p, independently, with v[0] .. v[Kh-1] the honest values
 * U[hrows[k]][p] ascending in the total order of dls_trimmed_mean_f32 (-0.0 below
 * +0.0, every NaN above +inf):
 *   1. acc = v[0]; acc = fl32(acc + v[i]) ascending; mu = fl32(acc / fl32(Kh)),
 *      correctly rounded (Kh == 1: mu = v[0]'s own bits): the bits of
 *      dls_trimmed_mean_f32 with trim 0 on the same rows;
 *   2. only when b != 0: s = +0; ascending d = fl32(v[i] - mu), s = fmaf(d, d, s);
 *      var = fl32(s / fl32(Kh)) (Kh == 1: var = s), the population variance; sigma
 *      = the correctly rounded fp32 square root of var (denormals included);
 *   3. t = base ? fl32(mu - base[p]) : mu; r = fl32(a * t); if b != 0, r = fl32(r +
 *      fl32(b * sigma)); out = base ? fl32(base[p] + r) : r.  Multiply, then add:
 *      nothing is contracted but the one fmaf of step 2.  A NaN result is 0x7fc00000;
 *   4. U[arows[j]][p] = out for every j < Ka.
 * The result depends only on the multiset of each column: the same bits for any
 * order of hrows.  b == 0 (either sign) skips step 2, so a variance that overflows
 * cannot turn a pure a * mu into a NaN.  Columns P .. ldu-1 of every row are
 * untouched. */
int dls_craft_rows_f32(float *U, int64_t ldu, const int32_t *hrows, int32_t Kh,
                       const int32_t *arows, int32_t Ka, float a, float b, const float *base,
                       int64_t P, dls_stream_t stream);

/* Pairwise squared distances between K client rows: the hot path of the
 * distance-based robust rules (Krum / multi-Krum, Blanchard et al. 2017) and of
 * client similarity.  Operands and layout rules of dls_trimmed_mean_f32 (rows
 * device int32 [K]; P, ldu multiples of 4, ldu >= P; U 16-byte aligned;
 * 1 <= K <= DLS_ROBUST_MAX_K); D is device fp64 [K*K] row-major (8-byte aligned);
 * workspace is device memory of dls_pairwise_sqdist_workspace(K, P) bytes (a
 * function of K and P alone; 16-byte aligned), scratch for this call only.
 * Every check, the null pointers included, runs before any device call; P == 0
 * writes an all-zero D.
 *   D[a][b] ~ sum_p (U[rows[a]][p] - U[rows[b]][p])^2,
 * every term formed from the difference of the two values (never the Gram form
 * |x|^2 + |y|^2 - 2 x.y, which cancels catastrophically when clients differ in
 * the 3rd or 4th digit):
 *   d = fl32(x - y); acc = fmaf(d, d, acc) in fp32 chains of at most 120 terms;
 *   the chain results are converted to fp64 and added in fp64 in a fixed order.
 * All terms are non-negative, so for finite inputs whose terms neither overflow
 * nor underflow D[a][b] is within (120 + 8) * 2^-24 = 2^-17 relative of the
 * exact squared distance of the fp32 inputs.
 * Exact properties: D[a][a] is +0.0 (written, not computed); D[a][b] has the bits
 * of D[b][a]; repeated calls give the same bits on any stream; the summation
 * order is a function of P and K alone (not of the device's CU count, ldu, the
 * rows' position in U or the order of `rows`), so permuting `rows` permutes D
 * without changing a bit, and rows of equal contents get equal distances to
 * every third row.  No atomics: a second launch adds the per-wave partials of
 * `workspace` in ascending order.
 * If a row of the pair holds an inf or NaN, or a chain overflows, D[a][b]
 * (a != b) is +inf or NaN; callers treat both as +inf.  Pairs of clean rows are
 * unaffected.
 * Launch shape: a period is the longest run of coordinates one fp32 chain covers
 * (7680, 1920, 448 or 96 for K <= 8, 16, 32, 64); with periods = ceil(P / period),
 * ppw = ceil(periods / DLS_PAIRDIST_MAX_WAVES) and nW = ceil(periods / ppw), wave w of
 * the nW waves takes the periods w, w + nW, ..., at most ppw of them; the workspace
 * holds nW * 4096 doubles. */
#define DLS_PAIRDIST_MAX_WAVES 2048
int64_t dls_pairwise_sqdist_workspace(int32_t K, int64_t P);
int dls_pairwise_sqdist_f32(const float *U, int64_t ldu, const int32_t *rows, int32_t K, int64_t P,
                            double *D, void *workspace, dls_stream_t stream);

/* Gram matrix (inner products) of K client rows, read-only and fused with the
 * in-place fold of the rows into a per-client history: the hot path of the
 * direction-based robust rules (FoolsGold, Fung, Yoon & Beschastnikh 2020) and the
 * base of cosine similarity, trust scores and spectral filtering.  Operands, layout
 * rules and checks of dls_pairwise_sqdist_f32: rows (and hrows) device int32 [K],
 * 1 <= K <= DLS_ROBUST_MAX_K; P, ldu and ldh multiples of 4 and >= P; U, H, base and
 * workspace 16-byte aligned; G is device fp64 [K*K] row-major (8-byte aligned);
 * workspace is device memory of dls_rows_gram_workspace(K, P) bytes (a function of K
 * and P alone, the same for both calls), scratch for this call only; base is NULL or
 * P device floats.  Every check, the null pointers included, runs before any device
 * call; P == 0 writes an all-zero G and touches nothing else.
 * Per coordinate p,  h_k = base ? fl32(U[rows[k]][p] - base[p]) : U[rows[k]][p].
 *   dls_rows_gram_f32:  G[a][b] ~ sum_p h_a * h_b for every pair and the diagonal;
 *     nothing but G and the workspace is written.
 *   dls_history_gram_f32, the fused per-round step: H'[hrows[k]][p] = fl32(H[hrows[k]][p]
 *     + h_k), stored in place, and G is the Gram matrix of the rows of H'.  The
 *     addition is rounded once and never contracted with the subtraction: given the
 *     bits of U, base and H, H' is defined bit for bit (numpy float32 reproduces it).
 *     U, H and base are each read once and H is written once.  Columns P .. ldh-1 of
 *     H and the rows not listed in hrows are untouched.  hrows must be distinct and H
 *     must not overlap U or base (preconditions: the tables live on the device and are
 *     not checked here).
 * The Gram arithmetic is that of dls_pairwise_sqdist_f32 with the subtraction removed:
 *   acc = fmaf(h_a, h_b, acc) in fp32 chains of at most 120 terms; the chain results
 *   are converted to fp64 and added in fp64 in a fixed order that is a function of P
 *   and K alone.
 * The terms are signed, so the bound is not relative to the result: for finite inputs
 * whose terms neither overflow nor underflow
 *   |G[a][b] - exact| <= (120 + 8) * 2^-24 * sum_p |h_a h_b| <= 2^-17 * |h_a| |h_b|,
 * an absolute error of at most 2^-17 of the cosine G[a][b] / (|h_a| |h_b|).
 * Exact properties: G[a][b] has the bits of G[b][a]; permuting rows (together with
 * hrows) permutes G without changing a bit; rows of equal contents give G[a][b] ==
 * G[a][a] == G[b][b] bit for bit (the same chain of the same operands); repeated
 * read-only calls give the same bits on any stream, at any ldu and for any position
 * of the rows in U.  No atomics: a second launch adds the per-wave partials of
 * `workspace` in ascending order.  A row that holds an inf or NaN makes its own row
 * and column of G non-finite and leaves the other entries alone. */
int64_t dls_rows_gram_workspace(int32_t K, int64_t P);
int dls_rows_gram_f32(const float *U, int64_t ldu, const int32_t *rows, int32_t K, int64_t P,
                      const float *base, double *G, void *workspace, dls_stream_t stream);
int dls_history_gram_f32(const float *U, int64_t ldu, const int32_t *rows, float *H, int64_t ldh,
                         const int32_t *hrows, int32_t K, int64_t P, const float *base, double *G,
                         void *workspace, dls_stream_t stream);

/* Fused Weiszfeld step and squared distances of K client rows to one point: the
 * hot path of the geometric median (the smoothed Weiszfeld iteration of RFA,
 * Pillutla, Kakade & Harchaoui) and of "how far is every client from the
 * aggregate".  Operands and layout rules of dls_trimmed_mean_f32 (rows device
 * int32 [K], 1 <= K <= DLS_ROBUST_MAX_K; P, ldu multiples of 4, ldu >= P; U and z
 * 16-byte aligned); w is device fp32 [K]; dist2 is device fp64 [K] (8-byte
 * aligned); workspace is device memory of dls_weiszfeld_workspace(K, P) bytes (a
 * function of K and P alone; 16-byte aligned), scratch for this call only.  Every
 * check, the null pointers included, runs before any device call.
 *   dls_rows_sqdist_to_f32: z fp32 [P] is read;
 *   dls_weiszfeld_step_f32: z is computed from the rows and written (the old
 *     contents are never read), and dist2 is taken to that new z in the same
 *     visit, so the K values of a coordinate are read from HBM once per step.
 * The iterate of the step, per coordinate p, in the order of `rows`, every
 * operation rounded once and never fused:
 *   t_k = fl32(w[k] * U[rows[k]][p]);  acc = t_0;  acc = fl32(acc + t_k) for
 *   k = 1 .. K-1;  z[p] = acc.
 * Given the bits of w, z is defined bit for bit (numpy float32 reproduces it);
 * K = 1 with w = 1.0 returns the row's own bits, -0.0 included.  z does not depend
 * on ldu, on the rows' position in U, on the stream or on the CU count.
 * The distances, dist2[k] ~ sum_p (U[rows[k]][p] - z[p])^2, use the arithmetic of
 * dls_pairwise_sqdist_f32:
 *   d = fl32(x - z); acc = fmaf(d, d, acc) in fp32 chains of at most 120 terms;
 *   the chain results are converted to fp64 and added in fp64 in a fixed order
 *   that is a function of P and K alone.
 * All terms are non-negative, so for finite inputs whose terms neither overflow
 * nor underflow dist2[k] is within (120 + 8) * 2^-24 = 2^-17 relative of the exact
 * squared distance of the fp32 row to the fp32 z.
 * Exact properties: rows of equal contents get the same bits; a row equal to z
 * gets +0.0; coordinates past P contribute d = 0; repeated calls give the same
 * bits on any stream.  No atomics: a second launch adds the per-wave partials of
 * `workspace` in ascending order.  A row that holds an inf or NaN (or whose chain
 * overflows) gets +inf or NaN; in dls_rows_sqdist_to_f32 the other rows are
 * unaffected (in the step such a row with a non-zero weight poisons z).
 * P == 0 writes zeros to dist2, writes nothing to z and launches nothing else. */
int64_t dls_weiszfeld_workspace(int32_t K, int64_t P);
int dls_rows_sqdist_to_f32(const float *U, int64_t ldu, const int32_t *rows, int32_t K, int64_t P,
                           const float *z, double *dist2, void *workspace, dls_stream_t stream);
int dls_weiszfeld_step_f32(const float *U, int64_t ldu, const int32_t *rows, int32_t K,
                           const float *w, int64_t P, float *z, double *dist2,
                           void *workspace, dls_stream_t stream);

/* Fused centered-clipping step (Karimireddy, He & Jaggi 2021): the iterate moves
 * from where it is towards the K client rows by their clipped differences, and the
 * squared distances to the new iterate come out of the same visit.  Operands, layout
 * rules, workspace (dls_weiszfeld_workspace(K, P) bytes: the same plan) and checks of
 * dls_weiszfeld_step_f32; c is device fp32 [K], the callers' c_k = min(1, tau /
 * |x_k - z|) / K.  Every check, the null pointers included, runs before any device
 * call.
 * z fp32 [P] is read and overwritten in place.  Per coordinate p, in the order of
 * `rows`, every operation rounded once and never fused:
 *   d_k = fl32(U[rows[k]][p] - z[p]);  t_k = fl32(c[k] * d_k);  acc = t_0;
 *   acc = fl32(acc + t_k) for k = 1 .. K-1;  z'[p] = fl32(z[p] + acc).
 * Given the bits of c and of the old z, z' is defined bit for bit (numpy float32
 * reproduces it) whenever the result is not NaN; where the arithmetic gives NaN the
 * kernel gives some NaN, and the sign of a zero result is whatever IEEE gives the
 * formula.  z' does not depend on ldu, on the rows' position in U, on the stream or
 * on the CU count.
 * dist2[k] ~ sum_p (U[rows[k]][p] - z'[p])^2 is taken to the new z, with the
 * arithmetic and the 2^-17 relative bound of dls_weiszfeld_step_f32: d = fl32(x -
 * z'), fma chains of at most 120 terms, an fp64 sum in a fixed order that is a
 * function of P and K alone, no atomics.
 * Exact properties: a row equal to z' gets +0.0; rows of equal contents get the same
 * bits; coordinates past P contribute nothing; repeated calls from the same old z
 * give the same bits on any stream.  A row that holds an inf or NaN poisons z' even
 * with c[k] = 0 (0 * inf is NaN): callers leave such rows out.
 * P == 0 writes zeros to dist2, touches nothing of z and launches nothing else. */
int dls_centered_clip_step_f32(const float *U, int64_t ldu, const int32_t *rows, int32_t K,
                               const float *c, int64_t P, float *z, double *dist2,
                               void *workspace, dls_stream_t stream);

/* Fused server-optimizer step: the round's aggregate becomes the next global model
 * through a server optimizer instead of being stored as it is.  It replaces the round
 * end of servers/fed_server.py (:81-84, where the aggregate is stored as the next
 * model: server learning rate 1, no momentum): agg - x is the pseudo-gradient of
 * FedAvgM (Hsu et al. 2019; DLS_SERVER_OPT_SGD) or of FedAdagrad / FedAdam / FedYogi
 * (Reddi et al. 2021, "Adaptive Federated Optimization"; no bias correction).
 * agg, x, m, v, out are device fp32 [P], 4-byte aligned (DLS_ELAYOUT otherwise); m and
 * v are read and overwritten in place.  Per coordinate p, every operation rounded
 * once to fp32 and never fused; the coefficients are the bits passed in (omb1 and omb2
 * are the caller's roundings of 1 - beta1 and 1 - beta2; they are not recomputed):
 *   d = fl(agg - x)
 *   SGD:      m' = fl(fl(beta1*m) + d)            (m may be NULL only with beta1 == 0:
 *             out = fl(x + fl(lr*m'))              then m' = d and is not stored; v
 *                                                  must be NULL)
 *   adaptive: m' = fl(fl(beta1*m) + fl(omb1*d));  d2 = fl(d*d)
 *     ADAGRAD: v' = fl(v + d2)
 *     ADAM:    v' = fl(fl(beta2*v) + fl(omb2*d2))
 *     YOGI:    t = fl(v - d2);  s = (t > 0) - (t < 0);  v' = fl(v - fl(fl(omb2*d2) * s))
 *             out = fl(x + fl(lr*m') / fl(sqrt(v') + tau))
 * with the division and the square root correctly rounded and denormals kept.  Given
 * the input bits, out, m' and v' are defined bit for bit (numpy float32 reproduces
 * them) wherever the result is not NaN; where the arithmetic gives NaN the kernel
 * gives some NaN.  A NaN or inf in one coordinate never changes another coordinate.
 * The bits do not depend on the stream, the CU count or the pointers' alignment.
 * out may be x itself (the same pointer) or disjoint from everything; any other
 * overlap among the operands is an error.
 * Checks, all before any device call (DLS_EINVAL): kind outside 0..3, P < 0, a null
 * agg, x or out, v given for SGD or missing for an adaptive kind, m missing where it
 * is needed, a non-finite coefficient, overlapping operands.  P == 0 launches
 * nothing.
 * Launch shape (a thread steps DLS_SERVER_OPT_UNROLL 16-byte vectors per visit; blocks
 * of DLS_SERVER_OPT_BLOCK threads, at most DLS_SERVER_OPT_MAX_BLOCKS, grid-strided):
 * 16-byte accesses where every operand shares one 16-byte phase (up to 3 elements at
 * either end go one by one), one element at a time otherwise. */
#define DLS_SERVER_OPT_SGD 0
#define DLS_SERVER_OPT_ADAGRAD 1
#define DLS_SERVER_OPT_ADAM 2
#define DLS_SERVER_OPT_YOGI 3
#define DLS_SERVER_OPT_BLOCK 256
#define DLS_SERVER_OPT_MAX_BLOCKS 2048
#define DLS_SERVER_OPT_UNROLL 2
int dls_server_opt_step_f32(int32_t kind, const float *agg, const float *x, float *m, float *v,
                            float *out, int64_t P, float lr, float beta1, float omb1,
                            float beta2, float omb2, float tau, dls_stream_t stream);

/* SCAFFOLD control variates and the FedProx proximal term (csrc/scaffold.hip; Karimireddy,
 * Kale, Mohri, Reddi, Stich & Suresh 2020, "SCAFFOLD: stochastic controlled averaging for
 * federated learning", with the paper's option II for the client control variate; Li et al.
 * 2020, "Federated optimization in heterogeneous networks").  The reference simulator has
 * neither: the definitions below are this library's and tests/scaffold_ref.py restates them
 * in numpy float32.  Every operation is rounded once to fp32 and never fused, so given the
 * input bits every output is defined bit for bit wherever it is not NaN.  Nothing is
 * synchronised inside a call and every check runs before any device call.
 *
 * dls_scaffold_local_step_f32, the client's optimizer step (plain SGD) over T tensors.  p, g,
 * off, n are HOST arrays of T entries: device pointers of the parameter and its gradient (n[t]
 * fp32 each, memory in logical order, 4-byte aligned, not overlapping), the tensor's first
 * index off[t] in the flat vectors x (the round's global model) and corr (c - c_i), fp32 [P].
 * Per element, q = off[t] + its index:
 *   d = g;  d = fl(d + fl(wd * p)) if wd != 0;  d = fl(d + fl(mu * fl(p - x[q]))) if mu != 0;
 *   d = fl(d + corr[q]) if control;  p = fl(p - fl(lr * d)).
 * x is not read (and may be NULL) when mu == 0, corr likewise when control == 0; then off is
 * not looked at either.  Launches: ceil(T' / DLS_SCAFFOLD_MAX_SEGS) for the T' tensors with
 * n > 0, the segment table passed in the kernel arguments; a wave steps DLS_SCAFFOLD_TILE
 * elements of one tensor, with 16-byte accesses where p[t], g[t], x + off[t] and corr +
 * off[t] are 16-byte aligned and one element per access otherwise: the bits do not depend
 * on the alignment.  Elements past n[t] are neither read nor written.  DLS_EINVAL: a null
 * pointer, T < 0, control not 0 or 1, a non-finite lr, wd or mu, a segment outside [0, P);
 * DLS_ELAYOUT: a pointer that is not 4-byte aligned.
 *
 * dls_scaffold_finish_f32, the client's round end: y the local model, x the round's global
 * model, c the server control variate, ci the client's, all fp32 [P], P a positive multiple
 * of 4, 16-byte aligned.  Per coordinate
 *   delta = fl(y - x);  ci' = fl(fl(ci - c) - fl(a * delta))   (option II; ci in place)
 * with a the caller's fl32(1 / (steps * lr)); stats[0] is set, not added to, to the number of
 * non-finite delta (the call completes, the caller decides).  control == 0 writes delta and
 * stats alone and c, ci may be NULL.  delta, ci and stats overlap nothing else.  One launch;
 * the count meets in one 64-bit word per HIP stream (as dls_drive_compress_f32).
 *
 * dls_scaffold_server_step_f32, the server's round end over the K delta rows U[rows[k]][0, P)
 * in the order of `rows` (operands as the rows family: P and ldu multiples of 4, ldu >= P, U
 * and the vectors 16-byte aligned; 1 <= K <= DLS_SCAFFOLD_MAX_K).  weight[k] = fl32(n_k),
 * total = fl32(sum n_k), b[k] = the caller's fl32(1 / (steps_k * lr_k * N)), f = fl32(K / N),
 * N the population.  Per coordinate
 *   acc: t_k = fl(fl(U_k * weight[k]) / total) (the correctly rounded division of
 *        DLS_FEDAVG_EXACT), acc = t_0, acc = fl(acc + t_k): dls_fedavg_f32's bits
 *   s:   s = fl(b[0] * U_0), s = fl(s + fl(b[k] * U_k))
 *   x_out = fl(x + fl(eta_g * acc));  c_out = fl(fl(c - fl(f * c)) - s)
 * x_out may be x itself and c_out c itself (the same pointer); nothing else may overlap.
 * control == 0 computes x_out alone: b, c and c_out are not touched and may be NULL.  One
 * launch, no atomics, (K + 2) * 4P bytes read and 8P written; the same bits for any pitch,
 * stream or CU count.  P == 0 launches nothing. */
#define DLS_SCAFFOLD_MAX_SEGS 32
#define DLS_SCAFFOLD_TILE 256
#define DLS_SCAFFOLD_MAX_K 1024
int dls_scaffold_local_step_f32(float *const *p, const float *const *g, const int64_t *off,
                                const int64_t *n, int32_t T, const float *x, const float *corr,
                                int64_t P, float lr, float wd, float mu, int32_t control,
                                dls_stream_t stream);
int dls_scaffold_finish_f32(const float *y, const float *x, const float *c, float *ci,
                            float *delta, int64_t P, float a, int32_t control, int32_t *stats,
                            dls_stream_t stream);
int dls_scaffold_server_step_f32(const float *U, int64_t ldu, const int32_t *rows,
                                 const float *weight, const float *b, int32_t K, float total,
                                 int64_t P, float eta_g, float f, const float *x, const float *c,
                                 float *x_out, float *c_out, int32_t control,
                                 dls_stream_t stream);

/* Width-heterogeneous FedAvg (csrc/hetero.hip; HeteroFL, Diao, Ding & Tarokh 2021; FedRolex,
 * Alam, Liu, Yan & Zhang 2022): clients train narrower copies of the model and the server
 * averages every coordinate over the clients that hold it.  The reference simulator has
 * neither: the definitions below are this library's and tests/hetero_ref.py restates them in
 * numpy float32.
 *
 * The slice model.  The global row is T tensors in the flat layout (each starts at a multiple
 * of 64 elements, the padding follows it); tensor t is an array [O, I, R] in row-major order.  A
 * width level l holds O_l <= O and I_l <= I indices of the first two dimensions: its local
 * index jo stands for the global index (shO + jo) mod O, ji for (shI + ji) mod I (shift 0: a
 * prefix, HeteroFL; shift = round mod C: FedRolex).  The level's own tensor is the contiguous
 * [O_l, I_l, R] at its own flat-layout offset in the level's compact row of P_l elements.
 *
 * The plan, int32 words, host-made; an entry point takes the host copy, checks EVERY word of
 * it before anything is launched (the kernels index with them), and hands the kernel the
 * device copy `plan_dev` of the same words, which the caller keeps in step:
 *   [0] DLS_HETERO_MAGIC  [1] T  [2] L  [3] tiles  [4] P  [5..7] 0  [8 + l] P_l (0 for l >= L)
 *   [16 + t]                    tile prefix: the DLS_HETERO_TILE-element tiles of tensors 0..t,
 *                               ceil(pad64(O I R) / DLS_HETERO_TILE) each
 *   [16 + T + t * 76 ...]       tensor t: 12 words  offset, O, I, R, m(I R), s(I R), m(R), s(R),
 *                               vector path (0 / 1), O I R, I R, pad64(O I R)
 *                               then per level l < 8 (zeros past L) 8 words  offset in the level's
 *                               row, O_l, I_l, shO, shI, I_l R, O_l I_l R, 0
 * (m, s)(d) divide by d without an integer divide: floor(n / d) = mulhi32(n, m) >> s for n <
 * 2^31 with l = ceil(log2 d), m = floor(2^(31 + l) / d) + 1, s = l - 1; d = 1 is m = s = 0.
 * The vector path is taken by a tensor with every shift 0 and I R and every I_l R multiples of
 * 4.  1 <= L <= DLS_HETERO_MAX_LEVELS, 1 <= T <= DLS_HETERO_MAX_TENSORS, a tensor has at
 * most 2^30 elements and P, P_l < 2^31.
 *
 * dls_hetero_fedavg_f32, the server's round in one launch.  clients: K records of 4 words in id
 * order, {level, the bits of w_k = fl32(n_k), row start low, high}, host copy and device copy
 * as for the plan; client k's compact row is ragged[start_k, start_k + P_level) (start_k a
 * multiple of 4, inside ragged_len).  Per global coordinate j of a tensor, M_j the clients
 * whose level holds j, in ascending k:
 *   M_j empty:  out[j] has the bits of prev[j] (NaN payloads and -0 kept)
 *   otherwise:  acc = fl(w_k u_k[j]) of the first member, acc = fl(acc + fl(w_k u_k[j])) of the
 *               rest; den = the same chain over w_k; out[j] = fl(acc / den), correctly rounded
 * Every operation is rounded once and never fused, so the bits are defined wherever the result
 * is not NaN; a non-finite value of one client reaches only the coordinates that client holds.
 * The padding after a tensor is written as zero.  out may be prev itself and overlaps nothing
 * else.  No atomics; the same bits for any stream or CU count.  sum_k 4 P_k + 8 P bytes of HBM
 * traffic.  DLS_EINVAL: a null pointer, a word of the plan that does not follow, K outside
 * 1..DLS_HETERO_MAX_K, a level outside the plan, a weight that is not finite and > 0, a row
 * outside ragged; DLS_ELAYOUT: a device pointer that is not 16-byte aligned.
 *
 * dls_hetero_extract_f32, the downlink in one launch: rows[sum_{m < l} P_m + ...] becomes level
 * l's compact row of `global`, every element a bit-for-bit copy, every padding zero; the global
 * row is read once.  rows_len >= sum_l P_l; rows overlaps nothing. */
#define DLS_HETERO_MAGIC 0x48545231
#define DLS_HETERO_MAX_LEVELS 8
#define DLS_HETERO_MAX_K 1024
#define DLS_HETERO_MAX_TENSORS 4096
#define DLS_HETERO_TILE 1024
#define DLS_HETERO_HEADER_WORDS 16
#define DLS_HETERO_TENSOR_WORDS 12
#define DLS_HETERO_LEVEL_WORDS 8
int dls_hetero_fedavg_f32(const int32_t *plan, const int32_t *plan_dev, int64_t plan_words,
                          const int32_t *clients, const int32_t *clients_dev, int32_t K,
                          const float *ragged, int64_t ragged_len, const float *prev, float *out,
                          dls_stream_t stream);
int dls_hetero_extract_f32(const int32_t *plan, const int32_t *plan_dev, int64_t plan_words,
                           const float *global, float *rows, int64_t rows_len,
                           dls_stream_t stream);

/* Subset aggregation as a dense fp32 MFMA contraction: out[S, P] = C[S, K] · U[rows, P]
 * (C row-major [S, K], c_si = n_i / N_S; rows[K] selects the K client rows of U).
 * fp32 in / fp32 accumulate (v_mfma_f32_32x32x2_f32): per element one fma chain in
 * the order of `rows`, started from +0.0; S is cut into chunks of 64 and K into chunks
 * of 256 clients, a later client chunk continuing the chain from the fp32 value the
 * chunk before it stored.
 * Accuracy, elementwise: |out[s][p] - sum_k c_sk U[rows[k]][p]| <= g * sum_k |c_sk|
 * |U[rows[k]][p]| with g = (K+1)u / (1 - (K+1)u), u = 2^-24 (every term: at most one
 * product rounding and K additions), while products and sums stay in the normal
 * range; subnormals are kept, not flushed.  Where every product and every partial sum
 * is exactly representable (small integers times dyadic coefficients) the result is
 * exact, bit for bit, for any S, K, P and pitch.
 * Layout: P, ldu and ldo are multiples of 4, U and out 16-byte aligned
 * (DLS_ELAYOUT otherwise); S, K, P > 0 (DLS_EINVAL otherwise); a failed check writes
 * nothing.  Exactly out[s][0 .. P) for s < S is written: out[s][P .. ldo) and rows of
 * out past S are left alone.  Only U[rows[k]][0 .. P) is read: rows of U that `rows`
 * does not name and U[..][P .. ldu) may hold anything.  A row may be listed more than
 * once in `rows`: each listing is a term of its own.
 * Non-finite rows: unlike the exact kernels, which read only a coalition's members,
 * the contraction multiplies EVERY selected row by its coefficient, so an inf or NaN
 * in U[rows[k]][p] makes out[s][p] non-finite in every coalition s of the call, the
 * ones with c_sk = 0 included (0 * inf is NaN; NaN where the row holds NaN or c_sk is
 * 0, +-inf where c_sk != 0 meets an inf).  Other columns are not affected.  A caller
 * that needs the coalitions without a diverged client to stay finite uses the exact
 * kernels, or a call whose `rows` leaves that row out. */
int dls_subset_gemm_f32(const float *C, int32_t S, int32_t K, const float *U, int64_t ldu,
                        const int32_t *rows, int64_t P, float *out, int64_t ldo,
                        dls_stream_t stream);

/* -------------------------------------------------------------- sign vote
 * Producer side of workers/sign_sgd_worker.py:44 (torch.sign) + the 16x smaller
 * wire format: pack fp32 vectors X [K, ldx] into planes [K, ldp] (ldp >=
 * DLS_SIGN_WORDS(P)).  Values other than -1, 0, +1, NaN are counted into
 * *nonternary (device int32, accumulated; caller zeroes it) when it is
 * non-null, because the vote of such inputs would differ from the reference's
 * fp32 sum. */
int dls_sign_pack_f32(const float *X, int64_t ldx, int32_t K, int64_t P, uint64_t *planes,
                      int64_t ldp, int32_t *nonternary, dls_stream_t stream);

/* SignSGDServer.__worker (servers/sign_sgd_server.py:12-21): counts[p] =
 * sum over the K client rows of (+1 pos, -1 neg, +NAN_MARK nan).  `rows` may be
 * NULL (rows 0..K-1).  counts may be all-reduced (int32 sum) across ranks. */
int dls_sign_vote_count(const uint64_t *planes, int64_t ldp, const int32_t *rows, int32_t K,
                        int64_t P, int32_t *counts, dls_stream_t stream);

/* counts -> torch.sign(sum) as fp32 {-1, +0, +1} (NaN-poisoned -> 0, as CPU
 * torch.sign(nan)), and optionally the vote packed in the plane format. */
int dls_sign_from_counts(const int32_t *counts, int64_t P, float *sign_out,
                         uint64_t *vote_planes, dls_stream_t stream);

/* Fused single-device vote: planes -> any of fp32 signs, int32 counts and the
 * vote packed in the plane format (DLS_SIGN_WORDS(P) words, NaN-poisoned and
 * tied parameters 0); NULL outputs are skipped, at least one must be given. */
int dls_sign_vote(const uint64_t *planes, int64_t ldp, const int32_t *rows, int32_t K, int64_t P,
                  int32_t *counts, float *sign_out, uint64_t *vote_planes, dls_stream_t stream);

/* dls_sign_vote_geometry / dls_sign_vote_wave_ranges: host-only queries (no
 * stream, no launch) of how dls_sign_vote and dls_sign_vote_count split a model
 * of P parameters and K client rows over waves.  A vote group is 64 parameters;
 * the vote walks DLS_SIGN_WORDS(P) / 2 of them.  *nwaves waves each own one
 * contiguous range of groups, a lane owns *G of a range's groups (1..4), and
 * *waves_per_block waves share a block; every range is at most 64 * *G groups
 * long.  cus: the compute units to size the launch for; cus <= 0 asks the current
 * device (the one call here that touches it).  The launch and the queries run
 * the same functions (csrc/sign_geometry.h).  Null outputs are skipped.
 * dls_sign_vote_wave_ranges writes the ranges [wlo[i], whi[i]) of the waves
 * first_wave + i, i < count; together the ranges of waves 0..*nwaves-1 partition
 * [0, DLS_SIGN_WORDS(P) / 2). */
int dls_sign_vote_geometry(int64_t P, int32_t K, int32_t cus, int64_t *nwaves, int32_t *G,
                           int32_t *waves_per_block);
int dls_sign_vote_wave_ranges(int64_t P, int32_t K, int32_t cus, int64_t first_wave, int64_t count,
                              int64_t *wlo, int64_t *whi);

/* Worker step, workers/sign_sgd_worker.py:32-44 fused: momentum / dampening /
 * nesterov on grad (buf updated in place; first=1 clones), torch.sign, pack to
 * planes, optional fp32 sign copy.  a = fl32(1 - dampening).  Writes exactly
 * 2*ceil(P/64) plane words, so one tensor can fill its slice of a shared row
 * (tensors start at multiples of 64 parameters). */
int dls_sign_sgd_direction(const float *grad, float *buf, int64_t P, float momentum,
                           float one_minus_dampening, int32_t nesterov, int32_t first,
                           uint64_t *planes, float *sign_out, dls_stream_t stream);

/* workers/sign_sgd_worker.py:48-57: p = fma(vote + wd*p, -lr, p) with the vote
 * read from packed planes (NaN-poisoned or tied -> 0). */
int dls_sign_sgd_apply(float *param, const uint64_t *vote_planes, int64_t P, float neg_lr,
                       float weight_decay, dls_stream_t stream);

/* ----------------------------------------------------------------- quant
 * Wave tile of the flattened parameter space for the fused dequant-FedAvg
 * kernels.  A tile lies inside one tensor; host code builds the table once per
 * layout, with the "fast" tiles first: int tiles (kind 1/2) whose real
 * elements all lie in channel chan0, grouped by 1 KiB slice count. */
typedef struct dls_qtile {
    int64_t dst;     /* first output element (flat layout offset, multiple of 16) */
    int64_t src;     /* first element within a client row of Q (kind 1/2) or F (kind 0) */
    int32_t len;     /* elements: <= 4096 for the grouped tiles, <= 1024 for the rest;
                        lanes cover 16-element chunks (lane l, KiB slice g: element
                        1024 g + 16 l) up to the next multiple of 64 (the rows are
                        padded to 64) and write 0 past len, so the output's row
                        padding is always zero */
    int32_t kind;    /* 0 = fp32 tensor, 1 = int8 per-channel, 2 = uint8 per-channel */
    int32_t chan0;   /* channel (index into the client's scale/zp row) of element 0 */
    int32_t row_len; /* elements per output channel */
    int32_t row_pos; /* position of element 0 inside its channel row */
    int32_t chan_end; /* one past the tensor's last channel (clamps padded tails) */
} dls_qtile;

/* FedQuantServer._process_client_parameter (servers/fed_quant_server.py:25-33)
 * fused into FedServer.get_subset_model (servers/fed_server.py:44-66):
 *   out[e] (+)= fl(fl(fl(fl(q - zp[c]) * scale[c]) * n_i) / N)  (int tensors)
 *   out[e] (+)= fl(fl(x * n_i) / N)                              (fp32 tensors)
 * bit-exact in client order.  Q int8/uint8 [*, ldq], F fp32 [*, ldf],
 * sz fp32 pairs (fl32(scale), zero_point): client row r, channel c at pair
 * r * sz_row + c * sz_chan (the store keeps them channel-major: sz_row = 1).
 * nfast: host array of DLS_QTILE_GROUPS counts; the table starts with
 * nfast[0..3] one-channel int tiles of 4, 3, 2, 1 KiB slices (every real
 * element in channel chan0), then nfast[4..7] multi-channel int tiles of 4, 3,
 * 2, 1 KiB slices (channel rows a multiple of 16 elements: no lane's 16-element
 * chunk straddles two channels; a tile spanning more than 4 channels takes the
 * per-client path), then nfast[8] fp32 tiles of <= 256 elements,
 * nfast[9] int tiles of <= 256 elements of tensors with channel rows of >= 4
 * elements (a lane's 4 elements span at most two channels); the remaining tiles
 * (len <= 1024) are int tiles of any shape (see dls_qtile). */
#define DLS_QTILE_GROUPS 10
int dls_dequant_fedavg(const dls_qtile *tiles, int32_t ntiles, const int32_t *nfast, const void *Q,
                       int64_t ldq, const float *F, int64_t ldf, const float *sz, int64_t sz_row,
                       int64_t sz_chan, const int32_t *rows, const float *weight, int32_t K,
                       float total, float *out, dls_stream_t stream);
/* The same with a mode (DLS_FEDAVG_EXACT: dls_dequant_fedavg, bit-exact;
 * DLS_FEDAVG_FMA: the int tiles of groups 0-7 accumulate out = fma(q - zp, c,
 * out) with one constant per (client, channel) c = fl(fl(scale * n_i) / N)
 * (q - zp exact) — a conversion and two packed ops per element pair instead of
 * the exact mode's six, a different rounding of each term: within the
 * north-star's 1e-6 FedAvg tolerance (normwise), not bit-exact; groups 8-9 and
 * the general tiles keep the exact arithmetic.  Groups 0-7 run on one kernel in
 * launch pieces of one wave per SIMD (groups 8-9 beside its first piece), so the one-channel / lane split does not
 * matter here: the store's FMA table lane-tiles every int tensor whose channel
 * rows are a multiple of 16 elements, long rows included). */
int dls_dequant_fedavg_mode(const dls_qtile *tiles, int32_t ntiles, const int32_t *nfast,
                            const void *Q, int64_t ldq, const float *F, int64_t ldf,
                            const float *sz, int64_t sz_row, int64_t sz_chan, const int32_t *rows,
                            const float *weight, int32_t K, float total, int32_t mode, float *out,
                            dls_stream_t stream);

/* Per-segment min / max of x over [seg_off[s], seg_off[s+1]) (torch.aminmax);
 * seg_off is device int64 [nseg+1] with seg_off[nseg] == total.  NaNs are
 * ignored (fminf/fmaxf); an empty or all-NaN segment gives the identities
 * (+inf, -inf).  Zeros compare by value: the sign of a zero result is not
 * defined (a segment of -0.0 alone has min == max == 0), +-inf are ordinary
 * values.  x needs fp32 alignment only (16-byte aligned chunks load as
 * vectors). */
int dls_segment_minmax_f32(const float *x, const int64_t *seg_off, int32_t nseg, float *mins,
                           float *maxs, int64_t total, dls_stream_t stream);

/* MinMaxObserver-style qparams on device (torch.ao _calculate_qparams, fp32):
 *   affine:    scale = max((max(hi,0) - min(lo,0)) / (qmax - qmin), eps),
 *              zp = clamp(qmin - rne(min(lo,0) / scale), qmin, qmax);
 *   symmetric: scale = max(max(-min(lo,0), max(hi,0)) / ((qmax - qmin) / 2), eps),
 *              zp = 0 (signed range) or (qmin + qmax + 1) / 2 (unsigned).
 * Every operation rounds once to fp32, eps = 2^-23, min / max are fminf /
 * fmaxf (a NaN operand is dropped).  So the identities (+inf, -inf) of an empty
 * segment give the range [0, 0]: scale = eps, affine zp = qmin.  A non-finite
 * bound gives scale = +inf; the affine zp is then qmin (lo / inf = -0, and for
 * lo = -inf the NaN of inf / inf is dropped by the clamp's fmaxf).  The
 * unsigned symmetric zp is the up-rounded midpoint, 128 for [0, 255] like
 * torch's quint8 default; torch's observers take the down-rounded midpoint when
 * given a custom range, and choose by dtype, not by the sign of qmin. */
int dls_qparams_minmax(const float *mins, const float *maxs, int32_t nseg, int32_t qmin,
                       int32_t qmax, int32_t symmetric, float *scale, int32_t *zp,
                       dls_stream_t stream);

/* Affine quantize per segment (torch quantize_per_tensor / _per_channel):
 * q = clamp(rne(x * fl(1/scale)) + zp, qmin, qmax) stored as one byte (int8 for
 * qmin < 0, else uint8); stochastic=1 replaces rne by floor(v + u),
 * u = counter-based uniform(seed, element) (parity unpinned).  deq (optional)
 * = fl(fl(q - zp) * scale), the client-side dequant formula.  A NaN quantizes
 * to qmin (the clamp's fmaxf drops it), +inf to qmax and -inf to qmin, in
 * either rounding mode; -0.0 quantizes like +0.0.  Only bytes [0, total) of q
 * and floats [0, total) of deq are written; q needs no alignment.  The uniform
 * of an element depends on (seed, element index) alone, not on the segments. */
int dls_quantize_affine(const float *x, const int64_t *seg_off, int32_t nseg, const float *scale,
                        const int32_t *zp, int32_t qmin, int32_t qmax, void *q, float *deq,
                        int32_t stochastic, uint64_t seed, int64_t total, dls_stream_t stream);

/* ------------------------------------------------------- utility evaluation
 * Eval-mode batch norm for the Shapley servers' utility inference
 * (servers/fed_server.py:26-32 get_metric -> tester.inference()).
 * dls_bn_fold_f32: per channel alpha = fl(invstd * w), beta = fl(b - fl(mean * alpha)),
 * invstd = fl(1 / fl(sqrt(fl(var + eps)))) (ATen's CPU inference constants);
 * weight / bias may be null (affine=False: w = 1, b = 0).
 * dls_bn_act_nhwc_f32: y = fl(fl(x * alpha_c) + beta_c), then + residual (if
 * not null) and ReLU (if relu) over a channels_last [rows = N*H*W, C] fp32
 * tensor in one pass; C a multiple of 4, 16-byte aligned pointers; y may
 * alias x or residual.
 * ReLU, here and in the exact passes below: t > 0 ? t : 0 with NaN kept, so a
 * pre-activation of -0 (x = -0, mean = +0, b = -0; or a -0 residual) gives +0,
 * the bits torch.relu gives on the device (measured on gfx950; on a CPU torch
 * keeps the -0).  Every step is IEEE fp32 with denormals kept. */
int dls_bn_fold_f32(const float *weight, const float *bias, const float *mean, const float *var,
                    float eps, int32_t C, float *alpha, float *beta, dls_stream_t stream);
int dls_bn_act_nhwc_f32(const float *x, int64_t rows, int32_t C, const float *alpha,
                        const float *beta, const float *residual, int32_t relu, float *y,
                        dls_stream_t stream);
/* The same pass with the GPU library's eval batch-norm arithmetic (the reference
 * model's own eval forward on this stack runs MIOpen's
 * MIOpenBatchNormFwdInferSpatialEst): y = fma(w_c, fl(fl(x - mean_c) * iv_c), b_c),
 * iv_c = v_rsq_f32(|var_c + eps|), then + residual and ReLU as above: bit-identical
 * to torch's eval BatchNorm2d here.  dls_bn_fold_exact_f32 writes
 * consts = [mean | iv | w | b] (4*C floats, 16-byte aligned).  iv is within 1 ulp
 * of 1 / sqrt(|var_c + eps|) for a normal argument (0.86 ulp measured), +inf at 0
 * and at a denormal argument (the instruction reads a denormal as zero), +0 at
 * inf, NaN at NaN. */
int dls_bn_fold_exact_f32(const float *weight, const float *bias, const float *mean,
                          const float *var, float eps, int32_t C, float *consts,
                          dls_stream_t stream);
int dls_bn_act_exact_nhwc_f32(const float *x, int64_t rows, int32_t C, const float *consts,
                              const float *residual, int32_t relu, float *y, dls_stream_t stream);
/* The same exact pass over an NCHW (contiguous) [N, C, H, W] fp32 tensor, HW =
 * H*W (MIOpen's deterministic convolutions are NCHW ones: the reproducible
 * utility evaluation runs in that layout): float4 planes when HW is a multiple
 * of 4 and the pointers 16-byte aligned, one element per lane otherwise (any
 * input size: ResNet-18's adaptive pooling takes 28x28, whose layer3 planes are
 * 7x7).  y may alias x or residual. */
int dls_bn_act_exact_nchw_f32(const float *x, int64_t N, int32_t C, int64_t HW,
                              const float *consts, const float *residual, int32_t relu, float *y,
                              dls_stream_t stream);

/* Deterministic convolutions of the utility evaluation (replace the tester's
 * torch / MIOpen conv2d in the model forward behind servers/fed_server.py:26-32;
 * csrc/conv.hip).  Every output is reduced in one fixed order by one wave: the
 * same inputs give the same bits in any process.  fp32 values are carried as
 * bf16 pairs (hi = rne(x), lo = rne(x - hi)), products as hi*hi + hi*lo + lo*hi
 * with fp32 accumulation.
 * "split NHWC" activation: uint16 [B][H][W][2C] (per pixel C hi, then C lo).
 * split weights: uint16 [Cout][2K] (K hi, then K lo), k = (ky*KW + kx)*Cp + ci.
 * dls_conv_pack_input_f32: NCHW fp32 [B][C][H][W] -> split NHWC with Cp channels
 * (Cp >= C, a multiple of 32; zeros beyond C).
 * dls_conv_pack_weights_f32: fp32 [Cout][Cin][KH][KW] -> split weights, Cp as above.
 * dls_conv_pack_im2col_f32 / dls_conv_pack_weights_im2col_f32: a first layer with
 * few input channels as a 1x1 convolution over its im2col: split NHWC
 * [B][Ho][Wo][2 Kp] / split weights [Cout][2 Kp], k = (ky*KW + kx)*C + ci, zero
 * for k >= KH*KW*C (Kp a multiple of 32).
 * dls_conv_bn_act_split: y = act(bn(conv(x, w)) [+ residual]) in split NHWC;
 * bn = the exact eval batch norm above (consts = [mean | iv | w | b], or null:
 * none); residual split NHWC of y's shape or null; relu 0/1.  C a multiple of
 * 32, Cout of 64; 16-byte aligned pointers; y must not alias x or residual.
 * dls_conv_stem_bn_act_f32: the same for a first layer whose reduction is one chunk
 * (KH*KW*C <= 32: a 3-channel 3x3 stem), straight from the fp32 NCHW image batch
 * (the im2col fused), w from dls_conv_pack_weights_im2col_f32 (Kp = 32).
 * dls_pool_linear_split: logits[b][o] = sum_c mean_pixels(x[b])[c] * weight[o][c]
 * + bias[o] over a split NHWC [B][HW][2C] activation (C <= 2048; bias may be
 * null), every sum in a fixed order.
 * The split of a value x: hi = rne_bf16(x), lo = rne_bf16(x - hi), and lo = 0
 * whenever hi is not finite — an inf or NaN x, and a finite x that rounds to
 * bf16 infinity (|x| >= 0x7f7f8000, as a plain bf16 conversion rounds it) — so
 * hi + lo is never inf - inf.
 * dls_conv_kernel_choice / dls_conv_stem_kernel_choice: host-only queries (no
 * device call, no stream): the kernel instantiation dls_conv_bn_act_split /
 * dls_conv_stem_bn_act_f32 launches for a shape (a DLS_CONV_KERNEL_* /
 * DLS_STEM_KERNEL_* id below; *_NONE for an empty batch, which launches
 * nothing), or the negative status the launch would return for that shape.
 * The launch and the query run the same decision code; the choice depends on
 * the shape alone. */
#define DLS_CONV_KERNEL_NONE 0          /* B = 0: no launch */
#define DLS_CONV_KERNEL_GENERIC64 1     /* k_conv_bf16x3<1,4>: 64 channels x 256 pixels */
#define DLS_CONV_KERNEL_GENERIC128 2    /* k_conv_bf16x3<2,2>: 128 x 128 */
#define DLS_CONV_KERNEL_PIPE64_H10 3    /* k_conv3x3_pipe16<1,4,10,1,2> */
#define DLS_CONV_KERNEL_PIPE64_H12 4    /* k_conv3x3_pipe16<1,4,12,1,2> */
#define DLS_CONV_KERNEL_PIPE128_W4 5    /* k_conv3x3_pipe16<2,2,5,1,2> */
#define DLS_CONV_KERNEL_PIPE128_W8_H5 6 /* k_conv3x3_pipe16<2,4,5> */
#define DLS_CONV_KERNEL_PIPE128_W8_H6 7 /* k_conv3x3_pipe16<2,4,6> */
#define DLS_CONV_KERNEL_HALO128 8       /* k_conv3x3_halo<2,2,9,false> */
#define DLS_CONV_KERNEL_HALO128_SKEW 9  /* k_conv3x3_halo<2,2,9,true> */
#define DLS_CONV_KERNEL_HALO64 10       /* k_conv3x3_halo<1,4,11,false> */
#define DLS_CONV_KERNEL_HALO64_SKEW 11  /* k_conv3x3_halo<1,4,11,true> */
#define DLS_CONV_KERNEL_PHASE 12        /* k_conv3x3s2_phase<2,4,5> */
#define DLS_STEM_KERNEL_NONE 0          /* B = 0: no launch */
#define DLS_STEM_KERNEL_WINDOW 1        /* k_conv_stem<4,3,3,true,2>: 3-channel 3x3, W = 32, H % 8 = 0 */
#define DLS_STEM_KERNEL_3X3 2           /* k_conv_stem<4,3,3> */
#define DLS_STEM_KERNEL_GENERIC 3       /* k_conv_stem<4> */
int dls_conv_kernel_choice(int64_t B, int32_t H, int32_t W, int32_t C, int32_t Cout, int32_t KH,
                           int32_t KW, int32_t stride, int32_t pad);
int dls_conv_stem_kernel_choice(int64_t B, int32_t C, int32_t H, int32_t W, int32_t Cout, int32_t KH,
                                int32_t KW, int32_t stride, int32_t pad);
int dls_conv_pack_input_f32(const float *x, int64_t B, int32_t C, int32_t H, int32_t W, int32_t Cp,
                            uint16_t *out, dls_stream_t stream);
int dls_conv_pack_weights_f32(const float *w, int32_t Cout, int32_t Cin, int32_t KH, int32_t KW,
                              int32_t Cp, uint16_t *out, dls_stream_t stream);
int dls_conv_pack_im2col_f32(const float *x, int64_t B, int32_t C, int32_t H, int32_t W, int32_t KH,
                             int32_t KW, int32_t stride, int32_t pad, int32_t Kp, uint16_t *out,
                             dls_stream_t stream);
int dls_conv_pack_weights_im2col_f32(const float *w, int32_t Cout, int32_t Cin, int32_t KH, int32_t KW,
                                     int32_t Kp, uint16_t *out, dls_stream_t stream);
int dls_conv_bn_act_split(const uint16_t *x, int64_t B, int32_t H, int32_t W, int32_t C,
                          const uint16_t *w, int32_t Cout, int32_t KH, int32_t KW, int32_t stride,
                          int32_t pad, const float *consts, const uint16_t *residual, int32_t relu,
                          uint16_t *y, dls_stream_t stream);
int dls_conv_stem_bn_act_f32(const float *x, int64_t B, int32_t C, int32_t H, int32_t W, const uint16_t *w,
                             int32_t Cout, int32_t KH, int32_t KW, int32_t stride, int32_t pad,
                             const float *consts, int32_t relu, uint16_t *y, dls_stream_t stream);
int dls_pool_linear_split(const uint16_t *x, int64_t B, int32_t HW, int32_t C, const float *weight,
                          const float *bias, int32_t O, float *out, dls_stream_t stream);

/* Batched deterministic LeNet-5 utility evaluation (the tester's model forward
 * and top-1 count behind servers/fed_server.py:26-32 for the reference's MNIST /
 * LeNet-5 example; csrc/lenet.hip): S models x B images in one launch.
 *   models  fp32 [S, ldm]     one LeNet-5 per row, read in place (a row of the
 *                             Shapley store's subset models, or one flat row)
 *   offsets int64 [10], HOST  element offset within a row of conv1.weight
 *                             [6,1,5,5], conv1.bias, conv2.weight [16,6,5,5],
 *                             conv2.bias, fc1.weight [120,400], fc1.bias,
 *                             fc2.weight [84,120], fc2.bias, fc3.weight [O,84],
 *                             fc3.bias (the flat layout's offsets); multiples of
 *                             4, every tensor inside ldm
 *   x       fp32 [B,1,32,32]  contiguous
 *   labels  int64 [B]         may be null when correct is null
 *   O       1..32             fc3's outputs
 *   logits  fp32 [S,B,O] or null
 *   correct int64 [S] or null correct[s] += #{b : argmax_o logits[s,b,:] ==
 *                             labels[b]} (accumulated; the caller zeroes it);
 *                             argmax as torch.argmax: the lowest index among
 *                             equal maxima, a NaN logit is a maximum
 * At least one output is non-null.  The function is the eval forward conv 5x5 ->
 * ReLU -> 2x2 max-pool (twice), flatten [c][y][x], fc1-ReLU-fc2-ReLU-fc3 with
 * biases, in fp32 (values, products, accumulation); every output's reduction
 * order is fixed by the layer shapes alone (not by B, S, ldm, the image's or
 * the model's position, the grid or the stream) and the count is an integer
 * atomic: the same bits in any process.  B == 0 returns 0 without a launch.
 * models, x and logits 16-byte aligned; ldm a multiple of 4.
 * Pinned by tests/test_gpu_lenet_exact.py against tests/lenet_ref.py (fp64):
 *  - accuracy: with u = 2^-24 and g(n) = n u / (1 - n u), a layer of reduction
 *    length K (25, 150, 400, 120, 84) adds at most g(K + 2) (sum |w| (|h| + e_in)
 *    + |b|) to the incoming error sum |w| e_in, h its fp64 input; ReLU and the
 *    pooling pass the error on (a window: the largest of its members'); every
 *    logit is within the bound this gives from e = 0 at the pixels.  Where every
 *    product and partial sum is representable (integer models below 2^24) the
 *    logits are the exact values bit for bit.
 *  - special values are IEEE's: 0 * inf = NaN.  ReLU keeps a NaN and gives +0 for
 *    -inf and -0; a pooling window with a NaN is NaN; in the count the first NaN
 *    logit is the argmax, before +inf, else the lowest index among equal maxima
 *    (a row of -inf: index 0).
 *  - isolation: a NaN or inf pixel reaches that image's logits only, a NaN or inf
 *    parameter that model's logits and count only; the zero images that fill a
 *    ragged last tile, the zero weight rows past O and the padded k steps of conv2
 *    produce nothing that is stored, whatever they are multiplied with; elements
 *    of a row that no offset names and the row pitch's padding are never read.
 *  - subnormals are kept (inputs, products, sums and results), in the VALU chains
 *    of conv1 and in the MFMA layers alike, as observed on gfx950. */
int dls_lenet5_eval_f32(const float *models, int64_t ldm, int32_t S, const int64_t *offsets,
                        const float *x, int64_t B, const int64_t *labels, int32_t O,
                        float *logits, int64_t *correct, dls_stream_t stream);

/* Deterministic loss utilities (the tester's mean cross-entropy, get_metric(model,
 * "loss"), servers/fed_server.py:26-32; csrc/loss.hip, csrc/loss_common.h).
 * The per-image loss of both kernels is one function, in fp32 and index order:
 *   m = max_o z[o] (a NaN is a maximum), s = sum_o expf(z[o] - m) for o ascending,
 *   loss = (m - z[label]) + logf(s)
 * with the device library's expf / logf, computed by one lane per image; a label
 * outside [0, O) gives NaN and reads nothing.
 * dls_softmax_ce_f32: loss[s*ldn + b] of logits fp32 [S, B, O] (contiguous, 16-byte
 * aligned), labels int64 [B]; S >= 1, B >= 0 (0: no launch), O >= 1, ldn >= B. */
int dls_softmax_ce_f32(const float *logits, int32_t S, int64_t B, int32_t O, const int64_t *labels,
                       float *loss, int64_t ldn, dls_stream_t stream);
/* dls_lenet5_eval_f32 with a third optional output (servers/fed_server.py:26-32, the
 * loss metric): loss fp32, loss[s*ldn + b] = the cross-entropy above of
 * logits[s,b,:] and labels[b], ldn >= B, stored by the launch that computes the
 * logits (the same bits as dls_softmax_ce_f32 of them).  At least one of logits,
 * correct, loss is non-null; labels is needed for correct and for loss.  logits
 * and correct are the bits dls_lenet5_eval_f32 gives, under the same pinned
 * contract (bound, special values, isolation, subnormals): the tests launch every
 * case through both entry points. */
int dls_lenet5_eval_loss_f32(const float *models, int64_t ldm, int32_t S, const int64_t *offsets,
                             const float *x, int64_t B, const int64_t *labels, int32_t O,
                             float *logits, int64_t *correct, float *loss, int64_t ldn,
                             dls_stream_t stream);
/* The sum the mean loss of servers/fed_server.py:26-32 divides by n:
 * out[s] = sum_{i<n} (double) v[s*ldn + i], S >= 1 rows, n >= 0 (0: out[s] = 0.0),
 * ldn >= n, out fp64 [S].  One block of 256 threads per row: thread t adds
 * elements t, t + 256, ... in ascending order in fp64, then the 256 partials are
 * combined by a fixed pairwise tree: the order is a function of n alone (not of
 * S, ldn, the row or the stream), so the same values give the same bits. */
int dls_sum_rows_f64(const float *v, int64_t ldn, int32_t S, int64_t n, double *out,
                     dls_stream_t stream);

/* Top-k sparsification with error feedback ("sparsified SGD with memory", Stich,
 * Cordonnier & Jaggi 2018; Aji & Heafield 2017; Lin et al. 2018; csrc/topk.hip).  The
 * reference simulator has no sparsifier, so there is no reference hook to cite: the
 * definitions below are this library's and tests/topk_ref.py restates them in numpy.
 *
 * The client's compressor.  All pointers are device memory the caller owns; nothing is
 * allocated and no pointer is kept.  In fp32, one rounding per operation:
 *   u[j]   = fl(fl(w[j] - base[j]) + e[j])          j in 0..P-1 (e: the residual, zero
 *                                                   before the first round)
 *   key[j] = bits(u[j]) & 0x7fffffff, compared as an unsigned integer: +x and -x tie,
 *            -0.0 ties with +0.0, infinities and NaNs carry the largest keys
 *   selected: exactly k coordinates, those with the k largest keys; among the
 *            coordinates whose key equals the k-th largest key the lowest indices win,
 *            so the selection is a function of u alone
 *   idx[0..k) the selected coordinates, strictly ascending; val[i] = u[idx[i]], the
 *            same bits (sign of zero included)
 *   e[j]   = +0.0 where j is selected, u[j] elsewhere (in place): for every j exactly
 *            one of the sent value and the new residual holds u[j] bit for bit
 *   stats[0] = k; stats[1] = #{j : u[j] is not finite} (the call completes with the
 *            outputs the key order defines; the caller decides)
 * Where the arithmetic gives NaN, u[j] is some NaN (the same one in val or e).
 * 1 <= k <= P < 2^31 (DLS_EINVAL); P a multiple of 4 and w, base, e, val, idx, workspace
 * 16-byte aligned (DLS_ELAYOUT); e must not overlap w or base (DLS_EINVAL); all checked
 * before any device call.  workspace: the number of bytes the query below returns for P
 * (negative: the status of a bad P); it may hold anything on entry.
 * One launch sequence on the stream (a memset and nine kernels: a radix select on the
 * key, digits of 11 + 10 + 10 bits, the threshold staying on the device, then a count
 * per 4096-coordinate chunk, a scan and an ordered write), five passes over P-sized
 * arrays, nothing synchronised inside the call.  Integer histogram counts use LDS and
 * global integer atomics (order-independent sums); every output position comes from
 * the scans; there are no floating-point atomics: the outputs do not depend on the
 * stream, the grid or the scheduling.
 * Launch shape: chunks of DLS_TOPK_CHUNK coordinates; the histogram passes run at most
 * DLS_TOPK_HIST_BLOCKS blocks, block b taking the chunks b, b + DLS_TOPK_HIST_BLOCKS,
 * ...; the scan is one block of DLS_TOPK_SCAN_BLOCK threads, each owning ceil(chunks /
 * DLS_TOPK_SCAN_BLOCK) consecutive chunks. */
#define DLS_TOPK_CHUNK 4096
#define DLS_TOPK_HIST_BLOCKS 2048
#define DLS_TOPK_SCAN_BLOCK 1024
int64_t dls_topk_workspace(int64_t P);
int dls_topk_compress_f32(const float *w, const float *base, float *e, int64_t P, int64_t k,
                          int32_t *idx, float *val, int32_t *stats, void *workspace,
                          dls_stream_t stream);
/* The server's side: FedAvg over sparse client updates, added to the model the clients
 * started from.  Client i, in the given order, holds the pairs idx / val[off[i] ..
 * off[i+1]) (off int64 [K+1], ascending); its indices are strictly ascending and lie in
 * 0..P-1; a segment may be empty (idx and val may both be null when all are).
 * weight[i] = fl32(n_i) and total = fl32(sum of the n_i), as dls_fedavg_f32 takes them.
 * Per coordinate c:
 *   no client sent c:  out[c] = base[c], the same bits (copied, so -0.0 survives)
 *   otherwise:         acc = the reference FedAvg chain (servers/fed_server.py:44-66)
 *                      over the clients that sent c, in client order: the first assigns
 *                      fl(fl(v * n_i) / N), the later ones add theirs with fp32 +;
 *                      out[c] = fl(base[c] + acc)
 * with the correctly rounded division of DLS_FEDAVG_EXACT.  K >= 1, 1 <= P < 2^31
 * (DLS_EINVAL); P a multiple of 4, base and out 16-byte aligned (DLS_ELAYOUT); out must
 * not overlap base (DLS_EINVAL).  An entry whose index falls outside the range its
 * position implies (indices not ascending) is skipped, never written out of bounds.
 * One launch; one wave per 2048 coordinates accumulates them in LDS, client after
 * client; no atomics: the same bits on every run and for any launch geometry. */
int dls_sparse_fedavg_f32(const float *base, const int32_t *idx, const float *val,
                          const int64_t *off, const float *weight, int32_t K, float total,
                          int64_t P, float *out, dls_stream_t stream);

/* The library's random stream and the DP-FedAvg step on it (csrc/dpnoise.hip).
 *
 * The stream is counter-based Philox4x32-10 (Salmon, Moraes, Dror & Shaw 2011):
 * multipliers 0xD2511F53 (on counter word 0) and 0xCD9E8D57 (on word 2), Weyl key
 * increments 0x9E3779B9 and 0xBB67AE85, ten rounds, the key bumped between rounds (the
 * Random123 known-answer vectors).  key = (seed & 0xffffffff, seed >> 32); counter =
 * (block & 0xffffffff, block >> 32, stream_id & 0xffffffff, stream_id >> 32) with
 * block = coordinate / 4; word coordinate % 4 of the block's output belongs to the
 * coordinate.  A value is a function of (seed, stream_id, coordinate) alone: never of
 * the launch shape, the CU count, the HIP stream, K, the vector width or the call it
 * is drawn in.  Two calls that share (seed, stream_id) draw the SAME values for the
 * same coordinates: callers give every use a stream_id of its own (FedServer: the
 * round number).
 *   uniform of a word w:  u = ((w >> 9) + 0.5) * 2^-23, exact in fp32, in
 *                         [2^-24, 1 - 2^-24]: never 0 and never 1
 *   normals (Box-Muller): words 0, 1 of a block give coordinates 4b, 4b+1 and words
 *                         2, 3 give 4b+2, 4b+3.  Of a word pair (a, b):
 *                           r = sqrtf(fl(-2 * logf(u_a)))
 *                           g_even = fl(r * cospif(fl(2 * u_b)))
 *                           g_odd  = fl(r * sinpif(fl(2 * u_b)))
 *                         2 * u_b and -2 * logf are exact, the square root is correctly
 *                         rounded, every operation is rounded once and none is fused
 *                         (-ffp-contract=off); logf, cospif and sinpif are the device
 *                         math library's, so the normals are defined up to its error:
 *                         |g - exact| <= (e_log / 2 + e_trig + 1.5) * 2^-23 * r with
 *                         e_log and e_trig the functions' errors in ulp (DESIGN.md has
 *                         the measured values).
 * The tail is truncated: u_a >= 2^-24 gives |g| <= sqrt(48 ln 2) ~ 5.768, which the
 * standard normal exceeds with probability 8e-9.
 *
 *   dls_philox_u32:          out[i] = the word of coordinate first + i, i < n; exact.
 *   dls_philox_normal_f32:   out[i] = the normal of coordinate first + i.
 *   dls_normal_from_bits_f32: out[2j], out[2j+1] = (g_even, g_odd) of the word pair
 *                            (bits[2j], bits[2j+1]), j < n / 2: the transform alone, on
 *                            words the caller chooses.  out may be bits itself.
 * out and bits are device arrays of n 4-byte elements, 4-byte aligned (DLS_ELAYOUT
 * otherwise); first >= 0, n >= 0, first + n <= 2^63 - 1, n even for
 * dls_normal_from_bits_f32, no null pointer (DLS_EINVAL otherwise).  Every check runs
 * before any device call; n == 0 launches nothing.  The bits of
 * dls_philox_normal_f32 are those of dls_normal_from_bits_f32 on the words of
 * dls_philox_u32 for any first and n (an odd first or n included: the pairing is by
 * coordinate, not by position in out).
 *
 * dls_dp_clip_noise_step_f32: one step of client-level DP-FedAvg (McMahan, Ramage,
 * Talwar & Zhang 2018): the clipped mean of dls_centered_clip_step_f32 and Gaussian
 * noise, in one read of the rows.  Operands, layout rules (P and ldu multiples of 4,
 * ldu >= P, U and z 16-byte aligned, c 4-byte aligned: DLS_ELAYOUT), the range of K
 * and the order of the checks are those of dls_centered_clip_step_f32; there is no
 * dist2 and no workspace.  sigma must be finite and >= 0 (DLS_EINVAL; checked after K,
 * before the layout).  Per coordinate p, in the order of `rows`, every operation
 * rounded once and never fused:
 *   d_k = fl32(U[rows[k]][p] - z[p]);  t_k = fl32(c[k] * d_k);  acc = t_0;
 *   acc = fl32(acc + t_k) for k = 1 .. K-1;  y = fl32(z[p] + acc)
 * (the bits of the clip step), then
 *   z'[p] = fl32(y + fl32(sigma * g_p)),  g_p the normal of coordinate p.
 * sigma == 0 draws nothing and stores y itself: z' then equals the clip step's bit
 * for bit, the sign of a zero included.  Given dls_philox_normal_f32's g, numpy float32
 * reproduces z' bit for bit wherever it is not NaN.  z' does not depend on ldu, on the
 * rows' position in U, on the HIP stream or on the CU count.  A row that holds an inf
 * or NaN poisons its coordinate even with c[k] = 0.  A failed check leaves z untouched;
 * P == 0 launches nothing.  Traffic: K rows and z read once, z written once:
 * (K + 2) * P * 4 bytes. */
int dls_philox_u32(uint32_t *out, int64_t n, uint64_t seed, uint64_t stream_id, int64_t first,
                   dls_stream_t stream);
int dls_philox_normal_f32(float *out, int64_t n, uint64_t seed, uint64_t stream_id,
                          int64_t first, dls_stream_t stream);
int dls_normal_from_bits_f32(const uint32_t *bits, int64_t n, float *out, dls_stream_t stream);
int dls_dp_clip_noise_step_f32(const float *U, int64_t ldu, const int32_t *rows, int32_t K,
                               const float *c, int64_t P, float *z, float sigma, uint64_t seed,
                               uint64_t stream_id, dls_stream_t stream);

/* Secure aggregation in the ring Z_2^32 on pairwise masks drawn from the stream above
 * (csrc/secagg.hip; Bonawitz et al. 2017, "Practical Secure Aggregation for
 * Privacy-Preserving Machine Learning").  The mask word m_t[p] of stream id t and
 * coordinate p is dls_philox_u32's word under (seed, t, p); every sum below is mod 2^32.
 * Both calls are exact: numpy reproduces them bit for bit, for any launch shape, HIP
 * stream, CU count, ldy and position of the rows in Y.
 *
 * dls_secagg_mask_f32: the client's fused encode + mask.  With L = 2^(bits-1) - 1, per
 * coordinate p, every fp32 operation rounded once:
 *   d = fl32(w[p] - base[p]);  r = rintf(fl32(d * 2^frac_bits)), ties to even
 *   q = clamp(r, -L, L) as int32; a d that is not finite (inf, NaN) gives q = 0
 *   y[p] = (uint32)q * weight + sum_{t in add_streams} m_t[p] - sum_{t in sub_streams} m_t[p]
 *   stats[0] += #{p : d finite and |r| > L} (saturated; an overflowed product counts)
 *   stats[1] += #{p : d not finite}
 * stats is ADDED to (int32 [2], device; integer atomics: an order-independent sum), so a
 * caller zeroes it once and may mask several pieces into it.
 *
 * dls_secagg_unmask_f32: the server's fused sum + mask recovery + decode over the K rows
 * Y[rows[k] * ldy ..] (uint32, rows device int32 [K]):
 *   S[p] = sum_k Y[rows[k]][p] + sum_{t in add_streams} m_t[p] - sum_{t in sub_streams} m_t[p]
 *   v = (int32)S[p], two's complement
 *   delta = (float)(((double)v * 2^-frac_bits) / total): the product is exact, the IEEE
 *           fp64 division rounds once and the cast to fp32 rounds once (to nearest even)
 *   out[p] = fl32(base[p] + delta);  sum_out[p] = S[p] when sum_out is not null
 * Nothing in the decode is fused, reassociated or approximated.  out may be base itself.
 *
 * Checks, each before any device call, in this order: no null pointer (sum_out may be
 * null; the stream tables come below) and, for unmask, 1 <= K <= DLS_ROBUST_MAX_K; for mask
 * 2 <= bits <= 31 and weight >= 1; 0 <= frac_bits <= 126; n_add, n_sub >= 0 and n_add +
 * n_sub <= DLS_SECAGG_MAX_STREAMS (64 self masks plus the worst survivor x dropped product,
 * 32 * 32); a stream table is null only when its count is 0; for unmask total finite and
 * >= 1 (DLS_EINVAL); then P >= 0 (DLS_EINVAL), P and ldy multiples of 4, ldy >= P, w, base, y,
 * Y, out and sum_out 16-byte aligned, the stream tables 8-byte and rows / stats 4-byte
 * aligned (DLS_ELAYOUT).  A failed check leaves the outputs untouched; P == 0 launches
 * nothing.  The stream tables are device arrays of uint64.  y must not overlap w or base,
 * out and sum_out must not overlap Y or each other (preconditions).
 * Launch shape: one launch each; 256-thread blocks, a lane owns four consecutive
 * coordinates (one Philox block), tile n of 256 coordinates belongs to wave n % nW with
 * nW <= 2048 a function of P alone; no LDS, no floating-point atomics.  Traffic: mask
 * 3 * P * 4 bytes and (n_add + n_sub) / 4 Philox blocks per coordinate; unmask (K + 2) * P
 * * 4 bytes (+ P * 4 with sum_out) and as many blocks. */
#define DLS_SECAGG_MAX_STREAMS 1088
int dls_secagg_mask_f32(const float *w, const float *base, int64_t P, int32_t frac_bits,
                        int32_t bits, uint32_t weight, const uint64_t *add_streams, int32_t n_add,
                        const uint64_t *sub_streams, int32_t n_sub, uint64_t seed, uint32_t *y,
                        int32_t *stats, dls_stream_t stream);
int dls_secagg_unmask_f32(const uint32_t *Y, int64_t ldy, const int32_t *rows, int32_t K,
                          const uint64_t *add_streams, int32_t n_add, const uint64_t *sub_streams,
                          int32_t n_sub, uint64_t seed, const float *base, int32_t frac_bits,
                          double total, int64_t P, float *out, uint32_t *sum_out,
                          dls_stream_t stream);

/* Scaled-sign compression with error feedback (Karimireddy, Rebjock, Stich & Jaggi 2019,
 * "Error feedback fixes SignSGD"; the compressor of 1-bit SGD / 1-bit Adam;
 * csrc/efsign.hip): one bit per coordinate and one fp32 scale per tensor.  The reference
 * simulator has no such compressor: the definitions below are this library's and
 * tests/efsign_ref.py restates them in numpy.
 *
 * Segments.  The row of P coordinates (the flat parameter layout) holds T tensors; tensor
 * t occupies [bounds[t], bounds[t+1]), bounds int64 [T+1] on the device, bounds[0] = 0,
 * bounds[T] = P, ascending, every entry a multiple of 64; count int64 [T] on the device, 1
 * <= count[t] <= bounds[t+1] - bounds[t], is its number of real elements: the slots at or
 * beyond bounds[t] + count[t] are padding.  A 64-coordinate word never straddles two
 * tensors.  Malformed segments are DLS_EINVAL, but who checks is split: the two arrays live
 * on the device, so the library checks what it can see (P, T, the pointers) and the
 * binding (_native.efsign_segments) checks the arrays' contents on the host before it
 * uploads them.  With arrays that break the rules the kernels still read and write inside
 * the row and the workspace; what they compute is then unspecified.
 *
 * The client's compressor.  In fp32, one rounding per operation:
 *   u[j]   = fl(fl(w[j] - base[j]) + e[j]) for a real j, as in dls_topk_compress_f32
 *   s[t]   = fl32(L1_t / count[t]): L1_t the fp64 sum of |u[j]| over the real j of tensor
 *            t, the division in fp64, the quotient rounded once to fp32; scales[t] = s[t]
 *   bit j % 64 of bits[j / 64] = 1 iff u[j] < 0 (a comparison: -0.0, +0.0 and NaN give 0);
 *            padding slots give 0
 *   e[j]   = fl(u[j] - s[t]) where the bit is 0, fl(u[j] + s[t]) where it is 1, in place;
 *            padding slots of e are written +0.0
 *   stats[0] = #{real j : u[j] not finite} (int32 [1]; the call completes, the caller
 *            decides; s[t], and with it e, of such a tensor are not finite)
 * The order of the sum L1_t is a function of count[t] alone: not of where the tensor sits
 * in the row, of T, the grid, the CU count or the stream.  Chunk c of a tensor is its real
 * elements c * DLS_EFSIGN_CHUNK .. ; of a chunk, thread i of 256 adds the elements 4 (256 v
 * + i) + k, v and then k ascending over 0..3, a wave's 64 sums are combined by the xor
 * butterfly (distances 32, 16, .., 1) and the four wave sums are added in wave order; a
 * tensor's chunk sums are added per lane l over the chunks l, l + 64, .. ascending and
 * combined by the same butterfly.  There are no floating-point atomics (the non-finite
 * counts meet in one integer atomic add).
 * No null pointer, 64 <= P < 2^31 (DLS_EINVAL); P a multiple of 64 (DLS_ELAYOUT); 1 <= T <=
 * P / 64 (DLS_EINVAL); every pointer 16-byte aligned (DLS_ELAYOUT); e must not overlap w or
 * base (DLS_EINVAL); all checked before any device call, in this order.  workspace: the bytes
 * dls_efsign_workspace(P, T) returns (negative: the status of a bad P or T); it may hold
 * anything on entry.  Four launches on the stream (the chunk plan, u and the chunk sums,
 * the scales, the bits and the residual); there is no grid cap: one block per chunk.
 * Nothing is allocated and nothing is synchronised inside the call.
 *
 * The server's side: FedAvg over K clients' bit rows, added to the model they started
 * from.  bits uint64 [K, ldb], ldb >= P / 64; scales fp32 [K, lds], lds >= T; weight[i] =
 * fl32(n_i) and total = fl32(sum of the n_i), as dls_fedavg_f32 takes them.  For a real
 * coordinate j of tensor t:
 *   c[i][t] = fl(fl(scales[i][t] * weight[i]) / total), the correctly rounded division
 *             of DLS_FEDAVG_EXACT
 *   acc     = the reference FedAvg chain (servers/fed_server.py:44-66) over the clients
 *             i = 0..K-1 in the given order: the first assigns +c or -c by its bit (-c
 *             is c with the sign bit flipped, so a zero scale gives -0.0), the later
 *             ones add theirs with fp32 +
 *   out[j]  = fl(base[j] + acc)
 * and out[j] = base[j], the same bits, on a padding slot.  K >= 1 without an upper limit
 * (clients are walked in tiles of DLS_EFSIGN_CLIENT_TILE), P and T as above (DLS_EINVAL);
 * ldb, lds and the 16-byte alignment of every pointer (DLS_ELAYOUT); out must not
 * overlap base (DLS_EINVAL); all checked before the launch.  One launch, no prologue, no
 * atomics: one lane walks a coordinate's chain, so the bits are the same for any launch
 * geometry.  Traffic: K / 8 + 8 bytes per coordinate. */
#define DLS_EFSIGN_CHUNK 4096
#define DLS_EFSIGN_CLIENT_TILE 64
int64_t dls_efsign_workspace(int64_t P, int64_t T);
int dls_efsign_compress_f32(const float *w, const float *base, float *e, int64_t P,
                            const int64_t *bounds, const int64_t *count, int32_t T,
                            uint64_t *bits, float *scales, int32_t *stats, void *workspace,
                            dls_stream_t stream);
int dls_efsign_fedavg_f32(const float *base, const uint64_t *bits, int64_t ldb,
                          const float *scales, int64_t lds, const int64_t *bounds,
                          const int64_t *count, int32_t T, const float *weight, float total,
                          int32_t K, int64_t P, float *out, dls_stream_t stream);

/* Rotated one-bit compression (csrc/drive.hip): a public random rotation shared by all
 * clients of a round (Suresh, Yu, Kumar & McMahan 2017, "Distributed mean estimation with
 * limited communication") and the scale that makes the one-bit estimate unbiased (Vargaftik
 * et al. 2021, "DRIVE: one-bit distributed mean estimation").  No client state: nothing is
 * kept from round to round.  The reference simulator has no such compressor: the definitions
 * below are this library's and tests/drive_ref.py restates them in numpy.
 *
 * The rotation.  A row of P coordinates, 64 <= P < 2^31, P a multiple of 64, is cut into NB =
 * ceil(P / DLS_DRIVE_BLOCK) blocks of D = DLS_DRIVE_BLOCK = 4096 coordinates, Pd = D * NB
 * rotated coordinates in all; a coordinate j >= P reads as +0.0 and is never written.
 *   sigma[j] = -1 where bit j % 32 of dls_philox_u32's word of coordinate j / 32 under (seed,
 *              stream_id) is set, else +1; applying it flips the sign bit (exact, also for
 *              zeros, inf and NaN)
 *   H        per block, the stages h = 1, 2, 4, .., 2048 in ascending order: every pair (i,
 *              i + h) of the block with i & h == 0 becomes (fl32(a + b), fl32(a - b)); then
 *              one fl32(2^-6 * x).  Every operation is rounded once and none is fused, so a
 *              result is a function of the block's 4096 inputs alone
 *   forward  y = 2^-6 H(sigma * x) per block;  inverse  x = sigma * 2^-6 H(y)
 * dls_hadamard_rotate_f32: inverse == 0 reads x[0, P) and writes out[0, Pd); inverse == 1
 * reads x[0, Pd) and writes out[0, P).  out must not overlap x.
 *
 * dls_drive_compress_f32, the client's side: u[j] = fl32(w[j] - base[j]), y the forward
 * rotation of u.
 *   bits    uint64 [Pd / 64]: bit j % 64 of word j / 64 is y[j] < 0 (a comparison: -0.0 and
 *           NaN give 0); all Pd bits carry information, those of the last block past P too
 *   scales  fp32 [NB]: with the fp64 sums sq = sum (double)y[j]^2 and l1 = sum |(double)y[j]|
 *           over the block's 4096 rotated coordinates, DLS_DRIVE_UNBIASED: (float)(sq / l1),
 *           DLS_DRIVE_MSE: (float)(l1 / 4096.0); l1 == 0 gives +0.0 in both.  The order of the
 *           sums depends on j alone: the thread that holds the coordinates 1024 v + 64 r + l of
 *           the block (v the wave, l the lane) adds them over r = 0..15 ascending, a wave's 64
 *           sums are combined by the xor butterfly (distances 32, 16, .., 1) and the four
 *           wave sums are added in wave order
 *   stats   int32 [1]: stats[0] is set, not added to, to #{j < P : u[j] not finite} (the call
 *           completes, the caller decides; the scales of such a block are not finite)
 * One launch, no workspace, no floating-point atomics.  Traffic: 8 P + P / 8 bytes.
 *
 * dls_drive_fedavg_f32, the server's side: FedAvg over K clients' bit rows in the rotated
 * domain, rotated back once and added to the model the clients started from.  bits uint64 [K,
 * ldb], ldb >= Pd / 64; scales fp32 [K, lds], lds >= NB; weight[i] = fl32(n_i), total =
 * fl32(sum of the n_i).  Per block B:
 *   c[i]   = fl(fl(scales[i][B] * weight[i]) / total), the correctly rounded division of
 *            DLS_FEDAVG_EXACT
 *   z[j]   = the chain over the clients i = 0..K-1 in the given order of -c[i] where client
 *            i's bit j is set, else +c[i]: the first assigns, the later ones add with fp32 +
 *   v      = the inverse rotation of z;  out[j] = fl(base[j] + v[j]) for j < P
 * K >= 1 without an upper limit (clients are walked in tiles of DLS_DRIVE_CLIENT_TILE).  One
 * launch, no atomics: the same bits for any launch geometry, HIP stream or pitch.  out must
 * not overlap base.  Traffic: (K / 8 + 8) P bytes and 4 K NB of scales.
 *
 * Checks, each before any device call, in this order: no null pointer; inverse 0 or 1,
 * scale_mode one of the two, K >= 1; 64 <= P < 2^31 (DLS_EINVAL); P a multiple of 64, ldb and
 * lds, every pointer 16-byte aligned (DLS_ELAYOUT); the overlaps named above, and for the
 * compressor bits, scales and stats against w and base (DLS_EINVAL).  A failed check writes
 * nothing.  Nothing is synchronised inside a call; the compressor keeps one 64-bit word of device
 * memory per HIP stream, allocated when a stream first compresses. */
#define DLS_DRIVE_BLOCK 4096
#define DLS_DRIVE_CLIENT_TILE 64
#define DLS_DRIVE_UNBIASED 0
#define DLS_DRIVE_MSE 1
int dls_hadamard_rotate_f32(const float *x, int64_t P, uint64_t seed, uint64_t stream_id,
                            int32_t inverse, float *out, dls_stream_t stream);
int dls_drive_compress_f32(const float *w, const float *base, int64_t P, uint64_t seed,
                           uint64_t stream_id, int32_t scale_mode, uint64_t *bits, float *scales,
                           int32_t *stats, dls_stream_t stream);
int dls_drive_fedavg_f32(const float *base, const uint64_t *bits, int64_t ldb, const float *scales,
                         int64_t lds, const float *weight, float total, int32_t K, int64_t P,
                         uint64_t seed, uint64_t stream_id, float *out, dls_stream_t stream);

/* Multi-bit rotated compression (csrc/eden.hip; Vargaftik et al. 2022, "EDEN: communication-
 * efficient and robust distributed mean estimation for federated learning"), DRIVE's successor
 * at b = 2 or 4 bits per coordinate: after the rotation above a block's coordinates are close
 * to N(0, sigma^2), so every coordinate goes as the nearest level of the fixed Lloyd-Max
 * quantizer of N(0, 1) with 2^b levels, scaled by the block's root mean square, and one scale
 * per block makes the decode unbiased.  No client state.  The reference simulator has no such
 * compressor: the definitions below are this library's and tests/eden_ref.py restates them in
 * numpy.
 *
 * The codebook is symmetric with M = 2^(b-1) magnitudes: centroids cent_b[0] < .. < cent_b[M-1]
 * (DLS_EDEN_CENT2 / _CENT4) and boundaries bound_b[m] = (cent_b[m] + cent_b[m+1]) / 2, m < M - 1
 * (DLS_EDEN_BOUND2 / _BOUND4), every centroid the mean of |N(0, 1)| over its cell; the values
 * are tools/eden_tables.py's output, rounded to fp32.
 *
 * dls_eden_compress_f32, the client's side.  Operands, blocks, (seed, stream_id), sigma and the
 * rotation are dls_drive_compress_f32's: u[j] = fl32(w[j] - base[j]), y the forward rotation of
 * u.  Per block B of 4096 rotated coordinates:
 *   sq      = sum (double)y[j]^2 in the order dls_drive_compress_f32 documents (a thread over r
 *             = 0..15 ascending, the xor butterfly 32..1, the four waves in order); so are dot
 *             and qq below
 *   rms     = (float)sqrt(sq / 4096.0), the square root in fp64;  thr[m] = fl32(bound_b[m] * rms)
 *   m_j     = #{m : |y[j]| > thr[m]}: a tie takes the lower cell, a NaN compares false
 *             everywhere and gives 0;  neg_j = (y[j] < 0), as in drive
 *   f_j     = m_j | neg_j << (b-1), the coordinate's field
 *   dot     = sum |(double)y[j]| * (double)cent_b[m_j] (each product exact in fp64),
 *   qq      = sum (double)cent_b[m_j]^2
 *   scales  fp32 [NB]: DLS_EDEN_UNBIASED: (float)(sq / dot), DLS_EDEN_MSE: (float)(dot / qq);
 *           dot == 0 gives +0.0 in both
 *   codes   uint32 [NB * 128 * b]: a word holds fpw = 32 / b fields.  With v = j >> 10, r = (j >>
 *           6) & 15, l = j & 63 of the block's coordinate j, its field sits at bit (r % fpw) * b
 *           of word B * 128 * b + (v * (b / 2) + r / fpw) * 64 + l: the thread of the rotation
 *           that owns the coordinates (v, l) packs its own 16 fields and a wave stores
 *           contiguous words.  All Pd fields carry information
 *   stats   int32 [1]: stats[0] is set, not added to, to #{j < P : u[j] not finite}, through
 *           dls_drive_compress_f32's per-stream word
 * One launch, no workspace, no floating-point atomics.  Traffic: 8 P + b P / 8 bytes.
 *
 * dls_eden_fedavg_f32, the server's side: FedAvg over K clients' code rows in the rotated
 * domain, rotated back once and added to the model the clients started from.  codes uint32 [K,
 * ldc], ldc >= NB * 128 * b; scales fp32 [K, lds], lds >= NB; weight[i] = fl32(n_i), total =
 * fl32(sum of the n_i).  Per block B:
 *   c[i]    = fl(fl(scales[i][B] * weight[i]) / total), the correctly rounded division of
 *             DLS_FEDAVG_EXACT
 *   t[i][f] = fl(c[i] * cent_b[f & (M-1)]), with the sign bit set where f has bit b-1
 *   z[j]    = the chain over the clients i = 0..K-1 in the given order of t[i][f_ij]: the first
 *             assigns, the later ones add with fp32 +
 *   v       = the inverse rotation of z;  out[j] = fl(base[j] + v[j]) for j < P
 * K >= 1 without an upper limit (clients are walked in tiles of DLS_EDEN_CLIENT_TILE).  One
 * launch, no atomics: the same bits for any launch geometry, HIP stream or pitch.  out must
 * not overlap base.  Traffic: (K b / 8 + 8) P bytes and 4 K NB of scales.
 *
 * Checks, each before any device call, in this order: no null pointer; bits 2 or 4, scale_mode
 * one of the two, K >= 1; 64 <= P < 2^31 (DLS_EINVAL); P a multiple of 64, ldc and lds, every
 * pointer 16-byte aligned (DLS_ELAYOUT); out against base, and for the compressor codes, scales
 * and stats against w and base (DLS_EINVAL).  A failed check writes nothing.  Nothing is
 * synchronised inside a call. */
#define DLS_EDEN_CLIENT_TILE 64
#define DLS_EDEN_UNBIASED 0
#define DLS_EDEN_MSE 1
#define DLS_EDEN_CENT2 {0x1.cfa592p-2f, 0x1.82aabap+0f}
#define DLS_EDEN_BOUND2 {0x1.f6941ep-1f}
#define DLS_EDEN_CENT4 {0x1.06f3fap-3f, 0x1.8d5c88p-2f, 0x1.5042bcp-1f, 0x1.e27a72p-1f, 0x1.41985ep+0f, 0x1.9e384ap+0f, 0x1.08d58ep+1f, 0x1.5dc57ep+1f}
#define DLS_EDEN_BOUND4 {0x1.086b42p-2f, 0x1.0b788p-1f, 0x1.995e96p-1f, 0x1.196accp+0f, 0x1.6fe854p+0f, 0x1.d7f1b4p+0f, 0x1.334d86p+1f}
int dls_eden_compress_f32(const float *w, const float *base, int64_t P, int32_t bits, uint64_t seed,
                          uint64_t stream_id, int32_t scale_mode, uint32_t *codes, float *scales,
                          int32_t *stats, dls_stream_t stream);
int dls_eden_fedavg_f32(const float *base, const uint32_t *codes, int64_t ldc, const float *scales,
                        int64_t lds, const float *weight, float total, int32_t K, int64_t P,
                        int32_t bits, uint64_t seed, uint64_t stream_id, float *out,
                        dls_stream_t stream);

/* Stochastic quantization (csrc/qsgd.hip; Alistarh et al. 2017, "QSGD: communication-efficient
 * SGD via gradient quantization and encoding"; Wen et al. 2017, "TernGrad", its one-level
 * max-norm case): an unbiased quantizer without client state and without anything the clients
 * share.  Per bucket of coordinates the norm goes in fp32 and every coordinate as a signed level
 * in -s .. s, rounded up or down at random so that the decode q * d is right in expectation.
 * The reference simulator has no such compressor: the definitions below are this library's and
 * tests/qsgd_ref.py restates them in numpy.
 *
 * Shape.  bits b in {2, 4, 8}; s = 2^(b-1) - 1 levels (1: ternary, 7, 127).  A row of P
 * coordinates, 64 <= P < 2^31, P a multiple of 64, is cut into NB = ceil(P / DLS_QSGD_BUCKET)
 * buckets of 512; a coordinate j >= P reads as +0.0, is coded 0 and is never written by the
 * server.  Every fp32 operation below is rounded once and none is fused.
 *
 * dls_qsgd_compress_f32, the client's side: u[j] = fl(w[j] - base[j]).  Per bucket B the norm n:
 *   DLS_QSGD_MAX  n = max |u[j]|, taken on the bit patterns of |u| as unsigned integers (exact
 *                 in any order; a NaN in the bucket makes n a NaN, else an inf makes it inf)
 *   DLS_QSGD_L2   n = (float)sqrt(S), S the fp64 sum of (double)u[j]^2 in an order that depends
 *                 on j alone: lane l of 64 adds the squares of the bucket's coordinates 8 l ..
 *                 8 l + 7 ascending, the 64 sums meet in the xor butterfly (distances 32, 16,
 *                 .., 1), and the square root is taken in fp64, correctly rounded
 *   r = fl((float)s / n), d = fl(n / (float)s), both correctly rounded;  scales[B] = d
 *   n == 0 or n not finite: all codes of the bucket are 0 and scales[B] = d as computed (+0.0
 *   or not finite).  Otherwise per coordinate
 *     a = |u[j]|, t = fl(a * r), l0 = floor(t), f = t - l0 (exact)
 *     xi = (word_j >> 8) * 2^-24, word_j dls_philox_u32's word of coordinate j under (seed,
 *          stream_id)
 *     l  = l0 + (xi < f), then s where l < s does not hold (so also where r overflowed to inf,
 *          n < s / FLT_MAX: every coordinate of such a bucket is coded +-s, decoded +-n)
 *     q  = -l where u[j] < 0 (a comparison: -0.0 and NaN give +l), else l
 *   xi takes the 2^24 values k 2^-24 and ceil(f 2^24) of them lie below f: a level is rounded
 *   up with probability f rounded up to the 2^-24 grid, not f itself (f == 0 never rounds up),
 *   and the decode's expectation exceeds |u| by less than 2^-24 d.
 *   codes   uint32 [NB * 16 * b]: the field of coordinate j is q & (2^b - 1) (two's complement;
 *           -2^(b-1) never occurs) at bit (j % (32 / b)) * b of word j / (32 / b); all words of
 *           the last bucket are written
 *   stats   int32 [1]: stats[0] is set, not added to, to #{j < P : u[j] not finite} (the call
 *           completes, the caller decides), through dls_drive_compress_f32's per-stream word
 * One launch, no workspace, no floating-point atomics.  Traffic: 8 P + b P / 8 bytes.
 *
 * dls_qsgd_fedavg_f32, the server's side: FedAvg over K clients' code rows, added to the model
 * the clients started from.  codes uint32 [K, ldc], ldc >= NB * 16 * b and a multiple of 4 (every
 * row 16-byte aligned); scales fp32 [K, lds], lds >= NB; weight[i] = fl32(n_i), total =
 * fl32(sum of the n_i).  Per bucket B:
 *   c[i]   = fl(fl(scales[i][B] * weight[i]) / total), the correctly rounded division of
 *            DLS_FEDAVG_EXACT
 *   acc[j] = the chain over the clients i = 0..K-1 in the given order of p_i = fl((float)q_i *
 *            c[i]): the first assigns, the later ones add with fp32 +
 *   out[j] = fl(base[j] + acc[j]) for j < P
 * K >= 1 without an upper limit (clients are walked in tiles of DLS_QSGD_CLIENT_TILE).  One
 * launch, no atomics; one lane walks a coordinate's chain: the same bits for any launch
 * geometry, HIP stream or pitch.  out must not overlap base.  Traffic: (K b / 8 + 8) P bytes and
 * 4 K NB of scales.
 *
 * Checks, each before any device call, in this order: no null pointer; bits in {2, 4, 8}, norm
 * one of the two, K >= 1, 64 <= P < 2^31 (DLS_EINVAL); P a multiple of 64, ldc and lds, every
 * pointer 16-byte aligned (DLS_ELAYOUT); out against base, and for the compressor codes, scales
 * and stats against w and base (DLS_EINVAL).  A failed check writes nothing.  Nothing is
 * synchronised inside a call. */
#define DLS_QSGD_BUCKET 512
#define DLS_QSGD_CLIENT_TILE 64
#define DLS_QSGD_MAX 0
#define DLS_QSGD_L2 1
int dls_qsgd_compress_f32(const float *w, const float *base, int64_t P, int32_t bits, int32_t norm,
                          uint64_t seed, uint64_t stream_id, uint32_t *codes, float *scales,
                          int32_t *stats, dls_stream_t stream);
int dls_qsgd_fedavg_f32(const float *base, const uint32_t *codes, int64_t ldc, const float *scales,
                        int64_t lds, const float *weight, float total, int32_t K, int64_t P,
                        int32_t bits, float *out, dls_stream_t stream);

/* OCP Microscaling (MX) update compression (csrc/mx.hip; Rouhani et al. 2023, "Microscaling Data
 * Formats for Deep Learning"; the OCP MX v1.0 specification; Wang et al. 2024, "Towards Federated
 * Learning with On-device Training and Communication in 8-bit Floating Point"): a narrow
 * floating-point payload, one power-of-two scale per block of 32 coordinates.  The reference
 * simulator has no such compressor: the definitions below are this library's and
 * tests/mx_ref.py restates them in numpy.
 *
 * Element formats (OCP encodings: sign, exponent field, M mantissa bits, no infinities used):
 *   DLS_MX_E4M3  M = 3, bias 7,  emax 8,  fmax 448,   least normal 2^-6,  below it multiples of 2^-9
 *   DLS_MX_E5M2  M = 2, bias 15, emax 15, fmax 57344, least normal 2^-14, below it multiples of 2^-16
 *   DLS_MX_E2M1  M = 1, bias 1,  emax 2,  fmax 6,     the grid 0, 0.5, 1, 1.5, 2, 3, 4, 6
 * E4M3 and E5M2 take a byte per coordinate, E2M1 four bits.  The grid step q at a real t >= 0 is
 * 2^(max(floor(log2 t), emin) - M), emin the least normal's exponent.
 *
 * Shape.  A row of P coordinates, 64 <= P < 2^31, P a multiple of 64, is cut into blocks of
 * DLS_MX_BLOCK = 32 and groups of DLS_MX_GROUP = 512, NG = ceil(P / 512); a coordinate j >= P
 * reads as +0.0, is coded 0 and is never written by the server.  Every fp32 operation below is
 * rounded once and none is fused.
 *
 * dls_mx_compress_f32, the client's side.  u[j] = fl(w[j] - base[j]); with a residual r
 * (nullable: null means it is neither read nor written) u[j] = fl(fl(w[j] - base[j]) + r[j]).
 * Per block, with m the largest |u[j]| (taken on the bit patterns as unsigned integers):
 *   e     the least integer in [-127, 127] with m <= fmax 2^e: exponent field of m - 127 - emax,
 *         plus one where m's mantissa field exceeds fmax's, then -127 where that is less (every
 *         denormal m and m == 0).  Nothing saturates; the OCP floor rule, which would clamp
 *         (fmax, 2^(emax+1)) 2^e, is not used
 *   scale byte = e + 127 (E8M0), in 0 .. 254
 *   a block holding a NaN or an infinity: scale byte 255, all codes 0, dec = 0 below
 * Per coordinate t = |u[j]| 2^-e as a real number, l0 the grid point at or below t, q the step
 * there, f = (t - l0) / q in [0, 1):
 *   DLS_MX_NEAREST     up where f > 1/2, or f == 1/2 and l0's code is odd (ties to the even code)
 *   DLS_MX_STOCHASTIC  up exactly where xi < f as real numbers, xi = (word_j >> 8) 2^-24, word_j
 *                      dls_philox_u32's word of coordinate j under (seed, stream_id): the
 *                      convention of dls_qsgd_compress_f32.  f is exact, also where fp32 could
 *                      not hold it: any f in (0, 2^-24) rounds up exactly when xi == 0
 *   code  = sign bit of u[j] (also for zeros: -0.0 and a negative u rounded to zero give the
 *           negative zero code) above the magnitude's OCP encoding; seed and stream_id are not
 *           read under DLS_MX_NEAREST
 *   dec   = code 2^e, exact in fp32 (where |u| is within half a step of 2^128 it is +-inf)
 *   r'[j] = fl(u[j] - dec[j]) for j < P, written over r[j]; u[j] itself in a non-finite block
 * codes   uint32 [NG * 128] (8-bit formats: code j is byte j) or [NG * 64] (E2M1: code j is
 *         nibble j & 1 of byte j >> 1, the low nibble the even coordinate), little endian; all
 *         words of the last group are written
 * scales  uint8 [NG * 16], one byte per block, all bytes of the last group written (0 past P)
 * stats   int32 [1]: stats[0] is set, not added to, to #{j < P : u[j] not finite} (the call
 *         completes, the caller decides), through dls_drive_compress_f32's per-stream word
 * One launch, no workspace, no floating-point atomics.  Traffic: 8 P + b P / 8 + P / 32 bytes,
 * 8 P more with a residual.
 *
 * dls_mx_fedavg_f32, the server's side: FedAvg over K clients' code rows, added to the model the
 * clients started from.  codes uint32 [K, ldc], ldc in words, at least the row's and a multiple
 * of 4; scales uint8 [K, lds], lds in bytes, at least 16 NG and a multiple of 16; weight[i] =
 * fl32(n_i), total = fl32(sum of the n_i).
 *   c[i]   = fl(weight[i] / total), the correctly rounded division of DLS_FEDAVG_EXACT
 *   x_i[j] = code 2^e, exact
 *   acc[j] = the chain over the clients i = 0..K-1 in the given order of fl(x_i[j] * c[i]): the
 *            first assigns, the later ones add with fp32 +
 *   out[j] = fl(base[j] + acc[j]) for j < P
 * Outside the contract: scale byte 255 and the code patterns the compressor never emits (E4M3's
 * S.1111.111, E5M2's exponent field 31).  K >= 1 without an upper limit (clients are walked in
 * tiles of DLS_MX_CLIENT_TILE).  One launch, no atomics; one lane walks a coordinate's chain: the
 * same bits for any launch geometry, HIP stream or pitch.  out must not overlap base.  Traffic:
 * (K (b / 8 + 1 / 32) + 8) P bytes.
 *
 * Checks, each before any device call, in this order: no null pointer (but residual); format one
 * of the three, rounding one of the two, K >= 1, 64 <= P < 2^31 (DLS_EINVAL); P a multiple of 64,
 * ldc and lds, every pointer 16-byte aligned (DLS_ELAYOUT); out against base, and for the
 * compressor codes, scales and stats against w, base and residual, residual against w and base
 * (DLS_EINVAL).  A failed check writes nothing.  Nothing is synchronised inside a call. */
#define DLS_MX_BLOCK 32
#define DLS_MX_GROUP 512
#define DLS_MX_CLIENT_TILE 64
#define DLS_MX_E4M3 0
#define DLS_MX_E5M2 1
#define DLS_MX_E2M1 2
#define DLS_MX_NEAREST 0
#define DLS_MX_STOCHASTIC 1
int dls_mx_compress_f32(const float *w, const float *base, float *residual, int64_t P,
                        int32_t format, int32_t rounding, uint64_t seed, uint64_t stream_id,
                        uint32_t *codes, uint8_t *scales, int32_t *stats, dls_stream_t stream);
int dls_mx_fedavg_f32(const float *base, const uint32_t *codes, int64_t ldc, const uint8_t *scales,
                      int64_t lds, const float *weight, float total, int32_t K, int64_t P,
                      int32_t format, float *out, dls_stream_t stream);

/* FetchSGD's Count Sketch (csrc/sketch.hip; Rothchild et al. 2020, "FetchSGD: Communication-
 * Efficient Federated Learning with Sketching"): sparsification without client state.  A client
 * sends an R x C table, a linear function of its update, so the server averages tables, keeps
 * momentum and the error accumulation in sketch space, and reads a top-k out of the inverse.
 * The reference simulator has no such compressor: the definitions below are this library's and
 * tests/sketch_ref.py restates them in numpy.
 *
 * Shape.  R rows, R in {1, 3, 5, 7} (DLS_SKETCH_MAX_ROWS); C columns, a power of two, 1024 <= C
 * <= 2^24; a row of P coordinates, 4 <= P < 2^31, P a multiple of 4, in NQ = ceil(P / C) blocks
 * of C: coordinate j = q C + t lies in block q at offset t.  A coordinate j >= P contributes
 * +0.0 and no sign is applied to it.
 *   m_r(q)  = (dls_philox_u32's word of coordinate 8 q + r under (seed, stream_id)) & (C - 1)
 *   bucket  of coordinate j in row r: t ^ m_r(q).  Within a block the map is a bijection onto
 *           the C buckets; coordinates of different blocks collide with probability 1 / C,
 *           independently per row.  Bucket b of row r so receives exactly one coordinate per
 *           block, q C + (b ^ m_r(q)): the sketch is a gather
 *   s_r(j)  = -1 where bit j % 32 of the word of coordinate 2^32 + r 2^26 + j / 32 under (seed,
 *           stream_id) is set, else +1; applying it flips the sign bit (exact, also for zeros,
 *           inf and NaN)
 * (seed, stream_id) is a run's: the server's accumulators live in sketch space across rounds.
 *
 * dls_sketch_f32, the client's side: u[j] = fl32(w[j] - base[j]); base may be null, then u = w.
 *   table   fp32 [R, C]: T[r][b] = the fp32 sum over q of s_r(i) u[i], i = q C + (b ^ m_r(q)).
 *           The blocks are taken in segments of DLS_SKETCH_QSEG = 32: within a segment q
 *           ascends, the first term assigns and each later one is added with one fp32 +; the
 *           segment partials are then added in ascending segment order, the first assigning.
 *           Nothing is fused
 *   stats   int32 [1]: stats[0] is set, not added to, to #{j < P : u[j] not finite}, counted
 *           once and not per row (the call completes, the caller decides)
 *   workspace  the bytes dls_sketch_workspace(P, R, C) returns (negative: the status of a bad
 *           shape); it may hold anything on entry.  With fewer than 1024 tiles of 1024 buckets
 *           in the table, the segments are spread over workgroups and their partials go
 *           through it (a second launch adds them); otherwise one launch
 * No floating-point atomics: the bits depend on neither the grid, the HIP stream nor the CU
 * count.  The non-finite counts meet in dls_drive_compress_f32's per-stream word.  Traffic: the
 * row (and base) is read R times, R * 4 P (8 P) bytes, all but the first from cache where the
 * row fits one; R C 4 bytes written.
 *
 * dls_unsketch_f32, the server's side: for j < P, e_r = s_r(j) T[r][(j % C) ^ m_r(j / C)] and
 * est[j] = the median of e_0 .. e_{R-1} under the total order on bit patterns key(x) = b if b
 * >= 0 else b ^ 0x7fffffff (b the bits as int32; keys compared as signed integers): est[j] has
 * the bits of the element of middle rank.  So -0.0 < +0.0, NaNs sort to the ends by their
 * sign and up to (R - 1) / 2 of them are outvoted; the result is a function of the table
 * alone.  One launch; traffic 4 P bytes written and the table.
 *
 * Checks, each before any device call, in this order: no null pointer (base may be null); R, C
 * and P in range (DLS_EINVAL); P a multiple of 4 and every pointer 16-byte aligned
 * (DLS_ELAYOUT); table, stats and workspace overlap neither w or base nor each other, est does
 * not overlap table (DLS_EINVAL).  A failed check writes nothing.  Nothing is synchronised. */
#define DLS_SKETCH_MAX_ROWS 7
#define DLS_SKETCH_QSEG 32
int64_t dls_sketch_workspace(int64_t P, int32_t R, int64_t C);
int dls_sketch_f32(const float *w, const float *base, int64_t P, int32_t R, int64_t C,
                   uint64_t seed, uint64_t stream_id, float *table, int32_t *stats,
                   void *workspace, dls_stream_t stream);
int dls_unsketch_f32(const float *table, int64_t P, int32_t R, int64_t C, uint64_t seed,
                     uint64_t stream_id, float *est, dls_stream_t stream);

/* Low-rank update compression with error feedback (Vogels, Karimireddy & Jaggi 2019,
 * "PowerSGD: practical low-rank gradient compression"; csrc/powersgd.hip): one power-iteration
 * step per weight matrix on the client, each client on its own (no all-reduce of P), and the
 * FedAvg of the clients' factors on the server.  The reference simulator has no such
 * compressor: the definitions below are this library's and tests/powersgd_ref.py restates them
 * in numpy.
 *
 * Tensors.  A tensor of shape (d0, d1, ..) is seen as the row-major matrix n = d0, m = numel /
 * d0 (a vector: m = 1).  At rank r, 1 <= r <= DLS_POWERSGD_MAX_RANK, it is COMPRESSED iff r <=
 * min(n, m) and (n + m) r < n m, else DENSE (every vector is dense: m = 1 fails the second
 * test).  A payload (fp32 [L]) holds per tensor, in tensor order, every block starting at a
 * multiple of 64 floats and padded to one with +0.0: compressed, the block P^ [n][r] and then
 * the block Q [m][r], both row-major; dense, one block of the n m values.
 *
 * The plan.  int64 [T + 1][DLS_POWERSGD_PLAN_WORDS] on the device; row t: 0 the tensor's
 * offset in the row of P coordinates (a multiple of 64; row T holds P, so tensor t occupies
 * [off[t], off[t + 1]) and the slots from n m on are padding), 1 n, 2 m, 3 kind (1
 * compressed, 0 dense), 4 the offset of its P^ (or value) block in the payload, 5 of its Q
 * block, 6 the byte offset of its region of the workspace (compressed: 128 n + 64 n ceil(m /
 * DLS_POWERSGD_CHUNK) bytes, from dls_powersgd_workspace's first 16-byte multiple >= 4 (P / 16
 * + T) on), 7 / 8 / 9 the number of work items of the tensors before it in the compressor's
 * first pass (compressed: ceil(n / 16) ceil(m / DLS_POWERSGD_CHUNK); dense: ceil(extent /
 * 1024)), its last pass (ceil(m / 16); 0) and the server (ceil(n / 32) ceil(m / 64); ceil(
 * extent / 1024)); row T holds the totals.  The plan lives on the device, so who checks is
 * split as for dls_efsign_*: the binding (_native.powersgd_plan) builds and checks it on the
 * host; the library checks what it can see, and the kernels test every row against P, L and
 * the workspace size and skip a tensor that does not fit, so they never read or write outside
 * the arrays of the call; what they compute from a malformed plan is unspecified.
 *
 * The client, per compressed tensor (U the n x m view of u):
 *   u   = fl(fl(w - base) + e), as dls_topk_compress_f32 defines it (e == NULL: u = fl(w - base))
 *   P   = U Q0        Q0 fp32 [m][r], read from q0 at the tensor's Q block offset (q0 has the
 *                     payload's layout)
 *   P^  = the columns of P orthonormalised by modified Gram-Schmidt in column order 0..r-1:
 *         column q is divided by the square root of its squared norm and at once projected
 *         out of the columns after it.  A column whose squared norm is then 0 or not finite
 *         becomes an all-zero column of P^ and is projected out of nothing.
 *   Q   = U^T P^      [m][r]
 *   e   = fl(u - R), R = P^ Q^T, in place; padding slots of e are written +0.0
 * The payload gets P^ and Q.  For a dense tensor the payload gets w's values and e of the
 * tensor, padding included, is written +0.0.  stats[0] (int32) = #{real j : u[j] not finite},
 * dense tensors included; the call completes and the caller decides.  With e == NULL nothing
 * is written back.
 * Arithmetic.  Every matrix product runs on v_mfma_f32_16x16x4_f32: each entry is an fp32 fma
 * chain from +0.0, zero-padded to whole instructions (adding an exact zero rounds nothing):
 *   P: the m columns are cut into chunks of DLS_POWERSGD_CHUNK; a chunk's partial is one chain
 *      over its columns; the partials are added in chunk order in fp64.  L = min(m,
 *      DLS_POWERSGD_CHUNK), c = 1 (the fp64 sum's slack)
 *   Q: one chain over the n rows, ascending: L = n, c = 0
 *   R: one chain over q ascending: L = r; then e = fl(u - R), one more rounding
 * with, elementwise, |computed - exact| <= g sum |a| |b| over the contraction, g = (L + c) u /
 * (1 - (L + c) u), u = 2^-24 (each term passes through at most L roundings; products are not
 * rounded), while the values stay in the normal range.  Gram-Schmidt runs in fp64 on the
 * fp64 P: thread i of 256 adds its rows i, i + 256, .. ascending, a wave's 64 sums meet in the
 * xor butterfly (distances 32, .., 1), the four wave sums are added in wave order: the order
 * depends on n alone.  The normalised column is rounded to fp32 once, so P^T P^ = I within
 * 3 u elementwise while kappa_2(P) n 2^-53 stays far below u.  A rank-deficient P whose
 * deficiency is not exact in fp64 yields a normalised column of rounding noise, not zeros.
 * Where every product and partial sum is exactly representable every output is exact, bit
 * for bit.  No floating-point atomics and no dependence on the grid, the CU count, T or the
 * tensor's place in the row: work items are cut relative to the tensor's own start.
 *
 * The server: out = base + the FedAvg of K clients' payloads (fp32 [K, ldp]); weight[i] =
 * fl32(n_i) and total = fl32(sum of the n_i), as dls_fedavg_f32 takes them.
 *   compressed, real coordinate (a, b):  c_i = fl(weight[i] / total) (correctly rounded);
 *     A_i[a][q] = fl(c_i P^_i[a][q]); acc = one fma chain from +0.0 over A_i[a][q] Q_i[b][q],
 *     client i ascending, then q ascending; out = fl(base + acc).  Elementwise |out - (base +
 *     sum A Q)| <= g (|base| + sum |A| |Q|) with L = K r, c = 1.  Clients are walked in tiles
 *     of DLS_POWERSGD_CLIENT_TILE, a later tile continuing the chain from the fp32 value
 *     the tile before it left; K has no upper limit.
 *   dense, real coordinate: the reference FedAvg chain (servers/fed_server.py:44-66) of the K
 *     sent values: the bits dls_fedavg_f32 (DLS_FEDAVG_EXACT) gives on that slice; base plays
 *     no part.
 *   padding slots: base's bits.
 * One launch.  A non-finite factor entry makes the out coordinates of its row (P^) or column
 * (Q) of that tensor non-finite, and no others.
 *
 * Checks, each before any device call, in this order.  DLS_EINVAL: a null pointer (e may be
 * null); K >= 1; 64 <= P < 2^31; 1 <= T <= P / 64; 1 <= r <= DLS_POWERSGD_MAX_RANK; 64 <= L <
 * 2^31; the compressor's workspace_bytes at least 4 (P / 16 + T) rounded up to 16, the
 * server's total positive and finite; e overlapping w or base, payload overlapping q0, out
 * overlapping base.  DLS_ELAYOUT: P and L multiples of 64; ldp a multiple of 4 and >= L; every
 * pointer 16-byte aligned.  A failed check writes nothing.  Nothing is allocated or
 * synchronised inside a call.  The two size queries take the host array dims int64 [T][2] =
 * (n, m) per tensor and return the payload's floats and the workspace's bytes (negative: the
 * status of bad arguments; n, m >= 1 and n m < 2^31). */
#define DLS_POWERSGD_MAX_RANK 16
#define DLS_POWERSGD_CHUNK 256
#define DLS_POWERSGD_CLIENT_TILE 64
#define DLS_POWERSGD_PLAN_WORDS 10
int64_t dls_powersgd_payload_len(const int64_t *dims, int64_t T, int32_t r);
int64_t dls_powersgd_workspace(const int64_t *dims, int64_t T, int32_t r, int64_t P);
int dls_powersgd_compress_f32(const float *w, const float *base, float *e, int64_t P,
                              const int64_t *plan, int32_t T, int32_t r, const float *q0,
                              float *payload, int64_t L, int32_t *stats, void *workspace,
                              int64_t workspace_bytes, dls_stream_t stream);
int dls_powersgd_fedavg_f32(const float *base, const float *payloads, int64_t ldp, int64_t L,
                            const int64_t *plan, int32_t T, int32_t r, const float *weight,
                            float total, int32_t K, int64_t P, float *out, dls_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DLS_HIP_H */
