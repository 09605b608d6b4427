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

#ifdef __cplusplus
}
#endif
#endif /* DLS_HIP_H */
