// Deterministic loss utilities for gfx950 (the tester's mean cross-entropy,
// FedServer.get_metric(model, "loss"), servers/fed_server.py:26-32).
//
//   dls_softmax_ce_f32   one lane per (model, image): ce_row (loss_common.h) over
//                        the O logits of that row, stored per image.
//   dls_sum_rows_f64     one block of 256 threads per model: thread t adds the
//                        elements t, t + 256, ... of the row in ascending order in
//                        fp64, then the 256 partials meet in a fixed pairwise tree
//                        in LDS.  The order is a function of n alone.
//
// Losses are stored per image and summed once over the whole test set, so the
// sum does not depend on how the forward was chunked; nothing is combined in
// arrival order (no floating-point atomics).
#include "dls_common.h"
#include "loss_common.h"

namespace dls {
namespace {

constexpr int kThreads = 256;

__global__ __launch_bounds__(kThreads) void k_softmax_ce(const float *__restrict__ logits,
                                                         int64_t rows, int64_t B, int O,
                                                         const int64_t *__restrict__ labels,
                                                         float *__restrict__ loss, int64_t ldn) {
    const int64_t r = (int64_t)blockIdx.x * kThreads + threadIdx.x;  // r = s * B + b
    if (r >= rows) return;
    const int64_t s = r / B, b = r - s * B;
    loss[s * ldn + b] = ce_row(logits + r * O, 1, O, labels[b]);
}

__global__ __launch_bounds__(kThreads) void k_sum_rows_f64(const float *__restrict__ v,
                                                           int64_t ldn, int64_t n,
                                                           double *__restrict__ out) {
    __shared__ double part[kThreads];
    const int t = threadIdx.x;
    const float *row = v + (int64_t)blockIdx.x * ldn;
    double acc = 0.0;
    for (int64_t i = t; i < n; i += kThreads) acc += (double)row[i];
    part[t] = acc;
    __syncthreads();
    for (int half = kThreads / 2; half >= 1; half >>= 1) {
        if (t < half) part[t] += part[t + half];
        __syncthreads();
    }
    if (t == 0) out[blockIdx.x] = part[0];
}

}  // namespace
}  // namespace dls

using namespace dls;

extern "C" int dls_softmax_ce_f32(const float *logits, int32_t S, int64_t B, int32_t O,
                                  const int64_t *labels, float *loss, int64_t ldn,
                                  dls_stream_t stream) {
    DLS_REQUIRE(logits, DLS_EINVAL, "dls_softmax_ce_f32: null pointer: logits");
    DLS_REQUIRE(labels, DLS_EINVAL, "dls_softmax_ce_f32: null pointer: labels");
    DLS_REQUIRE(loss, DLS_EINVAL, "dls_softmax_ce_f32: null pointer: loss");
    DLS_REQUIRE(S >= 1, DLS_EINVAL, "dls_softmax_ce_f32: S=%d (at least 1)", S);
    DLS_REQUIRE(B >= 0, DLS_EINVAL, "dls_softmax_ce_f32: B=%lld (negative)", (long long)B);
    DLS_REQUIRE(O >= 1, DLS_EINVAL, "dls_softmax_ce_f32: O=%d (at least 1)", O);
    DLS_REQUIRE(ldn >= B, DLS_EINVAL, "dls_softmax_ce_f32: ldn=%lld is less than B=%lld",
                (long long)ldn, (long long)B);
    DLS_REQUIRE(B <= (((int64_t)1 << 31) - 1) * kThreads / S, DLS_EINVAL,
                "dls_softmax_ce_f32: S=%d x B=%lld exceeds one grid", S, (long long)B);
    DLS_REQUIRE(aligned16(logits), DLS_ELAYOUT, "dls_softmax_ce_f32: logits: 16-byte alignment");
    DLS_REQUIRE((reinterpret_cast<uintptr_t>(labels) & 7u) == 0, DLS_ELAYOUT,
                "dls_softmax_ce_f32: labels: 8-byte alignment");
    DLS_REQUIRE((reinterpret_cast<uintptr_t>(loss) & 3u) == 0, DLS_ELAYOUT,
                "dls_softmax_ce_f32: loss: 4-byte alignment");
    if (B == 0) return DLS_OK;
    const int64_t rows = (int64_t)S * B;
    hipLaunchKernelGGL(k_softmax_ce, dim3((unsigned)((rows + kThreads - 1) / kThreads)),
                       dim3(kThreads), 0, as_stream(stream), logits, rows, B, (int)O, labels, loss,
                       ldn);
    return check_launch("dls_softmax_ce_f32");
}

extern "C" int dls_sum_rows_f64(const float *v, int64_t ldn, int32_t S, int64_t n, double *out,
                                dls_stream_t stream) {
    DLS_REQUIRE(v, DLS_EINVAL, "dls_sum_rows_f64: null pointer: v");
    DLS_REQUIRE(out, DLS_EINVAL, "dls_sum_rows_f64: null pointer: out");
    DLS_REQUIRE(S >= 1, DLS_EINVAL, "dls_sum_rows_f64: S=%d (at least 1)", S);
    DLS_REQUIRE(n >= 0, DLS_EINVAL, "dls_sum_rows_f64: n=%lld (negative)", (long long)n);
    DLS_REQUIRE(ldn >= n, DLS_EINVAL, "dls_sum_rows_f64: ldn=%lld is less than n=%lld",
                (long long)ldn, (long long)n);
    DLS_REQUIRE((reinterpret_cast<uintptr_t>(v) & 3u) == 0, DLS_ELAYOUT,
                "dls_sum_rows_f64: v: 4-byte alignment");
    DLS_REQUIRE((reinterpret_cast<uintptr_t>(out) & 7u) == 0, DLS_ELAYOUT,
                "dls_sum_rows_f64: out: 8-byte alignment");
    // one block per row (S < 2^31: always one grid); n == 0 stores 0.0
    hipLaunchKernelGGL(k_sum_rows_f64, dim3((unsigned)S), dim3(kThreads), 0, as_stream(stream), v,
                       ldn, n, out);
    return check_launch("dls_sum_rows_f64");
}
