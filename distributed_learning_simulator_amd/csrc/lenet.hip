// Batched deterministic LeNet-5 utility evaluation for gfx950 (the Shapley
// servers' v(S) = top-1 accuracy of a coalition model on the test set,
// FedServer.get_metric, servers/fed_server.py:26-32, for the reference's own
// MNIST / LeNet-5 example).
//
// One launch scores S models, each one row of a flat-layout matrix (a row of the
// Shapley store's subset models, or one ParameterLayout.flatten of a module), on
// B images: a block takes one model and a tile of kT = 16 images and keeps every
// activation of the tile on chip; only the 4 KB input per image and the logits /
// the correct count touch HBM.
//
//   conv1 (K = 25, 6 channels)   VALU: a thread owns one pooled position of one
//                                image, its 6x6 input patch in registers, the
//                                2x2 conv outputs of all 6 channels as 24 fma
//                                chains over the taps in (ky, kx) order; weights
//                                are LDS broadcasts.
//   conv2 (K = 150, 16 channels) implicit GEMM on v_mfma_f32_16x16x4_f32: M = the
//                                16 output channels, N = 16 (image, pooled
//                                position) columns, one accumulator per member
//                                of the 2x2 pooling window so that the max is
//                                per lane; k = (ci, ky, kx) in weight order.
//   fc1 / fc2 / fc3              the same MFMA: M = 16 neurons, N = the tile's 16
//                                images, weights straight from L2 (fc1 alone is
//                                192 KB: it does not fit beside the tile), two
//                                accumulators (even / odd k steps) added once.
//
// fp32 values, fp32 products, fp32 accumulation.  Every output's reduction order
// is fixed by the layer shapes: an MFMA column (one image, or one image's pooled
// position) never sees another column's data, invalid images of a ragged tile
// are zero inputs whose results are dropped, and nothing is combined in arrival
// order.  The correct count is an integer atomic, one per block.  The loss
// instantiation (dls_lenet5_eval_loss_f32) adds one epilogue: a lane per image
// runs ce_row (loss_common.h) on the image's logits in LDS and stores the loss.
//
// LDS: pooled conv1 activations 16 x 1176 fp32 (73.5 KB; the fc activations
// alias them once conv2 is done), features 16 x 402, conv weights 10.5 KB:
// ~110 KB, one block of 4 waves per CU.
#include "dls_common.h"
#include "loss_common.h"

namespace dls {
namespace {

constexpr int kT = 16;          // images per block = the MFMA's N
constexpr int kThreads = 256;   // 4 waves
constexpr int kP1 = 6 * 14 * 14;  // pooled conv1 activations per image
constexpr int kK2 = 150;        // conv2 reduction length (6 x 5 x 5)
constexpr int kK2p = 152;       // ... padded to the MFMA's k = 4
// row pitches (floats) of the LDS activations: the MFMA's B operand reads
// [image = lane & 15][k0 + (lane >> 4)], conflict-free within a half wave when
// the pitch is 2 mod 16 with distinct multiples
constexpr int kFeatLd = 402, kH1Ld = 122, kH2Ld = 90, kLgLd = 33;
constexpr int kOMax = 32;

static_assert(kT * 25 % 16 == 0, "conv2 columns are whole MFMA tiles");
static_assert(kT * (kH1Ld + kH2Ld + kLgLd) <= kT * kP1, "fc activations alias p1");

struct LenetOffsets {
    int64_t o[10];
};

__device__ __forceinline__ float relu_nan(float t) {  // relu keeps NaN, as torch
    return t > 0.f ? t : (t == t ? 0.f : t);
}

__device__ __forceinline__ float max_nan(float a, float b) {  // max_pool2d keeps NaN, as torch
    return (a > b || a != a) ? a : b;
}

// out[img][j] = act(sum_k W[j][k] * in[img][k] + bias[j]) for the tile's 16 images:
// M tiles of 16 neurons dealt over the waves.  Lane (n = lane & 15, q = lane >> 4)
// supplies A = W[16 mt + n][k0 + q] (global; zero past J) and B = in[n][k0 + q]
// (LDS); D[row 4q + r][col n] is neuron 16 mt + 4q + r of image n.
template <int K>
__device__ __forceinline__ void fc_layer(const float *__restrict__ W, const float *__restrict__ bias,
                                         int J, const float *in, int ldin, float *out, int ldout,
                                         bool relu, int wave, int lane) {
    static_assert(K % 4 == 0, "whole k steps");
    const int n = lane & 15, q = lane >> 4;
    const float *ir = in + n * ldin + q;
    for (int mt = wave; mt * 16 < J; mt += kThreads / 64) {
        const int j = mt * 16 + n;
        const bool jv = j < J;
        const float *wr = W + (int64_t)(jv ? j : 0) * K + q;
        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
        int k0 = 0;
#pragma unroll 4
        for (; k0 + 8 <= K; k0 += 8) {
            const float a0 = jv ? wr[k0] : 0.f;
            const float a1 = jv ? wr[k0 + 4] : 0.f;
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, ir[k0], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, ir[k0 + 4], acc1, 0, 0, 0);
        }
        if (k0 < K) {  // K = 84: an odd number of k steps
            const float a0 = jv ? wr[k0] : 0.f;
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, ir[k0], acc0, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int jo = mt * 16 + 4 * q + r;
            if (jo < J) {
                float t = (acc0[r] + acc1[r]) + bias[jo];
                if (relu) t = relu_nan(t);
                out[n * ldout + jo] = t;
            }
        }
    }
}

// kLoss = false is the kernel dls_lenet5_eval_f32 launches: loss / ldn are unused
template <bool kLoss>
__global__ __launch_bounds__(kThreads) void k_lenet5_eval(
    const float *__restrict__ models, int64_t ldm, LenetOffsets off, const float *__restrict__ x,
    int64_t B, const int64_t *__restrict__ labels, int O, int tiles, float *__restrict__ logits,
    unsigned long long *__restrict__ correct, float *__restrict__ loss, int64_t ldn) {
    __shared__ __attribute__((aligned(16))) float p1[kT * kP1];
    __shared__ __attribute__((aligned(16))) float feat[kT * kFeatLd];
    __shared__ __attribute__((aligned(16))) float w2t[kK2p * 16];  // [k][co]
    __shared__ __attribute__((aligned(16))) float w1s[25 * 8];     // [tap][co, 6 -> 8]
    __shared__ float b1[8];
    __shared__ float b2[16];
    __shared__ int kofs[kK2p];  // k = (ci, ky, kx) -> offset in an image's p1
    float *h1 = p1, *h2 = p1 + kT * kH1Ld, *lg = h2 + kT * kH2Ld;  // live after conv2 only

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int s = (int)(blockIdx.x / (unsigned)tiles);
    const int tile = (int)(blockIdx.x - (unsigned)s * (unsigned)tiles);
    const int64_t b0 = (int64_t)tile * kT;
    const float *m = models + (int64_t)s * ldm;

    // ---- the convolutions' weights
    for (int i = tid; i < 25 * 8; i += kThreads) {
        const int tap = i >> 3, co = i & 7;
        w1s[i] = co < 6 ? m[off.o[0] + co * 25 + tap] : 0.f;
    }
    if (tid < 8) b1[tid] = tid < 6 ? m[off.o[1] + tid] : 0.f;
    if (tid < 16) b2[tid] = m[off.o[3] + tid];
    for (int i = tid; i < 16 * kK2; i += kThreads) {
        const int co = i / kK2, k = i - co * kK2;
        w2t[k * 16 + co] = m[off.o[2] + i];
    }
    if (tid < (kK2p - kK2) * 16) w2t[kK2 * 16 + tid] = 0.f;
    for (int k = tid; k < kK2p; k += kThreads) {
        const int kk = k < kK2 ? k : 0;
        const int ci = kk / 25, r = kk - ci * 25;
        kofs[k] = ci * 196 + (r / 5) * 14 + r % 5;
    }
    __syncthreads();

    // ---- conv1 + ReLU + 2x2 max-pool -> p1[img][ci][14][14]
    for (int i = tid; i < kT * 196; i += kThreads) {
        const int img = i / 196, pos = i - img * 196;
        const int py = pos / 14, px = pos - py * 14;
        const int64_t b = b0 + img;
        float p[36];
        if (b < B) {
            const f32x2 *src = reinterpret_cast<const f32x2 *>(x + b * 1024 + (2 * py) * 32 + 2 * px);
#pragma unroll
            for (int r = 0; r < 6; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const f32x2 v = src[r * 16 + c];
                    p[r * 6 + 2 * c] = v[0];
                    p[r * 6 + 2 * c + 1] = v[1];
                }
        } else {
#pragma unroll
            for (int e = 0; e < 36; ++e) p[e] = 0.f;
        }
        float acc[6][4];
#pragma unroll
        for (int co = 0; co < 6; ++co)
#pragma unroll
            for (int d = 0; d < 4; ++d) acc[co][d] = b1[co];
#pragma unroll
        for (int ky = 0; ky < 5; ++ky)
#pragma unroll
            for (int kx = 0; kx < 5; ++kx) {
                const f32x4 wa = *reinterpret_cast<const f32x4 *>(&w1s[(ky * 5 + kx) * 8]);
                const f32x4 wb = *reinterpret_cast<const f32x4 *>(&w1s[(ky * 5 + kx) * 8 + 4]);
                const float w[6] = {wa[0], wa[1], wa[2], wa[3], wb[0], wb[1]};
#pragma unroll
                for (int co = 0; co < 6; ++co)
#pragma unroll
                    for (int d = 0; d < 4; ++d)
                        acc[co][d] = __builtin_fmaf(p[((d >> 1) + ky) * 6 + (d & 1) + kx], w[co],
                                                    acc[co][d]);
            }
#pragma unroll
        for (int co = 0; co < 6; ++co) {
            const float t = max_nan(max_nan(relu_nan(acc[co][0]), relu_nan(acc[co][1])),
                                    max_nan(relu_nan(acc[co][2]), relu_nan(acc[co][3])));
            p1[img * kP1 + co * 196 + pos] = t;
        }
    }
    __syncthreads();

    // ---- conv2 + ReLU + 2x2 max-pool -> feat[img][co * 25 + pos]
    {
        const int n = lane & 15, q = lane >> 4;
        for (int ct = wave; ct < kT * 25 / 16; ct += kThreads / 64) {
            const int c = ct * 16 + n;  // < kT * 25
            const int img = c / 25, pos = c - img * 25;
            const int py = pos / 5, px = pos - py * 5;
            const float *base = p1 + img * kP1 + (2 * py) * 14 + 2 * px;
            f32x4 a00 = {0.f, 0.f, 0.f, 0.f}, a01 = a00, a10 = a00, a11 = a00;
#pragma unroll 2
            for (int st = 0; st < kK2p / 4; ++st) {
                const int k = st * 4 + q;
                const float a = w2t[k * 16 + n];  // zero for k >= 150
                const float *pp = base + kofs[k];
                const bool kv = k < kK2;
                const float v00 = kv ? pp[0] : 0.f, v01 = kv ? pp[1] : 0.f;
                const float v10 = kv ? pp[14] : 0.f, v11 = kv ? pp[15] : 0.f;
                a00 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, v00, a00, 0, 0, 0);
                a01 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, v01, a01, 0, 0, 0);
                a10 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, v10, a10, 0, 0, 0);
                a11 = __builtin_amdgcn_mfma_f32_16x16x4f32(a, v11, a11, 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int co = 4 * q + r;
                const float bb = b2[co];
                const float t = max_nan(max_nan(relu_nan(a00[r] + bb), relu_nan(a01[r] + bb)),
                                        max_nan(relu_nan(a10[r] + bb), relu_nan(a11[r] + bb)));
                feat[img * kFeatLd + co * 25 + pos] = t;
            }
        }
    }
    __syncthreads();

    // ---- the fully-connected head (h1, h2, lg alias p1: conv2 is done with it)
    fc_layer<400>(m + off.o[4], m + off.o[5], 120, feat, kFeatLd, h1, kH1Ld, true, wave, lane);
    __syncthreads();
    fc_layer<120>(m + off.o[6], m + off.o[7], 84, h1, kH1Ld, h2, kH2Ld, true, wave, lane);
    __syncthreads();
    fc_layer<84>(m + off.o[8], m + off.o[9], O, h2, kH2Ld, lg, kLgLd, false, wave, lane);
    __syncthreads();

    if (logits) {
        for (int i = tid; i < kT * O; i += kThreads) {
            const int img = i / O, o = i - img * O;
            const int64_t b = b0 + img;
            if (b < B) logits[((int64_t)s * B + b) * O + o] = lg[img * kLgLd + o];
        }
    }
    if constexpr (kLoss) {
        const int64_t b = b0 + tid;
        if (tid < kT && b < B) loss[(int64_t)s * ldn + b] = ce_row(lg + tid * kLgLd, 1, O, labels[b]);
    }
    if (correct && tid < 64) {
        bool hit = false;
        const int64_t b = b0 + tid;
        if (tid < kT && b < B) {
            // torch.argmax: the lowest index among equal maxima; a NaN is a maximum
            int best = 0;
            float bv = lg[tid * kLgLd];
            for (int o = 1; o < O; ++o) {
                const float v = lg[tid * kLgLd + o];
                if (bv == bv && (v > bv || v != v)) {
                    bv = v;
                    best = o;
                }
            }
            hit = (int64_t)best == labels[b];
        }
        const unsigned long long mask = __ballot(hit);
        if (tid == 0 && mask) atomicAdd(&correct[s], (unsigned long long)__popcll(mask));
    }
}

}  // namespace
}  // namespace dls

using namespace dls;

// Both entry points: fn names the caller in the messages; with_loss is the newer
// one, whose third output (loss, row pitch ldn) is optional like the other two.
static int lenet5_eval(const char *fn, bool with_loss, const float *models, int64_t ldm, int32_t S,
                       const int64_t *offsets, const float *x, int64_t B, const int64_t *labels,
                       int32_t O, float *logits, int64_t *correct, float *loss, int64_t ldn,
                       dls_stream_t stream) {
    static const char *const kNames[10] = {"conv1.weight", "conv1.bias", "conv2.weight",
                                           "conv2.bias",   "fc1.weight", "fc1.bias",
                                           "fc2.weight",   "fc2.bias",   "fc3.weight",
                                           "fc3.bias"};
    DLS_REQUIRE(models, DLS_EINVAL, "%s: null pointer: models", fn);
    DLS_REQUIRE(offsets, DLS_EINVAL, "%s: null pointer: offsets", fn);
    DLS_REQUIRE(x, DLS_EINVAL, "%s: null pointer: x", fn);
    if (with_loss) {
        DLS_REQUIRE(logits || correct || loss, DLS_EINVAL,
                    "%s: logits, correct and loss are all null", fn);
        DLS_REQUIRE(labels || !(correct || loss), DLS_EINVAL,
                    "%s: null pointer: labels (needed for correct and loss)", fn);
    } else {
        DLS_REQUIRE(logits || correct, DLS_EINVAL, "%s: logits and correct are both null", fn);
        DLS_REQUIRE(labels || !correct, DLS_EINVAL,
                    "%s: null pointer: labels (needed for correct)", fn);
    }
    DLS_REQUIRE(S >= 1, DLS_EINVAL, "%s: S=%d (at least 1)", fn, S);
    DLS_REQUIRE(B >= 0, DLS_EINVAL, "%s: B=%lld (negative)", fn, (long long)B);
    DLS_REQUIRE(O >= 1 && O <= kOMax, DLS_EINVAL, "%s: O=%d (1..%d)", fn, O, kOMax);
    DLS_REQUIRE(!loss || ldn >= B, DLS_EINVAL, "%s: ldn=%lld is less than B=%lld", fn,
                (long long)ldn, (long long)B);
    const int64_t tiles = (B + kT - 1) / kT;
    DLS_REQUIRE(tiles * S < (int64_t)1 << 31, DLS_EINVAL, "%s: S=%d x B=%lld exceeds one grid", fn,
                S, (long long)B);
    DLS_REQUIRE(aligned16(models), DLS_ELAYOUT, "%s: models: 16-byte alignment", fn);
    DLS_REQUIRE(aligned16(x), DLS_ELAYOUT, "%s: x: 16-byte alignment", fn);
    DLS_REQUIRE(!logits || aligned16(logits), DLS_ELAYOUT, "%s: logits: 16-byte alignment", fn);
    DLS_REQUIRE((reinterpret_cast<uintptr_t>(labels) & 7u) == 0, DLS_ELAYOUT,
                "%s: labels: 8-byte alignment", fn);
    DLS_REQUIRE((reinterpret_cast<uintptr_t>(correct) & 7u) == 0, DLS_ELAYOUT,
                "%s: correct: 8-byte alignment", fn);
    DLS_REQUIRE((reinterpret_cast<uintptr_t>(loss) & 3u) == 0, DLS_ELAYOUT,
                "%s: loss: 4-byte alignment", fn);
    DLS_REQUIRE(ldm > 0 && ldm % 4 == 0, DLS_ELAYOUT, "%s: ldm=%lld (a positive multiple of 4)", fn,
                (long long)ldm);
    const int64_t numel[10] = {150, 6, 2400, 16, 48000, 120, 10080, 84, (int64_t)O * 84, O};
    LenetOffsets off;
    for (int i = 0; i < 10; ++i) {
        DLS_REQUIRE(offsets[i] >= 0 && offsets[i] % 4 == 0, DLS_ELAYOUT,
                    "%s: offsets[%d] (%s) = %lld (a non-negative multiple of 4)", fn, i, kNames[i],
                    (long long)offsets[i]);
        DLS_REQUIRE(offsets[i] <= ldm - numel[i], DLS_EINVAL,
                    "%s: offsets[%d] (%s) = %lld: the tensor ends past ldm=%lld", fn, i, kNames[i],
                    (long long)offsets[i], (long long)ldm);
        off.o[i] = offsets[i];
    }
    if (B == 0) return DLS_OK;
    // without loss: the instantiation with no loss code, whichever entry was called
    auto *kernel = loss ? k_lenet5_eval<true> : k_lenet5_eval<false>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)(tiles * S)), dim3(kThreads), 0, as_stream(stream),
                       models, ldm, off, x, B, labels, (int)O, (int)tiles, logits,
                       reinterpret_cast<unsigned long long *>(correct), loss, ldn);
    return check_launch(fn);
}

extern "C" int dls_lenet5_eval_f32(const float *models, int64_t ldm, int32_t S,
                                   const int64_t *offsets, const float *x, int64_t B,
                                   const int64_t *labels, int32_t O, float *logits,
                                   int64_t *correct, dls_stream_t stream) {
    return lenet5_eval("dls_lenet5_eval_f32", false, models, ldm, S, offsets, x, B, labels, O, logits,
                       correct, nullptr, 0, stream);
}

extern "C" int dls_lenet5_eval_loss_f32(const float *models, int64_t ldm, int32_t S,
                                        const int64_t *offsets, const float *x, int64_t B,
                                        const int64_t *labels, int32_t O, float *logits,
                                        int64_t *correct, float *loss, int64_t ldn,
                                        dls_stream_t stream) {
    return lenet5_eval("dls_lenet5_eval_loss_f32", true, models, ldm, S, offsets, x, B, labels, O,
                       logits, correct, loss, ldn, stream);
}
