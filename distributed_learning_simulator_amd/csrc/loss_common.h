// The per-image cross-entropy of the loss utilities (the tester's loss behind
// servers/fed_server.py:26-32), shared by the stand-alone kernel (loss.hip) and
// the LeNet-5 kernel's epilogue (lenet.hip) so that both give the same bits.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dls {

// loss = (m - z[label]) + log(sum_o exp(z[o] - m)), m = max_o z[o]; z[o] is read at
// z[o * stride].  fp32 throughout, every step in index order: the maximum as the
// kernels' argmax has it (a NaN is a maximum, so it reaches every term), the sum
// for o ascending, the device library's expf / logf (z[o] - m <= 0: no overflow at
// any scale).  A label outside [0, O) gives NaN and reads nothing.  One lane
// computes one image's loss: it cannot depend on the lane's neighbours.
__device__ __forceinline__ float ce_row(const float *z, int stride, int O, int64_t label) {
    if (label < 0 || label >= (int64_t)O) return __builtin_nanf("");
    float m = z[0];
    for (int o = 1; o < O; ++o) {
        const float v = z[(int64_t)o * stride];
        if (m == m && (v > m || v != v)) m = v;
    }
    float s = 0.f;
    for (int o = 0; o < O; ++o) s += expf(z[(int64_t)o * stride] - m);
    return (m - z[label * stride]) + logf(s);
}

}  // namespace dls
