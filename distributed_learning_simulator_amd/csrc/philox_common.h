// The library's random stream, shared by its users (dpnoise.hip, secagg.hip):
// Philox4x32-10 on (seed, stream_id, coordinate / 4); word coordinate % 4 of a block
// belongs to the coordinate (include/dls_hip.h has the contract).
#pragma once

#include "dls_common.h"

namespace dls {

struct PhiloxKey {
    uint32_t k0, k1;  // the seed's halves
    uint32_t s0, s1;  // the stream id's halves: counter words 2 and 3
};

__host__ __device__ inline PhiloxKey make_key(uint64_t seed, uint64_t stream_id) {
    return {(uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)stream_id,
            (uint32_t)(stream_id >> 32)};
}

// The four words of block `b`.
__device__ __forceinline__ u32x4 philox_block(uint64_t b, const PhiloxKey &key) {
    uint32_t c0 = (uint32_t)b, c1 = (uint32_t)(b >> 32), c2 = key.s0, c3 = key.s1;
    uint32_t k0 = key.k0, k1 = key.k1;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return (u32x4){c0, c1, c2, c3};
}

}  // namespace dls
