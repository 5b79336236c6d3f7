// The device's N(0, 1) stream: Philox4x32-10 (Salmon et al., SC'11) + Box-Muller, written once for
// the kernels that draw from it (k_u_normal, ugemm.hip: the U buffers; k_joint_normal,
// predict_joint.hip: the joint predictive's draws). The stream of one (seed, counter) is a flat
// sequence: block q yields elements 4q .. 4q + 3, and a kernel decides where element e goes.
#pragma once
#include "apm_common.h"

__device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
        const uint32_t hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
        const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
        c[0] = n0;
        c[1] = lo1;
        c[2] = n2;
        c[3] = lo0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
}

// Elements 4q .. 4q + 3 of the stream (sd, ct): counter = (q, ctr_lo, ctr_hi, q >> 32), key =
// (seed_lo, seed_hi); the block's 4 words give 2 Box-Muller pairs u = (w + 0.5) 2^-32 in fp32,
// z = sqrt(-2 log u1) (cos, sin)(2 pi u2)
__device__ __forceinline__ void philox_normal4(int64_t q, uint64_t sd, uint64_t ct, float (&z)[4]) {
    uint32_t c[4] = {(uint32_t)q, (uint32_t)ct, (uint32_t)(ct >> 32), (uint32_t)(q >> 32)};
    philox4x32_10(c, (uint32_t)sd, (uint32_t)(sd >> 32));
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const float u1 = ((float)c[2 * h] + 0.5f) * 2.3283064365386963e-10f;
        const float u2 = ((float)c[2 * h + 1] + 0.5f) * 2.3283064365386963e-10f;
        const float rr = sqrtf(-2.0f * logf(u1));
        float sn, cs;
        sincosf(6.283185307179586f * u2, &sn, &cs);
        z[2 * h] = rr * cs;
        z[2 * h + 1] = rr * sn;
    }
}
