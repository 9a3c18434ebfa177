// Philox4x32-10 (Salmon et al., Random123): four 32-bit words of a counter (c0..c3) under a key (k0, k1), ten rounds.  The one
// statement of the generator on the device; lav_amd.data.augment.philox4x32 is the same function over NumPy arrays.  Integer
// arithmetic only: every caller gets the same words whatever its translation unit's floating-point flags are.
#pragma once
#include <hip/hip_runtime.h>

namespace lav {

__device__ __forceinline__ void philox4x32(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned (&o)[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}

}  // namespace lav
