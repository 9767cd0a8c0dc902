// Philox4x32-10 for gfx950, shared by the sampler (sample_kernels.h) and the dropout masks (dropout_kernels.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "attn_common.h"

namespace fat5 {

// Philox4x32-10 (Salmon et al., SC'11; the Random123 constants)
FAT5_DEV void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t lo0 = 0xD2511F53u * c[0], hi0 = __umulhi(0xD2511F53u, c[0]);
    const uint32_t lo1 = 0xCD9E8D57u * c[2], hi1 = __umulhi(0xCD9E8D57u, c[2]);
    const uint32_t n0 = hi1 ^ c[1] ^ k0, n2 = hi0 ^ c[3] ^ k1;
    c[0] = n0, c[1] = lo1, c[2] = n2, c[3] = lo0;
    k0 += 0x9E3779B9u, k1 += 0xBB67AE85u;
  }
}

}  // namespace fat5
