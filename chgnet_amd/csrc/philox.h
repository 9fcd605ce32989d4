// philox.h -- counter-based standard normals for the Langevin thermostat of the MD step kernel (kernels_md.h, MD_NVT_LANGEVIN).
//
// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11).  No generator state lives in
// memory: the three normals of one atom in one step are a pure function of
//   key     = (seed & 0xffffffff, seed >> 32)                    one 64-bit seed per replica
//   counter = (atom index within its replica, steps completed by the replica, blk, 0)      blk = 0, 1
// so a replica draws the same noise alone, in any slot of a batch, after a retry and across split runs.  Each 4-word block gives two
// uniforms in (0, 1] with 53 random bits each, u = ((w_even >> 5) 2^26 + (w_odd >> 6) + 1/2) 2^-53, and Box-Muller in float64 turns
// them into two normals.  tests/langevin_ref.py restates this bit for bit up to the last place of log / sin / cos.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace chg {

__host__ __device__ __forceinline__ uint32_t philox_mulhi(uint32_t a, uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umulhi(a, b);
#else
  return (uint32_t)(((uint64_t)a * b) >> 32);
#endif
}

// w <- Philox4x32-10(counter c, key (k0, k1))
__host__ __device__ __forceinline__ void philox4x32_10(const uint32_t c[4], uint32_t k0, uint32_t k1, uint32_t w[4]) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
  uint32_t x0 = c[0], x1 = c[1], x2 = c[2], x3 = c[3];
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint32_t hi0 = philox_mulhi(M0, x0), lo0 = M0 * x0;
    const uint32_t hi1 = philox_mulhi(M1, x2), lo1 = M1 * x2;
    x0 = hi1 ^ x1 ^ k0; x1 = lo1; x2 = hi0 ^ x3 ^ k1; x3 = lo0;
    k0 += W0; k1 += W1;
  }
  w[0] = x0; w[1] = x1; w[2] = x2; w[3] = x3;
}

// 53 random bits from two words, centred in their cell: never 0
__host__ __device__ __forceinline__ double philox_uniform(uint32_t a, uint32_t b) {
  return ((double)(a >> 5) * 67108864.0 + (double)(b >> 6) + 0.5) * 0x1p-53;
}

// the two Box-Muller normals of block blk of (seed, atom, step)
__host__ __device__ __forceinline__ void philox_normal2(uint64_t seed, uint32_t atom, uint32_t step, uint32_t blk, double* z0, double* z1) {
  const uint32_t c[4] = {atom, step, blk, 0u};
  uint32_t w[4];
  philox4x32_10(c, (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), w);
  const double rho = sqrt(-2.0 * log(philox_uniform(w[0], w[1])));
  double s, co;
  sincos(6.283185307179586 * philox_uniform(w[2], w[3]), &s, &co);
  *z0 = rho * co;
  *z1 = rho * s;
}

// xi in R^3 of (seed, atom, step): both normals of block 0, the first of block 1
__host__ __device__ __forceinline__ void philox_normal3(uint64_t seed, uint32_t atom, uint32_t step, double xi[3]) {
  double spare;
  philox_normal2(seed, atom, step, 0u, &xi[0], &xi[1]);
  philox_normal2(seed, atom, step, 1u, &xi[2], &spare);
}

}  // namespace chg
