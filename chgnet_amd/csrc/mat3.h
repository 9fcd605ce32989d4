// mat3.h -- 3x3 (row-major) and wave-reduction helpers shared by the integrator step kernels (kernels_relax.h, kernels_md.h).
// The 3x3 helpers are host and device code: the drivers (engine_stepper.h) form the initial cell inverse with the same inv3.
#pragma once

#include <hip/hip_runtime.h>

namespace chg {

__host__ __device__ __forceinline__ void mm3(const double* a, const double* b, double* c) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) c[3 * i + j] = a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j] + a[3 * i + 2] * b[6 + j];
}
__host__ __device__ __forceinline__ double det3(const double* m) {
  return m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}
__host__ __device__ __forceinline__ void inv3(const double* m, double* r) {
  const double id = 1.0 / det3(m);
  r[0] = (m[4] * m[8] - m[5] * m[7]) * id; r[1] = (m[2] * m[7] - m[1] * m[8]) * id; r[2] = (m[1] * m[5] - m[2] * m[4]) * id;
  r[3] = (m[5] * m[6] - m[3] * m[8]) * id; r[4] = (m[0] * m[8] - m[2] * m[6]) * id; r[5] = (m[2] * m[3] - m[0] * m[5]) * id;
  r[6] = (m[3] * m[7] - m[4] * m[6]) * id; r[7] = (m[1] * m[6] - m[0] * m[7]) * id; r[8] = (m[0] * m[4] - m[1] * m[3]) * id;
}

__device__ __forceinline__ double wave_sum_f64(double x) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off);
  return x;
}
__device__ __forceinline__ double wave_max_f64(double x) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) x = fmax(x, __shfl_xor(x, off));
  return x;
}

}  // namespace chg
