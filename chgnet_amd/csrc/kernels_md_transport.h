// kernels_md_transport.h -- transport observables on the ring of kernels_md_obs.h (DESIGN.md "MD observables", include/chgnet_hip.h "MD
// observables"): the fourth moment of the displacement per species (non-Gaussian parameter), the collective displacement and current
// correlations between species (Einstein and Green-Kubo forms of the ionic conductivity, Onsager cross terms) and the self part of the
// van Hove function.  Not in the reference, which post-processes a trajectory on the host.
//
// Both kernels run after k_md_obs_push of the same sample and read the ring it filled, never the live state; a replica whose status
// is not MD_RUNNING is skipped, as there.
//
//   k_md_obs_current    one workgroup per replica: J_a(k) = sum_{i in a} p_i / m_i into slot k % L of a ring [L, B, S, 3], and the
//                       replica's two scalars (samples, vol_sum), which this workgroup alone owns
//   k_md_obs_transport  one workgroup per (lag, replica): one pass over the replica's atoms in a fixed order for |u_i|^4 per species,
//                       U_a = sum_{i in a} u_i and the displacement histogram (integer LDS atomics), then S x S dot products of the
//                       U_a and of J_a(k), J_b(k - l).  Every global cell has this one owner, which does a plain read-modify-write:
//                       no floating-point atomics, nothing depends on scheduling
//
// Float64 throughout; the per-species accumulators are selected, never indexed, so nothing lives in scratch.
#pragma once

#include "kernels_md_obs.h"

namespace chg {

constexpr int MD_OBS_VH_CELLS = 4096;   // S * vh_bins: 16 KB of uint32 counts in static LDS

struct MdTransportArgs {
  const double* cell;        // [B, 9] of the sampled snapshot
  const int* species;        // [N] 0 .. S - 1
  const int* status;         // status of replica o at status[o * status_stride]
  int status_stride;
  const int* aoff;           // [B + 1]
  int N, B, S;
  // the ring of the plain observers, slot k % L already pushed
  const double *ring_pos, *ring_vel;   // [L, N, 3]
  const double* ring_com;              // [L, B, 3]
  double* ring_j;                      // [L, B, S, 3]
  int L, slot;
  long long k;
  int subtract_com;
  int collective, non_gaussian;
  double* msd4;              // [B, L, S]
  double *cmsd, *jacf;       // [B, L, S, S]
  unsigned long long* vh;    // [B, vh_lags, S, vh_bins]
  long long* samples;        // [B]
  double* vol_sum;           // [B]
  int vh_bins, vh_lags, vh_stride;
  double vh_rmax;
};

// grid (B)
static __global__ __launch_bounds__(256) void k_md_obs_current(MdTransportArgs a) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int o = blockIdx.x;
  if (a.status[(size_t)o * a.status_stride] != MD_RUNNING) return;
  const int a0 = a.aoff[o], n = a.aoff[o + 1] - a0;
  const size_t row = ((size_t)a.slot * a.N + a0) * 3;
  __shared__ double red[4][3 * MD_OBS_SPECIES];
  double acc[3 * MD_OBS_SPECIES];
#pragma unroll
  for (int s = 0; s < 3 * MD_OBS_SPECIES; ++s) acc[s] = 0.0;
  for (int i = tid; i < n; i += 256) {
    const int sp = a.species[a0 + i];
    double v[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) v[j] = a.ring_vel[row + 3 * (size_t)i + j];
#pragma unroll
    for (int s = 0; s < MD_OBS_SPECIES; ++s)   // selected, not indexed: the accumulators stay in registers
#pragma unroll
      for (int j = 0; j < 3; ++j) acc[3 * s + j] += sp == s ? v[j] : 0.0;
  }
#pragma unroll
  for (int s = 0; s < 3 * MD_OBS_SPECIES; ++s) {
    acc[s] = wave_sum_f64(acc[s]);
    if (lane == 0) red[wv][s] = acc[s];
  }
  __syncthreads();
  if (a.collective && tid < 3 * a.S) a.ring_j[((size_t)a.slot * a.B + o) * a.S * 3 + tid] = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
  if (tid == 0) {
    double L[9];
    for (int i = 0; i < 9; ++i) L[i] = a.cell[9 * (size_t)o + i];
    a.samples[o] += 1;
    a.vol_sum[o] += fabs(det3(L));
  }
}

// grid (lags of this sample, B)
static __global__ __launch_bounds__(256) void k_md_obs_transport(MdTransportArgs a) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int l = blockIdx.x, o = blockIdx.y;
  if (a.status[(size_t)o * a.status_stride] != MD_RUNNING) return;
  const int a0 = a.aoff[o], n = a.aoff[o + 1] - a0;
  const int then = (int)((a.k - l) % a.L);
  const size_t r1 = ((size_t)a.slot * a.N + a0) * 3, r0 = ((size_t)then * a.N + a0) * 3;
  const int S = a.S, bins = a.vh_bins;
  const bool hist = bins > 0 && l % a.vh_stride == 0 && l / a.vh_stride < a.vh_lags;   // the same for the whole workgroup
  __shared__ unsigned int s_vh[MD_OBS_VH_CELLS];
  __shared__ double red[4][4 * MD_OBS_SPECIES];
  __shared__ double sU[3 * MD_OBS_SPECIES];
  if (hist) {
    for (int c = tid; c < S * bins; c += 256) s_vh[c] = 0u;
    __syncthreads();
  }
  double R1[3], R0[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    R1[j] = a.subtract_com ? a.ring_com[((size_t)a.slot * a.B + o) * 3 + j] : 0.0;
    R0[j] = a.subtract_com ? a.ring_com[((size_t)then * a.B + o) * 3 + j] : 0.0;
  }
  double acc[4 * MD_OBS_SPECIES];   // |u|^4 of species s at s, U_s at MD_OBS_SPECIES + 3 s ..
#pragma unroll
  for (int s = 0; s < 4 * MD_OBS_SPECIES; ++s) acc[s] = 0.0;
  const double rmax = a.vh_rmax;
  for (int i = tid; i < n; i += 256) {
    const int sp = a.species[a0 + i];
    double u[3], d2 = 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      u[j] = (a.ring_pos[r1 + 3 * (size_t)i + j] - R1[j]) - (a.ring_pos[r0 + 3 * (size_t)i + j] - R0[j]);
      d2 += u[j] * u[j];
    }
    const double d4 = d2 * d2;
#pragma unroll
    for (int s = 0; s < MD_OBS_SPECIES; ++s) {   // selected, not indexed: the accumulators stay in registers
      acc[s] += sp == s ? d4 : 0.0;
#pragma unroll
      for (int j = 0; j < 3; ++j) acc[MD_OBS_SPECIES + 3 * s + j] += sp == s ? u[j] : 0.0;
    }
    if (hist) {
      const double d = sqrt(d2);
      if (d < rmax) atomicAdd(s_vh + sp * bins + min((int)(d / rmax * bins), bins - 1), 1u);
    }
  }
#pragma unroll
  for (int s = 0; s < 4 * MD_OBS_SPECIES; ++s) {
    acc[s] = wave_sum_f64(acc[s]);
    if (lane == 0) red[wv][s] = acc[s];
  }
  __syncthreads();   // the partial sums and every count of the histogram are in LDS
  const size_t cell = (size_t)o * a.L + l;
  if (a.non_gaussian && tid < S) a.msd4[cell * S + tid] += red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
  if (tid < 3 * MD_OBS_SPECIES) {
    const int c = MD_OBS_SPECIES + tid;
    sU[tid] = red[0][c] + red[1][c] + red[2][c] + red[3][c];
  }
  __syncthreads();
  if (a.collective && tid < S * S) {
    const int p = tid / S, q = tid - p * S;
    const double* Jk = a.ring_j + (((size_t)a.slot * a.B + o) * S + p) * 3;
    const double* J0 = a.ring_j + (((size_t)then * a.B + o) * S + q) * 3;
    const double *Up = sU + 3 * p, *Uq = sU + 3 * q;
    // products commute, so the (p, q) and (q, p) cells of cmsd are the same bits
    a.cmsd[(cell * S + p) * S + q] += Up[0] * Uq[0] + Up[1] * Uq[1] + Up[2] * Uq[2];
    a.jacf[(cell * S + p) * S + q] += Jk[0] * J0[0] + Jk[1] * J0[1] + Jk[2] * J0[2];
  }
  if (hist) {
    unsigned long long* out = a.vh + ((size_t)o * a.vh_lags + l / a.vh_stride) * S * bins;
    for (int c = tid; c < S * bins; c += 256) {
      const unsigned int v = s_vh[c];
      if (v) out[c] += v;
    }
  }
}

}  // namespace chg
