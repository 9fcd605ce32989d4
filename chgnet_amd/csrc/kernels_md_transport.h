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
// Float64 throughout; the per-species accumulators are selected, never indexed, so nothing lives in scratch.  The kernels are built from
// the helpers of kernels_md_sample.h.
#pragma once

#include "kernels_md_obs.h"

namespace chg {

constexpr int MD_OBS_VH_CELLS = 4096;   // S * vh_bins: 16 KB of uint32 counts in static LDS

struct MdTransportArgs {
  MdSnapshot s;
  MdRing r;                  // the ring of the plain observers, slot k % L already pushed
  double* ring_j;            // [L, B, S, 3]
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
  const int tid = threadIdx.x, o = blockIdx.x;
  int a0, n;
  if (!md_running(a.s, o, a0, n)) return;
  const double* vel = a.r.ring_vel + ((size_t)a.r.slot * a.s.N + a0) * 3;
  __shared__ double red[4][3 * MD_OBS_SPECIES];
  double acc[3 * MD_OBS_SPECIES] = {};   // J_s at 3 s ..
  for (int i = tid; i < n; i += 256)
    species_add<3>(acc, a.s.species[a0 + i], {vel[3 * (size_t)i], vel[3 * (size_t)i + 1], vel[3 * (size_t)i + 2]});
  block_sum(acc, red);
  if (a.collective && tid < 3 * a.s.S) a.ring_j[((size_t)a.r.slot * a.s.B + o) * a.s.S * 3 + tid] = block_total(red, tid);
  if (tid == 0) md_count_sample(a.samples, a.vol_sum, o, md_volume(a.s, o));
}

// grid (lags of this sample, B)
static __global__ __launch_bounds__(256) void k_md_obs_transport(MdTransportArgs a) {
  const int tid = threadIdx.x, l = blockIdx.x, o = blockIdx.y;
  int a0, n;
  if (!md_running(a.s, o, a0, n)) return;
  const MdLag g = md_lag(a.r, a.s.N, a0, l);
  const double *p1 = a.r.ring_pos + 3 * g.row1, *p0 = a.r.ring_pos + 3 * g.row0;
  const int S = a.s.S, bins = a.vh_bins;
  const bool hist = bins > 0 && l % a.vh_stride == 0 && l / a.vh_stride < a.vh_lags;   // the same for the whole workgroup
  __shared__ unsigned int s_vh[MD_OBS_VH_CELLS];
  __shared__ double red[4][4 * MD_OBS_SPECIES];
  __shared__ double sU[3 * MD_OBS_SPECIES];
  if (hist) {
    hist_zero(s_vh, S * bins);
    __syncthreads();
  }
  double R1[3], R0[3];
  md_lag_com(a.r, a.s.B, o, g, R1, R0);
  double acc[4 * MD_OBS_SPECIES] = {};   // |u|^4 of species s at 4 s, U_s at 4 s + 1 ..
  const double rmax = a.vh_rmax;
  for (int i = tid; i < n; i += 256) {
    const int sp = a.s.species[a0 + i];
    double u[3], d2 = 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      u[j] = (p1[3 * (size_t)i + j] - R1[j]) - (p0[3 * (size_t)i + j] - R0[j]);
      d2 += u[j] * u[j];
    }
    species_add<4>(acc, sp, {d2 * d2, u[0], u[1], u[2]});
    if (hist) {
      const double d = sqrt(d2);
      if (d < rmax) atomicAdd(s_vh + sp * bins + hist_bin(d, rmax, bins), 1u);
    }
  }
  block_sum(acc, red);   // the partial sums and every count of the histogram are in LDS
  const size_t cell = (size_t)o * a.r.L + l;
  if (a.non_gaussian && tid < S) a.msd4[cell * S + tid] += block_total(red, 4 * tid);
  if (tid < 3 * MD_OBS_SPECIES) sU[tid] = block_total(red, 4 * (tid / 3) + 1 + tid % 3);
  __syncthreads();
  if (a.collective && tid < S * S) {
    const int p = tid / S, q = tid - p * S;
    const double* Jk = a.ring_j + (((size_t)a.r.slot * a.s.B + o) * S + p) * 3;
    const double* J0 = a.ring_j + (((size_t)g.then * a.s.B + o) * S + q) * 3;
    const double *Up = sU + 3 * p, *Uq = sU + 3 * q;
    // products commute, so the (p, q) and (q, p) cells of cmsd are the same bits
    a.cmsd[(cell * S + p) * S + q] += Up[0] * Uq[0] + Up[1] * Uq[1] + Up[2] * Uq[2];
    a.jacf[(cell * S + p) * S + q] += Jk[0] * J0[0] + Jk[1] * J0[1] + Jk[2] * J0[2];
  }
  if (hist) hist_flush_owned(s_vh, a.vh + ((size_t)o * a.vh_lags + l / a.vh_stride) * S * bins, S * bins);
}

}  // namespace chg
