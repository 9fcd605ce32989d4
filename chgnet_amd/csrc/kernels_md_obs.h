// kernels_md_obs.h -- observables accumulated on the device while a molecular-dynamics run goes on (DESIGN.md "MD observables"):
// mean-squared displacement and velocity autocorrelation per species over a ring of the last L sampled snapshots, and the pair
// histogram of the radial distribution function.  Not in the reference, which post-processes a trajectory on the host.
//
// Every kernel reads a SNAPSHOT of a completed step (a frame slot of the step kernels, kernels_md.h: positions, momenta and cell as
// float64), never the live state, which already holds the next step's half kick and drift.  A replica whose status is not MD_RUNNING
// is skipped: its frame slot was not written, and it never runs again.
//
//   k_md_obs_push   one workgroup per replica: positions, velocities p / m and the mass-weighted centre of mass into ring slot k % L
//   k_md_obs_corr   one workgroup per (lag, replica): reduces over the replica's atoms in a fixed order and does one plain
//                   read-modify-write of the cells it alone owns -- no floating-point atomics, nothing depends on scheduling
//   k_md_obs_rdf    one workgroup per (16 atoms i, replica): all j and all lattice shifts by brute force, counts in an LDS histogram
//                   (integer LDS atomics), flushed once with 64-bit integer adds -- integers, so exact and order-independent
//
// Float64 throughout; the per-species accumulators are selected, never indexed, so nothing lives in scratch.  The kernels are built from
// the helpers of kernels_md_sample.h.
#pragma once

#include "kernels_md_sample.h"   // the snapshot and ring views and the helpers every observer kernel is built from

namespace chg {

constexpr int MD_OBS_MAX_LAGS = 4096;    // L <= 4096
constexpr int MD_OBS_RDF_CELLS = 16384;  // S * S * bins: 64 KB of uint32 counts in LDS

struct MdObsArgs {
  MdSnapshot s;
  MdRing r;                  // MSD / VACF
  double *msd, *vacf;        // [B, L, S]
  long long* cnt;            // [B, L]
  // RDF
  unsigned long long* hist;  // [B, S, S, bins]
  long long* rdf_samples;    // [B]
  double* vol_sum;           // [B]
  int bins;
  double rmax;
};

static __global__ __launch_bounds__(256) void k_md_obs_push(MdObsArgs a) {
  const int tid = threadIdx.x, o = blockIdx.x;
  int a0, n;
  if (!md_running(a.s, o, a0, n)) return;
  const size_t row = ((size_t)a.r.slot * a.s.N + a0) * 3;
  __shared__ double red[4][4];
  // the centre of mass relative to the replica's first atom: the sum carries displacements, not unwrapped positions that may lie
  // thousands of cells away, and a single atom is its own centre of mass exactly
  const double x0[3] = {a.s.pos[3 * (size_t)a0], a.s.pos[3 * (size_t)a0 + 1], a.s.pos[3 * (size_t)a0 + 2]};
  double acc[4] = {0.0, 0.0, 0.0, 0.0};   // sum m (r - r_0), sum m
  for (int i = tid; i < n; i += 256) {
    const double m = a.s.mass[a0 + i];
    const size_t g = 3 * ((size_t)a0 + i);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double x = a.s.pos[g + j];
      a.r.ring_pos[row + 3 * (size_t)i + j] = x;
      a.r.ring_vel[row + 3 * (size_t)i + j] = a.s.mom[g + j] / m;
      acc[j] += m * (x - x0[j]);
    }
    acc[3] += m;
  }
  block_sum(acc, red);
  if (tid < 3) a.r.ring_com[((size_t)a.r.slot * a.s.B + o) * 3 + tid] = a.s.pos[3 * (size_t)a0 + tid] + block_total(red, tid) / block_total(red, 3);
}

// grid (lags of this sample, B)
static __global__ __launch_bounds__(256) void k_md_obs_corr(MdObsArgs a) {
  const int tid = threadIdx.x, l = blockIdx.x, o = blockIdx.y;
  int a0, n;
  if (!md_running(a.s, o, a0, n)) return;
  const MdLag g = md_lag(a.r, a.s.N, a0, l);
  const size_t r1 = 3 * g.row1, r0 = 3 * g.row0;
  double R1[3], R0[3];
  md_lag_com(a.r, a.s.B, o, g, R1, R0);
  __shared__ double red[4][2 * MD_OBS_SPECIES];
  double acc[2 * MD_OBS_SPECIES] = {};   // |u|^2 of species s at 2 s, v(k) . v(k - l) at 2 s + 1
  for (int i = tid; i < n; i += 256) {
    const int sp = a.s.species[a0 + i];
    double d2 = 0.0, vv = 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double d = (a.r.ring_pos[r1 + 3 * (size_t)i + j] - R1[j]) - (a.r.ring_pos[r0 + 3 * (size_t)i + j] - R0[j]);
      d2 += d * d;
      vv += a.r.ring_vel[r1 + 3 * (size_t)i + j] * a.r.ring_vel[r0 + 3 * (size_t)i + j];
    }
    species_add<2>(acc, sp, {d2, vv});
  }
  block_sum(acc, red);
  const size_t cell = (size_t)o * a.r.L + l;
  if (tid < a.s.S) {
    a.msd[cell * a.s.S + tid] += block_total(red, 2 * tid);
    a.vacf[cell * a.s.S + tid] += block_total(red, 2 * tid + 1);
  }
  if (tid == 0) a.cnt[cell] += 1;
}

// grid (ceil(largest replica / MD_OBS_RDF_ROWS), B), dynamic LDS S * S * bins * 4 bytes; rows are keyed by the species of i
static __global__ __launch_bounds__(256) void k_md_obs_rdf(MdObsArgs a) {
  extern __shared__ unsigned int s_hist[];
  __shared__ MdImageCell s_cell;
  const int o = blockIdx.y, i0 = blockIdx.x * MD_OBS_RDF_ROWS;
  int a0, n;
  if (!md_running(a.s, o, a0, n) || i0 >= n) return;
  md_pair_histogram(a.s, o, a0, n, i0, [&](int ii) {
    const int sp = a.s.species[a0 + i0 + ii];
    __builtin_assume(sp >= 0);   // checked on the host: no row is skipped, and no branch waits for this load
    return sp;
  }, a.s.S, a.bins, a.rmax, s_hist, s_cell, a.hist,
                    a.rdf_samples, a.vol_sum);   // the first row chunk alone owns the replica's two scalars
}

}  // namespace chg
