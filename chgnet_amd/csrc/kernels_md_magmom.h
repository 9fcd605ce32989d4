// kernels_md_magmom.h -- site magnetic moments in device molecular dynamics (DESIGN.md "MD observables -> Charge states",
// include/chgnet_hip.h "Charge-informed MD"): the moments of every completed step into the frames, and charge-state observers that
// classify every atom's moment against per-species boundaries (Mn2+/Mn3+/Mn4+ by thresholds, the reference's charge-informed MD) and
// accumulate on the ring logic of kernels_md_obs.h.  The reference logs moments per frame and post-processes them on the host.
//
//   k_md_mag_gather   one workgroup per replica, right after the step kernel of an evaluation that completes a step: the batch's
//                     moments (original atom order: MD never compacts) into the frame slot and into the "last completed step" array,
//                     under the step kernel's own rule for writing a frame
//   k_md_chg_sample   one workgroup per replica: classifies every atom, pushes moment and state into ring slot k % L, updates the
//                     per-atom previous state and occupancy, sums m and m^2 per species in a fixed order, counts the moment
//                     histogram, populations and transitions in LDS integers and flushes them once; owns samples / vol_sum / skipped
//   k_md_chg_corr     one workgroup per (lag, replica): sum m_i(k) m_i(k - l) per species in a fixed order, and the number of atoms
//                     that are in the same state at both ends of the lag (LDS integers)
//   k_md_chg_srdf     one workgroup per (16 centre rows, replica): distances from atoms of the centre species to all atoms and lattice
//                     images by brute force, as k_md_obs_rdf, binned by the STATE of the centre and the species of the neighbour
//
// All of them read a SNAPSHOT of a completed step and skip a replica that is not MD_RUNNING.  Float64 and integers; no floating-point
// atomics: every float cell has one owning workgroup that does a plain read-modify-write, counts are integers.  The per-species
// accumulators are selected, never indexed, so nothing lives in scratch.  The observer kernels are built from the helpers of
// kernels_md_sample.h.
#pragma once

#include "kernels_md_obs.h"

namespace chg {

constexpr int MD_CHG_STATES = 4;         // Q: at most 3 boundaries per species
constexpr int MD_CHG_BOUNDS = 3;
constexpr int MD_CHG_HIST_CELLS = 4096;  // S * mag_bins: 16 KB of uint32 counts in static LDS
constexpr int MD_CHG_SRDF_CELLS = 16384; // Q * S * srdf_bins: 64 KB of uint32 counts in dynamic LDS

struct MdMagArgs {
  const float* magmom;   // [N] of the evaluated batch
  float* frame;          // [N] frame slot, or null
  float* last;           // [N] moments of the last completed step
  const int* si;         // [B, MD_SI]: status at 1
  const int* retry;      // [B]
  const int* sel;        // [grid] or null
  const int* aoff;       // [B + 1]
  int final_try;
};

// grid: the replicas of the step launch it follows.  The step kernel has already set the status and the retry flag of this evaluation.
static __global__ __launch_bounds__(256) void k_md_mag_gather(MdMagArgs a) {
  const int o = a.sel ? a.sel[blockIdx.x] : blockIdx.x;
  if (a.si[(size_t)MD_SI * o + 1] != MD_RUNNING) return;      // stopped now or earlier: no frame
  if (a.retry[o] && !a.final_try) return;                     // held back: the retry launch writes the slot
  const int a0 = a.aoff[o], n = a.aoff[o + 1] - a0;
  for (int i = threadIdx.x; i < n; i += 256) {
    const float m = a.magmom[a0 + i];
    a.last[a0 + i] = m;
    if (a.frame) a.frame[a0 + i] = m;
  }
}

struct MdChgArgs {
  MdSnapshot s;              // the sampled step, with its moments
  MdRing r;                  // L, slot and k of the plain observers' ring (L may be 0: no lag sums); its arrays are not read
  const double* bounds;      // [S, MD_CHG_BOUNDS]
  const int* n_bounds;       // [S]
  double* ring_m;            // [L, N]
  int* ring_q;               // [L, N]
  int* prev_q;               // [N] state at the previous sample
  // accumulators
  unsigned long long* mhist; // [B, S, mag_bins]
  double *msum, *msq;        // [B, S]
  long long* pop;            // [B, S, Q]
  long long* trans;          // [B, S, Q, Q]
  long long* occ;            // [N, Q]
  double* mcorr;             // [B, L, S]
  long long* same;           // [B, L, S, Q]
  unsigned long long* shist; // [B, Q, S, srdf_bins]
  long long *samples, *skipped;   // [B]
  double* vol_sum;           // [B]
  int mag_bins, center, srdf_bins;
  double mag_max, srdf_rmax;
};

// the number of boundaries of the species that are <= m; -1 for a non-finite moment
__device__ __forceinline__ int md_chg_state(double m, const double* bounds, int nb) {
  if (!isfinite(m)) return -1;
  int q = 0;
#pragma unroll
  for (int b = 0; b < MD_CHG_BOUNDS; ++b) q += (b < nb && bounds[b] <= m) ? 1 : 0;
  return q;
}

// grid (B)
static __global__ __launch_bounds__(256) void k_md_chg_sample(MdChgArgs a) {
  const int tid = threadIdx.x, o = blockIdx.x;
  int a0, n;
  if (!md_running(a.s, o, a0, n)) return;
  const int S = a.s.S, bins = a.mag_bins;
  constexpr int Q = MD_CHG_STATES;
  __builtin_assume(S <= MD_OBS_SPECIES);   // checked on the host: the flushes of pop and trans are one pass
  __shared__ unsigned int s_hist[MD_CHG_HIST_CELLS];
  __shared__ unsigned int s_pop[MD_OBS_SPECIES * Q], s_trans[MD_OBS_SPECIES * Q * Q], s_skip;
  __shared__ double s_bounds[MD_OBS_SPECIES * MD_CHG_BOUNDS];
  __shared__ int s_nb[MD_OBS_SPECIES];
  __shared__ double red[4][2 * MD_OBS_SPECIES];
  hist_zero(s_hist, S * bins);
  hist_zero(s_pop, MD_OBS_SPECIES * Q);
  hist_zero(s_trans, MD_OBS_SPECIES * Q * Q);
  if (tid < S * MD_CHG_BOUNDS) s_bounds[tid] = a.bounds[tid];
  if (tid < S) s_nb[tid] = a.n_bounds[tid];
  if (tid == 0) s_skip = 0u;
  __syncthreads();
  double acc[2 * MD_OBS_SPECIES] = {};   // sum m of species s at 2 s, sum m^2 at 2 s + 1
  const double mmax = a.mag_max;
  const bool first = a.r.k == 0;
  for (int i = tid; i < n; i += 256) {
    const int g = a0 + i;
    const int sp = a.s.species[g];
    const double m = (double)a.s.mag[g];
    const int q = md_chg_state(m, s_bounds + sp * MD_CHG_BOUNDS, s_nb[sp]);
    const int before = first ? -1 : a.prev_q[g];
    a.prev_q[g] = q;
    if (a.r.L > 0) {
      a.ring_m[(size_t)a.r.slot * a.s.N + g] = m;
      a.ring_q[(size_t)a.r.slot * a.s.N + g] = q;
    }
    if (q < 0) {
      atomicAdd(&s_skip, 1u);
      continue;
    }
    a.occ[(size_t)g * Q + q] += 1;
    atomicAdd(s_pop + sp * Q + q, 1u);
    if (before >= 0) atomicAdd(s_trans + (sp * Q + before) * Q + q, 1u);
    if (bins > 0 && m >= 0.0 && m < mmax) atomicAdd(s_hist + sp * bins + hist_bin(m, mmax, bins), 1u);
    species_add<2>(acc, sp, {m, m * m});
  }
  block_sum(acc, red);   // the partial sums and every count are in LDS
  if (tid < S) {
    a.msum[(size_t)o * S + tid] += block_total(red, 2 * tid);
    a.msq[(size_t)o * S + tid] += block_total(red, 2 * tid + 1);
  }
  hist_flush_owned(s_pop, a.pop + (size_t)o * S * Q, S * Q);
  hist_flush_owned(s_trans, a.trans + (size_t)o * S * Q * Q, S * Q * Q);
  hist_flush_owned(s_hist, a.mhist + (size_t)o * S * bins, S * bins);
  if (tid == 0) {
    md_count_sample(a.samples, a.vol_sum, o, md_volume(a.s, o));
    a.skipped[o] += s_skip;
  }
}

// grid (lags of this sample, B); needs L > 0
static __global__ __launch_bounds__(256) void k_md_chg_corr(MdChgArgs a) {
  const int tid = threadIdx.x, l = blockIdx.x, o = blockIdx.y;
  int a0, n;
  if (!md_running(a.s, o, a0, n)) return;
  const MdLag g = md_lag(a.r, a.s.N, a0, l);
  const int S = a.s.S;
  constexpr int Q = MD_CHG_STATES;
  __builtin_assume(S <= MD_OBS_SPECIES);   // checked on the host: the flush of same is one pass
  __shared__ unsigned int s_same[MD_OBS_SPECIES * Q];
  __shared__ double red[4][MD_OBS_SPECIES];
  hist_zero(s_same, MD_OBS_SPECIES * Q);
  __syncthreads();
  double acc[MD_OBS_SPECIES] = {};
  for (int i = tid; i < n; i += 256) {
    const int q1 = a.ring_q[g.row1 + i], q0 = a.ring_q[g.row0 + i];
    if (q1 < 0 || q0 < 0) continue;   // a non-finite moment at either end: the pair is left out
    const int sp = a.s.species[a0 + i];
    if (q1 == q0) atomicAdd(s_same + sp * Q + q1, 1u);
    species_add<1>(acc, sp, {a.ring_m[g.row1 + i] * a.ring_m[g.row0 + i]});
  }
  block_sum(acc, red);
  const size_t cell = (size_t)o * a.r.L + l;
  if (tid < S) a.mcorr[cell * S + tid] += block_total(red, tid);
  hist_flush_owned(s_same, a.same + cell * S * Q, S * Q);
}

// grid (ceil(largest replica / MD_OBS_RDF_ROWS), B), dynamic LDS Q * S * srdf_bins * 4 bytes; rows are keyed by the state of the centre
static __global__ __launch_bounds__(256) void k_md_chg_srdf(MdChgArgs a) {
  extern __shared__ unsigned int s_sh[];
  __shared__ struct { MdImageCell cell; int state[MD_OBS_RDF_ROWS]; } sh;   // one block: the cell, then the key of every centre row
  const int tid = threadIdx.x, o = blockIdx.y, i0 = blockIdx.x * MD_OBS_RDF_ROWS;
  int a0, n;
  if (!md_running(a.s, o, a0, n) || i0 >= n) return;
  if (tid < min(MD_OBS_RDF_ROWS, n - i0)) {   // the state of a centre row, -1 for another species or a non-finite moment
    const int g = a0 + i0 + tid, sp = a.s.species[g];
    sh.state[tid] = sp == a.center ? md_chg_state((double)a.s.mag[g], a.bounds + sp * MD_CHG_BOUNDS, a.n_bounds[sp]) : -1;
  }
  md_pair_histogram(a.s, o, a0, n, i0, [&](int ii) { return sh.state[ii]; }, MD_CHG_STATES, a.srdf_bins, a.srdf_rmax, s_sh, sh.cell, a.shist,
                    nullptr, nullptr);   // its first barrier publishes the keys
}

}  // namespace chg
