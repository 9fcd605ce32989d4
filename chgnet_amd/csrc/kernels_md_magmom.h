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
// accumulators are selected, never indexed, so nothing lives in scratch.
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
  // snapshot of the sampled step
  const float* mag;          // [N]
  const double* pos;         // [N, 3]
  const double* cell;        // [B, 9]
  const int* species;        // [N]
  const int* status;
  int status_stride;
  const int* aoff;           // [B + 1]
  int N, B, S;
  const double* bounds;      // [S, MD_CHG_BOUNDS]
  const int* n_bounds;       // [S]
  // ring of the last L samples (L may be 0: no lag sums)
  double* ring_m;            // [L, N]
  int* ring_q;               // [L, N]
  int L, slot;
  long long k;
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
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int o = blockIdx.x;
  if (a.status[(size_t)o * a.status_stride] != MD_RUNNING) return;
  const int a0 = a.aoff[o], n = a.aoff[o + 1] - a0;
  const int S = a.S, bins = a.mag_bins;
  constexpr int Q = MD_CHG_STATES;
  __shared__ unsigned int s_hist[MD_CHG_HIST_CELLS];
  __shared__ unsigned int s_pop[MD_OBS_SPECIES * Q], s_trans[MD_OBS_SPECIES * Q * Q], s_skip;
  __shared__ double s_bounds[MD_OBS_SPECIES * MD_CHG_BOUNDS];
  __shared__ int s_nb[MD_OBS_SPECIES];
  __shared__ double red[4][2 * MD_OBS_SPECIES];
  for (int c = tid; c < S * bins; c += 256) s_hist[c] = 0u;
  if (tid < MD_OBS_SPECIES * Q) s_pop[tid] = 0u;
  if (tid < MD_OBS_SPECIES * Q * Q) s_trans[tid] = 0u;
  if (tid < S * MD_CHG_BOUNDS) s_bounds[tid] = a.bounds[tid];
  if (tid < S) s_nb[tid] = a.n_bounds[tid];
  if (tid == 0) s_skip = 0u;
  __syncthreads();
  double acc[2 * MD_OBS_SPECIES];   // sum m of species s at s, sum m^2 at MD_OBS_SPECIES + s
#pragma unroll
  for (int s = 0; s < 2 * MD_OBS_SPECIES; ++s) acc[s] = 0.0;
  const double mmax = a.mag_max;
  const bool first = a.k == 0;
  for (int i = tid; i < n; i += 256) {
    const int g = a0 + i;
    const int sp = a.species[g];
    const double m = (double)a.mag[g];
    const int q = md_chg_state(m, s_bounds + sp * MD_CHG_BOUNDS, s_nb[sp]);
    const int before = first ? -1 : a.prev_q[g];
    a.prev_q[g] = q;
    if (a.L > 0) {
      a.ring_m[(size_t)a.slot * a.N + g] = m;
      a.ring_q[(size_t)a.slot * a.N + g] = q;
    }
    if (q < 0) {
      atomicAdd(&s_skip, 1u);
      continue;
    }
    a.occ[(size_t)g * Q + q] += 1;
    atomicAdd(s_pop + sp * Q + q, 1u);
    if (before >= 0) atomicAdd(s_trans + (sp * Q + before) * Q + q, 1u);
    if (bins > 0 && m >= 0.0 && m < mmax) atomicAdd(s_hist + sp * bins + min((int)(m / mmax * bins), bins - 1), 1u);
#pragma unroll
    for (int s = 0; s < MD_OBS_SPECIES; ++s) {   // selected, not indexed: the accumulators stay in registers
      acc[s] += sp == s ? m : 0.0;
      acc[MD_OBS_SPECIES + s] += sp == s ? m * m : 0.0;
    }
  }
#pragma unroll
  for (int s = 0; s < 2 * MD_OBS_SPECIES; ++s) {
    acc[s] = wave_sum_f64(acc[s]);
    if (lane == 0) red[wv][s] = acc[s];
  }
  __syncthreads();   // the partial sums and every count are in LDS
  if (tid < S) {
    const int v = MD_OBS_SPECIES + tid;
    a.msum[(size_t)o * S + tid] += red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
    a.msq[(size_t)o * S + tid] += red[0][v] + red[1][v] + red[2][v] + red[3][v];
  }
  if (tid < S * Q) {
    const unsigned int v = s_pop[tid];
    if (v) a.pop[(size_t)o * S * Q + tid] += v;
  }
  if (tid < S * Q * Q) {
    const unsigned int v = s_trans[tid];
    if (v) a.trans[(size_t)o * S * Q * Q + tid] += v;
  }
  unsigned long long* out = a.mhist + (size_t)o * S * bins;
  for (int c = tid; c < S * bins; c += 256) {
    const unsigned int v = s_hist[c];
    if (v) out[c] += v;
  }
  if (tid == 0) {
    double L[9];
    for (int i = 0; i < 9; ++i) L[i] = a.cell[9 * (size_t)o + i];
    a.samples[o] += 1;
    a.skipped[o] += s_skip;
    a.vol_sum[o] += fabs(det3(L));
  }
}

// grid (lags of this sample, B); needs L > 0
static __global__ __launch_bounds__(256) void k_md_chg_corr(MdChgArgs a) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int l = blockIdx.x, o = blockIdx.y;
  if (a.status[(size_t)o * a.status_stride] != MD_RUNNING) return;
  const int a0 = a.aoff[o], n = a.aoff[o + 1] - a0;
  const int then = (int)((a.k - l) % a.L);
  const size_t r1 = (size_t)a.slot * a.N + a0, r0 = (size_t)then * a.N + a0;
  const int S = a.S;
  constexpr int Q = MD_CHG_STATES;
  __shared__ unsigned int s_same[MD_OBS_SPECIES * Q];
  __shared__ double red[4][MD_OBS_SPECIES];
  if (tid < MD_OBS_SPECIES * Q) s_same[tid] = 0u;
  __syncthreads();
  double acc[MD_OBS_SPECIES];
#pragma unroll
  for (int s = 0; s < MD_OBS_SPECIES; ++s) acc[s] = 0.0;
  for (int i = tid; i < n; i += 256) {
    const int q1 = a.ring_q[r1 + i], q0 = a.ring_q[r0 + i];
    if (q1 < 0 || q0 < 0) continue;   // a non-finite moment at either end: the pair is left out
    const int sp = a.species[a0 + i];
    const double mm = a.ring_m[r1 + i] * a.ring_m[r0 + i];
    if (q1 == q0) atomicAdd(s_same + sp * Q + q1, 1u);
#pragma unroll
    for (int s = 0; s < MD_OBS_SPECIES; ++s) acc[s] += sp == s ? mm : 0.0;
  }
#pragma unroll
  for (int s = 0; s < MD_OBS_SPECIES; ++s) {
    acc[s] = wave_sum_f64(acc[s]);
    if (lane == 0) red[wv][s] = acc[s];
  }
  __syncthreads();
  const size_t cell = (size_t)o * a.L + l;
  if (tid < S) a.mcorr[cell * S + tid] += red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
  if (tid < S * Q) {
    const unsigned int v = s_same[tid];
    if (v) a.same[cell * S * Q + tid] += v;
  }
}

// grid (ceil(largest replica / MD_OBS_RDF_ROWS), B), dynamic LDS Q * S * srdf_bins * 4 bytes
static __global__ __launch_bounds__(256) void k_md_chg_srdf(MdChgArgs a) {
  extern __shared__ unsigned int s_sh[];
  __shared__ double sL[9], sLi[9], s_q[3];
  __shared__ int s_m[3], s_state[MD_OBS_RDF_ROWS];
  const int tid = threadIdx.x;
  const int o = blockIdx.y;
  if (a.status[(size_t)o * a.status_stride] != MD_RUNNING) return;
  const int a0 = a.aoff[o], n = a.aoff[o + 1] - a0;
  const int i0 = blockIdx.x * MD_OBS_RDF_ROWS;
  if (i0 >= n) return;
  const int S = a.S, bins = a.srdf_bins, cells = MD_CHG_STATES * S * bins;
  const int ni = min(MD_OBS_RDF_ROWS, n - i0);
  for (int c = tid; c < cells; c += 256) s_sh[c] = 0u;
  if (tid < ni) {   // the state of a centre row, -1 for another species or a non-finite moment
    const int g = a0 + i0 + tid, sp = a.species[g];
    s_state[tid] = sp == a.center ? md_chg_state((double)a.mag[g], a.bounds + sp * MD_CHG_BOUNDS, a.n_bounds[sp]) : -1;
  }
  if (tid == 0) {
    double L[9], Li[9];
    for (int i = 0; i < 9; ++i) L[i] = a.cell[9 * (size_t)o + i];
    inv3(L, Li);
    const double vol = fabs(det3(L));
    for (int i = 0; i < 9; ++i) { sL[i] = L[i]; sLi[i] = Li[i]; }
    for (int c = 0; c < 3; ++c) {   // height along lattice vector c: the volume over the area of the face the other two span
      const double* u = sL + 3 * ((c + 1) % 3);
      const double* v = sL + 3 * ((c + 2) % 3);
      const double x = u[1] * v[2] - u[2] * v[1], y = u[2] * v[0] - u[0] * v[2], z = u[0] * v[1] - u[1] * v[0];
      const double q = a.srdf_rmax * sqrt(x * x + y * y + z * z) / vol;   // rmax / h_c
      s_q[c] = q;
      s_m[c] = (int)ceil(q) + 1;
    }
  }
  __syncthreads();
  const double rmax = a.srdf_rmax;
  for (int idx = tid; idx < ni * n; idx += 256) {
    const int ii = idx / n, j = idx - ii * n, i = i0 + ii;
    const int qi = s_state[ii];
    if (qi < 0) continue;
    const double* ri = a.pos + 3 * ((size_t)a0 + i);
    const double* rj = a.pos + 3 * ((size_t)a0 + j);
    const double dx = rj[0] - ri[0], dy = rj[1] - ri[1], dz = rj[2] - ri[2];
    double w[3];
    int lo[3], hi[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double f = dx * sLi[c] + dy * sLi[3 + c] + dz * sLi[6 + c];
      w[c] = f - floor(f + 0.5);   // [-0.5, 0.5)
      // |w + n| h <= d: shifts outside cannot come under rmax (1e-9 of a lattice vector is far above the rounding of w)
      lo[c] = max(-s_m[c], (int)ceil(-s_q[c] - w[c] - 1e-9));
      hi[c] = min(s_m[c], (int)floor(s_q[c] - w[c] + 1e-9));
    }
    unsigned int* h = s_sh + (qi * S + a.species[a0 + j]) * bins;
    for (int na = lo[0]; na <= hi[0]; ++na)
      for (int nb = lo[1]; nb <= hi[1]; ++nb)
        for (int nc = lo[2]; nc <= hi[2]; ++nc) {
          if (i == j && na == 0 && nb == 0 && nc == 0) continue;
          const double ga = w[0] + na, gb = w[1] + nb, gc = w[2] + nc;
          const double x = ga * sL[0] + gb * sL[3] + gc * sL[6];
          const double y = ga * sL[1] + gb * sL[4] + gc * sL[7];
          const double z = ga * sL[2] + gb * sL[5] + gc * sL[8];
          const double d = sqrt(x * x + y * y + z * z);
          if (d < rmax) atomicAdd(h + min((int)(d / rmax * bins), bins - 1), 1u);
        }
  }
  __syncthreads();
  unsigned long long* out = a.shist + (size_t)o * cells;
  for (int c = tid; c < cells; c += 256) {   // several row chunks share a replica's cells: 64-bit integer adds, exact in any order
    const unsigned int v = s_sh[c];
    if (v) atomicAdd(out + c, (unsigned long long)v);
  }
}

}  // namespace chg
