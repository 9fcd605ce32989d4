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
// Float64 throughout; the per-species accumulators are selected, never indexed, so nothing lives in scratch.
#pragma once

#include "kernels_md.h"   // MD_RUNNING; mat3.h: det3, inv3, wave_sum_f64

namespace chg {

constexpr int MD_OBS_SPECIES = 8;        // S <= 8
constexpr int MD_OBS_MAX_LAGS = 4096;    // L <= 4096
constexpr int MD_OBS_RDF_CELLS = 16384;  // S * S * bins: 64 KB of uint32 counts in LDS
constexpr int MD_OBS_RDF_ROWS = 16;      // atoms i per workgroup of k_md_obs_rdf

struct MdObsArgs {
  // snapshot of the completed step
  const double *pos, *mom;   // [N, 3]
  const double* cell;        // [B, 9] rows are the lattice vectors
  const double* mass;        // [N]
  const int* species;        // [N] 0 .. S - 1
  const int* status;         // status of replica o at status[o * status_stride]
  int status_stride;
  const int* aoff;           // [B + 1]
  int N, B, S;
  // MSD / VACF: ring of L slots, sample number k goes to slot k % L
  double *ring_pos, *ring_vel;   // [L, N, 3]
  double* ring_com;              // [L, B, 3]
  int L, slot;
  long long k;
  int subtract_com;
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
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int o = blockIdx.x;
  if (a.status[(size_t)o * a.status_stride] != MD_RUNNING) return;
  const int a0 = a.aoff[o], n = a.aoff[o + 1] - a0;
  const size_t row = ((size_t)a.slot * a.N + a0) * 3;
  __shared__ double red[4][4];
  // the centre of mass relative to the replica's first atom: the sum carries displacements, not unwrapped positions that may lie
  // thousands of cells away, and a single atom is its own centre of mass exactly
  const double x0[3] = {a.pos[3 * (size_t)a0], a.pos[3 * (size_t)a0 + 1], a.pos[3 * (size_t)a0 + 2]};
  double acc[4] = {0.0, 0.0, 0.0, 0.0};   // sum m (r - r_0), sum m
  for (int i = tid; i < n; i += 256) {
    const double m = a.mass[a0 + i];
    const size_t g = 3 * ((size_t)a0 + i);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double x = a.pos[g + j];
      a.ring_pos[row + 3 * (size_t)i + j] = x;
      a.ring_vel[row + 3 * (size_t)i + j] = a.mom[g + j] / m;
      acc[j] += m * (x - x0[j]);
    }
    acc[3] += m;
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = wave_sum_f64(acc[j]);
  if (lane == 0)
    for (int j = 0; j < 4; ++j) red[wv][j] = acc[j];
  __syncthreads();
  if (tid < 3) {
    const double M = red[0][3] + red[1][3] + red[2][3] + red[3][3];
    a.ring_com[((size_t)a.slot * a.B + o) * 3 + tid] = a.pos[3 * (size_t)a0 + tid] + (red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid]) / M;
  }
}

// grid (lags of this sample, B)
static __global__ __launch_bounds__(256) void k_md_obs_corr(MdObsArgs a) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int l = blockIdx.x, o = blockIdx.y;
  if (a.status[(size_t)o * a.status_stride] != MD_RUNNING) return;
  const int a0 = a.aoff[o], n = a.aoff[o + 1] - a0;
  const int then = (int)((a.k - l) % a.L);
  const size_t r1 = ((size_t)a.slot * a.N + a0) * 3, r0 = ((size_t)then * a.N + a0) * 3;
  double R1[3], R0[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    R1[j] = a.subtract_com ? a.ring_com[((size_t)a.slot * a.B + o) * 3 + j] : 0.0;
    R0[j] = a.subtract_com ? a.ring_com[((size_t)then * a.B + o) * 3 + j] : 0.0;
  }
  __shared__ double red[4][2 * MD_OBS_SPECIES];
  double acc[2 * MD_OBS_SPECIES];
#pragma unroll
  for (int s = 0; s < 2 * MD_OBS_SPECIES; ++s) acc[s] = 0.0;
  for (int i = tid; i < n; i += 256) {
    const int sp = a.species[a0 + i];
    double d2 = 0.0, vv = 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double d = (a.ring_pos[r1 + 3 * (size_t)i + j] - R1[j]) - (a.ring_pos[r0 + 3 * (size_t)i + j] - R0[j]);
      d2 += d * d;
      vv += a.ring_vel[r1 + 3 * (size_t)i + j] * a.ring_vel[r0 + 3 * (size_t)i + j];
    }
#pragma unroll
    for (int s = 0; s < MD_OBS_SPECIES; ++s) {   // selected, not indexed: the accumulators stay in registers
      acc[s] += sp == s ? d2 : 0.0;
      acc[MD_OBS_SPECIES + s] += sp == s ? vv : 0.0;
    }
  }
#pragma unroll
  for (int s = 0; s < 2 * MD_OBS_SPECIES; ++s) {
    acc[s] = wave_sum_f64(acc[s]);
    if (lane == 0) red[wv][s] = acc[s];
  }
  __syncthreads();
  const size_t cell = (size_t)o * a.L + l;
  if (tid < a.S) {
    a.msd[cell * a.S + tid] += red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
    const int v = MD_OBS_SPECIES + tid;
    a.vacf[cell * a.S + tid] += red[0][v] + red[1][v] + red[2][v] + red[3][v];
  }
  if (tid == 0) a.cnt[cell] += 1;
}

// grid (ceil(largest replica / MD_OBS_RDF_ROWS), B), dynamic LDS S * S * bins * 4 bytes
static __global__ __launch_bounds__(256) void k_md_obs_rdf(MdObsArgs a) {
  extern __shared__ unsigned int s_hist[];
  __shared__ double sL[9], sLi[9], s_q[3];
  __shared__ int s_m[3];
  const int tid = threadIdx.x;
  const int o = blockIdx.y;
  if (a.status[(size_t)o * a.status_stride] != MD_RUNNING) return;
  const int a0 = a.aoff[o], n = a.aoff[o + 1] - a0;
  const int i0 = blockIdx.x * MD_OBS_RDF_ROWS;
  if (i0 >= n) return;
  const int S = a.S, bins = a.bins, cells = S * S * bins;
  for (int c = tid; c < cells; c += 256) s_hist[c] = 0u;
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
      const double q = a.rmax * sqrt(x * x + y * y + z * z) / vol;   // rmax / h_c
      s_q[c] = q;
      s_m[c] = (int)ceil(q) + 1;
    }
    if (blockIdx.x == 0) {   // this workgroup alone owns the replica's two scalars
      a.rdf_samples[o] += 1;
      a.vol_sum[o] += vol;
    }
  }
  __syncthreads();
  const int ni = min(MD_OBS_RDF_ROWS, n - i0);
  const double rmax = a.rmax;
  for (int idx = tid; idx < ni * n; idx += 256) {
    const int ii = idx / n, j = idx - ii * n, i = i0 + ii;
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
    unsigned int* h = s_hist + (a.species[a0 + i] * S + a.species[a0 + j]) * bins;
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
  unsigned long long* out = a.hist + (size_t)o * cells;
  for (int c = tid; c < cells; c += 256) {
    const unsigned int v = s_hist[c];
    if (v) atomicAdd(out + c, (unsigned long long)v);
  }
}

}  // namespace chg
