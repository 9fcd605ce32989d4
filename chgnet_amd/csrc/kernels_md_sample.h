// kernels_md_sample.h -- what the observer kernels of kernels_md_obs.h, kernels_md_transport.h and kernels_md_magmom.h share (DESIGN.md
// "MD observables -> Helper layer"): the snapshot and ring views their argument structs embed, and inlined device functions for the
// running-replica check, the lag rows, the species-selected sums with their block reduction, the LDS histograms, the sample count and
// the brute-force pair-image histogram.  Each exists once; every float sum keeps one order: a thread walks i = tid, tid + 256, ..., then
// wave_sum_f64, then the four wave partials left to right, then one plain += by the workgroup that owns the cell.
#pragma once

#include "kernels_md.h"   // MD_RUNNING; mat3.h: det3, inv3, wave_sum_f64

namespace chg {

constexpr int MD_OBS_SPECIES = 8;     // S <= 8
constexpr int MD_OBS_RDF_ROWS = 16;   // atoms i per workgroup of the pair-image kernels

// a completed step (a frame slot of the step kernels, kernels_md.h), never the live state
struct MdSnapshot {
  const double *pos, *mom;   // [N, 3]
  const double* cell;        // [B, 9] rows are the lattice vectors
  const double* mass;        // [N]
  const int* species;        // [N] 0 .. S - 1
  const int* status;         // status of replica o at status[o * status_stride]
  int status_stride;
  const int* aoff;           // [B + 1]
  int N, B, S;
  const float* mag;          // [N] site moments; null for the plain observers
};

// the last L samples: sample number k goes to slot k % L (L may be 0: no ring, slot 0)
struct MdRing {
  double *ring_pos, *ring_vel;   // [L, N, 3]
  double* ring_com;              // [L, B, 3]
  int L, slot;
  long long k;
  int subtract_com;
};

// the atoms a0 .. a0 + n of replica o; false when it is not MD_RUNNING: its frame slot was not written, and it never runs again
__device__ __forceinline__ bool md_running(const MdSnapshot& s, int o, int& a0, int& n) {
  a0 = s.aoff[o];   // read beside the status, not behind it: one round trip less at the head of every kernel
  n = s.aoff[o + 1] - a0;
  return s.status[(size_t)o * s.status_stride] == MD_RUNNING;
}

// lag l of the sample in r.slot: the slot of sample k - l, and the first ring row (in atoms) of the replica at both ends
struct MdLag {
  int then;
  size_t row1, row0;
};
__device__ __forceinline__ MdLag md_lag(const MdRing& r, int N, int a0, int l) {
  const int then = (int)((r.k - l) % r.L);
  return {then, (size_t)r.slot * N + a0, (size_t)then * N + a0};
}
// the centres of mass at both ends of the lag, zero without subtract_com
__device__ __forceinline__ void md_lag_com(const MdRing& r, int B, int o, const MdLag& g, double (&R1)[3], double (&R0)[3]) {
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    R1[j] = r.subtract_com ? r.ring_com[((size_t)r.slot * B + o) * 3 + j] : 0.0;
    R0[j] = r.subtract_com ? r.ring_com[((size_t)g.then * B + o) * 3 + j] : 0.0;
  }
}

// K values of an atom of species sp into acc[K * s + c]: selected, not indexed, so the accumulators stay in registers
template <int K>
__device__ __forceinline__ void species_add(double (&acc)[K * MD_OBS_SPECIES], int sp, const double (&v)[K]) {
#pragma unroll
  for (int s = 0; s < MD_OBS_SPECIES; ++s)
#pragma unroll
    for (int c = 0; c < K; ++c) acc[K * s + c] += sp == s ? v[c] : 0.0;
}

// every accumulator over the workgroup: the wave sums into red[wave][c], then a barrier; block_total adds the four left to right
template <int C>
__device__ __forceinline__ void block_sum(double (&acc)[C], double (&red)[4][C]) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    acc[c] = wave_sum_f64(acc[c]);
    if (lane == 0) red[wv][c] = acc[c];
  }
  __syncthreads();
}
template <int C>
__device__ __forceinline__ double block_total(const double (&red)[4][C], int c) {
  return red[0][c] + red[1][c] + red[2][c] + red[3][c];
}

// LDS histograms of uint32 counts (integer LDS atomics): zero, and the two flushes into 64-bit global counts
__device__ __forceinline__ void hist_zero(unsigned int* h, int cells) {
  for (int c = threadIdx.x; c < cells; c += 256) h[c] = 0u;
}
// the workgroup owns the cells: a plain read-modify-write
template <class T>
__device__ __forceinline__ void hist_flush_owned(const unsigned int* h, T* out, int cells) {
  for (int c = threadIdx.x; c < cells; c += 256) {
    const unsigned int v = h[c];
    if (v) out[c] += v;
  }
}
// several workgroups share the cells: 64-bit integer adds, exact in any order
__device__ __forceinline__ void hist_flush_shared(const unsigned int* h, unsigned long long* out, int cells) {
  for (int c = threadIdx.x; c < cells; c += 256) {
    const unsigned int v = h[c];
    if (v) atomicAdd(out + c, (unsigned long long)v);
  }
}
// a value in [0, top) to its bin
__device__ __forceinline__ int hist_bin(double x, double top, int bins) { return min((int)(x / top * bins), bins - 1); }

// the replica's two scalars, by the one thread of the one workgroup that owns them
__device__ __forceinline__ double md_volume(const MdSnapshot& s, int o) {
  double L[9];
  for (int i = 0; i < 9; ++i) L[i] = s.cell[9 * (size_t)o + i];
  return fabs(det3(L));
}
__device__ __forceinline__ void md_count_sample(long long* samples, double* vol_sum, int o, double vol) {
  samples[o] += 1;
  vol_sum[o] += vol;
}

// the cell of a pair-image pass in LDS: lattice, inverse, rmax over the three heights and the shift bound that follows from it
struct MdImageCell {
  double L[9], Li[9], q[3];
  int m[3];
};

// The pairs (i0 + ii, j), ii < ni, of a running replica with all lattice shifts by brute force, counted in the LDS histogram
// s_hist[(key(ii) * S + species of j) * bins + bin] of rows * S * bins cells (zeroed here) and flushed once into out; a row whose key is
// negative is skipped.  With samples given, the first row chunk counts the sample.  Called by all threads of the workgroup.
template <class Key>
__device__ __forceinline__ void md_pair_histogram(const MdSnapshot& s, int o, int a0, int n, int i0, Key key, int rows, int bins, double rmax,
                                                  unsigned int* s_hist, MdImageCell& sc, unsigned long long* out, long long* samples,
                                                  double* vol_sum) {
  const int tid = threadIdx.x;
  const int S = s.S, cells = rows * S * bins;
  hist_zero(s_hist, cells);
  if (tid == 0) {
    double L[9], Li[9];
    for (int i = 0; i < 9; ++i) L[i] = s.cell[9 * (size_t)o + i];
    inv3(L, Li);
    const double vol = fabs(det3(L));
    for (int i = 0; i < 9; ++i) { sc.L[i] = L[i]; sc.Li[i] = Li[i]; }
    for (int c = 0; c < 3; ++c) {   // height along lattice vector c: the volume over the area of the face the other two span
      const double* u = sc.L + 3 * ((c + 1) % 3);
      const double* v = sc.L + 3 * ((c + 2) % 3);
      const double x = u[1] * v[2] - u[2] * v[1], y = u[2] * v[0] - u[0] * v[2], z = u[0] * v[1] - u[1] * v[0];
      const double q = rmax * sqrt(x * x + y * y + z * z) / vol;   // rmax / h_c
      sc.q[c] = q;
      sc.m[c] = (int)ceil(q) + 1;
    }
    if (samples && blockIdx.x == 0) md_count_sample(samples, vol_sum, o, vol);
  }
  __syncthreads();
  const int ni = min(MD_OBS_RDF_ROWS, n - i0);
  for (int idx = tid; idx < ni * n; idx += 256) {
    const int ii = idx / n, j = idx - ii * n, i = i0 + ii;
    const int row = key(ii);
    if (row < 0) continue;
    const double* ri = s.pos + 3 * ((size_t)a0 + i);
    const double* rj = s.pos + 3 * ((size_t)a0 + j);
    const double dx = rj[0] - ri[0], dy = rj[1] - ri[1], dz = rj[2] - ri[2];
    double w[3];
    int lo[3], hi[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double f = dx * sc.Li[c] + dy * sc.Li[3 + c] + dz * sc.Li[6 + c];
      w[c] = f - floor(f + 0.5);   // [-0.5, 0.5)
      // |w + n| h <= d: shifts outside cannot come under rmax (1e-9 of a lattice vector is far above the rounding of w)
      lo[c] = max(-sc.m[c], (int)ceil(-sc.q[c] - w[c] - 1e-9));
      hi[c] = min(sc.m[c], (int)floor(sc.q[c] - w[c] + 1e-9));
    }
    unsigned int* h = s_hist + (row * S + s.species[a0 + j]) * bins;
    for (int na = lo[0]; na <= hi[0]; ++na)
      for (int nb = lo[1]; nb <= hi[1]; ++nb)
        for (int nc = lo[2]; nc <= hi[2]; ++nc) {
          if (i == j && na == 0 && nb == 0 && nc == 0) continue;
          const double ga = w[0] + na, gb = w[1] + nb, gc = w[2] + nc;
          const double x = ga * sc.L[0] + gb * sc.L[3] + gc * sc.L[6];
          const double y = ga * sc.L[1] + gb * sc.L[4] + gc * sc.L[7];
          const double z = ga * sc.L[2] + gb * sc.L[5] + gc * sc.L[8];
          const double d = sqrt(x * x + y * y + z * z);
          if (d < rmax) atomicAdd(h + hist_bin(d, rmax, bins), 1u);
        }
  }
  __syncthreads();
  hist_flush_shared(s_hist, out + (size_t)o * cells, cells);
}

}  // namespace chg
