// kernels_dimer.h -- one dimer step for every active saddle search (chg_dimer_*): the rotation of the axis by one trial angle and a
// Fourier fit of the curvature (Heyden, Bell & Keil 2005), the force extrapolation of Kaestner & Sherwood (2008) and ONE FIRE
// optimizer on the modified force (Henkelman & Jonsson 1999) of the centre.
//
// The semantics are restated in float64 NumPy by tests/dimer_ref.py; DESIGN.md "Dimer saddle search" gives the state layout.
//
// One workgroup (4 waves) per search of n atoms in a fixed cell.  All state is f64 in HBM, in ORIGINAL numbering (search k owns the
// rows aoff[k] .. aoff[k + 1] of r, nvec, theta, v, f0, f1).  The evaluated batch holds, from structure tab[4 j + 1], the centre R and
// R + delta N (phase PROBE, two structures) or R + delta N* alone (phase TRIAL, N* = N cos phi1 + Theta sin phi1).
//   A  finiteness of everything evaluated; a search that fails is held back (retry flag) or stops, and nothing of it has been written
//   T  TRIAL only: Ct = (F0 - F1t).N* / delta -> the fit (thread 0) -> F1 extrapolated to the angle of the minimum, N rotated there
//   P  PROBE only: F0, F1 <- the results (held components 0)
//   1  d.N, F0.N, max row |F0|^2 (d = F1 - F0)          2  |g|^2 with g = (d - (d.N) N) / delta -> C0, gn, phi1 and the decision
//   R  another rotation: Theta = g / gn, the next fractional coordinates of R + delta N* (one image), phase TRIAL
//   3  translation: G.v, |G|^2, |v|^2 -> FIRE numbers   4  v <- c1 v + c2 G + dt G, |dr|^2
//   5  R += dr (clamped), next fractional coordinates of R and R + delta N (two images), phase PROBE
// Every sum is a fixed-order block reduction: the same input gives the same bits.  No synchronisation with the host, no allocation.
#pragma once

#include <hip/hip_runtime.h>

#include "kernels_relax.h"   // RELAX_* statuses, held_bits
#include "mat3.h"            // wave_sum_f64, wave_max_f64

namespace chg {

constexpr int DIMER_SD = 24;   // doubles per search: L[9] L^-1[9] dt a C0 gn phi1 fmax
constexpr int DIMER_SI = 8;    // ints per search: Nsteps (FIRE), translations taken, status, phase, rotations since the last translation,
                               // rotations in all (2 spare)
enum : int { DIMER_PROBE = 0, DIMER_TRIAL = 1 };
constexpr int DIMER_MAX_ROTATIONS = 32;

struct DimerStepArgs {
  // search state, original numbering
  double* r;                    // [N, 3] unwrapped cartesian positions of the centre
  double* nvec;                 // [N, 3] the axis, a unit vector over the 3 n components of a search
  double* theta;                // [N, 3] unit direction of the rotation in progress
  double* v;                    // [N, 3] FIRE velocity
  double* f0;                   // [N, 3] force at R as last evaluated (held components 0)
  double* f1;                   // [N, 3] force at R + delta N, evaluated or extrapolated (held components 0)
  double* sd;                   // [searches, DIMER_SD]
  int* si;                      // [searches, DIMER_SI]
  float* e_img;                 // [searches, 2] energies as last evaluated: the centre (last PROBE), the displaced or trial image
  float* f_img;                 // [2 N, 3] the engine's forces as last evaluated, 2 n rows per search: the centre, then the other image
  const int* aoff;              // [searches + 1] atom offsets
  const unsigned char* fixed;   // [N, 3] 1 = component held; null: none (the <false> instantiation)
  // the evaluated batch
  const float* energy;          // [b]
  const float* force;           // [n, 3]
  const int* b_atom_off;        // [b + 1]
  const int* tab;               // [active, 4] per active search: search, its first structure in the batch, structures evaluated (1 or 2),
                                // row offset of its images in frac_next (2 n rows are its own)
  const int* sel;               // [grid] active searches this launch steps (null: all of them)
  double* frac_next;            // rows of the next evaluation: two images after a translation, one after a rotation decision
  int* status_next;             // [active]
  int* phase_next;              // [active]
  int* retry;                   // [active] set to 1 (state untouched) when the results are non-finite and final_try == 0
  double fmax2, maxstep, dtmax, finc, fdec, astart, fa, delta, angle_tol;
  int max_steps, nmin, max_rotations, final_try;
};

// the four wave partials of up to three sums, in order; every thread returns with the totals.  red is reused: the leading barrier
// keeps a wave from overwriting partials another one still reads
template <int K>
__device__ __forceinline__ void block_sums(double (&x)[K], double (*red)[4], int lane, int wv) {
  __syncthreads();
#pragma unroll
  for (int i = 0; i < K; ++i) {
    x[i] = wave_sum_f64(x[i]);
    if (lane == 0) red[i][wv] = x[i];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < K; ++i) x[i] = ((red[i][0] + red[i][1]) + red[i][2]) + red[i][3];
}

// MASK: p.fixed is set
template <bool MASK>
static __global__ __launch_bounds__(256) void k_dimer_step(DimerStepArgs p) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int j = p.sel ? p.sel[blockIdx.x] : blockIdx.x;
  const int k = p.tab[4 * j], bs0 = p.tab[4 * j + 1], nev = p.tab[4 * j + 2];
  const size_t next0 = (size_t)p.tab[4 * j + 3];
  const int a0 = p.aoff[k], n = p.aoff[k + 1] - a0, nx = 3 * n;
  double* sd = p.sd + (size_t)DIMER_SD * k;
  int* si = p.si + (size_t)DIMER_SI * k;
  const unsigned char* fixed = MASK ? p.fixed + 3 * (size_t)a0 : nullptr;
  double* R = p.r + 3 * (size_t)a0;
  double* Nv = p.nvec + 3 * (size_t)a0;
  double* Th = p.theta + 3 * (size_t)a0;
  double* V = p.v + 3 * (size_t)a0;
  double* F0 = p.f0 + 3 * (size_t)a0;
  double* F1 = p.f1 + 3 * (size_t)a0;
  float* Fi = p.f_img + 6 * (size_t)a0;

  __shared__ double red[3][4];
  __shared__ double sLinv[9];
  __shared__ double s_x[4];     // scalars thread 0 hands to the block
  __shared__ int s_act;         // 0: stop (no move), 1: rotate, 2: translate

  if (si[2] != RELAX_RUNNING) {   // not an active search (chg_test_dimer_step may hand such states over): report it unchanged
    if (tid == 0) { p.status_next[j] = si[2]; p.phase_next[j] = si[3]; }
    return;
  }
  const int phase = si[3];
  const float* fb = p.force + 3 * (size_t)p.b_atom_off[bs0];   // structure i of the search, component x: fb[i nx + x]

  // A: finiteness
  int finite = 1;
  if (tid < nev) finite &= isfinite(p.energy[bs0 + tid]) ? 1 : 0;
  for (int x = tid; x < nev * nx; x += 256) finite &= isfinite(fb[x]) ? 1 : 0;
  finite = __syncthreads_and(finite);
  if (!finite) {
    if (tid == 0) {
      if (p.final_try) si[2] = RELAX_NONFINITE;
      else p.retry[j] = 1;
      p.status_next[j] = p.final_try ? RELAX_NONFINITE : RELAX_RUNNING;
      p.phase_next[j] = phase;
    }
    return;
  }
  if (tid < 9) sLinv[tid] = sd[9 + tid];
  auto held = [&](int x) { return MASK && fixed[x] != 0; };
  const double delta = p.delta;
  double nscale = 1.0;          // TRIAL: 1 / |N cos phim + Theta sin phim|, applied in pass 1

  if (phase == DIMER_TRIAL) {
    // T: curvature along the trial axis, the fit, the extrapolated F1 and the rotated axis (normalised in pass 1)
    const double phi1 = sd[22], c1 = cos(phi1), s1 = sin(phi1);
    double t[1] = {0.0};
    for (int x = tid; x < nx; x += 256) {
      const double f1t = held(x) ? 0.0 : (double)fb[x];
      t[0] += (F0[x] - f1t) * (Nv[x] * c1 + Th[x] * s1);
      Fi[nx + x] = fb[x];
    }
    if (tid == 0) p.e_img[2 * k + 1] = p.energy[bs0];
    block_sums(t, red, lane, wv);
    if (tid == 0) {
      const double C0 = sd[20], Ct = t[0] / delta, b1 = -sd[21];
      const double a1 = (C0 - Ct + b1 * sin(2.0 * phi1)) / (1.0 - cos(2.0 * phi1));
      const double mean = C0 - a1;
      double phim = 0.5 * atan2(b1, a1);
      if (mean + a1 * cos(2.0 * phim) + b1 * sin(2.0 * phim) > mean) phim += phim <= 0.0 ? M_PI / 2 : -M_PI / 2;   // a maximum of the fit
      s_x[0] = phim;
      s_x[1] = sin(phi1 - phim) / s1;
      s_x[2] = sin(phim) / s1;
      s_x[3] = 1.0 - cos(phim) - sin(phim) * tan(0.5 * phi1);
    }
    __syncthreads();
    const double phim = s_x[0], cA = s_x[1], cB = s_x[2], cC = s_x[3], cm = cos(phim), sm = sin(phim);
    double q[1] = {0.0};
    for (int x = tid; x < nx; x += 256) {
      const double f1t = held(x) ? 0.0 : (double)fb[x];
      F1[x] = cA * F1[x] + cB * f1t + cC * F0[x];
      const double nn = Nv[x] * cm + Th[x] * sm;
      Nv[x] = nn;
      q[0] += nn * nn;
    }
    block_sums(q, red, lane, wv);
    nscale = 1.0 / sqrt(q[0]);
  } else {
    // P: the results become F0 and F1
    for (int x = tid; x < nx; x += 256) {
      const bool h = held(x);
      F0[x] = h ? 0.0 : (double)fb[x];
      F1[x] = h ? 0.0 : (double)fb[nx + x];
      Fi[x] = fb[x];
      Fi[nx + x] = fb[nx + x];
    }
    if (tid == 0) { p.e_img[2 * k] = p.energy[bs0]; p.e_img[2 * k + 1] = p.energy[bs0 + 1]; }
  }

  // pass 1: d.N, F0.N (the loops over components give every thread the components it wrote itself above), then, after the barriers
  // of the sums, max row |F0|^2 over rows other threads wrote
  double s1[2] = {0.0, 0.0}, f2max = 0.0;
  for (int x = tid; x < nx; x += 256) {
    double nn = Nv[x];
    if (phase == DIMER_TRIAL) { nn *= nscale; Nv[x] = nn; }
    const double f0 = F0[x];
    s1[0] += (F1[x] - f0) * nn;
    s1[1] += f0 * nn;
  }
  block_sums(s1, red, lane, wv);
  const double dn = s1[0], f0n = s1[1];
  for (int a = tid; a < n; a += 256) {
    const double* f = F0 + 3 * (size_t)a;
    f2max = fmax(f2max, f[0] * f[0] + f[1] * f[1] + f[2] * f[2]);
  }
  f2max = wave_max_f64(f2max);
  if (lane == 0) red[2][wv] = f2max;   // red[2] is no part of the sums before pass 3
  __syncthreads();
  f2max = fmax(fmax(red[2][0], red[2][1]), fmax(red[2][2], red[2][3]));

  // pass 2: |g|^2
  double s2[1] = {0.0};
  for (int x = tid; x < nx; x += 256) {
    const double g = ((F1[x] - F0[x]) - dn * Nv[x]) / delta;
    s2[0] += g * g;
  }
  block_sums(s2, red, lane, wv);
  const double C0 = -dn / delta, gn = sqrt(s2[0]), phi1 = 0.5 * atan2(gn, fabs(C0));
  const int rot = si[4] + (phase == DIMER_TRIAL ? 1 : 0);
  const bool rotate = rot < p.max_rotations && phi1 >= p.angle_tol;
  __syncthreads();              // every thread has read si[4] and sd before thread 0 writes them
  if (tid == 0) {
    sd[20] = C0; sd[21] = gn; sd[22] = phi1; sd[23] = sqrt(f2max);
    si[4] = rot;
    if (phase == DIMER_TRIAL) si[5] += 1;
  }
  if (rotate) {
    // R: the next trial image
    const double c1 = cos(phi1), sn1 = sin(phi1);
    for (int a = tid; a < n; a += 256) {
      double u[3];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const int x = 3 * a + c;
        const double th = (((F1[x] - F0[x]) - dn * Nv[x]) / delta) / gn;
        Th[x] = th;
        u[c] = R[x] + delta * (Nv[x] * c1 + th * sn1);
      }
      double* fr = p.frac_next + 3 * (next0 + a);
#pragma unroll
      for (int c = 0; c < 3; ++c) fr[c] = u[0] * sLinv[c] + u[1] * sLinv[3 + c] + u[2] * sLinv[6 + c];
    }
    if (tid == 0) { si[3] = DIMER_TRIAL; p.status_next[j] = RELAX_RUNNING; p.phase_next[j] = DIMER_TRIAL; }
    return;
  }

  // pass 3: the modified force G = F0 - 2 (F0.N) N (negative curvature) or -(F0.N) N; G.v, |G|^2, |v|^2
  const double gA = C0 < 0.0 ? 1.0 : 0.0, gB = C0 < 0.0 ? -2.0 * f0n : -f0n;
  double s3[3] = {0.0, 0.0, 0.0};
  for (int x = tid; x < nx; x += 256) {
    const double g = gA * F0[x] + gB * Nv[x], vx = V[x];
    s3[0] += g * vx; s3[1] += g * g; s3[2] += vx * vx;
  }
  block_sums(s3, red, lane, wv);
  if (tid == 0) {
    int status = RELAX_RUNNING, act = 0;
    if (C0 < 0.0 && f2max < p.fmax2) {
      status = RELAX_CONVERGED;
    } else if (si[1] >= p.max_steps) {
      status = RELAX_MAX_STEPS;
    } else {
      act = 2;
      double dt = sd[18], a = sd[19], c1 = 0.0, c2 = 0.0;
      int nf = si[0];
      if (si[1] > 0) {                                   // ASE FIRE: the first step starts from v = 0
        if (s3[0] > 0.0) {
          c1 = 1.0 - a;
          c2 = s3[1] > 0.0 ? a * sqrt(s3[2]) / sqrt(s3[1]) : 0.0;
          if (nf > p.nmin) { dt = fmin(dt * p.finc, p.dtmax); a *= p.fa; }
          nf += 1;
        } else {
          a = p.astart; dt *= p.fdec; nf = 0;            // v <- 0
        }
      }
      sd[18] = dt; sd[19] = a; si[0] = nf; si[1] += 1;
      si[3] = DIMER_PROBE; si[4] = 0;
      s_x[0] = c1; s_x[1] = c2; s_x[2] = dt;
    }
    si[2] = status;
    p.status_next[j] = status;
    p.phase_next[j] = act ? DIMER_PROBE : phase;
    s_act = act;
  }
  __syncthreads();
  if (!s_act) return;

  // pass 4: v <- c1 v + c2 G + dt G, |dr|^2 with dr = dt v
  const double c1 = s_x[0], c2 = s_x[1], dt = s_x[2];
  double s4[1] = {0.0};
  for (int x = tid; x < nx; x += 256) {
    const double g = gA * F0[x] + gB * Nv[x];
    const double vn = c1 * V[x] + c2 * g + dt * g;
    V[x] = vn;
    const double d = dt * vn;
    s4[0] += d * d;
  }
  block_sums(s4, red, lane, wv);
  const double nd = sqrt(s4[0]), sc = nd > p.maxstep ? p.maxstep / nd : 1.0;

  // pass 5: R += dr (clamped to maxstep over the whole search), next fractional coordinates of R and of R + delta N
  for (int a = tid; a < n; a += 256) {
    double u[3], w[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const int x = 3 * a + c;
      u[c] = R[x] + (dt * V[x]) * sc;
      R[x] = u[c];
      w[c] = u[c] + delta * Nv[x];
    }
    double* fr = p.frac_next + 3 * (next0 + a);
    double* fr1 = fr + 3 * (size_t)n;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      fr[c] = u[0] * sLinv[c] + u[1] * sLinv[3 + c] + u[2] * sLinv[6 + c];
      fr1[c] = w[0] * sLinv[c] + w[1] * sLinv[3 + c] + w[2] * sLinv[6 + c];
    }
  }
}

}  // namespace chg
