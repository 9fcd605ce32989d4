// kernels_neb.h -- one nudged-elastic-band step for every active band of a transition-state search (chg_neb_*): improved tangents
// (Henkelman & Jonsson 2000), spring forces, the climbing image and ONE FIRE optimizer over the interior images of a band.
//
// The semantics are restated in float64 NumPy by tests/neb_ref.py; DESIGN.md "Nudged elastic band" gives the state layout.
//
// One workgroup (4 waves) per band of M images (3 <= M <= NEB_MAX_IMAGES) that share a cell and a species order.  All state is f64 in
// HBM, in ORIGINAL numbering (image i of a band with n atoms per image starts at atom aoff[band_off[k]] + i n); the evaluated batch
// holds the band's images 0..M-1 (all_images, the first evaluation) or 1..M-2 back to back from structure tab[3 j + 1].
//   A  finiteness of everything evaluated; a band that fails is held back (retry flag) or stops, and nothing of it has been written
//   B  energies into LDS (end points of later evaluations from the state), climbing image, tangent weights cp, cm per image
//      (tau = cp t+ + cm t-, not yet normalised)
//   C  one wave per interior image: |t+|^2, |t-|^2, t+.t-, F.t+, F.t- -> the two coefficients of G = F + A t+ + B t-
//   0  G into the arena, the frame of the evaluated configuration, G.v, |G|^2, |v|^2, max row |G|^2 -> decision and FIRE numbers
//   1  v <- c1 v + c2 G + dt G, |dr|^2          2  R += dr (clamped), next fractional coordinates R L^-1 of the interior images
// Every sum is a fixed-order block reduction: the same input gives the same bits.  No synchronisation with the host, no allocation.
#pragma once

#include <hip/hip_runtime.h>

#include "kernels_relax.h"   // RELAX_* statuses, held_bits
#include "mat3.h"            // wave_sum_f64, wave_max_f64

namespace chg {

constexpr int NEB_MIN_IMAGES = 3, NEB_MAX_IMAGES = 66;
constexpr int NEB_SD = 24;   // doubles per band: L[9] L^-1[9] dt a neb_fmax (3 spare)
constexpr int NEB_SI = 4;    // ints per band: Nsteps (FIRE), optimizer steps taken, status, climbing image (-1: none)

struct NebStepArgs {
  // band state, original numbering
  double* r;                    // [N, 3] unwrapped cartesian positions of every image
  double* v;                    // [N, 3] FIRE velocity (rows of the end points are never touched)
  double* g;                    // [N, 3] NEB force of the last evaluated configuration (interior rows)
  double* sd;                   // [n_bands, NEB_SD]
  int* si;                      // [n_bands, NEB_SI]
  float* e_img;                 // [B] energy of every image as last evaluated
  float* f_img;                 // [N, 3] engine force of every image as last evaluated
  double* frac_eval;            // [N, 3] fractional coordinates of the evaluated configuration (interior rows; or null)
  const int* band_off;          // [n_bands + 1] image offsets
  const int* aoff;              // [B + 1] atom offsets of the images
  const unsigned char* fixed;   // [N, 3] 1 = component held; null: none (the <false> instantiation)
  // the evaluated batch
  const float* energy;          // [b]
  const float* force;           // [n, 3]
  const int* b_atom_off;        // [b + 1]
  const int* tab;               // [active, 3] per active band: band, its first structure in the batch, atom offset of its rows in frac_next
  const int* sel;               // [grid] active bands this launch steps (null: all of them)
  double* frac_next;            // [sum (M - 2) n, 3] interior images of the active bands, back to back
  int* status_next;             // [active]
  int* retry;                   // [active] set to 1 (state untouched) when the results are non-finite and final_try == 0
  double fmax2, maxstep, dtmax, finc, fdec, astart, fa, spring;
  int max_steps, nmin, climb, all_images, final_try;
};

// MASK: p.fixed is set
template <bool MASK>
static __global__ __launch_bounds__(256) void k_neb_step(NebStepArgs p) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int j = p.sel ? p.sel[blockIdx.x] : blockIdx.x;
  const int k = p.tab[3 * j], bs0 = p.tab[3 * j + 1];
  const size_t next0 = (size_t)p.tab[3 * j + 2];
  const int i0 = p.band_off[k], M = p.band_off[k + 1] - i0;
  const int a0 = p.aoff[i0], n = p.aoff[i0 + 1] - a0;
  double* sd = p.sd + (size_t)NEB_SD * k;
  int* si = p.si + (size_t)NEB_SI * k;
  const unsigned char* fixed = MASK ? p.fixed + 3 * (size_t)a0 : nullptr;   // image i, atom a: fixed + 3 (i n + a)

  __shared__ float sE[NEB_MAX_IMAGES];
  __shared__ double sCp[NEB_MAX_IMAGES], sCm[NEB_MAX_IMAGES], sA[NEB_MAX_IMAGES], sB[NEB_MAX_IMAGES];
  __shared__ double sLinv[9];
  __shared__ double red[4][4];
  __shared__ double s_c1, s_c2, s_dt, s_scale;
  __shared__ int s_ci, s_act;   // climbing image; 0: stop / retry (no move), 1: step

  if (si[2] != RELAX_RUNNING) {   // not an active band (chg_test_neb_step may hand such states over): report it unchanged
    if (tid == 0) p.status_next[j] = si[2];
    return;
  }
  const int ev0 = p.all_images ? 0 : 1, nev = p.all_images ? M : M - 2;   // evaluated images ev0 .. ev0 + nev - 1
  const float* fb = p.force + 3 * (size_t)p.b_atom_off[bs0];              // image i, atom a: fb + 3 ((i - ev0) n + a)
  const int nint = (M - 2) * n;                                            // interior rows

  // A: finiteness
  int finite = 1;
  for (int i = tid; i < nev; i += 256) finite &= isfinite(p.energy[bs0 + i]) ? 1 : 0;
  for (size_t x = tid, nx = 3 * (size_t)nev * n; x < nx; x += 256) finite &= isfinite(fb[x]) ? 1 : 0;
  finite = __syncthreads_and(finite);
  if (!finite) {
    if (tid == 0) {
      if (p.final_try) si[2] = RELAX_NONFINITE;
      else p.retry[j] = 1;
      p.status_next[j] = p.final_try ? RELAX_NONFINITE : RELAX_RUNNING;
    }
    return;
  }

  // B: energies, climbing image, tangent weights
  for (int i = tid; i < M; i += 256) {
    const bool evaluated = i >= ev0 && i < ev0 + nev;
    const float e = evaluated ? p.energy[bs0 + i - ev0] : p.e_img[i0 + i];
    sE[i] = e;
    if (evaluated) p.e_img[i0 + i] = e;
  }
  if (tid < 9) sLinv[tid] = sd[9 + tid];
  if (p.all_images)   // the end points' forces are reported, never used
    for (int x = tid; x < 3 * n; x += 256) {
      p.f_img[3 * (size_t)a0 + x] = fb[x];
      p.f_img[3 * ((size_t)a0 + (size_t)(M - 1) * n) + x] = fb[3 * (size_t)(M - 1) * n + x];
    }
  __syncthreads();
  if (tid == 0) {
    int ci = -1;
    if (p.climb) {
      ci = 1;
      for (int i = 2; i < M - 1; ++i)
        if (sE[i] > sE[ci]) ci = i;   // the first index wins ties
    }
    s_ci = ci;
  }
  for (int i = 1 + tid; i < M - 1; i += 256) {
    const double ep = (double)sE[i + 1], e0 = (double)sE[i], em = (double)sE[i - 1];
    double cp, cm;
    if (ep > e0 && e0 > em) { cp = 1.0; cm = 0.0; }
    else if (ep < e0 && e0 < em) { cp = 0.0; cm = 1.0; }
    else {
      const double d1 = fabs(ep - e0), d2 = fabs(em - e0), dmax = fmax(d1, d2), dmin = fmin(d1, d2);
      if (ep > em) { cp = dmax; cm = dmin; }
      else { cp = dmin; cm = dmax; }
    }
    sCp[i] = cp; sCm[i] = cm;
  }
  __syncthreads();

  // C: the five sums of every interior image, one wave per image
  const int ci = s_ci;
  for (int i = 1 + wv; i < M - 1; i += 4) {
    const double* r0 = p.r + 3 * ((size_t)a0 + (size_t)i * n);
    const double *rm = r0 - 3 * (size_t)n, *rp = r0 + 3 * (size_t)n;
    const float* f = fb + 3 * (size_t)(i - ev0) * n;
    double pp = 0.0, mm = 0.0, pm = 0.0, fp = 0.0, fm = 0.0;
    for (int a = lane; a < n; a += 64) {
      const unsigned held = held_bits<MASK>(MASK ? fixed + 3 * (size_t)i * n : nullptr, n, a);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double x = r0[3 * a + c], tp = rp[3 * a + c] - x, tm = x - rm[3 * a + c];
        const double fc = (held >> c) & 1u ? 0.0 : (double)f[3 * a + c];
        pp += tp * tp; mm += tm * tm; pm += tp * tm; fp += fc * tp; fm += fc * tm;
      }
    }
    pp = wave_sum_f64(pp); mm = wave_sum_f64(mm); pm = wave_sum_f64(pm); fp = wave_sum_f64(fp); fm = wave_sum_f64(fm);
    if (lane == 0) {
      const double cp = sCp[i], cm = sCm[i];
      const double t2 = cp * cp * pp + 2.0 * cp * cm * pm + cm * cm * mm;   // |cp t+ + cm t-|^2
      const double s = t2 > 0.0 ? 1.0 / sqrt(t2) : 0.0;                     // a tangent of length 0 stays 0
      const double ft = (cp * fp + cm * fm) * s;                            // F . tau
      const double c = (i == ci) ? -2.0 * ft : p.spring * (sqrt(pp) - sqrt(mm)) - ft;
      sA[i] = c * s * cp; sB[i] = c * s * cm;
    }
  }
  __syncthreads();

  // pass 0: G = F + A t+ + B t- (held components 0), frame of the evaluated configuration, G.v, |G|^2, |v|^2, max row |G|^2
  double gv = 0.0, gg = 0.0, vv = 0.0, gmax = 0.0;
  for (int x = tid; x < nint; x += 256) {
    const int i = 1 + x / n, a = x - (i - 1) * n;
    const size_t ro = (size_t)a0 + (size_t)i * n + a;
    const double* r0 = p.r + 3 * ro;
    const double *rm = r0 - 3 * (size_t)n, *rp = r0 + 3 * (size_t)n;
    const float* f = fb + 3 * ((size_t)(i - ev0) * n + a);
    const unsigned held = held_bits<MASK>(MASK ? fixed + 3 * (size_t)i * n : nullptr, n, a);
    const double A = sA[i], B = sB[i];
    double g[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double tp = rp[c] - r0[c], tm = r0[c] - rm[c];
      g[c] = (held >> c) & 1u ? 0.0 : (double)f[c] + A * tp + B * tm;
      p.g[3 * ro + c] = g[c];
      p.f_img[3 * ro + c] = f[c];
    }
    if (p.frac_eval) {
#pragma unroll
      for (int c = 0; c < 3; ++c) p.frac_eval[3 * ro + c] = r0[0] * sLinv[c] + r0[1] * sLinv[3 + c] + r0[2] * sLinv[6 + c];
    }
    const double* vr = p.v + 3 * ro;
    const double rg = g[0] * g[0] + g[1] * g[1] + g[2] * g[2];
    gg += rg;
    gmax = fmax(gmax, rg);
    gv += g[0] * vr[0] + g[1] * vr[1] + g[2] * vr[2];
    vv += vr[0] * vr[0] + vr[1] * vr[1] + vr[2] * vr[2];
  }
  gv = wave_sum_f64(gv); gg = wave_sum_f64(gg); vv = wave_sum_f64(vv); gmax = wave_max_f64(gmax);
  if (lane == 0) { red[wv][0] = gv; red[wv][1] = gg; red[wv][2] = vv; red[wv][3] = gmax; }
  __syncthreads();
  if (tid == 0) {
    gv = red[0][0] + red[1][0] + red[2][0] + red[3][0];
    gg = red[0][1] + red[1][1] + red[2][1] + red[3][1];
    vv = red[0][2] + red[1][2] + red[2][2] + red[3][2];
    gmax = fmax(fmax(red[0][3], red[1][3]), fmax(red[2][3], red[3][3]));
    int status = RELAX_RUNNING, act = 0;
    if (gmax < p.fmax2) {
      status = RELAX_CONVERGED;
    } else if (si[1] >= p.max_steps) {
      status = RELAX_MAX_STEPS;
    } else {
      act = 1;
      double dt = sd[18], a = sd[19], c1 = 0.0, c2 = 0.0;
      int nf = si[0];
      if (si[1] > 0) {                                   // ASE FIRE: the first step starts from v = 0
        if (gv > 0.0) {
          c1 = 1.0 - a;
          c2 = gg > 0.0 ? a * sqrt(vv) / sqrt(gg) : 0.0;
          if (nf > p.nmin) { dt = fmin(dt * p.finc, p.dtmax); a *= p.fa; }
          nf += 1;
        } else {
          a = p.astart; dt *= p.fdec; nf = 0;            // v <- 0
        }
      }
      sd[18] = dt; sd[19] = a; si[0] = nf; si[1] += 1;
      s_c1 = c1; s_c2 = c2; s_dt = dt;
    }
    sd[20] = sqrt(gmax);
    si[2] = status; si[3] = ci;
    p.status_next[j] = status;
    s_act = act;
  }
  __syncthreads();
  if (!s_act) return;

  // pass 1: v <- c1 v + c2 G + dt G, |dr|^2 with dr = dt v
  const double c1 = s_c1, c2 = s_c2, dt = s_dt;
  double* vi = p.v + 3 * ((size_t)a0 + n);   // the interior rows are contiguous
  double* ri = p.r + 3 * ((size_t)a0 + n);
  const double* gi = p.g + 3 * ((size_t)a0 + n);
  double dr2 = 0.0;
  for (int x = tid; x < nint; x += 256) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double gc = gi[3 * (size_t)x + c];
      const double vn = c1 * vi[3 * (size_t)x + c] + c2 * gc + dt * gc;
      vi[3 * (size_t)x + c] = vn;
      const double d = dt * vn;
      dr2 += d * d;
    }
  }
  dr2 = wave_sum_f64(dr2);
  if (lane == 0) red[wv][0] = dr2;
  __syncthreads();
  if (tid == 0) {
    const double nd = sqrt(red[0][0] + red[1][0] + red[2][0] + red[3][0]);
    s_scale = nd > p.maxstep ? p.maxstep / nd : 1.0;
  }
  __syncthreads();

  // pass 2: R += dr (clamped to maxstep over the whole band), next fractional coordinates R L^-1
  const double sc = s_scale;
  for (int x = tid; x < nint; x += 256) {
    double u[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      u[c] = ri[3 * (size_t)x + c] + (dt * vi[3 * (size_t)x + c]) * sc;
      ri[3 * (size_t)x + c] = u[c];
    }
    double* fr = p.frac_next + 3 * (next0 + x);
#pragma unroll
    for (int c = 0; c < 3; ++c) fr[c] = u[0] * sLinv[c] + u[1] * sLinv[3 + c] + u[2] * sLinv[6 + c];
  }
}

}  // namespace chg
