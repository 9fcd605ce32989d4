// kernels_lbfgs.h -- one L-BFGS step (ASE's LBFGS with its defaults, no line search) for every active structure of a relaxation
// created by chg_relax_create_lbfgs.  Same generalized coordinates and forces, stop rules and retry protocol as k_relax_step
// (kernels_relax.h), whose thread-0 cell algebra it shares; tests/lbfgs_ref.py restates the step in float64 NumPy and DESIGN.md
// "L-BFGS" gives the state layout.
//
// One workgroup (4 waves) per structure, whatever its size: thread t owns rows t, t + 256, ... of the structure in every pass, so
// the work vector of the two-loop recursion (w, HBM scratch laid out like q) is only ever read and written by the thread that owns
// the row and needs no synchronisation of its own.  Each of the 2 m history passes is one fused sweep over the owned rows (apply the
// previous coefficient, accumulate the next dot product) and one workgroup reduction: xor-shuffle inside the wave, the four wave
// sums through LDS (two alternating slots, so one barrier per pass), added in a fixed order by every thread.  No atomics: the same
// input gives the same bits.  The coefficients a_i of the first loop wait for the second loop in HBM (abuf), written by thread 0 and
// read after at least one barrier.  All state is f64 in HBM; no synchronisation or allocation on the host side.
//
// A structure that stops, or is held back for the retry, is left bit-for-bit untouched (history included): nothing of the state is
// written before the decision.
#pragma once

#include "kernels_relax.h"

namespace chg {

struct LbfgsStepArgs {
  RelaxStepArgs c;        // the evaluated batch, outputs and stop rules; of its state q, sd, si, aoff (v and the FIRE numbers are unused)
  // si: [0] triples appended so far (the ring holds the last min(that, M)), [1] steps taken, [2] status
  double* r0;             // [R, 3] coordinates of the previous evaluation (rows as q)
  double* g0;             // [R, 3] generalized forces of the previous evaluation
  double* S;              // [M, R, 3] ring: s of the k-th triple appended (k from 0) is slot k % M
  double* Y;              // [M, R, 3]
  double* rho;            // [B, M] 1 / (y . s) per slot
  double* abuf;           // [B, M] scratch: a_i of the first loop
  double* w;              // [R, 3] scratch: work vector
  double alpha, damping;
  size_t R;               // N + 3 B
  int M;                  // slots (>= 1)
};

// sum over the workgroup, the same bits in every thread; `slot` alternates between consecutive calls
__device__ __forceinline__ double block_sum_f64(double x, double (*red)[4], int& slot) {
  x = wave_sum_f64(x);
  if ((threadIdx.x & 63) == 0) red[slot][threadIdx.x >> 6] = x;
  __syncthreads();
  const double s = ((red[slot][0] + red[slot][1]) + red[slot][2]) + red[slot][3];
  slot ^= 1;
  return s;
}

// MASK: mk.fixed is set; <false> is the unconstrained kernel, instruction for instruction
template <bool MASK>
static __global__ __launch_bounds__(256) void k_lbfgs_step(LbfgsStepArgs a, RelaxMask mk) {
  const RelaxStepArgs& p = a.c;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int bs = p.sel ? p.sel[blockIdx.x] : blockIdx.x;
  const int o = p.orig ? p.orig[bs] : bs;
  const int a0 = p.aoff[o], n = p.aoff[o + 1] - a0, b0 = p.b_atom_off[bs];
  const size_t row0 = (size_t)a0 + 3 * (size_t)o;
  double* q = p.q + 3 * row0;
  double* r0 = a.r0 + 3 * row0;
  double* g0 = a.g0 + 3 * row0;
  double* w = a.w + 3 * row0;
  double* rho = a.rho + (size_t)a.M * o;
  double* ab = a.abuf + (size_t)a.M * o;
  const double* sd = p.sd + (size_t)RELAX_SD * o;
  int* si = p.si + (size_t)RELAX_SI * o;
  const int nrows = n + (p.relax_cell ? 3 : 0);
  const float* force = p.force + 3 * (size_t)b0;
  const unsigned char* fixed = MASK ? mk.fixed + 3 * (size_t)a0 : nullptr;
  auto hist = [&](double* base, int slot) { return base + 3 * ((size_t)slot * a.R + row0); };

  __shared__ double sF[9], sG[9], sLinv[9];
  __shared__ double red[2][4];
  __shared__ double rmax[4], rys[4];
  __shared__ int rfin[4];
  __shared__ int s_act, s_append, s_napp;   // s_act 0: stop / retry (no move), 1: step; s_napp: triples appended, this step's included

  if (si[2] != RELAX_RUNNING) {   // not an active structure (chg_test_lbfgs_step may hand such states over): report it unchanged
    if (tid == 0) p.status_next[bs] = si[2];
    return;
  }
  const int steps = si[1];
  int finite = 1;
  if (tid == 0) {
    double F[9], G[9], L[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) sLinv[i] = sd[9 + i];
    const float e = p.energy[bs];
    finite = isfinite(e) & cell_frame(sd, q + 3 * (size_t)n, p.stress + 9 * (size_t)bs, p.stress_weight, p.relax_cell, F, G, L);
#pragma unroll
    for (int i = 0; i < 9; ++i) { sF[i] = F[i]; sG[i] = G[i]; }
    if (p.e_out) p.e_out[o] = e;
    if (p.s_out)
      for (int i = 0; i < 9; ++i) p.s_out[9 * (size_t)o + i] = p.stress[9 * (size_t)bs + i];
    if (p.lat_eval)
      for (int i = 0; i < 9; ++i) p.lat_eval[9 * (size_t)o + i] = L[i];
  }
  __syncthreads();

  // pass 0: finiteness, frame of the evaluated configuration, max row |g|^2, y0 . s0
  double gmax = 0.0, ys = 0.0;
  for (int r = tid; r < nrows; r += 256) {
    double g[3];
    gen_force_row(force, sF, sG, n, r, g, held_bits<MASK>(fixed, n, r));
    if (r < n) {
      const float* f = force + 3 * (size_t)r;
      const float m = p.magmom ? p.magmom[b0 + r] : 0.0f;
      finite &= isfinite(f[0]) && isfinite(f[1]) && isfinite(f[2]) && isfinite(m);
      const size_t ro = (size_t)a0 + r;
      if (p.f_out) {   // the reported forces are the masked ones; the finiteness test above saw the raw ones
        const unsigned held = held_bits<MASK>(fixed, n, r);
        p.f_out[3 * ro] = (held & 1u) ? 0.0f : f[0]; p.f_out[3 * ro + 1] = (held & 2u) ? 0.0f : f[1]; p.f_out[3 * ro + 2] = (held & 4u) ? 0.0f : f[2];
      }
      if (p.m_out && p.magmom) p.m_out[ro] = m;
      if (p.frac_eval) {
        const double u0 = q[3 * r], u1 = q[3 * r + 1], u2 = q[3 * r + 2];
#pragma unroll
        for (int j = 0; j < 3; ++j) p.frac_eval[3 * ro + j] = u0 * sLinv[j] + u1 * sLinv[3 + j] + u2 * sLinv[6 + j];
        if (MASK && mk.frac0 && held_bits<MASK>(fixed, n, r) == 7u)   // a fully held atom keeps the fractional coordinates it was given, bit for bit
          for (int j = 0; j < 3; ++j) p.frac_eval[3 * ro + j] = mk.frac0[3 * ro + j];
      }
    }
    finite &= isfinite(g[0]) && isfinite(g[1]) && isfinite(g[2]);
    gmax = fmax(gmax, g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
    if (steps > 0) {
#pragma unroll
      for (int j = 0; j < 3; ++j) ys += (g0[3 * r + j] - g[j]) * (q[3 * r + j] - r0[3 * r + j]);
    }
  }
  gmax = wave_max_f64(gmax);
  ys = wave_sum_f64(ys);
  finite = __all(finite);
  if (lane == 0) { rmax[wv] = gmax; rys[wv] = ys; rfin[wv] = finite; }
  __syncthreads();
  if (tid == 0) {
    gmax = fmax(fmax(rmax[0], rmax[1]), fmax(rmax[2], rmax[3]));
    ys = ((rys[0] + rys[1]) + rys[2]) + rys[3];
    finite = rfin[0] & rfin[1] & rfin[2] & rfin[3];
    int status = RELAX_RUNNING, act = 0;
    if (!finite) {
      if (p.final_try) status = RELAX_NONFINITE;
      else p.retry[bs] = 1;
    } else if (gmax < p.fmax2) {
      status = RELAX_CONVERGED;
    } else if (steps >= p.max_steps) {
      status = RELAX_MAX_STEPS;
    } else {
      act = 1;
      int napp = si[0];
      const int append = steps > 0 && isfinite(ys) && ys != 0.0;   // ASE would divide by zero: the triple is skipped
      if (append) {
        rho[napp % a.M] = 1.0 / ys;
        napp += 1;
      }
      si[0] = napp;
      si[1] = steps + 1;
      s_append = append;
      s_napp = napp;
    }
    si[2] = status;
    p.status_next[bs] = status;
    s_act = act;
  }
  __syncthreads();
  if (!s_act) return;

  // pass 1: the new triple into the ring, r0 <- q, g0 <- g, w <- -g; fused with the first dot product of the recursion
  const int napp = s_napp, m = min(napp, a.M);
  const int newest = napp - 1;            // triple i of the recursion (0 oldest .. m - 1 newest) is appended number napp - m + i
  int slot = 0;
  {
    double* sn = s_append ? hist(a.S, newest % a.M) : nullptr;
    double* yn = s_append ? hist(a.Y, newest % a.M) : nullptr;
    const double* s1 = m > 0 ? hist(a.S, newest % a.M) : nullptr;
    double part = 0.0;
    for (int r = tid; r < nrows; r += 256) {
      double g[3];
      gen_force_row(force, sF, sG, n, r, g, held_bits<MASK>(fixed, n, r));
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int k = 3 * r + j;
        const double qk = q[k];
        if (sn) { sn[k] = qk - r0[k]; yn[k] = g0[k] - g[j]; }
        r0[k] = qk;
        g0[k] = g[j];
        const double t = -g[j];
        w[k] = t;
        if (s1) part += s1[k] * t;      // the newest triple may be the one just written: the same thread wrote this element
      }
    }
    // first loop, newest to oldest: a_i = rho_i (s_i . t); t -= a_i y_i
    for (int i = m - 1; i >= 0; --i) {
      const int sl = (napp - m + i) % a.M;
      const double ai = rho[sl] * block_sum_f64(part, red, slot);
      if (tid == 0) ab[i] = ai;
      const double* y = hist(a.Y, sl);
      const double* sp = i > 0 ? hist(a.S, (napp - m + i - 1) % a.M) : nullptr;
      part = 0.0;
      for (int r = tid; r < nrows; r += 256) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const int k = 3 * r + j;
          const double t = w[k] - ai * y[k];
          w[k] = t;
          if (sp) part += sp[k] * t;
        }
      }
    }
  }
  // z = t / alpha; second loop, oldest to newest: b = rho_i (y_i . z); z += s_i (a_i - b)
  {
    const double h0 = 1.0 / a.alpha;
    const double* y1 = m > 0 ? hist(a.Y, (napp - m) % a.M) : nullptr;
    double part = 0.0;
    for (int r = tid; r < nrows; r += 256) {
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const int k = 3 * r + j;
        const double z = w[k] * h0;
        w[k] = z;
        if (y1) part += y1[k] * z;
      }
    }
    for (int i = 0; i < m; ++i) {
      const int sl = (napp - m + i) % a.M;
      const double b = rho[sl] * block_sum_f64(part, red, slot);
      const double coef = ab[i] - b;    // ab[i]: written by thread 0 before an earlier barrier
      const double* s = hist(a.S, sl);
      const double* yn = i + 1 < m ? hist(a.Y, (napp - m + i + 1) % a.M) : nullptr;
      part = 0.0;
      for (int r = tid; r < nrows; r += 256) {
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const int k = 3 * r + j;
          const double z = w[k] + s[k] * coef;
          w[k] = z;
          if (yn) part += yn[k] * z;
        }
      }
    }
  }
  // p = -z; the longest row of p (cell rows included) is clamped to maxstep
  double longest2 = 0.0;
  for (int r = tid; r < nrows; r += 256) longest2 = fmax(longest2, w[3 * r] * w[3 * r] + w[3 * r + 1] * w[3 * r + 1] + w[3 * r + 2] * w[3 * r + 2]);
  longest2 = wave_max_f64(longest2);
  if (lane == 0) rmax[wv] = longest2;     // last read before the barrier that followed the decision
  __syncthreads();
  const double longest = sqrt(fmax(fmax(rmax[0], rmax[1]), fmax(rmax[2], rmax[3])));
  const double sc = longest >= p.maxstep ? p.maxstep / longest : 1.0;

  // pass 2: (u, X) += damping p, next fractional coordinates u L0^-1 (independent of F)
  for (int r = tid; r < nrows; r += 256) {
#pragma unroll
    for (int j = 0; j < 3; ++j) q[3 * r + j] += a.damping * (-w[3 * r + j] * sc);
    if (r < n) {
      const double u0 = q[3 * r], u1 = q[3 * r + 1], u2 = q[3 * r + 2];
      double* fr = p.frac_next + 3 * ((size_t)b0 + r);
#pragma unroll
      for (int j = 0; j < 3; ++j) fr[j] = u0 * sLinv[j] + u1 * sLinv[3 + j] + u2 * sLinv[6 + j];
      if (MASK && mk.frac0 && held_bits<MASK>(fixed, n, r) == 7u)
        for (int j = 0; j < 3; ++j) fr[j] = mk.frac0[3 * ((size_t)a0 + r) + j];
    }
  }
  __syncthreads();
  if (tid == 0) {
    double L[9];
    next_lattice(sd, q + 3 * (size_t)n, p.relax_cell, L);
#pragma unroll
    for (int i = 0; i < 9; ++i) p.lat_next[9 * (size_t)bs + i] = L[i];
  }
}

}  // namespace chg
