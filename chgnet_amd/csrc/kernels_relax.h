// kernels_relax.h -- one FIRE step through the Frechet cell filter for every active structure of a relaxation (chg_relax_*).
//
// Reference driver replaced (file:line relative to /root/reference/chgnet):
//   StructOptimizer.relax: FIRE(FrechetCellFilter(atoms)).run(fmax, steps)   model/dynamics.py:184-346
// The semantics (generalized coordinates, forces, FIRE branches, stop rules) are restated in float64 NumPy / SciPy by
// tests/relax_ref.py; DESIGN.md "Structure relaxation" gives the state layout.
//
// One workgroup (4 waves) per structure.  Thread 0 does the 3x3 algebra (F = expm(X / c), F^-T, the Frechet derivative of expm
// for the cell rows) in registers; all 256 threads then stream the atom rows twice (pass 0: generalized forces and the FIRE dot
// products; pass 1: new velocity and |dr|^2) and once more to apply the clamped step (pass 2).  All state is f64 in HBM.  No
// synchronisation or allocation: the launch can be graph-captured.
#pragma once

#include <hip/hip_runtime.h>

#include "mat3.h"   // mm3, det3, inv3, wave_sum_f64, wave_max_f64

namespace chg {

enum : int { RELAX_RUNNING = 0, RELAX_CONVERGED = 1, RELAX_MAX_STEPS = 2, RELAX_NONFINITE = 3 };
constexpr int RELAX_SD = 24;   // doubles per structure: L0[9] L0^-1[9] c dt a (3 spare)
constexpr int RELAX_SI = 4;    // ints per structure: Nsteps (FIRE), optimizer steps taken, status (1 spare)

struct RelaxStepArgs {
  // relaxation state, original numbering (rows of structure o start at aoff[o] + 3 o: n atom rows, then 3 cell rows)
  double* q;              // [N + 3B, 3] u (cell relaxation) or cartesian r, then X
  double* v;              // [N + 3B, 3]
  double* sd;             // [B, RELAX_SD]
  int* si;                // [B, RELAX_SI]
  const int* aoff;        // [B + 1]
  // the evaluated batch (batch numbering)
  const float* energy;    // [b]
  const float* force;     // [n, 3]
  const float* stress;    // [b, 9] GPa
  const float* magmom;    // [n] or null
  const int* b_atom_off;  // [b + 1]
  const int* orig;        // [b] batch structure -> original (null: identity)
  const int* sel;         // [grid] batch structures this launch steps (null: all of them, grid = b)
  // frame of the evaluated configuration, original numbering (null: not kept)
  float *e_out, *f_out, *s_out, *m_out;
  double *frac_eval, *lat_eval;
  // next configuration and status, batch numbering
  double* frac_next;      // [n, 3]
  double* lat_next;       // [b, 9]
  int* status_next;       // [b]
  int* retry;             // [b] set to 1 (state untouched) when the results are non-finite and final_try == 0
  double fmax2, maxstep, dtmax, finc, fdec, astart, fa, stress_weight;
  int max_steps, nmin, relax_cell, final_try;
};

// constraint (DESIGN.md "Constraints"), a kernel argument of its own so that the layout of RelaxStepArgs stays what it was
struct RelaxMask {
  const unsigned char* fixed;   // [N, 3] original numbering, 1 = component held; null: none (the <false> instantiations)
  const double* frac0;          // [N, 3] original numbering: the fractional coordinates as given, which a fully held atom keeps (or null)
};

// expm(M) and, when e != null, the Frechet derivative L(M, E) = top-right block of expm([[M, E], [0, M]]).  The 6x6 block matrix is
// kept as its two distinct 3x3 blocks ([[P, Q], [0, P]] is closed under products), scaled by 2^-s until ||M||_1 <= 1/4, summed as a
// degree-14 Taylor polynomial (Horner) and squared back s times ([[P, Q], [0, P]]^2 = [[P^2, PQ + QP], [0, P^2]]).  The truncation
// error of both blocks is below 1e-19 relative (||M / 2^s|| <= 1/4; the Frechet terms carry k ||M||^(k-1) ||E|| / k!).
__device__ inline void expm_frechet3(const double* m, const double* e, double* out_exp, double* out_l) {
  double nrm = 0.0;
#pragma unroll
  for (int j = 0; j < 3; ++j) nrm = fmax(nrm, fabs(m[j]) + fabs(m[3 + j]) + fabs(m[6 + j]));
  int s = 0;
  if (nrm > 0.25) s = min(64, ilogb(nrm) + 3);      // nrm < 2^(ilogb + 1) -> nrm / 2^s < 1/4
  double a[9], b[9], p[9], q[9], t[9], u[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) { a[i] = ldexp(m[i], -s); b[i] = e ? ldexp(e[i], -s) : 0.0; p[i] = (i % 4 == 0) ? 1.0 : 0.0; q[i] = 0.0; }
  // Horner: [[P, Q], [0, P]] <- I + [[A, B], [0, A]] [[P, Q], [0, P]] / k  =  I + [[A P, A Q + B P], [0, A P]] / k
  for (int k = 14; k >= 1; --k) {
    const double rk = 1.0 / k;
    mm3(a, p, t);
    mm3(a, q, u);
    mm3(b, p, q);
#pragma unroll
    for (int i = 0; i < 9; ++i) { q[i] = (u[i] + q[i]) * rk; p[i] = t[i] * rk + ((i % 4 == 0) ? 1.0 : 0.0); }
  }
  for (int r = 0; r < s; ++r) {
    mm3(p, q, t);
    mm3(q, p, u);
#pragma unroll
    for (int i = 0; i < 9; ++i) q[i] = t[i] + u[i];
    mm3(p, p, t);
#pragma unroll
    for (int i = 0; i < 9; ++i) p[i] = t[i];
  }
#pragma unroll
  for (int i = 0; i < 9; ++i) { out_exp[i] = p[i]; if (out_l) out_l[i] = q[i]; }
}

// Thread-0 algebra of one evaluated configuration, shared by the step kernels (k_relax_step, k_lbfgs_step).  sd: L0[9] L0^-1[9] c;
// x: the 3 cell rows X of q; stress: the engine's [9] in GPa.  Out: F = expm(X / c) (identity without the cell), the cell rows
// G = (1/c) L(A^T, W) of the generalized force (zero without the cell) and the cell L = L0 F^T.  Returns whether the stress is finite.
__device__ inline int cell_frame(const double* sd, const double* x, const float* stress, double stress_weight, int relax_cell, double* F,
                                 double* G, double* L) {
  double L0[9], sig[9];
  int finite = 1;
#pragma unroll
  for (int i = 0; i < 9; ++i) L0[i] = sd[i];
#pragma unroll
  for (int i = 0; i < 9; ++i) { const float s = stress[i]; finite &= isfinite(s); sig[i] = (double)s * stress_weight; }
  if (relax_cell) {
    const double c = sd[18], ic = 1.0 / c;
    double A[9], At[9], FinvT[9], W[9], Fi[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) A[i] = x[i] * ic;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) At[3 * i + j] = A[3 * j + i];
    expm_frechet3(A, nullptr, F, nullptr);
#pragma unroll
    for (int i = 0; i < 3; ++i)   // cell = L0 F^T: L[i][j] = sum_k L0[i][k] F[j][k]
#pragma unroll
      for (int j = 0; j < 3; ++j) L[3 * i + j] = L0[3 * i] * F[3 * j] + L0[3 * i + 1] * F[3 * j + 1] + L0[3 * i + 2] * F[3 * j + 2];
    const double vol = fabs(det3(L));
    inv3(F, Fi);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) FinvT[3 * i + j] = Fi[3 * j + i];
    mm3(sig, FinvT, W);
#pragma unroll
    for (int i = 0; i < 9; ++i) W[i] *= -vol;                     // W = -V sigma F^-T
    double scratch[9];
    expm_frechet3(At, W, scratch, G);                             // L(A^T, W)
#pragma unroll
    for (int i = 0; i < 9; ++i) G[i] *= ic;
  } else {
#pragma unroll
    for (int i = 0; i < 9; ++i) { F[i] = (i % 4 == 0) ? 1.0 : 0.0; G[i] = 0.0; L[i] = L0[i]; }
  }
  return finite;
}

// bit j set: component j of atom row r is held (fixed: the structure's [n, 3] mask); cell rows are never held
template <bool MASK>
__device__ __forceinline__ unsigned held_bits(const unsigned char* fixed, int n, int r) {
  if (!MASK || r >= n) return 0u;
  const unsigned char* h = fixed + 3 * (size_t)r;
  return (h[0] ? 1u : 0u) | (h[1] ? 2u : 0u) | (h[2] ? 4u : 0u);
}

// generalized force of row r of a structure with n atoms (atom rows: f F; cell rows: (1/c) L(A^T, W)); force: the structure's [n, 3];
// the engine's force on a held component (bit of `held`) counts as 0
__device__ __forceinline__ void gen_force_row(const float* force, const double* F, const double* G, int n, int r, double g[3],
                                              unsigned held = 0u) {
  if (r < n) {
    const float* f = force + 3 * (size_t)r;
    const double f0 = (held & 1u) ? 0.0 : (double)f[0], f1 = (held & 2u) ? 0.0 : (double)f[1], f2 = (held & 4u) ? 0.0 : (double)f[2];
#pragma unroll
    for (int j = 0; j < 3; ++j) g[j] = f0 * F[j] + f1 * F[3 + j] + f2 * F[6 + j];
  } else {
#pragma unroll
    for (int j = 0; j < 3; ++j) g[j] = G[3 * (r - n) + j];
  }
}

// the cell L0 expm(X / c)^T of the moved coordinates (L0 without the cell)
__device__ inline void next_lattice(const double* sd, const double* x, int relax_cell, double* L) {
  if (relax_cell) {
    double A[9], F[9];
    const double ic = 1.0 / sd[18];
#pragma unroll
    for (int i = 0; i < 9; ++i) A[i] = x[i] * ic;
    expm_frechet3(A, nullptr, F, nullptr);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) L[3 * i + j] = sd[3 * i] * F[3 * j] + sd[3 * i + 1] * F[3 * j + 1] + sd[3 * i + 2] * F[3 * j + 2];
  } else {
#pragma unroll
    for (int i = 0; i < 9; ++i) L[i] = sd[i];
  }
}

// MASK: mk.fixed is set; <false> is the unconstrained kernel, instruction for instruction
template <bool MASK>
static __global__ __launch_bounds__(256) void k_relax_step(RelaxStepArgs p, RelaxMask mk) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int bs = p.sel ? p.sel[blockIdx.x] : blockIdx.x;
  const int o = p.orig ? p.orig[bs] : bs;
  const int a0 = p.aoff[o], n = p.aoff[o + 1] - a0, b0 = p.b_atom_off[bs];
  double* q = p.q + 3 * ((size_t)a0 + 3 * (size_t)o);
  double* v = p.v + 3 * ((size_t)a0 + 3 * (size_t)o);
  double* sd = p.sd + (size_t)RELAX_SD * o;
  int* si = p.si + (size_t)RELAX_SI * o;
  const int nrows = n + (p.relax_cell ? 3 : 0);
  const unsigned char* fixed = MASK ? mk.fixed + 3 * (size_t)a0 : nullptr;

  __shared__ double sF[9], sG[9], sLinv[9];
  __shared__ double red[4][4];
  __shared__ int rfin[4];
  __shared__ double s_c1, s_c2, s_dt, s_scale;
  __shared__ int s_act;   // 0: stop / retry (no move), 1: step

  if (si[2] != RELAX_RUNNING) {   // not an active structure (chg_test_relax_step may hand such states over): report it unchanged
    if (tid == 0) p.status_next[bs] = si[2];
    return;
  }
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

  auto gen_force = [&](int r, double g[3]) { gen_force_row(p.force + 3 * (size_t)b0, sF, sG, n, r, g, held_bits<MASK>(fixed, n, r)); };

  // pass 0: finiteness, frame of the evaluated configuration, g.v, |g|^2, |v|^2, max row |g|^2
  double gv = 0.0, gg = 0.0, vv = 0.0, gmax = 0.0;
  for (int r = tid; r < nrows; r += 256) {
    double g[3];
    gen_force(r, g);
    if (r < n) {
      const float* f = p.force + 3 * ((size_t)b0 + r);
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
    const double rg = g[0] * g[0] + g[1] * g[1] + g[2] * g[2];
    gg += rg;
    gmax = fmax(gmax, rg);
    gv += g[0] * v[3 * r] + g[1] * v[3 * r + 1] + g[2] * v[3 * r + 2];
    vv += v[3 * r] * v[3 * r] + v[3 * r + 1] * v[3 * r + 1] + v[3 * r + 2] * v[3 * r + 2];
  }
  gv = wave_sum_f64(gv); gg = wave_sum_f64(gg); vv = wave_sum_f64(vv); gmax = wave_max_f64(gmax);
  finite = __all(finite);
  if (lane == 0) { red[wv][0] = gv; red[wv][1] = gg; red[wv][2] = vv; red[wv][3] = gmax; rfin[wv] = finite; }
  __syncthreads();
  if (tid == 0) {
    gv = red[0][0] + red[1][0] + red[2][0] + red[3][0];
    gg = red[0][1] + red[1][1] + red[2][1] + red[3][1];
    vv = red[0][2] + red[1][2] + red[2][2] + red[3][2];
    gmax = fmax(fmax(red[0][3], red[1][3]), fmax(red[2][3], red[3][3]));
    finite = rfin[0] & rfin[1] & rfin[2] & rfin[3];
    int status = RELAX_RUNNING, act = 0;
    if (!finite) {
      if (p.final_try) status = RELAX_NONFINITE;
      else p.retry[bs] = 1;
    } else if (gmax < p.fmax2) {
      status = RELAX_CONVERGED;
    } else if (si[1] >= p.max_steps) {
      status = RELAX_MAX_STEPS;
    } else {
      act = 1;
      double dt = sd[19], a = sd[20], c1 = 0.0, c2 = 0.0;
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
      sd[19] = dt; sd[20] = a; si[0] = nf; si[1] += 1;
      s_c1 = c1; s_c2 = c2; s_dt = dt;
    }
    si[2] = status;
    p.status_next[bs] = status;
    s_act = act;
  }
  __syncthreads();
  if (!s_act) return;

  // pass 1: v <- c1 v + c2 g + dt g, |dr|^2 with dr = dt v
  const double c1 = s_c1, c2 = s_c2, dt = s_dt;
  double dr2 = 0.0;
  for (int r = tid; r < nrows; r += 256) {
    double g[3];
    gen_force(r, g);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double vn = c1 * v[3 * r + j] + c2 * g[j] + dt * g[j];
      v[3 * r + j] = vn;
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

  // pass 2: (u, X) += dr (clamped to maxstep), next fractional coordinates u L0^-1 (independent of F)
  const double sc = s_scale;
  for (int r = tid; r < nrows; r += 256) {
#pragma unroll
    for (int j = 0; j < 3; ++j) q[3 * r + j] += (dt * v[3 * r + j]) * sc;
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
