// kernels_md.h -- one molecular-dynamics step kernel for every replica of a batched MD run (chg_md_*).
//
// Reference driver replaced (file:line relative to /root/reference/chgnet):
//   MolecularDynamics: ASE VelocityVerlet / NVTBerendsen / Inhomogeneous_NPTBerendsen / NPTBerendsen   model/dynamics.py:433-780
// tests/md_ref.py restates the semantics in float64 NumPy; DESIGN.md "Molecular dynamics" gives the state layout.
//
// One workgroup (4 waves) per replica.  Thread 0 does the 3x3 algebra (thermostat factor, barostat scaling, cell inverse); all 256
// threads stream the atom rows with workgroup reductions.  All state is f64 in HBM.  No synchronisation or allocation: the launch
// can be graph-captured.  What one launch does is chosen by `flags`:
//   MD_ABSORB  take the evaluation of the configuration written last (energy, forces, stress): non-finite -> retry / NONFINITE.
//              Phase 0 (a full step's configuration): MD_KICK2 finishes the step with the second half kick; Ekin, T and the
//              ideal-gas tensor are formed and a frame is written when the frame pointers are set.
//              Phase 1 (NPT: the barostat's scaled configuration, which ASE evaluates again because set_cell(scale_atoms=True) moved
//              the atoms): first half kick with these forces, fixcm, drift.
//   MD_START   start the next step from the cached forces: thermostat lambda, then NPT: barostat scaling, write the scaled
//              configuration and go to phase 1; NVE / NVT: first half kick, fixcm, drift.
//              MD_NVT_LANGEVIN (no reference counterpart; BAOAB, Leimkuhler & Matthews 2013): half kick, half drift, the
//              Ornstein-Uhlenbeck step p <- c1 p + sqrt((1 - c1^2) m kB T) xi with counter-based noise (philox.h), mass-weighted
//              fixcm, half drift.  tests/langevin_ref.py restates it.
//              MD_NVT_NHC / MD_NPT_NHC (no reference counterpart; Martyna-Tobias-Klein with Nose-Hoover chains on the particles
//              and on the isotropic barostat, Tuckerman et al., J. Phys. A 39 (2006) 5629): barostat chain, particle chain,
//              barostat kick, half kick and drift with the strain-rate factors, cell scaled; MD_ABSORB | MD_KICK2 runs the mirror
//              image after the kick.  One evaluation per step (phase stays 0), no fixcm.  tests/nhc_ref.py restates it.
//              MD_NPT_NHC_FLEX / MD_NPT_NHC_AXES (k_md_step_flex, a kernel of its own so that k_md_step keeps its instruction stream):
//              the same factorisation with a symmetric strain-rate matrix Vg in place of veps -- all six components free, or the three
//              diagonal ones -- and 3x3 matrix exponentials in place of the scalar factors.  tests/nhc_flex_ref.py restates it.
#pragma once

#include <hip/hip_runtime.h>

#include "mat3.h"   // mm3, det3, inv3, wave_sum_f64
#include "philox.h"

namespace chg {

enum : int { MD_RUNNING = 0, MD_NONFINITE = 1 };
enum : int { MD_NVE = 0, MD_NVT_BERENDSEN = 1, MD_NPT_BERENDSEN_INHOMOGENEOUS = 2, MD_NPT_BERENDSEN = 3, MD_NVT_LANGEVIN = 4,
             MD_NVT_NHC = 5, MD_NPT_NHC = 6, MD_NPT_NHC_FLEX = 7, MD_NPT_NHC_AXES = 8 };   // 7, 8: k_md_step_flex only
enum : int { MD_ABSORB = 1, MD_KICK2 = 2, MD_START = 4 };
constexpr int MD_SD = 40;   // doubles per replica: L[9] L^-1[9] Epot Ekin T stress[9] (eV/A^3, no ideal gas) G[9] (sum p p / m) spare
constexpr int MD_SI = 4;    // ints per replica: steps completed, status, phase, spare
constexpr int MD_FRAME_SCAL = 3;   // frame scalars per replica: Epot (engine units), Ekin, T
// Nose-Hoover chains, doubles per replica: particle chain velocities v[4] and positions eta[4], barostat chain vb[4] and xi[4] (the
// first chain_length of each are used), strain rate veps, H - Epot of the last absorbed evaluation (eV), 2 spare
constexpr int MD_NHC = 20;
constexpr int MD_NHC_MAX = 4;
// flexible-cell chains (MD_NPT_NHC_FLEX / MD_NPT_NHC_AXES), doubles per replica: the symmetric strain-rate matrix Vg, row-major; it takes
// the place of veps, which stays 0 in the chain state
constexpr int MD_VG = 9;

struct MdStepArgs {
  // state, replica o owns atom rows aoff[o]..aoff[o+1] (the batch has the same numbering: every replica is evaluated every time)
  double* r;              // [N, 3] cartesian positions
  double* p;              // [N, 3] momenta
  double* f;              // [N, 3] forces of the last absorbed evaluation
  const double* m;        // [N]    masses
  double* sd;             // [B, MD_SD]
  int* si;                // [B, MD_SI]
  const int* aoff;        // [B + 1]
  // the evaluation (MD_ABSORB)
  const float* energy;    // [B]
  const float* force;     // [N, 3]
  const float* stress;    // [B, 9] GPa or null (task without stress)
  const float* cfea;      // [B, fea_dim] or null
  const int* sel;         // [grid] replicas this launch steps (null: all, grid = B)
  // frame slot (null fr_scal: no frame this launch)
  double *fr_scal, *fr_pos, *fr_mom, *fr_cell;
  float *fr_force, *fr_stress, *fr_cfea;
  // next configuration to evaluate
  double* frac_next;      // [N, 3]
  double* lat_next;       // [B, 9]
  int* retry;             // [B] set to 1 (state untouched) when the evaluation is non-finite and final_try == 0
  double dt, temperature, taut, taup, pressure, compressibility, kB, stress_weight;
  int ensemble, fixcm, flags, final_try, fea_dim;
  // MD_NVT_LANGEVIN: c1 = exp(-friction dt), sig = sqrt((1 - c1^2) kB T), one noise key per replica
  double lg_c1, lg_sig;
  const unsigned long long* seeds;   // [B]
  // MD_NVT_NHC / MD_NPT_NHC (null / 0 otherwise): chain state, chain length 1..MD_NHC_MAX, frame slot of H - Epot
  double* nhc;            // [B, MD_NHC]
  double* fr_cons;        // [B] or null
  int nhc_len;
  // constraint (DESIGN.md "Constraints"; null: none, the <false> instantiation): [N, 3] 1 = component held, and the number of free
  // components of every replica (3 n: nothing held, the replica keeps the unconstrained degrees of freedom)
  const unsigned char* fixed;
  const int* nfree;       // [B]
};

// bit j set: component j of atom i is held (fixed: the replica's [n, 3] mask)
template <bool MASK>
__device__ __forceinline__ unsigned md_held_bits(const unsigned char* fixed, int i) {
  if (!MASK) return 0u;
  const unsigned char* h = fixed + 3 * (size_t)i;
  return (h[0] ? 1u : 0u) | (h[1] ? 2u : 0u) | (h[2] ? 4u : 0u);
}
// x, or 0 for a held component j
template <bool MASK>
__device__ __forceinline__ double md_free(unsigned held, int j, double x) { return (MASK && ((held >> j) & 1u)) ? 0.0 : x; }

// masses and constants of the Nose-Hoover chains of one replica with nf_ degrees of freedom (3 (n - 1), or the free components of a
// replica that holds some)
struct NhcConst {
  double kT, nf, alpha, Q0, Qk, Qb, W;
  __device__ NhcConst(const MdStepArgs& a, double nf_) {
    kT = a.kB * a.temperature;
    nf = nf_;
    alpha = 1.0 + 3.0 / nf;
    Qk = kT * a.taut * a.taut;
    Q0 = nf * Qk;
    Qb = kT * a.taup * a.taup;
    W = (nf + 3.0) * Qb;
  }
};

// one sweep over the chain velocities, k = M-1 .. 0 (down) or 0 .. M-1: v[k] is scaled by exp(-tau/4 v[k+1]) around its kick tau/2 G(k),
// G(0) = (K2 - dof kT) / Q0, G(k) = (Q[k-1] v[k-1]^2 - kT) / Qk.  Fully unrolled: v stays in registers.
template <bool DOWN>
__device__ inline void nhc_sweep(double (&v)[MD_NHC_MAX], int M, double Q0, double Qk, double K2, double dof, double kT, double tau) {
#pragma unroll
  for (int kk = 0; kk < MD_NHC_MAX; ++kk) {
    constexpr int last = MD_NHC_MAX - 1;
    const int k = DOWN ? last - kk : kk;
    if (k < M) {
      const double below = v[k > 0 ? k - 1 : 0];
      const double G = k == 0 ? (K2 - dof * kT) / Q0 : ((k == 1 ? Q0 : Qk) * below * below - kT) / Qk;
      const bool inner = k + 1 < M;
      const double e = inner ? exp(-0.25 * tau * v[k < last ? k + 1 : last]) : 1.0;
      v[k] = (v[k] * e + 0.5 * tau * G) * e;
    }
  }
}

// half a step (tau) of one chain in registers: returns the factor s for what it thermostats (K2 = twice its kinetic energy)
__device__ inline double nhc_chain(double (&v)[MD_NHC_MAX], double (&eta)[MD_NHC_MAX], int M, double Q0, double Qk, double K2, double dof,
                                   double kT, double tau) {
  nhc_sweep<true>(v, M, Q0, Qk, K2, dof, kT, tau);
  const double s = exp(-tau * v[0]);
#pragma unroll
  for (int k = 0; k < MD_NHC_MAX; ++k)
    if (k < M) eta[k] += tau * v[k];
  nhc_sweep<false>(v, M, Q0, Qk, K2 * s * s, dof, kT, tau);
  return s;
}

// H - Epot of the extended system: kinetic energy, chain energies and, for NPT, Pext V and the barostat's
__device__ inline double nhc_extended_energy(const NhcConst& c, const double* x, int M, double K2, bool npt, double pext, double vol) {
  double h = 0.5 * K2;
  for (int k = 0; k < M; ++k) h += 0.5 * (k == 0 ? c.Q0 : c.Qk) * x[k] * x[k] + (k == 0 ? c.nf : 1.0) * c.kT * x[4 + k];
  if (npt) {
    h += pext * vol + 0.5 * c.W * x[16] * x[16];
    for (int k = 0; k < M; ++k) h += 0.5 * c.Qb * x[8 + k] * x[8 + k] + c.kT * x[12 + k];
  }
  return h;
}

// MASK: a.fixed and a.nfree are set; <false> is the unconstrained kernel, instruction for instruction.  Under MASK the absorbed forces
// and every write of p are masked (selects, no divergent branch), so held components neither drift nor enter a sum.
template <bool MASK>
static __global__ __launch_bounds__(256) void k_md_step(MdStepArgs a) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int o = a.sel ? a.sel[blockIdx.x] : blockIdx.x;
  const int a0 = a.aoff[o], n = a.aoff[o + 1] - a0;
  double* r = a.r + 3 * (size_t)a0;
  double* p = a.p + 3 * (size_t)a0;
  double* f = a.f + 3 * (size_t)a0;
  const double* m = a.m + a0;
  double* sd = a.sd + (size_t)MD_SD * o;
  int* si = a.si + (size_t)MD_SI * o;
  const bool npt = a.ensemble == MD_NPT_BERENDSEN_INHOMOGENEOUS || a.ensemble == MD_NPT_BERENDSEN;
  const bool nhc = a.ensemble == MD_NVT_NHC || a.ensemble == MD_NPT_NHC, nhc_npt = a.ensemble == MD_NPT_NHC;
  double* xs = nhc ? a.nhc + (size_t)MD_NHC * o : nullptr;
  const double hdt = 0.5 * a.dt;
  const unsigned char* fixed = MASK ? a.fixed + 3 * (size_t)a0 : nullptr;
  // degrees of freedom of the temperature and N_f of the chains (a held atom breaks momentum conservation): the free components of a
  // replica that holds any, else 3 n and 3 (n - 1); evaluated where they are used, as the unconstrained kernel always did
  auto dof = [&]() -> double { return (MASK && a.nfree[o] < 3 * n) ? (double)a.nfree[o] : 3.0 * n; };
  auto nhc_nf = [&]() -> double { return (MASK && a.nfree[o] < 3 * n) ? (double)a.nfree[o] : 3.0 * (n - 1); };

  __shared__ double red[4][9];
  __shared__ int rfin[4];
  __shared__ double sLinv[9], sM[9], s_lam, s_mean[3], s_e[2];
  __shared__ int s_status, s_phase, s_go, s_steps;

  if (tid == 0) { s_status = si[1]; s_phase = si[2]; }
  __syncthreads();
  if (s_status != MD_RUNNING) return;   // frozen (NONFINITE): neither moved nor logged again
  bool advance = false;                 // first half kick, fixcm, drift follow

  if (a.flags & MD_ABSORB) {
    int fin = 1;
    for (int i = tid; i < n; i += 256) {
      const float* fi = a.force + 3 * ((size_t)a0 + i);
      fin &= isfinite(fi[0]) && isfinite(fi[1]) && isfinite(fi[2]);
    }
    fin = __all(fin);
    if (lane == 0) rfin[wv] = fin;
    __syncthreads();
    if (tid == 0) {
      int ok = rfin[0] & rfin[1] & rfin[2] & rfin[3] & (int)isfinite(a.energy[o]);
      if (a.stress)
        for (int i = 0; i < 9; ++i) ok &= (int)isfinite(a.stress[9 * (size_t)o + i]);
      if (!ok) {
        if (a.final_try) si[1] = MD_NONFINITE;
        else a.retry[o] = 1;
      }
      s_go = ok;
    }
    __syncthreads();
    if (!s_go) return;

    if (s_phase == 1) {                 // NPT: forces of the scaled configuration
      for (int i = tid; i < n; i += 256) {
        const float* fi = a.force + 3 * ((size_t)a0 + i);
        const unsigned held = md_held_bits<MASK>(fixed, i);
        f[3 * i] = md_free<MASK>(held, 0, fi[0]); f[3 * i + 1] = md_free<MASK>(held, 1, fi[1]); f[3 * i + 2] = md_free<MASK>(held, 2, fi[2]);
      }
      if (tid == 0) {
        sd[18] = a.energy[o];
        if (a.stress)
          for (int i = 0; i < 9; ++i) sd[21 + i] = (double)a.stress[9 * (size_t)o + i] * a.stress_weight;
        si[2] = 0;
        s_lam = 1.0;
      }
      advance = true;
    } else if (nhc) {
      // second half of the step: kick with the strain-rate factor and sum p p / m in one pass, thread 0 runs the barostat kick and the
      // two chains (their factor s scales p, Ekin and G without another reduction), one scaling pass writes the frame's momenta
      const bool kick = a.flags & MD_KICK2;
      const bool frame = a.fr_scal != nullptr;
      const NhcConst c(a, nhc_nf());
      const double e1 = kick ? exp(-0.5 * c.alpha * xs[16] * hdt) : 1.0;
      double acc[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      for (int i = tid; i < n; i += 256) {
        const float* fi = a.force + 3 * ((size_t)a0 + i);
        const unsigned held = md_held_bits<MASK>(fixed, i);
        auto fm = [&](int j) -> float { return (MASK && ((held >> j) & 1u)) ? 0.0f : fi[j]; };   // cached, kicked with and reported
        double pi[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const double fj = fm(j);
          f[3 * i + j] = fj;
          pi[j] = md_free<MASK>(held, j, kick ? (p[3 * i + j] * e1 + hdt * fj) * e1 : p[3 * i + j]);
          p[3 * i + j] = pi[j];
        }
        const double im = 1.0 / m[i];
        acc[1] += pi[0] * pi[0] * im; acc[2] += pi[1] * pi[1] * im; acc[3] += pi[2] * pi[2] * im;
        acc[4] += pi[1] * pi[2] * im; acc[5] += pi[0] * pi[2] * im; acc[6] += pi[0] * pi[1] * im;
        if (frame) {
          const size_t ro = 3 * ((size_t)a0 + i);
#pragma unroll
          for (int j = 0; j < 3; ++j) { a.fr_pos[ro + j] = r[3 * i + j]; a.fr_force[ro + j] = fm(j); }
        }
      }
#pragma unroll
      for (int k = 1; k < 7; ++k) acc[k] = wave_sum_f64(acc[k]);
      if (lane == 0)
        for (int k = 1; k < 7; ++k) red[wv][k] = acc[k];
      __syncthreads();
      if (tid == 0) {
        double G[7];
        for (int k = 1; k < 7; ++k) G[k] = red[0][k] + red[1][k] + red[2][k] + red[3][k];
        double K2 = G[1] + G[2] + G[3], s = 1.0;
        const double vol = fabs(det3(sd));
        sd[18] = a.energy[o];
        if (a.stress)
          for (int i = 0; i < 9; ++i) sd[21 + i] = (double)a.stress[9 * (size_t)o + i] * a.stress_weight;
        if (kick) {
          const int M = a.nhc_len;
          double v[MD_NHC_MAX], eta[MD_NHC_MAX];
          double veps = xs[16];
          if (nhc_npt) veps += hdt * (c.alpha * K2 - vol * (sd[21] + sd[25] + sd[29]) - 3.0 * a.pressure * vol) / c.W;
#pragma unroll
          for (int k = 0; k < MD_NHC_MAX; ++k) { v[k] = xs[k]; eta[k] = xs[4 + k]; }
          s = nhc_chain(v, eta, M, c.Q0, c.Qk, K2, c.nf, c.kT, hdt);
          K2 *= s * s;
#pragma unroll
          for (int k = 0; k < MD_NHC_MAX; ++k) { xs[k] = v[k]; xs[4 + k] = eta[k]; }
          if (nhc_npt) {
#pragma unroll
            for (int k = 0; k < MD_NHC_MAX; ++k) { v[k] = xs[8 + k]; eta[k] = xs[12 + k]; }
            veps *= nhc_chain(v, eta, M, c.Qb, c.Qb, c.W * veps * veps, 1.0, c.kT, hdt);
#pragma unroll
            for (int k = 0; k < MD_NHC_MAX; ++k) { xs[8 + k] = v[k]; xs[12 + k] = eta[k]; }
            xs[16] = veps;
          }
          si[0] += 1;
        }
        const double ekin = 0.5 * K2;
        const double T = (!MASK || dof() > 0.0) ? 2.0 * ekin / (dof() * a.kB) : 0.0;   // everything held (NVE only): T = 0
        const double cons = nhc_extended_energy(c, xs, a.nhc_len, K2, nhc_npt, a.pressure, vol);
        xs[17] = cons;
        sd[19] = ekin;
        sd[20] = T;
        const double s2 = s * s;
        const double Gm[9] = {G[1], G[6], G[5], G[6], G[2], G[4], G[5], G[4], G[3]};
        for (int i = 0; i < 9; ++i) sd[30 + i] = Gm[i] * s2;
        s_lam = s;
        if (frame) {
          a.fr_scal[MD_FRAME_SCAL * (size_t)o] = a.energy[o];
          a.fr_scal[MD_FRAME_SCAL * (size_t)o + 1] = ekin;
          a.fr_scal[MD_FRAME_SCAL * (size_t)o + 2] = T;
          if (a.fr_cons) a.fr_cons[o] = cons;
          for (int i = 0; i < 9; ++i) a.fr_cell[9 * (size_t)o + i] = sd[i];
          for (int i = 0; i < 9; ++i) a.fr_stress[9 * (size_t)o + i] = a.stress ? a.stress[9 * (size_t)o + i] : 0.0f;
          if (a.cfea && a.fr_cfea)
            for (int i = 0; i < a.fea_dim; ++i) a.fr_cfea[(size_t)a.fea_dim * o + i] = a.cfea[(size_t)a.fea_dim * o + i];
        }
      }
      __syncthreads();
      if (kick || frame) {
        const double s = s_lam;
        for (int i = tid; i < n; i += 256) {
          const unsigned held = md_held_bits<MASK>(fixed, i);
#pragma unroll
          for (int j = 0; j < 3; ++j) {
            const double pj = md_free<MASK>(held, j, p[3 * i + j] * s);
            p[3 * i + j] = pj;
            if (frame) a.fr_mom[3 * ((size_t)a0 + i) + j] = pj;
          }
        }
      }
    } else {
      const bool kick = a.flags & MD_KICK2;
      const bool frame = a.fr_scal != nullptr;
      double acc[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // sum p.p / m, then G xx yy zz yz xz xy
      for (int i = tid; i < n; i += 256) {
        const float* fi = a.force + 3 * ((size_t)a0 + i);
        const unsigned held = md_held_bits<MASK>(fixed, i);
        auto fm = [&](int j) -> float { return (MASK && ((held >> j) & 1u)) ? 0.0f : fi[j]; };   // cached, kicked with and reported
        double pi[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const double fj = fm(j);
          f[3 * i + j] = fj;
          pi[j] = md_free<MASK>(held, j, kick ? p[3 * i + j] + hdt * fj : p[3 * i + j]);
          p[3 * i + j] = pi[j];
        }
        const double im = 1.0 / m[i];
        acc[1] += pi[0] * pi[0] * im; acc[2] += pi[1] * pi[1] * im; acc[3] += pi[2] * pi[2] * im;
        acc[4] += pi[1] * pi[2] * im; acc[5] += pi[0] * pi[2] * im; acc[6] += pi[0] * pi[1] * im;
        if (frame) {
          const size_t ro = 3 * ((size_t)a0 + i);
#pragma unroll
          for (int j = 0; j < 3; ++j) { a.fr_pos[ro + j] = r[3 * i + j]; a.fr_mom[ro + j] = pi[j]; a.fr_force[ro + j] = fm(j); }
        }
      }
#pragma unroll
      for (int k = 1; k < 7; ++k) acc[k] = wave_sum_f64(acc[k]);
      if (lane == 0)
        for (int k = 1; k < 7; ++k) red[wv][k] = acc[k];
      __syncthreads();
      if (tid == 0) {
        double G[7];
        for (int k = 1; k < 7; ++k) G[k] = red[0][k] + red[1][k] + red[2][k] + red[3][k];
        const double ekin = 0.5 * (G[1] + G[2] + G[3]);
        const double T = (!MASK || dof() > 0.0) ? 2.0 * ekin / (dof() * a.kB) : 0.0;   // everything held (NVE only): T = 0
        sd[18] = a.energy[o];
        sd[19] = ekin;
        sd[20] = T;
        if (a.stress)
          for (int i = 0; i < 9; ++i) sd[21 + i] = (double)a.stress[9 * (size_t)o + i] * a.stress_weight;
        const double Gm[9] = {G[1], G[6], G[5], G[6], G[2], G[4], G[5], G[4], G[3]};
        for (int i = 0; i < 9; ++i) sd[30 + i] = Gm[i];
        if (kick) si[0] += 1;
        if (frame) {
          a.fr_scal[MD_FRAME_SCAL * (size_t)o] = a.energy[o];
          a.fr_scal[MD_FRAME_SCAL * (size_t)o + 1] = ekin;
          a.fr_scal[MD_FRAME_SCAL * (size_t)o + 2] = T;
          for (int i = 0; i < 9; ++i) a.fr_cell[9 * (size_t)o + i] = sd[i];
          for (int i = 0; i < 9; ++i) a.fr_stress[9 * (size_t)o + i] = a.stress ? a.stress[9 * (size_t)o + i] : 0.0f;
          if (a.cfea && a.fr_cfea)
            for (int i = 0; i < a.fea_dim; ++i) a.fr_cfea[(size_t)a.fea_dim * o + i] = a.cfea[(size_t)a.fea_dim * o + i];
        }
      }
    }
  }

  if ((a.flags & MD_START) && a.ensemble == MD_NVT_LANGEVIN) {
    // BAOAB up to the evaluation: B A O A.  The noise counter is the number of steps this replica has completed (thread 0 has
    // just counted the step that MD_KICK2 finished)
    __syncthreads();
    if (tid == 0) {
      s_steps = si[0];
      for (int i = 0; i < 9; ++i) { sLinv[i] = sd[9 + i]; a.lat_next[9 * (size_t)o + i] = sd[i]; }
    }
    __syncthreads();
    const unsigned long long seed = a.seeds[o];
    const unsigned step = (unsigned)s_steps;
    const bool noisy = a.lg_sig > 0.0;
    double ps[4] = {0.0, 0.0, 0.0, 0.0};   // sum p, sum m
    for (int i = tid; i < n; i += 256) {
      const double mi = m[i];
      double xi[3] = {0.0, 0.0, 0.0};
      if (noisy) philox_normal3(seed, (unsigned)i, step, xi);
      const double sg = a.lg_sig * sqrt(mi);
      const unsigned held = md_held_bits<MASK>(fixed, i);   // the noise of a held component is drawn and dropped
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        double pj = md_free<MASK>(held, j, p[3 * i + j] + hdt * f[3 * i + j]);
        r[3 * i + j] += hdt * pj / mi;
        pj = md_free<MASK>(held, j, a.lg_c1 * pj + sg * xi[j]);
        p[3 * i + j] = pj;
        ps[j] += pj;
      }
      ps[3] += mi;
    }
    if (a.fixcm) {
#pragma unroll
      for (int j = 0; j < 4; ++j) ps[j] = wave_sum_f64(ps[j]);
      if (lane == 0)
        for (int j = 0; j < 4; ++j) red[wv][j] = ps[j];
      __syncthreads();
      if (tid == 0) {
        const double im = 1.0 / (red[0][3] + red[1][3] + red[2][3] + red[3][3]);
        for (int j = 0; j < 3; ++j) s_mean[j] = (red[0][j] + red[1][j] + red[2][j] + red[3][j]) * im;   // centre-of-mass velocity
      }
      __syncthreads();
    }
    for (int i = tid; i < n; i += 256) {
      const double mi = m[i];
      const unsigned held = md_held_bits<MASK>(fixed, i);
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const double pj = md_free<MASK>(held, j, a.fixcm ? p[3 * i + j] - mi * s_mean[j] : p[3 * i + j]);
        p[3 * i + j] = pj;
        r[3 * i + j] += hdt * pj / mi;
      }
      const double y0 = r[3 * i], y1 = r[3 * i + 1], y2 = r[3 * i + 2];
      double* fr = a.frac_next + 3 * ((size_t)a0 + i);
#pragma unroll
      for (int j = 0; j < 3; ++j) fr[j] = y0 * sLinv[j] + y1 * sLinv[3 + j] + y2 * sLinv[6 + j];
    }
    return;
  }

  if ((a.flags & MD_START) && nhc) {
    // up to the evaluation: barostat chain, particle chain, barostat kick (cached stress, sum p p / m scaled by s^2), then one pass
    // p <- (p s e1 + dt/2 f) e1, r <- (r e2 + dt p / m) e2 with e1 = exp(-alpha veps dt/4), e2 = exp(veps dt/2); the cell scales by e2^2
    __syncthreads();   // sd, the chain state and p written above
    if (tid == 0) {
      const NhcConst c(a, nhc_nf());
      const int M = a.nhc_len;
      double v[MD_NHC_MAX], eta[MD_NHC_MAX];
      double veps = xs[16], K2 = sd[30] + sd[34] + sd[38];
      if (nhc_npt) {
#pragma unroll
        for (int k = 0; k < MD_NHC_MAX; ++k) { v[k] = xs[8 + k]; eta[k] = xs[12 + k]; }
        veps *= nhc_chain(v, eta, M, c.Qb, c.Qb, c.W * veps * veps, 1.0, c.kT, hdt);
#pragma unroll
        for (int k = 0; k < MD_NHC_MAX; ++k) { xs[8 + k] = v[k]; xs[12 + k] = eta[k]; }
      }
#pragma unroll
      for (int k = 0; k < MD_NHC_MAX; ++k) { v[k] = xs[k]; eta[k] = xs[4 + k]; }
      const double s = nhc_chain(v, eta, M, c.Q0, c.Qk, K2, c.nf, c.kT, hdt);
      K2 *= s * s;
#pragma unroll
      for (int k = 0; k < MD_NHC_MAX; ++k) { xs[k] = v[k]; xs[4 + k] = eta[k]; }
      double L[9];
      for (int i = 0; i < 9; ++i) L[i] = sd[i];
      if (nhc_npt) {
        const double vol = fabs(det3(L));
        veps += hdt * (c.alpha * K2 - vol * (sd[21] + sd[25] + sd[29]) - 3.0 * a.pressure * vol) / c.W;
        xs[16] = veps;
        const double eh = exp(veps * a.dt);
        for (int i = 0; i < 9; ++i) { L[i] *= eh; sd[i] = L[i]; }
        inv3(L, sd + 9);
      }
      s_lam = s;
      s_e[0] = exp(-0.5 * c.alpha * veps * hdt);
      s_e[1] = exp(0.5 * veps * a.dt);
      for (int i = 0; i < 9; ++i) { sLinv[i] = sd[9 + i]; a.lat_next[9 * (size_t)o + i] = L[i]; }
    }
    __syncthreads();
    const double e1 = s_e[0], e2 = s_e[1], se1 = s_lam * e1;
    for (int i = tid; i < n; i += 256) {
      const double idm = a.dt / m[i];
      const unsigned held = md_held_bits<MASK>(fixed, i);
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const double pj = md_free<MASK>(held, j, (p[3 * i + j] * se1 + hdt * f[3 * i + j]) * e1);
        p[3 * i + j] = pj;
        r[3 * i + j] = (r[3 * i + j] * e2 + idm * pj) * e2;
      }
      const double y0 = r[3 * i], y1 = r[3 * i + 1], y2 = r[3 * i + 2];
      double* fr = a.frac_next + 3 * ((size_t)a0 + i);
#pragma unroll
      for (int j = 0; j < 3; ++j) fr[j] = y0 * sLinv[j] + y1 * sLinv[3 + j] + y2 * sLinv[6 + j];
    }
    return;
  }

  if ((a.flags & MD_START) && !advance) {
    // thermostat (ASE NVTBerendsen.scale_velocities) and barostat (NPTBerendsen / Inhomogeneous_NPTBerendsen.scale_positions_and_cell)
    __syncthreads();   // sd written by thread 0 above
    if (tid == 0) {
      double lam = 1.0;
      if (a.ensemble != MD_NVE) {
        const double T = sd[20];
        const double ratio = T > 0.0 ? a.temperature / T : (a.temperature > 0.0 ? (double)INFINITY : 1.0);
        lam = sqrt(1.0 + (ratio - 1.0) * (a.dt / a.taut));
        if (lam > 1.1) lam = 1.1;
        if (lam < 0.9) lam = 0.9;
      }
      s_lam = lam;
      if (npt) {
        double L[9], Ln[9], M[9], st[9];
        for (int i = 0; i < 9; ++i) L[i] = sd[i];
        const double iv = 1.0 / fabs(det3(L));
        for (int i = 0; i < 9; ++i) st[i] = sd[21 + i] - lam * lam * sd[30 + i] * iv;   // stress incl. the ideal-gas term
        double sc[3];
        if (a.ensemble == MD_NPT_BERENDSEN_INHOMOGENEOUS) {
          const double taupscl = a.dt * a.compressibility / a.taup / 3.0;
          for (int i = 0; i < 3; ++i) sc[i] = 1.0 - taupscl * (a.pressure - (-st[4 * i]));
        } else {
          const double taupscl = a.dt / a.taup;
          const double old_p = -(st[0] + st[4] + st[8]) / 3.0;
          sc[0] = sc[1] = sc[2] = 1.0 - taupscl * a.compressibility / 3.0 * (a.pressure - old_p);
        }
        for (int i = 0; i < 3; ++i)
          for (int j = 0; j < 3; ++j) Ln[3 * i + j] = sc[i] * L[3 * i + j];
        mm3(sd + 9, Ln, M);            // positions <- positions . solve(L, L')
        for (int i = 0; i < 9; ++i) { sM[i] = M[i]; sd[i] = Ln[i]; }
        inv3(Ln, sd + 9);
        for (int i = 0; i < 9; ++i) { sLinv[i] = sd[9 + i]; a.lat_next[9 * (size_t)o + i] = Ln[i]; }
        si[2] = 1;
      }
    }
    __syncthreads();
    const double lam = s_lam;
    for (int i = tid; i < n; i += 256) {
      const unsigned held = md_held_bits<MASK>(fixed, i);
#pragma unroll
      for (int j = 0; j < 3; ++j) p[3 * i + j] = md_free<MASK>(held, j, p[3 * i + j] * lam);
      if (npt) {
        const double x0 = r[3 * i], x1 = r[3 * i + 1], x2 = r[3 * i + 2];
        double* fr = a.frac_next + 3 * ((size_t)a0 + i);
#pragma unroll
        for (int j = 0; j < 3; ++j) r[3 * i + j] = x0 * sM[j] + x1 * sM[3 + j] + x2 * sM[6 + j];
        const double y0 = r[3 * i], y1 = r[3 * i + 1], y2 = r[3 * i + 2];
#pragma unroll
        for (int j = 0; j < 3; ++j) fr[j] = y0 * sLinv[j] + y1 * sLinv[3 + j] + y2 * sLinv[6 + j];
      }
    }
    if (npt) return;                    // the scaled configuration is evaluated before the half kick
    advance = true;
  }
  if (!advance) return;

  // first half kick with the cached forces, fixcm (mean momentum, not mass-weighted), drift r += dt p / m
  __syncthreads();
  double ps[3] = {0.0, 0.0, 0.0};
  for (int i = tid; i < n; i += 256) {
    const unsigned held = md_held_bits<MASK>(fixed, i);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double pj = md_free<MASK>(held, j, p[3 * i + j] + hdt * f[3 * i + j]);
      p[3 * i + j] = pj;
      ps[j] += pj;
    }
  }
  if (a.fixcm) {
#pragma unroll
    for (int j = 0; j < 3; ++j) ps[j] = wave_sum_f64(ps[j]);
    if (lane == 0)
      for (int j = 0; j < 3; ++j) red[wv][j] = ps[j];
  }
  if (tid == 0)
    for (int i = 0; i < 9; ++i) sLinv[i] = sd[9 + i];
  __syncthreads();
  if (tid == 0) {
    for (int j = 0; j < 3; ++j) s_mean[j] = a.fixcm ? (red[0][j] + red[1][j] + red[2][j] + red[3][j]) / (double)n : 0.0;
    for (int i = 0; i < 9; ++i) a.lat_next[9 * (size_t)o + i] = sd[i];
  }
  __syncthreads();
  for (int i = tid; i < n; i += 256) {
    const double mi = m[i];
    const unsigned held = md_held_bits<MASK>(fixed, i);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double pj = md_free<MASK>(held, j, a.fixcm ? p[3 * i + j] - s_mean[j] : p[3 * i + j]);
      p[3 * i + j] = pj;
      r[3 * i + j] += a.dt * pj / mi;
    }
    const double y0 = r[3 * i], y1 = r[3 * i + 1], y2 = r[3 * i + 2];
    double* fr = a.frac_next + 3 * ((size_t)a0 + i);
#pragma unroll
    for (int j = 0; j < 3; ++j) fr[j] = y0 * sLinv[j] + y1 * sLinv[3 + j] + y2 * sLinv[6 + j];
  }
}

// ---- flexible-cell Nose-Hoover-chain NPT ------------------------------------------------------------------------------------------------
// Symmetric 3x3 matrices travel as six numbers in the order of the kinetic sums: xx yy zz yz xz xy.

// the upper triangle of a b for two commuting symmetric matrices (a polynomial of a matrix and that matrix): the product is symmetric,
// and forming one triangle only keeps it so to the bit
__device__ __forceinline__ void sym_mul(const double (&a)[6], const double (&b)[6], double (&c)[6]) {
  c[0] = a[0] * b[0] + a[5] * b[5] + a[4] * b[4];
  c[1] = a[5] * b[5] + a[1] * b[1] + a[3] * b[3];
  c[2] = a[4] * b[4] + a[3] * b[3] + a[2] * b[2];
  c[3] = a[5] * b[4] + a[1] * b[3] + a[3] * b[2];
  c[4] = a[0] * b[4] + a[5] * b[3] + a[4] * b[2];
  c[5] = a[0] * b[5] + a[5] * b[1] + a[4] * b[3];
}

// exp(a): a is halved until its row-sum norm is <= 1/4 (exact), the Taylor polynomial of degree 14 (remainder 0.25^15 / 15! < 1e-21) is
// evaluated by Horner's rule and squared back.  Exactly I at a = 0, exactly diagonal for a multiple of I, no eigenvectors anywhere; exp(-a)
// runs the same operations on the negated entries and is the inverse of exp(a) to rounding.  The loops stay rolled: thread 0 only.
__device__ inline void sym_expm(const double (&a)[6], double (&e)[6]) {
  const double nrm = fmax(fabs(a[0]) + fabs(a[5]) + fabs(a[4]), fmax(fabs(a[5]) + fabs(a[1]) + fabs(a[3]), fabs(a[4]) + fabs(a[3]) + fabs(a[2])));
  double sc = 1.0;
  int sq = 0;
  while (nrm * sc > 0.25 && sq < 64) { sc *= 0.5; ++sq; }
  double x[6], y[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) { x[k] = a[k] * sc; e[k] = k < 3 ? 1.0 : 0.0; }
#pragma unroll 1
  for (int k = 14; k >= 1; --k) {
    sym_mul(x, e, y);
    const double ik = 1.0 / (double)k;
#pragma unroll
    for (int j = 0; j < 6; ++j) e[j] = (j < 3 ? 1.0 : 0.0) + y[j] * ik;
  }
#pragma unroll 1
  for (int s = 0; s < sq; ++s) {
    sym_mul(e, e, y);
#pragma unroll
    for (int j = 0; j < 6; ++j) e[j] = y[j];
  }
}

// masses of the flexible barostat on top of NhcConst: W_g = W / 3 per strain-rate component, d_b free components (6, or 3 for the
// axes), barostat chain masses Q'_1 = d_b kT taup^2, Q'_k = kT taup^2 (= NhcConst::Qb)
struct FlexConst {
  double Wg, db, Qb0;
  bool axes;
  __device__ FlexConst(const NhcConst& c, int ensemble) {
    axes = ensemble == MD_NPT_NHC_AXES;
    db = axes ? 3.0 : 6.0;
    Wg = c.W / 3.0;
    Qb0 = db * c.Qb;
  }
};

// W_g sum_ab Vg_ab^2: twice the kinetic energy of the cell
__device__ __forceinline__ double flex_k2(const FlexConst& fc, const double (&vg)[6]) {
  return fc.Wg * (vg[0] * vg[0] + vg[1] * vg[1] + vg[2] * vg[2] + 2.0 * (vg[3] * vg[3] + vg[4] * vg[4] + vg[5] * vg[5]));
}

// Vg_ab += tau G_ab / W_g on the free components, G = sum p p / m + (K2 / N_f - Pext V) I - V (sigma + sigma^T) / 2 with the stress sg[9]
__device__ __forceinline__ void flex_barostat_kick(const NhcConst& c, const FlexConst& fc, double (&vg)[6], const double (&pp)[6], double K2, double vol,
                                                   const double* sg, double pext, double tau) {
  const double iso = K2 / c.nf - pext * vol;
  vg[0] += tau * (pp[0] + iso - vol * sg[0]) / fc.Wg;
  vg[1] += tau * (pp[1] + iso - vol * sg[4]) / fc.Wg;
  vg[2] += tau * (pp[2] + iso - vol * sg[8]) / fc.Wg;
  if (!fc.axes) {
    vg[3] += tau * (pp[3] - vol * (0.5 * (sg[5] + sg[7]))) / fc.Wg;
    vg[4] += tau * (pp[4] - vol * (0.5 * (sg[2] + sg[6]))) / fc.Wg;
    vg[5] += tau * (pp[5] - vol * (0.5 * (sg[1] + sg[3]))) / fc.Wg;
  }
}

// half a step of the barostat chain: Vg *= s
__device__ inline void flex_barostat_chain(const NhcConst& c, const FlexConst& fc, double* xs, int M, double (&vg)[6], double tau) {
  double v[MD_NHC_MAX], eta[MD_NHC_MAX];
#pragma unroll
  for (int k = 0; k < MD_NHC_MAX; ++k) { v[k] = xs[8 + k]; eta[k] = xs[12 + k]; }
  const double s = nhc_chain(v, eta, M, fc.Qb0, c.Qb, flex_k2(fc, vg), fc.db, c.kT, tau);
#pragma unroll
  for (int k = 0; k < MD_NHC_MAX; ++k) { xs[8 + k] = v[k]; xs[12 + k] = eta[k]; }
#pragma unroll
  for (int k = 0; k < 6; ++k) vg[k] *= s;
}

// half a step of the particle chain: returns s, K2 *= s^2
__device__ inline double flex_particle_chain(const NhcConst& c, double* xs, int M, double& K2, double tau) {
  double v[MD_NHC_MAX], eta[MD_NHC_MAX];
#pragma unroll
  for (int k = 0; k < MD_NHC_MAX; ++k) { v[k] = xs[k]; eta[k] = xs[4 + k]; }
  const double s = nhc_chain(v, eta, M, c.Q0, c.Qk, K2, c.nf, c.kT, tau);
#pragma unroll
  for (int k = 0; k < MD_NHC_MAX; ++k) { xs[k] = v[k]; xs[4 + k] = eta[k]; }
  K2 *= s * s;
  return s;
}

__device__ __forceinline__ void flex_load_vg(const double* g, double (&vg)[6]) {
  vg[0] = g[0]; vg[1] = g[4]; vg[2] = g[8]; vg[3] = g[5]; vg[4] = g[2]; vg[5] = g[1];
}
__device__ __forceinline__ void flex_store_vg(double* g, const double (&vg)[6]) {
  g[0] = vg[0]; g[4] = vg[1]; g[8] = vg[2]; g[5] = g[7] = vg[3]; g[2] = g[6] = vg[4]; g[1] = g[3] = vg[5];
}

// exp(-(Vg + tr Vg / N_f I) tau / 2): the factor on either side of the half kick
__device__ inline void flex_kick_factor(const NhcConst& c, const double (&vg)[6], double tau, double (&e)[6]) {
  const double tr = (vg[0] + vg[1] + vg[2]) / c.nf;
  double arg[6];
#pragma unroll
  for (int k = 0; k < 6; ++k) arg[k] = -(vg[k] + (k < 3 ? tr : 0.0)) * (0.5 * tau);
  sym_expm(arg, e);
}

// row vector times symmetric matrix
__device__ __forceinline__ void row_sym(const double (&v)[3], const double* e, double (&w)[3]) {
  w[0] = v[0] * e[0] + v[1] * e[5] + v[2] * e[4];
  w[1] = v[0] * e[5] + v[1] * e[1] + v[2] * e[3];
  w[2] = v[0] * e[4] + v[1] * e[3] + v[2] * e[2];
}

struct MdFlexArgs {
  double* vg;   // [B, MD_VG]
};

// MD_NPT_NHC_FLEX / MD_NPT_NHC_AXES on the launch structure of k_md_step (one workgroup per replica, the chains and the matrix
// exponentials in thread 0, the factors handed to the row passes through LDS); phase stays 0, no fixcm.  MASK as in k_md_step.
template <bool MASK>
static __global__ __launch_bounds__(256) void k_md_step_flex(MdStepArgs a, MdFlexArgs x) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int o = a.sel ? a.sel[blockIdx.x] : blockIdx.x;
  const int a0 = a.aoff[o], n = a.aoff[o + 1] - a0;
  double* r = a.r + 3 * (size_t)a0;
  double* p = a.p + 3 * (size_t)a0;
  double* f = a.f + 3 * (size_t)a0;
  const double* m = a.m + a0;
  double* sd = a.sd + (size_t)MD_SD * o;
  int* si = a.si + (size_t)MD_SI * o;
  double* xs = a.nhc + (size_t)MD_NHC * o;
  double* gv = x.vg + (size_t)MD_VG * o;
  const double hdt = 0.5 * a.dt;
  const unsigned char* fixed = MASK ? a.fixed + 3 * (size_t)a0 : nullptr;
  auto dof = [&]() -> double { return (MASK && a.nfree[o] < 3 * n) ? (double)a.nfree[o] : 3.0 * n; };
  auto nhc_nf = [&]() -> double { return (MASK && a.nfree[o] < 3 * n) ? (double)a.nfree[o] : 3.0 * (n - 1); };

  __shared__ double red[4][7];
  __shared__ int rfin[4];
  __shared__ double sLinv[9], sE1[6], sE2[6], s_lam;
  __shared__ int s_status, s_go;

  if (tid == 0) s_status = si[1];
  __syncthreads();
  if (s_status != MD_RUNNING) return;

  if (a.flags & MD_ABSORB) {
    const bool kick = a.flags & MD_KICK2;
    const bool frame = a.fr_scal != nullptr;
    int fin = 1;
    for (int i = tid; i < n; i += 256) {
      const float* fi = a.force + 3 * ((size_t)a0 + i);
      fin &= isfinite(fi[0]) && isfinite(fi[1]) && isfinite(fi[2]);
    }
    fin = __all(fin);
    if (lane == 0) rfin[wv] = fin;
    __syncthreads();
    if (tid == 0) {
      int ok = rfin[0] & rfin[1] & rfin[2] & rfin[3] & (int)isfinite(a.energy[o]);
      if (a.stress)
        for (int i = 0; i < 9; ++i) ok &= (int)isfinite(a.stress[9 * (size_t)o + i]);
      if (!ok) {
        if (a.final_try) si[1] = MD_NONFINITE;
        else a.retry[o] = 1;
      }
      s_go = ok;
      if (ok && kick) {
        const NhcConst c(a, nhc_nf());
        double vg[6], e[6];
        flex_load_vg(gv, vg);
        flex_kick_factor(c, vg, hdt, e);
        for (int k = 0; k < 6; ++k) sE1[k] = e[k];
      }
    }
    __syncthreads();
    if (!s_go) return;

    // second half of the step: p <- (p E1 + dt/2 f) E1 and sum p p / m in one pass, thread 0 runs the barostat kick and the two chains,
    // one scaling pass writes the frame's momenta
    double acc[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = tid; i < n; i += 256) {
      const float* fi = a.force + 3 * ((size_t)a0 + i);
      const unsigned held = md_held_bits<MASK>(fixed, i);
      auto fm = [&](int j) -> float { return (MASK && ((held >> j) & 1u)) ? 0.0f : fi[j]; };
      double pi[3] = {p[3 * i], p[3 * i + 1], p[3 * i + 2]};
      const double fj[3] = {fm(0), fm(1), fm(2)};
      if (kick) {
        double q[3];
        row_sym(pi, sE1, q);
#pragma unroll
        for (int j = 0; j < 3; ++j) q[j] += hdt * fj[j];
        row_sym(q, sE1, pi);
      }
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        f[3 * i + j] = fj[j];
        pi[j] = md_free<MASK>(held, j, pi[j]);
        p[3 * i + j] = pi[j];
      }
      const double im = 1.0 / m[i];
      acc[1] += pi[0] * pi[0] * im; acc[2] += pi[1] * pi[1] * im; acc[3] += pi[2] * pi[2] * im;
      acc[4] += pi[1] * pi[2] * im; acc[5] += pi[0] * pi[2] * im; acc[6] += pi[0] * pi[1] * im;
      if (frame) {
        const size_t ro = 3 * ((size_t)a0 + i);
#pragma unroll
        for (int j = 0; j < 3; ++j) { a.fr_pos[ro + j] = r[3 * i + j]; a.fr_force[ro + j] = fm(j); }
      }
    }
#pragma unroll
    for (int k = 1; k < 7; ++k) acc[k] = wave_sum_f64(acc[k]);
    if (lane == 0)
      for (int k = 1; k < 7; ++k) red[wv][k] = acc[k];
    __syncthreads();
    if (tid == 0) {
      const NhcConst c(a, nhc_nf());
      const FlexConst fc(c, a.ensemble);
      double pp[6], vg[6];
      for (int k = 0; k < 6; ++k) pp[k] = red[0][k + 1] + red[1][k + 1] + red[2][k + 1] + red[3][k + 1];
      double K2 = pp[0] + pp[1] + pp[2], s = 1.0;
      const double vol = fabs(det3(sd));
      sd[18] = a.energy[o];
      if (a.stress)
        for (int i = 0; i < 9; ++i) sd[21 + i] = (double)a.stress[9 * (size_t)o + i] * a.stress_weight;
      flex_load_vg(gv, vg);
      if (kick) {
        flex_barostat_kick(c, fc, vg, pp, K2, vol, sd + 21, a.pressure, hdt);
        s = flex_particle_chain(c, xs, a.nhc_len, K2, hdt);
        flex_barostat_chain(c, fc, xs, a.nhc_len, vg, hdt);
        flex_store_vg(gv, vg);
        si[0] += 1;
      }
      const double ekin = 0.5 * K2;
      const double T = (!MASK || dof() > 0.0) ? 2.0 * ekin / (dof() * a.kB) : 0.0;
      double cons = 0.5 * K2 + a.pressure * vol + 0.5 * flex_k2(fc, vg);
      for (int k = 0; k < a.nhc_len; ++k)
        cons += 0.5 * (k == 0 ? c.Q0 : c.Qk) * xs[k] * xs[k] + (k == 0 ? c.nf : 1.0) * c.kT * xs[4 + k] +
                0.5 * (k == 0 ? fc.Qb0 : c.Qb) * xs[8 + k] * xs[8 + k] + (k == 0 ? fc.db : 1.0) * c.kT * xs[12 + k];
      xs[17] = cons;
      sd[19] = ekin;
      sd[20] = T;
      const double s2 = s * s;
      const double Gm[9] = {pp[0], pp[5], pp[4], pp[5], pp[1], pp[3], pp[4], pp[3], pp[2]};
      for (int i = 0; i < 9; ++i) sd[30 + i] = Gm[i] * s2;
      s_lam = s;
      if (frame) {
        a.fr_scal[MD_FRAME_SCAL * (size_t)o] = a.energy[o];
        a.fr_scal[MD_FRAME_SCAL * (size_t)o + 1] = ekin;
        a.fr_scal[MD_FRAME_SCAL * (size_t)o + 2] = T;
        if (a.fr_cons) a.fr_cons[o] = cons;
        for (int i = 0; i < 9; ++i) a.fr_cell[9 * (size_t)o + i] = sd[i];
        for (int i = 0; i < 9; ++i) a.fr_stress[9 * (size_t)o + i] = a.stress ? a.stress[9 * (size_t)o + i] : 0.0f;
        if (a.cfea && a.fr_cfea)
          for (int i = 0; i < a.fea_dim; ++i) a.fr_cfea[(size_t)a.fea_dim * o + i] = a.cfea[(size_t)a.fea_dim * o + i];
      }
    }
    __syncthreads();
    if (kick || frame) {
      const double s = s_lam;
      for (int i = tid; i < n; i += 256) {
        const unsigned held = md_held_bits<MASK>(fixed, i);
#pragma unroll
        for (int j = 0; j < 3; ++j) {
          const double pj = md_free<MASK>(held, j, p[3 * i + j] * s);
          p[3 * i + j] = pj;
          if (frame) a.fr_mom[3 * ((size_t)a0 + i) + j] = pj;
        }
      }
    }
  }

  if (!(a.flags & MD_START)) return;
  // up to the evaluation: barostat chain, particle chain, barostat kick (cached stress, sum p p / m scaled by s^2), then one pass
  // p <- (p s E1 + dt/2 f) E1, r <- (r E2 + dt p / m) E2 with E2 = exp(Vg dt/2); the cell is multiplied by E2 E2 = exp(Vg dt)
  __syncthreads();   // sd, the chain state and p written above
  if (tid == 0) {
    const NhcConst c(a, nhc_nf());
    const FlexConst fc(c, a.ensemble);
    double vg[6], e[6], e3[6], arg[6];
    flex_load_vg(gv, vg);
    flex_barostat_chain(c, fc, xs, a.nhc_len, vg, hdt);
    double K2 = sd[30] + sd[34] + sd[38];
    const double s = flex_particle_chain(c, xs, a.nhc_len, K2, hdt), s2 = s * s;
    const double pp[6] = {sd[30] * s2, sd[34] * s2, sd[38] * s2, sd[35] * s2, sd[32] * s2, sd[31] * s2};
    double L[9], Ln[9];
    for (int i = 0; i < 9; ++i) L[i] = sd[i];
    flex_barostat_kick(c, fc, vg, pp, K2, fabs(det3(L)), sd + 21, a.pressure, hdt);
    flex_store_vg(gv, vg);
    flex_kick_factor(c, vg, hdt, e);
    for (int k = 0; k < 6; ++k) sE1[k] = e[k];
    for (int k = 0; k < 6; ++k) arg[k] = vg[k] * hdt;
    sym_expm(arg, e);
    for (int k = 0; k < 6; ++k) sE2[k] = e[k];
    sym_mul(e, e, e3);
    const double E3[9] = {e3[0], e3[5], e3[4], e3[5], e3[1], e3[3], e3[4], e3[3], e3[2]};
    mm3(L, E3, Ln);
    for (int i = 0; i < 9; ++i) sd[i] = Ln[i];
    inv3(Ln, sd + 9);
    s_lam = s;
    for (int i = 0; i < 9; ++i) { sLinv[i] = sd[9 + i]; a.lat_next[9 * (size_t)o + i] = Ln[i]; }
  }
  __syncthreads();
  const double s = s_lam;
  for (int i = tid; i < n; i += 256) {
    const double idm = a.dt / m[i];
    const unsigned held = md_held_bits<MASK>(fixed, i);
    double pi[3] = {p[3 * i] * s, p[3 * i + 1] * s, p[3 * i + 2] * s}, q[3], ri[3] = {r[3 * i], r[3 * i + 1], r[3 * i + 2]}, y[3];
    row_sym(pi, sE1, q);
#pragma unroll
    for (int j = 0; j < 3; ++j) q[j] += hdt * f[3 * i + j];
    row_sym(q, sE1, pi);
    row_sym(ri, sE2, y);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      pi[j] = md_free<MASK>(held, j, pi[j]);
      p[3 * i + j] = pi[j];
      y[j] += idm * pi[j];
    }
    row_sym(y, sE2, ri);
#pragma unroll
    for (int j = 0; j < 3; ++j) r[3 * i + j] = ri[j];
    double* fr = a.frac_next + 3 * ((size_t)a0 + i);
#pragma unroll
    for (int j = 0; j < 3; ++j) fr[j] = ri[0] * sLinv[j] + ri[1] * sLinv[3 + j] + ri[2] * sLinv[6 + j];
  }
}

}  // namespace chg
