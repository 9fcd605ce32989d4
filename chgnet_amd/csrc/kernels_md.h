// kernels_md.h -- the molecular-dynamics step kernels of a batched MD run (chg_md_*): one kernel per integrator family over shared helpers.
//
// Reference driver replaced (file:line relative to /root/reference/chgnet):
//   MolecularDynamics: ASE VelocityVerlet / NVTBerendsen / Inhomogeneous_NPTBerendsen / NPTBerendsen   model/dynamics.py:433-780
// tests/md_ref.py restates the semantics in float64 NumPy; DESIGN.md "Molecular dynamics" gives the state layout.
//
// One workgroup (4 waves) per replica.  Thread 0 does the 3x3 algebra (thermostat factor, chains, barostat scaling, cell inverse); all
// 256 threads stream the atom rows with workgroup reductions.  All state is f64 in HBM.  No synchronisation or allocation: the launch
// can be graph-captured.  What one launch does is chosen by `flags`, with the same meaning in every kernel:
//   MD_ABSORB  take the evaluation of the configuration written last (energy, forces, stress): non-finite -> retry / NONFINITE.
//              MD_KICK2 finishes the step with the second half kick; Ekin, T and the ideal-gas tensor are formed and a frame is
//              written when a.fr is set.
//   MD_START   start the next step from the cached forces, up to the configuration that is evaluated next.
// The host picks the kernel from the ensemble code (engine_md.hip, launch_step); a.ensemble chooses inside a family.
//   k_md_step       the Verlet family.  NVE, NVT Berendsen: thermostat lambda, first half kick, fixcm, drift.  The two Berendsen NPT
//                   codes: MD_START scales cell and positions and goes to phase 1; MD_ABSORB at phase 1 takes the forces of the scaled
//                   configuration, which ASE evaluates again because set_cell(scale_atoms=True) moved the atoms, then kicks and drifts.
//                   MD_NVT_LANGEVIN (no reference counterpart; BAOAB, Leimkuhler & Matthews 2013): half kick, half drift, the
//                   Ornstein-Uhlenbeck step p <- c1 p + sqrt((1 - c1^2) m kB T) xi with counter-based noise (philox.h), mass-weighted
//                   fixcm, half drift.  tests/langevin_ref.py restates it.
//   k_md_step_nhc   MD_NVT_NHC / MD_NPT_NHC (no reference counterpart; Martyna-Tobias-Klein with Nose-Hoover chains on the particles
//                   and on the isotropic barostat, Tuckerman et al., J. Phys. A 39 (2006) 5629): barostat chain, particle chain,
//                   barostat kick, half kick and drift with the scalar strain-rate factors, cell scaled; MD_ABSORB | MD_KICK2 runs the
//                   mirror image after the kick.  One evaluation per step (phase stays 0), no fixcm.  tests/nhc_ref.py restates it.
//   k_md_step_flex  MD_NPT_NHC_FLEX / MD_NPT_NHC_AXES: the same factorisation with a symmetric strain-rate matrix Vg in place of veps
//                   -- all six components free, or the three diagonal ones -- and 3x3 matrix exponentials in place of the scalar
//                   factors.  tests/nhc_flex_ref.py restates it.
// What the families share is written once, as inlined helpers ("what every family shares" below): the replica view, the frozen and
// finite checks with the retry protocol, the absorb row pass with the family's kick as a functor, thread 0's bookkeeping, the momentum
// scaling pass and the next configuration; the chain families also share the chain state's way through registers and the extended energy.
#pragma once

#include <hip/hip_runtime.h>

#include "mat3.h"   // mm3, det3, inv3, wave_sum_f64
#include "philox.h"

namespace chg {

enum : int { MD_RUNNING = 0, MD_NONFINITE = 1 };
enum : int { MD_NVE = 0, MD_NVT_BERENDSEN = 1, MD_NPT_BERENDSEN_INHOMOGENEOUS = 2, MD_NPT_BERENDSEN = 3, MD_NVT_LANGEVIN = 4,   // k_md_step
             MD_NVT_NHC = 5, MD_NPT_NHC = 6,             // k_md_step_nhc
             MD_NPT_NHC_FLEX = 7, MD_NPT_NHC_AXES = 8 };   // k_md_step_flex
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


// one frame slot (null scal: no frame this launch)
struct MdFrame {
  double *scal, *pos, *mom, *cell;   // [B, MD_FRAME_SCAL] [N, 3] [N, 3] [B, 9]
  double* cons;                      // [B] H - Epot (Nose-Hoover chains) or null
  float *force, *stress, *cfea;      // [N, 3] [B, 9], [B, fea_dim] or null
  float* mag;                        // [N] site moments or null: written by k_md_mag_gather (kernels_md_magmom.h), not by the step kernels
};

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
  MdFrame fr;
  // next configuration to evaluate
  double* frac_next;      // [N, 3]
  double* lat_next;       // [B, 9]
  int* retry;             // [B] set to 1 (state untouched) when the evaluation is non-finite and final_try == 0
  double dt, temperature, taut, taup, pressure, compressibility, kB, stress_weight;
  int ensemble, fixcm, flags, final_try, fea_dim;
  // MD_NVT_LANGEVIN: c1 = exp(-friction dt), sig = sqrt((1 - c1^2) kB T), one noise key per replica
  double lg_c1, lg_sig;
  const unsigned long long* seeds;   // [B]
  // the Nose-Hoover-chain families (null / 0 otherwise): chain state, chain length 1..MD_NHC_MAX, and the strain-rate matrices of
  // k_md_step_flex
  double* nhc;            // [B, MD_NHC]
  double* vg;             // [B, MD_VG]
  int nhc_len;
  // constraint (DESIGN.md "Constraints"; null: none, the <false> instantiations): [N, 3] 1 = component held, and the number of free
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

// ---- what every family shares --------------------------------------------------------------------------------------------------------
// MASK: a.fixed and a.nfree are set; <false> is the unconstrained kernel.  Under MASK the absorbed forces and every write of p are
// masked (selects, no divergent branch), so held components neither drift nor enter a sum.

// the replica this workgroup steps: its rows of the state arrays, its doubles and ints
template <bool MASK>
struct MdReplica {
  int o, a0, n;
  double *r, *p, *f, *sd;
  const double* m;
  int* si;
  const unsigned char* fixed;
  const int* nfree;
  __device__ __forceinline__ explicit MdReplica(const MdStepArgs& a) {
    o = a.sel ? a.sel[blockIdx.x] : blockIdx.x;
    a0 = a.aoff[o];
    n = a.aoff[o + 1] - a0;
    r = a.r + 3 * (size_t)a0;
    p = a.p + 3 * (size_t)a0;
    f = a.f + 3 * (size_t)a0;
    m = a.m + a0;
    sd = a.sd + (size_t)MD_SD * o;
    si = a.si + (size_t)MD_SI * o;
    fixed = MASK ? a.fixed + 3 * (size_t)a0 : nullptr;
    nfree = MASK ? a.nfree + o : nullptr;
  }
  // degrees of freedom of the temperature and N_f of the chains (a held atom breaks momentum conservation): the free components of a
  // replica that holds any, else 3 n and 3 (n - 1); evaluated where they are used, so <false> never reads nfree
  __device__ __forceinline__ double dof() const { return (MASK && *nfree < 3 * n) ? (double)*nfree : 3.0 * n; }
  __device__ __forceinline__ double nhc_nf() const { return (MASK && *nfree < 3 * n) ? (double)*nfree : 3.0 * (n - 1); }
  __device__ __forceinline__ size_t row(int i) const { return 3 * ((size_t)a0 + i); }   // row i in the batch's numbering
};

// the LDS every kernel needs: workgroup reductions, thread 0's verdicts and factor, L^-1 of the next configuration
struct MdShared {
  double red[4][7], lam, Linv[9];
  int fin[4], status, phase, go;
};

// true for a frozen replica (NONFINITE): neither moved nor logged again.  Leaves the phase in sh.phase.
template <bool MASK>
__device__ __forceinline__ bool md_frozen(const MdReplica<MASK>& v, MdShared& sh) {
  if (threadIdx.x == 0) { sh.status = v.si[1]; sh.phase = v.si[2]; }
  __syncthreads();
  return sh.status != MD_RUNNING;
}

// MD_ABSORB: false when energy, forces or stress are non-finite; the replica then asks for the retry on the wide-range sweep, or on
// the final try is marked NONFINITE, and the caller returns with the state untouched
template <bool MASK>
__device__ __forceinline__ bool md_absorb_finite(const MdStepArgs& a, const MdReplica<MASK>& v, MdShared& sh) {
  const int tid = threadIdx.x;
  int fin = 1;
  for (int i = tid; i < v.n; i += 256) {
    const float* fi = a.force + v.row(i);
    fin &= isfinite(fi[0]) && isfinite(fi[1]) && isfinite(fi[2]);
  }
  fin = __all(fin);
  if ((tid & 63) == 0) sh.fin[tid >> 6] = fin;
  __syncthreads();
  if (tid == 0) {
    int ok = sh.fin[0] & sh.fin[1] & sh.fin[2] & sh.fin[3] & (int)isfinite(a.energy[v.o]);
    if (a.stress)
      for (int i = 0; i < 9; ++i) ok &= (int)isfinite(a.stress[9 * (size_t)v.o + i]);
    if (!ok) {
      if (a.final_try) v.si[1] = MD_NONFINITE;
      else a.retry[v.o] = 1;
    }
    sh.go = ok;
  }
  __syncthreads();
  return sh.go != 0;
}

// The row pass of MD_ABSORB: the new forces are masked and cached, p takes the family's kick -- kick(p_i[3], f_i[3]) on one row, a no-op
// without MD_KICK2 -- and the row goes to the frame (its momenta only with FRAME_MOM: a family that scales p afterwards writes them in
// md_scale_momenta).  G: sum p p / m as xx yy zz yz xz xy, reduced over the workgroup, on thread 0 only.
template <bool MASK, bool FRAME_MOM, class Kick>
__device__ __forceinline__ void md_absorb_rows(const MdStepArgs& a, const MdReplica<MASK>& v, MdShared& sh, Kick&& kick, double (&G)[6]) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const bool frame = a.fr.scal != nullptr;
  double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = tid; i < v.n; i += 256) {
    const float* fi = a.force + v.row(i);
    const unsigned held = md_held_bits<MASK>(v.fixed, i);
    auto fm = [&](int j) -> float { return (MASK && ((held >> j) & 1u)) ? 0.0f : fi[j]; };   // cached, kicked with and reported
    double pi[3] = {v.p[3 * i], v.p[3 * i + 1], v.p[3 * i + 2]};
    const double fj[3] = {fm(0), fm(1), fm(2)};
    kick(pi, fj);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      v.f[3 * i + j] = fj[j];
      pi[j] = md_free<MASK>(held, j, pi[j]);
      v.p[3 * i + j] = pi[j];
    }
    const double im = 1.0 / v.m[i];
    acc[0] += pi[0] * pi[0] * im; acc[1] += pi[1] * pi[1] * im; acc[2] += pi[2] * pi[2] * im;
    acc[3] += pi[1] * pi[2] * im; acc[4] += pi[0] * pi[2] * im; acc[5] += pi[0] * pi[1] * im;
    if (frame) {
      const size_t ro = v.row(i);
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        a.fr.pos[ro + j] = v.r[3 * i + j];
        if (FRAME_MOM) a.fr.mom[ro + j] = pi[j];
        a.fr.force[ro + j] = fm(j);
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 6; ++k) acc[k] = wave_sum_f64(acc[k]);
  if (lane == 0)
    for (int k = 0; k < 6; ++k) sh.red[wv][k] = acc[k];
  __syncthreads();
  if (tid == 0)
    for (int k = 0; k < 6; ++k) G[k] = sh.red[0][k] + sh.red[1][k] + sh.red[2][k] + sh.red[3][k];
}

// thread 0: Epot and the stress (eV/A^3) of the absorbed evaluation into sd
template <bool MASK>
__device__ __forceinline__ void md_store_potential(const MdStepArgs& a, const MdReplica<MASK>& v) {
  v.sd[18] = a.energy[v.o];
  if (a.stress)
    for (int i = 0; i < 9; ++i) v.sd[21 + i] = (double)a.stress[9 * (size_t)v.o + i] * a.stress_weight;
}

// thread 0, after the kick: Ekin, T and sum p p / m into sd, and the frame's per-replica entries.  G is the sum before the chain's
// factor s scaled the momenta (1: no chain), K2 = s^2 tr G; cons: H - Epot of the chain families, else null.
template <bool MASK>
__device__ __forceinline__ void md_store_kinetic_frame(const MdStepArgs& a, const MdReplica<MASK>& v, const double (&G)[6], double K2, double s,
                                                       const double* cons) {
  const size_t o = v.o;
  const double ekin = 0.5 * K2;
  const double T = (!MASK || v.dof() > 0.0) ? 2.0 * ekin / (v.dof() * a.kB) : 0.0;   // everything held (NVE only): T = 0
  v.sd[19] = ekin;
  v.sd[20] = T;
  const double s2 = s * s;
  const double Gm[9] = {G[0], G[5], G[4], G[5], G[1], G[3], G[4], G[3], G[2]};
  for (int i = 0; i < 9; ++i) v.sd[30 + i] = Gm[i] * s2;
  if (!a.fr.scal) return;
  a.fr.scal[MD_FRAME_SCAL * o] = a.energy[o];
  a.fr.scal[MD_FRAME_SCAL * o + 1] = ekin;
  a.fr.scal[MD_FRAME_SCAL * o + 2] = T;
  if (cons && a.fr.cons) a.fr.cons[o] = *cons;
  for (int i = 0; i < 9; ++i) a.fr.cell[9 * o + i] = v.sd[i];
  for (int i = 0; i < 9; ++i) a.fr.stress[9 * o + i] = a.stress ? a.stress[9 * o + i] : 0.0f;
  if (a.cfea && a.fr.cfea)
    for (int i = 0; i < a.fea_dim; ++i) a.fr.cfea[(size_t)a.fea_dim * o + i] = a.cfea[(size_t)a.fea_dim * o + i];
}

// p <- s p, and the frame's momenta when there is a frame
template <bool MASK>
__device__ __forceinline__ void md_scale_momenta(const MdStepArgs& a, const MdReplica<MASK>& v, double s) {
  const bool frame = a.fr.scal != nullptr;
  for (int i = threadIdx.x; i < v.n; i += 256) {
    const unsigned held = md_held_bits<MASK>(v.fixed, i);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double pj = md_free<MASK>(held, j, v.p[3 * i + j] * s);
      v.p[3 * i + j] = pj;
      if (frame) a.fr.mom[v.row(i) + j] = pj;
    }
  }
}

// thread 0: the cell in sd is the one evaluated next; its inverse goes to LDS for md_write_frac
template <bool MASK>
__device__ __forceinline__ void md_next_cell(const MdStepArgs& a, const MdReplica<MASK>& v, MdShared& sh) {
  for (int i = 0; i < 9; ++i) { sh.Linv[i] = v.sd[9 + i]; a.lat_next[9 * (size_t)v.o + i] = v.sd[i]; }
}

// row i of the next configuration: y L^-1 for the cartesian position y
template <bool MASK>
__device__ __forceinline__ void md_write_frac(const MdStepArgs& a, const MdReplica<MASK>& v, const MdShared& sh, int i, double y0, double y1,
                                              double y2) {
  double* fr = a.frac_next + v.row(i);
#pragma unroll
  for (int j = 0; j < 3; ++j) fr[j] = y0 * sh.Linv[j] + y1 * sh.Linv[3 + j] + y2 * sh.Linv[6 + j];
}

// ---- the Verlet family: NVE, Berendsen NVT / NPT, Langevin ------------------------------------------------------------------------------

// MD_START of MD_NVT_LANGEVIN, BAOAB up to the evaluation: B A O A.  The noise counter is the number of steps this replica has completed
// (thread 0 has just counted the step that MD_KICK2 finished).
template <bool MASK>
__device__ __forceinline__ void md_start_langevin(const MdStepArgs& a, const MdReplica<MASK>& v, MdShared& sh) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, n = v.n;
  double *r = v.r, *p = v.p;
  const double hdt = 0.5 * a.dt;
  __shared__ double s_mean[3];
  __shared__ int s_steps;
  __syncthreads();
  if (tid == 0) {
    s_steps = v.si[0];
    md_next_cell(a, v, sh);
  }
  __syncthreads();
  const unsigned long long seed = a.seeds[v.o];
  const unsigned step = (unsigned)s_steps;
  const bool noisy = a.lg_sig > 0.0;
  double ps[4] = {0.0, 0.0, 0.0, 0.0};   // sum p, sum m
  for (int i = tid; i < n; i += 256) {
    const double mi = v.m[i];
    double xi[3] = {0.0, 0.0, 0.0};
    if (noisy) philox_normal3(seed, (unsigned)i, step, xi);
    const double sg = a.lg_sig * sqrt(mi);
    const unsigned held = md_held_bits<MASK>(v.fixed, i);   // the noise of a held component is drawn and dropped
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      double pj = md_free<MASK>(held, j, p[3 * i + j] + hdt * v.f[3 * i + j]);
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
      for (int j = 0; j < 4; ++j) sh.red[wv][j] = ps[j];
    __syncthreads();
    if (tid == 0) {
      const double im = 1.0 / (sh.red[0][3] + sh.red[1][3] + sh.red[2][3] + sh.red[3][3]);
      for (int j = 0; j < 3; ++j) s_mean[j] = (sh.red[0][j] + sh.red[1][j] + sh.red[2][j] + sh.red[3][j]) * im;   // centre-of-mass velocity
    }
    __syncthreads();
  }
  for (int i = tid; i < n; i += 256) {
    const double mi = v.m[i];
    const unsigned held = md_held_bits<MASK>(v.fixed, i);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double pj = md_free<MASK>(held, j, a.fixcm ? p[3 * i + j] - mi * s_mean[j] : p[3 * i + j]);
      p[3 * i + j] = pj;
      r[3 * i + j] += hdt * pj / mi;
    }
    md_write_frac(a, v, sh, i, r[3 * i], r[3 * i + 1], r[3 * i + 2]);
  }
}

template <bool MASK>
static __global__ __launch_bounds__(256) void k_md_step(MdStepArgs a) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const MdReplica<MASK> v(a);
  const int n = v.n;
  double *r = v.r, *p = v.p, *sd = v.sd;
  const bool npt = a.ensemble == MD_NPT_BERENDSEN_INHOMOGENEOUS || a.ensemble == MD_NPT_BERENDSEN;
  const double hdt = 0.5 * a.dt;

  __shared__ MdShared sh;
  __shared__ double sM[9], s_mean[3];

  if (md_frozen(v, sh)) return;
  bool advance = false;                 // first half kick, fixcm, drift follow

  if (a.flags & MD_ABSORB) {
    if (!md_absorb_finite(a, v, sh)) return;
    if (sh.phase == 1) {                // NPT: forces of the scaled configuration
      for (int i = tid; i < n; i += 256) {
        const float* fi = a.force + v.row(i);
        const unsigned held = md_held_bits<MASK>(v.fixed, i);
#pragma unroll
        for (int j = 0; j < 3; ++j) v.f[3 * i + j] = md_free<MASK>(held, j, fi[j]);
      }
      if (tid == 0) {
        md_store_potential(a, v);
        v.si[2] = 0;
        sh.lam = 1.0;
      }
      advance = true;
    } else {
      const bool kick = a.flags & MD_KICK2;
      double G[6];
      md_absorb_rows<MASK, true>(a, v, sh, [&](double (&pi)[3], const double (&fj)[3]) {
        if (!kick) return;
#pragma unroll
        for (int j = 0; j < 3; ++j) pi[j] = pi[j] + hdt * fj[j];
      }, G);
      if (tid == 0) {
        md_store_potential(a, v);
        md_store_kinetic_frame(a, v, G, G[0] + G[1] + G[2], 1.0, nullptr);
        if (kick) v.si[0] += 1;
      }
    }
  }

  if ((a.flags & MD_START) && a.ensemble == MD_NVT_LANGEVIN) { md_start_langevin(a, v, sh); return; }

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
      sh.lam = lam;
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
        md_next_cell(a, v, sh);
        v.si[2] = 1;
      }
    }
    __syncthreads();
    const double lam = sh.lam;
    for (int i = tid; i < n; i += 256) {
      const unsigned held = md_held_bits<MASK>(v.fixed, i);
#pragma unroll
      for (int j = 0; j < 3; ++j) p[3 * i + j] = md_free<MASK>(held, j, p[3 * i + j] * lam);
      if (npt) {
        const double x0 = r[3 * i], x1 = r[3 * i + 1], x2 = r[3 * i + 2];
#pragma unroll
        for (int j = 0; j < 3; ++j) r[3 * i + j] = x0 * sM[j] + x1 * sM[3 + j] + x2 * sM[6 + j];
        md_write_frac(a, v, sh, i, r[3 * i], r[3 * i + 1], r[3 * i + 2]);
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
    const unsigned held = md_held_bits<MASK>(v.fixed, i);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double pj = md_free<MASK>(held, j, p[3 * i + j] + hdt * v.f[3 * i + j]);
      p[3 * i + j] = pj;
      ps[j] += pj;
    }
  }
  if (a.fixcm) {
#pragma unroll
    for (int j = 0; j < 3; ++j) ps[j] = wave_sum_f64(ps[j]);
    if (lane == 0)
      for (int j = 0; j < 3; ++j) sh.red[wv][j] = ps[j];
  }
  if (tid == 0) md_next_cell(a, v, sh);
  __syncthreads();
  if (tid == 0)
    for (int j = 0; j < 3; ++j) s_mean[j] = a.fixcm ? (sh.red[0][j] + sh.red[1][j] + sh.red[2][j] + sh.red[3][j]) / (double)n : 0.0;
  __syncthreads();
  for (int i = tid; i < n; i += 256) {
    const double mi = v.m[i];
    const unsigned held = md_held_bits<MASK>(v.fixed, i);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double pj = md_free<MASK>(held, j, a.fixcm ? p[3 * i + j] - s_mean[j] : p[3 * i + j]);
      p[3 * i + j] = pj;
      r[3 * i + j] += a.dt * pj / mi;
    }
    md_write_frac(a, v, sh, i, r[3 * i], r[3 * i + 1], r[3 * i + 2]);
  }
}

// ---- Nose-Hoover chains ----------------------------------------------------------------------------------------------------------------

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

// half a step (tau) of the chain kept at xs[at .. at + 4) (velocities) and xs[at + 4 .. at + 8) (positions), through registers: returns s
__device__ inline double nhc_chain_at(double* xs, int at, int M, double Q0, double Qk, double K2, double dof, double kT, double tau) {
  double v[MD_NHC_MAX], eta[MD_NHC_MAX];
#pragma unroll
  for (int k = 0; k < MD_NHC_MAX; ++k) { v[k] = xs[at + k]; eta[k] = xs[at + 4 + k]; }
  const double s = nhc_chain(v, eta, M, Q0, Qk, K2, dof, kT, tau);
#pragma unroll
  for (int k = 0; k < MD_NHC_MAX; ++k) { xs[at + k] = v[k]; xs[at + 4 + k] = eta[k]; }
  return s;
}

// half a step of the particle chain: returns s, K2 *= s^2
__device__ inline double nhc_particle_chain(const NhcConst& c, double* xs, int M, double& K2, double tau) {
  const double s = nhc_chain_at(xs, 0, M, c.Q0, c.Qk, K2, c.nf, c.kT, tau);
  K2 *= s * s;
  return s;
}

// half a step of the isotropic barostat's chain: veps *= s
__device__ inline void nhc_barostat_chain(const NhcConst& c, double* xs, int M, double& veps, double tau) {
  veps *= nhc_chain_at(xs, 8, M, c.Qb, c.Qb, c.W * veps * veps, 1.0, c.kT, tau);
}

// H - Epot of the extended system: kinetic energy, the particle chain's energies and, for NPT, Pext V and the barostat's: Kb its
// kinetic energy, Qb0 and db the first mass and the degrees of freedom of its chain (isotropic: Qb and 1)
__device__ inline double nhc_extended_energy(const NhcConst& c, const double* x, int M, double K2, bool npt, double pext, double vol, double Kb,
                                             double Qb0, double db) {
  double h = 0.5 * K2;
  for (int k = 0; k < M; ++k) h += 0.5 * (k == 0 ? c.Q0 : c.Qk) * x[k] * x[k] + (k == 0 ? c.nf : 1.0) * c.kT * x[4 + k];
  if (npt) {
    h += pext * vol + Kb;
    for (int k = 0; k < M; ++k) h += 0.5 * (k == 0 ? Qb0 : c.Qb) * x[8 + k] * x[8 + k] + (k == 0 ? db : 1.0) * c.kT * x[12 + k];
  }
  return h;
}

// Vt = alpha K2 - V tr sigma - 3 Pext V: the isotropic barostat's kick, veps += tau Vt / W (sd: the replica's, stress absorbed)
__device__ __forceinline__ void nhc_barostat_kick(const NhcConst& c, double& veps, double K2, double vol, const double* sd, double pext, double tau) {
  veps += tau * (c.alpha * K2 - vol * (sd[21] + sd[25] + sd[29]) - 3.0 * pext * vol) / c.W;
}

template <bool MASK>
static __global__ __launch_bounds__(256) void k_md_step_nhc(MdStepArgs a) {
  const int tid = threadIdx.x;
  const MdReplica<MASK> v(a);
  const int n = v.n, M = a.nhc_len;
  double *r = v.r, *p = v.p, *sd = v.sd;
  const bool npt = a.ensemble == MD_NPT_NHC;
  double* xs = a.nhc + (size_t)MD_NHC * v.o;
  const double hdt = 0.5 * a.dt;

  __shared__ MdShared sh;
  __shared__ double s_e[2];

  if (md_frozen(v, sh)) return;

  if (a.flags & MD_ABSORB) {
    if (!md_absorb_finite(a, v, sh)) return;
    // second half of the step: kick with the strain-rate factor and sum p p / m in one pass, thread 0 runs the barostat kick and the
    // two chains (their factor s scales p, Ekin and G without another reduction), one scaling pass writes the frame's momenta
    const bool kick = a.flags & MD_KICK2;
    const NhcConst c(a, v.nhc_nf());
    const double e1 = kick ? exp(-0.5 * c.alpha * xs[16] * hdt) : 1.0;
    double G[6];
    md_absorb_rows<MASK, false>(a, v, sh, [&](double (&pi)[3], const double (&fj)[3]) {
      if (!kick) return;
#pragma unroll
      for (int j = 0; j < 3; ++j) pi[j] = fma(hdt, fj[j], pi[j] * e1) * e1;   // (p e1 + dt/2 f) e1, the product p e1 rounded first
    }, G);
    if (tid == 0) {
      double K2 = G[0] + G[1] + G[2], s = 1.0;
      const double vol = fabs(det3(sd));
      md_store_potential(a, v);
      if (kick) {
        double veps = xs[16];
        if (npt) nhc_barostat_kick(c, veps, K2, vol, sd, a.pressure, hdt);
        s = nhc_particle_chain(c, xs, M, K2, hdt);
        if (npt) {
          nhc_barostat_chain(c, xs, M, veps, hdt);
          xs[16] = veps;
        }
        v.si[0] += 1;
      }
      const double cons = nhc_extended_energy(c, xs, M, K2, npt, a.pressure, vol, 0.5 * c.W * xs[16] * xs[16], c.Qb, 1.0);
      xs[17] = cons;
      md_store_kinetic_frame(a, v, G, K2, s, &cons);
      sh.lam = s;
    }
    __syncthreads();
    if (kick || a.fr.scal) md_scale_momenta(a, v, sh.lam);
  }

  if (!(a.flags & MD_START)) return;
  // up to the evaluation: barostat chain, particle chain, barostat kick (cached stress, sum p p / m scaled by s^2), then one pass
  // p <- (p s e1 + dt/2 f) e1, r <- (r e2 + dt p / m) e2 with e1 = exp(-alpha veps dt/4), e2 = exp(veps dt/2); the cell scales by e2^2
  __syncthreads();   // sd, the chain state and p written above
  if (tid == 0) {
    const NhcConst c(a, v.nhc_nf());
    double veps = xs[16], K2 = sd[30] + sd[34] + sd[38];
    if (npt) nhc_barostat_chain(c, xs, M, veps, hdt);
    const double s = nhc_particle_chain(c, xs, M, K2, hdt);
    if (npt) {
      double L[9];
      for (int i = 0; i < 9; ++i) L[i] = sd[i];
      nhc_barostat_kick(c, veps, K2, fabs(det3(L)), sd, a.pressure, hdt);
      xs[16] = veps;
      const double eh = exp(veps * a.dt);
      for (int i = 0; i < 9; ++i) { L[i] *= eh; sd[i] = L[i]; }
      inv3(L, sd + 9);
    }
    sh.lam = s;
    s_e[0] = exp(-0.5 * c.alpha * veps * hdt);
    s_e[1] = exp(0.5 * veps * a.dt);
    md_next_cell(a, v, sh);
  }
  __syncthreads();
  const double e1 = s_e[0], e2 = s_e[1], se1 = sh.lam * e1;
  for (int i = tid; i < n; i += 256) {
    const double idm = a.dt / v.m[i];
    const unsigned held = md_held_bits<MASK>(v.fixed, i);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double pj = md_free<MASK>(held, j, (p[3 * i + j] * se1 + hdt * v.f[3 * i + j]) * e1);
      p[3 * i + j] = pj;
      r[3 * i + j] = (r[3 * i + j] * e2 + idm * pj) * e2;
    }
    md_write_frac(a, v, sh, i, r[3 * i], r[3 * i + 1], r[3 * i + 2]);
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
  const double s = nhc_chain_at(xs, 8, M, fc.Qb0, c.Qb, flex_k2(fc, vg), fc.db, c.kT, tau);
#pragma unroll
  for (int k = 0; k < 6; ++k) vg[k] *= s;
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

template <bool MASK>
static __global__ __launch_bounds__(256) void k_md_step_flex(MdStepArgs a) {
  const int tid = threadIdx.x;
  const MdReplica<MASK> v(a);
  const int n = v.n, M = a.nhc_len;
  double *r = v.r, *p = v.p, *sd = v.sd;
  double* xs = a.nhc + (size_t)MD_NHC * v.o;
  double* gv = a.vg + (size_t)MD_VG * v.o;
  const double hdt = 0.5 * a.dt;

  __shared__ MdShared sh;
  __shared__ double sE1[6], sE2[6];

  if (md_frozen(v, sh)) return;

  if (a.flags & MD_ABSORB) {
    const bool kick = a.flags & MD_KICK2;
    if (tid == 0 && kick) {   // the kick's factor from the state alone: published by the barriers of the finite check
      const NhcConst c(a, v.nhc_nf());
      double vg[6], e[6];
      flex_load_vg(gv, vg);
      flex_kick_factor(c, vg, hdt, e);
      for (int k = 0; k < 6; ++k) sE1[k] = e[k];
    }
    if (!md_absorb_finite(a, v, sh)) return;

    // second half of the step: p <- (p E1 + dt/2 f) E1 and sum p p / m in one pass, thread 0 runs the barostat kick and the two chains,
    // one scaling pass writes the frame's momenta
    double pp[6];
    md_absorb_rows<MASK, false>(a, v, sh, [&](double (&pi)[3], const double (&fj)[3]) {
      if (!kick) return;
      double q[3];
      row_sym(pi, sE1, q);
#pragma unroll
      for (int j = 0; j < 3; ++j) q[j] += hdt * fj[j];
      row_sym(q, sE1, pi);
    }, pp);
    if (tid == 0) {
      const NhcConst c(a, v.nhc_nf());
      const FlexConst fc(c, a.ensemble);
      double vg[6];
      double K2 = pp[0] + pp[1] + pp[2], s = 1.0;
      const double vol = fabs(det3(sd));
      md_store_potential(a, v);
      flex_load_vg(gv, vg);
      if (kick) {
        flex_barostat_kick(c, fc, vg, pp, K2, vol, sd + 21, a.pressure, hdt);
        s = nhc_particle_chain(c, xs, M, K2, hdt);
        flex_barostat_chain(c, fc, xs, M, vg, hdt);
        flex_store_vg(gv, vg);
        v.si[0] += 1;
      }
      const double cons = nhc_extended_energy(c, xs, M, K2, true, a.pressure, vol, 0.5 * flex_k2(fc, vg), fc.Qb0, fc.db);
      xs[17] = cons;
      md_store_kinetic_frame(a, v, pp, K2, s, &cons);
      sh.lam = s;
    }
    __syncthreads();
    if (kick || a.fr.scal) md_scale_momenta(a, v, sh.lam);
  }

  if (!(a.flags & MD_START)) return;
  // up to the evaluation: barostat chain, particle chain, barostat kick (cached stress, sum p p / m scaled by s^2), then one pass
  // p <- (p s E1 + dt/2 f) E1, r <- (r E2 + dt p / m) E2 with E2 = exp(Vg dt/2); the cell is multiplied by E2 E2 = exp(Vg dt)
  __syncthreads();   // sd, the chain state and p written above
  if (tid == 0) {
    const NhcConst c(a, v.nhc_nf());
    const FlexConst fc(c, a.ensemble);
    double vg[6], e[6], e3[6], arg[6];
    flex_load_vg(gv, vg);
    flex_barostat_chain(c, fc, xs, M, vg, hdt);
    double K2 = sd[30] + sd[34] + sd[38];
    const double s = nhc_particle_chain(c, xs, M, K2, hdt), s2 = s * s;
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
    sh.lam = s;
    md_next_cell(a, v, sh);
  }
  __syncthreads();
  const double s = sh.lam;
  for (int i = tid; i < n; i += 256) {
    const double idm = a.dt / v.m[i];
    const unsigned held = md_held_bits<MASK>(v.fixed, i);
    double pi[3] = {p[3 * i] * s, p[3 * i + 1] * s, p[3 * i + 2] * s}, q[3], ri[3] = {r[3 * i], r[3 * i + 1], r[3 * i + 2]}, y[3];
    row_sym(pi, sE1, q);
#pragma unroll
    for (int j = 0; j < 3; ++j) q[j] += hdt * v.f[3 * i + j];
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
    md_write_frac(a, v, sh, i, ri[0], ri[1], ri[2]);
  }
}

}  // namespace chg
