// kernels_mc.h -- the step kernel of a batched canonical Monte Carlo run (chg_mc_*): species swaps and single-atom displacements with
// the Metropolis rule, every structure an independent replica at its own temperature.  Not in the reference.
// DESIGN.md "Monte Carlo" states the semantics; tests/mc_ref.py restates them in float64 NumPy.
//
// One workgroup (4 waves) per replica.  One lane draws the proposal and takes the decision, the others learn both through LDS; the
// frame, the best-configuration copy and the next configuration are strided over the replica's atoms by all 256 threads, so a replica
// of any size works.  All state is f64 (and integers) in HBM, no floating-point atomics.  No synchronisation or allocation: the launch
// can be graph-captured.  What one launch does is chosen by `flags`:
//   MC_ABSORB   take the evaluation of the pending trial (energy): non-finite -> retry / NONFINITE with the state untouched.  Else
//               decide, commit an accepted move to r (a swap also to site[]), count, add E_cur to the sums, keep the best configuration,
//               and write a frame when a.fr is set.  The first evaluation of a replica (si[2] == 0) only sets E_cur and the best record.
//   MC_PROPOSE  draw trial k = si[0], record it as pending, write frac_next = (r with the move applied) L^-1.
// In steady state one launch does both.  sel / final_try / retry are those of the other step kernels (engine_stepper.h).
//
// Random numbers: block(k, b) = Philox4x32-10(counter (k, b, 0, 1), key (seed & 0xffffffff, seed >> 32)); word 3 = 1 keeps the stream
// apart from the Langevin noise (philox.h, word 3 = 0).  Each block gives two uniforms.  A replica's stream depends on (seed, k) alone.
#pragma once

#include <hip/hip_runtime.h>

#include "philox.h"

namespace chg {

enum : int { MC_RUNNING = 0, MC_NONFINITE = 1 };
enum : int { MC_ABSORB = 1, MC_PROPOSE = 2 };
enum : int { MC_NONE = -1, MC_SWAP = 0, MC_DISPLACE = 1 };   // move kinds; NONE: no trial pending / the frame of the initial configuration
// doubles per replica: L[9] L^-1[9] E_cur E_best sumE sumE2 | E_trial of the last decision | pending: u_acc delta[3] | spare
constexpr int MC_SD = 32;
enum : int { MC_E_CUR = 18, MC_E_BEST = 19, MC_SUM_E = 20, MC_SUM_E2 = 21, MC_E_TRIAL = 22, MC_U_ACC = 23, MC_DELTA = 24 };
// ints per replica: trials proposed (k), status, first evaluation absorbed, pending kind, i, j, last decision accepted, spare
constexpr int MC_SI = 8;
// 64-bit counts per replica: swap trials, swap acceptances, displacement trials, displacement acceptances, samples, 3 spare
constexpr int MC_SL = 8;
constexpr int MC_FRAME_SCAL = 6;   // frame doubles per replica: E_cur, E_trial, u_acc, delta[3]
constexpr int MC_FRAME_INT = 6;    // frame ints per replica: trials decided, kind, i, j, accepted, spare

// one frame slot (null scal: no frame this launch)
struct McFrame {
  double *scal, *pos;   // [B, MC_FRAME_SCAL] [N, 3]
  int *ints, *site;     // [B, MC_FRAME_INT]  [N]
};

struct McStepArgs {
  // state, replica o owns atom rows aoff[o]..aoff[o+1]; atom indices inside a replica are local
  double* r;               // [N, 3] cartesian positions of the current configuration
  int* site;               // [N]    input row atom a sits on (local)
  double* sd;              // [B, MC_SD]
  int* si;                 // [B, MC_SI]
  long long* sl;           // [B, MC_SL]
  double* best_pos;        // [N, 3] positions and site[] of the lowest energy seen
  int* best_site;          // [N]
  const double* temp;      // [B] K
  const unsigned long long* seeds;   // [B]
  const int* aoff;         // [B + 1]
  // atom lists, fixed at creation; replica o owns entries aoff[o] .. aoff[o] + count
  const int* mov;          // movable atoms in atom order, n_mov[o] of them
  const int* swp;          // swappable atoms sorted by (species, atom), n_swp[o] of them
  const int* gstart;       // per entry of swp: where its species group starts in the replica's list
  const int* gsize;        // ... and how many members it has
  const int *n_mov, *n_swp;   // [B]
  // the evaluation (MC_ABSORB)
  const float* energy;     // [B] eV/atom if intensive else eV
  const int* sel;          // [grid] replicas this launch steps (null: all, grid = B)
  McFrame fr;
  double* frac_next;       // [N, 3] next configuration to evaluate (the cell never moves)
  int* retry;              // [B] set to 1 (state untouched) when the evaluation is non-finite and final_try == 0
  double swap_probability, max_displacement, kB;
  int flags, final_try, intensive;
};

// what the deciding lane tells the others
struct McShared {
  int status, go, kind, i, j, acc, keep_best;
  double d[3];
};

// the two uniforms of block b of trial k
__device__ __forceinline__ void mc_uniform2(unsigned long long seed, unsigned k, unsigned b, double* u0, double* u1) {
  const uint32_t c[4] = {k, b, 0u, 1u};
  uint32_t w[4];
  philox4x32_10(c, (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), w);
  *u0 = philox_uniform(w[0], w[1]);
  *u1 = philox_uniform(w[2], w[3]);
}

// min(floor(u n), n - 1); never negative, so an empty list (which creation refuses wherever it can be drawn from) stays in bounds
__device__ __forceinline__ int mc_pick(double u, int n) { return max(min((int)(u * (double)n), n - 1), 0); }

static __global__ __launch_bounds__(256) void k_mc_step(McStepArgs a) {
  __shared__ McShared sh;
  const int tid = threadIdx.x;
  const int o = a.sel ? a.sel[blockIdx.x] : blockIdx.x;
  const int a0 = a.aoff[o], n = a.aoff[o + 1] - a0;
  double* r = a.r + 3 * (size_t)a0;
  int* site = a.site + a0;
  double* sd = a.sd + (size_t)MC_SD * o;
  int* si = a.si + (size_t)MC_SI * o;
  if (tid == 0) sh.status = si[1];
  __syncthreads();
  if (sh.status != MC_RUNNING) return;   // NONFINITE: neither moved nor logged again

  if (a.flags & MC_ABSORB) {
    if (tid == 0) {   // the decision
      long long* sl = a.sl + (size_t)MC_SL * o;
      const float ef = a.energy[o];
      sh.go = 0; sh.kind = MC_NONE; sh.i = -1; sh.j = -1; sh.acc = 0; sh.keep_best = 0;
      sh.d[0] = sh.d[1] = sh.d[2] = 0.0;
      if (!isfinite(ef)) {
        if (a.final_try) si[1] = MC_NONFINITE;
        else a.retry[o] = 1;
      } else {
        const double E = a.intensive ? (double)ef * (double)n : (double)ef;
        double u_acc = 0.0;
        sh.go = 1;
        if (!si[2]) {   // the configuration as given: neither a trial nor a sample
          si[2] = 1;
          sd[MC_E_CUR] = E;
          sd[MC_E_BEST] = E;
          sh.keep_best = 1;
        } else if (si[3] != MC_NONE) {
          const int kind = si[3];
          const double dE = E - sd[MC_E_CUR], T = a.temp[o];
          u_acc = sd[MC_U_ACC];
          const int acc = (dE <= 0.0 || (T > 0.0 && u_acc < exp(-dE / (a.kB * T)))) ? 1 : 0;
          sh.kind = kind; sh.i = si[4]; sh.j = si[5]; sh.acc = acc;
          sh.d[0] = sd[MC_DELTA]; sh.d[1] = sd[MC_DELTA + 1]; sh.d[2] = sd[MC_DELTA + 2];
          sl[2 * kind] += 1;
          sl[2 * kind + 1] += acc;
          if (acc) sd[MC_E_CUR] = E;
          const double Ec = sd[MC_E_CUR];
          sl[4] += 1;
          sd[MC_SUM_E] += Ec;
          sd[MC_SUM_E2] += Ec * Ec;
          if (acc && Ec < sd[MC_E_BEST]) { sd[MC_E_BEST] = Ec; sh.keep_best = 1; }
          si[3] = MC_NONE;
          si[6] = acc;
        } else {
          sh.go = 0;   // nothing pending: the host never asks for this
        }
        if (sh.go) {
          sd[MC_E_TRIAL] = E;
          if (a.fr.scal) {
            double* fs = a.fr.scal + (size_t)MC_FRAME_SCAL * o;
            int* fi = a.fr.ints + (size_t)MC_FRAME_INT * o;
            fs[0] = sd[MC_E_CUR]; fs[1] = E; fs[2] = u_acc; fs[3] = sh.d[0]; fs[4] = sh.d[1]; fs[5] = sh.d[2];
            fi[0] = si[0]; fi[1] = sh.kind; fi[2] = sh.i; fi[3] = sh.j; fi[4] = sh.acc; fi[5] = 0;
          }
        }
      }
    }
    __syncthreads();
    if (!sh.go) return;
    if (sh.acc && tid < 3) {   // commit: at most two rows change, one lane per component
      const int i = sh.i, j = sh.j;
      if (sh.kind == MC_SWAP) {
        const double ri = r[3 * i + tid];
        r[3 * i + tid] = r[3 * j + tid];
        r[3 * j + tid] = ri;
        if (tid == 0) { const int s = site[i]; site[i] = site[j]; site[j] = s; }
      } else {
        r[3 * i + tid] += sh.d[tid];
      }
    }
    __syncthreads();
    if (a.fr.scal || sh.keep_best) {
      double *fp = a.fr.scal ? a.fr.pos + 3 * (size_t)a0 : nullptr, *bp = sh.keep_best ? a.best_pos + 3 * (size_t)a0 : nullptr;
      int *fsite = a.fr.scal ? a.fr.site + a0 : nullptr, *bsite = sh.keep_best ? a.best_site + a0 : nullptr;
      for (int x = tid; x < n; x += 256) {
        const double p0 = r[3 * x], p1 = r[3 * x + 1], p2 = r[3 * x + 2];
        const int s = site[x];
        if (fp) { fp[3 * x] = p0; fp[3 * x + 1] = p1; fp[3 * x + 2] = p2; fsite[x] = s; }
        if (bp) { bp[3 * x] = p0; bp[3 * x + 1] = p1; bp[3 * x + 2] = p2; bsite[x] = s; }
      }
    }
    __syncthreads();   // sh is rewritten below
  }

  if (a.flags & MC_PROPOSE) {
    if (tid == 0) {   // the draw
      const unsigned long long seed = a.seeds[o];
      const unsigned k = (unsigned)si[0];
      double u_kind, u_acc, u1, u2;
      mc_uniform2(seed, k, 0u, &u_kind, &u_acc);
      mc_uniform2(seed, k, 1u, &u1, &u2);
      int kind, i, j = -1;
      double d[3] = {0.0, 0.0, 0.0};
      if (u_kind < a.swap_probability) {
        const int ns = a.n_swp[o];
        const int* list = a.swp + a0;
        const int t = mc_pick(u1, ns);
        const int gs = a.gstart[a0 + t], ng = a.gsize[a0 + t];
        int t2 = mc_pick(u2, ns - ng);   // one of the entries outside t's species group
        if (t2 >= gs) t2 += ng;
        kind = MC_SWAP; i = list[t]; j = list[t2];
      } else {
        double u3, u4;
        mc_uniform2(seed, k, 2u, &u3, &u4);
        kind = MC_DISPLACE; i = a.mov[a0 + mc_pick(u1, a.n_mov[o])];
        d[0] = a.max_displacement * (2.0 * u2 - 1.0);
        d[1] = a.max_displacement * (2.0 * u3 - 1.0);
        d[2] = a.max_displacement * (2.0 * u4 - 1.0);
      }
      si[0] = (int)(k + 1u);
      si[3] = kind; si[4] = i; si[5] = j;
      sd[MC_U_ACC] = u_acc;
      sd[MC_DELTA] = d[0]; sd[MC_DELTA + 1] = d[1]; sd[MC_DELTA + 2] = d[2];
      sh.kind = kind; sh.i = i; sh.j = j;
      sh.d[0] = d[0]; sh.d[1] = d[1]; sh.d[2] = d[2];
    }
    __syncthreads();
    const int kind = sh.kind, i = sh.i, j = sh.j;
    const double* Li = sd + 9;
    double* fn = a.frac_next + 3 * (size_t)a0;
    for (int x = tid; x < n; x += 256) {
      const int src = (kind == MC_SWAP && x == i) ? j : (kind == MC_SWAP && x == j) ? i : x;
      double p0 = r[3 * src], p1 = r[3 * src + 1], p2 = r[3 * src + 2];
      if (kind == MC_DISPLACE && x == i) { p0 += sh.d[0]; p1 += sh.d[1]; p2 += sh.d[2]; }
#pragma unroll
      for (int c = 0; c < 3; ++c) fn[3 * x + c] = p0 * Li[c] + p1 * Li[3 + c] + p2 * Li[6 + c];
    }
  }
}

}  // namespace chg
