// kernels_mc_exchange.h -- the replica-exchange event of a Monte Carlo batch (chg_mc_set_exchange): neighbouring rungs of a tempering
// ladder exchange their configurations by the Metropolis rule on the two current energies.  Not in the reference.
// DESIGN.md "Monte Carlo", part "Replica exchange", states the rule; tests/mc_exchange_ref.py restates it in NumPy.
//
// A rung is a batch slot: it keeps its temperature, seed, Philox stream, counters, sums and best record.  What moves is the
// configuration: the n position rows, site[] and E_cur, and with them the walker id.  One workgroup (4 waves) per pair of the event; the
// pairs of one event are disjoint, so no two workgroups touch the same replica or the same walker and nothing needs an atomic.  Lane 0
// draws and decides and tells the others through LDS; the row exchange and the best-record copies are strided over the atoms by all 256
// threads, so a replica of any size works.  All f64 and integers in HBM, no floating-point atomics, no synchronisation or allocation.
//
// Random number of event m, pair with lower replica a: U(w0, w1) of Philox4x32-10(counter (m, 0, 0, 2), key (seed_a & 0xffffffff,
// seed_a >> 32)); word 3 = 2 keeps the stream apart from the proposals (1, kernels_mc.h) and the Langevin noise (0, philox.h).
#pragma once

#include "kernels_mc.h"

namespace chg {

// ints per replica of the exchange state xi
constexpr int MC_XI = 6;
enum : int { MC_X_WALKER = 0, MC_X_ATTEMPTS = 1, MC_X_ACCEPTS = 2, MC_X_MARK = 3, MC_X_TRIPS = 4 };
// walker marks: where the lineage was last seen at an end of its ladder (0: at neither yet)
enum : int { MC_MARK_NONE = 0, MC_MARK_BOTTOM = 1, MC_MARK_TOP = 2 };
constexpr int MC_PAIR_INTS = 3;   // per pair of a list: the lower replica a (the upper one is a + 1), its ladder's first slot and length

struct McExchangeArgs {
  double* r;               // [N, 3]
  int* site;               // [N]
  double* sd;              // [B, MC_SD]
  const int* si;           // [B, MC_SI]  only the status is read
  double* best_pos;        // [N, 3]
  int* best_site;          // [N]
  const double* temp;      // [B] K, > 0 for every ladder member
  const unsigned long long* seeds;   // [B]
  const int* aoff;         // [B + 1]
  int* xi;                 // [B, MC_XI]  walker, attempts, accepts | mark, trips of walker w of a ladder at row first + w | spare
  const int* pairs;        // [grid, MC_PAIR_INTS] the pairs of this event's parity
  double kB;
  unsigned m;              // the event number, >= 1
};

struct McExchangeShared {
  int acc, keep_a, keep_b;
};

static __global__ __launch_bounds__(256) void k_mc_exchange(McExchangeArgs x) {
  __shared__ McExchangeShared sh;
  const int tid = threadIdx.x;
  const int* pr = x.pairs + (size_t)MC_PAIR_INTS * blockIdx.x;
  const int a = pr[0], b = a + 1;
  const int a0 = x.aoff[a], b0 = x.aoff[b], n = x.aoff[a + 1] - a0;   // both members hold n atoms: the host refuses a ladder otherwise
  if (tid == 0) {
    sh.acc = 0; sh.keep_a = 0; sh.keep_b = 0;
    if (x.si[(size_t)MC_SI * a + 1] == MC_RUNNING && x.si[(size_t)MC_SI * b + 1] == MC_RUNNING) {
      const int first = pr[1], L = pr[2], p = a - first;
      double* sa = x.sd + (size_t)MC_SD * a;
      double* sb = x.sd + (size_t)MC_SD * b;
      int* xa = x.xi + (size_t)MC_XI * a;
      int* xb = x.xi + (size_t)MC_XI * b;
      const unsigned long long seed = x.seeds[a];
      const uint32_t c[4] = {x.m, 0u, 0u, 2u};
      uint32_t w[4];
      philox4x32_10(c, (uint32_t)(seed & 0xffffffffu), (uint32_t)(seed >> 32), w);
      const double u = philox_uniform(w[0], w[1]);
      const double Ea = sa[MC_E_CUR], Eb = sb[MC_E_CUR];
      const double beta_a = 1.0 / (x.kB * x.temp[a]), beta_b = 1.0 / (x.kB * x.temp[b]);
      const double delta = (beta_a - beta_b) * (Ea - Eb);
      const int acc = (delta >= 0.0 || u < exp(delta)) ? 1 : 0;
      xa[MC_X_ATTEMPTS] += 1;
      xa[MC_X_ACCEPTS] += acc;
      if (acc) {
        sa[MC_E_CUR] = Eb;
        sb[MC_E_CUR] = Ea;
        const int wa = xb[MC_X_WALKER], wb = xa[MC_X_WALKER];   // the walkers rungs a and b hold from now on
        xa[MC_X_WALKER] = wa;
        xb[MC_X_WALKER] = wb;
        if (p == 0) {   // wa reached the bottom: a journey that has seen the top is complete
          int* row = x.xi + (size_t)MC_XI * (first + wa);
          if (row[MC_X_MARK] == MC_MARK_TOP) row[MC_X_TRIPS] += 1;
          row[MC_X_MARK] = MC_MARK_BOTTOM;
        }
        if (p + 1 == L - 1) {   // wb reached the top
          int* row = x.xi + (size_t)MC_XI * (first + wb);
          if (row[MC_X_MARK] == MC_MARK_BOTTOM) row[MC_X_MARK] = MC_MARK_TOP;
        }
        if (Eb < sa[MC_E_BEST]) { sa[MC_E_BEST] = Eb; sh.keep_a = 1; }
        if (Ea < sb[MC_E_BEST]) { sb[MC_E_BEST] = Ea; sh.keep_b = 1; }
        sh.acc = 1;
      }
    }
  }
  __syncthreads();
  if (!sh.acc) return;
  double *ra = x.r + 3 * (size_t)a0, *rb = x.r + 3 * (size_t)b0;
  int *ta = x.site + a0, *tb = x.site + b0;
  double *ba = sh.keep_a ? x.best_pos + 3 * (size_t)a0 : nullptr, *bb = sh.keep_b ? x.best_pos + 3 * (size_t)b0 : nullptr;
  int *bsa = x.best_site + a0, *bsb = x.best_site + b0;
  for (int i = tid; i < n; i += 256) {   // every row is read and written by this thread alone
    const double p0 = ra[3 * i], p1 = ra[3 * i + 1], p2 = ra[3 * i + 2];
    const double q0 = rb[3 * i], q1 = rb[3 * i + 1], q2 = rb[3 * i + 2];
    const int s = ta[i], t = tb[i];
    ra[3 * i] = q0; ra[3 * i + 1] = q1; ra[3 * i + 2] = q2; ta[i] = t;
    rb[3 * i] = p0; rb[3 * i + 1] = p1; rb[3 * i + 2] = p2; tb[i] = s;
    if (ba) { ba[3 * i] = q0; ba[3 * i + 1] = q1; ba[3 * i + 2] = q2; bsa[i] = t; }
    if (bb) { bb[3 * i] = p0; bb[3 * i + 1] = p1; bb[3 * i + 2] = p2; bsb[i] = s; }
  }
}

}  // namespace chg
