// engine_md_observe.h -- host side of the MD observers (kernels_md_obs.h, kernels_md_transport.h, kernels_md_magmom.h): the plain
// observers with their ring, and the transport and charge-state accumulators that hang on them.  Host code of engine_md.hip alone, as
// engine_stepper.h is shared host code.  What the MD driver uses: create_observers / create_transport / create_charge (each block frees
// itself with its owner), sample_due, observe() for one sample, the three downloads, and carve_frame; test_observe and the
// chg_test_md_* entry points below run caller-given snapshots through the same observe().
#pragma once

#include <memory>

#include "engine_stepper.h"

#include "kernels_md_obs.h"
#include "kernels_md_transport.h"
#include "kernels_md_magmom.h"

// chg_md_set_charge_states / chg_test_md_charge_states: parameters and one device allocation of its own (boundaries, moment and state
// ring, accumulators, and for a run the moment slot of the observers' private frame)
struct MdCharge {
  chg_md_charge_params p{};
  DeviceBlock mem;
  double *bounds = nullptr, *ring_m = nullptr, *msum = nullptr, *msq = nullptr, *mcorr = nullptr, *vol_sum = nullptr;
  int *n_bounds = nullptr, *ring_q = nullptr, *prev_q = nullptr;
  unsigned long long *mhist = nullptr, *shist = nullptr;
  long long *pop = nullptr, *trans = nullptr, *occ = nullptr, *same = nullptr, *samples = nullptr, *skipped = nullptr;
  float* fr_mag = nullptr;
};

// chg_md_set_transport / chg_test_md_transport: parameters and one device allocation of its own (current ring and accumulators)
struct MdTransport {
  chg_md_transport_params p{};
  DeviceBlock mem;
  double *ring_j = nullptr, *msd4 = nullptr, *cmsd = nullptr, *jacf = nullptr, *vol_sum = nullptr;
  unsigned long long* vh = nullptr;
  long long* samples = nullptr;
};

// chg_md_set_observers / chg_test_md_observe: parameters, one device allocation of its own (ring, accumulators, and for a run the
// private frame slot), and the number of samples taken
struct MdObservers {
  chg_md_observe_params p{};
  int B = 0, N = 0, n_max = 0;   // n_max: atoms of the largest replica (grid of the pair-image kernels)
  long long k = 0;               // samples taken
  DeviceBlock mem;
  int* species = nullptr;
  double *ring_pos = nullptr, *ring_vel = nullptr, *ring_com = nullptr, *msd = nullptr, *vacf = nullptr, *vol_sum = nullptr;
  long long *cnt = nullptr, *rdf_samples = nullptr;
  unsigned long long* hist = nullptr;
  chg::MdFrame fr{};                 // private frame slot: what the step kernels write of a completed step that is sampled but not logged
  std::unique_ptr<MdTransport> tr;   // chg_md_set_transport: reads the ring above
  std::unique_ptr<MdCharge> cs;      // chg_md_set_charge_states: its own ring, the same sample number and slot
};

namespace {

// one frame slot of the step kernels (kernels_md.h): the MD driver's ring and the observers' private slot are made of these
MdFrame carve_frame(Carver& c, size_t B, size_t N, bool cfea, bool cons) {
  MdFrame f{};
  f.scal = c.take<double>(MD_FRAME_SCAL * B);
  f.pos = c.take<double>(3 * N);
  f.mom = c.take<double>(3 * N);
  f.cell = c.take<double>(9 * B);
  f.force = c.take<float>(3 * N);
  f.stress = c.take<float>(9 * B);
  if (cfea) f.cfea = c.take<float>(chg::D * B);
  if (cons) f.cons = c.take<double>(B);
  return f;
}

// the pair-image kernels (k_md_obs_rdf, k_md_chg_srdf): MD_OBS_RDF_ROWS atoms per workgroup, rows * S * bins uint32 counts of dynamic LDS
struct RdfLaunch {
  dim3 grid;
  size_t lds;
};
RdfLaunch rdf_launch(const MdObservers* x, int rows, int bins) {
  return {dim3((unsigned)((x->n_max + MD_OBS_RDF_ROWS - 1) / MD_OBS_RDF_ROWS), (unsigned)x->B), sizeof(unsigned) * rows * x->p.n_species * bins};
}
template <class K>
int rdf_set_lds(chg_engine* eng, const char* fn, K kernel, const RdfLaunch& g) {
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)g.lds) == hipSuccess) return CHG_OK;
  eng->err = std::string(fn) + ": the histogram does not fit the LDS";
  return CHG_EHIP;
}

// ---- observers (kernels_md_obs.h)

const char* bad_observe(const chg_md_observe_params* p) {
  if (p->sample_interval < 1) return "sample_interval must be >= 1";
  if (p->n_lags < 0 || p->n_lags > MD_OBS_MAX_LAGS) return "n_lags must be 0..4096";
  if (p->n_species < 1 || p->n_species > MD_OBS_SPECIES) return "n_species must be 1..8";
  if (p->rdf_bins < 0) return "rdf_bins must be >= 0";
  if (p->rdf_bins > 0 && (!(p->rdf_rmax > 0.0) || !std::isfinite(p->rdf_rmax))) return "rdf_rmax must be > 0 and finite";
  if ((int64_t)p->n_species * p->n_species * p->rdf_bins > MD_OBS_RDF_CELLS)
    return "n_species * n_species * rdf_bins must be <= 16384 (the histogram lives in 64 KB of LDS)";
  if (p->n_lags == 0 && p->rdf_bins == 0) return "nothing to observe: n_lags and rdf_bins are both 0";
  return nullptr;
}

void carve_obs(MdObservers* x, Carver& c, bool frame_slot) {
  const size_t B = x->B, N = x->N, L = x->p.n_lags, S = x->p.n_species, bins = x->p.rdf_bins;
  x->species = c.take<int>(N);
  x->ring_pos = c.take<double>(L * 3 * N);
  x->ring_vel = c.take<double>(L * 3 * N);
  x->ring_com = c.take<double>(L * 3 * B);
  x->msd = c.take<double>(B * L * S);
  x->vacf = c.take<double>(B * L * S);
  x->cnt = c.take<long long>(B * L);
  x->hist = c.take<unsigned long long>(B * S * S * bins);
  x->rdf_samples = c.take<long long>(B);
  x->vol_sum = c.take<double>(B);
  if (frame_slot) x->fr = carve_frame(c, B, N, false, false);
}

// parameters and species checked, buffers allocated, accumulators zeroed, species uploaded (synchronised)
int create_observers(chg_engine* eng, const char* fn, const chg_md_observe_params* p, int B, const int* aoff, const int32_t* species,
                     bool frame_slot, std::unique_ptr<MdObservers>& out) {
  if (const char* bad = bad_observe(p)) { eng->err = std::string(fn) + ": " + bad; return CHG_EINVAL; }
  const int N = aoff[B];
  for (int i = 0; i < N; ++i)
    if (species[i] < 0 || species[i] >= p->n_species) {
      eng->err = std::string(fn) + ": species index " + std::to_string(species[i]) + " of atom " + std::to_string(i) + " is outside 0.." +
                 std::to_string(p->n_species - 1);
      return CHG_EINVAL;
    }
  auto x = std::make_unique<MdObservers>();
  x->p = *p;
  x->B = B; x->N = N;
  for (int o = 0; o < B; ++o) x->n_max = std::max(x->n_max, aoff[o + 1] - aoff[o]);
  TRY(alloc_block(eng, fn, "observer state", [&](Carver& c) { carve_obs(x.get(), c, frame_slot); }, &x->mem.p, nullptr,
                  " (ring of " + std::to_string(p->n_lags) + " snapshots)"));
  StateUpload up{eng, fn};
  up(x->species, species, sizeof(int) * (size_t)N);
  up.zero(x->msd, (size_t)((char*)(x->vol_sum + B) - (char*)x->msd));   // every accumulator: msd .. vol_sum are carved in a row
  TRY(up.finish());
  if (p->rdf_bins > 0) TRY(rdf_set_lds(eng, fn, k_md_obs_rdf, rdf_launch(x.get(), p->n_species, p->rdf_bins)));
  out = std::move(x);
  return CHG_OK;
}

int download_observables(chg_engine* eng, const MdObservers* x, const chg_md_observables_host* o) {
  const size_t B = x->B, L = x->p.n_lags, S = x->p.n_species, bins = x->p.rdf_bins;
  TRY(d2h(eng, o->msd, x->msd, B * L * S));
  TRY(d2h(eng, o->vacf, x->vacf, B * L * S));
  TRY(d2h(eng, (long long*)o->cnt, x->cnt, B * L));
  TRY(d2h(eng, (unsigned long long*)o->rdf, x->hist, B * S * S * bins));
  TRY(d2h(eng, (long long*)o->rdf_samples, x->rdf_samples, B));
  TRY(d2h(eng, o->vol_sum, x->vol_sum, B));
  HIP_TRY(eng, hipStreamSynchronize(eng->stream));
  return CHG_OK;
}

// ---- transport accumulators on the observers' ring (kernels_md_transport.h)

const char* bad_transport(const MdObservers* x, const chg_md_transport_params* t) {
  if (!x || x->p.n_lags == 0) return "transport needs observers with n_lags > 0 (chg_md_set_observers)";
  if (t->vh_bins < 0) return "vh_bins must be >= 0";
  if (!t->collective && !t->non_gaussian && t->vh_bins == 0) return "nothing requested: collective, non_gaussian and vh_bins are all 0";
  if (t->vh_bins > 0) {
    if (!(t->vh_rmax > 0.0) || !std::isfinite(t->vh_rmax)) return "vh_rmax must be > 0 and finite";
    if (t->vh_stride < 1) return "vh_stride must be >= 1";
    if (t->vh_lags < 1) return "vh_lags must be >= 1";
    if (((int64_t)t->vh_lags - 1) * t->vh_stride >= x->p.n_lags) return "(vh_lags - 1) * vh_stride must be < n_lags";
    if ((int64_t)x->p.n_species * t->vh_bins > MD_OBS_VH_CELLS) return "n_species * vh_bins must be <= 4096 (the histogram lives in 16 KB of LDS)";
  }
  return nullptr;
}

void carve_transport(const MdObservers* x, MdTransport* t, Carver& c) {
  const size_t B = x->B, L = x->p.n_lags, S = x->p.n_species;
  const size_t cells = t->p.vh_bins > 0 ? B * t->p.vh_lags * S * t->p.vh_bins : 0;
  t->ring_j = c.take<double>(t->p.collective ? L * B * S * 3 : 0);
  t->msd4 = c.take<double>(t->p.non_gaussian ? B * L * S : 0);
  t->cmsd = c.take<double>(t->p.collective ? B * L * S * S : 0);
  t->jacf = c.take<double>(t->p.collective ? B * L * S * S : 0);
  t->vh = c.take<unsigned long long>(cells);
  t->samples = c.take<long long>(B);
  t->vol_sum = c.take<double>(B);
}

// parameters checked against the observers they hang on, buffers allocated and zeroed (synchronised)
int create_transport(chg_engine* eng, const char* fn, const MdObservers* x, const chg_md_transport_params* p, std::unique_ptr<MdTransport>& out) {
  if (const char* bad = bad_transport(x, p)) { eng->err = std::string(fn) + ": " + bad; return CHG_EINVAL; }
  auto t = std::make_unique<MdTransport>();
  t->p = *p;
  if (t->p.vh_bins == 0) { t->p.vh_lags = 0; t->p.vh_stride = 1; t->p.vh_rmax = 0.0; }
  size_t bytes = 0;
  TRY(alloc_block(eng, fn, "transport accumulators", [&](Carver& c) { carve_transport(x, t.get(), c); }, &t->mem.p, &bytes));
  StateUpload up{eng, fn};
  up.zero(t->mem.p, bytes);
  TRY(up.finish());
  out = std::move(t);
  return CHG_OK;
}

// the transport kernels of the sample k_md_obs_push has just put into the ring
void observe_transport(chg_engine* eng, const MdObservers* x, const MdSnapshot& s, const MdRing& r, unsigned lags) {
  const MdTransport* t = x->tr.get();
  const MdTransportArgs b{s, r, t->ring_j, t->p.collective != 0, t->p.non_gaussian != 0, t->msd4, t->cmsd, t->jacf, t->vh, t->samples, t->vol_sum,
                          t->p.vh_bins, t->p.vh_lags, t->p.vh_stride, t->p.vh_rmax};
  hipLaunchKernelGGL(k_md_obs_current, dim3((unsigned)x->B), dim3(256), 0, eng->stream, b);
  hipLaunchKernelGGL(k_md_obs_transport, dim3(lags, (unsigned)x->B), dim3(256), 0, eng->stream, b);
}

int download_transport(chg_engine* eng, const MdObservers* x, const chg_md_transport_host* o) {
  const MdTransport* t = x->tr.get();
  const size_t B = x->B, L = x->p.n_lags, S = x->p.n_species;
  TRY(d2h(eng, o->msd4, t->msd4, t->p.non_gaussian ? B * L * S : 0));
  TRY(d2h(eng, o->cmsd, t->cmsd, t->p.collective ? B * L * S * S : 0));
  TRY(d2h(eng, o->jacf, t->jacf, t->p.collective ? B * L * S * S : 0));
  TRY(d2h(eng, (unsigned long long*)o->vh, t->vh, t->p.vh_bins > 0 ? B * t->p.vh_lags * S * t->p.vh_bins : 0));
  TRY(d2h(eng, (long long*)o->samples, t->samples, B));
  TRY(d2h(eng, o->vol_sum, t->vol_sum, B));
  HIP_TRY(eng, hipStreamSynchronize(eng->stream));
  return CHG_OK;
}

// ---- charge-state observers on the observers' sample counter (kernels_md_magmom.h)

const char* bad_charge(const MdObservers* x, const chg_md_charge_params* p, const double* bounds) {
  if (!x) return "charge states need observers (chg_md_set_observers)";
  const int S = x->p.n_species;
  int total = 0;
  for (int s = 0; s < S; ++s) {
    if (p->n_bounds[s] < 0 || p->n_bounds[s] > MD_CHG_BOUNDS) return "n_bounds must be 0..3";
    for (int j = 0; j < p->n_bounds[s]; ++j) {
      const double v = bounds[MD_CHG_BOUNDS * s + j];
      if (!std::isfinite(v) || v < 0.0 || (j > 0 && !(v > bounds[MD_CHG_BOUNDS * s + j - 1]))) return "boundaries must be finite, >= 0 and ascending";
    }
    total += p->n_bounds[s];
  }
  if (p->mag_bins < 0) return "mag_bins must be >= 0";
  if (p->srdf_bins < 0) return "srdf_bins must be >= 0";
  if (total == 0 && p->mag_bins == 0 && p->srdf_bins == 0) return "nothing requested: no boundary, mag_bins and srdf_bins are 0";
  if ((int64_t)S * p->mag_bins > MD_CHG_HIST_CELLS) return "n_species * mag_bins must be <= 4096 (the histogram lives in 16 KB of LDS)";
  if (p->mag_bins > 0 && (!(p->mag_max > 0.0) || !std::isfinite(p->mag_max))) return "mag_max must be > 0 and finite";
  if ((int64_t)MD_CHG_STATES * S * p->srdf_bins > MD_CHG_SRDF_CELLS)
    return "4 * n_species * srdf_bins must be <= 16384 (the histogram lives in 64 KB of LDS)";
  if (p->srdf_bins > 0) {
    if (p->center_species < 0 || p->center_species >= S) return "center_species must be 0 .. n_species - 1 when srdf_bins > 0";
    if (!(p->srdf_rmax > 0.0) || !std::isfinite(p->srdf_rmax)) return "srdf_rmax must be > 0 and finite";
  }
  return nullptr;
}

void carve_charge(const MdObservers* x, MdCharge* c, Carver& k, bool frame_slot) {
  const size_t B = x->B, N = x->N, L = x->p.n_lags, S = x->p.n_species, Q = MD_CHG_STATES;
  c->bounds = k.take<double>(S * MD_CHG_BOUNDS);
  c->n_bounds = k.take<int>(S);
  c->ring_m = k.take<double>(L * N);
  c->ring_q = k.take<int>(L * N);
  c->prev_q = k.take<int>(N);
  c->mhist = k.take<unsigned long long>(B * S * c->p.mag_bins);
  c->msum = k.take<double>(B * S);
  c->msq = k.take<double>(B * S);
  c->pop = k.take<long long>(B * S * Q);
  c->trans = k.take<long long>(B * S * Q * Q);
  c->occ = k.take<long long>(N * Q);
  c->mcorr = k.take<double>(B * L * S);
  c->same = k.take<long long>(B * L * S * Q);
  c->shist = k.take<unsigned long long>(B * Q * S * c->p.srdf_bins);
  c->samples = k.take<long long>(B);
  c->skipped = k.take<long long>(B);
  c->vol_sum = k.take<double>(B);
  if (frame_slot) c->fr_mag = k.take<float>(N);
}

// parameters checked against the observers they hang on, buffers allocated and zeroed, boundaries uploaded (synchronised)
int create_charge(chg_engine* eng, const char* fn, const MdObservers* x, const chg_md_charge_params* p, const double* bounds, bool frame_slot,
                  std::unique_ptr<MdCharge>& out) {
  if (const char* bad = bad_charge(x, p, bounds)) { eng->err = std::string(fn) + ": " + bad; return CHG_EINVAL; }
  auto c = std::make_unique<MdCharge>();
  c->p = *p;
  const int S = x->p.n_species;
  if (c->p.mag_bins == 0) c->p.mag_max = 0.0;
  if (c->p.srdf_bins == 0) { c->p.center_species = -1; c->p.srdf_rmax = 0.0; }
  size_t bytes = 0;
  TRY(alloc_block(eng, fn, "charge-state ring and accumulators", [&](Carver& k) { carve_charge(x, c.get(), k, frame_slot); }, &c->mem.p, &bytes));
  std::vector<double> hb((size_t)S * MD_CHG_BOUNDS, 0.0);
  for (int s = 0; s < S; ++s)
    for (int j = 0; j < p->n_bounds[s]; ++j) hb[MD_CHG_BOUNDS * s + j] = bounds[MD_CHG_BOUNDS * s + j];
  StateUpload up{eng, fn};
  up.zero(c->mem.p, bytes);
  if (up.s == CHG_OK && hipMemsetAsync(c->prev_q, 0xFF, sizeof(int) * (size_t)x->N, eng->stream) != hipSuccess) up.fail("state initialisation failed");
  up(c->bounds, hb.data(), sizeof(double) * hb.size());
  up(c->n_bounds, p->n_bounds, sizeof(int) * S);
  TRY(up.finish());
  if (p->srdf_bins > 0) TRY(rdf_set_lds(eng, fn, k_md_chg_srdf, rdf_launch(x, MD_CHG_STATES, p->srdf_bins)));
  out = std::move(c);
  return CHG_OK;
}

// the charge-state kernels of the sample (s carries its moments)
void observe_charge(chg_engine* eng, const MdObservers* x, const MdSnapshot& s, const MdRing& r, unsigned lags) {
  const MdCharge* c = x->cs.get();
  const MdChgArgs b{s, r, c->bounds, c->n_bounds, c->ring_m, c->ring_q, c->prev_q, c->mhist, c->msum, c->msq, c->pop, c->trans, c->occ, c->mcorr,
                    c->same, c->shist, c->samples, c->skipped, c->vol_sum, c->p.mag_bins, c->p.center_species, c->p.srdf_bins, c->p.mag_max,
                    c->p.srdf_rmax};
  hipLaunchKernelGGL(k_md_chg_sample, dim3((unsigned)x->B), dim3(256), 0, eng->stream, b);
  if (r.L > 0) hipLaunchKernelGGL(k_md_chg_corr, dim3(lags, (unsigned)x->B), dim3(256), 0, eng->stream, b);
  if (c->p.srdf_bins > 0) {
    const RdfLaunch g = rdf_launch(x, MD_CHG_STATES, c->p.srdf_bins);
    hipLaunchKernelGGL(k_md_chg_srdf, g.grid, dim3(256), g.lds, eng->stream, b);
  }
}

int download_charge(chg_engine* eng, const MdObservers* x, const chg_md_charge_host* o) {
  const MdCharge* c = x->cs.get();
  const size_t B = x->B, N = x->N, L = x->p.n_lags, S = x->p.n_species, Q = MD_CHG_STATES;
  TRY(d2h(eng, (unsigned long long*)o->mhist, c->mhist, B * S * c->p.mag_bins));
  TRY(d2h(eng, o->msum, c->msum, B * S));
  TRY(d2h(eng, o->msq, c->msq, B * S));
  TRY(d2h(eng, (long long*)o->pop, c->pop, B * S * Q));
  TRY(d2h(eng, (long long*)o->trans, c->trans, B * S * Q * Q));
  TRY(d2h(eng, (long long*)o->occ, c->occ, N * Q));
  TRY(d2h(eng, o->mcorr, c->mcorr, B * L * S));
  TRY(d2h(eng, (long long*)o->same, c->same, B * L * S * Q));
  TRY(d2h(eng, (unsigned long long*)o->shist, c->shist, B * Q * S * c->p.srdf_bins));
  TRY(d2h(eng, (long long*)o->samples, c->samples, B));
  TRY(d2h(eng, (long long*)o->skipped, c->skipped, B));
  TRY(d2h(eng, o->vol_sum, c->vol_sum, B));
  HIP_TRY(eng, hipStreamSynchronize(eng->stream));
  return CHG_OK;
}

// ---- one sample

bool sample_due(const MdObservers* x, int step) { return x && step % x->p.sample_interval == 0; }

// the snapshot of a completed step through the ring and the accumulators of every family (enqueued on the engine's stream): the two
// views are filled once and handed to all three
int observe(chg_engine* eng, const char* fn, MdObservers* x, const double* pos, const double* mom, const double* cell, const double* mass,
            const int* status, int status_stride, const int* d_aoff, const float* mag = nullptr) {
  LaunchScope ls(eng, "md_observe");
  const chg_md_observe_params& p = x->p;
  const int L = p.n_lags;
  const MdSnapshot s{pos, mom, cell, mass, x->species, status, status_stride, d_aoff, x->N, x->B, p.n_species, mag};
  const MdRing r{x->ring_pos, x->ring_vel, x->ring_com, L, L > 0 ? (int)(x->k % L) : 0, x->k, p.subtract_com};
  const unsigned lags = (unsigned)std::min<long long>(x->k, std::max(L - 1, 0)) + 1;   // of this sample, with L > 0
  const MdObsArgs a{s, r, x->msd, x->vacf, x->cnt, x->hist, x->rdf_samples, x->vol_sum, p.rdf_bins, p.rdf_rmax};
  if (L > 0) {
    hipLaunchKernelGGL(k_md_obs_push, dim3((unsigned)x->B), dim3(256), 0, eng->stream, a);
    hipLaunchKernelGGL(k_md_obs_corr, dim3(lags, (unsigned)x->B), dim3(256), 0, eng->stream, a);
    if (x->tr) observe_transport(eng, x, s, r, lags);
  }
  if (p.rdf_bins > 0) {
    const RdfLaunch g = rdf_launch(x, p.n_species, p.rdf_bins);
    hipLaunchKernelGGL(k_md_obs_rdf, g.grid, dim3(256), g.lds, eng->stream, a);
  }
  if (x->cs) observe_charge(eng, x, s, r, lags);
  x->k += 1;
  if (hipGetLastError() != hipSuccess) { eng->err = std::string(fn) + ": observer kernel launch failed"; return CHG_EHIP; }
  return CHG_OK;
}

// ---- chg_test_md_observe / chg_test_md_transport / chg_test_md_charge_states

// what chg_test_md_charge_states adds to the snapshots
struct TestCharge {
  const chg_md_charge_params* params;
  const double* bounds;
  const float* magmoms;   // [T, N]
  const chg_md_charge_host* out;
};

// caller-given snapshots through observe(), then the downloads that were asked for
int test_observe(chg_engine* eng, const char* fn, const chg_md_observe_params* params, const chg_md_transport_params* transport,
                 int32_t n_struct, const int32_t* atom_off, const int32_t* species, const double* masses, int32_t n_samples,
                 const double* positions, const double* momenta, const double* cell, const int32_t* status,
                 const chg_md_observables_host* out, const chg_md_transport_host* tout, const TestCharge* charge = nullptr) {
  using namespace chgh;
  if (!eng || !params || n_struct <= 0 || !atom_off || !species || !masses || n_samples < 1 || !positions || !momenta || !cell || !status)
    return CHG_EINVAL;
  const size_t B = n_struct, T = n_samples;
  if (atom_off[0] != 0) return CHG_EINVAL;
  for (size_t o = 0; o < B; ++o)
    if (atom_off[o + 1] <= atom_off[o]) return CHG_EINVAL;
  const size_t N = atom_off[n_struct];
  HIP_TRY(eng, hipSetDevice(eng->device));
  std::unique_ptr<MdObservers> x;
  TRY(create_observers(eng, fn, params, n_struct, atom_off, species, false, x));
  if (transport) TRY(create_transport(eng, fn, x.get(), transport, x->tr));
  if (charge) TRY(create_charge(eng, fn, x.get(), charge->params, charge->bounds, false, x->cs));
  TestBuf bufs[] = {{positions, nullptr, sizeof(double) * T * 3 * N}, {momenta, nullptr, sizeof(double) * T * 3 * N},
                    {cell, nullptr, sizeof(double) * T * 9 * B}, {status, nullptr, sizeof(int) * T * B}, {masses, nullptr, sizeof(double) * N},
                    {atom_off, nullptr, sizeof(int) * (B + 1)},
                    {charge ? charge->magmoms : nullptr, nullptr, sizeof(float) * (charge ? T * N : 1)}};
  int rc = CHG_OK;
  TRY(run_test_step(eng, fn, bufs, [&] {
    for (size_t t = 0; t < T && rc == CHG_OK; ++t)
      rc = observe(eng, fn, x.get(), (const double*)bufs[0].d + t * 3 * N, (const double*)bufs[1].d + t * 3 * N,
                   (const double*)bufs[2].d + t * 9 * B, (const double*)bufs[4].d, (const int*)bufs[3].d + t * B, 1, (const int*)bufs[5].d,
                   charge ? (const float*)bufs[6].d + t * N : nullptr);
  }));
  TRY(rc);
  if (out) TRY(download_observables(eng, x.get(), out));
  if (tout) TRY(download_transport(eng, x.get(), tout));
  if (charge) TRY(download_charge(eng, x.get(), charge->out));
  return CHG_OK;
}

}  // namespace

extern "C" int chg_test_md_observe(chg_engine* eng, const chg_md_observe_params* params, int32_t n_struct, const int32_t* atom_off,
                                   const int32_t* species, const double* masses, int32_t n_samples, const double* positions,
                                   const double* momenta, const double* cell, const int32_t* status,
                                   const chg_md_observables_host* out) {
  if (!out) return CHG_EINVAL;
  return test_observe(eng, "chg_test_md_observe", params, nullptr, n_struct, atom_off, species, masses, n_samples, positions, momenta, cell,
                      status, out, nullptr);
}

extern "C" int chg_test_md_transport(chg_engine* eng, const chg_md_observe_params* params, const chg_md_transport_params* transport,
                                     int32_t n_struct, const int32_t* atom_off, const int32_t* species, const double* masses,
                                     int32_t n_samples, const double* positions, const double* momenta, const double* cell,
                                     const int32_t* status, const chg_md_observables_host* plain, const chg_md_transport_host* out) {
  if (!transport || !out) return CHG_EINVAL;
  return test_observe(eng, "chg_test_md_transport", params, transport, n_struct, atom_off, species, masses, n_samples, positions, momenta,
                      cell, status, plain, out);
}

extern "C" int chg_test_md_charge_states(chg_engine* eng, const chg_md_observe_params* params, const chg_md_charge_params* charge,
                                         const double* bounds, int32_t n_struct, const int32_t* atom_off, const int32_t* species,
                                         const double* masses, int32_t n_samples, const double* positions, const double* momenta,
                                         const double* cell, const int32_t* status, const float* magmoms,
                                         const chg_md_observables_host* plain, const chg_md_charge_host* out) {
  if (!charge || !bounds || !magmoms || !out) return CHG_EINVAL;
  const TestCharge tc{charge, bounds, magmoms, out};
  return test_observe(eng, "chg_test_md_charge_states", params, nullptr, n_struct, atom_off, species, masses, n_samples, positions, momenta,
                      cell, status, plain, nullptr, &tc);
}
