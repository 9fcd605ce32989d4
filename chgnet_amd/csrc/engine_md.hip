// engine_md.hip -- batched molecular dynamics (chg_md_*): NVE, NVT Berendsen, NPT Berendsen (inhomogeneous and isotropic), NVT
// Langevin (BAOAB with counter-based noise, chg_md_create_langevin; not in the reference), Nose-Hoover-chain NVT and isotropic NPT
// (Martyna-Tobias-Klein, chg_md_create_nhc; not in the reference) and its flexible-cell forms (chg_md_create_nhc_flex: a symmetric
// strain-rate matrix, all six components or the three diagonal ones), one independent replica per structure, state in HBM
// (kernels_md.h).  Reference: MolecularDynamics, chgnet/model/dynamics.py:433-780.
//
// One evaluation of chg_md_run is one evaluate_and_step of the shared driver (engine_stepper.h) on ALL replicas, with the ensemble's
// step kernel (kernels_md.h: k_md_step, k_md_step_nhc or k_md_step_flex) as the step launch (one workgroup per replica: finish the
// step, frame, start the next one).  Every replica runs the same number of
// steps, so there is no compaction.  NPT takes two evaluations per step, as ASE does: the barostat's set_cell(scale_atoms=True)
// moves the atoms and the forces are evaluated again before the first half kick.  The Nose-Hoover-chain NPT scales the cell inside
// the step and takes one evaluation (task efs) like every other ensemble.  chg_md_set_magmoms / chg_md_set_charge_states add the site
// moments to the task and one gather launch (kernels_md_magmom.h) after the step launch of every evaluation that completes a step.
#include "engine_stepper.h"

#include "kernels_md.h"
#include "kernels_md_obs.h"
#include "kernels_md_transport.h"
#include "kernels_md_magmom.h"

// chg_md_set_charge_states / chg_test_md_charge_states: parameters and one device allocation of its own (boundaries, moment and state
// ring, accumulators, and for a run the moment slot of the observers' private frame)
struct MdCharge {
  chg_md_charge_params p{};
  char* mem = nullptr;
  double *bounds = nullptr, *ring_m = nullptr, *msum = nullptr, *msq = nullptr, *mcorr = nullptr, *vol_sum = nullptr;
  int *n_bounds = nullptr, *ring_q = nullptr, *prev_q = nullptr;
  unsigned long long *mhist = nullptr, *shist = nullptr;
  long long *pop = nullptr, *trans = nullptr, *occ = nullptr, *same = nullptr, *samples = nullptr, *skipped = nullptr;
  float* fr_mag = nullptr;
};

// chg_md_set_transport / chg_test_md_transport: parameters and one device allocation of its own (current ring and accumulators)
struct MdTransport {
  chg_md_transport_params p{};
  char* mem = nullptr;
  double *ring_j = nullptr, *msd4 = nullptr, *cmsd = nullptr, *jacf = nullptr, *vol_sum = nullptr;
  unsigned long long* vh = nullptr;
  long long* samples = nullptr;
};

// chg_md_set_observers / chg_test_md_observe: parameters, one device allocation of its own (ring, accumulators, and for a run the
// private frame slot), and the number of samples taken
struct MdObservers {
  chg_md_observe_params p{};
  int B = 0, N = 0, n_max = 0;   // n_max: atoms of the largest replica (grid of k_md_obs_rdf)
  long long k = 0;               // samples taken
  char* mem = nullptr;
  int* species = nullptr;
  double *ring_pos = nullptr, *ring_vel = nullptr, *ring_com = nullptr, *msd = nullptr, *vacf = nullptr, *vol_sum = nullptr;
  long long *cnt = nullptr, *rdf_samples = nullptr;
  unsigned long long* hist = nullptr;
  chg::MdFrame fr{};             // private frame slot: what the step kernels write of a completed step that is sampled but not logged
  MdTransport* tr = nullptr;     // chg_md_set_transport: reads the ring above
  MdCharge* cs = nullptr;        // chg_md_set_charge_states: its own ring, the same sample number and slot
};

// the chg_md_create* / chg_test_md_step* entry point that was called: it decides which ensembles may run (bad_params)
enum class MdEntry { Plain, Langevin, Nhc, NhcFlex };

// what an entry point was given besides the structures
struct MdSpec {
  chg_md_params p{};
  MdEntry entry = MdEntry::Plain;
  double friction = 0.0;            // Langevin: inverse ASE time units
  const uint64_t* seeds = nullptr;  // Langevin: [B] noise keys on the host, read while the entry point runs
  int chain_length = 0;             // Nhc, NhcFlex
};

struct chg_md : chgh::Stepper {
  MdSpec spec;
  bool started = false;      // the initial configuration has been evaluated (frame of step 0 written)
  std::vector<double> p0;    // the momenta as created: chg_md_set_fixed derives the masked ones from them on every call
  int step = 0;              // steps completed (all replicas; a NONFINITE replica stops counting)
  // device: state + per-evaluation buffers
  double *r, *pm, *f, *m, *sd;
  int *si, *d_aoff;
  unsigned long long* seeds = nullptr;   // [B] noise keys (MD_NVT_LANGEVIN)
  double* nhc = nullptr;                 // [B, MD_NHC] chain and barostat state
  double* vg = nullptr;                  // [B, MD_VG] strain-rate matrix (MD_NPT_NHC_FLEX / MD_NPT_NHC_AXES)
  // frame ring: K slots
  int K = 0, ring_head = 0, ring_count = 0;
  std::vector<int> ring_step;
  std::vector<chg::MdFrame> ring;        // cfea only when logged, cons only for Nose-Hoover chains
  MdObservers* obs = nullptr;            // chg_md_set_observers
  // chg_md_set_magmoms (or implied by chg_md_set_charge_states): task M, k_md_mag_gather after every evaluation that completes a step
  bool mag = false, mag_frames = false;
  float *mag_mem = nullptr, *mag_last = nullptr;   // [N] moments of the last completed step, then the ring frames' slots
};

namespace {

constexpr int FEA = chg::D;

bool is_npt(int e) { return e == MD_NPT_BERENDSEN_INHOMOGENEOUS || e == MD_NPT_BERENDSEN; }   // the two-evaluation Berendsen loop
bool is_flex(int e) { return e == MD_NPT_NHC_FLEX || e == MD_NPT_NHC_AXES; }   // chg_md_create_nhc_flex only
bool is_nhc(int e) { return e == MD_NVT_NHC || e == MD_NPT_NHC || is_flex(e); }

// one frame slot
MdFrame carve_frame(Carver& c, size_t B, size_t N, bool cfea, bool cons) {
  MdFrame f{};
  f.scal = c.take<double>(MD_FRAME_SCAL * B);
  f.pos = c.take<double>(3 * N);
  f.mom = c.take<double>(3 * N);
  f.cell = c.take<double>(9 * B);
  f.force = c.take<float>(3 * N);
  f.stress = c.take<float>(9 * B);
  if (cfea) f.cfea = c.take<float>(FEA * B);
  if (cons) f.cons = c.take<double>(B);
  return f;
}

void carve_md(chg_md* d, Carver& c) {
  const size_t B = d->B, N = d->N;
  const int ensemble = d->spec.p.ensemble;
  d->r = c.take<double>(3 * N);
  d->pm = c.take<double>(3 * N);
  d->f = c.take<double>(3 * N);
  d->m = c.take<double>(N);
  d->sd = c.take<double>(MD_SD * B);
  d->frac_next = c.take<double>(3 * N);
  d->lat_next = c.take<double>(9 * B);
  d->si = c.take<int>(MD_SI * B);
  d->seeds = c.take<unsigned long long>(ensemble == MD_NVT_LANGEVIN ? B : 0);
  d->nhc = c.take<double>(is_nhc(ensemble) ? MD_NHC * B : 0);
  d->vg = c.take<double>(is_flex(ensemble) ? MD_VG * B : 0);
  d->d_aoff = c.take<int>(B + 1);
  d->d_sel = c.take<int>(B);
  d->retry = c.take<int>(B);
  d->ring.resize(d->K);
  for (MdFrame& f : d->ring) f = carve_frame(c, B, N, d->spec.p.log_crystal_fea, is_nhc(ensemble));
  d->d_fixed = c.take<unsigned char>(3 * N);
  d->d_nfree = c.take<int>(B);
}

bool nhc_npt(int e) { return e == MD_NPT_NHC || is_flex(e); }
bool moving_cell(int e) { return is_npt(e) || nhc_npt(e); }

bool is_langevin(int e) { return e == MD_NVT_LANGEVIN; }
bool is_nhc_iso(int e) { return e == MD_NVT_NHC || e == MD_NPT_NHC; }

// The entry points that carry more than chg_md_params, the ensembles only they may run, and what is said when the two do not match:
// to such an entry point about another ensemble, and to another entry point about such an ensemble.  The plain entry point runs the rest.
const struct { MdEntry entry; bool (*runs)(int ensemble); const char *other_ensemble, *other_entry; } ENTRY_RULES[] = {
    {MdEntry::NhcFlex, is_flex, "ensemble must be CHG_MD_NPT_NHC_FLEX or CHG_MD_NPT_NHC_AXES",
     "CHG_MD_NPT_NHC_FLEX / CHG_MD_NPT_NHC_AXES need a strain-rate matrix: use chg_md_create_nhc_flex"},
    {MdEntry::Nhc, is_nhc_iso, "ensemble must be CHG_MD_NVT_NHC or CHG_MD_NPT_NHC",
     "CHG_MD_NVT_NHC / CHG_MD_NPT_NHC need a chain length: use chg_md_create_nhc"},
    {MdEntry::Langevin, is_langevin, "ensemble must be CHG_MD_NVT_LANGEVIN",
     "CHG_MD_NVT_LANGEVIN needs friction and seeds: use chg_md_create_langevin"},
};

const char* bad_params(const MdSpec& s) {
  const chg_md_params* p = &s.p;
  for (const auto& rule : ENTRY_RULES)
    if ((s.entry == rule.entry) != rule.runs(p->ensemble)) return s.entry == rule.entry ? rule.other_ensemble : rule.other_entry;
  if (is_nhc(p->ensemble)) {
    if (s.chain_length < 1 || s.chain_length > MD_NHC_MAX) return "chain_length must be 1..4";
    if (!(p->temperature > 0.0) || !std::isfinite(p->temperature)) return "temperature must be > 0 (the thermostat masses are kB T tau^2)";
    if (!(p->taut > 0.0) || !std::isfinite(p->taut)) return "taut must be > 0";
    if (nhc_npt(p->ensemble) && (!(p->taup > 0.0) || !std::isfinite(p->taup) || !std::isfinite(p->pressure)))
      return "taup must be > 0 and pressure finite";
  }
  if (is_langevin(p->ensemble)) {
    if (!(s.friction >= 0.0) || !std::isfinite(s.friction)) return "friction must be >= 0 and finite";
    if (!(p->temperature >= 0.0) || !std::isfinite(p->temperature)) return "temperature must be >= 0";
  }
  if (p->ensemble < MD_NVE || p->ensemble > MD_NPT_NHC_AXES) return "unknown ensemble";
  if (!(p->dt > 0.0) || !std::isfinite(p->dt)) return "dt must be > 0";
  if (!is_langevin(p->ensemble) && p->ensemble != MD_NVE && (!(p->taut > 0.0) || !(p->temperature >= 0.0))) return "taut must be > 0 and temperature >= 0";
  if (is_npt(p->ensemble) && (!(p->taup > 0.0) || !(p->compressibility > 0.0) || !std::isfinite(p->pressure)))
    return "taup and compressibility must be > 0 and pressure finite";
  if (p->loginterval < 0 || p->ring_frames < 0) return "loginterval and ring_frames must be >= 0";
  if (p->loginterval > 0 && p->ring_frames < 1) return "frames need ring_frames >= 1";
  if (!(p->r_atom > 0.0) || !(p->r_bond > 0.0)) return "graph cutoffs must be > 0";
  return nullptr;
}

// what the parameters decide; the device pointers are the caller's
MdStepArgs base_args(const MdSpec& s) {
  MdStepArgs a{};
  const chg_md_params& p = s.p;
  a.dt = p.dt; a.temperature = p.temperature; a.taut = p.taut; a.taup = p.taup; a.pressure = p.pressure;
  a.compressibility = p.compressibility; a.kB = p.kB > 0.0 ? p.kB : 8.6173303e-5;
  a.stress_weight = p.stress_weight > 0.0 ? p.stress_weight : 1.0 / 160.21766208;
  a.ensemble = p.ensemble; a.fixcm = p.ensemble != MD_NVE && p.fixcm; a.fea_dim = FEA;
  if (is_langevin(p.ensemble)) {
    a.lg_c1 = std::exp(-s.friction * p.dt);
    a.lg_sig = std::sqrt((1.0 - a.lg_c1 * a.lg_c1) * a.kB * p.temperature);
  }
  if (is_nhc(p.ensemble)) a.nhc_len = s.chain_length;
  return a;
}

MdStepArgs handle_args(chg_md* d, int flags) {
  MdStepArgs a = base_args(d->spec);
  a.flags = flags;
  a.r = d->r; a.p = d->pm; a.f = d->f; a.m = d->m; a.sd = d->sd; a.si = d->si; a.aoff = d->d_aoff;
  a.frac_next = d->frac_next; a.lat_next = d->lat_next; a.retry = d->retry;
  a.seeds = d->seeds; a.nhc = d->nhc; a.vg = d->vg;   // placeholders of one element where the ensemble has none
  if (d->has_fixed) { a.fixed = d->d_fixed; a.nfree = d->d_nfree; }
  return a;
}

// the one place that maps the ensemble code to its kernel
void launch_step(chg_engine* eng, const MdStepArgs& a, int grid) {
  LaunchScope ls(eng, "md_step");
  void (*kernel)(MdStepArgs) = is_flex(a.ensemble) ? (a.fixed ? k_md_step_flex<true> : k_md_step_flex<false>)
                               : is_nhc(a.ensemble) ? (a.fixed ? k_md_step_nhc<true> : k_md_step_nhc<false>)
                                                    : (a.fixed ? k_md_step<true> : k_md_step<false>);
  hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(256), 0, eng->stream, a);
}

// evaluate all replicas, then one step launch with `a` (flags and frame slot set by the caller); completes: the evaluation finishes a
// step, so with chg_md_set_magmoms its moments are gathered under the rule the step kernel wrote the frame by
int evaluate_and_step(chg_engine* eng, chg_md* d, MdStepArgs a, bool completes) {
  return chgh::evaluate_and_step(eng, "chg_md_run", d, d->B, nullptr, nullptr, [&](const chg_batch* b, const int* sel, int final_try, int grid) {
    a.energy = b->energy; a.force = b->force; a.stress = (d->task & CHG_TASK_S) ? b->virial : nullptr;
    a.cfea = a.fr.cfea ? b->crystal_fea : nullptr;
    a.sel = sel;
    a.final_try = final_try;
    launch_step(eng, a, grid);
    if (d->mag && completes) {
      LaunchScope ls(eng, "md_mag_gather");
      const MdMagArgs g{b->magmom, a.fr.mag, d->mag_last, d->si, d->retry, sel, d->d_aoff, final_try};
      hipLaunchKernelGGL(k_md_mag_gather, dim3((unsigned)grid), dim3(256), 0, eng->stream, g);
    }
  });
}

// frame slot for step `step` (the caller checked that the ring has room)
void set_frame(chg_md* d, MdStepArgs& a, int step) {
  const size_t slot = (size_t)((d->ring_head + d->ring_count) % d->K);
  a.fr = d->ring[slot];
  d->ring_step[slot] = step;
  d->ring_count += 1;
}

bool frame_due(const chg_md* d, int step) { return d->spec.p.loginterval > 0 && step % d->spec.p.loginterval == 0; }

// every chg_md_create*: spec.p.ensemble, spec.entry and what that entry point carries are set by the caller
int create(chg_engine* eng, const char* fn, const chg_structs_host* h, const double* masses, const double* momenta, const MdSpec& spec,
           chg_md** out) {
  if (!eng || !h || !masses || !out) return CHG_EINVAL;
  *out = nullptr;
  const chg_md_params* params = &spec.p;
  if (const char* bad = bad_params(spec)) { eng->err = std::string(fn) + ": " + bad; return CHG_EINVAL; }
  TRY(check_structs(eng, fn, h));
  const int B = h->n_struct, N = h->n_atoms;
  if (is_nhc(params->ensemble))
    for (int o = 0; o < B; ++o)
      if (h->atom_off[o + 1] - h->atom_off[o] < 2) {
        eng->err = std::string(fn) + ": a structure of one atom has no internal degrees of freedom to thermostat";
        return CHG_EINVAL;
      }
  for (int i = 0; i < N; ++i)
    if (!(masses[i] > 0.0)) { eng->err = std::string(fn) + ": masses must be > 0"; return CHG_EINVAL; }
  HIP_TRY(eng, hipSetDevice(eng->device));
  chg_md* d = new chg_md();
  d->spec = spec;
  d->spec.seeds = nullptr;   // the caller's array: uploaded below, not kept
  d->K = params->loginterval > 0 ? params->ring_frames : 0;
  d->ring_step.assign(std::max(d->K, 1), 0);
  d->task = CHG_TASK_E | CHG_TASK_F | ((is_npt(params->ensemble) || nhc_npt(params->ensemble) || params->log_stress) ? CHG_TASK_S : 0u);
  d->r_atom = params->r_atom; d->r_bond = params->r_bond; d->numerical_tol = params->numerical_tol;
  int s = alloc_state(eng, fn, d, h, 0, [&](Carver& c) { carve_md(d, c); });
  if (s != CHG_OK) { chg_md_free(eng, d); return s; }
  // initial state on the host, one upload: cartesian positions frac . L, the cell and its inverse
  std::vector<double> r(3 * (size_t)N), sd((size_t)MD_SD * B, 0.0);
  std::vector<int> si((size_t)MD_SI * B, 0);
  for (int o = 0; o < B; ++o) initial_geometry(h, o, r.data() + 3 * (size_t)h->atom_off[o], sd.data() + (size_t)MD_SD * o);
  StateUpload up{eng, fn};
  up(d->r, r.data(), sizeof(double) * r.size());
  up(d->m, masses, sizeof(double) * N);
  up(d->sd, sd.data(), sizeof(double) * sd.size());
  up(d->si, si.data(), sizeof(int) * si.size());
  if (spec.seeds) up(d->seeds, spec.seeds, sizeof(uint64_t) * B);
  if (is_nhc(params->ensemble)) up.zero(d->nhc, sizeof(double) * MD_NHC * (size_t)B);
  if (is_flex(params->ensemble)) up.zero(d->vg, sizeof(double) * MD_VG * (size_t)B);
  up(d->d_aoff, h->atom_off, sizeof(int) * (B + 1));
  up(d->frac_next, h->frac, sizeof(double) * 3 * N);
  up(d->lat_next, h->lattice, sizeof(double) * 9 * B);
  d->p0.assign(3 * (size_t)N, 0.0);
  if (momenta) std::memcpy(d->p0.data(), momenta, sizeof(double) * 3 * (size_t)N);
  up(d->pm, d->p0.data(), sizeof(double) * 3 * N);
  up.zero(d->f, sizeof(double) * 3 * (size_t)N);
  if ((s = up.finish()) != CHG_OK) { chg_md_free(eng, d); return s; }
  *out = d;
  return CHG_OK;
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

void free_transport(MdTransport* t) {
  if (!t) return;
  if (t->mem) hipFree(t->mem);
  delete t;
}

void free_charge(MdCharge* c) {
  if (!c) return;
  if (c->mem) hipFree(c->mem);
  delete c;
}

void free_observers(MdObservers* x) {
  if (!x) return;
  free_transport(x->tr);
  free_charge(x->cs);
  if (x->mem) hipFree(x->mem);
  delete x;
}

// parameters and species checked, buffers allocated, accumulators zeroed, species uploaded (synchronised)
int create_observers(chg_engine* eng, const char* fn, const chg_md_observe_params* p, int B, const int* aoff, const int32_t* species,
                     bool frame_slot, MdObservers** out) {
  if (const char* bad = bad_observe(p)) { eng->err = std::string(fn) + ": " + bad; return CHG_EINVAL; }
  const int N = aoff[B];
  for (int i = 0; i < N; ++i)
    if (species[i] < 0 || species[i] >= p->n_species) {
      eng->err = std::string(fn) + ": species index " + std::to_string(species[i]) + " of atom " + std::to_string(i) + " is outside 0.." +
                 std::to_string(p->n_species - 1);
      return CHG_EINVAL;
    }
  MdObservers* x = new MdObservers();
  x->p = *p;
  x->B = B; x->N = N;
  for (int o = 0; o < B; ++o) x->n_max = std::max(x->n_max, aoff[o + 1] - aoff[o]);
  Carver sizer{nullptr};
  carve_obs(x, sizer, frame_slot);
  if (hipMalloc(&x->mem, sizer.pos) != hipSuccess) {
    (void)hipGetLastError();
    x->mem = nullptr;
    free_observers(x);
    eng->err = std::string(fn) + ": observer state of " + std::to_string(sizer.pos) + " bytes (ring of " + std::to_string(p->n_lags) +
               " snapshots) cannot be allocated";
    return CHG_ENOMEM;
  }
  Carver carver{x->mem};
  carve_obs(x, carver, frame_slot);
  StateUpload up{eng, fn};
  up(x->species, species, sizeof(int) * (size_t)N);
  up.zero(x->msd, (size_t)((char*)(x->vol_sum + B) - (char*)x->msd));   // every accumulator: msd .. vol_sum are carved in a row
  int s = up.finish();
  if (s == CHG_OK && p->rdf_bins > 0 &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(k_md_obs_rdf), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)(sizeof(unsigned) * p->n_species * p->n_species * p->rdf_bins)) != hipSuccess) {
    eng->err = std::string(fn) + ": the histogram does not fit the LDS";
    s = CHG_EHIP;
  }
  if (s != CHG_OK) { free_observers(x); return s; }
  *out = x;
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
int create_transport(chg_engine* eng, const char* fn, const MdObservers* x, const chg_md_transport_params* p, MdTransport** out) {
  if (const char* bad = bad_transport(x, p)) { eng->err = std::string(fn) + ": " + bad; return CHG_EINVAL; }
  MdTransport* t = new MdTransport();
  t->p = *p;
  if (t->p.vh_bins == 0) { t->p.vh_lags = 0; t->p.vh_stride = 1; t->p.vh_rmax = 0.0; }
  Carver sizer{nullptr};
  carve_transport(x, t, sizer);
  if (hipMalloc(&t->mem, sizer.pos) != hipSuccess) {
    (void)hipGetLastError();
    t->mem = nullptr;
    free_transport(t);
    eng->err = std::string(fn) + ": transport accumulators of " + std::to_string(sizer.pos) + " bytes cannot be allocated";
    return CHG_ENOMEM;
  }
  Carver carver{t->mem};
  carve_transport(x, t, carver);
  StateUpload up{eng, fn};
  up.zero(t->mem, carver.pos);
  const int s = up.finish();
  if (s != CHG_OK) { free_transport(t); return s; }
  *out = t;
  return CHG_OK;
}

// the transport kernels of the sample k_md_obs_push has just put into the ring (a: the arguments of that launch)
void observe_transport(chg_engine* eng, const MdObservers* x, const MdObsArgs& a, unsigned lags) {
  const MdTransport* t = x->tr;
  MdTransportArgs b{};
  b.cell = a.cell; b.species = a.species; b.status = a.status; b.status_stride = a.status_stride; b.aoff = a.aoff;
  b.N = a.N; b.B = a.B; b.S = a.S;
  b.ring_pos = a.ring_pos; b.ring_vel = a.ring_vel; b.ring_com = a.ring_com; b.ring_j = t->ring_j; b.L = a.L; b.slot = a.slot; b.k = a.k;
  b.subtract_com = a.subtract_com; b.collective = t->p.collective != 0; b.non_gaussian = t->p.non_gaussian != 0;
  b.msd4 = t->msd4; b.cmsd = t->cmsd; b.jacf = t->jacf; b.vh = t->vh; b.samples = t->samples; b.vol_sum = t->vol_sum;
  b.vh_bins = t->p.vh_bins; b.vh_lags = t->p.vh_lags; b.vh_stride = t->p.vh_stride; b.vh_rmax = t->p.vh_rmax;
  hipLaunchKernelGGL(k_md_obs_current, dim3((unsigned)x->B), dim3(256), 0, eng->stream, b);
  hipLaunchKernelGGL(k_md_obs_transport, dim3(lags, (unsigned)x->B), dim3(256), 0, eng->stream, b);
}

int download_transport(chg_engine* eng, const MdObservers* x, const chg_md_transport_host* o) {
  const MdTransport* t = x->tr;
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
                  MdCharge** out) {
  if (const char* bad = bad_charge(x, p, bounds)) { eng->err = std::string(fn) + ": " + bad; return CHG_EINVAL; }
  MdCharge* c = new MdCharge();
  c->p = *p;
  const int S = x->p.n_species;
  if (c->p.mag_bins == 0) c->p.mag_max = 0.0;
  if (c->p.srdf_bins == 0) { c->p.center_species = -1; c->p.srdf_rmax = 0.0; }
  Carver sizer{nullptr};
  carve_charge(x, c, sizer, frame_slot);
  if (hipMalloc(&c->mem, sizer.pos) != hipSuccess) {
    (void)hipGetLastError();
    c->mem = nullptr;
    free_charge(c);
    eng->err = std::string(fn) + ": charge-state ring and accumulators of " + std::to_string(sizer.pos) + " bytes cannot be allocated";
    return CHG_ENOMEM;
  }
  Carver carver{c->mem};
  carve_charge(x, c, carver, frame_slot);
  std::vector<double> hb((size_t)S * MD_CHG_BOUNDS, 0.0);
  for (int s = 0; s < S; ++s)
    for (int j = 0; j < p->n_bounds[s]; ++j) hb[MD_CHG_BOUNDS * s + j] = bounds[MD_CHG_BOUNDS * s + j];
  StateUpload up{eng, fn};
  up.zero(c->mem, carver.pos);
  if (up.s == CHG_OK && hipMemsetAsync(c->prev_q, 0xFF, sizeof(int) * (size_t)x->N, eng->stream) != hipSuccess) up.fail("state initialisation failed");
  up(c->bounds, hb.data(), sizeof(double) * hb.size());
  up(c->n_bounds, p->n_bounds, sizeof(int) * S);
  int s = up.finish();
  if (s == CHG_OK && p->srdf_bins > 0 &&
      hipFuncSetAttribute(reinterpret_cast<const void*>(k_md_chg_srdf), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)(sizeof(unsigned) * MD_CHG_STATES * S * p->srdf_bins)) != hipSuccess) {
    eng->err = std::string(fn) + ": the histogram does not fit the LDS";
    s = CHG_EHIP;
  }
  if (s != CHG_OK) { free_charge(c); return s; }
  *out = c;
  return CHG_OK;
}

// the charge-state kernels of sample x->k (a: the arguments of the plain observers' launches of the same sample; mag: its moments)
void observe_charge(chg_engine* eng, const MdObservers* x, const MdObsArgs& a, const float* mag) {
  const MdCharge* c = x->cs;
  MdChgArgs b{};
  b.mag = mag; b.pos = a.pos; b.cell = a.cell; b.species = a.species; b.status = a.status; b.status_stride = a.status_stride; b.aoff = a.aoff;
  b.N = a.N; b.B = a.B; b.S = a.S; b.bounds = c->bounds; b.n_bounds = c->n_bounds;
  b.ring_m = c->ring_m; b.ring_q = c->ring_q; b.L = a.L; b.slot = a.L > 0 ? (int)(x->k % a.L) : 0; b.k = x->k; b.prev_q = c->prev_q;
  b.mhist = c->mhist; b.msum = c->msum; b.msq = c->msq; b.pop = c->pop; b.trans = c->trans; b.occ = c->occ; b.mcorr = c->mcorr;
  b.same = c->same; b.shist = c->shist; b.samples = c->samples; b.skipped = c->skipped; b.vol_sum = c->vol_sum;
  b.mag_bins = c->p.mag_bins; b.center = c->p.center_species; b.srdf_bins = c->p.srdf_bins; b.mag_max = c->p.mag_max; b.srdf_rmax = c->p.srdf_rmax;
  hipLaunchKernelGGL(k_md_chg_sample, dim3((unsigned)x->B), dim3(256), 0, eng->stream, b);
  if (a.L > 0) {
    const unsigned lags = (unsigned)std::min<long long>(x->k, a.L - 1) + 1;
    hipLaunchKernelGGL(k_md_chg_corr, dim3(lags, (unsigned)x->B), dim3(256), 0, eng->stream, b);
  }
  if (c->p.srdf_bins > 0) {
    const unsigned chunks = (unsigned)((x->n_max + MD_OBS_RDF_ROWS - 1) / MD_OBS_RDF_ROWS);
    const size_t lds = sizeof(unsigned) * MD_CHG_STATES * a.S * c->p.srdf_bins;
    hipLaunchKernelGGL(k_md_chg_srdf, dim3(chunks, (unsigned)x->B), dim3(256), lds, eng->stream, b);
  }
}

int download_charge(chg_engine* eng, const MdObservers* x, const chg_md_charge_host* o) {
  const MdCharge* c = x->cs;
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

// one sample: the snapshot of a completed step through the ring and the accumulators (enqueued on the engine's stream)
int observe(chg_engine* eng, const char* fn, MdObservers* x, const double* pos, const double* mom, const double* cell, const double* mass,
            const int* status, int status_stride, const int* d_aoff, const float* mag = nullptr) {
  LaunchScope ls(eng, "md_observe");
  const chg_md_observe_params& p = x->p;
  MdObsArgs a{};
  a.pos = pos; a.mom = mom; a.cell = cell; a.mass = mass; a.species = x->species; a.status = status; a.status_stride = status_stride;
  a.aoff = d_aoff; a.N = x->N; a.B = x->B; a.S = p.n_species;
  a.ring_pos = x->ring_pos; a.ring_vel = x->ring_vel; a.ring_com = x->ring_com; a.L = p.n_lags; a.k = x->k;
  a.subtract_com = p.subtract_com; a.msd = x->msd; a.vacf = x->vacf; a.cnt = x->cnt;
  a.hist = x->hist; a.rdf_samples = x->rdf_samples; a.vol_sum = x->vol_sum; a.bins = p.rdf_bins; a.rmax = p.rdf_rmax;
  if (p.n_lags > 0) {
    a.slot = (int)(x->k % p.n_lags);
    const unsigned lags = (unsigned)std::min<long long>(x->k, p.n_lags - 1) + 1;
    hipLaunchKernelGGL(k_md_obs_push, dim3((unsigned)x->B), dim3(256), 0, eng->stream, a);
    hipLaunchKernelGGL(k_md_obs_corr, dim3(lags, (unsigned)x->B), dim3(256), 0, eng->stream, a);
    if (x->tr) observe_transport(eng, x, a, lags);
  }
  if (p.rdf_bins > 0) {
    const unsigned chunks = (unsigned)((x->n_max + MD_OBS_RDF_ROWS - 1) / MD_OBS_RDF_ROWS);
    const size_t lds = sizeof(unsigned) * p.n_species * p.n_species * p.rdf_bins;
    hipLaunchKernelGGL(k_md_obs_rdf, dim3(chunks, (unsigned)x->B), dim3(256), lds, eng->stream, a);
  }
  if (x->cs) observe_charge(eng, x, a, mag);
  x->k += 1;
  if (hipGetLastError() != hipSuccess) { eng->err = std::string(fn) + ": observer kernel launch failed"; return CHG_EHIP; }
  return CHG_OK;
}

int download_observables(chg_engine* eng, MdObservers* x, const chg_md_observables_host* o) {
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

bool sample_due(const chg_md* d, int step) { return d->obs && step % d->obs->p.sample_interval == 0; }

// one evaluation that completes step `step`: its frame goes to the ring when one is due, to the observers' private slot (not part
// of the ring, not counted in ring_count) when only a sample is, and the observers read it once the step launch -- a wide-range retry included -- has returned
int evaluate_step_observe(chg_engine* eng, chg_md* d, MdStepArgs& a, int step) {
  const bool sample = sample_due(d, step);
  if (frame_due(d, step)) set_frame(d, a, step);
  else if (sample) a.fr = d->obs->fr;
  if (sample && d->obs->cs && !a.fr.mag) a.fr.mag = d->obs->cs->fr_mag;   // a ring frame without moment slots: the observers' own
  TRY(evaluate_and_step(eng, d, a, true));
  if (sample) TRY(observe(eng, "chg_md_run", d->obs, a.fr.pos, a.fr.mom, a.fr.cell, d->m, d->si + 1, MD_SI, d->d_aoff, a.fr.mag));
  return CHG_OK;
}

// task M and the moment slots: [N] of the last completed step, then [N] per ring frame with log_frames
int enable_magmoms(chg_engine* eng, const char* fn, chg_md* d, bool log_frames) {
  const size_t N = d->N, slots = 1 + (log_frames ? (size_t)d->K : 0);
  float* mem = nullptr;
  if (hipMalloc(&mem, sizeof(float) * N * slots) != hipSuccess) {
    (void)hipGetLastError();
    eng->err = std::string(fn) + ": moment slots of " + std::to_string(sizeof(float) * N * slots) + " bytes cannot be allocated";
    return CHG_ENOMEM;
  }
  StateUpload up{eng, fn};
  up.zero(mem, sizeof(float) * N * slots);
  const int s = up.finish();
  if (s != CHG_OK) { hipFree(mem); return s; }
  if (d->mag_mem) hipFree(d->mag_mem);
  d->mag_mem = d->mag_last = mem;
  for (int k = 0; k < d->K; ++k) d->ring[k].mag = log_frames ? mem + N * (size_t)(k + 1) : nullptr;
  d->mag = true;
  d->mag_frames = log_frames;
  d->task |= CHG_TASK_M;
  return CHG_OK;
}
}  // namespace

extern "C" {

int chg_md_create(chg_engine* eng, const chg_structs_host* h, const double* masses, const double* momenta, const chg_md_params* params,
                  chg_md** out) {
  if (!params) return CHG_EINVAL;
  return create(eng, "chg_md_create", h, masses, momenta, MdSpec{*params}, out);
}

int chg_md_create_langevin(chg_engine* eng, const chg_structs_host* h, const double* masses, const double* momenta,
                           const chg_md_params* params, double friction, const uint64_t* seeds, chg_md** out) {
  if (!params || !seeds) return CHG_EINVAL;
  return create(eng, "chg_md_create_langevin", h, masses, momenta, MdSpec{*params, MdEntry::Langevin, friction, seeds}, out);
}

int chg_md_create_nhc(chg_engine* eng, const chg_structs_host* h, const double* masses, const double* momenta, const chg_md_params* params,
                      int32_t chain_length, chg_md** out) {
  if (!params) return CHG_EINVAL;
  return create(eng, "chg_md_create_nhc", h, masses, momenta, MdSpec{*params, MdEntry::Nhc, 0.0, nullptr, chain_length}, out);
}

int chg_md_create_nhc_flex(chg_engine* eng, const chg_structs_host* h, const double* masses, const double* momenta, const chg_md_params* params,
                           int32_t chain_length, int32_t cell_mode, chg_md** out) {
  if (!eng || !params) return CHG_EINVAL;
  if (cell_mode != CHG_MD_CELL_FLEXIBLE && cell_mode != CHG_MD_CELL_AXES) {
    eng->err = "chg_md_create_nhc_flex: cell_mode must be CHG_MD_CELL_FLEXIBLE or CHG_MD_CELL_AXES";
    return CHG_EINVAL;
  }
  MdSpec spec{*params, MdEntry::NhcFlex, 0.0, nullptr, chain_length};
  spec.p.ensemble = cell_mode == CHG_MD_CELL_FLEXIBLE ? MD_NPT_NHC_FLEX : MD_NPT_NHC_AXES;   // params->ensemble is ignored
  return create(eng, "chg_md_create_nhc_flex", h, masses, momenta, spec, out);
}

int chg_md_set_fixed(chg_engine* eng, chg_md* d, const uint8_t* fixed) {
  if (!eng || !d) return CHG_EINVAL;
  const char* fn = "chg_md_set_fixed";
  if (d->started) { eng->err = std::string(fn) + ": the run has already started"; return CHG_EINVAL; }
  const size_t B = d->B, N = d->N;
  std::vector<int> nfree(B);
  if (fixed) TRY(check_fixed(eng, fn, d->B, d->h_aoff, fixed, moving_cell(d->spec.p.ensemble), d->spec.p.ensemble != MD_NVE, nfree.data()));
  HIP_TRY(eng, hipSetDevice(eng->device));
  {   // the momenta as created, with the held ones at 0: a later call with another mask, or with null, starts from the created ones again
    std::vector<double> pm(d->p0);
    for (size_t k = 0; fixed && k < 3 * N; ++k)
      if (fixed[k]) pm[k] = 0.0;
    HIP_TRY(eng, hipMemcpy(d->pm, pm.data(), sizeof(double) * 3 * N, hipMemcpyHostToDevice));
  }
  return upload_fixed(eng, fn, d, fixed, nfree.data());
}

int chg_md_set_observers(chg_engine* eng, chg_md* d, const chg_md_observe_params* params, const int32_t* species) {
  if (!eng || !d || !params || !species) return CHG_EINVAL;
  const char* fn = "chg_md_set_observers";
  if (d->started) { eng->err = std::string(fn) + ": the run has already started"; return CHG_EINVAL; }
  HIP_TRY(eng, hipSetDevice(eng->device));
  MdObservers* x = nullptr;
  TRY(create_observers(eng, fn, params, d->B, d->h_aoff, species, true, &x));
  free_observers(d->obs);
  d->obs = x;
  return CHG_OK;
}

int chg_md_set_transport(chg_engine* eng, chg_md* d, const chg_md_transport_params* params) {
  if (!eng || !d || !params) return CHG_EINVAL;
  const char* fn = "chg_md_set_transport";
  if (d->started) { eng->err = std::string(fn) + ": the run has already started"; return CHG_EINVAL; }
  HIP_TRY(eng, hipSetDevice(eng->device));
  MdTransport* t = nullptr;
  TRY(create_transport(eng, fn, d->obs, params, &t));
  free_transport(d->obs->tr);
  d->obs->tr = t;
  return CHG_OK;
}

int chg_md_download_transport(chg_engine* eng, chg_md* d, const chg_md_transport_host* o) {
  if (!eng || !d || !o) return CHG_EINVAL;
  if (!d->obs || !d->obs->tr) { eng->err = "chg_md_download_transport: the handle has no transport accumulators (chg_md_set_transport)"; return CHG_EINVAL; }
  HIP_TRY(eng, hipSetDevice(eng->device));
  return download_transport(eng, d->obs, o);
}

int chg_md_set_magmoms(chg_engine* eng, chg_md* d, int32_t log_frames) {
  if (!eng || !d) return CHG_EINVAL;
  const char* fn = "chg_md_set_magmoms";
  if (d->started) { eng->err = std::string(fn) + ": the run has already started"; return CHG_EINVAL; }
  HIP_TRY(eng, hipSetDevice(eng->device));
  return enable_magmoms(eng, fn, d, log_frames != 0);
}

int chg_md_download_magmoms(chg_engine* eng, chg_md* d, float* magmom, float* frame_magmom, int32_t frame_capacity) {
  if (!eng || !d) return CHG_EINVAL;
  if (!d->mag) { eng->err = "chg_md_download_magmoms: the handle does not evaluate moments (chg_md_set_magmoms)"; return CHG_EINVAL; }
  HIP_TRY(eng, hipSetDevice(eng->device));
  const size_t N = d->N;
  TRY(d2h(eng, magmom, d->mag_last, N));
  const int take = d->mag_frames ? std::min(d->ring_count, std::max(frame_capacity, 0)) : 0;
  for (int k = 0; k < take; ++k) {   // oldest first; the ring is left as it is (chg_md_download drains it)
    TRY(d2h(eng, frame_magmom ? frame_magmom + k * N : nullptr, d->ring[(d->ring_head + k) % d->K].mag, N));
  }
  HIP_TRY(eng, hipStreamSynchronize(eng->stream));
  return CHG_OK;
}

int chg_md_set_charge_states(chg_engine* eng, chg_md* d, const chg_md_charge_params* params, const double* bounds) {
  if (!eng || !d || !params || !bounds) return CHG_EINVAL;
  const char* fn = "chg_md_set_charge_states";
  if (d->started) { eng->err = std::string(fn) + ": the run has already started"; return CHG_EINVAL; }
  HIP_TRY(eng, hipSetDevice(eng->device));
  MdCharge* c = nullptr;
  TRY(create_charge(eng, fn, d->obs, params, bounds, true, &c));
  if (!d->mag) {   // the observers read moments: task M and the gather, no frame slots
    const int s = enable_magmoms(eng, fn, d, false);
    if (s != CHG_OK) { free_charge(c); return s; }
  }
  free_charge(d->obs->cs);
  d->obs->cs = c;
  return CHG_OK;
}

int chg_md_download_charge_states(chg_engine* eng, chg_md* d, const chg_md_charge_host* o) {
  if (!eng || !d || !o) return CHG_EINVAL;
  if (!d->obs || !d->obs->cs) {
    eng->err = "chg_md_download_charge_states: the handle has no charge-state observers (chg_md_set_charge_states)";
    return CHG_EINVAL;
  }
  HIP_TRY(eng, hipSetDevice(eng->device));
  return download_charge(eng, d->obs, o);
}

int chg_md_download_observables(chg_engine* eng, chg_md* d, const chg_md_observables_host* o) {
  if (!eng || !d || !o) return CHG_EINVAL;
  if (!d->obs) { eng->err = "chg_md_download_observables: the handle has no observers (chg_md_set_observers)"; return CHG_EINVAL; }
  HIP_TRY(eng, hipSetDevice(eng->device));
  return download_observables(eng, d->obs, o);
}

int chg_md_run(chg_engine* eng, chg_md* d, int32_t n_steps) {
  if (!eng || !d || n_steps < 0) return CHG_EINVAL;
  // the frames this call writes must fit the ring: refuse before anything runs
  int due = (!d->started && frame_due(d, 0)) ? 1 : 0;
  for (int k = 1; k <= n_steps; ++k) due += frame_due(d, d->step + k) ? 1 : 0;
  if (due > d->K - d->ring_count) {
    eng->err = "chg_md_run: " + std::to_string(due) + " frames do not fit the ring (" + std::to_string(d->K - d->ring_count) +
               " slots free): drain it with chg_md_download or run fewer steps";
    return CHG_EINVAL;
  }
  HIP_TRY(eng, hipSetDevice(eng->device));
  const bool npt = is_npt(d->spec.p.ensemble);
  if (!d->started) {   // evaluate the initial configuration: cached forces, Ekin / T, frame of step 0, and the first step's start
    MdStepArgs a = handle_args(d, MD_ABSORB | (n_steps > 0 ? MD_START : 0));
    TRY(evaluate_step_observe(eng, d, a, 0));
    d->started = true;
  } else if (n_steps > 0) {   // a later call: start the step from the cached forces (ASE: get_forces() is cached)
    MdStepArgs a = handle_args(d, MD_START);
    launch_step(eng, a, d->B);
    if (hipGetLastError() != hipSuccess) { eng->err = "chg_md_run: step kernel launch failed"; return CHG_EHIP; }
    TRY(copy_back(eng, "chg_md_run", d, d->B, nullptr, nullptr));
  }
  for (int k = 0; k < n_steps; ++k) {
    if (npt) {   // the barostat's scaled configuration: forces, first half kick, fixcm, drift
      TRY(evaluate_and_step(eng, d, handle_args(d, MD_ABSORB), false));
    }
    const int next = d->step + 1;
    MdStepArgs a = handle_args(d, MD_ABSORB | MD_KICK2 | (k + 1 < n_steps ? MD_START : 0));
    TRY(evaluate_step_observe(eng, d, a, next));
    d->step = next;
  }
  if (eng->profiling) return collect_profile(eng);
  return CHG_OK;
}

int chg_md_download(chg_engine* eng, chg_md* d, const chg_md_out_host* o) {
  if (!eng || !d || !o) return CHG_EINVAL;
  HIP_TRY(eng, hipSetDevice(eng->device));
  const size_t B = d->B, N = d->N;
  TRY(d2h(eng, o->positions, d->r, 3 * N));
  TRY(d2h(eng, o->momenta, d->pm, 3 * N));
  std::vector<double> sd;
  std::vector<int> si;
  if (o->cell) { sd.resize((size_t)MD_SD * B); TRY(d2h(eng, sd.data(), d->sd, sd.size())); }
  if (o->n_steps || o->status) { si.resize((size_t)MD_SI * B); TRY(d2h(eng, si.data(), d->si, si.size())); }
  // frames, oldest first
  const int take = std::min(d->ring_count, std::max(o->frame_capacity, 0));
  for (int k = 0; k < take; ++k) {
    const size_t slot = (size_t)((d->ring_head + k) % std::max(d->K, 1));
    const MdFrame& fr = d->ring[slot];
    if (o->frame_step) o->frame_step[k] = d->ring_step[slot];
    TRY(d2h(eng, o->frame_scalars ? o->frame_scalars + k * MD_FRAME_SCAL * B : nullptr, fr.scal, MD_FRAME_SCAL * B));
    TRY(d2h(eng, o->frame_positions ? o->frame_positions + k * 3 * N : nullptr, fr.pos, 3 * N));
    TRY(d2h(eng, o->frame_momenta ? o->frame_momenta + k * 3 * N : nullptr, fr.mom, 3 * N));
    TRY(d2h(eng, o->frame_cell ? o->frame_cell + k * 9 * B : nullptr, fr.cell, 9 * B));
    TRY(d2h(eng, o->frame_force ? o->frame_force + k * 3 * N : nullptr, fr.force, 3 * N));
    TRY(d2h(eng, o->frame_stress ? o->frame_stress + k * 9 * B : nullptr, fr.stress, 9 * B));
    if (fr.cfea) TRY(d2h(eng, o->frame_crystal_fea ? o->frame_crystal_fea + k * (size_t)FEA * B : nullptr, fr.cfea, FEA * B));
  }
  HIP_TRY(eng, hipStreamSynchronize(eng->stream));
  d->ring_head = d->K > 0 ? (d->ring_head + take) % d->K : 0;
  d->ring_count -= take;
  if (o->n_frames) *o->n_frames = take;
  for (size_t i = 0; i < B; ++i) {
    if (o->cell) std::memcpy(o->cell + 9 * i, sd.data() + MD_SD * i, sizeof(double) * 9);
    if (o->n_steps) o->n_steps[i] = si[MD_SI * i];
    if (o->status) o->status[i] = si[MD_SI * i + 1];
  }
  return CHG_OK;
}

int chg_md_download_nhc(chg_engine* eng, chg_md* d, double* nhc_state, double* frame_conserved, int32_t frame_capacity) {
  if (!eng || !d) return CHG_EINVAL;
  if (!is_nhc(d->spec.p.ensemble)) { eng->err = "chg_md_download_nhc: the handle was not created by chg_md_create_nhc"; return CHG_EINVAL; }
  HIP_TRY(eng, hipSetDevice(eng->device));
  const size_t B = d->B;
  TRY(d2h(eng, nhc_state, d->nhc, MD_NHC * B));
  const int take = std::min(d->ring_count, std::max(frame_capacity, 0));
  for (int k = 0; k < take; ++k) {   // oldest first; the ring is left as it is (chg_md_download drains it)
    TRY(d2h(eng, frame_conserved ? frame_conserved + k * B : nullptr, d->ring[(d->ring_head + k) % d->K].cons, B));
  }
  HIP_TRY(eng, hipStreamSynchronize(eng->stream));
  return CHG_OK;
}

int chg_md_download_vg(chg_engine* eng, chg_md* d, double* vg) {
  if (!eng || !d || !vg) return CHG_EINVAL;
  if (!is_flex(d->spec.p.ensemble)) { eng->err = "chg_md_download_vg: the handle was not created by chg_md_create_nhc_flex"; return CHG_EINVAL; }
  HIP_TRY(eng, hipSetDevice(eng->device));
  TRY(d2h(eng, vg, d->vg, MD_VG * (size_t)d->B));
  HIP_TRY(eng, hipStreamSynchronize(eng->stream));
  return CHG_OK;
}

int chg_md_free(chg_engine* eng, chg_md* d) {
  if (!d) return CHG_OK;
  release(eng, d);
  free_observers(d->obs);
  if (d->mag_mem) hipFree(d->mag_mem);
  delete d;
  return CHG_OK;
}

}  // extern "C"

namespace {

// what the chg_test_md_step* entry points hand over: host arrays, null where an entry point has none
struct TestStepIo {
  int32_t n_struct;
  const int32_t* atom_off;
  int32_t flags;
  double *r, *momenta, *forces;
  const double* masses;
  double* sd;
  int32_t* si;
  const float *energy, *force, *stress;
  double *frac_next, *lat_next, *nhc = nullptr, *vg = nullptr;
  const uint8_t* fixed = nullptr;
};

// one step launch on uploaded copies of t's arrays; spec as for create
int test_step(chg_engine* eng, const char* fn, const MdSpec& spec, const TestStepIo& t) {
  if (!eng || t.n_struct <= 0 || !t.atom_off || !t.r || !t.momenta || !t.forces || !t.masses || !t.sd || !t.si || !t.frac_next || !t.lat_next)
    return CHG_EINVAL;
  if ((t.flags & MD_ABSORB) && (!t.energy || !t.force)) return CHG_EINVAL;
  if (t.flags & ~(MD_ABSORB | MD_KICK2 | MD_START)) return CHG_EINVAL;
  if (const char* bad = bad_params(spec)) { eng->err = std::string(fn) + ": " + bad; return CHG_EINVAL; }
  const int ensemble = spec.p.ensemble;
  if (nhc_npt(ensemble) && (t.flags & MD_ABSORB) && !t.stress) return CHG_EINVAL;
  const size_t B = t.n_struct, N = t.atom_off[t.n_struct];
  if (t.atom_off[0] != 0) return CHG_EINVAL;
  for (size_t o = 0; o < B; ++o)
    if (t.atom_off[o + 1] - t.atom_off[o] < (t.nhc ? 2 : 1)) return CHG_EINVAL;
  std::vector<int> nfree(B);
  if (t.fixed) TRY(check_fixed(eng, fn, (int)B, t.atom_off, t.fixed, moving_cell(ensemble), ensemble != MD_NVE, nfree.data()));
  enum { R, P, F, M, SD, SI, AOFF, ENERGY, FORCE, STRESS, FRAC_NEXT, LAT_NEXT, RETRY, SEEDS, NHC, FIXED, NFREE, VG, N_BUFS };
  TestBuf bufs[N_BUFS];
  bufs[R] = {t.r, t.r, sizeof(double) * 3 * N};
  bufs[P] = {t.momenta, t.momenta, sizeof(double) * 3 * N};
  bufs[F] = {t.forces, t.forces, sizeof(double) * 3 * N};
  bufs[M] = {t.masses, nullptr, sizeof(double) * N};
  bufs[SD] = {t.sd, t.sd, sizeof(double) * MD_SD * B};
  bufs[SI] = {t.si, t.si, sizeof(int) * MD_SI * B};
  bufs[AOFF] = {t.atom_off, nullptr, sizeof(int) * (B + 1)};
  bufs[ENERGY] = {t.energy, nullptr, sizeof(float) * B};
  bufs[FORCE] = {t.force, nullptr, sizeof(float) * 3 * N};
  bufs[STRESS] = {t.stress, nullptr, sizeof(float) * 9 * B};
  bufs[FRAC_NEXT] = {t.frac_next, t.frac_next, sizeof(double) * 3 * N};
  bufs[LAT_NEXT] = {t.lat_next, t.lat_next, sizeof(double) * 9 * B};
  bufs[RETRY] = {nullptr, nullptr, sizeof(int) * B};
  bufs[SEEDS] = {spec.seeds, nullptr, sizeof(uint64_t) * B};
  bufs[NHC] = {t.nhc, t.nhc, sizeof(double) * MD_NHC * B};
  bufs[FIXED] = {t.fixed, nullptr, 3 * N};
  bufs[NFREE] = {t.fixed ? nfree.data() : nullptr, nullptr, sizeof(int) * B};
  bufs[VG] = {t.vg, t.vg, sizeof(double) * MD_VG * B};
  return run_test_step(eng, fn, bufs, [&] {
    MdStepArgs a = base_args(spec);
    a.r = (double*)bufs[R].d; a.p = (double*)bufs[P].d; a.f = (double*)bufs[F].d; a.m = (const double*)bufs[M].d;
    a.sd = (double*)bufs[SD].d; a.si = (int*)bufs[SI].d; a.aoff = (const int*)bufs[AOFF].d;
    a.energy = t.energy ? (const float*)bufs[ENERGY].d : nullptr; a.force = t.force ? (const float*)bufs[FORCE].d : nullptr;
    a.stress = t.stress ? (const float*)bufs[STRESS].d : nullptr;
    a.frac_next = (double*)bufs[FRAC_NEXT].d; a.lat_next = (double*)bufs[LAT_NEXT].d; a.retry = (int*)bufs[RETRY].d;
    a.seeds = (const unsigned long long*)bufs[SEEDS].d; a.nhc = (double*)bufs[NHC].d; a.vg = (double*)bufs[VG].d;
    a.flags = t.flags;
    a.final_try = 1;
    if (t.fixed) { a.fixed = (const unsigned char*)bufs[FIXED].d; a.nfree = (const int*)bufs[NFREE].d; }
    launch_step(eng, a, (int)B);
  });
}

}  // namespace

extern "C" {

int chg_test_md_step(chg_engine* eng, const chg_md_params* params, int32_t n_struct, const int32_t* atom_off, int32_t flags, double* r,
                     double* momenta, double* forces, const double* masses, double* sd, int32_t* si, const float* energy, const float* force,
                     const float* stress, double* frac_next, double* lat_next) {
  if (!params) return CHG_EINVAL;
  return test_step(eng, "chg_test_md_step", MdSpec{*params},
                   {n_struct, atom_off, flags, r, momenta, forces, masses, sd, si, energy, force, stress, frac_next, lat_next});
}

int chg_test_md_step_langevin(chg_engine* eng, const chg_md_params* params, int32_t n_struct, const int32_t* atom_off, int32_t flags, double* r,
                              double* momenta, double* forces, const double* masses, double* sd, int32_t* si, const float* energy,
                              const float* force, const float* stress, double* frac_next, double* lat_next, double friction,
                              const uint64_t* seeds) {
  if (!params || !seeds) return CHG_EINVAL;
  return test_step(eng, "chg_test_md_step_langevin", MdSpec{*params, MdEntry::Langevin, friction, seeds},
                   {n_struct, atom_off, flags, r, momenta, forces, masses, sd, si, energy, force, stress, frac_next, lat_next});
}

int chg_test_md_step_nhc(chg_engine* eng, const chg_md_params* params, int32_t n_struct, const int32_t* atom_off, int32_t flags, double* r,
                         double* momenta, double* forces, const double* masses, double* sd, int32_t* si, const float* energy,
                         const float* force, const float* stress, double* frac_next, double* lat_next, int32_t chain_length, double* nhc) {
  if (!params || !nhc) return CHG_EINVAL;
  return test_step(eng, "chg_test_md_step_nhc", MdSpec{*params, MdEntry::Nhc, 0.0, nullptr, chain_length},
                   {n_struct, atom_off, flags, r, momenta, forces, masses, sd, si, energy, force, stress, frac_next, lat_next, nhc});
}

int chg_test_md_step_nhc_flex(chg_engine* eng, const chg_md_params* params, int32_t n_struct, const int32_t* atom_off, int32_t flags, double* r,
                              double* momenta, double* forces, const double* masses, double* sd, int32_t* si, const float* energy,
                              const float* force, const float* stress, double* frac_next, double* lat_next, int32_t chain_length, double* nhc,
                              double* vg, const uint8_t* fixed) {
  if (!params || !nhc || !vg) return CHG_EINVAL;
  return test_step(eng, "chg_test_md_step_nhc_flex", MdSpec{*params, MdEntry::NhcFlex, 0.0, nullptr, chain_length},
                   {n_struct, atom_off, flags, r, momenta, forces, masses, sd, si, energy, force, stress, frac_next, lat_next, nhc, vg, fixed});
}

// the entry point follows from the ensemble: Langevin with friction and seeds, the isotropic chains with chain_length and nhc
int chg_test_md_step_fixed(chg_engine* eng, const chg_md_params* params, int32_t n_struct, const int32_t* atom_off, int32_t flags, double* r,
                           double* momenta, double* forces, const double* masses, double* sd, int32_t* si, const float* energy,
                           const float* force, const float* stress, double* frac_next, double* lat_next, double friction,
                           const uint64_t* seeds, int32_t chain_length, double* nhc, const uint8_t* fixed) {
  if (!params) return CHG_EINVAL;
  MdSpec spec{*params};
  TestStepIo t{n_struct, atom_off, flags, r, momenta, forces, masses, sd, si, energy, force, stress, frac_next, lat_next, nullptr, nullptr, fixed};
  if (params->ensemble == MD_NVT_LANGEVIN) {
    if (!seeds) return CHG_EINVAL;
    spec = MdSpec{*params, MdEntry::Langevin, friction, seeds};
  } else if (is_nhc(params->ensemble)) {
    if (!nhc) return CHG_EINVAL;
    spec = MdSpec{*params, MdEntry::Nhc, 0.0, nullptr, chain_length};
    t.nhc = nhc;
  }
  return test_step(eng, "chg_test_md_step_fixed", spec, t);
}

}  // extern "C"

namespace {

// what chg_test_md_charge_states adds to the snapshots
struct TestCharge {
  const chg_md_charge_params* params;
  const double* bounds;
  const float* magmoms;   // [T, N]
  const chg_md_charge_host* out;
};

// chg_test_md_observe / chg_test_md_transport / chg_test_md_charge_states: caller-given snapshots through observe(), then the
// downloads that were asked for
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
  MdObservers* x = nullptr;
  TRY(create_observers(eng, fn, params, n_struct, atom_off, species, false, &x));
  if (transport) {
    const int s = create_transport(eng, fn, x, transport, &x->tr);
    if (s != CHG_OK) { free_observers(x); return s; }
  }
  if (charge) {
    const int s = create_charge(eng, fn, x, charge->params, charge->bounds, false, &x->cs);
    if (s != CHG_OK) { free_observers(x); return s; }
  }
  TestBuf bufs[] = {{positions, nullptr, sizeof(double) * T * 3 * N}, {momenta, nullptr, sizeof(double) * T * 3 * N},
                    {cell, nullptr, sizeof(double) * T * 9 * B}, {status, nullptr, sizeof(int) * T * B}, {masses, nullptr, sizeof(double) * N},
                    {atom_off, nullptr, sizeof(int) * (B + 1)},
                    {charge ? charge->magmoms : nullptr, nullptr, sizeof(float) * (charge ? T * N : 1)}};
  int rc = CHG_OK;
  int s = run_test_step(eng, fn, bufs, [&] {
    for (size_t t = 0; t < T && rc == CHG_OK; ++t)
      rc = observe(eng, fn, x, (const double*)bufs[0].d + t * 3 * N, (const double*)bufs[1].d + t * 3 * N, (const double*)bufs[2].d + t * 9 * B,
                   (const double*)bufs[4].d, (const int*)bufs[3].d + t * B, 1, (const int*)bufs[5].d,
                   charge ? (const float*)bufs[6].d + t * N : nullptr);
  });
  if (s == CHG_OK) s = rc;
  if (s == CHG_OK && out) s = download_observables(eng, x, out);
  if (s == CHG_OK && tout) s = download_transport(eng, x, tout);
  if (s == CHG_OK && charge) s = download_charge(eng, x, charge->out);
  free_observers(x);
  return s;
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
