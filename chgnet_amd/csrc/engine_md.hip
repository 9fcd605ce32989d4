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
// The observers' host side is engine_md_observe.h; this unit creates them, asks sample_due and hands observe() the frame of a sample.
#include "engine_stepper.h"

#include "kernels_md.h"
#include "engine_md_observe.h"

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
  std::unique_ptr<MdObservers> obs;      // chg_md_set_observers
  // chg_md_set_magmoms (or implied by chg_md_set_charge_states): task M, k_md_mag_gather after every evaluation that completes a step
  bool mag = false, mag_frames = false;
  DeviceBlock mag_mem;
  float* mag_last = nullptr;   // [N] moments of the last completed step, then the ring frames' slots
};

namespace {

constexpr int FEA = chg::D;

bool is_npt(int e) { return e == MD_NPT_BERENDSEN_INHOMOGENEOUS || e == MD_NPT_BERENDSEN; }   // the two-evaluation Berendsen loop
bool is_flex(int e) { return e == MD_NPT_NHC_FLEX || e == MD_NPT_NHC_AXES; }   // chg_md_create_nhc_flex only
bool is_nhc(int e) { return e == MD_NVT_NHC || e == MD_NPT_NHC || is_flex(e); }

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

// one evaluation that completes step `step`: its frame goes to the ring when one is due, to the observers' private slot (not part
// of the ring, not counted in ring_count) when only a sample is, and the observers read it once the step launch -- a wide-range retry included -- has returned
int evaluate_step_observe(chg_engine* eng, chg_md* d, MdStepArgs& a, int step) {
  const bool sample = sample_due(d->obs.get(), step);
  if (frame_due(d, step)) set_frame(d, a, step);
  else if (sample) a.fr = d->obs->fr;
  if (sample && d->obs->cs && !a.fr.mag) a.fr.mag = d->obs->cs->fr_mag;   // a ring frame without moment slots: the observers' own
  TRY(evaluate_and_step(eng, d, a, true));
  if (sample) TRY(observe(eng, "chg_md_run", d->obs.get(), a.fr.pos, a.fr.mom, a.fr.cell, d->m, d->si + 1, MD_SI, d->d_aoff, a.fr.mag));
  return CHG_OK;
}

// task M and the moment slots: [N] of the last completed step, then [N] per ring frame with log_frames
int enable_magmoms(chg_engine* eng, const char* fn, chg_md* d, bool log_frames) {
  const size_t N = d->N, slots = 1 + (log_frames ? (size_t)d->K : 0);
  DeviceBlock block;
  float* mem = nullptr;
  TRY(alloc_block(eng, fn, "moment slots", [&](Carver& c) { mem = c.take<float>(N * slots); }, &block.p));
  StateUpload up{eng, fn};
  up.zero(mem, sizeof(float) * N * slots);
  TRY(up.finish());
  std::swap(d->mag_mem.p, block.p);   // slots of an earlier call go with the block
  d->mag_last = mem;
  for (int k = 0; k < d->K; ++k) d->ring[k].mag = log_frames ? mem + N * (size_t)(k + 1) : nullptr;
  d->mag = true;
  d->mag_frames = log_frames;
  d->task |= CHG_TASK_M;
  return CHG_OK;
}

// the observer and moment setters: before the first chg_md_run only, on the engine's device (chg_md_set_fixed checks its mask in between)
int before_run(chg_engine* eng, const char* fn, const chg_md* d) {
  if (d->started) { eng->err = std::string(fn) + ": the run has already started"; return CHG_EINVAL; }
  HIP_TRY(eng, hipSetDevice(eng->device));
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
  TRY(before_run(eng, fn, d));
  return create_observers(eng, fn, params, d->B, d->h_aoff, species, true, d->obs);   // replaces earlier ones only on success
}

int chg_md_set_transport(chg_engine* eng, chg_md* d, const chg_md_transport_params* params) {
  if (!eng || !d || !params) return CHG_EINVAL;
  const char* fn = "chg_md_set_transport";
  TRY(before_run(eng, fn, d));
  std::unique_ptr<MdTransport> t;
  TRY(create_transport(eng, fn, d->obs.get(), params, t));   // refuses a handle without observers
  d->obs->tr = std::move(t);
  return CHG_OK;
}

int chg_md_download_transport(chg_engine* eng, chg_md* d, const chg_md_transport_host* o) {
  if (!eng || !d || !o) return CHG_EINVAL;
  if (!d->obs || !d->obs->tr) { eng->err = "chg_md_download_transport: the handle has no transport accumulators (chg_md_set_transport)"; return CHG_EINVAL; }
  HIP_TRY(eng, hipSetDevice(eng->device));
  return download_transport(eng, d->obs.get(), o);
}

int chg_md_set_magmoms(chg_engine* eng, chg_md* d, int32_t log_frames) {
  if (!eng || !d) return CHG_EINVAL;
  const char* fn = "chg_md_set_magmoms";
  TRY(before_run(eng, fn, d));
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
  TRY(before_run(eng, fn, d));
  std::unique_ptr<MdCharge> c;
  TRY(create_charge(eng, fn, d->obs.get(), params, bounds, true, c));   // refuses a handle without observers
  if (!d->mag) TRY(enable_magmoms(eng, fn, d, false));   // the observers read moments: task M and the gather, no frame slots
  d->obs->cs = std::move(c);
  return CHG_OK;
}

int chg_md_download_charge_states(chg_engine* eng, chg_md* d, const chg_md_charge_host* o) {
  if (!eng || !d || !o) return CHG_EINVAL;
  if (!d->obs || !d->obs->cs) {
    eng->err = "chg_md_download_charge_states: the handle has no charge-state observers (chg_md_set_charge_states)";
    return CHG_EINVAL;
  }
  HIP_TRY(eng, hipSetDevice(eng->device));
  return download_charge(eng, d->obs.get(), o);
}

int chg_md_download_observables(chg_engine* eng, chg_md* d, const chg_md_observables_host* o) {
  if (!eng || !d || !o) return CHG_EINVAL;
  if (!d->obs) { eng->err = "chg_md_download_observables: the handle has no observers (chg_md_set_observers)"; return CHG_EINVAL; }
  HIP_TRY(eng, hipSetDevice(eng->device));
  return download_observables(eng, d->obs.get(), o);
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
  delete d;   // the observers and the moment slots go with it
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
