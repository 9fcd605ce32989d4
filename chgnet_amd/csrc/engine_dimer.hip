// engine_dimer.hip -- batched dimer saddle search (chg_dimer_*): every image of every search is a structure of the batch, one step
// kernel per evaluation (kernels_dimer.h), state in HBM.  DESIGN.md "Dimer saddle search".
//
// The state, the staging and the test launch are the shared driver's (engine_stepper.h).  The evaluate-and-step loop is this file's
// own, because its unit is the search and the size of a search in the batch changes from one evaluation to the next: the centre and
// the displaced image after a translation (phase PROBE), the trial image alone during rotations (phase TRIAL; the centre is never
// evaluated again while it stands still).  The kernel decides; the host learns the next phase with the next coordinates and packs the
// staging accordingly.  A search with a non-finite image is held back and stepped again as a whole; a search that stops leaves the
// next build.
#include "engine_stepper.h"

#include "kernels_dimer.h"

struct chg_dimer : chgh::Stepper {
  chg_dimer_params p{};
  int S = 0, NA = 0;                // searches and their atoms (Stepper::B, N count the staging: two structures per search)
  // device: state (original numbering) and the per-launch tables
  double *r, *nvec, *theta, *v, *f0, *f1, *sd;
  float *e_img, *f_img;             // [S, 2] and [2 NA, 3]: the engine's results as last evaluated, two images per search
  int *si, *d_aoff, *d_tab, *status_next, *phase_next;
  // host: the searches as given (the staging holds only what the next build evaluates)
  std::vector<int> aoff, z, phase, evaluated, active;
  std::vector<double> lat, linv;    // [S, 9] each
  std::vector<double> r0, mode0;    // [NA, 3] the centres and the modes as given, for chg_dimer_set_fixed
  // pinned (Stepper::h_extra): the atom offsets of the staging are double-buffered -- the next layout is written while the arrays of
  // this one may still be referenced by the build in flight
  int *h_aoff2, *h_tab, *h_status, *h_phase;
  int n_staged = 0;                 // structures staged for the next build
  bool first = true;
};

namespace {

void carve_dimer(chg_dimer* s, Carver& c) {
  const size_t S = s->S, NA = s->NA;
  s->r = c.take<double>(3 * NA);
  s->nvec = c.take<double>(3 * NA);
  s->theta = c.take<double>(3 * NA);
  s->v = c.take<double>(3 * NA);
  s->f0 = c.take<double>(3 * NA);
  s->f1 = c.take<double>(3 * NA);
  s->sd = c.take<double>(DIMER_SD * S);
  s->frac_next = c.take<double>(3 * 2 * NA);
  s->e_img = c.take<float>(2 * S);
  s->f_img = c.take<float>(3 * 2 * NA);
  s->si = c.take<int>(DIMER_SI * S);
  s->d_aoff = c.take<int>(S + 1);
  s->d_tab = c.take<int>(4 * S);
  s->d_sel = c.take<int>(S);
  s->status_next = c.take<int>(S);
  s->phase_next = c.take<int>(S);
  s->retry = c.take<int>(S);
  s->d_fixed = c.take<unsigned char>(3 * NA);
}

int check_params(chg_engine* eng, const char* fn, const chg_dimer_params* p) {
  const char* bad = nullptr;
  if (!(p->fmax >= 0.0)) bad = "fmax must be >= 0";
  else if (p->max_steps < 0) bad = "max_steps must be >= 0";
  else if (!(p->r_atom > 0.0) || !(p->r_bond > 0.0)) bad = "graph cutoffs must be > 0";
  else if (!(p->dt > 0.0) || !(p->maxstep > 0.0) || !(p->dtmax > 0.0)) bad = "dt, maxstep and dtmax must be > 0";
  else if (!(p->finc > 0.0) || !(p->fdec > 0.0) || !(p->astart >= 0.0) || !(p->fa > 0.0)) bad = "finc, fdec, fa must be > 0 and astart >= 0";
  else if (!(p->delta > 0.0) || !(p->delta <= 0.5)) bad = "delta must lie in (0, 0.5] A";
  else if (p->max_rotations < 0 || p->max_rotations > DIMER_MAX_ROTATIONS) bad = "max_rotations must lie in 0..32";
  else if (!(p->angle_tol >= 1e-4) || !(p->angle_tol < M_PI / 4)) bad = "angle_tol must lie in [1e-4, pi/4) rad";
  if (bad) { eng->err = std::string(fn) + ": " + bad; return CHG_EINVAL; }
  return CHG_OK;
}

DimerStepArgs step_args(const chg_dimer_params& p) {
  DimerStepArgs a{};
  a.fmax2 = p.fmax * p.fmax;
  a.maxstep = p.maxstep; a.dtmax = p.dtmax; a.finc = p.finc; a.fdec = p.fdec; a.astart = p.astart; a.fa = p.fa;
  a.delta = p.delta; a.angle_tol = p.angle_tol;
  a.max_steps = p.max_steps; a.nmin = p.nmin; a.max_rotations = p.max_rotations;
  return a;
}

// a.fixed null: the unconstrained kernel
void launch_step(chg_engine* eng, const DimerStepArgs& a, int grid) {
  LaunchScope ls(eng, "dimer_step");
  if (a.fixed) hipLaunchKernelGGL(k_dimer_step<true>, dim3((unsigned)grid), dim3(256), 0, eng->stream, a);
  else hipLaunchKernelGGL(k_dimer_step<false>, dim3((unsigned)grid), dim3(256), 0, eng->stream, a);
}

// The axes of all searches from the modes as given: held components zeroed, every search normalised over its 3 n components.
// CHG_EINVAL with a message when a search is left without a free component.
int axes(chg_engine* eng, const char* fn, const chg_dimer* s, const double* mode, const uint8_t* fixed, std::vector<double>& nv) {
  nv.assign(mode, mode + 3 * (size_t)s->NA);
  for (int k = 0; k < s->S; ++k) {
    double nn = 0.0;
    for (size_t x = 3 * (size_t)s->aoff[k]; x < 3 * (size_t)s->aoff[k + 1]; ++x) {
      if (fixed && fixed[x]) nv[x] = 0.0;
      nn += nv[x] * nv[x];
    }
    if (!(nn > 0.0) || !std::isfinite(nn)) {
      eng->err = std::string(fn) + ": the mode of search " + std::to_string(k) +
                 (std::isfinite(nn) ? (fixed ? " has no free component" : " is zero") : " is not finite");
      return CHG_EINVAL;
    }
    const double sc = 1.0 / std::sqrt(nn);
    for (size_t x = 3 * (size_t)s->aoff[k]; x < 3 * (size_t)s->aoff[k + 1]; ++x) nv[x] *= sc;
  }
  return CHG_OK;
}

// fractional coordinates x L^-1 of n cartesian rows
void to_frac(const double* x, const double* linv, int n, double* frac) {
  for (int i = 0; i < n; ++i)
    for (int c = 0; c < 3; ++c) frac[3 * i + c] = x[3 * i] * linv[c] + x[3 * i + 1] * linv[3 + c] + x[3 * i + 2] * linv[6 + c];
}

// the staging of the first evaluation: R and R + delta N of every search; frac [2 NA, 3]
void first_images(const chg_dimer* s, const double* nv, double* frac) {
  std::vector<double> x;
  for (int k = 0; k < s->S; ++k) {
    const int a0 = s->aoff[k], n = s->aoff[k + 1] - a0;
    const double* linv = s->linv.data() + 9 * (size_t)k;
    x.assign(s->r0.begin() + 3 * (size_t)a0, s->r0.begin() + 3 * (size_t)(a0 + n));
    to_frac(x.data(), linv, n, frac + 3 * (size_t)(2 * a0));
    for (int i = 0; i < 3 * n; ++i) x[i] += s->p.delta * nv[3 * (size_t)a0 + i];
    to_frac(x.data(), linv, n, frac + 3 * (size_t)(2 * a0 + n));
  }
}

// species, cells and atom offsets of the next staging: per search in `active` two structures (PROBE) or one; returns the structures
int stage_layout(chg_dimer* s, int* aoff_out) {
  int st = 0, na = 0;
  for (int k : s->active) {
    const int a0 = s->aoff[k], n = s->aoff[k + 1] - a0;
    for (int i = 0, m = s->phase[k] == DIMER_PROBE ? 2 : 1; i < m; ++i) {
      aoff_out[st] = na;
      std::memcpy(s->h_z + na, s->z.data() + a0, sizeof(int) * n);
      std::memcpy(s->h_lat + 9 * (size_t)st, s->lat.data() + 9 * (size_t)k, sizeof(double) * 9);
      na += n;
      ++st;
    }
  }
  aoff_out[st] = na;
  return st;
}

// One evaluation of the staged structures and the dimer steps that follow it
int evaluate_and_step_searches(chg_engine* eng, const char* fn, chg_dimer* s, DimerStepArgs& a) {
  hipStream_t st = eng->stream;
  const int nst = s->n_staged, nact = (int)s->active.size();
  const chg_structs_host hs{nst, s->h_aoff[nst], s->h_z, s->h_frac, s->h_lat, s->h_aoff};
  chg_batch* b = nullptr;
  int32_t counts[6];
  TRY(chg_batch_build_predict(eng, &hs, s->r_atom, s->r_bond, s->numerical_tol, s->task, &b, counts));
  auto fail = [&](const char* what, int code) {
    if (what) eng->err = std::string(fn) + ": " + what;
    chg_batch_free(eng, b);
    return code;
  };
  // where every active search sits in this batch; each owns 2 n rows of frac_next, of which it writes n or 2 n
  int bs = 0, noff = 0;
  for (int j = 0; j < nact; ++j) {
    const int k = s->active[j], nev = s->phase[k] == DIMER_PROBE ? 2 : 1;
    s->h_tab[4 * j] = k; s->h_tab[4 * j + 1] = bs; s->h_tab[4 * j + 2] = nev; s->h_tab[4 * j + 3] = noff;
    bs += nev;
    noff += 2 * (s->aoff[k + 1] - s->aoff[k]);
  }
  if (hipMemcpyAsync(s->d_tab, s->h_tab, sizeof(int) * 4 * nact, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemsetAsync(s->retry, 0, sizeof(int) * nact, st) != hipSuccess)
    return fail("search table upload failed", CHG_EHIP);
  a.energy = b->energy; a.force = b->force; a.b_atom_off = b->atom_off;
  auto step = [&](const int* sel, int final_try, int grid) -> int {
    a.sel = sel; a.final_try = final_try;
    launch_step(eng, a, grid);
    if (hipGetLastError() != hipSuccess) return fail("step kernel launch failed", CHG_EHIP);
    if (hipMemcpyAsync(s->h_status, s->status_next, sizeof(int) * nact, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(s->h_phase, s->phase_next, sizeof(int) * nact, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(s->h_retry, s->retry, sizeof(int) * nact, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipMemcpyAsync(s->h_frac, s->frac_next, sizeof(double) * 3 * (size_t)noff, hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
      return fail("copy of the next configuration failed", CHG_EHIP);
    return CHG_OK;
  };
  TRY(step(nullptr, b->wide_range ? 1 : 0, nact));
  int n_sel = 0;
  for (int j = 0; j < nact; ++j)
    if (s->h_retry[j]) s->h_sel[n_sel++] = j;
  if (n_sel > 0) {   // as evaluate_and_step: the whole batch again on the wide-range sweep, then the held-back searches only
    b->wide_range = true;
    if (b->graph_exec) { hipGraphExecDestroy(b->graph_exec); b->graph_exec = nullptr; }
    const int rc = chgh_wide::run_predict(eng, b, b->last_task ? b->last_task : s->task);
    if (rc != CHG_OK) return fail(nullptr, rc);
    if (hipMemcpyAsync(s->d_sel, s->h_sel, sizeof(int) * n_sel, hipMemcpyHostToDevice, st) != hipSuccess) return fail("index upload failed", CHG_EHIP);
    TRY(step(s->d_sel, 1, n_sel));
  }
  TRY(chg_batch_free(eng, b));
  s->first = false;
  // compaction: the searches still running keep their order, their rows (n or 2 n of the 2 n they own) only move towards the front
  std::vector<int> still;
  int na = 0, from = 0;
  for (int j = 0; j < nact; ++j) {
    const int k = s->active[j], n = s->aoff[k + 1] - s->aoff[k];
    s->evaluated[k] += s->h_tab[4 * j + 2];
    if (s->h_status[j] == CHG_RELAX_RUNNING) {
      s->phase[k] = s->h_phase[j];
      const int rows = s->phase[k] == DIMER_PROBE ? 2 * n : n;
      if (na != from) std::memmove(s->h_frac + 3 * (size_t)na, s->h_frac + 3 * (size_t)from, sizeof(double) * 3 * rows);
      na += rows;
      still.push_back(k);
    }
    from += 2 * n;
  }
  s->active.swap(still);
  s->n_staged = stage_layout(s, s->h_aoff2);
  std::swap(s->h_aoff, s->h_aoff2);
  return CHG_OK;
}

}  // namespace

extern "C" {

int chg_dimer_create(chg_engine* eng, const chg_structs_host* h, const double* mode, const chg_dimer_params* params, chg_dimer** out) {
  const char* fn = "chg_dimer_create";
  if (!eng || !h || !mode || !params || !out) return CHG_EINVAL;
  *out = nullptr;
  TRY(check_params(eng, fn, params));
  TRY(check_structs(eng, fn, h));
  const int S = h->n_struct, NA = h->n_atoms;
  if (NA > (1 << 28)) { eng->err = std::string(fn) + ": too many atoms"; return CHG_EINVAL; }
  chg_dimer* s = new chg_dimer();
  s->p = *params;
  s->S = S; s->NA = NA;
  s->task = CHG_TASK_E | CHG_TASK_F;
  s->r_atom = params->r_atom; s->r_bond = params->r_bond; s->numerical_tol = params->numerical_tol;
  s->aoff.assign(h->atom_off, h->atom_off + S + 1);
  s->z.assign(h->z, h->z + NA);
  s->lat.assign(h->lattice, h->lattice + 9 * (size_t)S);
  s->linv.resize(9 * (size_t)S);
  s->r0.resize(3 * (size_t)NA);
  s->mode0.assign(mode, mode + 3 * (size_t)NA);
  s->phase.assign(S, DIMER_PROBE);
  s->evaluated.assign(S, 0);
  s->active.resize(S);
  std::vector<double> sd((size_t)DIMER_SD * S, 0.0), geo(18), nv;
  for (int k = 0; k < S; ++k) {
    s->active[k] = k;
    initial_geometry(h, k, s->r0.data() + 3 * (size_t)h->atom_off[k], geo.data());
    std::memcpy(s->linv.data() + 9 * (size_t)k, geo.data() + 9, sizeof(double) * 9);
    double* d = sd.data() + (size_t)DIMER_SD * k;
    for (int i = 0; i < 18; ++i) d[i] = geo[i];
    d[18] = params->dt;
    d[19] = params->astart;
  }
  int rc = axes(eng, fn, s, mode, nullptr, nv);
  if (rc != CHG_OK) { delete s; return rc; }
  // the staging of the first evaluation, two structures per search, is what alloc_state copies into pinned memory
  std::vector<double> frac2(6 * (size_t)NA), lat2(18 * (size_t)S);
  std::vector<int> z2(2 * (size_t)NA), aoff2(2 * (size_t)S + 1);
  first_images(s, nv.data(), frac2.data());
  for (int k = 0; k < S; ++k) {
    const int a0 = s->aoff[k], n = s->aoff[k + 1] - a0;
    for (int i = 0; i < 2; ++i) {
      aoff2[2 * k + i] = 2 * a0 + i * n;
      std::memcpy(z2.data() + 2 * a0 + i * n, h->z + a0, sizeof(int) * n);
      std::memcpy(lat2.data() + 9 * (size_t)(2 * k + i), h->lattice + 9 * (size_t)k, sizeof(double) * 9);
    }
  }
  aoff2[2 * S] = 2 * NA;
  const chg_structs_host h2{2 * S, 2 * NA, z2.data(), frac2.data(), lat2.data(), aoff2.data()};
  if (hipSetDevice(eng->device) != hipSuccess) { delete s; eng->err = std::string(fn) + ": hipSetDevice failed"; return CHG_EHIP; }
  rc = alloc_state(eng, fn, s, &h2, 5, [&](Carver& c) { carve_dimer(s, c); });
  if (rc != CHG_OK) { chg_dimer_free(eng, s); return rc; }
  // h_extra [5 B = 10 S] ints: the second offsets buffer [2 S + 1], the search table [4 S], statuses [S] and phases [S]
  s->h_aoff2 = s->h_extra;
  s->h_tab = s->h_extra + 2 * (size_t)S + 1;
  s->h_status = s->h_tab + 4 * (size_t)S;
  s->h_phase = s->h_status + S;
  s->n_staged = 2 * S;
  StateUpload up{eng, fn};
  up(s->r, s->r0.data(), sizeof(double) * 3 * (size_t)NA);
  up(s->nvec, nv.data(), sizeof(double) * 3 * (size_t)NA);
  up(s->sd, sd.data(), sizeof(double) * sd.size());
  up(s->d_aoff, h->atom_off, sizeof(int) * (S + 1));
  up.zero(s->theta, sizeof(double) * 3 * (size_t)NA);
  up.zero(s->v, sizeof(double) * 3 * (size_t)NA);
  up.zero(s->f0, sizeof(double) * 3 * (size_t)NA);
  up.zero(s->f1, sizeof(double) * 3 * (size_t)NA);
  up.zero(s->frac_next, sizeof(double) * 6 * (size_t)NA);
  up.zero(s->e_img, sizeof(float) * 2 * S);
  up.zero(s->f_img, sizeof(float) * 6 * (size_t)NA);
  up.zero(s->si, sizeof(int) * DIMER_SI * (size_t)S);
  up.zero(s->status_next, sizeof(int) * S);
  up.zero(s->phase_next, sizeof(int) * S);
  up.zero(s->retry, sizeof(int) * S);
  if ((rc = up.finish()) != CHG_OK) { chg_dimer_free(eng, s); return rc; }
  *out = s;
  return CHG_OK;
}

int chg_dimer_set_fixed(chg_engine* eng, chg_dimer* s, const uint8_t* fixed) {
  if (!eng || !s) return CHG_EINVAL;
  const char* fn = "chg_dimer_set_fixed";
  if (!s->first) { eng->err = std::string(fn) + ": the search has already run"; return CHG_EINVAL; }
  std::vector<double> nv;
  TRY(axes(eng, fn, s, s->mode0.data(), fixed, nv));
  HIP_TRY(eng, hipSetDevice(eng->device));
  s->has_fixed = false;
  StateUpload up{eng, fn};
  up(s->nvec, nv.data(), sizeof(double) * nv.size());
  if (fixed) up(s->d_fixed, fixed, 3 * (size_t)s->NA);
  TRY(up.finish());
  first_images(s, nv.data(), s->h_frac);
  s->has_fixed = fixed != nullptr;
  return CHG_OK;
}

int chg_dimer_run(chg_engine* eng, chg_dimer* s, int32_t n_evaluations, int32_t* n_active) {
  if (!eng || !s || n_evaluations < 0) return CHG_EINVAL;
  HIP_TRY(eng, hipSetDevice(eng->device));
  DimerStepArgs a = step_args(s->p);
  a.r = s->r; a.nvec = s->nvec; a.theta = s->theta; a.v = s->v; a.f0 = s->f0; a.f1 = s->f1; a.sd = s->sd; a.si = s->si;
  a.e_img = s->e_img; a.f_img = s->f_img;
  a.aoff = s->d_aoff; a.fixed = s->has_fixed ? s->d_fixed : nullptr;
  a.tab = s->d_tab; a.frac_next = s->frac_next; a.status_next = s->status_next; a.phase_next = s->phase_next; a.retry = s->retry;
  for (int it = 0; it < n_evaluations && !s->active.empty(); ++it) TRY(evaluate_and_step_searches(eng, "chg_dimer_run", s, a));
  if (n_active) *n_active = (int32_t)s->active.size();
  if (eng->profiling) return collect_profile(eng);
  return CHG_OK;
}

int chg_dimer_download(chg_engine* eng, chg_dimer* s, const chg_dimer_out_host* o) {
  if (!eng || !s || !o) return CHG_EINVAL;
  HIP_TRY(eng, hipSetDevice(eng->device));
  const size_t S = s->S, NA = s->NA;
  std::vector<double> r(o->frac ? 3 * NA : 0), sd((size_t)DIMER_SD * S);
  std::vector<int> si((size_t)DIMER_SI * S);
  TRY(d2h(eng, r.data(), s->r, r.size()));
  TRY(d2h(eng, o->mode, s->nvec, 3 * NA));
  TRY(d2h(eng, o->force, s->f0, 3 * NA));
  TRY(d2h(eng, o->image_energy, s->e_img, 2 * S));
  TRY(d2h(eng, o->image_force, s->f_img, 6 * NA));
  TRY(d2h(eng, sd.data(), s->sd, sd.size()));
  TRY(d2h(eng, si.data(), s->si, si.size()));
  HIP_TRY(eng, hipStreamSynchronize(eng->stream));
  for (size_t k = 0; k < S; ++k) {
    if (o->frac) to_frac(r.data() + 3 * (size_t)s->aoff[k], s->linv.data() + 9 * k, s->aoff[k + 1] - s->aoff[k], o->frac + 3 * (size_t)s->aoff[k]);
    if (o->curvature) o->curvature[k] = sd[DIMER_SD * k + 20];
    if (o->fmax) o->fmax[k] = sd[DIMER_SD * k + 23];
    if (o->n_steps) o->n_steps[k] = si[DIMER_SI * k + 1];
    if (o->status) o->status[k] = si[DIMER_SI * k + 2];
    if (o->phase) o->phase[k] = si[DIMER_SI * k + 3];
    if (o->n_rotations) o->n_rotations[k] = si[DIMER_SI * k + 5];
    if (o->n_evaluated) o->n_evaluated[k] = s->evaluated[k];
  }
  return CHG_OK;
}

int chg_dimer_free(chg_engine* eng, chg_dimer* s) {
  if (!s) return CHG_OK;
  release(eng, s);
  delete s;
  return CHG_OK;
}

int chg_test_dimer_step(chg_engine* eng, const chg_dimer_params* params, int32_t n_searches, const int32_t* atom_off, double* r, double* nvec,
                        double* theta, double* v, double* f0, double* f1, double* sd, int32_t* si, float* e_img, float* f_img,
                        const float* energy, const float* force, int32_t final_try, const uint8_t* fixed, double* frac_next,
                        int32_t* phase_next, int32_t* status_next, int32_t* retry) {
  const char* fn = "chg_test_dimer_step";
  if (!eng || !params || n_searches <= 0 || !atom_off || !r || !nvec || !theta || !v || !f0 || !f1 || !sd || !si || !e_img || !f_img || !energy ||
      !force || !frac_next || !phase_next || !status_next || !retry)
    return CHG_EINVAL;
  TRY(check_params(eng, fn, params));
  const size_t S = n_searches;
  if (atom_off[0] != 0) return CHG_EINVAL;
  for (size_t k = 0; k < S; ++k)
    if (atom_off[k + 1] <= atom_off[k]) return CHG_EINVAL;
  const size_t NA = atom_off[S];
  // the evaluated batch: two structures of a search in phase PROBE, one of a search in phase TRIAL, search after search
  std::vector<int> tab(4 * S), b_aoff;
  int bs = 0;
  b_aoff.push_back(0);
  for (size_t k = 0; k < S; ++k) {
    const int n = atom_off[k + 1] - atom_off[k], nev = si[DIMER_SI * k + 3] == DIMER_PROBE ? 2 : 1;
    tab[4 * k] = (int)k; tab[4 * k + 1] = bs; tab[4 * k + 2] = nev; tab[4 * k + 3] = 2 * atom_off[k];
    for (int i = 0; i < nev; ++i) b_aoff.push_back(b_aoff.back() + n);
    bs += nev;
  }
  const size_t nbs = bs, nba = b_aoff.back();
  TestBuf bufs[] = {{r, r, sizeof(double) * 3 * NA}, {nvec, nvec, sizeof(double) * 3 * NA}, {theta, theta, sizeof(double) * 3 * NA},
                    {v, v, sizeof(double) * 3 * NA}, {f0, f0, sizeof(double) * 3 * NA}, {f1, f1, sizeof(double) * 3 * NA},
                    {sd, sd, sizeof(double) * DIMER_SD * S}, {si, si, sizeof(int) * DIMER_SI * S}, {e_img, e_img, sizeof(float) * 2 * S},
                    {atom_off, nullptr, sizeof(int) * (S + 1)}, {energy, nullptr, sizeof(float) * nbs}, {force, nullptr, sizeof(float) * 3 * nba},
                    {b_aoff.data(), nullptr, sizeof(int) * (nbs + 1)}, {tab.data(), nullptr, sizeof(int) * 4 * S},
                    {frac_next, frac_next, sizeof(double) * 6 * NA}, {phase_next, phase_next, sizeof(int) * S},
                    {status_next, status_next, sizeof(int) * S}, {retry, retry, sizeof(int) * S}, {fixed, nullptr, 3 * NA},
                    {f_img, f_img, sizeof(float) * 6 * NA}};
  return run_test_step(eng, fn, bufs, [&] {
    DimerStepArgs a = step_args(*params);
    a.r = (double*)bufs[0].d; a.nvec = (double*)bufs[1].d; a.theta = (double*)bufs[2].d; a.v = (double*)bufs[3].d;
    a.f0 = (double*)bufs[4].d; a.f1 = (double*)bufs[5].d; a.sd = (double*)bufs[6].d; a.si = (int*)bufs[7].d;
    a.e_img = (float*)bufs[8].d; a.f_img = (float*)bufs[19].d;
    a.aoff = (const int*)bufs[9].d; a.energy = (const float*)bufs[10].d; a.force = (const float*)bufs[11].d;
    a.b_atom_off = (const int*)bufs[12].d; a.tab = (const int*)bufs[13].d; a.frac_next = (double*)bufs[14].d;
    a.phase_next = (int*)bufs[15].d; a.status_next = (int*)bufs[16].d; a.retry = (int*)bufs[17].d;
    a.fixed = fixed ? (const unsigned char*)bufs[18].d : nullptr;
    a.final_try = final_try ? 1 : 0;
    launch_step(eng, a, (int)S);
  });
}

}  // extern "C"
