// engine_relax.hip -- batched structure relaxation (chg_relax_*): FIRE (kernels_relax.h) or L-BFGS (kernels_lbfgs.h, handles made by
// chg_relax_create_lbfgs) through the Frechet cell filter, one independent optimizer per structure, state in HBM.  Reference:
// StructOptimizer.relax, chgnet/model/dynamics.py:184-346.
//
// One step of chg_relax_run is one evaluate_and_step of the shared driver (engine_stepper.h) on the ACTIVE structures, with
// k_relax_step or k_lbfgs_step as the step launch (one workgroup per active structure, batch -> original index array) and the statuses copied back
// with the next coordinates; then compaction on the host: structures that stopped drop out of the next build.
#include "engine_stepper.h"

#include "kernels_lbfgs.h"
#include "kernels_relax.h"

struct chg_relax : chgh::Stepper {
  chg_relax_params p{};
  bool lbfgs = false;
  chg_lbfgs_params lp{};
  int M = 0;                                   // L-BFGS: slots of the history ring, min(memory, max_steps) and at least 1
  // device: state (original numbering) + per-step buffers (batch numbering, sized for the whole set)
  double *q, *v, *sd, *frac_eval, *lat_eval;
  double *r0, *g0, *S, *Y, *rho, *abuf, *w;    // L-BFGS (v is FIRE's); S / Y are indexed by original number: compaction never moves them
  int *si, *d_aoff, *d_orig, *status_next;
  float *e_out, *f_out, *s_out, *m_out;
  // pinned host (Stepper::h_extra): batch -> original index and the step's statuses, in batch order
  int *h_orig, *h_status;
  int n_active = 0;
  bool ran = false;                            // chg_relax_run has been called: the mask can no longer change
  double* frac0 = nullptr;                     // the fractional coordinates as given (fully held atoms keep them)
};

namespace {

void carve_relax(chg_relax* r, Carver& c) {
  const size_t B = r->B, N = r->N, rows = N + 3 * B;
  r->q = c.take<double>(3 * rows);
  if (r->lbfgs) {
    const size_t M = r->M;
    r->v = nullptr;
    r->r0 = c.take<double>(3 * rows);
    r->g0 = c.take<double>(3 * rows);
    r->w = c.take<double>(3 * rows);
    r->S = c.take<double>(M * 3 * rows);
    r->Y = c.take<double>(M * 3 * rows);
    r->rho = c.take<double>(M * B);
    r->abuf = c.take<double>(M * B);
  } else {
    r->v = c.take<double>(3 * rows);
  }
  r->sd = c.take<double>(RELAX_SD * B);
  r->frac_eval = c.take<double>(3 * N);
  r->lat_eval = c.take<double>(9 * B);
  r->frac_next = c.take<double>(3 * N);
  r->lat_next = c.take<double>(9 * B);
  r->si = c.take<int>(RELAX_SI * B);
  r->d_aoff = c.take<int>(B + 1);
  r->d_orig = c.take<int>(B);
  r->d_sel = c.take<int>(B);
  r->status_next = c.take<int>(B);
  r->retry = c.take<int>(B);
  r->e_out = c.take<float>(B);
  r->f_out = c.take<float>(3 * N);
  r->s_out = c.take<float>(9 * B);
  r->m_out = c.take<float>(N);
  r->d_fixed = c.take<unsigned char>(3 * N);
  r->d_nfree = c.take<int>(B);
  r->frac0 = c.take<double>(3 * N);
}

// lbfgs null: the FIRE numbers of *p are checked; otherwise they are ignored and *lbfgs is checked
int check_params(chg_engine* eng, const char* fn, const chg_relax_params* p, const chg_lbfgs_params* lbfgs) {
  const char* bad = nullptr;
  if (!(p->fmax >= 0.0)) bad = "fmax must be >= 0";
  else if (p->max_steps < 0) bad = "max_steps must be >= 0";
  else if (!(p->r_atom > 0.0) || !(p->r_bond > 0.0)) bad = "graph cutoffs must be > 0";
  else if (lbfgs) {
    if (!(lbfgs->maxstep > 0.0) || !(lbfgs->damping > 0.0) || !(lbfgs->alpha > 0.0)) bad = "maxstep, damping and alpha must be > 0";
    else if (lbfgs->memory < 1) bad = "memory must be >= 1";
  }
  else if (!(p->dt > 0.0) || !(p->maxstep > 0.0) || !(p->dtmax > 0.0)) bad = "dt, maxstep and dtmax must be > 0";
  else if (!(p->finc > 0.0) || !(p->fdec > 0.0) || !(p->astart >= 0.0) || !(p->fa > 0.0)) bad = "finc, fdec, fa must be > 0 and astart >= 0";
  if (bad) { eng->err = std::string(fn) + ": " + bad; return CHG_EINVAL; }
  return CHG_OK;
}

RelaxStepArgs step_args(const chg_relax_params& p, int relax_cell) {
  RelaxStepArgs a{};
  a.fmax2 = p.fmax * p.fmax;
  a.maxstep = p.maxstep; a.dtmax = p.dtmax; a.finc = p.finc; a.fdec = p.fdec; a.astart = p.astart; a.fa = p.fa;
  a.stress_weight = p.stress_weight > 0.0 ? p.stress_weight : 1.0 / 160.21766208;
  a.max_steps = p.max_steps; a.nmin = p.nmin; a.relax_cell = relax_cell;
  return a;
}

// host-side initial state of structure o (original numbering) into q / sd / si images
void init_state(const chg_structs_host* h, const chg_relax_params* p, int o, double* q, double* sd, int* si) {
  const int a0 = h->atom_off[o], n = h->atom_off[o + 1] - a0;
  double* qo = q + 3 * ((size_t)a0 + 3 * (size_t)o);
  initial_geometry(h, o, qo, sd);                     // u = r F^-T = r at F = I; L0, L0^-1
  for (int i = 0; i < 9; ++i) qo[3 * n + i] = 0.0;   // X = c log F = 0
  sd[18] = p->exp_cell_factor > 0.0 ? p->exp_cell_factor : (double)n;
  sd[19] = p->dt;
  sd[20] = p->astart;
  sd[21] = sd[22] = sd[23] = 0.0;
  si[0] = si[1] = si[2] = si[3] = 0;
}

// mk.fixed null: the unconstrained kernel
void launch_step(chg_engine* eng, const RelaxStepArgs& a, const RelaxMask& mk, int grid) {
  LaunchScope ls(eng, "relax_step");
  if (mk.fixed) hipLaunchKernelGGL(k_relax_step<true>, dim3((unsigned)grid), dim3(256), 0, eng->stream, a, mk);
  else hipLaunchKernelGGL(k_relax_step<false>, dim3((unsigned)grid), dim3(256), 0, eng->stream, a, mk);
}

LbfgsStepArgs lbfgs_args(const chg_relax_params& p, const chg_lbfgs_params& lp, int M, size_t rows) {
  LbfgsStepArgs a{};
  a.c = step_args(p, p.relax_cell);
  a.c.maxstep = lp.maxstep;
  a.alpha = lp.alpha; a.damping = lp.damping;
  a.M = M; a.R = rows;
  return a;
}

int ring_slots(const chg_relax_params& p, const chg_lbfgs_params& lp) { return std::max(1, std::min(lp.memory, p.max_steps)); }

void launch_lbfgs(chg_engine* eng, const LbfgsStepArgs& a, const RelaxMask& mk, int grid) {
  LaunchScope ls(eng, "lbfgs_step");
  if (mk.fixed) hipLaunchKernelGGL(k_lbfgs_step<true>, dim3((unsigned)grid), dim3(256), 0, eng->stream, a, mk);
  else hipLaunchKernelGGL(k_lbfgs_step<false>, dim3((unsigned)grid), dim3(256), 0, eng->stream, a, mk);
}

// chg_relax_create and chg_relax_create_lbfgs (lbfgs non-null)
int create(chg_engine* eng, const char* fn, const chg_structs_host* h, const chg_relax_params* params, const chg_lbfgs_params* lbfgs,
           chg_relax** out) {
  if (!eng || !h || !params || !out) return CHG_EINVAL;
  *out = nullptr;
  TRY(check_params(eng, fn, params, lbfgs));
  TRY(check_structs(eng, fn, h));
  HIP_TRY(eng, hipSetDevice(eng->device));
  const int B = h->n_struct, N = h->n_atoms;
  chg_relax* r = new chg_relax();
  r->p = *params;
  if (lbfgs) { r->lbfgs = true; r->lp = *lbfgs; r->M = ring_slots(*params, *lbfgs); }
  r->task = CHG_TASK_E | CHG_TASK_F | CHG_TASK_S | CHG_TASK_M;
  r->r_atom = params->r_atom; r->r_bond = params->r_bond; r->numerical_tol = params->numerical_tol;
  int s = alloc_state(eng, fn, r, h, 2, [&](Carver& c) { carve_relax(r, c); });
  if (s != CHG_OK) { chg_relax_free(eng, r); return s; }
  r->h_orig = r->h_extra;
  r->h_status = r->h_extra + B;
  for (int o = 0; o < B; ++o) r->h_orig[o] = o;
  r->n_active = B;
  // initial state on the host, one upload (L-BFGS: r0, g0 and the ring are written before they are read, the counters start at 0)
  std::vector<double> q(3 * ((size_t)N + 3 * (size_t)B)), sd((size_t)RELAX_SD * B);
  std::vector<int> si((size_t)RELAX_SI * B);
  for (int o = 0; o < B; ++o) init_state(h, params, o, q.data(), sd.data() + (size_t)RELAX_SD * o, si.data() + (size_t)RELAX_SI * o);
  StateUpload up{eng, fn};
  up(r->q, q.data(), sizeof(double) * q.size());
  up(r->sd, sd.data(), sizeof(double) * sd.size());
  up(r->si, si.data(), sizeof(int) * si.size());
  up(r->d_aoff, h->atom_off, sizeof(int) * (B + 1));
  if (r->lbfgs) {
    up.zero(r->r0, sizeof(double) * q.size());
    up.zero(r->g0, sizeof(double) * q.size());
  } else {
    up.zero(r->v, sizeof(double) * q.size());
  }
  up.zero(r->e_out, sizeof(float) * B);
  up.zero(r->f_out, sizeof(float) * 3 * (size_t)N);
  up.zero(r->s_out, sizeof(float) * 9 * (size_t)B);
  up.zero(r->m_out, sizeof(float) * N);
  up.zero(r->frac_eval, sizeof(double) * 3 * (size_t)N);
  up.zero(r->lat_eval, sizeof(double) * 9 * (size_t)B);
  if ((s = up.finish()) != CHG_OK) { chg_relax_free(eng, r); return s; }
  *out = r;
  return CHG_OK;
}

}  // namespace

extern "C" {

int chg_relax_create(chg_engine* eng, const chg_structs_host* h, const chg_relax_params* params, chg_relax** out) {
  return create(eng, "chg_relax_create", h, params, nullptr, out);
}

int chg_relax_create_lbfgs(chg_engine* eng, const chg_structs_host* h, const chg_relax_params* params, const chg_lbfgs_params* lbfgs,
                           chg_relax** out) {
  if (!lbfgs) return CHG_EINVAL;
  return create(eng, "chg_relax_create_lbfgs", h, params, lbfgs, out);
}

int chg_relax_run(chg_engine* eng, chg_relax* r, int32_t n_steps, int32_t* n_active) {
  if (!eng || !r || n_steps < 0) return CHG_EINVAL;
  HIP_TRY(eng, hipSetDevice(eng->device));
  RelaxStepArgs a = step_args(r->p, r->p.relax_cell);
  a.q = r->q; a.v = r->v; a.sd = r->sd; a.si = r->si; a.aoff = r->d_aoff;
  a.e_out = r->e_out; a.f_out = r->f_out; a.s_out = r->s_out; a.m_out = r->m_out; a.frac_eval = r->frac_eval; a.lat_eval = r->lat_eval;
  a.frac_next = r->frac_next; a.lat_next = r->lat_next; a.status_next = r->status_next; a.retry = r->retry;
  a.orig = r->d_orig;
  RelaxMask mk{};
  if (r->has_fixed) { mk.fixed = r->d_fixed; mk.frac0 = r->frac0; }
  r->ran = true;
  LbfgsStepArgs l{};
  if (r->lbfgs) {
    l = lbfgs_args(r->p, r->lp, r->M, (size_t)r->N + 3 * (size_t)r->B);
    l.r0 = r->r0; l.g0 = r->g0; l.S = r->S; l.Y = r->Y; l.rho = r->rho; l.abuf = r->abuf; l.w = r->w;
  }
  auto launch = [&](const chg_batch* b, const int* sel, int final_try, int grid) {
    a.energy = b->energy; a.force = b->force; a.stress = b->virial; a.magmom = b->magmom; a.b_atom_off = b->atom_off;
    a.sel = sel;
    a.final_try = final_try;
    if (r->lbfgs) {
      const double maxstep = l.c.maxstep;
      l.c = a;
      l.c.maxstep = maxstep;
      launch_lbfgs(eng, l, mk, grid);
    } else {
      launch_step(eng, a, mk, grid);
    }
  };
  for (int it = 0; it < n_steps && r->n_active > 0; ++it) {
    const int Ba = r->n_active;
    if (hipMemcpyAsync(r->d_orig, r->h_orig, sizeof(int) * Ba, hipMemcpyHostToDevice, eng->stream) != hipSuccess) {
      eng->err = "chg_relax_run: index upload failed";
      return CHG_EHIP;
    }
    TRY(evaluate_and_step(eng, "chg_relax_run", r, Ba, r->status_next, r->h_status, launch));
    // compaction: the structures still running keep their order; rows only move towards the front
    int j = 0, na = 0;
    for (int i = 0; i < Ba; ++i) {
      if (r->h_status[i] != CHG_RELAX_RUNNING) continue;
      const int s0 = r->h_aoff[i], n = r->h_aoff[i + 1] - s0;
      if (j != i) {
        std::memmove(r->h_frac + 3 * (size_t)na, r->h_frac + 3 * (size_t)s0, sizeof(double) * 3 * n);
        std::memmove(r->h_z + na, r->h_z + s0, sizeof(int) * n);
        std::memcpy(r->h_lat + 9 * (size_t)j, r->h_lat + 9 * (size_t)i, sizeof(double) * 9);
        r->h_orig[j] = r->h_orig[i];
      }
      r->h_aoff[j] = na;
      na += n;
      ++j;
    }
    r->h_aoff[j] = na;
    r->n_active = j;
  }
  if (n_active) *n_active = r->n_active;
  if (eng->profiling) return collect_profile(eng);
  return CHG_OK;
}

int chg_relax_set_fixed(chg_engine* eng, chg_relax* r, const uint8_t* fixed) {
  if (!eng || !r) return CHG_EINVAL;
  const char* fn = "chg_relax_set_fixed";
  if (r->ran) { eng->err = std::string(fn) + ": the relaxation has already run"; return CHG_EINVAL; }
  std::vector<int> nfree((size_t)r->B);
  if (fixed) TRY(check_fixed(eng, fn, r->B, r->h_aoff, fixed, r->p.relax_cell != 0, false, nfree.data()));
  HIP_TRY(eng, hipSetDevice(eng->device));
  if (fixed && hipMemcpyAsync(r->frac0, r->h_frac, sizeof(double) * 3 * (size_t)r->N, hipMemcpyHostToDevice, eng->stream) != hipSuccess) {
    eng->err = std::string(fn) + ": mask upload failed";
    return CHG_EHIP;
  }
  return upload_fixed(eng, fn, r, fixed, nfree.data());
}

int chg_relax_download(chg_engine* eng, chg_relax* r, const chg_relax_out_host* o) {
  if (!eng || !r || !o) return CHG_EINVAL;
  HIP_TRY(eng, hipSetDevice(eng->device));
  const size_t B = r->B, N = r->N;
  TRY(d2h(eng, o->frac, r->frac_eval, 3 * N));
  TRY(d2h(eng, o->lattice, r->lat_eval, 9 * B));
  TRY(d2h(eng, o->energy, r->e_out, B));
  TRY(d2h(eng, o->force, r->f_out, 3 * N));
  TRY(d2h(eng, o->stress, r->s_out, 9 * B));
  TRY(d2h(eng, o->magmom, r->m_out, N));
  std::vector<int> si;
  if (o->n_steps || o->status) {
    si.resize((size_t)RELAX_SI * B);
    TRY(d2h(eng, si.data(), r->si, si.size()));
  }
  HIP_TRY(eng, hipStreamSynchronize(eng->stream));
  for (size_t i = 0; i < B && !si.empty(); ++i) {
    if (o->n_steps) o->n_steps[i] = si[RELAX_SI * i + 1];
    if (o->status) o->status[i] = si[RELAX_SI * i + 2];
  }
  return CHG_OK;
}

int chg_relax_free(chg_engine* eng, chg_relax* r) {
  if (!r) return CHG_OK;
  release(eng, r);
  delete r;
  return CHG_OK;
}

// chg_test_relax_step (fixed null) and chg_test_relax_step_fixed
static int test_relax_step(chg_engine* eng, const char* fn, const chg_relax_params* params, int32_t n_struct, const int32_t* atom_off, double* q,
                           double* v, double* sd, int32_t* si, const float* energy, const float* force, const float* stress,
                           const float* magmom, double* frac_next, double* lat_next, const uint8_t* fixed) {
  if (!eng || !params || n_struct <= 0 || !atom_off || !q || !v || !sd || !si || !energy || !force || !stress || !frac_next || !lat_next)
    return CHG_EINVAL;
  const size_t B = n_struct, N = atom_off[n_struct], rows = N + 3 * B;
  if (atom_off[0] != 0) return CHG_EINVAL;
  for (size_t o = 0; o < B; ++o)
    if (atom_off[o + 1] <= atom_off[o]) return CHG_EINVAL;
  std::vector<int> nfree(B);
  if (fixed) TRY(check_fixed(eng, fn, (int)B, atom_off, fixed, params->relax_cell != 0, false, nfree.data()));
  TestBuf bufs[] = {{q, q, sizeof(double) * 3 * rows}, {v, v, sizeof(double) * 3 * rows}, {sd, sd, sizeof(double) * RELAX_SD * B},
                    {si, si, sizeof(int) * RELAX_SI * B}, {atom_off, nullptr, sizeof(int) * (B + 1)}, {energy, nullptr, sizeof(float) * B},
                    {force, nullptr, sizeof(float) * 3 * N}, {stress, nullptr, sizeof(float) * 9 * B}, {magmom, nullptr, sizeof(float) * N},
                    {frac_next, frac_next, sizeof(double) * 3 * N}, {lat_next, lat_next, sizeof(double) * 9 * B},
                    {nullptr, nullptr, sizeof(int) * B}, {nullptr, nullptr, sizeof(int) * B}, {fixed, nullptr, 3 * N}};
  return run_test_step(eng, fn, bufs, [&] {
    RelaxStepArgs a = step_args(*params, params->relax_cell);
    a.q = (double*)bufs[0].d; a.v = (double*)bufs[1].d; a.sd = (double*)bufs[2].d; a.si = (int*)bufs[3].d; a.aoff = (const int*)bufs[4].d;
    a.energy = (const float*)bufs[5].d; a.force = (const float*)bufs[6].d; a.stress = (const float*)bufs[7].d;
    a.magmom = magmom ? (const float*)bufs[8].d : nullptr; a.b_atom_off = (const int*)bufs[4].d;
    a.frac_next = (double*)bufs[9].d; a.lat_next = (double*)bufs[10].d; a.status_next = (int*)bufs[11].d; a.retry = (int*)bufs[12].d;
    a.final_try = 1;
    RelaxMask mk{};
    if (fixed) mk.fixed = (const unsigned char*)bufs[13].d;
    launch_step(eng, a, mk, (int)B);
  });
}

int chg_test_relax_step(chg_engine* eng, const chg_relax_params* params, int32_t n_struct, const int32_t* atom_off, double* q, double* v,
                        double* sd, int32_t* si, const float* energy, const float* force, const float* stress, const float* magmom,
                        double* frac_next, double* lat_next) {
  return test_relax_step(eng, "chg_test_relax_step", params, n_struct, atom_off, q, v, sd, si, energy, force, stress, magmom, frac_next,
                         lat_next, nullptr);
}

int chg_test_relax_step_fixed(chg_engine* eng, const chg_relax_params* params, int32_t n_struct, const int32_t* atom_off, double* q, double* v,
                              double* sd, int32_t* si, const float* energy, const float* force, const float* stress, const float* magmom,
                              double* frac_next, double* lat_next, const uint8_t* fixed) {
  return test_relax_step(eng, "chg_test_relax_step_fixed", params, n_struct, atom_off, q, v, sd, si, energy, force, stress, magmom, frac_next,
                         lat_next, fixed);
}

// chg_test_lbfgs_step (fixed null) and chg_test_lbfgs_step_fixed
static int test_lbfgs_step(chg_engine* eng, const char* fn, const chg_relax_params* params, const chg_lbfgs_params* lbfgs, int32_t n_struct,
                           const int32_t* atom_off, double* q, double* r0, double* g0, double* S, double* Y, double* rho, double* sd,
                           int32_t* si, const float* energy, const float* force, const float* stress, const float* magmom, int32_t final_try,
                           double* frac_next, double* lat_next, int32_t* retry, const uint8_t* fixed) {
  if (!eng || !params || !lbfgs || n_struct <= 0 || !atom_off || !q || !r0 || !g0 || !S || !Y || !rho || !sd || !si || !energy || !force ||
      !stress || !frac_next || !lat_next || !retry)
    return CHG_EINVAL;
  TRY(check_params(eng, fn, params, lbfgs));
  const size_t B = n_struct, N = atom_off[n_struct], rows = N + 3 * B, M = ring_slots(*params, *lbfgs);
  if (atom_off[0] != 0) return CHG_EINVAL;
  for (size_t o = 0; o < B; ++o)
    if (atom_off[o + 1] <= atom_off[o]) return CHG_EINVAL;
  std::vector<int> nfree(B);
  if (fixed) TRY(check_fixed(eng, fn, (int)B, atom_off, fixed, params->relax_cell != 0, false, nfree.data()));
  TestBuf bufs[] = {{q, q, sizeof(double) * 3 * rows}, {r0, r0, sizeof(double) * 3 * rows}, {g0, g0, sizeof(double) * 3 * rows},
                    {S, S, sizeof(double) * M * 3 * rows}, {Y, Y, sizeof(double) * M * 3 * rows}, {rho, rho, sizeof(double) * M * B},
                    {sd, sd, sizeof(double) * RELAX_SD * B}, {si, si, sizeof(int) * RELAX_SI * B}, {atom_off, nullptr, sizeof(int) * (B + 1)},
                    {energy, nullptr, sizeof(float) * B}, {force, nullptr, sizeof(float) * 3 * N}, {stress, nullptr, sizeof(float) * 9 * B},
                    {magmom, nullptr, sizeof(float) * N}, {frac_next, frac_next, sizeof(double) * 3 * N},
                    {lat_next, lat_next, sizeof(double) * 9 * B}, {retry, retry, sizeof(int) * B}, {nullptr, nullptr, sizeof(int) * B},
                    {nullptr, nullptr, sizeof(double) * M * B}, {nullptr, nullptr, sizeof(double) * 3 * rows}, {fixed, nullptr, 3 * N}};
  return run_test_step(eng, fn, bufs, [&] {
    LbfgsStepArgs a = lbfgs_args(*params, *lbfgs, (int)M, rows);
    a.c.q = (double*)bufs[0].d; a.r0 = (double*)bufs[1].d; a.g0 = (double*)bufs[2].d; a.S = (double*)bufs[3].d; a.Y = (double*)bufs[4].d;
    a.rho = (double*)bufs[5].d; a.c.sd = (double*)bufs[6].d; a.c.si = (int*)bufs[7].d; a.c.aoff = (const int*)bufs[8].d;
    a.c.energy = (const float*)bufs[9].d; a.c.force = (const float*)bufs[10].d; a.c.stress = (const float*)bufs[11].d;
    a.c.magmom = magmom ? (const float*)bufs[12].d : nullptr; a.c.b_atom_off = (const int*)bufs[8].d;
    a.c.frac_next = (double*)bufs[13].d; a.c.lat_next = (double*)bufs[14].d; a.c.retry = (int*)bufs[15].d; a.c.status_next = (int*)bufs[16].d;
    a.abuf = (double*)bufs[17].d; a.w = (double*)bufs[18].d;
    a.c.final_try = final_try ? 1 : 0;
    RelaxMask mk{};
    if (fixed) mk.fixed = (const unsigned char*)bufs[19].d;
    launch_lbfgs(eng, a, mk, (int)B);
  });
}

int chg_test_lbfgs_step(chg_engine* eng, const chg_relax_params* params, const chg_lbfgs_params* lbfgs, int32_t n_struct,
                        const int32_t* atom_off, double* q, double* r0, double* g0, double* S, double* Y, double* rho, double* sd, int32_t* si,
                        const float* energy, const float* force, const float* stress, const float* magmom, int32_t final_try,
                        double* frac_next, double* lat_next, int32_t* retry) {
  return test_lbfgs_step(eng, "chg_test_lbfgs_step", params, lbfgs, n_struct, atom_off, q, r0, g0, S, Y, rho, sd, si, energy, force, stress,
                         magmom, final_try, frac_next, lat_next, retry, nullptr);
}

int chg_test_lbfgs_step_fixed(chg_engine* eng, const chg_relax_params* params, const chg_lbfgs_params* lbfgs, int32_t n_struct,
                              const int32_t* atom_off, double* q, double* r0, double* g0, double* S, double* Y, double* rho, double* sd,
                              int32_t* si, const float* energy, const float* force, const float* stress, const float* magmom,
                              int32_t final_try, double* frac_next, double* lat_next, int32_t* retry, const uint8_t* fixed) {
  return test_lbfgs_step(eng, "chg_test_lbfgs_step_fixed", params, lbfgs, n_struct, atom_off, q, r0, g0, S, Y, rho, sd, si, energy, force,
                         stress, magmom, final_try, frac_next, lat_next, retry, fixed);
}

}  // extern "C"
