// engine_neb.hip -- batched nudged elastic band (chg_neb_*): every image of every band is a structure of the batch, one FIRE
// optimizer per band (kernels_neb.h), state in HBM.  DESIGN.md "Nudged elastic band".
//
// The state, the staging and the test launch are the shared driver's (engine_stepper.h).  The evaluate-and-step loop is this file's
// own, because its unit is the band: the first evaluation stages every image (the end points' energies feed the tangents), later ones
// the interior images of the bands still running; a band with a non-finite image is held back and stepped again as a whole; a band
// that stops takes all its images out of the next build.
#include "engine_stepper.h"

#include "kernels_neb.h"

struct chg_neb : chgh::Stepper {
  chg_neb_params p{};
  int n_bands = 0;
  // device: state (original numbering) and the per-launch tables
  double *r, *v, *g, *sd, *frac_eval;
  int *si, *d_band_off, *d_aoff, *d_tab, *status_next;
  float *e_img, *f_img;
  // host: the bands as given (the staging holds only what the next build evaluates)
  std::vector<int> band_off, aoff, z;
  std::vector<double> lat;          // [n_bands, 9]
  std::vector<int> evaluated;       // [n_bands] structures predicted so far
  std::vector<int> active;          // bands still running, in order
  // pinned (Stepper::h_extra): the atom offsets of the staging are double-buffered -- the layout of the next build is needed for the
  // copy back while the arrays of this one may still be in flight
  int *h_aoff2, *h_tab, *h_status;
  int n_staged = 0;                 // structures staged for the next build
  bool first = true;                // the next evaluation is the first: all images are staged
};

namespace {

void carve_neb(chg_neb* s, Carver& c) {
  const size_t B = s->B, N = s->N, nb = s->n_bands;
  s->r = c.take<double>(3 * N);
  s->v = c.take<double>(3 * N);
  s->g = c.take<double>(3 * N);
  s->sd = c.take<double>(NEB_SD * nb);
  s->frac_eval = c.take<double>(3 * N);
  s->frac_next = c.take<double>(3 * N);
  s->lat_next = c.take<double>(9 * B);
  s->si = c.take<int>(NEB_SI * nb);
  s->d_band_off = c.take<int>(nb + 1);
  s->d_aoff = c.take<int>(B + 1);
  s->d_tab = c.take<int>(3 * nb);
  s->d_sel = c.take<int>(B);
  s->status_next = c.take<int>(B);
  s->retry = c.take<int>(B);
  s->e_img = c.take<float>(B);
  s->f_img = c.take<float>(3 * N);
  s->d_fixed = c.take<unsigned char>(3 * N);
  s->d_nfree = c.take<int>(B);
}

int check_params(chg_engine* eng, const char* fn, const chg_neb_params* p) {
  const char* bad = nullptr;
  if (!(p->fmax >= 0.0)) bad = "fmax must be >= 0";
  else if (p->max_steps < 0) bad = "max_steps must be >= 0";
  else if (!(p->r_atom > 0.0) || !(p->r_bond > 0.0)) bad = "graph cutoffs must be > 0";
  else if (!(p->dt > 0.0) || !(p->maxstep > 0.0) || !(p->dtmax > 0.0)) bad = "dt, maxstep and dtmax must be > 0";
  else if (!(p->finc > 0.0) || !(p->fdec > 0.0) || !(p->astart >= 0.0) || !(p->fa > 0.0)) bad = "finc, fdec, fa must be > 0 and astart >= 0";
  else if (!(p->spring >= 0.0)) bad = "spring must be >= 0";
  if (bad) { eng->err = std::string(fn) + ": " + bad; return CHG_EINVAL; }
  return CHG_OK;
}

// band_off against the images: lengths 3..66, every image of a band with the atoms, species and cell of its first one
int check_bands(chg_engine* eng, const char* fn, int B, const int* aoff, const int* z, const double* lat, const int* band_off, int n_bands) {
  auto bad = [&](const std::string& what) { eng->err = std::string(fn) + ": " + what; return CHG_EINVAL; };
  if (n_bands <= 0 || !band_off || band_off[0] != 0 || band_off[n_bands] != B) return bad("band_off must run from 0 to n_struct");
  for (int k = 0; k < n_bands; ++k) {
    const int i0 = band_off[k], M = band_off[k + 1] - i0;
    if (M < NEB_MIN_IMAGES || M > NEB_MAX_IMAGES)
      return bad("band " + std::to_string(k) + " has " + std::to_string(M) + " images; a band takes " + std::to_string(NEB_MIN_IMAGES) +
                 " to " + std::to_string(NEB_MAX_IMAGES));
    const int n = aoff[i0 + 1] - aoff[i0];
    for (int i = i0 + 1; i < i0 + M; ++i) {
      const std::string who = "image " + std::to_string(i - i0) + " of band " + std::to_string(k);
      if (aoff[i + 1] - aoff[i] != n) return bad(who + " differs from image 0 in atom count");
      if (z && std::memcmp(z + aoff[i], z + aoff[i0], sizeof(int) * n) != 0) return bad(who + " differs from image 0 in species");
      if (lat && std::memcmp(lat + 9 * (size_t)i, lat + 9 * (size_t)i0, sizeof(double) * 9) != 0) return bad(who + " differs from image 0 in cell");
    }
  }
  return CHG_OK;
}

NebStepArgs step_args(const chg_neb_params& p) {
  NebStepArgs a{};
  a.fmax2 = p.fmax * p.fmax;
  a.maxstep = p.maxstep; a.dtmax = p.dtmax; a.finc = p.finc; a.fdec = p.fdec; a.astart = p.astart; a.fa = p.fa; a.spring = p.spring;
  a.max_steps = p.max_steps; a.nmin = p.nmin; a.climb = p.climb ? 1 : 0;
  return a;
}

// a.fixed null: the unconstrained kernel
void launch_step(chg_engine* eng, const NebStepArgs& a, int grid) {
  LaunchScope ls(eng, "neb_step");
  if (a.fixed) hipLaunchKernelGGL(k_neb_step<true>, dim3((unsigned)grid), dim3(256), 0, eng->stream, a);
  else hipLaunchKernelGGL(k_neb_step<false>, dim3((unsigned)grid), dim3(256), 0, eng->stream, a);
}

// stage the interior images of the bands in `active` (coordinates apart) at aoff_out; returns the structures staged
int stage_interior(chg_neb* s, const std::vector<int>& active, int* aoff_out, bool with_species) {
  int st = 0, na = 0;
  for (int k : active) {
    const int i0 = s->band_off[k], M = s->band_off[k + 1] - i0, n = s->aoff[i0 + 1] - s->aoff[i0];
    for (int i = 1; i < M - 1; ++i) {
      aoff_out[st] = na;
      if (with_species) {
        std::memcpy(s->h_z + na, s->z.data() + s->aoff[i0], sizeof(int) * n);
        std::memcpy(s->h_lat + 9 * (size_t)st, s->lat.data() + 9 * (size_t)k, sizeof(double) * 9);
      }
      na += n;
      ++st;
    }
  }
  aoff_out[st] = na;
  return st;
}

// One evaluation of the staged structures and the band steps that follow it
int evaluate_and_step_bands(chg_engine* eng, const char* fn, chg_neb* s, NebStepArgs& a) {
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
  // where every active band sits in this batch and where its interior rows go in the next staging
  int bs = 0, noff = 0;
  for (int j = 0; j < nact; ++j) {
    const int k = s->active[j], i0 = s->band_off[k], M = s->band_off[k + 1] - i0, n = s->aoff[i0 + 1] - s->aoff[i0];
    s->h_tab[3 * j] = k; s->h_tab[3 * j + 1] = bs; s->h_tab[3 * j + 2] = noff;
    bs += s->first ? M : M - 2;
    noff += (M - 2) * n;
  }
  if (hipMemcpyAsync(s->d_tab, s->h_tab, sizeof(int) * 3 * nact, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemsetAsync(s->retry, 0, sizeof(int) * nact, st) != hipSuccess)
    return fail("band table upload failed", CHG_EHIP);
  // the next staging, should every band go on: its offsets go into the other buffer, which copy_back reads.  copy_back is the shared
  // one and copies per STRUCTURE of that staging: n_next >= nact entries of retry and status_next (device arrays of B ints, zeroed at
  // create; only the first nact mean anything) and 9 n_next doubles of lat_next, which no NEB kernel writes (the cell is fixed) and
  // which therefore overwrites h_lat with zeros -- stage_interior(..., true) at the end of this function rewrites h_z, h_lat and the
  // offsets from the bands as given, and must stay after the last copy_back
  const int n_next = stage_interior(s, s->active, s->h_aoff2, false);
  std::swap(s->h_aoff, s->h_aoff2);
  a.energy = b->energy; a.force = b->force; a.b_atom_off = b->atom_off; a.all_images = s->first ? 1 : 0;
  auto step = [&](const int* sel, int final_try, int grid) {
    a.sel = sel; a.final_try = final_try;
    launch_step(eng, a, grid);
    if (hipGetLastError() != hipSuccess) return fail("step kernel launch failed", CHG_EHIP);
    const int rc = copy_back(eng, fn, s, n_next, s->status_next, s->h_status);
    return rc == CHG_OK ? CHG_OK : fail(nullptr, rc);
  };
  TRY(step(nullptr, b->wide_range ? 1 : 0, nact));
  int n_sel = 0;
  for (int j = 0; j < nact; ++j)
    if (s->h_retry[j]) s->h_sel[n_sel++] = j;
  if (n_sel > 0) {   // as evaluate_and_step: the whole batch again on the wide-range sweep, then the held-back bands only
    b->wide_range = true;
    if (b->graph_exec) { hipGraphExecDestroy(b->graph_exec); b->graph_exec = nullptr; }
    const int rc = chgh_wide::run_predict(eng, b, b->last_task ? b->last_task : s->task);
    if (rc != CHG_OK) return fail(nullptr, rc);
    if (hipMemcpyAsync(s->d_sel, s->h_sel, sizeof(int) * n_sel, hipMemcpyHostToDevice, st) != hipSuccess) return fail("index upload failed", CHG_EHIP);
    TRY(step(s->d_sel, 1, n_sel));
  }
  TRY(chg_batch_free(eng, b));
  for (int k : s->active) s->evaluated[k] += s->first ? s->band_off[k + 1] - s->band_off[k] : s->band_off[k + 1] - s->band_off[k] - 2;
  s->first = false;
  // compaction: the bands still running keep their order, their interior rows only move towards the front
  std::vector<int> still;
  int na = 0, from = 0;
  for (int j = 0; j < nact; ++j) {
    const int k = s->active[j], i0 = s->band_off[k], M = s->band_off[k + 1] - i0, n = s->aoff[i0 + 1] - s->aoff[i0];
    const int rows = (M - 2) * n;
    if (s->h_status[j] == CHG_RELAX_RUNNING) {
      if (na != from) std::memmove(s->h_frac + 3 * (size_t)na, s->h_frac + 3 * (size_t)from, sizeof(double) * 3 * rows);
      na += rows;
      still.push_back(k);
    }
    from += rows;
  }
  s->active.swap(still);
  s->n_staged = stage_interior(s, s->active, s->h_aoff, true);
  return CHG_OK;
}

}  // namespace

extern "C" {

int chg_neb_create(chg_engine* eng, const chg_structs_host* h, const int32_t* band_off, int32_t n_bands, const chg_neb_params* params,
                   chg_neb** out) {
  const char* fn = "chg_neb_create";
  if (!eng || !h || !params || !out) return CHG_EINVAL;
  *out = nullptr;
  TRY(check_params(eng, fn, params));
  TRY(check_structs(eng, fn, h));
  TRY(check_bands(eng, fn, h->n_struct, h->atom_off, h->z, h->lattice, band_off, n_bands));
  HIP_TRY(eng, hipSetDevice(eng->device));
  const int B = h->n_struct, N = h->n_atoms;
  chg_neb* s = new chg_neb();
  s->p = *params;
  s->n_bands = n_bands;
  s->task = CHG_TASK_E | CHG_TASK_F;
  s->r_atom = params->r_atom; s->r_bond = params->r_bond; s->numerical_tol = params->numerical_tol;
  int rc = alloc_state(eng, fn, s, h, 4, [&](Carver& c) { carve_neb(s, c); });
  if (rc != CHG_OK) { chg_neb_free(eng, s); return rc; }
  // h_extra [4 B] ints: the second offsets buffer [B + 1 <= 2 B], the band table [3 n_bands <= B] and the statuses [B]
  s->h_aoff2 = s->h_extra;
  s->h_tab = s->h_extra + 2 * (size_t)B;
  s->h_status = s->h_extra + 3 * (size_t)B;
  s->band_off.assign(band_off, band_off + n_bands + 1);
  s->aoff.assign(h->atom_off, h->atom_off + B + 1);
  s->z.assign(h->z, h->z + N);
  s->lat.resize(9 * (size_t)n_bands);
  s->evaluated.assign(n_bands, 0);
  s->active.resize(n_bands);
  for (int k = 0; k < n_bands; ++k) {
    s->active[k] = k;
    std::memcpy(s->lat.data() + 9 * (size_t)k, h->lattice + 9 * (size_t)band_off[k], sizeof(double) * 9);
  }
  s->n_staged = B;
  // initial state on the host, one upload
  std::vector<double> r(3 * (size_t)N), sd((size_t)NEB_SD * n_bands, 0.0), geo(18);
  std::vector<int> si((size_t)NEB_SI * n_bands, 0);
  for (int o = 0; o < B; ++o) initial_geometry(h, o, r.data() + 3 * (size_t)h->atom_off[o], geo.data());
  for (int k = 0; k < n_bands; ++k) {
    double* d = sd.data() + (size_t)NEB_SD * k;
    for (int i = 0; i < 9; ++i) d[i] = s->lat[9 * (size_t)k + i];
    chg::inv3(d, d + 9);
    d[18] = params->dt;
    d[19] = params->astart;
    si[(size_t)NEB_SI * k + 3] = -1;
  }
  StateUpload up{eng, fn};
  up(s->r, r.data(), sizeof(double) * r.size());
  up(s->sd, sd.data(), sizeof(double) * sd.size());
  up(s->si, si.data(), sizeof(int) * si.size());
  up(s->d_band_off, band_off, sizeof(int) * (n_bands + 1));
  up(s->d_aoff, h->atom_off, sizeof(int) * (B + 1));
  up(s->frac_eval, h->frac, sizeof(double) * 3 * (size_t)N);
  up.zero(s->v, sizeof(double) * 3 * (size_t)N);
  up.zero(s->g, sizeof(double) * 3 * (size_t)N);
  up.zero(s->frac_next, sizeof(double) * 3 * (size_t)N);
  up.zero(s->lat_next, sizeof(double) * 9 * (size_t)B);
  up.zero(s->e_img, sizeof(float) * B);
  up.zero(s->f_img, sizeof(float) * 3 * (size_t)N);
  up.zero(s->status_next, sizeof(int) * B);
  up.zero(s->retry, sizeof(int) * B);
  if ((rc = up.finish()) != CHG_OK) { chg_neb_free(eng, s); return rc; }
  *out = s;
  return CHG_OK;
}

int chg_neb_set_fixed(chg_engine* eng, chg_neb* s, const uint8_t* fixed) {
  if (!eng || !s) return CHG_EINVAL;
  const char* fn = "chg_neb_set_fixed";
  if (!s->first) { eng->err = std::string(fn) + ": the band has already run"; return CHG_EINVAL; }
  std::vector<int> nfree((size_t)s->B);
  if (fixed) TRY(check_fixed(eng, fn, s->B, s->aoff.data(), fixed, false, false, nfree.data()));
  HIP_TRY(eng, hipSetDevice(eng->device));
  return upload_fixed(eng, fn, s, fixed, nfree.data());
}

int chg_neb_run(chg_engine* eng, chg_neb* s, int32_t n_steps, int32_t* n_active) {
  if (!eng || !s || n_steps < 0) return CHG_EINVAL;
  HIP_TRY(eng, hipSetDevice(eng->device));
  NebStepArgs a = step_args(s->p);
  a.r = s->r; a.v = s->v; a.g = s->g; a.sd = s->sd; a.si = s->si; a.e_img = s->e_img; a.f_img = s->f_img; a.frac_eval = s->frac_eval;
  a.band_off = s->d_band_off; a.aoff = s->d_aoff; a.fixed = s->has_fixed ? s->d_fixed : nullptr;
  a.tab = s->d_tab; a.frac_next = s->frac_next; a.status_next = s->status_next; a.retry = s->retry;
  for (int it = 0; it < n_steps && !s->active.empty(); ++it) TRY(evaluate_and_step_bands(eng, "chg_neb_run", s, a));
  if (n_active) *n_active = (int32_t)s->active.size();
  if (eng->profiling) return collect_profile(eng);
  return CHG_OK;
}

int chg_neb_download(chg_engine* eng, chg_neb* s, const chg_neb_out_host* o) {
  if (!eng || !s || !o) return CHG_EINVAL;
  HIP_TRY(eng, hipSetDevice(eng->device));
  const size_t B = s->B, N = s->N, nb = s->n_bands;
  TRY(d2h(eng, o->frac, s->frac_eval, 3 * N));
  TRY(d2h(eng, o->energy, s->e_img, B));
  TRY(d2h(eng, o->force, s->f_img, 3 * N));
  std::vector<int> si((size_t)NEB_SI * nb);
  std::vector<double> sd((size_t)NEB_SD * nb);
  TRY(d2h(eng, si.data(), s->si, si.size()));
  TRY(d2h(eng, sd.data(), s->sd, sd.size()));
  HIP_TRY(eng, hipStreamSynchronize(eng->stream));
  for (size_t k = 0; k < nb; ++k) {
    if (o->neb_fmax) o->neb_fmax[k] = sd[NEB_SD * k + 20];
    if (o->climbing_image) o->climbing_image[k] = si[NEB_SI * k + 3];
    if (o->n_steps) o->n_steps[k] = si[NEB_SI * k + 1];
    if (o->status) o->status[k] = si[NEB_SI * k + 2];
    if (o->n_evaluated) o->n_evaluated[k] = s->evaluated[k];
  }
  return CHG_OK;
}

int chg_neb_free(chg_engine* eng, chg_neb* s) {
  if (!s) return CHG_OK;
  release(eng, s);
  delete s;
  return CHG_OK;
}

int chg_test_neb_step(chg_engine* eng, const chg_neb_params* params, int32_t n_bands, const int32_t* band_off, const int32_t* atom_off,
                      double* r, double* v, double* g, double* sd, int32_t* si, float* e_img, const float* energy, const float* force,
                      int32_t all_images, int32_t final_try, const uint8_t* fixed, double* frac_next, int32_t* retry) {
  const char* fn = "chg_test_neb_step";
  if (!eng || !params || n_bands <= 0 || !band_off || !atom_off || !r || !v || !g || !sd || !si || !e_img || !energy || !force || !frac_next ||
      !retry)
    return CHG_EINVAL;
  TRY(check_params(eng, fn, params));
  const size_t nb = n_bands, B = band_off[n_bands] > 0 ? band_off[n_bands] : 0, N = B ? atom_off[B] : 0;
  if (B == 0 || atom_off[0] != 0) return CHG_EINVAL;
  for (size_t o = 0; o < B; ++o)
    if (atom_off[o + 1] <= atom_off[o]) return CHG_EINVAL;
  TRY(check_bands(eng, fn, (int)B, atom_off, nullptr, nullptr, band_off, n_bands));
  // the evaluated batch: every image, or the interior ones band after band
  std::vector<int> tab(3 * nb), b_aoff;
  int bs = 0, noff = 0;
  b_aoff.push_back(0);
  for (size_t k = 0; k < nb; ++k) {
    const int i0 = band_off[k], M = band_off[k + 1] - i0, n = atom_off[i0 + 1] - atom_off[i0], nev = all_images ? M : M - 2;
    tab[3 * k] = (int)k; tab[3 * k + 1] = bs; tab[3 * k + 2] = noff;
    for (int i = 0; i < nev; ++i) b_aoff.push_back(b_aoff.back() + n);
    bs += nev;
    noff += (M - 2) * n;
  }
  const size_t nbs = bs, nba = b_aoff.back();
  TestBuf bufs[] = {{r, r, sizeof(double) * 3 * N}, {v, v, sizeof(double) * 3 * N}, {g, g, sizeof(double) * 3 * N},
                    {sd, sd, sizeof(double) * NEB_SD * nb}, {si, si, sizeof(int) * NEB_SI * nb}, {e_img, e_img, sizeof(float) * B},
                    {band_off, nullptr, sizeof(int) * (nb + 1)}, {atom_off, nullptr, sizeof(int) * (B + 1)},
                    {energy, nullptr, sizeof(float) * nbs}, {force, nullptr, sizeof(float) * 3 * nba},
                    {b_aoff.data(), nullptr, sizeof(int) * (nbs + 1)}, {tab.data(), nullptr, sizeof(int) * 3 * nb},
                    {frac_next, frac_next, sizeof(double) * 3 * N}, {retry, retry, sizeof(int) * nb}, {nullptr, nullptr, sizeof(int) * nb},
                    {nullptr, nullptr, sizeof(float) * 3 * N}, {fixed, nullptr, 3 * N}};
  return run_test_step(eng, fn, bufs, [&] {
    NebStepArgs a = step_args(*params);
    a.r = (double*)bufs[0].d; a.v = (double*)bufs[1].d; a.g = (double*)bufs[2].d; a.sd = (double*)bufs[3].d; a.si = (int*)bufs[4].d;
    a.e_img = (float*)bufs[5].d; a.band_off = (const int*)bufs[6].d; a.aoff = (const int*)bufs[7].d;
    a.energy = (const float*)bufs[8].d; a.force = (const float*)bufs[9].d; a.b_atom_off = (const int*)bufs[10].d;
    a.tab = (const int*)bufs[11].d; a.frac_next = (double*)bufs[12].d; a.retry = (int*)bufs[13].d; a.status_next = (int*)bufs[14].d;
    a.f_img = (float*)bufs[15].d; a.frac_eval = nullptr;
    a.fixed = fixed ? (const unsigned char*)bufs[16].d : nullptr;
    a.all_images = all_images ? 1 : 0; a.final_try = final_try ? 1 : 0;
    launch_step(eng, a, (int)nb);
  });
}

}  // extern "C"
