// engine_md.hip -- batched molecular dynamics (chg_md_*): NVE, NVT Berendsen, NPT Berendsen (inhomogeneous and isotropic), one
// independent replica per structure, state in HBM (kernels_md.h).  Reference: MolecularDynamics, chgnet/model/dynamics.py:433-780.
//
// One evaluation of chg_md_run:
//   chg_batch_build_predict on ALL replicas (host coordinates: the device graph build takes them from the host)
//   -> k_md_step, one workgroup per replica (finish the step, frame, start the next one)
//   -> one asynchronous copy of the next coordinates into pinned memory, one stream synchronisation.
// Every replica runs the same number of steps, so there is no compaction.  NPT takes two evaluations per step, as ASE does: the
// barostat's set_cell(scale_atoms=True) moves the atoms and the forces are evaluated again before the first half kick.
#include "engine_internal.h"

#include "kernels_md.h"

struct chg_md {
  int B = 0, N = 0;
  chg_md_params p{};
  uint32_t task = 0;
  bool started = false;      // the initial configuration has been evaluated (frame of step 0 written)
  int step = 0;              // steps completed (all replicas; a NONFINITE replica stops counting)
  // device: state + per-evaluation buffers
  char* d_mem = nullptr;
  double *r, *pm, *f, *m, *sd, *frac_next, *lat_next;
  int *si, *d_aoff, *d_sel, *retry;
  // frame ring: K slots
  int K = 0, ring_head = 0, ring_count = 0;
  std::vector<int> ring_step;
  double *fr_scal, *fr_pos, *fr_mom, *fr_cell;
  float *fr_force, *fr_stress, *fr_cfea;
  // pinned host: the next configuration (the build's input) and the retry flags
  char* h_mem = nullptr;
  double *h_frac, *h_lat;
  int *h_z, *h_aoff, *h_retry, *h_sel;
};

namespace {

constexpr int FEA = chg::D;

template <class Take>
void carve_md(chg_md* d, Take&& take_d) {
  const size_t B = d->B, N = d->N, K = d->K;
  d->r = take_d((double*)nullptr, 3 * N);
  d->pm = take_d((double*)nullptr, 3 * N);
  d->f = take_d((double*)nullptr, 3 * N);
  d->m = take_d((double*)nullptr, N);
  d->sd = take_d((double*)nullptr, MD_SD * B);
  d->frac_next = take_d((double*)nullptr, 3 * N);
  d->lat_next = take_d((double*)nullptr, 9 * B);
  d->si = take_d((int*)nullptr, MD_SI * B);
  d->d_aoff = take_d((int*)nullptr, B + 1);
  d->d_sel = take_d((int*)nullptr, B);
  d->retry = take_d((int*)nullptr, B);
  d->fr_scal = take_d((double*)nullptr, K * MD_FRAME_SCAL * B);
  d->fr_pos = take_d((double*)nullptr, K * 3 * N);
  d->fr_mom = take_d((double*)nullptr, K * 3 * N);
  d->fr_cell = take_d((double*)nullptr, K * 9 * B);
  d->fr_force = take_d((float*)nullptr, K * 3 * N);
  d->fr_stress = take_d((float*)nullptr, K * 9 * B);
  d->fr_cfea = take_d((float*)nullptr, d->p.log_crystal_fea ? K * FEA * B : 0);
}

struct Bump {   // offsets inside one allocation, 256-byte aligned (as engine_relax.hip)
  char* base;
  size_t pos = 0;
  template <class T>
  T* operator()(T*, size_t n) {
    pos = (pos + 255) & ~size_t(255);
    T* out = base ? reinterpret_cast<T*>(base + pos) : nullptr;
    pos += std::max<size_t>(n, 1) * sizeof(T);
    return out;
  }
};

void inv3h(const double* m, double* r) {
  const double det = m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6]) + m[2] * (m[3] * m[7] - m[4] * m[6]);
  const double id = 1.0 / det;
  r[0] = (m[4] * m[8] - m[5] * m[7]) * id; r[1] = (m[2] * m[7] - m[1] * m[8]) * id; r[2] = (m[1] * m[5] - m[2] * m[4]) * id;
  r[3] = (m[5] * m[6] - m[3] * m[8]) * id; r[4] = (m[0] * m[8] - m[2] * m[6]) * id; r[5] = (m[2] * m[3] - m[0] * m[5]) * id;
  r[6] = (m[3] * m[7] - m[4] * m[6]) * id; r[7] = (m[1] * m[6] - m[0] * m[7]) * id; r[8] = (m[0] * m[4] - m[1] * m[3]) * id;
}

bool is_npt(int e) { return e == MD_NPT_BERENDSEN_INHOMOGENEOUS || e == MD_NPT_BERENDSEN; }

const char* bad_params(const chg_md_params* p) {
  if (p->ensemble < MD_NVE || p->ensemble > MD_NPT_BERENDSEN) return "unknown ensemble";
  if (!(p->dt > 0.0) || !std::isfinite(p->dt)) return "dt must be > 0";
  if (p->ensemble != MD_NVE && (!(p->taut > 0.0) || !(p->temperature >= 0.0))) return "taut must be > 0 and temperature >= 0";
  if (is_npt(p->ensemble) && (!(p->taup > 0.0) || !(p->compressibility > 0.0) || !std::isfinite(p->pressure)))
    return "taup and compressibility must be > 0 and pressure finite";
  if (p->loginterval < 0 || p->ring_frames < 0) return "loginterval and ring_frames must be >= 0";
  if (p->loginterval > 0 && p->ring_frames < 1) return "frames need ring_frames >= 1";
  if (!(p->r_atom > 0.0) || !(p->r_bond > 0.0)) return "graph cutoffs must be > 0";
  return nullptr;
}

chg::MdStepArgs base_args(chg_md* d) {
  MdStepArgs a{};
  a.r = d->r; a.p = d->pm; a.f = d->f; a.m = d->m; a.sd = d->sd; a.si = d->si; a.aoff = d->d_aoff;
  a.frac_next = d->frac_next; a.lat_next = d->lat_next; a.retry = d->retry;
  const chg_md_params& p = d->p;
  a.dt = p.dt; a.temperature = p.temperature; a.taut = p.taut; a.taup = p.taup; a.pressure = p.pressure;
  a.compressibility = p.compressibility; a.kB = p.kB > 0.0 ? p.kB : 8.6173303e-5;
  a.stress_weight = p.stress_weight > 0.0 ? p.stress_weight : 1.0 / 160.21766208;
  a.ensemble = p.ensemble; a.fixcm = p.ensemble != MD_NVE && p.fixcm; a.fea_dim = FEA;
  return a;
}

void launch_step(chg_engine* eng, const MdStepArgs& a, int grid) {
  LaunchScope ls(eng, "md_step");
  hipLaunchKernelGGL(k_md_step, dim3((unsigned)grid), dim3(256), 0, eng->stream, a);
}

// copy the next configuration (and the retry flags) into pinned memory and wait for it
int copy_back(chg_engine* eng, chg_md* d) {
  hipStream_t st = eng->stream;
  if (hipMemcpyAsync(d->h_retry, d->retry, sizeof(int) * d->B, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipMemcpyAsync(d->h_frac, d->frac_next, sizeof(double) * 3 * (size_t)d->N, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipMemcpyAsync(d->h_lat, d->lat_next, sizeof(double) * 9 * (size_t)d->B, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess) {
    eng->err = "chg_md_run: copy of the next configuration failed";
    return CHG_EHIP;
  }
  return CHG_OK;
}

// evaluate the configuration in h_frac / h_lat, then one step launch with `a` (flags and frame slot set by the caller)
int evaluate_and_step(chg_engine* eng, chg_md* d, MdStepArgs a) {
  hipStream_t st = eng->stream;
  const chg_structs_host hs{d->B, d->N, d->h_z, d->h_frac, d->h_lat, d->h_aoff};
  chg_batch* b = nullptr;
  int32_t counts[6];
  TRY(chg_batch_build_predict(eng, &hs, d->p.r_atom, d->p.r_bond, d->p.numerical_tol, d->task, &b, counts));
  auto fail = [&](int s) { chg_batch_free(eng, b); return s; };
  a.energy = b->energy; a.force = b->force; a.stress = (d->task & CHG_TASK_S) ? b->virial : nullptr;
  a.cfea = a.fr_cfea ? b->crystal_fea : nullptr;
  a.sel = nullptr;
  a.final_try = b->wide_range ? 1 : 0;
  if (hipMemsetAsync(d->retry, 0, sizeof(int) * d->B, st) != hipSuccess) { eng->err = "chg_md_run: memset failed"; return fail(CHG_EHIP); }
  launch_step(eng, a, d->B);
  if (hipGetLastError() != hipSuccess) { eng->err = "chg_md_run: step kernel launch failed"; return fail(CHG_EHIP); }
  int s = copy_back(eng, d);
  if (s != CHG_OK) return fail(s);
  // non-finite results: the batch is evaluated again on the wide-range sweep (chg_batch_download does the same) and only the
  // replicas that were held back step; what is still non-finite there stops as NONFINITE with its state untouched
  int n_sel = 0;
  for (int i = 0; i < d->B; ++i)
    if (d->h_retry[i]) d->h_sel[n_sel++] = i;
  if (n_sel > 0) {
    b->wide_range = true;
    if (b->graph_exec) { hipGraphExecDestroy(b->graph_exec); b->graph_exec = nullptr; }
    s = chgh_wide::run_predict(eng, b, b->last_task ? b->last_task : d->task);
    if (s != CHG_OK) return fail(s);
    a.sel = d->d_sel;
    a.final_try = 1;
    if (hipMemcpyAsync(d->d_sel, d->h_sel, sizeof(int) * n_sel, hipMemcpyHostToDevice, st) != hipSuccess) {
      eng->err = "chg_md_run: index upload failed";
      return fail(CHG_EHIP);
    }
    launch_step(eng, a, n_sel);
    if (hipGetLastError() != hipSuccess) { eng->err = "chg_md_run: step kernel launch failed"; return fail(CHG_EHIP); }
    s = copy_back(eng, d);
    if (s != CHG_OK) return fail(s);
  }
  return chg_batch_free(eng, b);
}

// frame slot for step `step` (the caller checked that the ring has room)
void set_frame(chg_md* d, MdStepArgs& a, int step) {
  const size_t slot = (size_t)((d->ring_head + d->ring_count) % d->K), B = d->B, N = d->N;
  a.fr_scal = d->fr_scal + slot * MD_FRAME_SCAL * B;
  a.fr_pos = d->fr_pos + slot * 3 * N;
  a.fr_mom = d->fr_mom + slot * 3 * N;
  a.fr_cell = d->fr_cell + slot * 9 * B;
  a.fr_force = d->fr_force + slot * 3 * N;
  a.fr_stress = d->fr_stress + slot * 9 * B;
  a.fr_cfea = d->p.log_crystal_fea ? d->fr_cfea + slot * FEA * B : nullptr;
  d->ring_step[slot] = step;
  d->ring_count += 1;
}

bool frame_due(const chg_md* d, int step) { return d->p.loginterval > 0 && step % d->p.loginterval == 0; }

}  // namespace

extern "C" {

int chg_md_create(chg_engine* eng, const chg_structs_host* h, const double* masses, const double* momenta, const chg_md_params* params,
                  chg_md** out) {
  if (!eng || !h || !masses || !params || !out) return CHG_EINVAL;
  *out = nullptr;
  if (const char* bad = bad_params(params)) { eng->err = std::string("chg_md_create: ") + bad; return CHG_EINVAL; }
  const int B = h->n_struct, N = h->n_atoms;
  if (B <= 0 || N <= 0 || !h->z || !h->frac || !h->lattice || !h->atom_off) { eng->err = "chg_md_create: empty or null structures"; return CHG_EINVAL; }
  if (h->atom_off[0] != 0 || h->atom_off[B] != N) { eng->err = "chg_md_create: atom_off must run from 0 to n_atoms"; return CHG_EINVAL; }
  for (int o = 0; o < B; ++o)
    if (h->atom_off[o + 1] <= h->atom_off[o]) { eng->err = "chg_md_create: every structure needs at least one atom"; return CHG_EINVAL; }
  for (int i = 0; i < N; ++i)
    if (!(masses[i] > 0.0)) { eng->err = "chg_md_create: masses must be > 0"; return CHG_EINVAL; }
  HIP_TRY(eng, hipSetDevice(eng->device));
  chg_md* d = new chg_md();
  d->B = B; d->N = N; d->p = *params;
  d->K = params->loginterval > 0 ? params->ring_frames : 0;
  d->ring_step.assign(std::max(d->K, 1), 0);
  d->task = CHG_TASK_E | CHG_TASK_F | ((is_npt(params->ensemble) || params->log_stress) ? CHG_TASK_S : 0u);
  Bump sizer{nullptr};
  carve_md(d, sizer);
  const size_t dbytes = sizer.pos;
  if (hipMalloc(&d->d_mem, dbytes) != hipSuccess) {
    (void)hipGetLastError();
    delete d;
    eng->err = "chg_md_create: device state of " + std::to_string(dbytes) + " bytes cannot be allocated";
    return CHG_ENOMEM;
  }
  Bump carver{d->d_mem};
  carve_md(d, carver);
  const size_t hbytes = sizeof(double) * (3 * (size_t)N + 9 * (size_t)B) + sizeof(int) * ((size_t)N + 3 * (size_t)B + 1) + 1024;
  if (hipHostMalloc(&d->h_mem, hbytes, hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    hipFree(d->d_mem);
    delete d;
    eng->err = "chg_md_create: pinned staging cannot be allocated";
    return CHG_ENOMEM;
  }
  char* hp = d->h_mem;
  auto take_h = [&](size_t bytes) { char* x = hp; hp += (bytes + 7) & ~size_t(7); return x; };
  d->h_frac = (double*)take_h(sizeof(double) * 3 * N);
  d->h_lat = (double*)take_h(sizeof(double) * 9 * B);
  d->h_z = (int*)take_h(sizeof(int) * N);
  d->h_aoff = (int*)take_h(sizeof(int) * (B + 1));
  d->h_retry = (int*)take_h(sizeof(int) * B);
  d->h_sel = (int*)take_h(sizeof(int) * B);
  // initial state on the host, one upload: cartesian positions frac . L, the cell and its inverse
  std::vector<double> r(3 * (size_t)N), sd((size_t)MD_SD * B, 0.0);
  std::vector<int> si((size_t)MD_SI * B, 0);
  for (int o = 0; o < B; ++o) {
    const double* L = h->lattice + 9 * (size_t)o;
    for (int i = h->atom_off[o]; i < h->atom_off[o + 1]; ++i)
      for (int j = 0; j < 3; ++j) {
        const double* fr = h->frac + 3 * (size_t)i;
        r[3 * (size_t)i + j] = fr[0] * L[j] + fr[1] * L[3 + j] + fr[2] * L[6 + j];
      }
    for (int i = 0; i < 9; ++i) sd[(size_t)MD_SD * o + i] = L[i];
    inv3h(L, sd.data() + (size_t)MD_SD * o + 9);
  }
  std::memcpy(d->h_frac, h->frac, sizeof(double) * 3 * N);     // the first build evaluates the structures exactly as given
  std::memcpy(d->h_lat, h->lattice, sizeof(double) * 9 * B);
  std::memcpy(d->h_z, h->z, sizeof(int) * N);
  std::memcpy(d->h_aoff, h->atom_off, sizeof(int) * (B + 1));
  int s = CHG_OK;
  auto up = [&](void* dst, const void* src, size_t bytes) {
    if (s == CHG_OK && hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, eng->stream) != hipSuccess) {
      eng->err = "chg_md_create: state upload failed"; s = CHG_EHIP;
    }
  };
  up(d->r, r.data(), sizeof(double) * r.size());
  up(d->m, masses, sizeof(double) * N);
  up(d->sd, sd.data(), sizeof(double) * sd.size());
  up(d->si, si.data(), sizeof(int) * si.size());
  up(d->d_aoff, h->atom_off, sizeof(int) * (B + 1));
  up(d->frac_next, h->frac, sizeof(double) * 3 * N);
  up(d->lat_next, h->lattice, sizeof(double) * 9 * B);
  if (momenta) up(d->pm, momenta, sizeof(double) * 3 * N);
  else if (s == CHG_OK && hipMemsetAsync(d->pm, 0, sizeof(double) * 3 * (size_t)N, eng->stream) != hipSuccess) s = CHG_EHIP;
  if (s == CHG_OK && hipMemsetAsync(d->f, 0, sizeof(double) * 3 * (size_t)N, eng->stream) != hipSuccess) s = CHG_EHIP;
  if (s == CHG_OK && hipStreamSynchronize(eng->stream) != hipSuccess) { eng->err = "chg_md_create: synchronisation failed"; s = CHG_EHIP; }
  if (s != CHG_OK) { chg_md_free(eng, d); return s; }
  *out = d;
  return CHG_OK;
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
  const bool npt = is_npt(d->p.ensemble);
  if (!d->started) {   // evaluate the initial configuration: cached forces, Ekin / T, frame of step 0, and the first step's start
    MdStepArgs a = base_args(d);
    a.flags = MD_ABSORB | (n_steps > 0 ? MD_START : 0);
    if (frame_due(d, 0)) set_frame(d, a, 0);
    TRY(evaluate_and_step(eng, d, a));
    d->started = true;
  } else if (n_steps > 0) {   // a later call: start the step from the cached forces (ASE: get_forces() is cached)
    MdStepArgs a = base_args(d);
    a.flags = MD_START;
    launch_step(eng, a, d->B);
    if (hipGetLastError() != hipSuccess) { eng->err = "chg_md_run: step kernel launch failed"; return CHG_EHIP; }
    TRY(copy_back(eng, d));
  }
  for (int k = 0; k < n_steps; ++k) {
    if (npt) {   // the barostat's scaled configuration: forces, first half kick, fixcm, drift
      MdStepArgs a = base_args(d);
      a.flags = MD_ABSORB;
      TRY(evaluate_and_step(eng, d, a));
    }
    const int next = d->step + 1;
    MdStepArgs a = base_args(d);
    a.flags = MD_ABSORB | MD_KICK2 | (k + 1 < n_steps ? MD_START : 0);
    if (frame_due(d, next)) set_frame(d, a, next);
    TRY(evaluate_and_step(eng, d, a));
    d->step = next;
  }
  if (eng->profiling) return collect_profile(eng);
  return CHG_OK;
}

int chg_md_download(chg_engine* eng, chg_md* d, const chg_md_out_host* o) {
  if (!eng || !d || !o) return CHG_EINVAL;
  HIP_TRY(eng, hipSetDevice(eng->device));
  hipStream_t st = eng->stream;
  const size_t B = d->B, N = d->N;
  auto get = [&](void* dst, const void* src, size_t bytes) -> int {
    if (dst) HIP_TRY(eng, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st));
    return CHG_OK;
  };
  TRY(get(o->positions, d->r, sizeof(double) * 3 * N));
  TRY(get(o->momenta, d->pm, sizeof(double) * 3 * N));
  std::vector<double> sd;
  std::vector<int> si;
  if (o->cell) { sd.resize((size_t)MD_SD * B); TRY(get(sd.data(), d->sd, sizeof(double) * sd.size())); }
  if (o->n_steps || o->status) { si.resize((size_t)MD_SI * B); TRY(get(si.data(), d->si, sizeof(int) * si.size())); }
  // frames, oldest first
  const int take = std::min(d->ring_count, std::max(o->frame_capacity, 0));
  for (int k = 0; k < take; ++k) {
    const size_t slot = (size_t)((d->ring_head + k) % std::max(d->K, 1));
    if (o->frame_step) o->frame_step[k] = d->ring_step[slot];
    TRY(get(o->frame_scalars ? o->frame_scalars + k * MD_FRAME_SCAL * B : nullptr, d->fr_scal + slot * MD_FRAME_SCAL * B, sizeof(double) * MD_FRAME_SCAL * B));
    TRY(get(o->frame_positions ? o->frame_positions + k * 3 * N : nullptr, d->fr_pos + slot * 3 * N, sizeof(double) * 3 * N));
    TRY(get(o->frame_momenta ? o->frame_momenta + k * 3 * N : nullptr, d->fr_mom + slot * 3 * N, sizeof(double) * 3 * N));
    TRY(get(o->frame_cell ? o->frame_cell + k * 9 * B : nullptr, d->fr_cell + slot * 9 * B, sizeof(double) * 9 * B));
    TRY(get(o->frame_force ? o->frame_force + k * 3 * N : nullptr, d->fr_force + slot * 3 * N, sizeof(float) * 3 * N));
    TRY(get(o->frame_stress ? o->frame_stress + k * 9 * B : nullptr, d->fr_stress + slot * 9 * B, sizeof(float) * 9 * B));
    if (d->p.log_crystal_fea)
      TRY(get(o->frame_crystal_fea ? o->frame_crystal_fea + k * (size_t)FEA * B : nullptr, d->fr_cfea + slot * FEA * B, sizeof(float) * FEA * B));
  }
  HIP_TRY(eng, hipStreamSynchronize(st));
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

int chg_md_free(chg_engine* eng, chg_md* d) {
  if (!d) return CHG_OK;
  if (eng) { hipSetDevice(eng->device); hipStreamSynchronize(eng->stream); }
  if (d->d_mem) hipFree(d->d_mem);
  if (d->h_mem) hipHostFree(d->h_mem);
  delete d;
  return CHG_OK;
}

int chg_test_md_step(chg_engine* eng, const chg_md_params* params, int32_t n_struct, const int32_t* atom_off, int32_t flags, double* r,
                     double* momenta, double* forces, const double* masses, double* sd, int32_t* si, const float* energy, const float* force,
                     const float* stress, double* frac_next, double* lat_next) {
  if (!eng || !params || n_struct <= 0 || !atom_off || !r || !momenta || !forces || !masses || !sd || !si || !frac_next || !lat_next)
    return CHG_EINVAL;
  if ((flags & MD_ABSORB) && (!energy || !force)) return CHG_EINVAL;
  if (flags & ~(MD_ABSORB | MD_KICK2 | MD_START)) return CHG_EINVAL;
  if (const char* bad = bad_params(params)) { eng->err = std::string("chg_test_md_step: ") + bad; return CHG_EINVAL; }
  const size_t B = n_struct, N = atom_off[n_struct];
  if (atom_off[0] != 0) return CHG_EINVAL;
  for (size_t o = 0; o < B; ++o)
    if (atom_off[o + 1] <= atom_off[o]) return CHG_EINVAL;
  HIP_TRY(eng, hipSetDevice(eng->device));
  struct Buf { void* d; const void* h; size_t bytes; };
  Buf bufs[] = {{nullptr, r, sizeof(double) * 3 * N}, {nullptr, momenta, sizeof(double) * 3 * N}, {nullptr, forces, sizeof(double) * 3 * N},
                {nullptr, masses, sizeof(double) * N}, {nullptr, sd, sizeof(double) * MD_SD * B}, {nullptr, si, sizeof(int) * MD_SI * B},
                {nullptr, atom_off, sizeof(int) * (B + 1)}, {nullptr, energy, sizeof(float) * B}, {nullptr, force, sizeof(float) * 3 * N},
                {nullptr, stress, sizeof(float) * 9 * B}, {nullptr, frac_next, sizeof(double) * 3 * N}, {nullptr, lat_next, sizeof(double) * 9 * B},
                {nullptr, nullptr, sizeof(int) * B}};
  int s = CHG_OK;
  for (Buf& x : bufs) {
    if (s == CHG_OK && hipMalloc(&x.d, x.bytes) != hipSuccess) { eng->err = "chg_test_md_step: allocation failed"; s = CHG_ENOMEM; }
    if (s == CHG_OK && x.h && hipMemcpy(x.d, x.h, x.bytes, hipMemcpyHostToDevice) != hipSuccess) { eng->err = "chg_test_md_step: upload failed"; s = CHG_EHIP; }
  }
  if (s == CHG_OK) {
    chg_md tmp;
    tmp.p = *params;
    MdStepArgs a = base_args(&tmp);
    a.r = (double*)bufs[0].d; a.p = (double*)bufs[1].d; a.f = (double*)bufs[2].d; a.m = (const double*)bufs[3].d;
    a.sd = (double*)bufs[4].d; a.si = (int*)bufs[5].d; a.aoff = (const int*)bufs[6].d;
    a.energy = energy ? (const float*)bufs[7].d : nullptr; a.force = force ? (const float*)bufs[8].d : nullptr;
    a.stress = stress ? (const float*)bufs[9].d : nullptr;
    a.frac_next = (double*)bufs[10].d; a.lat_next = (double*)bufs[11].d; a.retry = (int*)bufs[12].d;
    a.flags = flags;
    a.final_try = 1;
    launch_step(eng, a, (int)B);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(eng->stream) != hipSuccess) { eng->err = "chg_test_md_step: kernel failed"; s = CHG_EHIP; }
  }
  void* outs[] = {r, momenta, forces, nullptr, sd, si, nullptr, nullptr, nullptr, nullptr, frac_next, lat_next};
  for (int i = 0; i < 12 && s == CHG_OK; ++i)
    if (outs[i] && hipMemcpy(outs[i], bufs[i].d, bufs[i].bytes, hipMemcpyDeviceToHost) != hipSuccess) {
      eng->err = "chg_test_md_step: download failed"; s = CHG_EHIP;
    }
  for (Buf& x : bufs)
    if (x.d) hipFree(x.d);
  return s;
}

}  // extern "C"
