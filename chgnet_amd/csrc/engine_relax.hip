// engine_relax.hip -- batched structure relaxation (chg_relax_*): FIRE through the Frechet cell filter, one independent optimizer per
// structure, state in HBM (kernels_relax.h).  Reference: StructOptimizer.relax, chgnet/model/dynamics.py:184-346.
//
// One step of chg_relax_run:
//   chg_batch_build_predict on the ACTIVE structures (host coordinates: the device graph build takes them from the host)
//   -> k_relax_step, one workgroup per active structure, batch -> original index array
//   -> one asynchronous copy of the next coordinates and statuses into pinned memory, one stream synchronisation
//   -> compaction on the host: structures that stopped drop out of the next build.
#include "engine_internal.h"

#include "kernels_relax.h"

struct chg_relax {
  int B = 0, N = 0;
  chg_relax_params p{};
  std::vector<int> z, aoff;      // original numbering
  // device: state (original numbering) + per-step buffers (batch numbering, sized for the whole set)
  char* d_mem = nullptr;
  double *q, *v, *sd, *frac_eval, *lat_eval, *frac_next, *lat_next;
  int *si, *d_aoff, *d_orig, *d_sel, *status_next, *retry;
  float *e_out, *f_out, *s_out, *m_out;
  // pinned host: the active set in batch order (next build's input) and the step's small outputs
  char* h_mem = nullptr;
  double *h_frac, *h_lat;
  int *h_z, *h_aoff, *h_orig, *h_status, *h_retry, *h_sel;
  int n_active = 0;
};

namespace {

template <class Take>
void carve_relax(chg_relax* r, Take&& take_d) {
  const size_t B = r->B, N = r->N, rows = N + 3 * B;
  r->q = take_d((double*)nullptr, 3 * rows);
  r->v = take_d((double*)nullptr, 3 * rows);
  r->sd = take_d((double*)nullptr, RELAX_SD * B);
  r->frac_eval = take_d((double*)nullptr, 3 * N);
  r->lat_eval = take_d((double*)nullptr, 9 * B);
  r->frac_next = take_d((double*)nullptr, 3 * N);
  r->lat_next = take_d((double*)nullptr, 9 * B);
  r->si = take_d((int*)nullptr, RELAX_SI * B);
  r->d_aoff = take_d((int*)nullptr, B + 1);
  r->d_orig = take_d((int*)nullptr, B);
  r->d_sel = take_d((int*)nullptr, B);
  r->status_next = take_d((int*)nullptr, B);
  r->retry = take_d((int*)nullptr, B);
  r->e_out = take_d((float*)nullptr, B);
  r->f_out = take_d((float*)nullptr, 3 * N);
  r->s_out = take_d((float*)nullptr, 9 * B);
  r->m_out = take_d((float*)nullptr, N);
}

struct Bump {   // offsets inside one allocation, 256-byte aligned
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

int check_params(chg_engine* eng, const chg_relax_params* p) {
  const char* bad = nullptr;
  if (!(p->fmax >= 0.0)) bad = "fmax must be >= 0";
  else if (p->max_steps < 0) bad = "max_steps must be >= 0";
  else if (!(p->dt > 0.0) || !(p->maxstep > 0.0) || !(p->dtmax > 0.0)) bad = "dt, maxstep and dtmax must be > 0";
  else if (!(p->finc > 0.0) || !(p->fdec > 0.0) || !(p->astart >= 0.0) || !(p->fa > 0.0)) bad = "finc, fdec, fa must be > 0 and astart >= 0";
  else if (!(p->r_atom > 0.0) || !(p->r_bond > 0.0)) bad = "graph cutoffs must be > 0";
  if (bad) { eng->err = std::string("chg_relax_create: ") + bad; return CHG_EINVAL; }
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
  const double* L0 = h->lattice + 9 * (size_t)o;
  double* qo = q + 3 * ((size_t)a0 + 3 * (size_t)o);
  for (int i = 0; i < n; ++i)            // u = r F^-T = r at F = I
    for (int j = 0; j < 3; ++j) {
      const double* f = h->frac + 3 * ((size_t)a0 + i);
      qo[3 * i + j] = f[0] * L0[j] + f[1] * L0[3 + j] + f[2] * L0[6 + j];
    }
  for (int i = 0; i < 9; ++i) qo[3 * n + i] = 0.0;   // X = c log F = 0
  for (int i = 0; i < 9; ++i) sd[i] = L0[i];
  inv3h(L0, sd + 9);
  sd[18] = p->exp_cell_factor > 0.0 ? p->exp_cell_factor : (double)n;
  sd[19] = p->dt;
  sd[20] = p->astart;
  sd[21] = sd[22] = sd[23] = 0.0;
  si[0] = si[1] = si[2] = si[3] = 0;
}

void launch_step(chg_engine* eng, const RelaxStepArgs& a, int grid) {
  LaunchScope ls(eng, "relax_step");
  hipLaunchKernelGGL(k_relax_step, dim3((unsigned)grid), dim3(256), 0, eng->stream, a);
}

}  // namespace

extern "C" {

int chg_relax_create(chg_engine* eng, const chg_structs_host* h, const chg_relax_params* params, chg_relax** out) {
  if (!eng || !h || !params || !out) return CHG_EINVAL;
  *out = nullptr;
  TRY(check_params(eng, params));
  const int B = h->n_struct, N = h->n_atoms;
  if (B <= 0 || N <= 0 || !h->z || !h->frac || !h->lattice || !h->atom_off) { eng->err = "chg_relax_create: empty or null structures"; return CHG_EINVAL; }
  if (h->atom_off[0] != 0 || h->atom_off[B] != N) { eng->err = "chg_relax_create: atom_off must run from 0 to n_atoms"; return CHG_EINVAL; }
  for (int o = 0; o < B; ++o)
    if (h->atom_off[o + 1] <= h->atom_off[o]) { eng->err = "chg_relax_create: every structure needs at least one atom"; return CHG_EINVAL; }
  HIP_TRY(eng, hipSetDevice(eng->device));
  chg_relax* r = new chg_relax();
  r->B = B; r->N = N; r->p = *params;
  r->z.assign(h->z, h->z + N);
  r->aoff.assign(h->atom_off, h->atom_off + B + 1);
  Bump sizer{nullptr};
  carve_relax(r, sizer);
  const size_t dbytes = sizer.pos;
  if (hipMalloc(&r->d_mem, dbytes) != hipSuccess) {
    (void)hipGetLastError();
    delete r;
    eng->err = "chg_relax_create: device state of " + std::to_string(dbytes) + " bytes cannot be allocated";
    return CHG_ENOMEM;
  }
  Bump carver{r->d_mem};
  carve_relax(r, carver);
  const size_t hbytes = sizeof(double) * (3 * (size_t)N + 9 * (size_t)B) + sizeof(int) * ((size_t)N + 5 * (size_t)B + 1) + 1024;
  if (hipHostMalloc(&r->h_mem, hbytes, hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    hipFree(r->d_mem);
    delete r;
    eng->err = "chg_relax_create: pinned staging cannot be allocated";
    return CHG_ENOMEM;
  }
  char* hp = r->h_mem;
  auto take_h = [&](size_t bytes) { char* x = hp; hp += (bytes + 7) & ~size_t(7); return x; };
  r->h_frac = (double*)take_h(sizeof(double) * 3 * N);
  r->h_lat = (double*)take_h(sizeof(double) * 9 * B);
  r->h_z = (int*)take_h(sizeof(int) * N);
  r->h_aoff = (int*)take_h(sizeof(int) * (B + 1));
  r->h_orig = (int*)take_h(sizeof(int) * B);
  r->h_status = (int*)take_h(sizeof(int) * B);
  r->h_retry = (int*)take_h(sizeof(int) * B);
  r->h_sel = (int*)take_h(sizeof(int) * B);
  // initial state on the host, one upload
  std::vector<double> q(3 * ((size_t)N + 3 * (size_t)B)), sd((size_t)RELAX_SD * B);
  std::vector<int> si((size_t)RELAX_SI * B);
  for (int o = 0; o < B; ++o) init_state(h, params, o, q.data(), sd.data() + (size_t)RELAX_SD * o, si.data() + (size_t)RELAX_SI * o);
  std::memcpy(r->h_frac, h->frac, sizeof(double) * 3 * N);     // the first build evaluates the structures exactly as given
  std::memcpy(r->h_lat, h->lattice, sizeof(double) * 9 * B);
  std::memcpy(r->h_z, h->z, sizeof(int) * N);
  std::memcpy(r->h_aoff, h->atom_off, sizeof(int) * (B + 1));
  for (int o = 0; o < B; ++o) r->h_orig[o] = o;
  r->n_active = B;
  int s = CHG_OK;
  auto up = [&](void* dst, const void* src, size_t bytes) {
    if (s == CHG_OK && hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, eng->stream) != hipSuccess) {
      eng->err = "chg_relax_create: state upload failed"; s = CHG_EHIP;
    }
  };
  up(r->q, q.data(), sizeof(double) * q.size());
  up(r->sd, sd.data(), sizeof(double) * sd.size());
  up(r->si, si.data(), sizeof(int) * si.size());
  up(r->d_aoff, h->atom_off, sizeof(int) * (B + 1));
  if (s == CHG_OK && (hipMemsetAsync(r->v, 0, sizeof(double) * 3 * ((size_t)N + 3 * (size_t)B), eng->stream) != hipSuccess ||
                      hipMemsetAsync(r->e_out, 0, sizeof(float) * B, eng->stream) != hipSuccess ||
                      hipMemsetAsync(r->f_out, 0, sizeof(float) * 3 * (size_t)N, eng->stream) != hipSuccess ||
                      hipMemsetAsync(r->s_out, 0, sizeof(float) * 9 * (size_t)B, eng->stream) != hipSuccess ||
                      hipMemsetAsync(r->m_out, 0, sizeof(float) * N, eng->stream) != hipSuccess ||
                      hipMemsetAsync(r->frac_eval, 0, sizeof(double) * 3 * (size_t)N, eng->stream) != hipSuccess ||
                      hipMemsetAsync(r->lat_eval, 0, sizeof(double) * 9 * (size_t)B, eng->stream) != hipSuccess)) {
    eng->err = "chg_relax_create: state initialisation failed"; s = CHG_EHIP;
  }
  if (s == CHG_OK && hipStreamSynchronize(eng->stream) != hipSuccess) { eng->err = "chg_relax_create: synchronisation failed"; s = CHG_EHIP; }
  if (s != CHG_OK) { chg_relax_free(eng, r); return s; }
  *out = r;
  return CHG_OK;
}

int chg_relax_run(chg_engine* eng, chg_relax* r, int32_t n_steps, int32_t* n_active) {
  if (!eng || !r || n_steps < 0) return CHG_EINVAL;
  HIP_TRY(eng, hipSetDevice(eng->device));
  hipStream_t st = eng->stream;
  const uint32_t task = CHG_TASK_E | CHG_TASK_F | CHG_TASK_S | CHG_TASK_M;
  RelaxStepArgs a = step_args(r->p, r->p.relax_cell);
  a.q = r->q; a.v = r->v; a.sd = r->sd; a.si = r->si; a.aoff = r->d_aoff;
  a.e_out = r->e_out; a.f_out = r->f_out; a.s_out = r->s_out; a.m_out = r->m_out; a.frac_eval = r->frac_eval; a.lat_eval = r->lat_eval;
  a.frac_next = r->frac_next; a.lat_next = r->lat_next; a.status_next = r->status_next; a.retry = r->retry;
  a.orig = r->d_orig;
  for (int it = 0; it < n_steps && r->n_active > 0; ++it) {
    const int Ba = r->n_active, Na = r->h_aoff[Ba];
    const chg_structs_host hs{Ba, Na, r->h_z, r->h_frac, r->h_lat, r->h_aoff};
    chg_batch* b = nullptr;
    int32_t counts[6];
    TRY(chg_batch_build_predict(eng, &hs, r->p.r_atom, r->p.r_bond, r->p.numerical_tol, task, &b, counts));
    auto fail = [&](int s) { chg_batch_free(eng, b); return s; };
    auto copy_back = [&]() -> int {
      if (hipMemcpyAsync(r->h_status, r->status_next, sizeof(int) * Ba, hipMemcpyDeviceToHost, st) != hipSuccess ||
          hipMemcpyAsync(r->h_retry, r->retry, sizeof(int) * Ba, hipMemcpyDeviceToHost, st) != hipSuccess ||
          hipMemcpyAsync(r->h_frac, r->frac_next, sizeof(double) * 3 * (size_t)Na, hipMemcpyDeviceToHost, st) != hipSuccess ||
          hipMemcpyAsync(r->h_lat, r->lat_next, sizeof(double) * 9 * (size_t)Ba, hipMemcpyDeviceToHost, st) != hipSuccess ||
          hipStreamSynchronize(st) != hipSuccess) {
        eng->err = "chg_relax_run: copy of the next configuration failed";
        return CHG_EHIP;
      }
      return CHG_OK;
    };
    a.energy = b->energy; a.force = b->force; a.stress = b->virial; a.magmom = b->magmom; a.b_atom_off = b->atom_off;
    a.sel = nullptr;
    a.final_try = b->wide_range ? 1 : 0;
    if (hipMemcpyAsync(r->d_orig, r->h_orig, sizeof(int) * Ba, hipMemcpyHostToDevice, st) != hipSuccess ||
        hipMemsetAsync(r->retry, 0, sizeof(int) * Ba, st) != hipSuccess) {
      eng->err = "chg_relax_run: index upload failed";
      return fail(CHG_EHIP);
    }
    launch_step(eng, a, Ba);
    if (hipGetLastError() != hipSuccess) { eng->err = "chg_relax_run: step kernel launch failed"; return fail(CHG_EHIP); }
    int s = copy_back();
    if (s != CHG_OK) return fail(s);
    // non-finite results: the batch is evaluated again on the wide-range sweep (chg_batch_download does the same) and only the
    // structures that were held back step; what is still non-finite there stops as NONFINITE
    int n_sel = 0;
    for (int i = 0; i < Ba; ++i)
      if (r->h_retry[i]) r->h_sel[n_sel++] = i;
    if (n_sel > 0) {
      b->wide_range = true;
      if (b->graph_exec) { hipGraphExecDestroy(b->graph_exec); b->graph_exec = nullptr; }
      s = chgh_wide::run_predict(eng, b, b->last_task ? b->last_task : task);
      if (s != CHG_OK) return fail(s);
      a.sel = r->d_sel;
      a.final_try = 1;
      if (hipMemcpyAsync(r->d_sel, r->h_sel, sizeof(int) * n_sel, hipMemcpyHostToDevice, st) != hipSuccess) {
        eng->err = "chg_relax_run: index upload failed";
        return fail(CHG_EHIP);
      }
      launch_step(eng, a, n_sel);
      if (hipGetLastError() != hipSuccess) { eng->err = "chg_relax_run: step kernel launch failed"; return fail(CHG_EHIP); }
      s = copy_back();
      if (s != CHG_OK) return fail(s);
    }
    TRY(chg_batch_free(eng, b));
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

int chg_relax_download(chg_engine* eng, chg_relax* r, const chg_relax_out_host* o) {
  if (!eng || !r || !o) return CHG_EINVAL;
  HIP_TRY(eng, hipSetDevice(eng->device));
  hipStream_t st = eng->stream;
  const size_t B = r->B, N = r->N;
  auto get = [&](void* dst, const void* src, size_t bytes) -> int {
    if (dst) HIP_TRY(eng, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, st));
    return CHG_OK;
  };
  TRY(get(o->frac, r->frac_eval, sizeof(double) * 3 * N));
  TRY(get(o->lattice, r->lat_eval, sizeof(double) * 9 * B));
  TRY(get(o->energy, r->e_out, sizeof(float) * B));
  TRY(get(o->force, r->f_out, sizeof(float) * 3 * N));
  TRY(get(o->stress, r->s_out, sizeof(float) * 9 * B));
  TRY(get(o->magmom, r->m_out, sizeof(float) * N));
  std::vector<int> si;
  if (o->n_steps || o->status) {
    si.resize((size_t)RELAX_SI * B);
    TRY(get(si.data(), r->si, sizeof(int) * si.size()));
  }
  HIP_TRY(eng, hipStreamSynchronize(st));
  for (size_t i = 0; i < B && !si.empty(); ++i) {
    if (o->n_steps) o->n_steps[i] = si[RELAX_SI * i + 1];
    if (o->status) o->status[i] = si[RELAX_SI * i + 2];
  }
  return CHG_OK;
}

int chg_relax_free(chg_engine* eng, chg_relax* r) {
  if (!r) return CHG_OK;
  if (eng) { hipSetDevice(eng->device); hipStreamSynchronize(eng->stream); }
  if (r->d_mem) hipFree(r->d_mem);
  if (r->h_mem) hipHostFree(r->h_mem);
  delete r;
  return CHG_OK;
}

int chg_test_relax_step(chg_engine* eng, const chg_relax_params* params, int32_t n_struct, const int32_t* atom_off, double* q, double* v,
                        double* sd, int32_t* si, const float* energy, const float* force, const float* stress, const float* magmom,
                        double* frac_next, double* lat_next) {
  if (!eng || !params || n_struct <= 0 || !atom_off || !q || !v || !sd || !si || !energy || !force || !stress || !frac_next || !lat_next)
    return CHG_EINVAL;
  const size_t B = n_struct, N = atom_off[n_struct], rows = N + 3 * B;
  if (atom_off[0] != 0) return CHG_EINVAL;
  for (size_t o = 0; o < B; ++o)
    if (atom_off[o + 1] <= atom_off[o]) return CHG_EINVAL;
  HIP_TRY(eng, hipSetDevice(eng->device));
  struct Buf { void* d; const void* h; size_t bytes; };
  Buf bufs[] = {{nullptr, q, sizeof(double) * 3 * rows}, {nullptr, v, sizeof(double) * 3 * rows}, {nullptr, sd, sizeof(double) * RELAX_SD * B},
                {nullptr, si, sizeof(int) * RELAX_SI * B}, {nullptr, atom_off, sizeof(int) * (B + 1)}, {nullptr, energy, sizeof(float) * B},
                {nullptr, force, sizeof(float) * 3 * N}, {nullptr, stress, sizeof(float) * 9 * B}, {nullptr, magmom, sizeof(float) * N},
                {nullptr, frac_next, sizeof(double) * 3 * N}, {nullptr, lat_next, sizeof(double) * 9 * B}, {nullptr, nullptr, sizeof(int) * B},
                {nullptr, nullptr, sizeof(int) * B}};
  int s = CHG_OK;
  for (Buf& x : bufs) {
    if (s == CHG_OK && hipMalloc(&x.d, x.bytes) != hipSuccess) { eng->err = "chg_test_relax_step: allocation failed"; s = CHG_ENOMEM; }
    if (s == CHG_OK && x.h && hipMemcpy(x.d, x.h, x.bytes, hipMemcpyHostToDevice) != hipSuccess) { eng->err = "chg_test_relax_step: upload failed"; s = CHG_EHIP; }
  }
  if (s == CHG_OK) {
    RelaxStepArgs a = step_args(*params, params->relax_cell);
    a.q = (double*)bufs[0].d; a.v = (double*)bufs[1].d; a.sd = (double*)bufs[2].d; a.si = (int*)bufs[3].d; a.aoff = (const int*)bufs[4].d;
    a.energy = (const float*)bufs[5].d; a.force = (const float*)bufs[6].d; a.stress = (const float*)bufs[7].d;
    a.magmom = magmom ? (const float*)bufs[8].d : nullptr; a.b_atom_off = (const int*)bufs[4].d;
    a.frac_next = (double*)bufs[9].d; a.lat_next = (double*)bufs[10].d; a.status_next = (int*)bufs[11].d; a.retry = (int*)bufs[12].d;
    a.final_try = 1;
    launch_step(eng, a, (int)B);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(eng->stream) != hipSuccess) { eng->err = "chg_test_relax_step: kernel failed"; s = CHG_EHIP; }
  }
  double* outs[] = {q, v, sd};
  for (int i = 0; i < 3 && s == CHG_OK; ++i)
    if (hipMemcpy(outs[i], bufs[i].d, bufs[i].bytes, hipMemcpyDeviceToHost) != hipSuccess) s = CHG_EHIP;
  if (s == CHG_OK && (hipMemcpy(si, bufs[3].d, bufs[3].bytes, hipMemcpyDeviceToHost) != hipSuccess ||
                      hipMemcpy(frac_next, bufs[9].d, bufs[9].bytes, hipMemcpyDeviceToHost) != hipSuccess ||
                      hipMemcpy(lat_next, bufs[10].d, bufs[10].bytes, hipMemcpyDeviceToHost) != hipSuccess)) {
    eng->err = "chg_test_relax_step: download failed"; s = CHG_EHIP;
  }
  for (Buf& x : bufs)
    if (x.d) hipFree(x.d);
  return s;
}

}  // extern "C"
