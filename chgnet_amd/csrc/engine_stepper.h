// engine_stepper.h -- host driver shared by the batched integrators behind the C-ABI: relaxation (engine_relax.hip, chg_relax_*) and
// molecular dynamics (engine_md.hip, chg_md_*).  Host code only; each integrator keeps its own translation unit and step kernel.
//
// Both keep their state in one device arena and stage the next configuration in pinned memory, because the device graph build takes
// its coordinates from the host.  One evaluation (evaluate_and_step):
//   chg_batch_build_predict on the staged structures
//   -> the integrator's step launch on all of them (sel = null, final_try = the batch already runs on the wide-range sweep)
//   -> one asynchronous copy of the retry flags and the next coordinates (plus the ints the caller names) into pinned memory, one
//      stream synchronisation
//   -> if a structure's results were non-finite: the batch is evaluated again on the wide-range sweep (chg_batch_download does the
//      same) and only the held-back structures step, with final_try = 1 (what is still non-finite there stops), copied back again.
#pragma once

#include "engine_internal.h"

#include "mat3.h"

namespace chgh {

// what relaxation and MD share: chg_relax and chg_md derive from it
struct Stepper {
  int B = 0, N = 0;
  uint32_t task = 0;                           // what each evaluation predicts
  double r_atom = 0.0, r_bond = 0.0, numerical_tol = 0.0;
  // device arena (carved by the integrator); the next configuration and the retry protocol are written by its step kernel
  char* d_mem = nullptr;
  double *frac_next = nullptr, *lat_next = nullptr;
  int *d_sel = nullptr, *retry = nullptr;
  // constraint (chg_relax_set_fixed / chg_md_set_fixed, DESIGN.md "Constraints"): the mask [N, 3] in original numbering and the free
  // components of every structure; the step kernels see them only while has_fixed
  unsigned char* d_fixed = nullptr;
  int* d_nfree = nullptr;
  bool has_fixed = false;
  // pinned staging: the configuration the next build evaluates (first n structures of h_aoff), retry flags, held-back structures,
  // and the integrator's own per-structure ints
  char* h_mem = nullptr;
  double *h_frac = nullptr, *h_lat = nullptr;
  int *h_z = nullptr, *h_aoff = nullptr, *h_retry = nullptr, *h_sel = nullptr, *h_extra = nullptr;
};

inline int check_structs(chg_engine* eng, const char* fn, const chg_structs_host* h) {
  const int B = h->n_struct, N = h->n_atoms;
  const char* bad = nullptr;
  if (B <= 0 || N <= 0 || !h->z || !h->frac || !h->lattice || !h->atom_off) bad = "empty or null structures";
  else if (h->atom_off[0] != 0 || h->atom_off[B] != N) bad = "atom_off must run from 0 to n_atoms";
  else
    for (int o = 0; o < B && !bad; ++o)
      if (h->atom_off[o + 1] <= h->atom_off[o]) bad = "every structure needs at least one atom";
  if (bad) { eng->err = std::string(fn) + ": " + bad; return CHG_EINVAL; }
  return CHG_OK;
}

// A mask [N, 3] (1 = component held) against the rules both integrators share: a partially held atom needs a cell that stays put, and
// a thermostat needs something to act on.  nfree [B]: free components per structure.
inline int check_fixed(chg_engine* eng, const char* fn, int B, const int* aoff, const uint8_t* fixed, bool moving_cell, bool needs_dof,
                       int* nfree) {
  for (int o = 0; o < B; ++o) {
    int held = 0;
    for (int i = aoff[o]; i < aoff[o + 1]; ++i) {
      const int h = (fixed[3 * (size_t)i] ? 1 : 0) + (fixed[3 * (size_t)i + 1] ? 1 : 0) + (fixed[3 * (size_t)i + 2] ? 1 : 0);
      if (moving_cell && h != 0 && h != 3) {
        eng->err = std::string(fn) + ": structure " + std::to_string(o) + " holds only some components of atom " + std::to_string(i - aoff[o]) +
                   ", which has no meaning while the cell moves";
        return CHG_EINVAL;
      }
      held += h;
    }
    nfree[o] = 3 * (aoff[o + 1] - aoff[o]) - held;
    if (needs_dof && nfree[o] == 0) {
      eng->err = std::string(fn) + ": structure " + std::to_string(o) + " has no free component left for the thermostat";
      return CHG_EINVAL;
    }
  }
  return CHG_OK;
}

// chg_*_set_fixed after the checks: the mask and the counts into the arena (null: the handle is unconstrained again)
inline int upload_fixed(chg_engine* eng, const char* fn, Stepper* s, const uint8_t* fixed, const int* nfree) {
  s->has_fixed = false;
  if (!fixed) return CHG_OK;
  if (hipMemcpyAsync(s->d_fixed, fixed, 3 * (size_t)s->N, hipMemcpyHostToDevice, eng->stream) != hipSuccess ||
      hipMemcpyAsync(s->d_nfree, nfree, sizeof(int) * (size_t)s->B, hipMemcpyHostToDevice, eng->stream) != hipSuccess ||
      hipStreamSynchronize(eng->stream) != hipSuccess) {
    eng->err = std::string(fn) + ": mask upload failed";
    return CHG_EHIP;
  }
  s->has_fixed = true;
  return CHG_OK;
}

// The device arena (carve(Carver&) places the integrator's arrays: called once to size it, once to place them) and the pinned staging
// with `extra` ints per structure, holding the structures exactly as given: the first build evaluates them.  On failure the caller
// releases what was allocated.
template <class Carve>
int alloc_state(chg_engine* eng, const char* fn, Stepper* s, const chg_structs_host* h, int extra, Carve&& carve) {
  const size_t B = h->n_struct, N = h->n_atoms;
  s->B = (int)B; s->N = (int)N;
  TRY(alloc_block(eng, fn, "device state", carve, &s->d_mem));
  const size_t hbytes = sizeof(double) * (3 * N + 9 * B) + sizeof(int) * (N + (3 + extra) * B + 1) + 1024;
  if (hipHostMalloc(&s->h_mem, hbytes, hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    s->h_mem = nullptr;
    eng->err = std::string(fn) + ": pinned staging cannot be allocated";
    return CHG_ENOMEM;
  }
  char* hp = s->h_mem;
  auto take_h = [&](size_t bytes) { char* x = hp; hp += (bytes + 7) & ~size_t(7); return x; };
  s->h_frac = (double*)take_h(sizeof(double) * 3 * N);
  s->h_lat = (double*)take_h(sizeof(double) * 9 * B);
  s->h_z = (int*)take_h(sizeof(int) * N);
  s->h_aoff = (int*)take_h(sizeof(int) * (B + 1));
  s->h_retry = (int*)take_h(sizeof(int) * B);
  s->h_sel = (int*)take_h(sizeof(int) * B);
  s->h_extra = (int*)take_h(sizeof(int) * extra * B);
  std::memcpy(s->h_frac, h->frac, sizeof(double) * 3 * N);
  std::memcpy(s->h_lat, h->lattice, sizeof(double) * 9 * B);
  std::memcpy(s->h_z, h->z, sizeof(int) * N);
  std::memcpy(s->h_aoff, h->atom_off, sizeof(int) * (B + 1));
  return CHG_OK;
}

// initial geometry of structure o: cartesian positions frac . L into r (its rows), the cell L and L^-1 into sd[0..18)
inline void initial_geometry(const chg_structs_host* h, int o, double* r, double* sd) {
  const int a0 = h->atom_off[o], n = h->atom_off[o + 1] - a0;
  const double* L = h->lattice + 9 * (size_t)o;
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < 3; ++j) {
      const double* f = h->frac + 3 * ((size_t)a0 + i);
      r[3 * i + j] = f[0] * L[j] + f[1] * L[3 + j] + f[2] * L[6 + j];
    }
  for (int i = 0; i < 9; ++i) sd[i] = L[i];
  chg::inv3(L, sd + 9);
}

// the initial state's host-to-device copies and memsets in *_create; the first failure is kept, finish() waits for them
struct StateUpload {
  chg_engine* eng;
  const char* fn;
  int s = CHG_OK;
  void operator()(void* dst, const void* src, size_t bytes) {
    if (s == CHG_OK && hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, eng->stream) != hipSuccess) fail("state upload failed");
  }
  void zero(void* dst, size_t bytes) {
    if (s == CHG_OK && hipMemsetAsync(dst, 0, bytes, eng->stream) != hipSuccess) fail("state initialisation failed");
  }
  int finish() {
    if (s == CHG_OK && hipStreamSynchronize(eng->stream) != hipSuccess) fail("synchronisation failed");
    return s;
  }
  void fail(const char* what) { eng->err = std::string(fn) + ": " + what; s = CHG_EHIP; }
};

inline void release(chg_engine* eng, Stepper* s) {
  if (eng) { hipSetDevice(eng->device); hipStreamSynchronize(eng->stream); }
  if (s->d_mem) hipFree(s->d_mem);
  if (s->h_mem) hipHostFree(s->h_mem);
}

// the retry flags and the next configuration of the first nb structures (and d_ints -> h_ints when named) into pinned memory, then wait
inline int copy_back(chg_engine* eng, const char* fn, Stepper* s, int nb, const int* d_ints, int* h_ints) {
  hipStream_t st = eng->stream;
  if ((d_ints && hipMemcpyAsync(h_ints, d_ints, sizeof(int) * nb, hipMemcpyDeviceToHost, st) != hipSuccess) ||
      hipMemcpyAsync(s->h_retry, s->retry, sizeof(int) * nb, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipMemcpyAsync(s->h_frac, s->frac_next, sizeof(double) * 3 * (size_t)s->h_aoff[nb], hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipMemcpyAsync(s->h_lat, s->lat_next, sizeof(double) * 9 * (size_t)nb, hipMemcpyDeviceToHost, st) != hipSuccess ||
      hipStreamSynchronize(st) != hipSuccess) {
    eng->err = std::string(fn) + ": copy of the next configuration failed";
    return CHG_EHIP;
  }
  return CHG_OK;
}

// One evaluation of the first nb staged structures and the step that follows it (file comment).  launch(b, sel, final_try, grid)
// enqueues the integrator's step kernel on the evaluated batch b: grid structures, sel null (all nb) or the held-back ones.
template <class Launch>
int evaluate_and_step(chg_engine* eng, const char* fn, Stepper* s, int nb, const int* d_ints, int* h_ints, Launch&& launch) {
  hipStream_t st = eng->stream;
  const chg_structs_host hs{nb, s->h_aoff[nb], s->h_z, s->h_frac, s->h_lat, s->h_aoff};
  chg_batch* b = nullptr;
  int32_t counts[6];
  TRY(chg_batch_build_predict(eng, &hs, s->r_atom, s->r_bond, s->numerical_tol, s->task, &b, counts));
  auto fail = [&](const char* what, int code) {
    if (what) eng->err = std::string(fn) + ": " + what;
    chg_batch_free(eng, b);
    return code;
  };
  auto step = [&](const int* sel, int final_try, int grid) {
    launch(b, sel, final_try, grid);
    if (hipGetLastError() != hipSuccess) return fail("step kernel launch failed", CHG_EHIP);
    const int rc = copy_back(eng, fn, s, nb, d_ints, h_ints);
    return rc == CHG_OK ? CHG_OK : fail(nullptr, rc);
  };
  if (hipMemsetAsync(s->retry, 0, sizeof(int) * nb, st) != hipSuccess) return fail("retry flag reset failed", CHG_EHIP);
  TRY(step(nullptr, b->wide_range ? 1 : 0, nb));
  int n_sel = 0;
  for (int i = 0; i < nb; ++i)
    if (s->h_retry[i]) s->h_sel[n_sel++] = i;
  if (n_sel > 0) {
    b->wide_range = true;
    if (b->graph_exec) { hipGraphExecDestroy(b->graph_exec); b->graph_exec = nullptr; }
    const int rc = chgh_wide::run_predict(eng, b, b->last_task ? b->last_task : s->task);
    if (rc != CHG_OK) return fail(nullptr, rc);
    if (hipMemcpyAsync(s->d_sel, s->h_sel, sizeof(int) * n_sel, hipMemcpyHostToDevice, st) != hipSuccess) return fail("index upload failed", CHG_EHIP);
    TRY(step(s->d_sel, 1, n_sel));
  }
  return chg_batch_free(eng, b);
}

// chg_test_*_step: every buffer to the device (in null: scratch), one launch, the buffers with an `out` back to the host
struct TestBuf {
  const void* in;
  void* out;
  size_t bytes;
  void* d = nullptr;
};

template <size_t K, class Launch>
int run_test_step(chg_engine* eng, const char* fn, TestBuf (&bufs)[K], Launch&& launch) {
  HIP_TRY(eng, hipSetDevice(eng->device));
  int s = CHG_OK;
  auto fail = [&](const char* what, int code) { eng->err = std::string(fn) + ": " + what; s = code; };
  for (TestBuf& x : bufs) {
    if (s == CHG_OK && hipMalloc(&x.d, x.bytes) != hipSuccess) fail("allocation failed", CHG_ENOMEM);
    if (s == CHG_OK && x.in && hipMemcpy(x.d, x.in, x.bytes, hipMemcpyHostToDevice) != hipSuccess) fail("upload failed", CHG_EHIP);
  }
  if (s == CHG_OK) {
    launch();
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(eng->stream) != hipSuccess) fail("kernel failed", CHG_EHIP);
  }
  for (TestBuf& x : bufs)
    if (s == CHG_OK && x.out && hipMemcpy(x.out, x.d, x.bytes, hipMemcpyDeviceToHost) != hipSuccess) fail("download failed", CHG_EHIP);
  for (TestBuf& x : bufs)
    if (x.d) hipFree(x.d);
  return s;
}

}  // namespace chgh
