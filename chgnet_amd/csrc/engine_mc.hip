// engine_mc.hip -- batched canonical Monte Carlo (chg_mc_*): species swaps and single-atom displacements with the Metropolis rule, one
// independent replica per structure at its own temperature, fixed cells, state in HBM (kernels_mc.h).  Not in the reference.
//
// One trial of chg_mc_run is one evaluate_and_step of the shared driver (engine_stepper.h) on ALL replicas: graph build on the device,
// energy-only prediction (CHG_TASK_E: forward sweep, no reverse sweep), then k_mc_step as the step launch (one workgroup per replica:
// decide the pending trial, frame, propose the next one).  Every replica runs the same number of trials, so there is no compaction.
//
// Replica exchange (chg_mc_set_exchange, kernels_mc_exchange.h): on a trial that ends with an exchange event the step launch only
// decides, k_mc_exchange swaps the configurations of the accepted pairs, and a propose-only launch draws the next trial from what the
// rungs hold now.  A handle without a ladder launches exactly what it launched before.
#include "engine_stepper.h"

#include "kernels_mc.h"
#include "kernels_mc_exchange.h"

struct chg_mc : chgh::Stepper {
  chg_mc_params p{};
  bool started = false;   // the initial configuration has been evaluated (frame 0 written)
  int trials = 0;         // trials decided (all replicas; a NONFINITE replica stops counting)
  // device state
  double *r, *sd, *temp, *best_pos;
  int *site, *si, *best_site, *d_aoff, *mov, *swp, *gstart, *gsize, *n_mov, *n_swp;
  long long* sl;
  unsigned long long* seeds;
  // frame ring: K slots
  int K = 0, ring_head = 0, ring_count = 0;
  std::vector<int> ring_trial;
  std::vector<chg::McFrame> ring;
  // replica exchange (chg_mc_set_exchange): what a ladder's members must share, kept from creation, and an allocation of its own
  std::vector<uint8_t> h_fixed, h_swap_mask;   // [N] as given (null: none held, all may swap)
  std::vector<double> h_temp;                  // [B] the temperatures in force
  std::vector<int> ladder;                     // [B] empty: no ladder set
  int x_interval = 0;                          // an event after every x_interval-th trial; 0: none
  char* x_mem = nullptr;                       // xi [B, MC_XI], then the pair lists of the two parities
  int* xi = nullptr;
  int* x_pairs[2] = {nullptr, nullptr};
  int x_npairs[2] = {0, 0};
};

namespace {

// the atom lists of every replica (kernels_mc.h McStepArgs), entries of replica o at aoff[o]
struct McLists {
  std::vector<int> mov, swp, gstart, gsize, n_mov, n_swp;
};

const char* bad_params(const chg_mc_params* p) {
  if (!(p->swap_probability >= 0.0) || !(p->swap_probability <= 1.0)) return "swap_probability must be in [0, 1]";
  if (!(p->max_displacement >= 0.0) || !std::isfinite(p->max_displacement)) return "max_displacement must be >= 0 and finite";
  if (p->loginterval < 0 || p->ring_frames < 0) return "loginterval and ring_frames must be >= 0";
  if (p->loginterval > 0 && p->ring_frames < 1) return "frames need ring_frames >= 1";
  if (!(p->r_atom > 0.0) || !(p->r_bond > 0.0)) return "graph cutoffs must be > 0";
  return nullptr;
}

int check_temperatures(chg_engine* eng, const char* fn, int B, const double* temperatures) {
  for (int o = 0; o < B; ++o)
    if (!(temperatures[o] >= 0.0) || !std::isfinite(temperatures[o])) {
      eng->err = std::string(fn) + ": the temperature of structure " + std::to_string(o) + " must be >= 0 and finite";
      return CHG_EINVAL;
    }
  return CHG_OK;
}

// movable: atoms not held, in atom order.  swappable: movable atoms whose swap_mask is set (null: all), sorted by (species, atom), with
// the start and the size of its species group beside every entry.  Refuses a replica that could not make the moves it may draw.
int build_lists(chg_engine* eng, const char* fn, int B, const int* aoff, const int* z, const uint8_t* swap_mask, const uint8_t* fixed,
                double swap_probability, McLists& l) {
  const size_t N = aoff[B];
  l.mov.assign(N, 0); l.swp.assign(N, 0); l.gstart.assign(N, 0); l.gsize.assign(N, 0);
  l.n_mov.assign(B, 0); l.n_swp.assign(B, 0);
  for (int o = 0; o < B; ++o) {
    const int a0 = aoff[o], n = aoff[o + 1] - a0;
    int nm = 0, ns = 0, groups = 0;
    for (int i = 0; i < n; ++i)
      if (!(fixed && fixed[a0 + i])) {
        l.mov[a0 + nm++] = i;
        if (!swap_mask || swap_mask[a0 + i]) l.swp[a0 + ns++] = i;
      }
    int* s = l.swp.data() + a0;
    std::stable_sort(s, s + ns, [&](int x, int y) { return z[a0 + x] < z[a0 + y]; });   // atom order is kept inside a species
    for (int t = 0; t < ns;) {
      int e = t;
      while (e < ns && z[a0 + s[e]] == z[a0 + s[t]]) ++e;
      for (int u = t; u < e; ++u) { l.gstart[a0 + u] = t; l.gsize[a0 + u] = e - t; }
      groups += 1;
      t = e;
    }
    l.n_mov[o] = nm; l.n_swp[o] = ns;
    if (swap_probability > 0.0 && groups < 2) {
      eng->err = std::string(fn) + ": structure " + std::to_string(o) + " has " + std::to_string(groups) +
                 " swappable species among its free atoms, a swap needs two";
      return CHG_EINVAL;
    }
    if (swap_probability < 1.0 && nm == 0) {
      eng->err = std::string(fn) + ": structure " + std::to_string(o) + " has no free atom to displace";
      return CHG_EINVAL;
    }
  }
  return CHG_OK;
}

McFrame carve_frame(Carver& c, size_t B, size_t N) {
  McFrame f{};
  f.scal = c.take<double>(MC_FRAME_SCAL * B);
  f.pos = c.take<double>(3 * N);
  f.ints = c.take<int>(MC_FRAME_INT * B);
  f.site = c.take<int>(N);
  return f;
}

void carve_mc(chg_mc* d, Carver& c) {
  const size_t B = d->B, N = d->N;
  d->r = c.take<double>(3 * N);
  d->sd = c.take<double>(MC_SD * B);
  d->temp = c.take<double>(B);
  d->best_pos = c.take<double>(3 * N);
  d->frac_next = c.take<double>(3 * N);
  d->lat_next = c.take<double>(9 * B);
  d->site = c.take<int>(N);
  d->best_site = c.take<int>(N);
  d->si = c.take<int>(MC_SI * B);
  d->sl = c.take<long long>(MC_SL * B);
  d->seeds = c.take<unsigned long long>(B);
  d->d_aoff = c.take<int>(B + 1);
  d->mov = c.take<int>(N);
  d->swp = c.take<int>(N);
  d->gstart = c.take<int>(N);
  d->gsize = c.take<int>(N);
  d->n_mov = c.take<int>(B);
  d->n_swp = c.take<int>(B);
  d->d_sel = c.take<int>(B);
  d->retry = c.take<int>(B);
  d->ring.resize(d->K);
  for (McFrame& f : d->ring) f = carve_frame(c, B, N);
}

// what the parameters decide; the device pointers are the caller's
McStepArgs base_args(const chg_mc_params& p, int intensive, int flags) {
  McStepArgs a{};
  a.swap_probability = p.swap_probability; a.max_displacement = p.max_displacement; a.kB = p.kB > 0.0 ? p.kB : 8.6173303e-5;
  a.flags = flags; a.intensive = intensive;
  return a;
}

McStepArgs handle_args(chg_engine* eng, chg_mc* d, int flags) {
  McStepArgs a = base_args(d->p, eng->desc.is_intensive ? 1 : 0, flags);
  a.r = d->r; a.site = d->site; a.sd = d->sd; a.si = d->si; a.sl = d->sl; a.best_pos = d->best_pos; a.best_site = d->best_site;
  a.temp = d->temp; a.seeds = d->seeds; a.aoff = d->d_aoff;
  a.mov = d->mov; a.swp = d->swp; a.gstart = d->gstart; a.gsize = d->gsize; a.n_mov = d->n_mov; a.n_swp = d->n_swp;
  a.frac_next = d->frac_next; a.retry = d->retry;
  return a;
}

void launch_step(chg_engine* eng, const McStepArgs& a, int grid) {
  LaunchScope ls(eng, "mc_step");
  hipLaunchKernelGGL(k_mc_step, dim3((unsigned)grid), dim3(256), 0, eng->stream, a);
}

// evaluate all replicas, then one step launch with `a` (flags and frame slot set by the caller)
int evaluate_and_step(chg_engine* eng, chg_mc* d, McStepArgs a) {
  return chgh::evaluate_and_step(eng, "chg_mc_run", d, d->B, nullptr, nullptr, [&](const chg_batch* b, const int* sel, int final_try, int grid) {
    a.energy = b->energy;
    a.sel = sel;
    a.final_try = final_try;
    launch_step(eng, a, grid);
  });
}

bool frame_due(const chg_mc* d, int trial) { return d->p.loginterval > 0 && trial % d->p.loginterval == 0; }

// frame slot for the decision that makes `trial` trials (the caller checked that the ring has room)
void set_frame(chg_mc* d, McStepArgs& a, int trial) {
  const size_t slot = (size_t)((d->ring_head + d->ring_count) % d->K);
  a.fr = d->ring[slot];
  d->ring_trial[slot] = trial;
  d->ring_count += 1;
}

// ---- replica exchange
// The pairs of the two parities, MC_PAIR_INTS ints each (kernels_mc_exchange.h): list[q] holds the rungs (p, p + 1) with p % 2 == q.
struct McPairs {
  std::vector<int> list[2];
};

// The ladders of `ladder` [B] (-1: never exchanged) against what the pair lists alone need: ids >= -1, the members of an id consecutive,
// at least two of them, the same atom count, T > 0.  Fills the two pair lists.
int build_pairs(chg_engine* eng, const char* fn, int B, const int* aoff, const int* ladder, const double* temperatures, McPairs& out) {
  auto refuse = [&](int o, const std::string& what) {
    eng->err = std::string(fn) + ": replica " + std::to_string(o) + " " + what;
    return CHG_EINVAL;
  };
  out.list[0].clear(); out.list[1].clear();
  std::vector<int> closed;   // ids whose run has ended
  for (int first = 0; first < B;) {
    const int id = ladder[first];
    if (id < -1) return refuse(first, "has the ladder id " + std::to_string(id) + ", which must be -1 or >= 0");
    if (id == -1) { first += 1; continue; }
    if (std::find(closed.begin(), closed.end(), id) != closed.end())
      return refuse(first, "takes up ladder " + std::to_string(id) + " again after another id: the members of a ladder must be consecutive");
    int end = first + 1;
    while (end < B && ladder[end] == id) ++end;
    const int L = end - first;
    if (L < 2) return refuse(first, "is the only member of ladder " + std::to_string(id) + ": a ladder needs at least two");
    for (int o = first; o < end; ++o) {
      if (aoff[o + 1] - aoff[o] != aoff[first + 1] - aoff[first])
        return refuse(o, "has " + std::to_string(aoff[o + 1] - aoff[o]) + " atoms, the first member of ladder " + std::to_string(id) + " has " +
                             std::to_string(aoff[first + 1] - aoff[first]));
      if (!(temperatures[o] > 0.0) || !std::isfinite(temperatures[o]))
        return refuse(o, "of ladder " + std::to_string(id) + " needs a temperature > 0: an exchange divides by it");
    }
    for (int p = 0; p + 1 < L; ++p) {
      std::vector<int>& l = out.list[p & 1];
      l.push_back(first + p); l.push_back(first); l.push_back(L);
    }
    closed.push_back(id);
    first = end;
  }
  return CHG_OK;
}

// rung index as walker, walker 0 of every ladder marked as seen at the bottom
std::vector<int> initial_xi(int B, const int* ladder) {
  std::vector<int> xi((size_t)MC_XI * B, 0);
  for (int o = 0, first = 0; o < B; ++o) {
    if (ladder[o] < 0) continue;
    if (o == 0 || ladder[o - 1] != ladder[o]) first = o;
    xi[(size_t)MC_XI * o + MC_X_WALKER] = o - first;
    if (o == first) xi[(size_t)MC_XI * o + MC_X_MARK] = MC_MARK_BOTTOM;
  }
  return xi;
}

void launch_exchange(chg_engine* eng, const McExchangeArgs& x, int grid) {
  LaunchScope ls(eng, "mc_exchange");
  hipLaunchKernelGGL(k_mc_exchange, dim3((unsigned)grid), dim3(256), 0, eng->stream, x);
}

void free_exchange(chg_mc* d) {
  if (d->x_mem) hipFree(d->x_mem);
  d->x_mem = nullptr; d->xi = nullptr; d->x_pairs[0] = d->x_pairs[1] = nullptr; d->x_npairs[0] = d->x_npairs[1] = 0;
  d->ladder.clear();
  d->x_interval = 0;
}

// exchange event m of the handle: the pairs of its parity, one workgroup each
int exchange_event(chg_engine* eng, chg_mc* d, int m) {
  const int q = (m - 1) & 1;
  if (d->x_npairs[q] == 0) return CHG_OK;   // a batch of two-rung ladders has no pair on the odd parity
  McExchangeArgs x{};
  x.r = d->r; x.site = d->site; x.sd = d->sd; x.si = d->si; x.best_pos = d->best_pos; x.best_site = d->best_site;
  x.temp = d->temp; x.seeds = d->seeds; x.aoff = d->d_aoff; x.xi = d->xi; x.pairs = d->x_pairs[q];
  x.kB = d->p.kB > 0.0 ? d->p.kB : 8.6173303e-5; x.m = (unsigned)m;
  launch_exchange(eng, x, d->x_npairs[q]);
  if (hipGetLastError() != hipSuccess) { eng->err = "chg_mc_run: exchange kernel launch failed"; return CHG_EHIP; }
  return CHG_OK;
}

// a later call's start, and what follows an exchange event: nothing is pending, propose from the current configuration
int propose_only(chg_engine* eng, chg_mc* d) {
  launch_step(eng, handle_args(eng, d, MC_PROPOSE), d->B);
  if (hipGetLastError() != hipSuccess) { eng->err = "chg_mc_run: step kernel launch failed"; return CHG_EHIP; }
  return copy_back(eng, "chg_mc_run", d, d->B, nullptr, nullptr);
}

}  // namespace

extern "C" {

int chg_mc_create(chg_engine* eng, const chg_structs_host* h, const double* temperatures, const uint64_t* seeds, const uint8_t* swap_mask,
                  const uint8_t* fixed, const chg_mc_params* params, chg_mc** out) {
  if (!eng || !h || !temperatures || !seeds || !params || !out) return CHG_EINVAL;
  const char* fn = "chg_mc_create";
  *out = nullptr;
  if (const char* bad = bad_params(params)) { eng->err = std::string(fn) + ": " + bad; return CHG_EINVAL; }
  TRY(check_structs(eng, fn, h));
  const int B = h->n_struct, N = h->n_atoms;
  TRY(check_temperatures(eng, fn, B, temperatures));
  McLists lists;
  TRY(build_lists(eng, fn, B, h->atom_off, h->z, swap_mask, fixed, params->swap_probability, lists));
  HIP_TRY(eng, hipSetDevice(eng->device));
  chg_mc* d = new chg_mc();
  d->p = *params;
  d->K = params->loginterval > 0 ? params->ring_frames : 0;
  d->ring_trial.assign(std::max(d->K, 1), 0);
  d->task = CHG_TASK_E;
  d->r_atom = params->r_atom; d->r_bond = params->r_bond; d->numerical_tol = params->numerical_tol;
  d->h_temp.assign(temperatures, temperatures + B);
  d->h_fixed.assign(N, 0); d->h_swap_mask.assign(N, 1);
  for (int i = 0; i < N; ++i) {
    if (fixed) d->h_fixed[i] = fixed[i] ? 1 : 0;
    if (swap_mask) d->h_swap_mask[i] = swap_mask[i] ? 1 : 0;
  }
  int s = alloc_state(eng, fn, d, h, 0, [&](Carver& c) { carve_mc(d, c); });
  if (s != CHG_OK) { chg_mc_free(eng, d); return s; }
  // initial state on the host, one upload: cartesian positions frac . L, the cell and its inverse, site[] the identity
  std::vector<double> r(3 * (size_t)N), sd((size_t)MC_SD * B, 0.0);
  std::vector<int> si((size_t)MC_SI * B, 0), site(N);
  for (int o = 0; o < B; ++o) {
    initial_geometry(h, o, r.data() + 3 * (size_t)h->atom_off[o], sd.data() + (size_t)MC_SD * o);
    si[(size_t)MC_SI * o + 3] = MC_NONE;
    for (int i = h->atom_off[o]; i < h->atom_off[o + 1]; ++i) site[i] = i - h->atom_off[o];
  }
  StateUpload up{eng, fn};
  up(d->r, r.data(), sizeof(double) * r.size());
  up(d->best_pos, r.data(), sizeof(double) * r.size());
  up(d->sd, sd.data(), sizeof(double) * sd.size());
  up(d->temp, temperatures, sizeof(double) * B);
  up(d->site, site.data(), sizeof(int) * N);
  up(d->best_site, site.data(), sizeof(int) * N);
  up(d->si, si.data(), sizeof(int) * si.size());
  up.zero(d->sl, sizeof(long long) * MC_SL * (size_t)B);
  up(d->seeds, seeds, sizeof(uint64_t) * B);
  up(d->d_aoff, h->atom_off, sizeof(int) * (B + 1));
  up(d->mov, lists.mov.data(), sizeof(int) * N);
  up(d->swp, lists.swp.data(), sizeof(int) * N);
  up(d->gstart, lists.gstart.data(), sizeof(int) * N);
  up(d->gsize, lists.gsize.data(), sizeof(int) * N);
  up(d->n_mov, lists.n_mov.data(), sizeof(int) * B);
  up(d->n_swp, lists.n_swp.data(), sizeof(int) * B);
  up(d->frac_next, h->frac, sizeof(double) * 3 * N);
  up(d->lat_next, h->lattice, sizeof(double) * 9 * B);   // the cell never moves: the step kernel leaves it alone
  if ((s = up.finish()) != CHG_OK) { chg_mc_free(eng, d); return s; }
  *out = d;
  return CHG_OK;
}

int chg_mc_set_temperatures(chg_engine* eng, chg_mc* d, const double* temperatures) {
  if (!eng || !d || !temperatures) return CHG_EINVAL;
  TRY(check_temperatures(eng, "chg_mc_set_temperatures", d->B, temperatures));
  for (size_t o = 0; o < d->ladder.size(); ++o)
    if (d->ladder[o] >= 0 && !(temperatures[o] > 0.0)) {
      eng->err = "chg_mc_set_temperatures: replica " + std::to_string(o) + " of ladder " + std::to_string(d->ladder[o]) +
                 " needs a temperature > 0: an exchange divides by it";
      return CHG_EINVAL;
    }
  HIP_TRY(eng, hipSetDevice(eng->device));
  HIP_TRY(eng, hipMemcpyAsync(d->temp, temperatures, sizeof(double) * (size_t)d->B, hipMemcpyHostToDevice, eng->stream));
  HIP_TRY(eng, hipStreamSynchronize(eng->stream));
  d->h_temp.assign(temperatures, temperatures + d->B);
  return CHG_OK;
}

int chg_mc_set_exchange(chg_engine* eng, chg_mc* d, const int32_t* ladder, int32_t interval) {
  if (!eng || !d || !ladder) return CHG_EINVAL;
  const char* fn = "chg_mc_set_exchange";
  const int B = d->B;
  if (d->started) { eng->err = std::string(fn) + ": the ladders must be set before the handle's first chg_mc_run"; return CHG_EINVAL; }
  if (interval < 0) { eng->err = std::string(fn) + ": interval must be >= 0 (0: no exchanges)"; return CHG_EINVAL; }
  // nothing has run: the pinned staging still holds the structures as given
  McPairs pairs;
  TRY(build_pairs(eng, fn, B, d->h_aoff, ladder, d->h_temp.data(), pairs));
  for (int o = 1; o < B; ++o) {
    if (ladder[o] < 0 || ladder[o] != ladder[o - 1]) continue;
    const int a0 = d->h_aoff[o - 1], b0 = d->h_aoff[o], n = d->h_aoff[o + 1] - b0;
    const char* what = nullptr;
    if (std::memcmp(d->h_z + a0, d->h_z + b0, sizeof(int) * n) != 0) what = "species in another order than";
    else if (std::memcmp(d->h_lat + 9 * (size_t)(o - 1), d->h_lat + 9 * (size_t)o, sizeof(double) * 9) != 0) what = "another lattice than";
    else if (std::memcmp(d->h_fixed.data() + a0, d->h_fixed.data() + b0, n) != 0) what = "other held atoms (fixed) than";
    else if (std::memcmp(d->h_swap_mask.data() + a0, d->h_swap_mask.data() + b0, n) != 0) what = "another swap_mask than";
    if (what) {
      eng->err = std::string(fn) + ": replica " + std::to_string(o) + " has " + what + " replica " + std::to_string(o - 1) + " of ladder " +
                 std::to_string(ladder[o]) + ": the rungs of a ladder exchange whole configurations";
      return CHG_EINVAL;
    }
  }
  HIP_TRY(eng, hipSetDevice(eng->device));
  const std::vector<int> xi = initial_xi(B, ladder);
  const size_t n0 = pairs.list[0].size(), n1 = pairs.list[1].size();
  char* mem = nullptr;
  int *d_xi = nullptr, *d_p0 = nullptr, *d_p1 = nullptr;
  TRY(alloc_block(eng, fn, "exchange state", [&](Carver& c) { d_xi = c.take<int>(xi.size()); d_p0 = c.take<int>(n0); d_p1 = c.take<int>(n1); }, &mem));
  StateUpload up{eng, fn};
  up(d_xi, xi.data(), sizeof(int) * xi.size());
  if (n0) up(d_p0, pairs.list[0].data(), sizeof(int) * n0);
  if (n1) up(d_p1, pairs.list[1].data(), sizeof(int) * n1);
  const int s = up.finish();
  if (s != CHG_OK) { hipFree(mem); return s; }
  free_exchange(d);   // a ladder set before
  d->x_mem = mem; d->xi = d_xi; d->x_pairs[0] = d_p0; d->x_pairs[1] = d_p1;
  d->x_npairs[0] = (int)(n0 / MC_PAIR_INTS); d->x_npairs[1] = (int)(n1 / MC_PAIR_INTS);
  d->ladder.assign(ladder, ladder + B);
  d->x_interval = interval;
  return CHG_OK;
}

int chg_mc_download_exchange(chg_engine* eng, chg_mc* d, int32_t* xi) {
  if (!eng || !d || !xi) return CHG_EINVAL;
  if (!d->xi) { eng->err = "chg_mc_download_exchange: the handle has no ladder (chg_mc_set_exchange)"; return CHG_EINVAL; }
  HIP_TRY(eng, hipSetDevice(eng->device));
  TRY(d2h(eng, (int*)xi, (const int*)d->xi, (size_t)MC_XI * d->B));
  HIP_TRY(eng, hipStreamSynchronize(eng->stream));
  return CHG_OK;
}

int chg_mc_run(chg_engine* eng, chg_mc* d, int32_t n_trials) {
  if (!eng || !d || n_trials < 0) return CHG_EINVAL;
  if (n_trials > INT32_MAX - d->trials) { eng->err = "chg_mc_run: a handle counts at most 2^31 - 1 trials"; return CHG_EINVAL; }
  // the frames this call writes must fit the ring: refuse before anything runs
  int due = (!d->started && frame_due(d, 0)) ? 1 : 0;
  for (int k = 1; k <= n_trials; ++k) due += frame_due(d, d->trials + k) ? 1 : 0;
  if (due > d->K - d->ring_count) {
    eng->err = "chg_mc_run: " + std::to_string(due) + " frames do not fit the ring (" + std::to_string(d->K - d->ring_count) +
               " slots free): drain it with chg_mc_download or run fewer trials";
    return CHG_EINVAL;
  }
  HIP_TRY(eng, hipSetDevice(eng->device));
  if (!d->started) {   // evaluate the configuration as given: E_cur, the best record, frame 0, and the first proposal
    McStepArgs a = handle_args(eng, d, MC_ABSORB | (n_trials > 0 ? MC_PROPOSE : 0));
    if (frame_due(d, 0)) set_frame(d, a, 0);
    TRY(evaluate_and_step(eng, d, a));
    d->started = true;
  } else if (n_trials > 0) {   // a later call
    TRY(propose_only(eng, d));
  }
  for (int k = 0; k < n_trials; ++k) {
    const int next = d->trials + 1;
    // an exchange event belongs to the trial it follows: the decision alone, the event, then the proposal from what the rungs hold now
    const bool event = d->x_interval > 0 && next % d->x_interval == 0, more = k + 1 < n_trials;
    McStepArgs a = handle_args(eng, d, MC_ABSORB | (more && !event ? MC_PROPOSE : 0));
    if (frame_due(d, next)) set_frame(d, a, next);
    TRY(evaluate_and_step(eng, d, a));
    d->trials = next;
    if (event) {
      TRY(exchange_event(eng, d, next / d->x_interval));
      if (more) TRY(propose_only(eng, d));
    }
  }
  if (eng->profiling) return collect_profile(eng);
  return CHG_OK;
}

int chg_mc_download(chg_engine* eng, chg_mc* d, const chg_mc_out_host* o) {
  if (!eng || !d || !o) return CHG_EINVAL;
  HIP_TRY(eng, hipSetDevice(eng->device));
  const size_t B = d->B, N = d->N;
  TRY(d2h(eng, o->positions, d->r, 3 * N));
  TRY(d2h(eng, o->site, d->site, N));
  TRY(d2h(eng, o->best_positions, d->best_pos, 3 * N));
  TRY(d2h(eng, o->best_site, d->best_site, N));
  TRY(d2h(eng, (long long*)o->counts, d->sl, MC_SL * B));
  TRY(d2h(eng, o->temperatures, d->temp, B));
  std::vector<double> sd;
  std::vector<int> si;
  if (o->energy || o->best_energy || o->sums) { sd.resize((size_t)MC_SD * B); TRY(d2h(eng, sd.data(), d->sd, sd.size())); }
  if (o->status || o->n_trials) { si.resize((size_t)MC_SI * B); TRY(d2h(eng, si.data(), d->si, si.size())); }
  // frames, oldest first
  const int take = std::min(d->ring_count, std::max(o->frame_capacity, 0));
  for (int k = 0; k < take; ++k) {
    const size_t slot = (size_t)((d->ring_head + k) % std::max(d->K, 1));
    const McFrame& fr = d->ring[slot];
    if (o->frame_trial) o->frame_trial[k] = d->ring_trial[slot];
    TRY(d2h(eng, o->frame_scalars ? o->frame_scalars + k * MC_FRAME_SCAL * B : nullptr, fr.scal, MC_FRAME_SCAL * B));
    TRY(d2h(eng, o->frame_moves ? o->frame_moves + k * MC_FRAME_INT * B : nullptr, fr.ints, MC_FRAME_INT * B));
    TRY(d2h(eng, o->frame_positions ? o->frame_positions + k * 3 * N : nullptr, fr.pos, 3 * N));
    TRY(d2h(eng, o->frame_site ? o->frame_site + k * N : nullptr, fr.site, N));
  }
  HIP_TRY(eng, hipStreamSynchronize(eng->stream));
  d->ring_head = d->K > 0 ? (d->ring_head + take) % d->K : 0;
  d->ring_count -= take;
  if (o->n_frames) *o->n_frames = take;
  for (size_t i = 0; i < B; ++i) {
    if (o->energy) o->energy[i] = sd[MC_SD * i + MC_E_CUR];
    if (o->best_energy) o->best_energy[i] = sd[MC_SD * i + MC_E_BEST];
    if (o->sums) { o->sums[2 * i] = sd[MC_SD * i + MC_SUM_E]; o->sums[2 * i + 1] = sd[MC_SD * i + MC_SUM_E2]; }
    if (o->status) o->status[i] = si[MC_SI * i + 1];
    if (o->n_trials) o->n_trials[i] = si[MC_SI * i];
  }
  return CHG_OK;
}

int chg_mc_free(chg_engine* eng, chg_mc* d) {
  if (!d) return CHG_OK;
  release(eng, d);
  free_exchange(d);
  delete d;
  return CHG_OK;
}

int chg_test_mc_step(chg_engine* eng, const chg_mc_params* params, int32_t n_struct, const int32_t* atom_off, const int32_t* z,
                     const uint8_t* swap_mask, const uint8_t* fixed, const double* temperatures, const uint64_t* seeds, int32_t flags,
                     int32_t final_try, int32_t intensive, double* r, int32_t* site, double* sd, int32_t* si, int64_t* counts,
                     double* best_positions, int32_t* best_site, const float* energy, double* frac_next, int32_t* retry,
                     double* frame_scalars, int32_t* frame_moves, double* frame_positions, int32_t* frame_site) {
  if (!eng || !params || n_struct <= 0 || !atom_off || !z || !temperatures || !seeds || !r || !site || !sd || !si || !counts ||
      !best_positions || !best_site || !frac_next || !retry)
    return CHG_EINVAL;
  const char* fn = "chg_test_mc_step";
  if ((flags & MC_ABSORB) && !energy) return CHG_EINVAL;
  if (flags & ~(MC_ABSORB | MC_PROPOSE)) return CHG_EINVAL;
  const bool frame = frame_scalars != nullptr;
  if (frame && (!frame_moves || !frame_positions || !frame_site)) return CHG_EINVAL;
  if (const char* bad = bad_params(params)) { eng->err = std::string(fn) + ": " + bad; return CHG_EINVAL; }
  const size_t B = n_struct;
  if (atom_off[0] != 0) return CHG_EINVAL;
  for (size_t o = 0; o < B; ++o)
    if (atom_off[o + 1] <= atom_off[o]) return CHG_EINVAL;
  const size_t N = atom_off[n_struct];
  TRY(check_temperatures(eng, fn, n_struct, temperatures));
  McLists lists;
  TRY(build_lists(eng, fn, n_struct, atom_off, z, swap_mask, fixed, params->swap_probability, lists));
  for (size_t o = 0; o < B; ++o) {   // the pending move indexes the replica's rows
    const int n = atom_off[o + 1] - atom_off[o], kind = si[MC_SI * o + 3], i = si[MC_SI * o + 4], j = si[MC_SI * o + 5];
    if (kind < MC_NONE || kind > MC_DISPLACE) return CHG_EINVAL;
    if (kind != MC_NONE && (i < 0 || i >= n || (kind == MC_SWAP && (j < 0 || j >= n)))) return CHG_EINVAL;
  }
  std::vector<int> zero_retry(B, 0);   // the driver clears the flags before every evaluation
  enum { R, SITE, SD, SI, SL, BPOS, BSITE, TEMP, SEEDS, AOFF, MOV, SWP, GSTART, GSIZE, NMOV, NSWP, ENERGY, FRAC_NEXT, RETRY, FSCAL, FINT, FPOS,
         FSITE, N_BUFS };
  TestBuf bufs[N_BUFS];
  bufs[R] = {r, r, sizeof(double) * 3 * N};
  bufs[SITE] = {site, site, sizeof(int) * N};
  bufs[SD] = {sd, sd, sizeof(double) * MC_SD * B};
  bufs[SI] = {si, si, sizeof(int) * MC_SI * B};
  bufs[SL] = {counts, counts, sizeof(long long) * MC_SL * B};
  bufs[BPOS] = {best_positions, best_positions, sizeof(double) * 3 * N};
  bufs[BSITE] = {best_site, best_site, sizeof(int) * N};
  bufs[TEMP] = {temperatures, nullptr, sizeof(double) * B};
  bufs[SEEDS] = {seeds, nullptr, sizeof(uint64_t) * B};
  bufs[AOFF] = {atom_off, nullptr, sizeof(int) * (B + 1)};
  bufs[MOV] = {lists.mov.data(), nullptr, sizeof(int) * N};
  bufs[SWP] = {lists.swp.data(), nullptr, sizeof(int) * N};
  bufs[GSTART] = {lists.gstart.data(), nullptr, sizeof(int) * N};
  bufs[GSIZE] = {lists.gsize.data(), nullptr, sizeof(int) * N};
  bufs[NMOV] = {lists.n_mov.data(), nullptr, sizeof(int) * B};
  bufs[NSWP] = {lists.n_swp.data(), nullptr, sizeof(int) * B};
  bufs[ENERGY] = {energy, nullptr, sizeof(float) * B};
  bufs[FRAC_NEXT] = {frac_next, frac_next, sizeof(double) * 3 * N};
  bufs[RETRY] = {zero_retry.data(), retry, sizeof(int) * B};
  bufs[FSCAL] = {frame_scalars, frame_scalars, sizeof(double) * MC_FRAME_SCAL * B};
  bufs[FINT] = {frame_moves, frame_moves, sizeof(int) * MC_FRAME_INT * B};
  bufs[FPOS] = {frame_positions, frame_positions, sizeof(double) * 3 * N};
  bufs[FSITE] = {frame_site, frame_site, sizeof(int) * N};
  return run_test_step(eng, fn, bufs, [&] {
    McStepArgs a = base_args(*params, intensive ? 1 : 0, flags);
    a.r = (double*)bufs[R].d; a.site = (int*)bufs[SITE].d; a.sd = (double*)bufs[SD].d; a.si = (int*)bufs[SI].d;
    a.sl = (long long*)bufs[SL].d; a.best_pos = (double*)bufs[BPOS].d; a.best_site = (int*)bufs[BSITE].d;
    a.temp = (const double*)bufs[TEMP].d; a.seeds = (const unsigned long long*)bufs[SEEDS].d; a.aoff = (const int*)bufs[AOFF].d;
    a.mov = (const int*)bufs[MOV].d; a.swp = (const int*)bufs[SWP].d; a.gstart = (const int*)bufs[GSTART].d;
    a.gsize = (const int*)bufs[GSIZE].d; a.n_mov = (const int*)bufs[NMOV].d; a.n_swp = (const int*)bufs[NSWP].d;
    a.energy = energy ? (const float*)bufs[ENERGY].d : nullptr;
    a.frac_next = (double*)bufs[FRAC_NEXT].d; a.retry = (int*)bufs[RETRY].d;
    if (frame) { a.fr.scal = (double*)bufs[FSCAL].d; a.fr.ints = (int*)bufs[FINT].d; a.fr.pos = (double*)bufs[FPOS].d; a.fr.site = (int*)bufs[FSITE].d; }
    a.final_try = final_try ? 1 : 0;
    launch_step(eng, a, (int)B);
  });
}

int chg_test_mc_exchange(chg_engine* eng, int32_t n_struct, const int32_t* atom_off, const int32_t* ladder, const double* temperatures,
                         const uint64_t* seeds, double kB, int32_t m, double* r, int32_t* site, double* sd, int32_t* si,
                         double* best_positions, int32_t* best_site, int32_t* xi) {
  if (!eng || n_struct <= 0 || !atom_off || !ladder || !temperatures || !seeds || m < 1 || !r || !site || !sd || !si || !best_positions ||
      !best_site || !xi)
    return CHG_EINVAL;
  const char* fn = "chg_test_mc_exchange";
  const size_t B = n_struct;
  if (atom_off[0] != 0) return CHG_EINVAL;
  for (size_t o = 0; o < B; ++o)
    if (atom_off[o + 1] <= atom_off[o]) return CHG_EINVAL;
  const size_t N = atom_off[n_struct];
  McPairs pairs;
  TRY(build_pairs(eng, fn, n_struct, atom_off, ladder, temperatures, pairs));
  const std::vector<int>& list = pairs.list[(m - 1) & 1];
  for (size_t k = 0; k < list.size(); k += MC_PAIR_INTS)   // the walker ids index the rows of their ladder
    for (int o = list[k]; o <= list[k] + 1; ++o) {
      const int w = xi[(size_t)MC_XI * o + MC_X_WALKER];
      if (w < 0 || w >= list[k + 2]) { eng->err = std::string(fn) + ": replica " + std::to_string(o) + " holds a walker outside its ladder"; return CHG_EINVAL; }
    }
  if (list.empty()) return CHG_OK;   // no pair on this parity: nothing to launch
  enum { R, SITE, SD, SI, BPOS, BSITE, TEMP, SEEDS, AOFF, XI, PAIRS, N_BUFS };
  TestBuf bufs[N_BUFS];
  bufs[R] = {r, r, sizeof(double) * 3 * N};
  bufs[SITE] = {site, site, sizeof(int) * N};
  bufs[SD] = {sd, sd, sizeof(double) * MC_SD * B};
  bufs[SI] = {si, si, sizeof(int) * MC_SI * B};
  bufs[BPOS] = {best_positions, best_positions, sizeof(double) * 3 * N};
  bufs[BSITE] = {best_site, best_site, sizeof(int) * N};
  bufs[TEMP] = {temperatures, nullptr, sizeof(double) * B};
  bufs[SEEDS] = {seeds, nullptr, sizeof(uint64_t) * B};
  bufs[AOFF] = {atom_off, nullptr, sizeof(int) * (B + 1)};
  bufs[XI] = {xi, xi, sizeof(int) * MC_XI * B};
  bufs[PAIRS] = {list.data(), nullptr, sizeof(int) * list.size()};
  return run_test_step(eng, fn, bufs, [&] {
    McExchangeArgs x{};
    x.r = (double*)bufs[R].d; x.site = (int*)bufs[SITE].d; x.sd = (double*)bufs[SD].d; x.si = (const int*)bufs[SI].d;
    x.best_pos = (double*)bufs[BPOS].d; x.best_site = (int*)bufs[BSITE].d; x.temp = (const double*)bufs[TEMP].d;
    x.seeds = (const unsigned long long*)bufs[SEEDS].d; x.aoff = (const int*)bufs[AOFF].d; x.xi = (int*)bufs[XI].d;
    x.pairs = (const int*)bufs[PAIRS].d; x.kB = kB > 0.0 ? kB : 8.6173303e-5; x.m = (unsigned)m;
    launch_exchange(eng, x, (int)(list.size() / MC_PAIR_INTS));
  });
}

}  // extern "C"
