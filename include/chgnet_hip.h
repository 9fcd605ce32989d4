/* chgnet_hip.h -- C-ABI of the MI355X (gfx950) CHGNet engine (libchgnet_hip.so).
 *
 * The reference has no FFI for this path: its boundary is the Python class API
 *   CHGNet.predict_graph / forward      chgnet/model/model.py:593-665, 330-387
 *   BatchedGraph.from_graphs            chgnet/model/model.py:792-913
 *   CHGNet._compute                     chgnet/model/model.py:389-542
 * This header is what a ctypes/cffi binding inside that class binds instead of running the
 * torch modules.  Entry points:
 *
 *   chg_engine_create   <- CHGNet.__init__/load_state_dict (weights re-laid by pack.py)
 *   chg_batch_upload    <- [g.to(device) for g in graphs] + index offsetting of from_graphs
 *                          (model.py:640-644, 856-857, 873-877)
 *   chg_predict         <- from_graphs geometry/bases + _compute + the two autograd.grad sweeps
 *                          (model.py:826-871, 427-540, 517-535) + AtomRef (model.py:356-358,378)
 *   chg_batch_download  <- tensor.cpu().detach().numpy() per key (model.py:651-663)
 *
 * Conventions: plain C types only; every function returns 0 or a negative chg_status and
 * never throws; chg_last_error() gives the text of the last failure on that engine.  One
 * engine per GPU; calls on one engine must be serialised by the caller; engines on different
 * devices are independent (one process or thread per GPU).  Host buffers belong to the
 * caller, device memory to the library.  All floating point is fp32, all indices int32.
 */
#ifndef CHGNET_HIP_H
#define CHGNET_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  CHG_OK = 0,
  CHG_EINVAL = -1,     /* bad argument */
  CHG_EHIP = -2,       /* HIP runtime error (text in chg_last_error) */
  CHG_ENOMEM = -3,     /* device or host allocation failed */
  CHG_ENODEV = -4,     /* no usable gfx950 device */
  CHG_EUNSUPPORTED = -5,
  CHG_ERANGE = -6      /* a WEIGHT left the operand range of the split-precision contractions (|w| >= 65504: the tile kernels hold
                          their weights as f16 hi / lo images) -- chg_engine_create / chg_engine_update_weights.  ACTIVATIONS of any fp32
                          magnitude are computed: a batch whose product sweep overflows the f16 operands is detected at
                          chg_batch_download (non-finite results) and run again on the wide-range sweep (csrc/engine_predict_wide.hip),
                          like the reference's fp32 path (crystalgraph.py:12 TORCH_DTYPE); chg_backward follows it there
                          (csrc/engine_train_wide.hip) */
} chg_status;

/* task bits (reference task strings "e","ef","em","efs","efsm": chgnet/__init__.py:15) */
enum {
  CHG_TASK_E = 1u,
  CHG_TASK_F = 2u,
  CHG_TASK_S = 4u,
  CHG_TASK_M = 8u
};

typedef struct chg_engine chg_engine;
typedef struct chg_batch chg_batch;

typedef struct chg_model_desc {
  int32_t n_conv;              /* 4 for every released checkpoint */
  int32_t cutoff_coeff;        /* envelope exponent p (8 for 0.3.0) */
  int32_t is_intensive;
  int32_t has_composition;     /* AtomRef present */
  float atom_graph_cutoff;     /* 6 A */
  float bond_graph_cutoff;     /* 3 A */
  int64_t n_weights;           /* length of the blob in floats; layout = chgnet_amd/pack.py:weight_layout */
  int32_t n_mlp_hidden;        /* hidden layers of the energy head: 3 (0.3.0 / r2scan, mlp_hidden_dims=[64,64,64]) or 2 (0.2.0, [64,64]);
                                  0 = 3.  The blob keeps the third layer's slots either way (unused, zero, when 2) */
  int32_t mlp_out_bias;        /* 1: the mlp_out Linears of AtomConv / BondConv carry a bias (0.2.0 checkpoint, model.py:734) -- chg_backward then
                                  also forms their gradients and W_bond's term through the bonds outside the bond graph */
} chg_model_desc;

/* Packed batch of B structures in global (batch-wide) numbering: chgnet_amd/pack.py:pack_batch. */
typedef struct chg_batch_host {
  int32_t n_struct, n_atoms, n_directed, n_undirected, n_angles, n_bnodes;
  const int32_t* z;            /* [N]     atomic numbers                          */
  const float* frac;           /* [N,3]   fractional coordinates                  */
  const float* lattice;        /* [B,3,3] rows a,b,c                              */
  const int32_t* atom_owner;   /* [N]     structure index                         */
  const int32_t* atom_off;     /* [B+1]                                           */
  const int32_t* e_center;     /* [Ed]    atom_graph[:,0]                         */
  const int32_t* e_nbr;        /* [Ed]    atom_graph[:,1]                         */
  const float* e_image;        /* [Ed,3]  neighbor_image                          */
  const int32_t* e_d2u;        /* [Ed]    directed2undirected                     */
  const int32_t* e_owner;      /* [Ed]    structure index                         */
  const int32_t* e_rev;        /* [Ed]    index of the opposite directed edge     */
  const int32_t* p_center;     /* [Ed]    centre atom, bond-pair order (rows 2k,2k+1 = bond k) */
  const int32_t* p_nbr;        /* [Ed]    neighbour atom, bond-pair order         */
  const int32_t* u_u2d;        /* [Eu]    undirected2directed                     */
  const int32_t* u_bnode;      /* [Eu]    compact bond-graph node id or -1        */
  const int32_t* bn_und;       /* [Eb]    undirected index of each node           */
  const int32_t* a_ctr;        /* [A]     bond_graph[:,0]                         */
  const int32_t* a_b1c;        /* [A]     node id of bond_graph[:,1]              */
  const int32_t* a_b2c;        /* [A]     node id of bond_graph[:,3]              */
  const int32_t* a_d1;         /* [A]     bond_graph[:,2]                         */
  const int32_t* a_d2;         /* [A]     bond_graph[:,4]                         */
} chg_batch_host;

/* Host destinations for chg_batch_download; null pointers are skipped. */
typedef struct chg_out_host {
  float* energy;        /* [B]    eV/atom if is_intensive else eV (incl. AtomRef) */
  float* force;         /* [N,3]  eV/A            (needs CHG_TASK_F)              */
  float* stress;        /* [B,9]  GPa             (needs CHG_TASK_S)              */
  float* magmom;        /* [N]    mu_B            (needs CHG_TASK_M)              */
  float* site_energy;   /* [N]    eV, incl. AtomRef site shift                    */
  float* atom_fea;      /* [N,64] atom features before the last AtomConv          */
  float* crystal_fea;   /* [B,64]                                                 */
} chg_out_host;

/* Version of this interface: bumped whenever a struct of this header grows or an entry point changes meaning (chg_model_desc gained
 * n_mlp_hidden / mlp_out_bias at 2; chg_batch_build_predict arrived at 3; the chg_relax_* entry points at 4; the chg_md_* entry points at 5;
 * chg_hessian_vector and chg_hessian_vector_strain were added at 5 without a bump: new entry points only, no struct or signature changed;
 * so were chg_md_create_langevin and chg_test_md_step_langevin, whose extra parameters travel as arguments, not in chg_md_params;
 * so were chg_relax_create_lbfgs and chg_test_lbfgs_step, whose parameters travel in a struct of their own, chg_lbfgs_params;
 * so were chg_md_create_nhc, chg_md_download_nhc and chg_test_md_step_nhc: the chain length travels as an argument, the chain state and
 * the conserved energy in arrays of their own; so were chg_relax_set_fixed, chg_md_set_fixed and the chg_test_*_step_fixed siblings: the
 * mask travels as an argument to entry points of its own; so were chg_md_create_nhc_flex, chg_md_download_vg and
 * chg_test_md_step_nhc_flex: the cell mode travels as an argument, the strain-rate matrix in an array of its own;
 * so were chg_md_set_observers, chg_md_download_observables and chg_test_md_observe: their parameters and results travel in two structs
 * of their own, chg_md_observe_params and chg_md_observables_host, and no older struct or signature changed;
 * so were chg_md_set_transport, chg_md_download_transport and chg_test_md_transport, with chg_md_transport_params and
 * chg_md_transport_host; so were chg_md_set_magmoms, chg_md_download_magmoms, chg_md_set_charge_states, chg_md_download_charge_states
 * and chg_test_md_charge_states, with chg_md_charge_params and chg_md_charge_host; so were the chg_neb_* entry points and
 * chg_test_neb_step, with chg_neb_params and chg_neb_out_host; so were the chg_dimer_* entry points and chg_test_dimer_step, with
 * chg_dimer_params and chg_dimer_out_host).  A binding compiled against another value must refuse the
 * library: chg_engine_create COPIES *desc, so an older, shorter chg_model_desc would be read past its end. */
#define CHG_ABI_VERSION 5
int chg_abi_version(void);
int chg_device_count(void);
/* Length in floats of the weight blob for an n_conv-block model (same table as pack.py:weight_layout). */
int64_t chg_weights_required(int32_t n_conv);
int chg_engine_create(const chg_model_desc* desc, const float* weights_blob, int device, chg_engine** out);
int chg_engine_destroy(chg_engine* eng);
const char* chg_last_error(const chg_engine* eng);

/* Device-memory contract.  A batch lives in ONE arena (inputs + every activation / gradient buffer of the
 * forward and reverse sweeps); chg_batch_bytes_required gives its exact size from the counts alone, so a
 * caller can size chunks before uploading (the reference's only memory knob is batch_size,
 * chgnet/model/model.py:639-650).  chg_batch_upload / chg_batch_build return CHG_ENOMEM -- and leave the
 * engine usable -- when the arena cannot be allocated or exceeds the limit set here (0 = no limit); the
 * host side then splits the chunk and retries (chgnet_amd/model.py). */
int chg_engine_build_stats(chg_engine* eng, int64_t* single_pass_builds, int64_t* capacity_overflows);
int chg_engine_set_memory_limit(chg_engine* eng, int64_t bytes);
int chg_engine_memory_info(chg_engine* eng, int64_t* free_bytes, int64_t* total_bytes);
int64_t chg_batch_bytes_required(int32_t n_conv, int32_t n_struct, int32_t n_atoms, int32_t n_directed, int32_t n_angles, int32_t n_bnodes);

int chg_batch_upload(chg_engine* eng, const chg_batch_host* host, chg_batch** out);
/* Page-locked host buffers for the arrays of a chg_batch_host (optional): uploads from them run as asynchronous DMA at the link rate
 * instead of staged copies from pageable memory (the reference's counterpart is DataLoader(pin_memory=True), data/dataset.py). */
int chg_host_alloc(int64_t bytes, void** out);
int chg_host_free(void* p);

/* Structures only (no graph): the periodic neighbour list, bond numbering and bond graph are built on
 * the device, bit-for-bit the arrays of chg_graph_build (include/chgnet_graph.h) + pack.py.  Replaces
 * CrystalGraphConverter.forward (chgnet/graph/converter.py:102-190) for structures headed to the GPU. */
typedef struct chg_structs_host {
  int32_t n_struct, n_atoms;
  const int32_t* z;           /* [N]                                  */
  const double* frac;         /* [N,3]   float64 fractional coordinates (unwrapped is fine) */
  const double* lattice;      /* [B,3,3] float64, rows a,b,c          */
  const int32_t* atom_off;    /* [B+1]                                */
} chg_structs_host;
/* counts_out[6] = { n_directed, n_undirected, n_angles, n_bnodes, n_isolated_atoms, single_pass }.
 * The first build on an engine takes three blocking count round trips; later builds size their scratch from the previous
 * build's per-atom counts (+25 %), take every count from device memory and read them once at the end (single_pass = 1);
 * a capacity that proves too small is caught by a device-side flag and the build repeats on the exact path.
 * chg_engine_build_stats reports how many builds went each way. */
int chg_batch_build(chg_engine* eng, const chg_structs_host* host, double r_atom, double r_bond, double numerical_tol,
                    chg_batch** out, int32_t* counts_out);
/* chg_batch_build followed at once by chg_predict(task_mask) on the new batch, in ONE call: between the two the device of a
 * single-structure caller (an MD / relaxation step through CHGNetCalculator.calculate, reference chgnet/model/dynamics.py:129-181) sat
 * idle for the trip back into the host language (~15 us of a ~1 ms step).  Same results and errors as the two calls. */
int chg_batch_build_predict(chg_engine* eng, const chg_structs_host* host, double r_atom, double r_bond, double numerical_tol,
                            uint32_t task_mask, chg_batch** out, int32_t* counts_out);
/* Neighbour search of chg_batch_build, the device-side twin of chg_graph_build_with's `search` (chgnet_graph.h):
 * 0 = by size (structures with at least cell_min_atoms atoms -- default 2048, 0 keeps the current value -- are binned on
 * the host and searched through a cell list, one wave per centre, rows sorted in LDS), 1 = all pairs, 2 = cell list for
 * every structure.  The rows are the same bit for bit either way; a centre with more than 1024 rows makes the build
 * repeat with all pairs (counted by chg_engine_cell_stats). */
int chg_engine_set_graph_search(chg_engine* eng, int32_t search, int32_t cell_min_atoms);
int chg_engine_cell_stats(chg_engine* eng, int64_t* cell_builds, int64_t* all_pairs_fallbacks);
/* int32 index array of a batch by pack.py name (e_center, e_nbr, e_d2u, u_u2d, a_ctr, ...) -- tests only; "wide_range": one int,
 * 1 when chg_batch_download has moved the batch to the wide-range sweeps (an activation beyond the f16 operand range); "route": five
 * ints (0 / 1) for the last prediction of the batch -- the launch sequence of MD-size batches, its chained row GEMMs, z rows kept for
 * the angle adjoints (zsave), the per-atom window index, TEAM mode; a sixth int when the capacity allows: 1 = the large-batch tile
 * kernels ran with 32-bit row offsets (every table span below 4 GiB; CHGNET_ADDR_MODE=32 / 64 forces a mode, CHGNET_ADDR32_MAX_BYTES
 * moves the threshold), 0 = 64-bit */
int chg_debug_fetch_i32(chg_engine* eng, chg_batch* batch, const char* name, int32_t* dst, int64_t capacity, int64_t* n_written);
/* new positions / cells on an unchanged graph topology (finite differences, strain scans, a relaxation step that keeps its neighbours) */
int chg_batch_update_geometry(chg_engine* eng, chg_batch* batch, const float* frac, const float* lattice);
int chg_batch_free(chg_engine* eng, chg_batch* batch);
int64_t chg_batch_device_bytes(const chg_batch* batch);

/* Asynchronous on the engine's stream; results stay in HBM until downloaded. */
int chg_predict(chg_engine* eng, chg_batch* batch, uint32_t task_mask);
int chg_synchronize(chg_engine* eng);

/* Fine-tuning backward (reference: loss.backward() through CHGNet.forward, chgnet/trainer/trainer.py:399-411, model.py:427-542,
 * and through the create_graph=True forces / stress of model.py:517-535).  After chg_predict on `batch`:
 *   grad_blob[i] = d( sum_b ce[b] energy[b] + sum_i gm[i] magmom[i] + sum_i gF[i] . force[i] + sum_b gS[b] : stress[b] ) / d weights_blob[i]
 * in the layout of the weight blob (chgnet_amd/pack.py:weight_layout; derived entries -- transposed copies, q_bias -- and the
 * frozen AtomRef stay 0; pack.py:unpack_weight_grads maps it back to state_dict names).  All cotangents are host arrays in the
 * units chg_batch_download returns the quantities in: energy_cotangent [B] (null = ones), magmom_cotangent [N] or null,
 * force_cotangent [N,3] or null, stress_cotangent [B,9] or null; grad_blob: host [n_weights].  Synchronous.
 * Without force / stress terms this is a first-order reverse sweep (fused kernels).  With them it is ONE tangent sweep along
 * (ux = -gF, strain direction (160.2 / V) gS) followed by a reverse sweep with two adjoints per activation, one fused tile kernel
 * per layer and direction (kernels_train2_tile.h).  That
 * sweep reuses the first-order adjoints the force / stress sweep of chg_predict leaves in the batch: if the last prediction on
 * `batch` was energy-only, chg_backward runs the prediction with forces itself first.  Overwrites the batch's gradient workspace:
 * download forces / stress before calling. */
int chg_backward(chg_engine* eng, chg_batch* batch, const float* energy_cotangent, const float* magmom_cotangent,
                 const float* force_cotangent, const float* stress_cotangent, float* grad_blob);
/* The same, for a data-parallel step: the gradient blob is summed over the ranks of `comm` (ncclAllReduce on the engine's
 * stream, in HBM) before it is copied to the host -- every rank receives the summed blob.  comm = NULL: chg_backward. */
struct chg_comm;
int chg_backward_allreduce(chg_engine* eng, chg_batch* batch, const float* energy_cotangent, const float* magmom_cotangent,
                           const float* force_cotangent, const float* stress_cotangent, struct chg_comm* comm, float* grad_blob);
/* H u per structure: hvp[i] = sum_j d2 E_b / (dx_i dx_j) u_j over the atoms j of i's structure (E_b the total energy, eV; fixed
 * neighbour list; cartesian positions, cell fixed).  direction: host [N,3] (A); hvp: host [N,3] (eV/A^2).  After chg_predict on
 * `batch` (runs the force prediction first if the last one was energy-only).  Overwrites the gradient workspace.  Synchronous.
 * The tangent + two-adjoint sweep of chg_backward without its weight-gradient contractions, then the adjoints of the bond lengths
 * and angles (csrc/kernels_hvp.h) scattered to the atoms. */
int chg_hessian_vector(chg_engine* eng, chg_batch* batch, const float* direction, float* hvp);
/* The same with strain blocks: the full Hessian of E_b(x, eps) at eps = 0 along (u, W), with the lattice L (I + eps) and the atoms at
 * fixed fractional coordinates (every bond vector v0 (I + eps)):  hvp = d2E/dx dx . u + d2E/dx deps : W  [N,3] (eV/A^2),
 * hvp_strain[b] = d2E/deps dx . u + d2E/deps deps : W  [B,9] (eV, row-major [a][b] = d/d eps[a][b], the virial's convention).
 * direction: host [N,3] (A); strain: host [B,9] (dimensionless W per structure).  Preconditions and the wide-range fallback (on either
 * output) of chg_hessian_vector; strain = 0 gives its hvp.  The (x, eps) adjoints are scattered by k_hvp_strain_scatter
 * (csrc/kernels_hvp.h).  Added at 5 without a bump, as chg_hessian_vector. */
int chg_hessian_vector_strain(chg_engine* eng, chg_batch* batch, const float* direction, const float* strain, float* hvp,
                              float* hvp_strain);
/* All-gather of the batch's per-structure energies (after chg_predict) from HBM on the engine's stream: every rank
 * contributes `width` floats (its n_struct energies, zero-padded), table: host [nranks * width] in rank order. */
int chg_batch_all_gather_energy(chg_engine* eng, chg_batch* batch, struct chg_comm* comm, int64_t width, float* table);
/* The engine's HIP stream (a hipStream_t) and device ordinal, for callers that enqueue their own device work behind it. */
void* chg_engine_stream(chg_engine* eng);
int chg_engine_device(chg_engine* eng);
/* New parameter values for an existing engine (optimizer step): same blob layout and length as at creation.  Also rebuilds the
 * prebuilt LDS weight images the inference kernels read (captured hipGraphs stay valid: they hold the image buffer, not its contents). */
int chg_engine_update_weights(chg_engine* eng, const float* weights_blob);
int chg_batch_download(chg_engine* eng, chg_batch* batch, const chg_out_host* out);

/* Wall time of the stream between two marks, from HIP events recorded on the engine's stream. */
int chg_timer_start(chg_engine* eng);
int chg_timer_stop_ms(chg_engine* eng, float* elapsed_ms);

/* STREAM-like device copy of `bytes` (read + write) repeated `iters` times on the engine's stream; the average
 * time of one copy.  2 * bytes / time is the measured HBM ceiling quoted next to the HBM-bound kernels. */
int chg_stream_copy(chg_engine* eng, int64_t bytes, int iters, float* ms_per_iter);

/* Per-kernel profile: when enabled every launch is bracketed by HIP events on the engine's
 * stream.  chg_profile_read returns, for entry i, the kernel label, launch count and total ms. */
int chg_profile_enable(chg_engine* eng, int on);
int chg_profile_reset(chg_engine* eng);
int chg_profile_count(chg_engine* eng);
int chg_profile_read(chg_engine* eng, int i, char* label, int label_cap, int64_t* launches, double* total_ms);

/* Copy a named intermediate device buffer of the last chg_predict to the host (tests only).
 * Returns the number of floats written in *n_written; CHG_EINVAL if the name is unknown. */
int chg_debug_fetch(chg_engine* eng, chg_batch* batch, const char* name, float* dst, int64_t capacity, int64_t* n_written);

/* Self-test of the MFMA tile primitives: Y[rows,nout] = X[rows,k] . Wt[nout,k]^T + bias (k, nout in {64,128}). */
int chg_test_rows_gemm(chg_engine* eng, const float* x, const float* wt, const float* bias, float* y, int rows, int k, int nout);
/* Self-test of the split-precision contractions every tile kernel runs on (csrc/mfma_split.h: three f16 MFMAs per f32 product,
 * f32 accumulation), W [f][64] row-major with f in {64, 128}:
 *   mode 0  Y[rows,f]  = X[rows,64] . W^T   forward operands, split image [plane][k/32][g][f][8]
 *   mode 1  Y[rows,64] = X[rows,f]  . W     adjoint operands (rows scaled by a power of two), split image of W^T
 *   mode 2 / 3  the same two products from ONE row-major image (forward ds_read_b64, adjoint ds_read_b64_tr_b16) */
int chg_test_split_gemm(chg_engine* eng, const float* x, const float* w, float* y, int rows, int f, int mode);

/* ---- structure relaxation: FIRE through the Frechet cell filter, every structure an independent optimizer -------------------
 * Reference: StructOptimizer.relax (chgnet/model/dynamics.py:184-346), ASE FIRE(FrechetCellFilter(atoms)).run(fmax, steps) with ASE's
 * defaults.  The state of every structure (generalized coordinates u / X, velocity, dt, a, Nsteps, step count, status) lives in HBM
 * in float64; one step = graph built on the device from the active structures + prediction (chg_batch_build_predict) + one step
 * kernel (csrc/kernels_relax.h) + one asynchronous copy of the next coordinates.  Structures that have stopped drop out of the next
 * build.  DESIGN.md "Structure relaxation" states the semantics; tests/relax_ref.py restates them in float64 NumPy. */
enum { CHG_RELAX_RUNNING = 0, CHG_RELAX_CONVERGED = 1, CHG_RELAX_MAX_STEPS = 2, CHG_RELAX_NONFINITE = 3 };
typedef struct chg_relax_params {
  double fmax;                 /* converged: max over rows |g_row|^2 < fmax^2 (cell rows included)                     */
  int32_t max_steps, relax_cell;
  double dt, maxstep, dtmax, finc, fdec, astart, fa;   /* ASE FIRE: 0.1, 0.2, 1.0, 1.1, 0.5, 0.1, 0.99                 */
  int32_t nmin;                /* 5                                                                                     */
  double exp_cell_factor;      /* <= 0: atoms of each structure                                                        */
  double r_atom, r_bond, numerical_tol;                /* graph build (6, 3, 1e-8)                                      */
  double stress_weight;        /* engine stress (GPa) -> eV/A^3; <= 0: 1 / 160.21766208                                  */
} chg_relax_params;
typedef struct chg_relax chg_relax;
/* Frame of the LAST evaluated configuration of every structure (null pointers are skipped).  Units as chg_batch_download. */
typedef struct chg_relax_out_host {
  double* frac;        /* [N,3]   fractional coordinates of the evaluated configuration */
  double* lattice;     /* [B,3,3] rows a,b,c                                            */
  float* energy;       /* [B]     eV/atom if is_intensive else eV                       */
  float* force;        /* [N,3]   eV/A                                                   */
  float* stress;       /* [B,9]   GPa                                                    */
  float* magmom;       /* [N]     mu_B                                                   */
  int32_t* n_steps;    /* [B]     optimizer steps taken                                 */
  int32_t* status;     /* [B]     CHG_RELAX_*                                           */
} chg_relax_out_host;
/* Copies the structures and the parameters; no evaluation yet.  CHG_ENOMEM when the state cannot be allocated. */
int chg_relax_create(chg_engine* eng, const chg_structs_host* host, const chg_relax_params* params, chg_relax** out);
/* Up to n_steps evaluations, each followed by a step of every structure still running; *n_active = structures still running
 * (0: done).  A batch whose results are non-finite is evaluated again on the wide-range sweep (as chg_batch_download does); a
 * structure that is non-finite even there stops as CHG_RELAX_NONFINITE without moving.  CHG_ENOMEM: the batch arena does not fit. */
int chg_relax_run(chg_engine* eng, chg_relax* relax, int32_t n_steps, int32_t* n_active);
int chg_relax_download(chg_engine* eng, chg_relax* relax, const chg_relax_out_host* out);
int chg_relax_free(chg_engine* eng, chg_relax* relax);
/* Tests only: ONE step kernel on caller-given state and results (like chg_test_rows_gemm), in place.  Layout of the state (structure o
 * with atoms atom_off[o]..atom_off[o+1]): q, v [N + 3B, 3] (rows of o start at atom_off[o] + 3 o: atom rows u or r, then 3 cell rows X),
 * sd [B, 24] doubles (L0[9], L0^-1[9], exp_cell_factor, dt, a, 3 spare), si [B, 4] ints (FIRE Nsteps, steps taken, status, spare).
 * energy [B], force [N,3], stress [B,9] GPa, magmom [N] or null; out: frac_next [N,3], lat_next [B,9] (the moved structures'). */
int chg_test_relax_step(chg_engine* eng, const chg_relax_params* params, int32_t n_struct, const int32_t* atom_off, double* q, double* v,
                        double* sd, int32_t* si, const float* energy, const float* force, const float* stress, const float* magmom,
                        double* frac_next, double* lat_next);

/* L-BFGS instead of FIRE (the reference's StructOptimizer(optimizer_class="LBFGS")): ASE's LBFGS with its defaults and no line search,
 * on the same generalized coordinates q and forces g, with the same stop rules, retry and compaction.  Per structure and evaluation
 * that neither stops nor is held back (q, g flattened; the ring holds the last m <= M = max(1, min(memory, max_steps)) triples):
 *   steps taken > 0:  s0 = q - r0, y0 = g0 - g; when y0 . s0 is finite and not 0 the triple (s0, y0, 1 / (y0 . s0)) is appended,
 *                     the oldest one dropped beyond M (ASE would divide by zero where this one skips the triple)
 *   t = -g;  newest to oldest: a_i = rho_i (s_i . t), t -= a_i y_i;  z = t / alpha;  oldest to newest: z += s_i (a_i - rho_i (y_i . z))
 *   p = -z; when the longest ROW of p (cell rows included) is >= maxstep, p is scaled so that it is maxstep (FIRE clamps the norm)
 *   r0 = q, g0 = g, q += damping p, steps taken += 1
 * One step kernel (csrc/kernels_lbfgs.h); tests/lbfgs_ref.py restates it in float64 NumPy.  The history takes
 * 2 M 3 (N + 3 B) 8 bytes of the state and does not move when structures drop out. */
typedef struct chg_lbfgs_params {
  double maxstep, damping, alpha;   /* ASE LBFGS: 0.2, 1.0, 70.0 (H0 = 1 / alpha); all > 0                               */
  int32_t memory;                   /* 100; >= 1                                                                        */
  int32_t reserved;                 /* 0                                                                                */
} chg_lbfgs_params;
/* As chg_relax_create; of *params dt, maxstep, dtmax, finc, fdec, astart, fa and nmin are ignored.  The handle is an ordinary
 * chg_relax for chg_relax_run / chg_relax_download / chg_relax_free.  CHG_ENOMEM when the state (history included) cannot be allocated. */
int chg_relax_create_lbfgs(chg_engine* eng, const chg_structs_host* host, const chg_relax_params* params, const chg_lbfgs_params* lbfgs,
                           chg_relax** out);
/* Tests only: ONE L-BFGS step kernel on caller-given state and results, in place.  R = N + 3 B rows; the rows of structure o start at
 * atom_off[o] + 3 o (atom rows, then 3 cell rows) in every row array:
 *   q, r0, g0 [R, 3];  S, Y [M, R, 3]: the k-th triple appended (k from 0) sits in slot k % M;  rho [B, M] by slot;
 *   sd [B, 24] as chg_test_relax_step (L0[9], L0^-1[9], exp_cell_factor, rest unused);
 *   si [B, 4] ints: triples appended so far (the ring holds the last min(that, M)), steps taken, status, spare.
 * energy [B], force [N,3], stress [B,9] GPa, magmom [N] or null.  final_try 0: a structure with non-finite results is left untouched
 * and retry[o] is set to 1 (retry [B] is in / out, the caller zeroes it); 1: it stops as CHG_RELAX_NONFINITE.
 * out: frac_next [N,3], lat_next [B,9] (the moved structures'). */
int chg_test_lbfgs_step(chg_engine* eng, const chg_relax_params* params, const chg_lbfgs_params* lbfgs, int32_t n_struct,
                        const int32_t* atom_off, double* q, double* r0, double* g0, double* S, double* Y, double* rho, double* sd, int32_t* si,
                        const float* energy, const float* force, const float* stress, const float* magmom, int32_t final_try,
                        double* frac_next, double* lat_next, int32_t* retry);

/* ---- molecular dynamics: NVE, NVT Berendsen, NPT Berendsen, every structure an independent replica ---------------------------
 * Reference: MolecularDynamics (chgnet/model/dynamics.py:433-780) with ASE VelocityVerlet, NVTBerendsen, Inhomogeneous_NPTBerendsen and
 * NPTBerendsen.  The state of every replica (cartesian positions, momenta, masses, cached forces, cell and its inverse, step count,
 * status) lives in HBM in float64; one evaluation = graph built on the device from all replicas + prediction (chg_batch_build_predict,
 * task ef, efs for NPT or logged stress) + one step kernel (csrc/kernels_md.h) + one asynchronous copy of the next coordinates.  NPT
 * takes two evaluations per step, as ASE does (the barostat moves the atoms before the first half kick).  Units are ASE's: eV, A,
 * amu, time in A sqrt(amu / eV).  DESIGN.md "Molecular dynamics" states the semantics; tests/md_ref.py restates them in NumPy. */
enum { CHG_MD_NVE = 0, CHG_MD_NVT_BERENDSEN = 1, CHG_MD_NPT_BERENDSEN_INHOMOGENEOUS = 2, CHG_MD_NPT_BERENDSEN = 3,
       CHG_MD_NVT_LANGEVIN = 4 /* chg_md_create_langevin only */, CHG_MD_NVT_NHC = 5, CHG_MD_NPT_NHC = 6 /* chg_md_create_nhc only */,
       CHG_MD_NPT_NHC_FLEX = 7, CHG_MD_NPT_NHC_AXES = 8 /* chg_md_create_nhc_flex only */ };
enum { CHG_MD_RUNNING = 0, CHG_MD_NONFINITE = 1 };
typedef struct chg_md_params {
  int32_t ensemble;            /* CHG_MD_*                                                                                 */
  int32_t fixcm;               /* NVT / NPT: subtract the mean momentum after the first half kick (ASE fixcm=True)         */
  double dt;                   /* time step, ASE time units                                                                */
  double temperature;          /* K (NVT / NPT)                                                                            */
  double taut, taup;           /* ASE time units                                                                           */
  double pressure;             /* eV/A^3 (NPT)                                                                             */
  double compressibility;      /* A^3/eV (NPT)                                                                             */
  double kB;                   /* eV/K; <= 0: 8.6173303e-5 (CODATA 2014, ASE units.kB)                                      */
  double stress_weight;        /* engine stress (GPa) -> eV/A^3; <= 0: 1 / 160.21766208                                    */
  int32_t loginterval;         /* a frame every loginterval steps, step 0 included; 0: no frames                           */
  int32_t ring_frames;         /* frames the device ring holds between two chg_md_download calls                          */
  int32_t log_stress;          /* evaluate the stress every step (task efs) even without NPT: frames then carry it        */
  int32_t log_crystal_fea;     /* frames carry crystal_fea [64]                                                            */
  double r_atom, r_bond, numerical_tol;                /* graph build (6, 3, 1e-8)                                          */
} chg_md_params;
typedef struct chg_md chg_md;
/* Current state (null pointers are skipped) and up to frame_capacity of the oldest frames in the ring, which are removed from it. */
typedef struct chg_md_out_host {
  double* positions;           /* [N,3]   cartesian, A (unwrapped)                                                         */
  double* momenta;             /* [N,3]   amu A / ASE time unit                                                            */
  double* cell;                /* [B,3,3] rows a,b,c                                                                       */
  int32_t* n_steps;            /* [B]     steps completed                                                                  */
  int32_t* status;             /* [B]     CHG_MD_*                                                                         */
  int32_t frame_capacity;      /* K: frames the arrays below hold                                                          */
  int32_t* n_frames;           /* out: frames written                                                                      */
  int32_t* frame_step;         /* [K]                                                                                      */
  double* frame_scalars;       /* [K,B,3] energy as the engine gives it (eV/atom if is_intensive), Ekin (eV), T (K)        */
  double* frame_positions;     /* [K,N,3]                                                                                  */
  double* frame_momenta;       /* [K,N,3]                                                                                  */
  double* frame_cell;          /* [K,B,3,3]                                                                                */
  float* frame_force;          /* [K,N,3] eV/A                                                                             */
  float* frame_stress;         /* [K,B,9] GPa, the model's stress (no ideal-gas term); 0 when not evaluated               */
  float* frame_crystal_fea;    /* [K,B,64] (log_crystal_fea)                                                               */
} chg_md_out_host;
/* Copies the structures, masses [N] (amu) and initial momenta [N,3] (null: zero); no evaluation yet.  CHG_ENOMEM when the state
 * cannot be allocated. */
int chg_md_create(chg_engine* eng, const chg_structs_host* host, const double* masses, const double* momenta, const chg_md_params* params,
                  chg_md** out);
/* NVT Langevin (not in the reference): BAOAB, one evaluation per step, fixed cell.  Per step with c1 = exp(-friction dt):
 *   p += dt/2 f;  r += dt/2 p/m;  p <- c1 p + sqrt((1 - c1^2) m kB T) xi;  fixcm: p_i -= m_i sum p / sum m;  r += dt/2 p/m;
 *   evaluation;  p += dt/2 f.
 * xi (three standard normals per atom) is a pure function of (seeds[replica], atom index within the replica, steps the replica has
 * completed): Philox4x32-10 and Box-Muller in the step kernel (csrc/philox.h), no generator state in memory, so a replica's
 * trajectory does not depend on its slot in the batch, on retries or on how chg_md_run calls split the steps.
 * params->ensemble must be CHG_MD_NVT_LANGEVIN (chg_md_create refuses it with CHG_EINVAL: it has no friction or seeds to give);
 * friction >= 0 and finite, in inverse ASE time units (0: velocity Verlet); temperature >= 0; taut, taup, pressure and compressibility
 * are ignored; seeds [B] are copied.  The handle is an ordinary chg_md for chg_md_run / chg_md_download / chg_md_free.
 * tests/langevin_ref.py restates integrator and noise in NumPy. */
int chg_md_create_langevin(chg_engine* eng, const chg_structs_host* host, const double* masses, const double* momenta,
                           const chg_md_params* params, double friction, const uint64_t* seeds, chg_md** out);
/* Nose-Hoover-chain NVT (CHG_MD_NVT_NHC) and isotropic NPT (CHG_MD_NPT_NHC), not in the reference: the Martyna-Tobias-Klein equations
 * with a chain of chain_length (1..4) thermostats on the particles and another on the barostat, integrated reversibly to second order
 * (Tuckerman et al., J. Phys. A 39 (2006) 5629), one evaluation per step (task efs for NPT), any cell shape: the cell only scales.
 * With kT = kB temperature, N_f = 3 (n - 1): Q_1 = N_f kT taut^2, Q_k = kT taut^2, Q'_k = kT taup^2, W = (N_f + 3) kT taup^2.
 * tests/nhc_ref.py restates the step in NumPy; DESIGN.md "Nose-Hoover chains" gives the equations.  temperature > 0, taut > 0 (NPT: taup > 0,
 * pressure finite, eV/A^3); compressibility and fixcm are ignored: the centre-of-mass momentum is never touched, the caller removes it
 * from the initial momenta.  Every structure needs at least two atoms.  chg_md_create refuses the two codes with CHG_EINVAL.  The
 * handle is an ordinary chg_md for chg_md_run / chg_md_download / chg_md_free.
 * State per replica, CHG_MD_NHC_STATE doubles, all zero at creation: chain velocities v[4] and positions eta[4] of the particles, vb[4]
 * and xi[4] of the barostat (the first chain_length of each are used), the strain rate veps, H - Epot of the last evaluation (eV), 2 spare.
 * H = Epot + sum p^2/2m + sum Q_k v_k^2 / 2 + N_f kT eta_1 + kT sum_{k>1} eta_k (+ Pext V + W veps^2 / 2 + sum Q'_k vb_k^2 / 2 + kT sum xi_k)
 * is conserved. */
#define CHG_MD_NHC_STATE 20
int chg_md_create_nhc(chg_engine* eng, const chg_structs_host* host, const double* masses, const double* momenta, const chg_md_params* params,
                      int32_t chain_length, chg_md** out);
/* The chain state nhc_state [B, CHG_MD_NHC_STATE] and H - Epot (eV) of up to frame_capacity of the oldest frames in the ring,
 * frame_conserved [K, B], in the order chg_md_download returns them.  The ring is NOT drained: call this before chg_md_download.  Null
 * pointers are skipped.  CHG_EINVAL for a handle of another ensemble. */
int chg_md_download_nhc(chg_engine* eng, chg_md* md, double* nhc_state, double* frame_conserved, int32_t frame_capacity);
/* Flexible-cell Nose-Hoover-chain NPT, not in the reference: the same equations and factorisation with a symmetric strain-rate matrix Vg
 * (1/time) in place of the scalar veps.  cell_mode CHG_MD_CELL_FLEXIBLE frees all six components of Vg (lengths and angles move;
 * ensemble code CHG_MD_NPT_NHC_FLEX), CHG_MD_CELL_AXES the three cartesian diagonal ones (the off-diagonal ones stay exactly 0: an
 * orthogonal cell keeps its angles; CHG_MD_NPT_NHC_AXES); the isotropic cell is chg_md_create_nhc.  params->ensemble is ignored: the cell
 * mode chooses the code.  With d_b = 6 or 3 free components: W_g = W / 3 per component, barostat chain masses Q'_1 = d_b kT taup^2,
 * Q'_k = kT taup^2; the barostat chain thermostats W_g sum_ab Vg_ab^2 with d_b degrees of freedom; the barostat kick is
 * Vg_ab += dt/2 (sum p_a p_b / m + (sum p^2/m / N_f - Pext V) delta_ab - V (sigma + sigma^T)_ab / 2) / W_g; particles and cell move with
 * exponentials of symmetric 3x3 matrices (DESIGN.md "Nose-Hoover chains"; tests/nhc_flex_ref.py restates the step in NumPy).  pressure is
 * a scalar.  Everything chg_md_create_nhc requires for CHG_MD_NPT_NHC is required here, task efs every step; chg_md_create and
 * chg_md_create_nhc refuse the two codes with CHG_EINVAL.  The chain state is that of chg_md_download_nhc with veps = 0 and
 * H - Epot = ... + Pext V + W_g sum_ab Vg_ab^2 / 2 + sum Q'_k vb_k^2 / 2 + d_b kT xi_1 + kT sum_{k>1} xi_k; the strain-rate matrix,
 * CHG_MD_VG doubles per replica (row-major 3x3, symmetric, zero at creation), is read with chg_md_download_vg [B, CHG_MD_VG]
 * (CHG_EINVAL for a handle of another ensemble). */
enum { CHG_MD_CELL_FLEXIBLE = 1, CHG_MD_CELL_AXES = 2 };
#define CHG_MD_VG 9
int chg_md_create_nhc_flex(chg_engine* eng, const chg_structs_host* host, const double* masses, const double* momenta,
                           const chg_md_params* params, int32_t chain_length, int32_t cell_mode, chg_md** out);
int chg_md_download_vg(chg_engine* eng, chg_md* md, double* vg);
/* n_steps steps of every replica (the first call evaluates the initial configuration first and writes the frame of step 0).  A batch
 * whose results are non-finite is evaluated again on the wide-range sweep; a replica that is non-finite even there stops as
 * CHG_MD_NONFINITE with its state untouched.  CHG_EINVAL (nothing run) when the frames due do not fit the ring. */
int chg_md_run(chg_engine* eng, chg_md* md, int32_t n_steps);
int chg_md_download(chg_engine* eng, chg_md* md, const chg_md_out_host* out);
int chg_md_free(chg_engine* eng, chg_md* md);
/* Tests only: ONE step kernel launch on caller-given state, in place.  flags: 1 absorb the evaluation (energy [B], force [N,3],
 * stress [B,9] GPa or null), 2 second half kick, 4 start the next step.  State: r, momenta, forces (cached), masses [N,3] / [N];
 * sd [B, 40] doubles (L[9], L^-1[9], Epot, Ekin, T, stress[9] eV/A^3, sum p p / m [9], spare); si [B, 4] ints (steps completed,
 * status, phase (1: NPT scaled configuration awaiting its evaluation), spare); out: frac_next [N,3], lat_next [B,9]. */
int chg_test_md_step(chg_engine* eng, const chg_md_params* params, int32_t n_struct, const int32_t* atom_off, int32_t flags, double* r,
                     double* momenta, double* forces, const double* masses, double* sd, int32_t* si, const float* energy, const float* force,
                     const float* stress, double* frac_next, double* lat_next);
/* The same for CHG_MD_NVT_LANGEVIN: friction and seeds [n_struct] as in chg_md_create_langevin; the noise counter is si[0]. */
int chg_test_md_step_langevin(chg_engine* eng, const chg_md_params* params, int32_t n_struct, const int32_t* atom_off, int32_t flags, double* r,
                              double* momenta, double* forces, const double* masses, double* sd, int32_t* si, const float* energy,
                              const float* force, const float* stress, double* frac_next, double* lat_next, double friction,
                              const uint64_t* seeds);
/* The same for CHG_MD_NVT_NHC / CHG_MD_NPT_NHC: nhc [n_struct, CHG_MD_NHC_STATE] in place.  MD_START reads the cached forces, the stress
 * sd[21..29] and the trace of sd[30..38]; stress is required with flag 1 for CHG_MD_NPT_NHC. */
int chg_test_md_step_nhc(chg_engine* eng, const chg_md_params* params, int32_t n_struct, const int32_t* atom_off, int32_t flags, double* r,
                         double* momenta, double* forces, const double* masses, double* sd, int32_t* si, const float* energy,
                         const float* force, const float* stress, double* frac_next, double* lat_next, int32_t chain_length, double* nhc);
/* The same for CHG_MD_NPT_NHC_FLEX / CHG_MD_NPT_NHC_AXES (params->ensemble names the code): vg [n_struct, CHG_MD_VG] in place, and a mask
 * fixed [N,3] or null as in chg_test_md_step_fixed (which refuses the two codes).  MD_START reads all of sd[30..38]. */
int chg_test_md_step_nhc_flex(chg_engine* eng, const chg_md_params* params, int32_t n_struct, const int32_t* atom_off, int32_t flags, double* r,
                              double* momenta, double* forces, const double* masses, double* sd, int32_t* si, const float* energy,
                              const float* force, const float* stress, double* frac_next, double* lat_next, int32_t chain_length, double* nhc,
                              double* vg, const uint8_t* fixed);

/* ---- constraints: fixed atoms and fixed cartesian components in relaxation and molecular dynamics --------------------------------
 * fixed [N,3] uint8, 1 = the component is held (ASE FixAtoms: all three of an atom; FixCartesian: some).  A constrained step is the
 * unconstrained step with the constraint projected after every update, as ASE does (DESIGN.md "Constraints";
 * tests/constraint_ref.py restates it in NumPy):
 *   relaxation  the engine's force on a held component counts as 0 (generalized force, dot products, maxstep clamp, convergence test and
 *               the reported forces; the finiteness test sees the raw forces).  With relax_cell a held atom keeps its fractional
 *               coordinates and follows the cell; the stress is not masked.
 *   MD          the absorbed forces and every write of the momenta are masked, so are the sums they feed.  A replica that holds at least
 *               one component has dof = its free components: T = 2 Ekin / (dof kB), and N_f = dof in the Nose-Hoover chains (alpha, Q_1,
 *               W, the N_f kT eta_1 term of H).  A replica that holds nothing keeps 3 n and 3 (n - 1).  Langevin noise stays a function
 *               of (seed, atom, step): what is drawn for a held component is dropped.  Under a moving cell held atoms scale with it.
 * Both calls are valid between create and the first run; null clears the mask (an all-zero mask computes bit for bit what no mask
 * computes).  chg_md_set_fixed also sets the momenta: those given to the create call, with the held ones at 0 -- every call derives
 * them from the created ones again, so another mask, or null, gives back what an earlier mask had zeroed.
 * A fully held atom of a relaxation is evaluated at, and reported with, exactly the fractional coordinates the create call was given:
 * the handle keeps a copy of them (u L0^-1 would round them in the last bit).  The chg_test_*_step_fixed entry points have no such
 * copy and report u L0^-1 for every atom.  CHG_EINVAL with a message: after the first run; an atom with only some
 * components held while the cell moves (relax_cell, CHG_MD_NPT_BERENDSEN*, CHG_MD_NPT_NHC*); a replica with no free component in any
 * ensemble but CHG_MD_NVE. */
int chg_relax_set_fixed(chg_engine* eng, chg_relax* relax, const uint8_t* fixed /* [N,3] */);
int chg_md_set_fixed(chg_engine* eng, chg_md* md, const uint8_t* fixed /* [N,3] */);
/* Tests only: chg_test_relax_step, chg_test_lbfgs_step and the three chg_test_md_step* with a mask (null: exactly the entry point they
 * extend; the refusals above apply).  chg_test_md_step_fixed takes the arguments of all three: friction and seeds for
 * CHG_MD_NVT_LANGEVIN, chain_length and nhc for the two chain ensembles, null / 0 otherwise. */
int chg_test_relax_step_fixed(chg_engine* eng, const chg_relax_params* params, int32_t n_struct, const int32_t* atom_off, double* q, double* v,
                              double* sd, int32_t* si, const float* energy, const float* force, const float* stress, const float* magmom,
                              double* frac_next, double* lat_next, const uint8_t* fixed);
int chg_test_lbfgs_step_fixed(chg_engine* eng, const chg_relax_params* params, const chg_lbfgs_params* lbfgs, int32_t n_struct,
                              const int32_t* atom_off, double* q, double* r0, double* g0, double* S, double* Y, double* rho, double* sd,
                              int32_t* si, const float* energy, const float* force, const float* stress, const float* magmom,
                              int32_t final_try, double* frac_next, double* lat_next, int32_t* retry, const uint8_t* fixed);
int chg_test_md_step_fixed(chg_engine* eng, const chg_md_params* params, int32_t n_struct, const int32_t* atom_off, int32_t flags, double* r,
                           double* momenta, double* forces, const double* masses, double* sd, int32_t* si, const float* energy,
                           const float* force, const float* stress, double* frac_next, double* lat_next, double friction,
                           const uint64_t* seeds, int32_t chain_length, double* nhc, const uint8_t* fixed);

/* ---- MD observables accumulated on the device (DESIGN.md "MD observables"; tests/md_observe_ref.py restates them in NumPy) --------
 * Every sample_interval-th COMPLETED step (step 0 included, counted across chg_md_run calls) is sampled; sample number k = 0, 1, ...
 * of the handle.  species [N] maps every atom to 0 .. n_species - 1.  With n_lags = L > 0 a ring holds the last L sampled snapshots
 * (positions, velocities p / m, centre of mass), and for every lag l in 0 .. min(k, L - 1), every replica o still CHG_MD_RUNNING and
 * every species s
 *   msd [o,l,s] += sum_{i in o, species s} |(r_i(k) - R_o(k)) - (r_i(k-l) - R_o(k-l))|^2      (A^2, unwrapped positions)
 *   vacf[o,l,s] += sum_{i in o, species s} v_i(k) . v_i(k-l)                                   (ASE velocity units squared)
 *   cnt [o,l]   += 1
 * with R_o the mass-weighted centre of mass of the replica when subtract_com is set and 0 otherwise.  With rdf_bins > 0, for every
 * ordered pair (i, j) of a running replica and every lattice shift n (i == j with n == 0 excluded) with d = |r_j - r_i + n L| <
 * rdf_rmax, rdf[o, s_i, s_j, floor(d / rdf_rmax * rdf_bins)] += 1; rdf_samples[o] += 1 and vol_sum[o] += |det L| per sample.  The
 * sums do not depend on scheduling: no floating-point atomics, integer counts.  A replica that stopped is skipped for good.
 * chg_md_set_observers is valid between create and the first run (a second call replaces the first); CHG_EINVAL with a message for
 * a bad parameter (n_species * n_species * rdf_bins > 16384 included), a species index out of range and a call after the first run;
 * CHG_ENOMEM when the ring (L * (48 N + 24 B) bytes) does not fit.  chg_md_free releases what it allocated.  Without observers a run
 * launches exactly what it launched before they existed. */
typedef struct chg_md_observe_params {
  int32_t sample_interval;  /* sample every this many completed steps, step 0 included; >= 1 */
  int32_t n_lags;           /* L, 0: no MSD / VACF; <= 4096 */
  int32_t subtract_com;
  int32_t n_species;        /* S, 1..8 */
  int32_t rdf_bins;         /* 0: no RDF */
  int32_t reserved;
  double rdf_rmax;          /* A, > 0 when rdf_bins > 0 */
} chg_md_observe_params;
int chg_md_set_observers(chg_engine* eng, chg_md* md, const chg_md_observe_params* params, const int32_t* species /* [N] */);
typedef struct chg_md_observables_host {
  double* msd;              /* [B,L,S] */
  double* vacf;             /* [B,L,S] */
  int64_t* cnt;             /* [B,L]   */
  uint64_t* rdf;            /* [B,S,S,bins] */
  int64_t* rdf_samples;     /* [B] */
  double* vol_sum;          /* [B] A^3 */
} chg_md_observables_host;
/* The accumulators as they stand (nothing is reset); null pointers are skipped.  CHG_EINVAL for a handle without observers. */
int chg_md_download_observables(chg_engine* eng, chg_md* md, const chg_md_observables_host* out);
/* Tests only: n_samples caller-given snapshots -- positions [T,N,3], momenta [T,N,3], cell [T,B,9], status [T,B] -- through exactly
 * the kernels and the ring logic of a run, then the accumulators into out. */
int chg_test_md_observe(chg_engine* eng, const chg_md_observe_params* params, int32_t n_struct, const int32_t* atom_off,
                        const int32_t* species, const double* masses, int32_t n_samples, const double* positions, const double* momenta,
                        const double* cell, const int32_t* status, const chg_md_observables_host* out);

/* Transport accumulators (csrc/kernels_md_transport.h; tests/md_transport_ref.py restates them in NumPy) hang on observers with
 * n_lags = L > 0 and use their sample_interval, ring, subtract_com, species map and status rule: a replica that is not
 * CHG_MD_RUNNING is skipped for good.  For sample number k, replica o and every lag l in 0 .. min(k, L - 1), with
 *   u_i  = (r_i(k) - R_o(k)) - (r_i(k-l) - R_o(k-l))      the displacement the MSD is made of (R_o = 0 without subtract_com)
 *   U_a  = sum_{i in o, species a} u_i                     summed over the atoms in a fixed order, never as a difference of position sums
 *   J_a(k) = sum_{i in o, species a} p_i / m_i             raw velocities, as the VACF uses them; kept per sample in a ring [L,B,S,3]
 * the sums are
 *   msd4[o,l,s_i] += (|u_i|^2)^2                           (non_gaussian)
 *   cmsd[o,l,a,b] += U_a . U_b                             (collective; the full S x S block, symmetric bit for bit)
 *   jacf[o,l,a,b] += J_a(k) . J_b(k-l)                     (collective; not symmetric in a, b)
 *   vh[o, l / vh_stride, s_i, floor(|u_i| / vh_rmax * vh_bins)] += 1   if l % vh_stride == 0, l / vh_stride < vh_lags and
 *                                                          |u_i| < vh_rmax: integer counts, a displacement at or beyond vh_rmax is not counted
 * and per sample samples[o] += 1, vol_sum[o] += |det L| (the vol_sum of chg_md_observables_host exists only with an RDF and is left
 * alone).  cnt[o,l] of chg_md_observables_host normalises these sums too.  Float64, no floating-point atomics: every cell has one
 * owning workgroup, the histogram is counted in LDS (n_species * vh_bins <= 4096) and flushed once, so two runs of the same input
 * give the same bits.  chg_md_set_transport is valid after chg_md_set_observers and before the first run (a second call replaces the
 * first; a later chg_md_set_observers drops it); CHG_EINVAL with a message for: no observers or n_lags == 0; nothing requested;
 * vh_bins < 0; with vh_bins > 0 a vh_rmax that is not finite and positive, vh_stride < 1, vh_lags < 1, (vh_lags - 1) * vh_stride >= L
 * or n_species * vh_bins > 4096; a call after the first run.  CHG_ENOMEM when the accumulators (24 L B S bytes of ring,
 * 8 B L S (1 + 2 S) + 8 B vh_lags S vh_bins of sums) do not fit.  chg_md_free releases them.  A run without transport launches
 * exactly what it launched before it existed. */
typedef struct chg_md_transport_params {
  int32_t collective;       /* cmsd and jacf */
  int32_t non_gaussian;     /* msd4 */
  int32_t vh_bins;          /* 0: no van Hove histogram */
  int32_t vh_lags;          /* histograms kept: lags 0, vh_stride, .., (vh_lags - 1) vh_stride */
  int32_t vh_stride;
  int32_t reserved;
  double vh_rmax;           /* A, > 0 when vh_bins > 0 */
} chg_md_transport_params;
int chg_md_set_transport(chg_engine* eng, chg_md* md, const chg_md_transport_params* params);
typedef struct chg_md_transport_host {
  double* msd4;             /* [B,L,S]   */
  double* cmsd;             /* [B,L,S,S] */
  double* jacf;             /* [B,L,S,S] ASE velocity units squared */
  uint64_t* vh;             /* [B,vh_lags,S,vh_bins] */
  int64_t* samples;         /* [B] */
  double* vol_sum;          /* [B] A^3 */
} chg_md_transport_host;
/* The accumulators as they stand; null pointers and sums that were not requested are skipped.  CHG_EINVAL for a handle without transport. */
int chg_md_download_transport(chg_engine* eng, chg_md* md, const chg_md_transport_host* out);
/* Tests only: as chg_test_md_observe with the transport accumulators on top; plain (the sums of the observers) may be null. */
int chg_test_md_transport(chg_engine* eng, const chg_md_observe_params* params, const chg_md_transport_params* transport, int32_t n_struct,
                          const int32_t* atom_off, const int32_t* species, const double* masses, int32_t n_samples,
                          const double* positions, const double* momenta, const double* cell, const int32_t* status,
                          const chg_md_observables_host* plain, const chg_md_transport_host* out);

/* ---- Charge-informed MD: site magnetic moments per frame and charge-state observers (csrc/kernels_md_magmom.h; DESIGN.md "MD
 * observables -> Charge states"; tests/md_charge_ref.py restates the sums in NumPy) ------------------------------------------------
 * Both are opt-in; a handle that uses neither evaluates the task it always did and launches what it always launched.
 *
 * chg_md_set_magmoms adds CHG_TASK_M to what every evaluation of the handle predicts.  After every evaluation that COMPLETES a step
 * (step 0 included; not NPT Berendsen's first evaluation) one more launch copies the moments of every replica that wrote its frame --
 * CHG_MD_RUNNING and not held back for the wide-range retry, whose launch then writes them -- into an array of the last completed
 * step and, with log_frames, into a float [N] slot of the ring frame of that step.  A non-finite moment is stored as it is.  Valid
 * between create and the first run (a second call replaces the first); CHG_EINVAL with a message afterwards; CHG_ENOMEM when the
 * slots (4 N (ring_frames + 1) bytes) do not fit.  chg_md_params and chg_md_out_host keep their layout: the moments are read with
 * chg_md_download_magmoms -- magmom [N] of the last completed step (zeros before the first run), frame_magmom [K,N] of the oldest
 * min(frames in the ring, frame_capacity) frames in the order chg_md_download returns them (only with log_frames).  The ring is NOT
 * drained: call it before chg_md_download.  Null pointers are skipped.  CHG_EINVAL on a handle without chg_md_set_magmoms (the
 * charge-state observers below imply it without frame slots). */
int chg_md_set_magmoms(chg_engine* eng, chg_md* md, int32_t log_frames);
int chg_md_download_magmoms(chg_engine* eng, chg_md* md, float* magmom /* [N], may be null */, float* frame_magmom /* [K,N] */,
                            int32_t frame_capacity);

/* Charge-state observers hang on the observers (chg_md_set_observers; n_lags = L may be 0) and use their sample_interval, sample
 * number k, species map, ring index k % L and status rule; they imply CHG_TASK_M and the gather above.  Species s has n_bounds[s] in
 * 0..3 ascending boundaries bounds[s][0..n_bounds[s]) (mu_B, >= 0) and so 1..4 states; every array has Q = CHG_MD_CHARGE_STATES slots.
 * For sample k, a running replica o and atom i of species s, with m = (double)mag_i(k):
 *   q_i(k) = the number of boundaries of s that are <= m      (a moment exactly on a boundary belongs to the upper state)
 * An atom whose m is not finite has state -1: it is left out of every sum of that sample and of every lag pair it is part of, and
 * counted in skipped[o].  Otherwise
 *   mhist[o,s,floor(m / mag_max * mag_bins)] += 1   if 0 <= m < mag_max            (mag_bins > 0)
 *   msum[o,s] += m,  msq[o,s] += m^2                                               (summed over the atoms in a fixed order)
 *   pop[o,s,q_i(k)] += 1,  occ[i,q_i(k)] += 1
 *   trans[o,s,q_i(k-1),q_i(k)] += 1                 for k >= 1 and q_i(k-1) >= 0   (diagonal included)
 * and for every lag l in 0 .. min(k, L - 1), over the atoms with q_i(k) >= 0 and q_i(k-l) >= 0
 *   mcorr[o,l,s] += sum_i m_i(k) m_i(k-l)
 *   same[o,l,s,q] += the number of i with q_i(k-l) = q_i(k) = q
 * and, with srdf_bins > 0, for every atom i of species center_species with q_i(k) >= 0, every atom j of the replica (whatever its
 * moment) and every lattice shift n (i == j with n == 0 excluded) with d = |r_j - r_i + n L| < srdf_rmax
 *   shist[o,q_i(k),s_j,floor(d / srdf_rmax * srdf_bins)] += 1
 * with positions and cell of the snapshot the plain observers read; per sample samples[o] += 1 and vol_sum[o] += |det L|.  cnt[o,l]
 * of chg_md_observables_host normalises the lag sums.  Float64 and integers, no floating-point atomics, every float cell has one
 * owning workgroup: two runs of the same input give the same bits.  chg_md_set_charge_states is valid after chg_md_set_observers and
 * before the first run (a second call replaces the first; a later chg_md_set_observers drops it); CHG_EINVAL with a message for: no
 * observers; n_bounds outside 0..3; boundaries that are not finite, not ascending or negative; nothing requested (no boundary,
 * mag_bins == 0 and srdf_bins == 0); mag_bins < 0 or n_species * mag_bins > 4096; with mag_bins > 0 a mag_max that is not finite and
 * positive; srdf_bins < 0 or Q * n_species * srdf_bins > 16384; srdf_bins > 0 without a center_species in 0 .. n_species - 1 or a
 * finite positive srdf_rmax; a call after the first run.  CHG_ENOMEM when the ring (12 L N bytes) and the sums do not fit. */
#define CHG_MD_CHARGE_STATES 4
#define CHG_MD_CHARGE_BOUNDS 3
typedef struct chg_md_charge_params {
  int32_t n_bounds[8];      /* per species, 0..3; entries from n_species on are ignored */
  int32_t mag_bins;         /* 0: no moment histogram */
  int32_t center_species;   /* -1: none */
  int32_t srdf_bins;        /* 0: no state-resolved RDF */
  int32_t reserved;
  double mag_max;           /* mu_B, > 0 when mag_bins > 0 */
  double srdf_rmax;         /* A, > 0 when srdf_bins > 0 */
} chg_md_charge_params;
int chg_md_set_charge_states(chg_engine* eng, chg_md* md, const chg_md_charge_params* params, const double* bounds /* [S,3] */);
typedef struct chg_md_charge_host {
  uint64_t* mhist;          /* [B,S,mag_bins] */
  double* msum;             /* [B,S] */
  double* msq;              /* [B,S] */
  int64_t* pop;             /* [B,S,Q] */
  int64_t* trans;           /* [B,S,Q,Q] from, to */
  int64_t* occ;             /* [N,Q] */
  double* mcorr;            /* [B,L,S] */
  int64_t* same;            /* [B,L,S,Q] */
  uint64_t* shist;          /* [B,Q,S,srdf_bins] */
  int64_t* samples;         /* [B] */
  int64_t* skipped;         /* [B] */
  double* vol_sum;          /* [B] A^3 */
} chg_md_charge_host;
/* The accumulators as they stand; null pointers are skipped.  CHG_EINVAL for a handle without charge-state observers. */
int chg_md_download_charge_states(chg_engine* eng, chg_md* md, const chg_md_charge_host* out);
/* Tests only: chg_test_md_observe plus the moments magmoms [T,N] of every snapshot, through exactly the ring logic and kernels of a
 * run; plain (the sums of the observers) may be null. */
int chg_test_md_charge_states(chg_engine* eng, const chg_md_observe_params* params, const chg_md_charge_params* charge, const double* bounds,
                              int32_t n_struct, const int32_t* atom_off, const int32_t* species, const double* masses, int32_t n_samples,
                              const double* positions, const double* momenta, const double* cell, const int32_t* status,
                              const float* magmoms, const chg_md_observables_host* plain, const chg_md_charge_host* out);

/* ---- canonical Monte Carlo: species swaps and single-atom displacements, every structure an independent replica -----------------
 * Not in the reference.  Every replica has a fixed cell, its own temperature (K, >= 0; 0 is greedy descent) and its own 64-bit seed; its
 * float64 state lives in HBM.  One trial = graph built on the device from all replicas + energy-only prediction
 * (chg_batch_build_predict, CHG_TASK_E) + one step kernel (csrc/kernels_mc.h) that decides the pending trial by the Metropolis rule and
 * proposes the next one.  Atoms keep their species: a swap exchanges the POSITIONS of two atoms of different species, and site[a] is the
 * input row atom a now sits on.  The random numbers of trial k are Philox4x32-10 blocks with counter (k, b, 0, 1) and the seed as key, so a
 * replica's stream depends on (seed, k) alone: not on its slot in the batch, on retries or on how chg_mc_run calls split the trials.
 * DESIGN.md "Monte Carlo" states the semantics exactly; tests/mc_ref.py restates them in NumPy. */
enum { CHG_MC_RUNNING = 0, CHG_MC_NONFINITE = 1 };
enum { CHG_MC_NONE = -1, CHG_MC_SWAP = 0, CHG_MC_DISPLACE = 1 };   /* move kinds; NONE: the frame of the configuration as given */
typedef struct chg_mc_params {
  double swap_probability;     /* a trial is a swap iff u_kind < swap_probability: 1 always swaps, 0 never does                */
  double max_displacement;     /* A: a displacement is max_displacement (2 u - 1) per cartesian component                     */
  double kB;                   /* eV/K; <= 0: 8.6173303e-5                                                                    */
  int32_t loginterval;         /* a frame after every loginterval-th decision, the initial configuration included; 0: none    */
  int32_t ring_frames;         /* frames the device ring holds between two chg_mc_download calls                              */
  double r_atom, r_bond, numerical_tol;                /* graph build (6, 3, 1e-8)                                             */
} chg_mc_params;
typedef struct chg_mc chg_mc;
#define CHG_MC_COUNTS 8        /* int64 per replica: swap trials, swap acceptances, displacement trials, displacement acceptances, samples, 3 spare */
#define CHG_MC_FRAME_SCALARS 6 /* doubles per replica and frame: E_cur, E_trial (eV, total), u_acc, delta[3] (A)                 */
#define CHG_MC_FRAME_MOVES 6   /* ints per replica and frame: trials decided, kind (CHG_MC_*), i, j, accepted, spare             */
/* Current state, statistics and best configuration (null pointers are skipped) and up to frame_capacity of the oldest frames in the
 * ring, which are removed from it.  Energies are totals in eV (an intensive model's eV/atom times the atom count). */
typedef struct chg_mc_out_host {
  double* positions;           /* [N,3]   cartesian, A: atom order kept, positions moved                                     */
  int32_t* site;               /* [N]     input row (within the replica) atom a sits on                                      */
  double* energy;              /* [B]     E_cur                                                                               */
  double* temperatures;        /* [B]     K                                                                                   */
  int32_t* status;             /* [B]     CHG_MC_*                                                                            */
  int32_t* n_trials;           /* [B]     trials proposed                                                                     */
  int64_t* counts;             /* [B,CHG_MC_COUNTS]                                                                           */
  double* sums;                /* [B,2]   sum of E_cur and of E_cur^2 over the samples (one after every decision)             */
  double* best_energy;         /* [B]     lowest energy seen ...                                                              */
  double* best_positions;      /* [N,3]   ... with its positions ...                                                          */
  int32_t* best_site;          /* [N]     ... and site[]                                                                      */
  int32_t frame_capacity;      /* K: frames the arrays below hold                                                             */
  int32_t* n_frames;           /* out: frames written                                                                         */
  int32_t* frame_trial;        /* [K]     trials decided when the frame was written                                           */
  double* frame_scalars;       /* [K,B,CHG_MC_FRAME_SCALARS]                                                                  */
  int32_t* frame_moves;        /* [K,B,CHG_MC_FRAME_MOVES] the last move's record                                             */
  double* frame_positions;     /* [K,N,3]                                                                                     */
  int32_t* frame_site;         /* [K,N]                                                                                       */
} chg_mc_out_host;
/* Copies the structures, temperatures [B], seeds [B] and the two per-atom masks [N] (swap_mask: 1 = the atom's species may swap, null:
 * all; fixed: 1 = the atom is held, null: none); no evaluation yet.  The atom lists are fixed here: movable = atoms not held, in atom
 * order; swappable = movable atoms whose swap_mask is set, sorted by (species, atom).  CHG_EINVAL with a message naming the structure
 * when swap_probability > 0 and its swappable list holds fewer than two species, or swap_probability < 1 and its movable list is empty. */
int chg_mc_create(chg_engine* eng, const chg_structs_host* host, const double* temperatures, const uint64_t* seeds, const uint8_t* swap_mask,
                  const uint8_t* fixed, const chg_mc_params* params, chg_mc** out);
/* New temperatures [B] (K, >= 0) for the trials decided from now on: callable between runs (annealing schedules). */
int chg_mc_set_temperatures(chg_engine* eng, chg_mc* mc, const double* temperatures);
/* n_trials trials of every replica (the first call evaluates the configuration as given first: it sets E_cur and the best record, writes
 * frame 0 and is neither a trial nor a sample).  A batch with a non-finite energy is evaluated again on the wide-range sweep; a replica
 * that is non-finite even there stops as CHG_MC_NONFINITE with its configuration and statistics untouched.  CHG_EINVAL (nothing run)
 * when the frames due do not fit the ring. */
int chg_mc_run(chg_engine* eng, chg_mc* mc, int32_t n_trials);
int chg_mc_download(chg_engine* eng, chg_mc* mc, const chg_mc_out_host* out);
int chg_mc_free(chg_engine* eng, chg_mc* mc);
/* Tests only: ONE step kernel launch on caller-given state, in place.  flags: 1 absorb the evaluation of the pending trial (energy [B]
 * as the engine gives it: eV/atom when `intensive`), 2 propose the next trial.  z [N] are the species the lists are built from, with
 * swap_mask and fixed as in chg_mc_create.  State: r [N,3], site [N]; sd [B,32] doubles (L[9], L^-1[9], E_cur, E_best, sumE, sumE2, E_trial
 * of the last decision, pending u_acc, pending delta[3], spare); si [B,8] ints (trials proposed, status, first evaluation absorbed,
 * pending kind, i, j, last decision accepted, spare); counts [B,CHG_MC_COUNTS]; best_positions, best_site.  Out: frac_next [N,3],
 * retry [B] (1: non-finite energy with final_try == 0, state untouched), and the frame arrays of one slot (all four or none). */
int chg_test_mc_step(chg_engine* eng, const chg_mc_params* params, int32_t n_struct, const int32_t* atom_off, const int32_t* z,
                     const uint8_t* swap_mask, const uint8_t* fixed, const double* temperatures, const uint64_t* seeds, int32_t flags,
                     int32_t final_try, int32_t intensive, double* r, int32_t* site, double* sd, int32_t* si, int64_t* counts,
                     double* best_positions, int32_t* best_site, const float* energy, double* frac_next, int32_t* retry,
                     double* frame_scalars, int32_t* frame_moves, double* frame_positions, int32_t* frame_site);
/* Replica exchange (parallel tempering; DESIGN.md "Monte Carlo", part "Replica exchange"; tests/mc_exchange_ref.py restates it).
 * ladder [B]: replicas that follow one another with the same id >= 0 form a tempering ladder, -1 is never exchanged.  A rung is a batch
 * slot: it keeps its temperature, seed, stream, counters, sums and best record; an accepted exchange moves the configuration (positions,
 * site[], E_cur) and its walker id between two neighbouring rungs.  With t the trials the handle has decided, exchange event m =
 * t / interval follows the decisions of every trial with t % interval == 0, the last trial of a chg_mc_run call included, and pairs the
 * rungs (p, p + 1) with p % 2 == (m - 1) & 1.  A pair with a member that is not CHG_MC_RUNNING is skipped.  Otherwise, a the lower
 * and b the upper replica: accept iff D >= 0 or u < exp(D), D = (1/(kB T_a) - 1/(kB T_b)) (E_cur,a - E_cur,b), u the first uniform of
 * Philox4x32-10(counter (m, 0, 0, 2), key seed_a).  interval 0 switches the events off.  The exchange state is an allocation of its
 * own, freed by chg_mc_free.  CHG_EINVAL, naming the replica and changing nothing: an id that reappears after another one, a ladder of
 * one replica, members that differ in atom count, species array, lattice (bit for bit), fixed or swap_mask, a member with T <= 0,
 * interval < 0, a call after the handle's first chg_mc_run.  From then on chg_mc_set_temperatures refuses T <= 0 for ladder members. */
#define CHG_MC_EXCHANGE_INTS 6 /* int32 per replica: walker held (ladder-local lineage id, the rung index at the start), exchange attempts and
                                  acceptances of the pair (this rung, the next one) | mark (0 none, 1 bottom, 2 top) and completed
                                  bottom -> top -> bottom round trips of walker w of the ladder at row first + w | spare                  */
int chg_mc_set_exchange(chg_engine* eng, chg_mc* mc, const int32_t* ladder /*[B]*/, int32_t interval);
int chg_mc_download_exchange(chg_engine* eng, chg_mc* mc, int32_t* xi /*[B,CHG_MC_EXCHANGE_INTS]*/);
/* Tests only: exchange event m (>= 1) on caller-given state, in place, pair lists built by the host code of chg_mc_set_exchange (which
 * here checks ids, ladder lengths, atom counts and T > 0).  r, site, sd, si, best_positions, best_site as in chg_test_mc_step; xi
 * [B,CHG_MC_EXCHANGE_INTS]. */
int chg_test_mc_exchange(chg_engine* eng, int32_t n_struct, const int32_t* atom_off, const int32_t* ladder, const double* temperatures,
                         const uint64_t* seeds, double kB, int32_t m, double* r, int32_t* site, double* sd, int32_t* si,
                         double* best_positions, int32_t* best_site, int32_t* xi);

/* ---- nudged elastic band: batched bands, improved tangents, climbing image, one FIRE optimizer per band ------------------------
 * A band is M images (3 <= M <= 66) that share one fixed cell and one species order; images 0 and M-1 never move.  The state holds the
 * UNWRAPPED cartesian positions frac . L of every image in float64: the caller applies the minimum image when it interpolates, the step
 * takes plain differences between neighbouring images.  Every image of every band is an independent structure for the graph build and
 * the force sweep (chg_batch_build_predict, task ef); the first evaluation predicts all images, every later one the interior images of
 * the bands still running, and one step kernel (csrc/kernels_neb.h, one workgroup per band) follows it.  For interior image i with
 * t+ = R[i+1] - R[i], t- = R[i] - R[i-1] and the engine's f32 energies E compared as they are:
 *   tau = t+ when E[i+1] > E[i] > E[i-1], t- when E[i+1] < E[i] < E[i-1]; otherwise, dmax / dmin the larger / smaller of |E[i+1] - E[i]|
 *   and |E[i-1] - E[i]|: t+ dmax + t- dmin when E[i+1] > E[i-1], else t+ dmin + t- dmax (ties take these branches); tau is normalised
 *   (a tangent of length 0 stays 0);  G[i] = F[i] - (F[i] . tau) tau + spring (|t+| - |t-|) tau;  with `climb` the interior image of
 *   highest energy (first index on ties, chosen anew at every evaluation) takes G = F - 2 (F . tau) tau instead.
 * Held components (chg_neb_set_fixed) of F count as 0 before the projection, those of G are zeroed after it.  FIRE as in
 * chg_relax_params runs over the concatenated interior rows of a band (maxstep clamps the norm of the whole band's step); the band is
 * converged when the largest row norm of G at the evaluated configuration is below fmax.  Statuses are CHG_RELAX_*.  A band with a
 * non-finite energy or force in any evaluated image is held back as a whole; the batch is evaluated again on the wide-range sweep and
 * a band that is non-finite even there stops as CHG_RELAX_NONFINITE, untouched.  DESIGN.md "Nudged elastic band"; tests/neb_ref.py
 * restates the step in float64 NumPy. */
typedef struct chg_neb_params {
  double fmax;
  int32_t max_steps, climb;
  double dt, maxstep, dtmax, finc, fdec, astart, fa;   /* ASE FIRE: 0.1, 0.2, 1.0, 1.1, 0.5, 0.1, 0.99                          */
  int32_t nmin, reserved;                              /* 5, 0                                                                  */
  double spring;                                       /* eV/A^2 (0.1)                                                          */
  double r_atom, r_bond, numerical_tol;                /* graph build (6, 3, 1e-8)                                              */
} chg_neb_params;
typedef struct chg_neb chg_neb;
/* Null pointers are skipped.  B images, N atoms, n_bands bands, all in the order they were given. */
typedef struct chg_neb_out_host {
  double* frac;             /* [N,3] fractional coordinates of the last evaluated configuration (end points: as given, bit for bit) */
  float* energy;            /* [B]   as last evaluated, eV/atom if is_intensive else eV                                               */
  float* force;             /* [N,3] the engine's force of the last evaluated configuration, eV/A (not projected, not masked)          */
  double* neb_fmax;         /* [n_bands] largest row norm of G at the last evaluated configuration                                   */
  int32_t* climbing_image;  /* [n_bands] index within the band, -1: none                                                             */
  int32_t* n_steps;         /* [n_bands] optimizer steps taken                                                                       */
  int32_t* status;          /* [n_bands] CHG_RELAX_*                                                                                 */
  int32_t* n_evaluated;     /* [n_bands] structures of the band predicted so far                                                     */
} chg_neb_out_host;
/* host: the images band after band; band_off [n_bands + 1]: image offsets, from 0 to host->n_struct.  Copies everything; no evaluation
 * yet.  CHG_EINVAL with a message: a band with fewer than 3 or more than 66 images; images of a band that differ in atom count,
 * species or cell (bit for bit).  CHG_ENOMEM when the state cannot be allocated. */
int chg_neb_create(chg_engine* eng, const chg_structs_host* host, const int32_t* band_off, int32_t n_bands, const chg_neb_params* params,
                   chg_neb** out);
/* The mask [N,3] over all images (1 = component held; null: none), valid until the first chg_neb_run. */
int chg_neb_set_fixed(chg_engine* eng, chg_neb* neb, const uint8_t* fixed);
/* Up to n_steps evaluations, each followed by a step of every band still running; *n_active = bands still running (0: done). */
int chg_neb_run(chg_engine* eng, chg_neb* neb, int32_t n_steps, int32_t* n_active);
int chg_neb_download(chg_engine* eng, chg_neb* neb, const chg_neb_out_host* out);
int chg_neb_free(chg_engine* eng, chg_neb* neb);
/* Tests only: ONE launch of the step kernel on caller-given state and results, in place.  atom_off [B + 1] over the images, band_off as
 * above.  State: r, v, g [N,3]; sd [n_bands,24] doubles (L[9], L^-1[9], dt, a, neb_fmax, 3 spare); si [n_bands,4] ints (FIRE Nsteps,
 * steps taken, status, climbing image); e_img [B] the energies the state holds (the end points' are read when all_images == 0).
 * Results: all_images 1: energy [B] and force [N,3] of every image; 0: of the interior images only, band after band.  final_try 0: a
 * band with non-finite results is left untouched and retry[band] is set to 1 (retry [n_bands] is in / out, the caller zeroes it);
 * 1: it stops as CHG_RELAX_NONFINITE.  fixed [N,3] or null.  out: frac_next [N,3], of which the first sum (M - 2) n rows are
 * written: the interior images of the bands that moved, band after band. */
int chg_test_neb_step(chg_engine* eng, const chg_neb_params* params, int32_t n_bands, const int32_t* band_off, const int32_t* atom_off,
                      double* r, double* v, double* g, double* sd, int32_t* si, float* e_img, const float* energy, const float* force,
                      int32_t all_images, int32_t final_try, const uint8_t* fixed, double* frac_next, int32_t* retry);

/* ---- dimer saddle search: batched searches from one basin, rotation by a trial angle, one FIRE optimizer per search --------------
 * A search is a centre R (n atoms, one fixed cell, UNWRAPPED cartesian positions frac . L in float64) and a unit axis N over all 3 n
 * components.  Every image of every search is an independent structure for the graph build and the force sweep
 * (chg_batch_build_predict, task ef).  An evaluation in phase PROBE (0) predicts R and R + delta N of a search, one in phase TRIAL (1)
 * predicts R + delta N* alone, N* = N cos phi1 + Theta sin phi1: the centre stands still during rotations and its force F0 is kept.
 * One step kernel (csrc/kernels_dimer.h, one workgroup per search) follows every evaluation, on float64 copies of the engine's f32
 * forces:
 *   TRIAL: Ct = (F0 - F1t).N* / delta, b1 = -gn, a1 = (C0 - Ct + b1 sin 2 phi1) / (1 - cos 2 phi1), phim = atan2(b1, a1) / 2, moved by
 *   pi/2 (towards 0) when it is a maximum of the fit C0 - a1 + a1 cos 2 phi + b1 sin 2 phi;  F1 <- sin(phi1 - phim) / sin(phi1) F1 +
 *   sin(phim) / sin(phi1) F1t + (1 - cos phim - sin phim tan(phi1 / 2)) F0;  N <- normalise(N cos phim + Theta sin phim)
 *   then, in both phases: d = F1 - F0, C0 = -(d.N) / delta (curvature along N, eV/A^2), g = (d - (d.N) N) / delta, gn = |g|,
 *   phi1 = atan2(gn, |C0|) / 2;  while fewer than max_rotations rotations were made since the last translation and phi1 >= angle_tol:
 *   Theta = g / gn and the next evaluation is a TRIAL
 *   otherwise the translation: CHG_RELAX_CONVERGED when C0 < 0 and the largest row norm of F0 is below fmax, CHG_RELAX_MAX_STEPS after
 *   max_steps translations, else one FIRE step (as in chg_relax_params, over all 3 n components, maxstep clamps the whole step) on
 *   G = F0 - 2 (F0.N) N when C0 < 0, G = -(F0.N) N otherwise; the next evaluation is a PROBE.
 * Held components (chg_dimer_set_fixed) of N are zeroed before N is normalised, those of every evaluated force count as 0.  A search
 * with a non-finite energy or force in an evaluated image is held back as a whole; the batch is evaluated again on the wide-range
 * sweep and a search that is non-finite even there stops as CHG_RELAX_NONFINITE, untouched.  Statuses are CHG_RELAX_*.  DESIGN.md
 * "Dimer saddle search"; tests/dimer_ref.py restates the step in float64 NumPy. */
typedef struct chg_dimer_params {
  double fmax;
  int32_t max_steps, max_rotations;                    /* translations; rotations per translation, 0..32 (4)                    */
  double dt, maxstep, dtmax, finc, fdec, astart, fa;   /* ASE FIRE: 0.1, 0.2, 1.0, 1.1, 0.5, 0.1, 0.99                          */
  int32_t nmin, reserved;                              /* 5, 0                                                                  */
  double delta, angle_tol;                             /* A in (0, 0.5] (0.01); rad in [1e-4, pi/4) (0.05)                      */
  double r_atom, r_bond, numerical_tol;                /* graph build (6, 3, 1e-8)                                              */
} chg_dimer_params;
typedef struct chg_dimer chg_dimer;
/* Null pointers are skipped.  S searches, N atoms, in the order they were given. */
typedef struct chg_dimer_out_host {
  double* frac;           /* [N,3] fractional coordinates R L^-1 of the centre (unwrapped)                                        */
  double* mode;           /* [N,3] the axis N                                                                                     */
  double* force;          /* [N,3] F0: the engine's force at the last evaluated centre, eV/A, held components 0                   */
  float* image_energy;    /* [S,2] as last evaluated, eV/atom if is_intensive else eV: the centre (at the last PROBE), then the    */
                          /*       displaced image (PROBE) or the trial image (TRIAL)                                             */
  float* image_force;     /* [2N,3] the engine's forces of the same two images, eV/A, not masked: search k owns rows               */
                          /*       2 atom_off[k] .. 2 atom_off[k+1], the centre first                                             */
  double* curvature;      /* [S]   C0, eV/A^2                                                                                     */
  double* fmax;           /* [S]   largest row norm of F0                                                                         */
  int32_t* n_steps;       /* [S]   translations taken                                                                             */
  int32_t* n_rotations;   /* [S]   rotations made in all                                                                          */
  int32_t* n_evaluated;   /* [S]   structures of the search predicted so far                                                      */
  int32_t* status;        /* [S]   CHG_RELAX_*                                                                                    */
  int32_t* phase;         /* [S]   what the next evaluation of the search predicts: 0 PROBE, 1 TRIAL                              */
} chg_dimer_out_host;
/* host: the centres; mode [N,3]: one direction per search, normalised here.  Copies everything; no evaluation yet.  CHG_EINVAL with a
 * message: delta, max_rotations or angle_tol outside their ranges; a mode that is zero or not finite.  CHG_ENOMEM when the state
 * cannot be allocated. */
int chg_dimer_create(chg_engine* eng, const chg_structs_host* host, const double* mode, const chg_dimer_params* params, chg_dimer** out);
/* The mask [N,3] (1 = component held; null: none), valid until the first chg_dimer_run.  CHG_EINVAL with a message, the handle
 * unchanged, when a mode has no free component. */
int chg_dimer_set_fixed(chg_engine* eng, chg_dimer* dimer, const uint8_t* fixed);
/* Up to n_evaluations evaluations, each followed by a step of every search still running; *n_active = searches still running. */
int chg_dimer_run(chg_engine* eng, chg_dimer* dimer, int32_t n_evaluations, int32_t* n_active);
int chg_dimer_download(chg_engine* eng, chg_dimer* dimer, const chg_dimer_out_host* out);
int chg_dimer_free(chg_engine* eng, chg_dimer* dimer);
/* Tests only: ONE launch of the step kernel on caller-given state and results, in place.  atom_off [S + 1].  State: r, nvec, theta, v,
 * f0, f1 [N,3]; sd [S,24] doubles (L[9], L^-1[9], dt, a, C0, gn, phi1, fmax); si [S,8] ints (FIRE Nsteps, translations, status, phase,
 * rotations since the last translation, rotations in all, 2 spare); e_img [S,2] and f_img [2N,3] as image_energy and image_force of
 * chg_dimer_out_host.  Results, search after search: energy and force of two
 * structures (R, R + delta N) where si says PROBE, of one where it says TRIAL (stopped searches included).  final_try 0: a search with
 * non-finite results is left untouched and retry[search] is set to 1 (retry [S] is in / out, the caller zeroes it); 1: it stops as
 * CHG_RELAX_NONFINITE.  fixed [N,3] or null.  out: frac_next [2 N,3], search k owns rows 2 atom_off[k] .. 2 atom_off[k + 1] and
 * writes the first 2 n of them (next phase PROBE), the first n (TRIAL) or none (stopped, held back); phase_next, status_next [S]. */
int chg_test_dimer_step(chg_engine* eng, const chg_dimer_params* params, int32_t n_searches, const int32_t* atom_off, double* r, double* nvec,
                        double* theta, double* v, double* f0, double* f1, double* sd, int32_t* si, float* e_img, float* f_img,
                        const float* energy, const float* force, int32_t final_try, const uint8_t* fixed, double* frac_next,
                        int32_t* phase_next, int32_t* status_next, int32_t* retry);

/* ---- exchange steps of the multi-GPU path, straight on RCCL (one communicator per process = per GPU) ----------
 * The reference is single-device; these carry what SURVEY 8e needs and nothing else: the all-gather of per-structure
 * energies after a sweep sharded over independent structures, and the sum of the 412,525-float parameter gradient of a
 * data-parallel train step (the slot is loss.backward() -> optimizer.step(), chgnet/trainer/trainer.py:399-411).
 * librccl is opened at run time (CHG_EUNSUPPORTED when it is missing).  Rank 0 calls chg_comm_unique_id and hands the
 * CHG_COMM_ID_BYTES bytes to the other ranks by any means (chgnet_amd/distributed.py uses a TCP socket on MASTER_ADDR);
 * every rank then calls chg_comm_create.  Buffers are HOST pointers; counts are per rank; all calls block until done.
 * all_gather: recv holds world * count floats in rank order. */
#define CHG_COMM_ID_BYTES 128
typedef struct chg_comm chg_comm;
int chg_comm_unique_id(uint8_t* id_out);
int chg_comm_create(const uint8_t* id, int32_t rank, int32_t world, int32_t device, chg_comm** out);
int chg_comm_all_gather_f32(chg_comm* comm, const float* send, int64_t count, float* recv);
int chg_comm_all_reduce_sum_f32(chg_comm* comm, float* data, int64_t count);
/* Device-pointer forms, enqueued on `stream` (a hipStream_t, e.g. chg_engine_stream) without synchronisation: the two
 * exchange steps of the path act on buffers that already live in HBM (per-structure energies, the gradient blob). */
int chg_comm_all_gather_f32_device(chg_comm* comm, const float* d_send, int64_t count, float* d_recv, void* stream);
int chg_comm_all_reduce_sum_f32_device(chg_comm* comm, float* d_data, int64_t count, void* stream);
int chg_comm_reserve(chg_comm* comm, int64_t floats, float** device_ptr);   /* grow-only device staging of the communicator */
int chg_comm_info(chg_comm* comm, int32_t* rank, int32_t* nranks, int32_t* device);   /* nranks = ncclCommCount */
int chg_comm_barrier(chg_comm* comm);
int chg_comm_destroy(chg_comm* comm);
const char* chg_comm_last_error(const chg_comm* comm);   /* NULL: the error of the last failed call without a communicator */

#ifdef __cplusplus
}
#endif
#endif /* CHGNET_HIP_H */
