"""ctypes binding of libchgnet_hip.so (include/chgnet_hip.h).  No fallback: a missing or
unloadable library raises ``RuntimeError`` -- the product never computes on the CPU."""

from __future__ import annotations

import ctypes
import os

c_int_p = ctypes.POINTER(ctypes.c_int32)
c_float_p = ctypes.POINTER(ctypes.c_float)

TASK_BITS = {"e": 1, "f": 2, "s": 4, "m": 8}

EXPORTED_SYMBOLS = (
    "chg_abi_version", "chg_device_count", "chg_weights_required", "chg_engine_create", "chg_engine_destroy", "chg_last_error",
    "chg_batch_upload", "chg_batch_build", "chg_batch_build_predict", "chg_debug_fetch_i32", "chg_batch_update_geometry", "chg_batch_free", "chg_batch_device_bytes",
    "chg_predict", "chg_synchronize", "chg_batch_download", "chg_timer_start", "chg_timer_stop_ms",
    "chg_profile_enable", "chg_profile_reset", "chg_profile_count", "chg_profile_read",
    "chg_debug_fetch", "chg_test_rows_gemm", "chg_test_split_gemm",
    "chg_engine_set_memory_limit", "chg_engine_memory_info", "chg_batch_bytes_required",
    "chg_stream_copy", "chg_backward", "chg_engine_build_stats", "chg_engine_update_weights",
    "chg_engine_set_graph_search", "chg_engine_cell_stats",
    "chg_comm_unique_id", "chg_comm_create", "chg_comm_all_gather_f32", "chg_comm_all_reduce_sum_f32", "chg_comm_barrier",
    "chg_comm_destroy", "chg_comm_last_error",
    "chg_comm_all_gather_f32_device", "chg_comm_all_reduce_sum_f32_device", "chg_comm_reserve", "chg_comm_info",
    "chg_backward_allreduce", "chg_batch_all_gather_energy", "chg_engine_stream", "chg_engine_device",
    "chg_host_alloc", "chg_host_free",
    "chg_relax_create", "chg_relax_run", "chg_relax_download", "chg_relax_free", "chg_test_relax_step",
    "chg_relax_create_lbfgs", "chg_test_lbfgs_step",
    "chg_md_create", "chg_md_run", "chg_md_download", "chg_md_free", "chg_test_md_step",
    "chg_md_create_langevin", "chg_test_md_step_langevin",
    "chg_md_create_nhc", "chg_md_download_nhc", "chg_test_md_step_nhc",
    "chg_md_create_nhc_flex", "chg_md_download_vg", "chg_test_md_step_nhc_flex",
    "chg_hessian_vector", "chg_hessian_vector_strain",
    "chg_relax_set_fixed", "chg_md_set_fixed", "chg_test_relax_step_fixed", "chg_test_lbfgs_step_fixed", "chg_test_md_step_fixed",
    "chg_md_set_observers", "chg_md_download_observables", "chg_test_md_observe",
    "chg_md_set_transport", "chg_md_download_transport", "chg_test_md_transport",
    "chg_md_set_magmoms", "chg_md_download_magmoms",
    "chg_md_set_charge_states", "chg_md_download_charge_states", "chg_test_md_charge_states",
    "chg_mc_create", "chg_mc_set_temperatures", "chg_mc_run", "chg_mc_download", "chg_mc_free", "chg_test_mc_step",
    "chg_mc_set_exchange", "chg_mc_download_exchange", "chg_test_mc_exchange",
    "chg_neb_create", "chg_neb_set_fixed", "chg_neb_run", "chg_neb_download", "chg_neb_free", "chg_test_neb_step",
    "chg_dimer_create", "chg_dimer_set_fixed", "chg_dimer_run", "chg_dimer_download", "chg_dimer_free", "chg_test_dimer_step",
)


class ModelDesc(ctypes.Structure):
    _fields_ = [
        ("n_conv", ctypes.c_int32), ("cutoff_coeff", ctypes.c_int32), ("is_intensive", ctypes.c_int32),
        ("has_composition", ctypes.c_int32), ("atom_graph_cutoff", ctypes.c_float),
        ("bond_graph_cutoff", ctypes.c_float), ("n_weights", ctypes.c_int64),
        ("n_mlp_hidden", ctypes.c_int32), ("mlp_out_bias", ctypes.c_int32),
    ]


class BatchHost(ctypes.Structure):
    _fields_ = [
        ("n_struct", ctypes.c_int32), ("n_atoms", ctypes.c_int32), ("n_directed", ctypes.c_int32),
        ("n_undirected", ctypes.c_int32), ("n_angles", ctypes.c_int32), ("n_bnodes", ctypes.c_int32),
        ("z", c_int_p), ("frac", c_float_p), ("lattice", c_float_p), ("atom_owner", c_int_p), ("atom_off", c_int_p),
        ("e_center", c_int_p), ("e_nbr", c_int_p), ("e_image", c_float_p), ("e_d2u", c_int_p), ("e_owner", c_int_p),
        ("e_rev", c_int_p), ("p_center", c_int_p), ("p_nbr", c_int_p),
        ("u_u2d", c_int_p), ("u_bnode", c_int_p), ("bn_und", c_int_p),
        ("a_ctr", c_int_p), ("a_b1c", c_int_p), ("a_b2c", c_int_p), ("a_d1", c_int_p), ("a_d2", c_int_p),
    ]


class StructsHost(ctypes.Structure):
    _fields_ = [("n_struct", ctypes.c_int32), ("n_atoms", ctypes.c_int32), ("z", c_int_p),
                ("frac", ctypes.POINTER(ctypes.c_double)), ("lattice", ctypes.POINTER(ctypes.c_double)), ("atom_off", c_int_p)]


class OutHost(ctypes.Structure):
    _fields_ = [(n, c_float_p) for n in ("energy", "force", "stress", "magmom", "site_energy", "atom_fea", "crystal_fea")]


class RelaxParams(ctypes.Structure):
    _fields_ = [("fmax", ctypes.c_double), ("max_steps", ctypes.c_int32), ("relax_cell", ctypes.c_int32),
                ("dt", ctypes.c_double), ("maxstep", ctypes.c_double), ("dtmax", ctypes.c_double), ("finc", ctypes.c_double),
                ("fdec", ctypes.c_double), ("astart", ctypes.c_double), ("fa", ctypes.c_double), ("nmin", ctypes.c_int32),
                ("exp_cell_factor", ctypes.c_double), ("r_atom", ctypes.c_double), ("r_bond", ctypes.c_double),
                ("numerical_tol", ctypes.c_double), ("stress_weight", ctypes.c_double)]


class LbfgsParams(ctypes.Structure):
    _fields_ = [("maxstep", ctypes.c_double), ("damping", ctypes.c_double), ("alpha", ctypes.c_double), ("memory", ctypes.c_int32),
                ("reserved", ctypes.c_int32)]


class RelaxOutHost(ctypes.Structure):
    _fields_ = [("frac", ctypes.POINTER(ctypes.c_double)), ("lattice", ctypes.POINTER(ctypes.c_double)), ("energy", c_float_p),
                ("force", c_float_p), ("stress", c_float_p), ("magmom", c_float_p), ("n_steps", c_int_p), ("status", c_int_p)]


class MdParams(ctypes.Structure):
    _fields_ = [("ensemble", ctypes.c_int32), ("fixcm", ctypes.c_int32), ("dt", ctypes.c_double), ("temperature", ctypes.c_double),
                ("taut", ctypes.c_double), ("taup", ctypes.c_double), ("pressure", ctypes.c_double), ("compressibility", ctypes.c_double),
                ("kB", ctypes.c_double), ("stress_weight", ctypes.c_double), ("loginterval", ctypes.c_int32), ("ring_frames", ctypes.c_int32),
                ("log_stress", ctypes.c_int32), ("log_crystal_fea", ctypes.c_int32), ("r_atom", ctypes.c_double), ("r_bond", ctypes.c_double),
                ("numerical_tol", ctypes.c_double)]


class MdOutHost(ctypes.Structure):
    _dp = ctypes.POINTER(ctypes.c_double)
    _fields_ = [("positions", _dp), ("momenta", _dp), ("cell", _dp), ("n_steps", c_int_p), ("status", c_int_p),
                ("frame_capacity", ctypes.c_int32), ("n_frames", c_int_p), ("frame_step", c_int_p), ("frame_scalars", _dp),
                ("frame_positions", _dp), ("frame_momenta", _dp), ("frame_cell", _dp), ("frame_force", c_float_p),
                ("frame_stress", c_float_p), ("frame_crystal_fea", c_float_p)]


class MdObserveParams(ctypes.Structure):
    _fields_ = [("sample_interval", ctypes.c_int32), ("n_lags", ctypes.c_int32), ("subtract_com", ctypes.c_int32),
                ("n_species", ctypes.c_int32), ("rdf_bins", ctypes.c_int32), ("reserved", ctypes.c_int32), ("rdf_rmax", ctypes.c_double)]


class MdObservablesHost(ctypes.Structure):
    _dp, _ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)
    _fields_ = [("msd", _dp), ("vacf", _dp), ("cnt", _ip), ("rdf", ctypes.POINTER(ctypes.c_uint64)), ("rdf_samples", _ip), ("vol_sum", _dp)]


class MdTransportParams(ctypes.Structure):
    _fields_ = [("collective", ctypes.c_int32), ("non_gaussian", ctypes.c_int32), ("vh_bins", ctypes.c_int32), ("vh_lags", ctypes.c_int32),
                ("vh_stride", ctypes.c_int32), ("reserved", ctypes.c_int32), ("vh_rmax", ctypes.c_double)]


class MdTransportHost(ctypes.Structure):
    _dp, _ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)
    _fields_ = [("msd4", _dp), ("cmsd", _dp), ("jacf", _dp), ("vh", ctypes.POINTER(ctypes.c_uint64)), ("samples", _ip), ("vol_sum", _dp)]


class MdChargeParams(ctypes.Structure):
    _fields_ = [("n_bounds", ctypes.c_int32 * 8), ("mag_bins", ctypes.c_int32), ("center_species", ctypes.c_int32),
                ("srdf_bins", ctypes.c_int32), ("reserved", ctypes.c_int32), ("mag_max", ctypes.c_double), ("srdf_rmax", ctypes.c_double)]


class MdChargeHost(ctypes.Structure):
    _dp, _ip, _up = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_uint64)
    _fields_ = [("mhist", _up), ("msum", _dp), ("msq", _dp), ("pop", _ip), ("trans", _ip), ("occ", _ip), ("mcorr", _dp), ("same", _ip),
                ("shist", _up), ("samples", _ip), ("skipped", _ip), ("vol_sum", _dp)]


class McParams(ctypes.Structure):
    _fields_ = [("swap_probability", ctypes.c_double), ("max_displacement", ctypes.c_double), ("kB", ctypes.c_double),
                ("loginterval", ctypes.c_int32), ("ring_frames", ctypes.c_int32), ("r_atom", ctypes.c_double), ("r_bond", ctypes.c_double),
                ("numerical_tol", ctypes.c_double)]


class McOutHost(ctypes.Structure):
    _dp, _lp = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int64)
    _fields_ = [("positions", _dp), ("site", c_int_p), ("energy", _dp), ("temperatures", _dp), ("status", c_int_p), ("n_trials", c_int_p),
                ("counts", _lp), ("sums", _dp), ("best_energy", _dp), ("best_positions", _dp), ("best_site", c_int_p),
                ("frame_capacity", ctypes.c_int32), ("n_frames", c_int_p), ("frame_trial", c_int_p), ("frame_scalars", _dp),
                ("frame_moves", c_int_p), ("frame_positions", _dp), ("frame_site", c_int_p)]


class NebParams(ctypes.Structure):
    _fields_ = [("fmax", ctypes.c_double), ("max_steps", ctypes.c_int32), ("climb", ctypes.c_int32),
                ("dt", ctypes.c_double), ("maxstep", ctypes.c_double), ("dtmax", ctypes.c_double), ("finc", ctypes.c_double),
                ("fdec", ctypes.c_double), ("astart", ctypes.c_double), ("fa", ctypes.c_double), ("nmin", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("spring", ctypes.c_double), ("r_atom", ctypes.c_double), ("r_bond", ctypes.c_double),
                ("numerical_tol", ctypes.c_double)]


class NebOutHost(ctypes.Structure):
    _fields_ = [("frac", ctypes.POINTER(ctypes.c_double)), ("energy", c_float_p), ("force", c_float_p),
                ("neb_fmax", ctypes.POINTER(ctypes.c_double)), ("climbing_image", c_int_p), ("n_steps", c_int_p), ("status", c_int_p),
                ("n_evaluated", c_int_p)]


class DimerParams(ctypes.Structure):
    _fields_ = [("fmax", ctypes.c_double), ("max_steps", ctypes.c_int32), ("max_rotations", ctypes.c_int32),
                ("dt", ctypes.c_double), ("maxstep", ctypes.c_double), ("dtmax", ctypes.c_double), ("finc", ctypes.c_double),
                ("fdec", ctypes.c_double), ("astart", ctypes.c_double), ("fa", ctypes.c_double), ("nmin", ctypes.c_int32),
                ("reserved", ctypes.c_int32), ("delta", ctypes.c_double), ("angle_tol", ctypes.c_double), ("r_atom", ctypes.c_double),
                ("r_bond", ctypes.c_double), ("numerical_tol", ctypes.c_double)]


class DimerOutHost(ctypes.Structure):
    _dp = ctypes.POINTER(ctypes.c_double)
    _fields_ = [("frac", _dp), ("mode", _dp), ("force", _dp), ("image_energy", c_float_p), ("image_force", c_float_p), ("curvature", _dp), ("fmax", _dp), ("n_steps", c_int_p),
                ("n_rotations", c_int_p), ("n_evaluated", c_int_p), ("status", c_int_p), ("phase", c_int_p)]


NEB_SD, NEB_SI, NEB_MAX_IMAGES = 24, 4, 66              # csrc/kernels_neb.h: state doubles and ints per band (chg_test_neb_step)
DIMER_SD, DIMER_SI, DIMER_MAX_ROTATIONS = 24, 8, 32     # csrc/kernels_dimer.h: state doubles and ints per search (chg_test_dimer_step)
MC_COUNTS, MC_FRAME_SCALARS, MC_FRAME_MOVES = 8, 6, 6   # include/chgnet_hip.h CHG_MC_*
MC_SD, MC_SI = 32, 8                                    # csrc/kernels_mc.h: state doubles and ints per replica (chg_test_mc_step)
MC_EXCHANGE_INTS = 6                                    # include/chgnet_hip.h CHG_MC_EXCHANGE_INTS: walker, attempts, accepts, mark, trips, spare
MD_OBS_MAX_LAGS, MD_OBS_MAX_SPECIES, MD_OBS_RDF_CELLS = 4096, 8, 16384   # csrc/kernels_md_obs.h
MD_OBS_VH_CELLS = 4096                                                   # csrc/kernels_md_transport.h
MD_CHG_STATES, MD_CHG_BOUNDS, MD_CHG_HIST_CELLS, MD_CHG_SRDF_CELLS = 4, 3, 4096, 16384   # csrc/kernels_md_magmom.h
MD_NHC_STATE = 20   # include/chgnet_hip.h CHG_MD_NHC_STATE
MD_VG = 9           # include/chgnet_hip.h CHG_MD_VG
MD_CELL_MODES = {"flexible": 1, "axes": 2}   # CHG_MD_CELL_*

_POINTER_OF = {"float64": ctypes.POINTER(ctypes.c_double), "float32": c_float_p, "int32": c_int_p,
               "int64": ctypes.POINTER(ctypes.c_int64), "uint64": ctypes.POINTER(ctypes.c_uint64)}


def fill_out(out: ctypes.Structure, arrays: dict) -> ctypes.Structure:
    """Point the fields of a ``*_out_host`` struct at NumPy arrays named like them (pointer type by dtype); returns ``out``."""
    for name, a in arrays.items():
        setattr(out, name, a.ctypes.data_as(_POINTER_OF[a.dtype.name]))
    return out


_LIB = None


def hip_lib_path() -> str:
    from chgnet_amd.build import HIP_LIB

    return os.environ.get("CHGNET_HIP_LIB", HIP_LIB)   # override: kernel timing experiments only


ABI_VERSION = 5   # include/chgnet_hip.h CHG_ABI_VERSION


def load() -> ctypes.CDLL:
    """Load the HIP engine library; raise loudly if it is not built or cannot be loaded."""
    global _LIB  # noqa: PLW0603
    if _LIB is not None:
        return _LIB
    path = hip_lib_path()
    if not os.path.exists(path):
        raise RuntimeError(
            f"chgnet_amd: HIP extension {path} is missing. Build it with `python -m chgnet_amd.build` "
            "(needs hipcc). There is no CPU fallback.")
    try:
        lib = ctypes.CDLL(path)
    except OSError as exc:
        raise RuntimeError(f"chgnet_amd: cannot load HIP extension {path}: {exc}") from exc
    # the struct layouts below are those of include/chgnet_hip.h at this interface version: a library built from another one is refused
    try:
        lib.chg_abi_version.restype = ctypes.c_int
        found = int(lib.chg_abi_version())
    except AttributeError:
        found = -1
    if found != ABI_VERSION:
        raise RuntimeError(f"chgnet_amd: HIP extension {path} has interface version {found}, this binding was written for {ABI_VERSION}: "
                           "rebuild it with `python -m chgnet_amd.build --force`")
    vp = ctypes.c_void_p
    lib.chg_device_count.restype = ctypes.c_int
    lib.chg_weights_required.argtypes = [ctypes.c_int32]
    lib.chg_weights_required.restype = ctypes.c_int64
    lib.chg_engine_create.argtypes = [ctypes.POINTER(ModelDesc), c_float_p, ctypes.c_int, ctypes.POINTER(vp)]
    lib.chg_engine_destroy.argtypes = [vp]
    lib.chg_last_error.argtypes = [vp]
    lib.chg_last_error.restype = ctypes.c_char_p
    lib.chg_engine_build_stats.argtypes = [vp, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]
    lib.chg_engine_set_graph_search.argtypes = [vp, ctypes.c_int32, ctypes.c_int32]
    u8p = ctypes.POINTER(ctypes.c_uint8)
    lib.chg_comm_unique_id.argtypes = [u8p]
    lib.chg_comm_create.argtypes = [u8p, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(vp)]
    lib.chg_comm_all_gather_f32.argtypes = [vp, c_float_p, ctypes.c_int64, c_float_p]
    lib.chg_comm_all_reduce_sum_f32.argtypes = [vp, c_float_p, ctypes.c_int64]
    lib.chg_comm_all_gather_f32_device.argtypes = [vp, vp, ctypes.c_int64, vp, vp]
    lib.chg_comm_all_reduce_sum_f32_device.argtypes = [vp, vp, ctypes.c_int64, vp]
    lib.chg_comm_reserve.argtypes = [vp, ctypes.c_int64, ctypes.POINTER(vp)]
    lib.chg_comm_info.argtypes = [vp, c_int_p, c_int_p, c_int_p]
    lib.chg_comm_barrier.argtypes = [vp]
    lib.chg_comm_destroy.argtypes = [vp]
    lib.chg_comm_last_error.argtypes = [vp]
    lib.chg_comm_last_error.restype = ctypes.c_char_p
    lib.chg_engine_cell_stats.argtypes = [vp, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]
    lib.chg_engine_set_memory_limit.argtypes = [vp, ctypes.c_int64]
    lib.chg_engine_memory_info.argtypes = [vp, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int64)]
    lib.chg_batch_bytes_required.argtypes = [ctypes.c_int32] * 6
    lib.chg_batch_bytes_required.restype = ctypes.c_int64
    lib.chg_batch_upload.argtypes = [vp, ctypes.POINTER(BatchHost), ctypes.POINTER(vp)]
    lib.chg_host_alloc.argtypes = [ctypes.c_int64, ctypes.POINTER(vp)]
    lib.chg_host_free.argtypes = [vp]
    lib.chg_batch_build.argtypes = [vp, ctypes.POINTER(StructsHost), ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                    ctypes.POINTER(vp), c_int_p]
    lib.chg_batch_build_predict.argtypes = [vp, ctypes.POINTER(StructsHost), ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_uint32,
                                            ctypes.POINTER(vp), c_int_p]
    lib.chg_debug_fetch_i32.argtypes = [vp, vp, ctypes.c_char_p, c_int_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]
    lib.chg_batch_update_geometry.argtypes = [vp, vp, c_float_p, c_float_p]
    lib.chg_batch_free.argtypes = [vp, vp]
    lib.chg_batch_device_bytes.argtypes = [vp]
    lib.chg_batch_device_bytes.restype = ctypes.c_int64
    lib.chg_predict.argtypes = [vp, vp, ctypes.c_uint32]
    lib.chg_synchronize.argtypes = [vp]
    lib.chg_backward.argtypes = [vp, vp, c_float_p, c_float_p, c_float_p, c_float_p, c_float_p]
    lib.chg_backward_allreduce.argtypes = [vp, vp, c_float_p, c_float_p, c_float_p, c_float_p, vp, c_float_p]
    lib.chg_hessian_vector.argtypes = [vp, vp, c_float_p, c_float_p]
    lib.chg_hessian_vector_strain.argtypes = [vp, vp, c_float_p, c_float_p, c_float_p, c_float_p]
    lib.chg_batch_all_gather_energy.argtypes = [vp, vp, vp, ctypes.c_int64, c_float_p]
    lib.chg_engine_stream.argtypes = [vp]
    lib.chg_engine_stream.restype = ctypes.c_void_p
    lib.chg_engine_device.argtypes = [vp]
    lib.chg_engine_update_weights.argtypes = [vp, c_float_p]
    lib.chg_batch_download.argtypes = [vp, vp, ctypes.POINTER(OutHost)]
    lib.chg_timer_start.argtypes = [vp]
    lib.chg_timer_stop_ms.argtypes = [vp, c_float_p]
    lib.chg_stream_copy.argtypes = [vp, ctypes.c_int64, ctypes.c_int, c_float_p]
    lib.chg_profile_enable.argtypes = [vp, ctypes.c_int]
    lib.chg_profile_reset.argtypes = [vp]
    lib.chg_profile_count.argtypes = [vp]
    lib.chg_profile_read.argtypes = [vp, ctypes.c_int, ctypes.c_char_p, ctypes.c_int, ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)]
    lib.chg_debug_fetch.argtypes = [vp, vp, ctypes.c_char_p, c_float_p, ctypes.c_int64, ctypes.POINTER(ctypes.c_int64)]
    lib.chg_test_rows_gemm.argtypes = [vp, c_float_p, c_float_p, c_float_p, c_float_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    lib.chg_test_split_gemm.argtypes = [vp, c_float_p, c_float_p, c_float_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    dp = ctypes.POINTER(ctypes.c_double)
    lib.chg_relax_create.argtypes = [vp, ctypes.POINTER(StructsHost), ctypes.POINTER(RelaxParams), ctypes.POINTER(vp)]
    lib.chg_relax_run.argtypes = [vp, vp, ctypes.c_int32, c_int_p]
    lib.chg_relax_download.argtypes = [vp, vp, ctypes.POINTER(RelaxOutHost)]
    lib.chg_relax_free.argtypes = [vp, vp]
    lib.chg_test_relax_step.argtypes = [vp, ctypes.POINTER(RelaxParams), ctypes.c_int32, c_int_p, dp, dp, dp, c_int_p, c_float_p, c_float_p,
                                        c_float_p, c_float_p, dp, dp]
    lib.chg_relax_create_lbfgs.argtypes = [vp, ctypes.POINTER(StructsHost), ctypes.POINTER(RelaxParams), ctypes.POINTER(LbfgsParams),
                                           ctypes.POINTER(vp)]
    lib.chg_test_lbfgs_step.argtypes = [vp, ctypes.POINTER(RelaxParams), ctypes.POINTER(LbfgsParams), ctypes.c_int32, c_int_p, dp, dp, dp, dp, dp,
                                        dp, dp, c_int_p, c_float_p, c_float_p, c_float_p, c_float_p, ctypes.c_int32, dp, dp, c_int_p]
    lib.chg_md_create.argtypes = [vp, ctypes.POINTER(StructsHost), dp, dp, ctypes.POINTER(MdParams), ctypes.POINTER(vp)]
    lib.chg_md_run.argtypes = [vp, vp, ctypes.c_int32]
    lib.chg_md_download.argtypes = [vp, vp, ctypes.POINTER(MdOutHost)]
    lib.chg_md_free.argtypes = [vp, vp]
    lib.chg_test_md_step.argtypes = [vp, ctypes.POINTER(MdParams), ctypes.c_int32, c_int_p, ctypes.c_int32, dp, dp, dp, dp, dp, c_int_p,
                                     c_float_p, c_float_p, c_float_p, dp, dp]
    u64p = ctypes.POINTER(ctypes.c_uint64)
    lib.chg_md_create_langevin.argtypes = [*lib.chg_md_create.argtypes[:5], ctypes.c_double, u64p, ctypes.POINTER(vp)]
    lib.chg_test_md_step_langevin.argtypes = [*lib.chg_test_md_step.argtypes, ctypes.c_double, u64p]
    lib.chg_md_create_nhc.argtypes = [*lib.chg_md_create.argtypes[:5], ctypes.c_int32, ctypes.POINTER(vp)]
    lib.chg_md_download_nhc.argtypes = [vp, vp, dp, dp, ctypes.c_int32]
    lib.chg_test_md_step_nhc.argtypes = [*lib.chg_test_md_step.argtypes, ctypes.c_int32, dp]
    lib.chg_md_create_nhc_flex.argtypes = [*lib.chg_md_create.argtypes[:5], ctypes.c_int32, ctypes.c_int32, ctypes.POINTER(vp)]
    lib.chg_md_download_vg.argtypes = [vp, vp, dp]
    lib.chg_test_md_step_nhc_flex.argtypes = [*lib.chg_test_md_step_nhc.argtypes, dp, u8p]
    # constraints: the mask [N,3] uint8 travels as an argument of entry points of its own
    lib.chg_relax_set_fixed.argtypes = [vp, vp, u8p]
    lib.chg_md_set_fixed.argtypes = [vp, vp, u8p]
    lib.chg_test_relax_step_fixed.argtypes = [*lib.chg_test_relax_step.argtypes, u8p]
    lib.chg_test_lbfgs_step_fixed.argtypes = [*lib.chg_test_lbfgs_step.argtypes, u8p]
    lib.chg_test_md_step_fixed.argtypes = [*lib.chg_test_md_step.argtypes, ctypes.c_double, u64p, ctypes.c_int32, dp, u8p]
    # MD observables: parameters and species in, accumulators out
    lib.chg_md_set_observers.argtypes = [vp, vp, ctypes.POINTER(MdObserveParams), c_int_p]
    lib.chg_md_download_observables.argtypes = [vp, vp, ctypes.POINTER(MdObservablesHost)]
    lib.chg_test_md_observe.argtypes = [vp, ctypes.POINTER(MdObserveParams), ctypes.c_int32, c_int_p, c_int_p, dp, ctypes.c_int32, dp, dp, dp,
                                        c_int_p, ctypes.POINTER(MdObservablesHost)]
    lib.chg_md_set_transport.argtypes = [vp, vp, ctypes.POINTER(MdTransportParams)]
    lib.chg_md_download_transport.argtypes = [vp, vp, ctypes.POINTER(MdTransportHost)]
    lib.chg_test_md_transport.argtypes = [vp, ctypes.POINTER(MdObserveParams), ctypes.POINTER(MdTransportParams), ctypes.c_int32, c_int_p,
                                          c_int_p, dp, ctypes.c_int32, dp, dp, dp, c_int_p, ctypes.POINTER(MdObservablesHost),
                                          ctypes.POINTER(MdTransportHost)]
    # moments per frame and charge-state observers: boundaries [S, 3] and the moments of the test snapshots travel beside the params struct
    lib.chg_md_set_magmoms.argtypes = [vp, vp, ctypes.c_int32]
    lib.chg_md_download_magmoms.argtypes = [vp, vp, c_float_p, c_float_p, ctypes.c_int32]
    lib.chg_md_set_charge_states.argtypes = [vp, vp, ctypes.POINTER(MdChargeParams), dp]
    lib.chg_md_download_charge_states.argtypes = [vp, vp, ctypes.POINTER(MdChargeHost)]
    lib.chg_test_md_charge_states.argtypes = [vp, ctypes.POINTER(MdObserveParams), ctypes.POINTER(MdChargeParams), dp, ctypes.c_int32, c_int_p,
                                              c_int_p, dp, ctypes.c_int32, dp, dp, dp, c_int_p, c_float_p, ctypes.POINTER(MdObservablesHost),
                                              ctypes.POINTER(MdChargeHost)]
    # Monte Carlo: temperatures, seeds and the two per-atom masks travel beside the params struct
    lp = ctypes.POINTER(ctypes.c_int64)
    lib.chg_mc_create.argtypes = [vp, ctypes.POINTER(StructsHost), dp, u64p, u8p, u8p, ctypes.POINTER(McParams), ctypes.POINTER(vp)]
    lib.chg_mc_set_temperatures.argtypes = [vp, vp, dp]
    lib.chg_mc_run.argtypes = [vp, vp, ctypes.c_int32]
    lib.chg_mc_download.argtypes = [vp, vp, ctypes.POINTER(McOutHost)]
    lib.chg_mc_free.argtypes = [vp, vp]
    lib.chg_test_mc_step.argtypes = [vp, ctypes.POINTER(McParams), ctypes.c_int32, c_int_p, c_int_p, u8p, u8p, dp, u64p, ctypes.c_int32,
                                     ctypes.c_int32, ctypes.c_int32, dp, c_int_p, dp, c_int_p, lp, dp, c_int_p, c_float_p, dp, c_int_p,
                                     dp, c_int_p, dp, c_int_p]
    # replica exchange: the ladder ids in, the exchange state [B, MC_EXCHANGE_INTS] out
    lib.chg_mc_set_exchange.argtypes = [vp, vp, c_int_p, ctypes.c_int32]
    lib.chg_mc_download_exchange.argtypes = [vp, vp, c_int_p]
    lib.chg_test_mc_exchange.argtypes = [vp, ctypes.c_int32, c_int_p, c_int_p, dp, u64p, ctypes.c_double, ctypes.c_int32, dp, c_int_p, dp,
                                         c_int_p, dp, c_int_p, c_int_p]
    # nudged elastic band: the band offsets travel beside the structures, the mask [N,3] over all images as an argument of its own
    lib.chg_neb_create.argtypes = [vp, ctypes.POINTER(StructsHost), c_int_p, ctypes.c_int32, ctypes.POINTER(NebParams), ctypes.POINTER(vp)]
    lib.chg_neb_set_fixed.argtypes = [vp, vp, u8p]
    lib.chg_neb_run.argtypes = [vp, vp, ctypes.c_int32, c_int_p]
    lib.chg_neb_download.argtypes = [vp, vp, ctypes.POINTER(NebOutHost)]
    lib.chg_neb_free.argtypes = [vp, vp]
    lib.chg_test_neb_step.argtypes = [vp, ctypes.POINTER(NebParams), ctypes.c_int32, c_int_p, c_int_p, dp, dp, dp, dp, c_int_p, c_float_p,
                                      c_float_p, c_float_p, ctypes.c_int32, ctypes.c_int32, u8p, dp, c_int_p]
    # dimer saddle search: the modes [N,3] travel beside the structures, the mask [N,3] as an argument of its own
    lib.chg_dimer_create.argtypes = [vp, ctypes.POINTER(StructsHost), dp, ctypes.POINTER(DimerParams), ctypes.POINTER(vp)]
    lib.chg_dimer_set_fixed.argtypes = [vp, vp, u8p]
    lib.chg_dimer_run.argtypes = [vp, vp, ctypes.c_int32, c_int_p]
    lib.chg_dimer_download.argtypes = [vp, vp, ctypes.POINTER(DimerOutHost)]
    lib.chg_dimer_free.argtypes = [vp, vp]
    lib.chg_test_dimer_step.argtypes = [vp, ctypes.POINTER(DimerParams), ctypes.c_int32, c_int_p, dp, dp, dp, dp, dp, dp, dp, c_int_p, c_float_p,
                                        c_float_p, c_float_p, c_float_p, ctypes.c_int32, u8p, dp, c_int_p, c_int_p, c_int_p]
    for name in EXPORTED_SYMBOLS:
        fn = getattr(lib, name)
        if fn.restype is ctypes.c_int and name not in ("chg_device_count", "chg_profile_count"):
            fn.restype = ctypes.c_int
    _LIB = lib
    return lib


def task_mask(task: str) -> int:
    mask = 0
    for ch in task:
        mask |= TASK_BITS[ch]
    return mask
