"""ctypes binding of the C ABI in include/mcamd.h (libmcamd.so).

Host-side plumbing only: device buffers and streams come from the caller (torch tensors'
data_ptr / torch.cuda.current_stream in the tests and bench).  Nothing here computes a price:
every call goes to the HIP library, and loading fails loudly if the library is missing.
"""
from __future__ import annotations

import ctypes as C
import math
import os

PKG = os.path.dirname(os.path.abspath(__file__))
# MCAMD_LIB: diagnostic override for same-box A/B runs of a variant build (build.build_variant, tools/ab_lib.py)
LIB_PATH = os.environ.get("MCAMD_LIB") or os.path.join(PKG, "libmcamd.so")

OK, ERR_INVALID, ERR_HIP, ERR_NODEVICE, ERR_NOMEM = 0, 1, 2, 3, 4
F32, F64 = 32, 64
STEP_MAJOR, PATH_MAJOR = 0, 1
NMC_WAVE_PER_POINT, NMC_BLOCK_PER_POINT, NMC_BLOCK_PER_POINT_PLAIN = 0, 1, 2
FLAG_LOG_SPACE, FLAG_ANTITHETIC, FLAG_CONTROL_VARIATE, FLAG_SEPARATE_REDUCE, FLAG_PRODUCT_FORM = 1, 2, 4, 8, 16
REDUCE_SEQUENTIAL, REDUCE_FIRST_ADD, REDUCE_UNROLL_LAST, REDUCE_GRID_STRIDE = 3, 4, 5, 6
GREEKS_AUTO, GREEKS_PATHWISE, GREEKS_LIKELIHOOD_RATIO = 0, 1, 2
GREEK_PRICE, GREEK_DELTA, GREEK_GAMMA, GREEK_VEGA, GREEK_RHO, GREEK_THETA = range(6)
GREEK_NAMES = ("price", "delta", "gamma", "vega", "rho", "theta")
GREEKS_STATS = 16   # doubles of a Greeks statistics record: six (sum, sumsq) pairs, n, zeros
PAYOFF_CALL, PAYOFF_PUT = 0, 1
BARRIER_DOWN_OUT, BARRIER_DOWN_IN, BARRIER_UP_OUT, BARRIER_UP_IN = 0, 1, 2, 3
MONITOR_DISCRETE, MONITOR_CONTINUOUS = 0, 1
LOOKBACK_FLOATING, LOOKBACK_FIXED = 0, 1
ASIAN_ARITHMETIC, ASIAN_GEOMETRIC = 0, 1
ASIAN_FIXED, ASIAN_FLOATING = 0, 1
ASIAN_CONTROL_NONE, ASIAN_CONTROL_GEOMETRIC = 0, 1
AUTOCALL_MAX_DATES = 64
AUTOCALL_KI_NONE, AUTOCALL_KI_AT_MATURITY, AUTOCALL_KI_EVERY_STEP = 0, 1, 2
LOCALVOL_NO_BARRIER = -1
LOCALVOL_MAX_NODES = 2048
SMILE_MAX_STRIKES, SMILE_MAX_EXPIRIES = 64, 32
LOCALVOL_GREEKS_MAX_BUCKETS = 8
(LOCALVOL_GREEK_PRICE, LOCALVOL_GREEK_DELTA, LOCALVOL_GREEK_GAMMA, LOCALVOL_GREEK_VEGA, LOCALVOL_GREEK_RHO,
 LOCALVOL_GREEK_RHO_Q) = range(6)
LOCALVOL_GREEK_NAMES = ("price", "delta", "gamma", "vega", "rho", "rho_q")
LOCALVOL_GREEKS_STATS = 32   # doubles of the record: six (sum, sumsq) pairs, eight bucket pairs, n, zeros
CLIQUET_SUM, CLIQUET_COMPOUND, CLIQUET_VARIANCE = 0, 1, 2
HESTON_FULL_TRUNCATION = 0
HESTON_XI_MIN = 1e-8   # below it heston_price takes the variance as deterministic
BASKET_MAX_ASSETS = 8
BASKET_ARITHMETIC, BASKET_GEOMETRIC, BASKET_BEST_OF, BASKET_WORST_OF = 0, 1, 2, 3
BASKET_NO_BARRIER, BASKET_DOWN_OUT, BASKET_DOWN_IN, BASKET_UP_OUT, BASKET_UP_IN = 0, 1, 2, 3, 4

# every symbol include/mcamd.h declares
EXPORTS = [
    "mcamd_abi_version", "mcamd_last_error", "mcamd_build_id", "mcamd_device_count", "mcamd_ctx_create", "mcamd_ctx_destroy",
    "mcamd_get_device_info", "mcamd_device_malloc", "mcamd_device_free", "mcamd_memcpy_to_host",
    "mcamd_memcpy_to_device", "mcamd_price_paths", "mcamd_price_paths_enqueue", "mcamd_enqueued_kernel_ms",
    "mcamd_finalize_stats", "mcamd_group_create", "mcamd_group_destroy", "mcamd_group_size",
    "mcamd_group_price_paths", "mcamd_group_ctx", "mcamd_group_shard", "mcamd_group_simulate_trajectories",
    "mcamd_group_nmc_inner", "mcamd_group_nmc_fused", "mcamd_simulate_trajectories_enqueue", "mcamd_diag_store_pattern", "mcamd_nmc_inner_enqueue",
    "mcamd_nmc_fused_enqueue", "mcamd_finalize_nmc_stats", "mcamd_simulate_trajectories", "mcamd_price_from_normals",
    "mcamd_generate_normals", "mcamd_reduce_sum", "mcamd_reduce_partials", "mcamd_cpu_mc_f32", "mcamd_nmc_inner", "mcamd_nmc_fused", "mcamd_finalize", "mcamd_finalize_cv", "mcamd_cnd_f32",
    "mcamd_bs_call_f32", "mcamd_bs_call_f64", "mcamd_price_greeks", "mcamd_price_greeks_enqueue",
    "mcamd_finalize_greeks_stats", "mcamd_group_price_greeks", "mcamd_bs_greeks_f64",
    "mcamd_american_workspace_bytes", "mcamd_price_american",
    "mcamd_american_dual_workspace_bytes", "mcamd_american_upper_bound",
    "mcamd_price_barrier", "mcamd_price_barrier_enqueue", "mcamd_barrier_price_f64",
    "mcamd_price_lookback", "mcamd_price_lookback_enqueue", "mcamd_lookback_price_f64",
    "mcamd_price_basket", "mcamd_price_basket_enqueue", "mcamd_basket_geometric_price_f64", "mcamd_exchange_price_f64",
    "mcamd_price_asian", "mcamd_price_asian_enqueue", "mcamd_asian_geometric_price_f64",
    "mcamd_price_autocall", "mcamd_price_autocall_enqueue", "mcamd_autocall_single_date_price_f64",
    "mcamd_localvol_surface_create", "mcamd_localvol_surface_destroy", "mcamd_price_localvol",
    "mcamd_price_localvol_enqueue", "mcamd_localvol_sigma_f64", "mcamd_bs_price_f64",
    "mcamd_bs_implied_vol_f64", "mcamd_price_localvol_smile", "mcamd_price_localvol_smile_enqueue", "mcamd_finalize_smile",
    "mcamd_price_autocall_localvol", "mcamd_price_autocall_localvol_enqueue",
    "mcamd_price_localvol_greeks", "mcamd_price_localvol_greeks_enqueue", "mcamd_finalize_localvol_greeks_stats",
    "mcamd_price_cliquet", "mcamd_price_cliquet_enqueue", "mcamd_cliquet_price_f64",
    "mcamd_price_heston", "mcamd_price_heston_enqueue", "mcamd_heston_price_f64",
    "mcamd_price_heston_smile", "mcamd_price_heston_smile_enqueue",
    "mcamd_price_heston_cliquet", "mcamd_price_heston_cliquet_enqueue", "mcamd_heston_cliquet_price_f64",
    "mcamd_price_heston_barrier", "mcamd_price_heston_barrier_enqueue",
]


class Option(C.Structure):
    _fields_ = [("S0", C.c_double), ("T", C.c_double), ("K", C.c_double), ("r", C.c_double), ("v", C.c_double),
                ("B", C.c_double), ("P1", C.c_int32), ("P2", C.c_int32), ("use_window", C.c_int32),
                ("Ik", C.c_int32), ("Sk", C.c_double), ("Tk", C.c_int32), ("reserved", C.c_int32), ("dt", C.c_double)]


class Sim(C.Structure):
    _fields_ = [("n_paths", C.c_uint64), ("path_offset", C.c_uint64), ("n_paths_local", C.c_uint64),
                ("n_steps", C.c_uint32), ("n_paths_inner", C.c_uint32), ("seed", C.c_uint64),
                ("precision", C.c_int32), ("flags", C.c_int32)]


class Result(C.Structure):
    _fields_ = [("sum", C.c_double), ("sumsq", C.c_double), ("n", C.c_uint64), ("price", C.c_double),
                ("std_err", C.c_double), ("ci_lo", C.c_double), ("ci_hi", C.c_double), ("kernel_ms", C.c_float),
                ("total_ms", C.c_float), ("grid", C.c_uint32), ("block", C.c_uint32), ("sum_c", C.c_double),
                ("sum_cc", C.c_double), ("sum_yc", C.c_double), ("cv_beta", C.c_double), ("cv_rho", C.c_double),
                ("work_steps", C.c_double), ("live_steps", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class Greeks(C.Structure):
    """mcamd_greeks: value / std_err / raw sums of price, delta, gamma, vega, rho, theta (indexed GREEK_*)."""
    _fields_ = [("value", C.c_double * 6), ("std_err", C.c_double * 6), ("sum", C.c_double * 6),
                ("sumsq", C.c_double * 6), ("n", C.c_uint64), ("method", C.c_int32), ("kernel_ms", C.c_float),
                ("total_ms", C.c_float), ("grid", C.c_uint32), ("block", C.c_uint32), ("reserved", C.c_int32)]

    def as_dict(self):
        """{name: (value, std_err)} of the six quantities"""
        return {name: (self.value[i], self.std_err[i]) for i, name in enumerate(GREEK_NAMES)}


class American(C.Structure):
    """mcamd_american: exercise rule and training set of mcamd_price_american."""
    _fields_ = [("payoff", C.c_int32), ("exercise_every", C.c_uint32), ("n_basis", C.c_uint32),
                ("reserved", C.c_uint32), ("n_train", C.c_uint64), ("train_seed", C.c_uint64)]


class AmericanResult(C.Structure):
    """mcamd_american_result: out-of-sample and in-sample estimates, raw shard sums, dates, timings."""
    _fields_ = [("price", C.c_double), ("std_err", C.c_double), ("ci_lo", C.c_double), ("ci_hi", C.c_double),
                ("sum", C.c_double), ("sumsq", C.c_double), ("n", C.c_uint64), ("in_sample_price", C.c_double),
                ("in_sample_std_err", C.c_double), ("in_sample_sum", C.c_double), ("in_sample_sumsq", C.c_double),
                ("n_train", C.c_uint64), ("n_early", C.c_uint64), ("sum_t_exercise", C.c_double),
                ("n_dates", C.c_uint32), ("n_regressed", C.c_uint32), ("immediate_exercise", C.c_int32),
                ("train_ms", C.c_float), ("price_ms", C.c_float), ("total_ms", C.c_float), ("grid", C.c_uint32),
                ("block", C.c_uint32), ("train_grid", C.c_uint32), ("reserved", C.c_int32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class AmericanDual(C.Structure):
    """mcamd_american_dual: the nested sample of mcamd_american_upper_bound."""
    _fields_ = [("n_inner", C.c_uint32), ("reserved", C.c_uint32), ("inner_seed", C.c_uint64)]


class AmericanDualResult(C.Structure):
    """mcamd_american_dual_result: the dual (upper) estimate, raw shard sums, lane-step counts, timings."""
    _fields_ = [("upper", C.c_double), ("std_err", C.c_double), ("ci_hi", C.c_double), ("sum", C.c_double),
                ("sumsq", C.c_double), ("n", C.c_uint64), ("sum_q0", C.c_double), ("work_steps", C.c_double),
                ("live_steps", C.c_double), ("n_dates", C.c_uint32), ("immediate_exercise", C.c_int32),
                ("outer_ms", C.c_float), ("inner_ms", C.c_float), ("scan_ms", C.c_float), ("total_ms", C.c_float),
                ("grid", C.c_uint32), ("block", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class Barrier(C.Structure):
    """mcamd_barrier: which single barrier mcamd_price_barrier prices, and how it is monitored."""
    _fields_ = [("kind", C.c_int32), ("payoff", C.c_int32), ("monitoring", C.c_int32), ("reserved", C.c_int32)]


class Lookback(C.Structure):
    """mcamd_lookback: which lookback mcamd_price_lookback prices, and how the extremum is monitored."""
    _fields_ = [("strike", C.c_int32), ("payoff", C.c_int32), ("monitoring", C.c_int32), ("reserved", C.c_int32)]


class Basket(C.Structure):
    """mcamd_basket: the assets (spots, volatilities, weights, correlations with row stride 8), the aggregate and the
    optional barrier mcamd_price_basket prices."""
    _fields_ = [("n_assets", C.c_int32), ("kind", C.c_int32), ("payoff", C.c_int32), ("barrier", C.c_int32),
                ("reserved", C.c_int32 * 2), ("S0", C.c_double * 8), ("v", C.c_double * 8), ("w", C.c_double * 8),
                ("corr", C.c_double * 64)]


class Asian(C.Structure):
    """mcamd_asian: which average mcamd_price_asian takes, over which dates, against which strike, and whether the
    geometric average serves as control variate."""
    _fields_ = [("average", C.c_int32), ("strike", C.c_int32), ("payoff", C.c_int32), ("include_spot", C.c_int32),
                ("control", C.c_int32), ("reserved", C.c_int32)]


class Autocall(C.Structure):
    """mcamd_autocall: the terms of the worst-of autocallable note mcamd_price_autocall prices, and its assets."""
    _fields_ = [("n_assets", C.c_int32), ("ki_monitoring", C.c_int32), ("observe_every", C.c_uint32),
                ("first_call_date", C.c_uint32), ("reserved", C.c_int32 * 2), ("call_level", C.c_double),
                ("call_step_down", C.c_double), ("coupon", C.c_double), ("ki_level", C.c_double),
                ("v", C.c_double * 8), ("corr", C.c_double * 64)]


class AutocallResult(C.Structure):
    """mcamd_autocall_result"""
    _fields_ = [("price", C.c_double), ("std_err", C.c_double), ("ci_lo", C.c_double), ("ci_hi", C.c_double),
                ("sum", C.c_double), ("sumsq", C.c_double), ("n", C.c_uint64), ("n_called", C.c_uint64),
                ("sum_t_call", C.c_double), ("n_knocked_in", C.c_uint64), ("work_steps", C.c_double),
                ("live_steps", C.c_double), ("kernel_ms", C.c_float), ("total_ms", C.c_float), ("grid", C.c_uint32),
                ("block", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class AutocallLocalVol(C.Structure):
    """mcamd_autocall_localvol: the terms of the worst-of autocallable note mcamd_price_autocall_localvol prices, the
    dividend yields of its assets and their correlations (mcamd_autocall with q in the place of v)."""
    _fields_ = [("n_assets", C.c_int32), ("ki_monitoring", C.c_int32), ("observe_every", C.c_uint32),
                ("first_call_date", C.c_uint32), ("reserved", C.c_int32 * 2), ("call_level", C.c_double),
                ("call_step_down", C.c_double), ("coupon", C.c_double), ("ki_level", C.c_double),
                ("q", C.c_double * 8), ("corr", C.c_double * 64)]


class LocalVolGrid(C.Structure):
    """mcamd_localvol_grid: n_t time slices of n_x nodes, equally spaced in ln(S / S0) on [x_min, x_max]."""
    _fields_ = [("n_t", C.c_uint32), ("n_x", C.c_uint32), ("x_min", C.c_double), ("x_max", C.c_double)]


class LocalVol(C.Structure):
    """mcamd_localvol: the payoff, the optional barrier with its monitoring, and the dividend yield
    mcamd_price_localvol prices under a surface."""
    _fields_ = [("payoff", C.c_int32), ("barrier", C.c_int32), ("monitoring", C.c_int32), ("reserved", C.c_int32),
                ("q", C.c_double)]


class LocalVolGreeksJob(C.Structure):
    """mcamd_localvol_greeks_job: the payoff, the number of vega time buckets, the dividend yield and gamma's bump in
    ln(S) (0: no gamma) of mcamd_price_localvol_greeks."""
    _fields_ = [("payoff", C.c_int32), ("n_vega_buckets", C.c_uint32), ("q", C.c_double), ("gamma_bump", C.c_double)]


class LocalVolGreeks(C.Structure):
    """mcamd_localvol_greeks: value / std_err / raw sums of price, delta, gamma, vega, rho, rho_q (indexed
    LOCALVOL_GREEK_*) and of the vega buckets."""
    _fields_ = [("value", C.c_double * 6), ("std_err", C.c_double * 6), ("bucket_value", C.c_double * 8),
                ("bucket_std_err", C.c_double * 8), ("sum", C.c_double * 6), ("sumsq", C.c_double * 6),
                ("bucket_sum", C.c_double * 8), ("bucket_sumsq", C.c_double * 8), ("n", C.c_uint64),
                ("kernel_ms", C.c_float), ("total_ms", C.c_float), ("grid", C.c_uint32), ("block", C.c_uint32)]

    def as_dict(self):
        """{name: (value, std_err)} of the six quantities"""
        return {name: (self.value[i], self.std_err[i]) for i, name in enumerate(LOCALVOL_GREEK_NAMES)}


class Cliquet(C.Structure):
    """mcamd_cliquet: the kind (CLIQUET_*), the reset schedule, the local bounds of a period's return, the global bounds
    of the accumulated payoff (-inf / +inf: none) and the dividend yield mcamd_price_cliquet prices with."""
    _fields_ = [("kind", C.c_int32), ("reset_every", C.c_uint32), ("first_period", C.c_uint32), ("reserved", C.c_int32),
                ("local_floor", C.c_double), ("local_cap", C.c_double), ("global_floor", C.c_double),
                ("global_cap", C.c_double), ("q", C.c_double)]


class CliquetResult(C.Structure):
    """mcamd_cliquet_result"""
    _fields_ = [("price", C.c_double), ("std_err", C.c_double), ("ci_lo", C.c_double), ("ci_hi", C.c_double),
                ("sum", C.c_double), ("sumsq", C.c_double), ("n", C.c_uint64), ("n_floored", C.c_uint64),
                ("n_capped", C.c_uint64), ("work_steps", C.c_double), ("kernel_ms", C.c_float), ("total_ms", C.c_float),
                ("grid", C.c_uint32), ("block", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class Heston(C.Structure):
    """mcamd_heston: the payoff, the scheme (HESTON_FULL_TRUNCATION), the dividend yield and the model's parameters
    mcamd_price_heston prices a European option with."""
    _fields_ = [("payoff", C.c_int32), ("scheme", C.c_int32), ("q", C.c_double), ("v0", C.c_double),
                ("kappa", C.c_double), ("theta", C.c_double), ("xi", C.c_double), ("rho", C.c_double),
                ("reserved", C.c_double)]


class HestonResult(C.Structure):
    """mcamd_heston_result"""
    _fields_ = [("price", C.c_double), ("std_err", C.c_double), ("ci_lo", C.c_double), ("ci_hi", C.c_double),
                ("sum", C.c_double), ("sumsq", C.c_double), ("n", C.c_uint64), ("truncated_steps", C.c_double),
                ("mean_variance", C.c_double), ("work_steps", C.c_double), ("kernel_ms", C.c_float),
                ("total_ms", C.c_float), ("grid", C.c_uint32), ("block", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class HestonCliquetResult(C.Structure):
    """mcamd_heston_cliquet_result: mcamd_cliquet_result's fields, then mcamd_heston_result's two diagnostics"""
    _fields_ = CliquetResult._fields_ + [("truncated_steps", C.c_double), ("mean_variance", C.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


assert C.sizeof(HestonCliquetResult) == 112   # pinned in include/mcamd.h


class HestonBarrierResult(C.Structure):
    """mcamd_heston_barrier_result"""
    _fields_ = [("price", C.c_double), ("std_err", C.c_double), ("ci_lo", C.c_double), ("ci_hi", C.c_double),
                ("sum", C.c_double), ("sumsq", C.c_double), ("n", C.c_uint64), ("live_steps", C.c_double),
                ("work_steps", C.c_double), ("truncated_steps", C.c_double), ("mean_variance", C.c_double),
                ("kernel_ms", C.c_float), ("total_ms", C.c_float), ("grid", C.c_uint32), ("block", C.c_uint32)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


assert C.sizeof(HestonBarrierResult) == 104   # pinned in include/mcamd.h


class Smile(C.Structure):
    """mcamd_smile: the payoff of every node, the numbers of expiries and strikes, and the dividend yield
    mcamd_price_localvol_smile prices a strike-by-expiry set of vanillas with."""
    _fields_ = [("payoff", C.c_int32), ("n_expiries", C.c_uint32), ("n_strikes", C.c_uint32), ("reserved", C.c_int32),
                ("q", C.c_double)]


class DeviceInfo(C.Structure):
    _fields_ = [("name", C.c_char * 256), ("arch", C.c_char * 64), ("total_mem", C.c_uint64),
                ("free_mem", C.c_uint64), ("compute_units", C.c_int32), ("wavefront_size", C.c_int32),
                ("max_threads_per_block", C.c_int32), ("clock_khz", C.c_int32), ("mem_clock_khz", C.c_int32),
                ("mem_bus_bits", C.c_int32), ("lds_per_block", C.c_int32), ("regs_per_block", C.c_int32),
                ("l2_bytes", C.c_int32), ("device_index", C.c_int32), ("device_count", C.c_int32),
                ("reserved", C.c_int32)]


class McamdError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"mcamd error {code}: {msg}")
        self.code = code


_lib = None


def load() -> C.CDLL:
    """Loads libmcamd.so; raises if it has not been built (there is no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"{LIB_PATH} not built: run `python __graft_entry__.py build` "
                          "(hipcc --offload-arch=gfx950); the engine has no CPU fallback")
    L = C.CDLL(LIB_PATH)
    vp, u64, i32, f32, f64 = C.c_void_p, C.c_uint64, C.c_int, C.c_float, C.c_double
    L.mcamd_abi_version.restype = i32
    L.mcamd_last_error.restype = C.c_char_p
    L.mcamd_build_id.restype = C.c_char_p
    L.mcamd_device_count.argtypes = [C.POINTER(i32)]
    L.mcamd_ctx_create.argtypes = [i32, vp, C.POINTER(vp)]
    L.mcamd_ctx_destroy.argtypes = [vp]
    L.mcamd_get_device_info.argtypes = [vp, C.POINTER(DeviceInfo)]
    L.mcamd_device_malloc.argtypes = [vp, u64, C.POINTER(vp)]
    L.mcamd_device_free.argtypes = [vp, vp]
    L.mcamd_memcpy_to_host.argtypes = [vp, vp, vp, u64]
    L.mcamd_memcpy_to_device.argtypes = [vp, vp, vp, u64]
    L.mcamd_price_paths.argtypes = [vp, C.POINTER(Option), C.POINTER(Sim), C.POINTER(Result)]
    L.mcamd_price_paths_enqueue.argtypes = [vp, C.POINTER(Option), C.POINTER(Sim), vp]
    L.mcamd_enqueued_kernel_ms.argtypes = [vp, C.c_uint32, C.POINTER(f32)]
    L.mcamd_finalize_stats.argtypes = [C.POINTER(f64), f64, f64, i32, C.POINTER(Result)]
    L.mcamd_group_create.argtypes = [i32, C.POINTER(i32), C.POINTER(vp)]
    L.mcamd_group_destroy.argtypes = [vp]
    L.mcamd_group_size.argtypes = [vp, C.POINTER(i32)]
    L.mcamd_group_price_paths.argtypes = [vp, C.POINTER(Option), C.POINTER(Sim), C.POINTER(Result)]
    L.mcamd_simulate_trajectories.argtypes = [vp, C.POINTER(Option), C.POINTER(Sim), i32, vp, vp, vp,
                                              C.POINTER(Result)]
    L.mcamd_simulate_trajectories_enqueue.argtypes = [vp, C.POINTER(Option), C.POINTER(Sim), i32, vp, vp, vp, vp]
    L.mcamd_nmc_inner_enqueue.argtypes = [vp, C.POINTER(Option), C.POINTER(Sim), i32, i32, vp, vp, vp, vp]
    L.mcamd_nmc_fused_enqueue.argtypes = [vp, C.POINTER(Option), C.POINTER(Sim), u64, i32, vp, vp, vp, vp]
    L.mcamd_finalize_nmc_stats.argtypes = [C.POINTER(f64), C.POINTER(Result)]
    pvp = C.POINTER(vp)
    L.mcamd_group_ctx.argtypes = [vp, i32, C.POINTER(vp)]
    L.mcamd_group_shard.argtypes = [vp, C.POINTER(Sim), i32, C.POINTER(u64), C.POINTER(u64)]
    L.mcamd_group_simulate_trajectories.argtypes = [vp, C.POINTER(Option), C.POINTER(Sim), i32, pvp, pvp, pvp,
                                                    C.POINTER(Result)]
    L.mcamd_group_nmc_inner.argtypes = [vp, C.POINTER(Option), C.POINTER(Sim), i32, i32, pvp, pvp, pvp, C.POINTER(Result)]
    L.mcamd_group_nmc_fused.argtypes = [vp, C.POINTER(Option), C.POINTER(Sim), u64, i32, pvp, pvp, pvp, C.POINTER(Result)]
    L.mcamd_diag_store_pattern.argtypes = [vp, u64, C.c_uint32, i32, vp, vp, C.POINTER(f32)]
    L.mcamd_price_from_normals.argtypes = [vp, C.POINTER(Option), C.POINTER(Sim), vp, vp, C.POINTER(Result)]
    L.mcamd_generate_normals.argtypes = [vp, u64, u64, i32, vp, C.POINTER(f32)]
    L.mcamd_reduce_sum.argtypes = [vp, vp, u64, i32, i32, C.POINTER(f64), C.POINTER(f32)]
    L.mcamd_reduce_partials.argtypes = [vp, vp, u64, i32, i32, C.c_uint32, C.POINTER(f64), C.POINTER(f32)]
    L.mcamd_cpu_mc_f32.argtypes = [C.POINTER(Option), u64, C.c_uint32, u64, i32, C.POINTER(f32), C.POINTER(f32)]
    L.mcamd_nmc_inner.argtypes = [vp, C.POINTER(Option), C.POINTER(Sim), i32, i32, vp, vp, vp, C.POINTER(Result)]
    L.mcamd_nmc_fused.argtypes = [vp, C.POINTER(Option), C.POINTER(Sim), u64, i32, vp, vp, vp, C.POINTER(Result)]
    L.mcamd_finalize.argtypes = [f64, f64, u64, f64, f64, C.POINTER(Result)]
    L.mcamd_finalize_cv.argtypes = [C.POINTER(f64), u64, f64, f64, C.POINTER(Result)]
    L.mcamd_cnd_f32.argtypes = [f32]
    L.mcamd_cnd_f32.restype = f32
    L.mcamd_bs_call_f32.argtypes = [f32] * 5
    L.mcamd_bs_call_f32.restype = f32
    L.mcamd_bs_call_f64.argtypes = [f64] * 5
    L.mcamd_bs_call_f64.restype = f64
    L.mcamd_price_greeks.argtypes = [vp, C.POINTER(Option), C.POINTER(Sim), i32, C.POINTER(Greeks)]
    L.mcamd_price_greeks_enqueue.argtypes = [vp, C.POINTER(Option), C.POINTER(Sim), i32, vp]
    L.mcamd_finalize_greeks_stats.argtypes = [C.POINTER(f64), f64, f64, i32, C.POINTER(Greeks)]
    L.mcamd_group_price_greeks.argtypes = [vp, C.POINTER(Option), C.POINTER(Sim), i32, C.POINTER(Greeks)]
    L.mcamd_bs_greeks_f64.argtypes = [f64, f64, f64, f64, f64, C.POINTER(f64)]
    L.mcamd_american_workspace_bytes.argtypes = [C.POINTER(American), C.POINTER(Sim), C.POINTER(u64)]
    L.mcamd_price_american.argtypes = [vp, C.POINTER(Option), C.POINTER(Sim), C.POINTER(American), vp, u64,
                                       C.POINTER(f64), C.POINTER(AmericanResult)]
    L.mcamd_american_dual_workspace_bytes.argtypes = [C.POINTER(American), C.POINTER(Sim), C.POINTER(AmericanDual),
                                                      C.POINTER(u64)]
    L.mcamd_american_upper_bound.argtypes = [vp, C.POINTER(Option), C.POINTER(Sim), C.POINTER(American),
                                             C.POINTER(AmericanDual), C.POINTER(f64), vp, u64, vp,
                                             C.POINTER(AmericanDualResult)]
    L.mcamd_price_barrier.argtypes = [vp, C.POINTER(Option), C.POINTER(Sim), C.POINTER(Barrier), vp, C.POINTER(Result)]
    L.mcamd_price_barrier_enqueue.argtypes = [vp, C.POINTER(Option), C.POINTER(Sim), C.POINTER(Barrier), vp, vp]
    L.mcamd_barrier_price_f64.argtypes = [f64, f64, f64, f64, f64, f64, i32, i32, C.POINTER(f64)]
    L.mcamd_price_lookback.argtypes = [vp, C.POINTER(Option), C.POINTER(Sim), C.POINTER(Lookback), vp, C.POINTER(Result)]
    L.mcamd_price_lookback_enqueue.argtypes = [vp, C.POINTER(Option), C.POINTER(Sim), C.POINTER(Lookback), vp, vp]
    L.mcamd_lookback_price_f64.argtypes = [f64, f64, f64, f64, f64, i32, i32, C.POINTER(f64)]
    L.mcamd_price_basket.argtypes = [vp, C.POINTER(Option), C.POINTER(Sim), C.POINTER(Basket), vp, C.POINTER(Result)]
    L.mcamd_price_basket_enqueue.argtypes = [vp, C.POINTER(Option), C.POINTER(Sim), C.POINTER(Basket), vp, vp]
    L.mcamd_basket_geometric_price_f64.argtypes = [C.POINTER(Basket), f64, f64, f64, C.POINTER(f64)]
    L.mcamd_exchange_price_f64.argtypes = [f64, f64, f64, f64, f64, f64, C.POINTER(f64)]
    L.mcamd_price_asian.argtypes = [vp, C.POINTER(Option), C.POINTER(Sim), C.POINTER(Asian), vp, C.POINTER(Result)]
    L.mcamd_price_asian_enqueue.argtypes = [vp, C.POINTER(Option), C.POINTER(Sim), C.POINTER(Asian), vp, vp]
    L.mcamd_asian_geometric_price_f64.argtypes = [f64, f64, f64, f64, f64, C.c_uint32, i32, i32, i32, C.POINTER(f64)]
    L.mcamd_price_autocall.argtypes = [vp, C.POINTER(Option), C.POINTER(Sim), C.POINTER(Autocall), vp,
                                       C.POINTER(AutocallResult)]
    L.mcamd_price_autocall_enqueue.argtypes = [vp, C.POINTER(Option), C.POINTER(Sim), C.POINTER(Autocall), vp, vp]
    L.mcamd_price_autocall_localvol.argtypes = [vp, C.POINTER(Option), C.POINTER(Sim), C.POINTER(AutocallLocalVol),
                                                C.POINTER(vp), vp, C.POINTER(AutocallResult)]
    L.mcamd_price_autocall_localvol_enqueue.argtypes = [vp, C.POINTER(Option), C.POINTER(Sim),
                                                        C.POINTER(AutocallLocalVol), C.POINTER(vp), vp, vp]
    L.mcamd_autocall_single_date_price_f64.argtypes = [f64, f64, f64, f64, f64, f64, i32, C.POINTER(f64)]
    L.mcamd_localvol_surface_create.argtypes = [vp, C.POINTER(LocalVolGrid), C.POINTER(f64), C.POINTER(vp)]
    L.mcamd_localvol_surface_destroy.argtypes = [vp]
    L.mcamd_price_localvol.argtypes = [vp, C.POINTER(Option), C.POINTER(Sim), C.POINTER(LocalVol), vp, vp,
                                       C.POINTER(Result)]
    L.mcamd_price_localvol_enqueue.argtypes = [vp, C.POINTER(Option), C.POINTER(Sim), C.POINTER(LocalVol), vp, vp, vp]
    L.mcamd_price_cliquet.argtypes = [vp, C.POINTER(Option), C.POINTER(Sim), C.POINTER(Cliquet), vp, vp,
                                      C.POINTER(CliquetResult)]
    L.mcamd_price_cliquet_enqueue.argtypes = [vp, C.POINTER(Option), C.POINTER(Sim), C.POINTER(Cliquet), vp, vp, vp]
    L.mcamd_cliquet_price_f64.argtypes = [i32, f64, f64, f64, C.c_uint32, C.c_uint32, C.POINTER(f64), f64, f64,
                                          C.POINTER(f64)]
    L.mcamd_price_heston.argtypes = [vp, C.POINTER(Option), C.POINTER(Sim), C.POINTER(Heston), vp, vp,
                                     C.POINTER(HestonResult)]
    L.mcamd_price_heston_enqueue.argtypes = [vp, C.POINTER(Option), C.POINTER(Sim), C.POINTER(Heston), vp, vp, vp]
    L.mcamd_heston_price_f64.argtypes = [f64] * 10 + [i32, C.POINTER(f64)]
    L.mcamd_price_heston_cliquet.argtypes = [vp, C.POINTER(Option), C.POINTER(Sim), C.POINTER(Heston), C.POINTER(Cliquet),
                                             vp, C.POINTER(HestonCliquetResult)]
    L.mcamd_price_heston_cliquet_enqueue.argtypes = [vp, C.POINTER(Option), C.POINTER(Sim), C.POINTER(Heston),
                                                     C.POINTER(Cliquet), vp, vp]
    L.mcamd_price_heston_barrier.argtypes = [vp, C.POINTER(Option), C.POINTER(Sim), C.POINTER(Heston), C.POINTER(Barrier),
                                             vp, vp, C.POINTER(HestonBarrierResult)]
    L.mcamd_price_heston_barrier_enqueue.argtypes = [vp, C.POINTER(Option), C.POINTER(Sim), C.POINTER(Heston),
                                                     C.POINTER(Barrier), vp, vp, vp]
    L.mcamd_heston_cliquet_price_f64.argtypes =[i32] + [f64] * 8 + [C.c_uint32, C.c_uint32, f64, f64, C.POINTER(f64)]
    L.mcamd_localvol_sigma_f64.argtypes = [C.POINTER(LocalVolGrid), C.POINTER(f64), C.c_uint32, C.c_uint32, f64,
                                           C.POINTER(f64)]
    L.mcamd_bs_price_f64.argtypes = [f64, f64, f64, f64, f64, f64, i32, C.POINTER(f64)]
    L.mcamd_bs_implied_vol_f64.argtypes = [f64, f64, f64, f64, f64, i32, f64, C.POINTER(f64)]
    u32p = C.POINTER(C.c_uint32)
    L.mcamd_price_localvol_smile.argtypes = [vp, C.POINTER(Option), C.POINTER(Sim), C.POINTER(Smile), u32p,
                                             C.POINTER(f64), vp, vp, C.POINTER(f64), C.POINTER(Result)]
    L.mcamd_price_localvol_smile_enqueue.argtypes = [vp, C.POINTER(Option), C.POINTER(Sim), C.POINTER(Smile), u32p,
                                                     C.POINTER(f64), vp, vp, vp]
    L.mcamd_finalize_smile.argtypes = [C.POINTER(f64), u64, C.POINTER(Option), C.c_uint32, C.POINTER(Smile), u32p,
                                       C.POINTER(f64), C.POINTER(f64)]
    L.mcamd_price_heston_smile.argtypes = [vp, C.POINTER(Option), C.POINTER(Sim), C.POINTER(Heston), C.c_uint32, C.c_uint32,
                                           u32p, C.POINTER(f64), vp, C.POINTER(f64), C.POINTER(Result)]
    L.mcamd_price_heston_smile_enqueue.argtypes = [vp, C.POINTER(Option), C.POINTER(Sim), C.POINTER(Heston), C.c_uint32,
                                                   C.c_uint32, u32p, C.POINTER(f64), vp, vp]
    L.mcamd_price_localvol_greeks.argtypes = [vp, C.POINTER(Option), C.POINTER(Sim), C.POINTER(LocalVolGreeksJob), vp, vp,
                                              C.POINTER(LocalVolGreeks)]
    L.mcamd_price_localvol_greeks_enqueue.argtypes = [vp, C.POINTER(Option), C.POINTER(Sim), C.POINTER(LocalVolGreeksJob),
                                                      vp, vp, vp]
    L.mcamd_finalize_localvol_greeks_stats.argtypes = [C.POINTER(f64), f64, f64, C.c_uint32, i32,
                                                       C.POINTER(LocalVolGreeks)]
    for name in EXPORTS:
        fn = getattr(L, name)
        if fn.restype is C.c_int and name not in ("mcamd_abi_version",):
            fn.restype = C.c_int
    _lib = L
    return L


def _check(rc: int):
    if rc != OK:
        raise McamdError(rc, load().mcamd_last_error().decode())


def make_option(S0=100.0, T=1.0, K=100.0, r=0.1, v=0.2, B=0.0, P1=0, P2=0, use_window=0, Ik=0, Sk=0.0,
                Tk=0, dt=0.0) -> Option:
    return Option(S0, T, K, r, v, B, P1, P2, use_window, Ik, Sk, Tk, 0, dt)


def make_sim(n_paths, n_steps=1, precision=F64, seed=1234, path_offset=0, n_paths_local=None,
             n_paths_inner=0, flags=0) -> Sim:
    return Sim(n_paths, path_offset, n_paths if n_paths_local is None else n_paths_local, n_steps, n_paths_inner,
               seed, precision, flags)


def make_american(payoff=PAYOFF_PUT, exercise_every=1, n_basis=0, n_train=100_000, train_seed=4321) -> American:
    return American(payoff, exercise_every, n_basis, 0, n_train, train_seed)


def american_workspace_bytes(am: American, sim: Sim) -> int:
    """bytes of the device workspace mcamd_price_american needs for this rule, training set and step count"""
    b = C.c_uint64(0)
    _check(load().mcamd_american_workspace_bytes(C.byref(am), C.byref(sim), C.byref(b)))
    return b.value


def make_american_dual(n_inner=256, inner_seed=8765) -> AmericanDual:
    return AmericanDual(n_inner, 0, inner_seed)


def american_dual_workspace_bytes(am: American, sim: Sim, dual: AmericanDual) -> int:
    """bytes of the device workspace mcamd_american_upper_bound needs for this outer shard and these dates"""
    b = C.c_uint64(0)
    _check(load().mcamd_american_dual_workspace_bytes(C.byref(am), C.byref(sim), C.byref(dual), C.byref(b)))
    return b.value


def make_barrier(kind=BARRIER_DOWN_OUT, payoff=PAYOFF_CALL, monitoring=MONITOR_CONTINUOUS) -> Barrier:
    return Barrier(kind, payoff, monitoring, 0)


def barrier_price_f64(S0, K, B, T, r, sigma, kind=BARRIER_DOWN_OUT, payoff=PAYOFF_CALL) -> float:
    """closed form of the continuously monitored single barrier (Reiner-Rubinstein), rebate 0"""
    p = C.c_double(0)
    _check(load().mcamd_barrier_price_f64(S0, K, B, T, r, sigma, kind, payoff, C.byref(p)))
    return p.value


def make_lookback(strike=LOOKBACK_FLOATING, payoff=PAYOFF_CALL, monitoring=MONITOR_CONTINUOUS) -> Lookback:
    return Lookback(strike, payoff, monitoring, 0)


def lookback_price_f64(S0, K, T, r, sigma, strike=LOOKBACK_FLOATING, payoff=PAYOFF_CALL) -> float:
    """closed form of the continuously monitored, newly issued lookback (Goldman-Sosin-Gatto, Conze-Viswanathan)"""
    p = C.c_double(0)
    _check(load().mcamd_lookback_price_f64(S0, K, T, r, sigma, strike, payoff, C.byref(p)))
    return p.value


def make_basket(S0, v, w, corr, kind=BASKET_ARITHMETIC, payoff=PAYOFF_CALL, barrier=BASKET_NO_BARRIER) -> Basket:
    """S0, v, w: d values each (d = len(S0), at most BASKET_MAX_ASSETS); corr: d x d (nested sequences or an array)."""
    d = len(S0)
    if not 1 <= d <= BASKET_MAX_ASSETS or len(v) != d or len(w) != d or len(corr) != d or any(len(row) != d for row in corr):
        raise ValueError(f"a basket takes 1..{BASKET_MAX_ASSETS} assets and S0, v, w of d and corr of d x d values")
    b = Basket(d, kind, payoff, barrier)
    for j in range(d):
        b.S0[j], b.v[j], b.w[j] = float(S0[j]), float(v[j]), float(w[j])
        for k in range(d):
            b.corr[8 * j + k] = float(corr[j][k])
    return b


def basket_geometric_price_f64(basket: Basket, K, T, r) -> float:
    """closed form of the geometric basket (a lognormal); basket.payoff selects call or put"""
    p = C.c_double(0)
    _check(load().mcamd_basket_geometric_price_f64(C.byref(basket), K, T, r, C.byref(p)))
    return p.value


def exchange_price_f64(a_S1, b_S2, T, v1, v2, rho) -> float:
    """Margrabe's closed form of (a S1 - b S2)+, with a_S1 = a S1(0) and b_S2 = b S2(0)"""
    p = C.c_double(0)
    _check(load().mcamd_exchange_price_f64(a_S1, b_S2, T, v1, v2, rho, C.byref(p)))
    return p.value


def make_asian(average=ASIAN_ARITHMETIC, strike=ASIAN_FIXED, payoff=PAYOFF_CALL, include_spot=0,
               control=ASIAN_CONTROL_NONE) -> Asian:
    return Asian(average, strike, payoff, include_spot, control, 0)


def asian_geometric_price_f64(S0, K, T, r, sigma, n_steps, include_spot=0, strike=ASIAN_FIXED, payoff=PAYOFF_CALL) -> float:
    """closed form of the discrete geometric-average option over the n_steps step ends (and t = 0 with include_spot)"""
    p = C.c_double(0)
    _check(load().mcamd_asian_geometric_price_f64(S0, K, T, r, sigma, n_steps, include_spot, strike, payoff, C.byref(p)))
    return p.value


def make_autocall(v, corr, observe_every=1, call_level=1.0, coupon=0.0, ki_level=0.0,
                  ki_monitoring=AUTOCALL_KI_NONE, call_step_down=0.0, first_call_date=1) -> Autocall:
    """v: d volatilities (d at most BASKET_MAX_ASSETS); corr: d x d (nested sequences or an array)."""
    d = len(v)
    if not 1 <= d <= BASKET_MAX_ASSETS or len(corr) != d or any(len(row) != d for row in corr):
        raise ValueError(f"an autocallable takes 1..{BASKET_MAX_ASSETS} assets, v of d and corr of d x d values")
    a = Autocall(d, ki_monitoring, observe_every, first_call_date)
    a.call_level, a.call_step_down, a.coupon, a.ki_level = call_level, call_step_down, coupon, ki_level
    for j in range(d):
        a.v[j] = float(v[j])
        for k in range(d):
            a.corr[8 * j + k] = float(corr[j][k])
    return a


def make_autocall_localvol(q, corr, observe_every=1, call_level=1.0, coupon=0.0, ki_level=0.0,
                           ki_monitoring=AUTOCALL_KI_NONE, call_step_down=0.0, first_call_date=1) -> AutocallLocalVol:
    """q: d dividend yields (d at most BASKET_MAX_ASSETS); corr: d x d (nested sequences or an array)."""
    d = len(q)
    if not 1 <= d <= BASKET_MAX_ASSETS or len(corr) != d or any(len(row) != d for row in corr):
        raise ValueError(f"an autocallable takes 1..{BASKET_MAX_ASSETS} assets, q of d and corr of d x d values")
    a = AutocallLocalVol(d, ki_monitoring, observe_every, first_call_date)
    a.call_level, a.call_step_down, a.coupon, a.ki_level = call_level, call_step_down, coupon, ki_level
    for j in range(d):
        a.q[j] = float(q[j])
        for k in range(d):
            a.corr[8 * j + k] = float(corr[j][k])
    return a


def surface_array(surfaces):
    """the host array of surface pointers the autocall calls under local volatility take: None stays NULL, and so does
    an entry that is None"""
    if surfaces is None:
        return None
    return (C.c_void_p * max(len(surfaces), 1))(*[None if s is None else s._h for s in surfaces])


def autocall_single_date_price_f64(T, r, sigma, call_level, coupon, ki_level=0.0, ki_monitoring=AUTOCALL_KI_NONE) -> float:
    """closed form of the autocallable on one asset with one date (no knock-in, or a knock-in at maturity)"""
    p = C.c_double(0)
    _check(load().mcamd_autocall_single_date_price_f64(T, r, sigma, call_level, coupon, ki_level, ki_monitoring,
                                                       C.byref(p)))
    return p.value


def make_localvol(payoff=PAYOFF_CALL, barrier=LOCALVOL_NO_BARRIER, monitoring=MONITOR_DISCRETE, q=0.0) -> LocalVol:
    return LocalVol(payoff, barrier, monitoring, 0, q)


def make_cliquet(kind=CLIQUET_SUM, reset_every=1, first_period=1, local_floor=-math.inf, local_cap=math.inf,
                 global_floor=-math.inf, global_cap=math.inf, q=0.0) -> Cliquet:
    return Cliquet(kind, reset_every, first_period, 0, local_floor, local_cap, global_floor, global_cap, q)


def cliquet_price(kind, T, r, q, period_vol, first_period=1, local_floor=-math.inf, local_cap=math.inf) -> float:
    """Closed form of a cliquet without a global clip where the volatility varies in time only
    (mcamd_cliquet_price_f64); period_vol: the rms volatility of each of the n_periods = len(period_vol) periods."""
    vols = (C.c_double * len(period_vol))(*[float(v) for v in period_vol])
    out = C.c_double()
    _check(load().mcamd_cliquet_price_f64(kind, T, r, q, len(period_vol), first_period, vols, local_floor, local_cap,
                                          C.byref(out)))
    return out.value


def make_heston(payoff=PAYOFF_CALL, q=0.0, v0=0.04, kappa=2.0, theta=0.04, xi=0.3, rho=-0.7,
                scheme=HESTON_FULL_TRUNCATION) -> Heston:
    return Heston(payoff, scheme, q, v0, kappa, theta, xi, rho, 0.0)


def heston_price(S0, K, T, r, q, v0, kappa, theta, xi, rho, payoff=PAYOFF_CALL) -> float:
    """Closed form of a European option under Heston (mcamd_heston_price_f64): the model's price, which the
    full-truncation scheme of price_heston approaches at first order in the step."""
    out = C.c_double()
    _check(load().mcamd_heston_price_f64(S0, K, T, r, q, v0, kappa, theta, xi, rho, payoff, C.byref(out)))
    return out.value


def heston_cliquet_price(kind, T, r, q, v0, kappa, theta, xi, rho, n_periods, first_period=1, local_floor=-math.inf,
                         local_cap=math.inf) -> float:
    """Closed form of an additive cliquet, a one-period compounding one or a discretely sampled variance swap under
    Heston, without a global clip (mcamd_heston_cliquet_price_f64): the model's price, through the forward
    characteristic function of the period returns."""
    out = C.c_double()
    _check(load().mcamd_heston_cliquet_price_f64(kind, T, r, q, v0, kappa, theta, xi, rho, n_periods, first_period,
                                                 local_floor, local_cap, C.byref(out)))
    return out.value


def heston_smile_prices(S0, strikes, times, r, q, v0, kappa, theta, xi, rho, payoff=PAYOFF_CALL):
    """The closed-form grid of a Heston smile: heston_price (mcamd_heston_price_f64) at every node, as a
    (len(times), len(strikes)) numpy array; times[m] is the expiry of row m in years."""
    import numpy as np
    return np.array([[heston_price(S0, float(K), float(t), r, q, v0, kappa, theta, xi, rho, payoff) for K in strikes]
                     for t in times])


def make_localvol_greeks_job(payoff=PAYOFF_CALL, n_vega_buckets=0, q=0.0, gamma_bump=0.0) -> LocalVolGreeksJob:
    return LocalVolGreeksJob(payoff, n_vega_buckets, q, gamma_bump)


def make_localvol_grid(n_t, n_x, x_min, x_max) -> LocalVolGrid:
    return LocalVolGrid(n_t, n_x, x_min, x_max)


def _sigma_array(grid: LocalVolGrid, sigma):
    """the table as n_t * n_x C doubles (any nested sequence or numpy array of that many finite-or-not values)"""
    flat = [float(v) for row in sigma for v in (row if hasattr(row, "__iter__") else (row,))]
    if len(flat) != grid.n_t * grid.n_x:
        raise ValueError(f"sigma holds {len(flat)} values; the grid has n_t * n_x = {grid.n_t * grid.n_x} nodes")
    return (C.c_double * len(flat))(*flat)


def localvol_sigma_f64(grid, sigma, n_steps, step, x) -> float:
    """the volatility step `step` of n_steps uses at x = ln(S / S0) (mcamd_localvol_sigma_f64); grid: a LocalVolGrid
    or its (n_t, n_x, x_min, x_max)"""
    g = grid if isinstance(grid, LocalVolGrid) else make_localvol_grid(*grid)
    out = C.c_double(0)
    _check(load().mcamd_localvol_sigma_f64(C.byref(g), _sigma_array(g, sigma), n_steps, step, x, C.byref(out)))
    return out.value


def bs_price_f64(S0, K, T, r, q, sigma, payoff=PAYOFF_CALL) -> float:
    """Black-Scholes with a continuous dividend yield q"""
    p = C.c_double(0)
    _check(load().mcamd_bs_price_f64(S0, K, T, r, q, sigma, payoff, C.byref(p)))
    return p.value


def bs_implied_vol(S0, K, T, r, q, price, payoff=PAYOFF_CALL) -> float:
    """the volatility at which bs_price_f64 gives `price` (mcamd_bs_implied_vol_f64); raises McamdError for a price
    that is not strictly inside the no-arbitrage bounds"""
    v = C.c_double(0)
    _check(load().mcamd_bs_implied_vol_f64(S0, K, T, r, q, payoff, price, C.byref(v)))
    return v.value


def make_smile(n_expiries, n_strikes, payoff=PAYOFF_CALL, q=0.0) -> Smile:
    return Smile(payoff, n_expiries, n_strikes, 0, q)


def _smile_arrays(smile: Smile, expiry_steps, strikes):
    """the expiry steps and strikes as C arrays of the lengths the smile states"""
    steps, ks = [int(s) for s in expiry_steps], [float(k) for k in strikes]
    if len(steps) != smile.n_expiries or len(ks) != smile.n_strikes:
        raise ValueError(f"the smile states {smile.n_expiries} expiries and {smile.n_strikes} strikes; got {len(steps)} "
                         f"and {len(ks)}")
    return (C.c_uint32 * max(len(steps), 1))(*steps), (C.c_double * max(len(ks), 1))(*ks)


def finalize_smile(stats, n, opt: Option, n_steps, smile: Smile, expiry_steps):
    """(price, std_err) as (n_expiries, n_strikes) numpy arrays from the 2 n_e n_K sums of n paths
    (mcamd_finalize_smile): every node is discounted to its own expiry"""
    import numpy as np
    nodes = smile.n_expiries * smile.n_strikes
    arr = (C.c_double * (2 * nodes))(*[float(x) for x in list(stats)[:2 * nodes]])
    steps, _ = _smile_arrays(smile, expiry_steps, [1.0] * smile.n_strikes)
    price, se = (C.c_double * nodes)(), (C.c_double * nodes)()
    _check(load().mcamd_finalize_smile(arr, int(n), C.byref(opt), n_steps, C.byref(smile), steps, price, se))
    shape = (smile.n_expiries, smile.n_strikes)
    return np.array(price[:]).reshape(shape), np.array(se[:]).reshape(shape)


def _smile_sync(opt: Option, sim: Sim, smile: Smile, expiry_steps, call):
    """the tail of both synchronous smile methods: call(stats, res) runs the C call on the host sums' buffer and the
    result's reference; returns (price, std_err, stats, res)"""
    import numpy as np
    nodes = smile.n_expiries * smile.n_strikes
    stats, res = (C.c_double * max(2 * nodes, 1))(), Result()
    _check(call(stats, C.byref(res)))
    price, se = finalize_smile(stats, res.n, opt, sim.n_steps, smile, expiry_steps)
    return price, se, np.array(stats[:2 * nodes]), res


def implied_vols(S0, strikes, times, r, q, prices, payoff=PAYOFF_CALL):
    """bs_implied_vol over a price array: prices[m][k] is the option at times[m] struck at strikes[k].  NaN where a
    price lies outside the no-arbitrage bounds; never raises for that."""
    import numpy as np
    prices = np.asarray(prices, dtype=np.float64)
    out = np.full(prices.shape, np.nan)
    L, v = load(), C.c_double(0)
    for m, t in enumerate(times):
        for k, K in enumerate(strikes):
            if L.mcamd_bs_implied_vol_f64(S0, float(K), float(t), r, q, payoff, float(prices[m, k]), C.byref(v)) == OK:
                out[m, k] = v.value
    return out


def _ptr(t):
    """device pointer of a torch tensor (or None / int passthrough)"""
    if t is None:
        return None
    if isinstance(t, int):
        return C.c_void_p(t)
    return C.c_void_p(t.data_ptr())


def finalize(sum_, sumsq, n, r, T) -> Result:
    res = Result()
    _check(load().mcamd_finalize(sum_, sumsq, n, r, T, C.byref(res)))
    return res


def finalize_cv(sums, n, r, T) -> Result:
    res = Result()
    arr = (C.c_double * 5)(*sums)
    _check(load().mcamd_finalize_cv(arr, n, r, T, C.byref(res)))
    return res


def finalize_stats(stats6, r, T, control_variate=False) -> Result:
    res = Result()
    arr = (C.c_double * 6)(*[float(x) for x in stats6])
    _check(load().mcamd_finalize_stats(arr, r, T, int(control_variate), C.byref(res)))
    return res


def finalize_nmc_stats(stats6) -> Result:
    res = Result()
    arr = (C.c_double * 6)(*[float(x) for x in stats6])
    _check(load().mcamd_finalize_nmc_stats(arr, C.byref(res)))
    return res


def finalize_greeks_stats(stats16, r, T, theta_defined=True) -> Greeks:
    """Greeks of a (possibly all-reduced) 16-double record left by Context.price_greeks_enqueue."""
    out = Greeks()
    arr = (C.c_double * GREEKS_STATS)(*[float(x) for x in stats16])
    _check(load().mcamd_finalize_greeks_stats(arr, r, T, int(theta_defined), C.byref(out)))
    return out


def finalize_localvol_greeks_stats(stats32, r, T, n_vega_buckets=0, gamma_defined=True) -> LocalVolGreeks:
    """Greeks of a (possibly all-reduced) 32-double record left by Context.price_localvol_greeks_enqueue."""
    out = LocalVolGreeks()
    arr = (C.c_double * LOCALVOL_GREEKS_STATS)(*[float(x) for x in stats32])
    _check(load().mcamd_finalize_localvol_greeks_stats(arr, r, T, n_vega_buckets, int(gamma_defined), C.byref(out)))
    return out


def bs_greeks_f64(S0, K, T, r, sigma):
    """closed-form (price, delta, gamma, vega, rho, theta) of the call"""
    arr = (C.c_double * 6)()
    _check(load().mcamd_bs_greeks_f64(S0, K, T, r, sigma, arr))
    return list(arr)


def cpu_mc_f32(opt: Option, n_paths: int, n_steps: int, seed: int = 0, from_random_device: bool = False):
    """(price, undiscounted fp32 payoff sum) of the reference's serial CPU Monte Carlo (mcamd_cpu_mc_f32)"""
    p, s = C.c_float(0), C.c_float(0)
    _check(load().mcamd_cpu_mc_f32(C.byref(opt), n_paths, n_steps, seed, int(from_random_device), C.byref(p), C.byref(s)))
    return p.value, s.value


def cnd_f32(x):
    return float(load().mcamd_cnd_f32(x))


def bs_call_f32(S0, K, T, r, sigma):
    return float(load().mcamd_bs_call_f32(S0, K, T, r, sigma))


def bs_call_f64(S0, K, T, r, sigma):
    return float(load().mcamd_bs_call_f64(S0, K, T, r, sigma))


def build_id() -> str:
    return load().mcamd_build_id().decode()


def device_count() -> int:
    n = C.c_int(0)
    rc = load().mcamd_device_count(C.byref(n))
    return n.value if rc == OK else 0


class Context:
    """Owns one mcamd_ctx (one device, one stream)."""

    def __init__(self, device: int = 0, stream: int | None = None):
        self._L = load()
        self._h = C.c_void_p()
        _check(self._L.mcamd_ctx_create(device, C.c_void_p(stream) if stream else None, C.byref(self._h)))

    def close(self):
        if self._h:
            self._L.mcamd_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def device_info(self) -> DeviceInfo:
        info = DeviceInfo()
        _check(self._L.mcamd_get_device_info(self._h, C.byref(info)))
        return info

    def price_paths(self, opt: Option, sim: Sim) -> Result:
        res = Result()
        _check(self._L.mcamd_price_paths(self._h, C.byref(opt), C.byref(sim), C.byref(res)))
        return res

    def price_paths_enqueue(self, opt: Option, sim: Sim, stats) -> None:
        """Asynchronous: leaves {sum, sumsq, sum_c, sum_cc, sum_yc, n} in the device tensor `stats` (>= 6 doubles)."""
        _check(self._L.mcamd_price_paths_enqueue(self._h, C.byref(opt), C.byref(sim), _ptr(stats)))

    def price_greeks(self, opt: Option, sim: Sim, method: int = GREEKS_AUTO) -> Greeks:
        out = Greeks()
        _check(self._L.mcamd_price_greeks(self._h, C.byref(opt), C.byref(sim), method, C.byref(out)))
        return out

    def price_greeks_enqueue(self, opt: Option, sim: Sim, stats, method: int = GREEKS_AUTO) -> None:
        """Asynchronous: leaves the 16-double Greeks record in the device tensor `stats` (finalize_greeks_stats)."""
        _check(self._L.mcamd_price_greeks_enqueue(self._h, C.byref(opt), C.byref(sim), method, _ptr(stats)))

    def price_barrier(self, opt: Option, sim: Sim, barrier: Barrier, samples=None) -> Result:
        """Single-barrier option (mcamd_price_barrier); opt.B is the level.  samples: optional device tensor of
        n_paths_local values of the path precision that receives each path's undiscounted sample."""
        res = Result()
        _check(self._L.mcamd_price_barrier(self._h, C.byref(opt), C.byref(sim), C.byref(barrier), _ptr(samples),
                                           C.byref(res)))
        return res

    def price_barrier_enqueue(self, opt: Option, sim: Sim, barrier: Barrier, stats, samples=None) -> None:
        """Asynchronous: leaves {sum, sumsq, 0, 0, 0, n} in the device tensor `stats` (>= 6 doubles; finalize_stats)."""
        _check(self._L.mcamd_price_barrier_enqueue(self._h, C.byref(opt), C.byref(sim), C.byref(barrier),
                                                   _ptr(samples), _ptr(stats)))

    def localvol_surface(self, grid_args, sigma) -> "LocalVolSurface":
        """An immutable local-volatility surface on this context (mcamd_localvol_surface_create).  grid_args: a
        LocalVolGrid or its (n_t, n_x, x_min, x_max); sigma: n_t rows of n_x volatilities.  close() it (or use it as a
        context manager) before the context is closed."""
        return LocalVolSurface(self, grid_args, sigma)

    def price_localvol(self, opt: Option, sim: Sim, localvol: LocalVol, surface: "LocalVolSurface", samples=None) -> Result:
        """European or single-barrier option under a local-volatility surface (mcamd_price_localvol); opt.v is
        ignored, opt.B is the barrier level.  samples: optional device tensor of n_paths_local values of the path
        precision that receives each path's undiscounted sample."""
        res = Result()
        _check(self._L.mcamd_price_localvol(self._h, C.byref(opt), C.byref(sim), C.byref(localvol), surface._h,
                                            _ptr(samples), C.byref(res)))
        return res

    def price_localvol_enqueue(self, opt: Option, sim: Sim, localvol: LocalVol, surface: "LocalVolSurface", stats,
                               samples=None) -> None:
        """Asynchronous: leaves {sum, sumsq, 0, 0, 0, n} in the device tensor `stats` (>= 6 doubles; finalize_stats)."""
        _check(self._L.mcamd_price_localvol_enqueue(self._h, C.byref(opt), C.byref(sim), C.byref(localvol), surface._h,
                                                    _ptr(samples), _ptr(stats)))

    def price_cliquet(self, opt: Option, sim: Sim, cliquet: Cliquet, surface: "LocalVolSurface",
                      samples=None) -> CliquetResult:
        """Cliquet, forward-start option or realized-variance swap on the paths of price_localvol
        (mcamd_price_cliquet); r, T and S0 come from opt, opt.v, opt.K and opt.B are ignored.  samples: optional device
        tensor of n_paths_local values of the path precision that receives each path's undiscounted sample."""
        res = CliquetResult()
        _check(self._L.mcamd_price_cliquet(self._h, C.byref(opt), C.byref(sim), C.byref(cliquet), surface._h,
                                           _ptr(samples), C.byref(res)))
        return res

    def price_cliquet_enqueue(self, opt: Option, sim: Sim, cliquet: Cliquet, surface: "LocalVolSurface", stats,
                              samples=None) -> None:
        """Asynchronous: leaves {sum, sumsq, n_floored, n_capped, 0, n} in the device tensor `stats` (>= 6 doubles;
        finalize_stats)."""
        _check(self._L.mcamd_price_cliquet_enqueue(self._h, C.byref(opt), C.byref(sim), C.byref(cliquet), surface._h,
                                                   _ptr(samples), _ptr(stats)))

    def price_heston(self, opt: Option, sim: Sim, heston: Heston, samples=None, state=None) -> HestonResult:
        """European option under Heston stochastic volatility, full-truncation Euler in the log-price
        (mcamd_price_heston); r, T, S0 and K come from opt, opt.v and opt.B are ignored.  samples: optional device
        tensor of n_paths_local values of the path precision that receives each path's undiscounted sample; state:
        optional device tensor of 2 x n_paths_local such values that receives S_T, then the raw final variance."""
        res = HestonResult()
        _check(self._L.mcamd_price_heston(self._h, C.byref(opt), C.byref(sim), C.byref(heston), _ptr(samples),
                                          _ptr(state), C.byref(res)))
        return res

    def price_heston_enqueue(self, opt: Option, sim: Sim, heston: Heston, stats, samples=None, state=None) -> None:
        """Asynchronous: leaves {sum, sumsq, truncated_steps, sum of the paths' average variance, 0, n} in the device
        tensor `stats` (>= 6 doubles; finalize_stats)."""
        _check(self._L.mcamd_price_heston_enqueue(self._h, C.byref(opt), C.byref(sim), C.byref(heston), _ptr(samples),
                                                  _ptr(state), _ptr(stats)))

    def price_heston_cliquet(self, opt: Option, sim: Sim, heston: Heston, cliquet: Cliquet,
                             samples=None) -> HestonCliquetResult:
        """Cliquet, forward-start option or realized-variance swap on the paths of price_heston
        (mcamd_price_heston_cliquet); r, T and S0 come from opt, opt.v, opt.K and opt.B are ignored, heston.payoff is
        not read and cliquet.q must equal heston.q.  samples: optional device tensor of n_paths_local values of the
        path precision that receives each path's undiscounted sample."""
        res = HestonCliquetResult()
        _check(self._L.mcamd_price_heston_cliquet(self._h, C.byref(opt), C.byref(sim), C.byref(heston), C.byref(cliquet),
                                                  _ptr(samples), C.byref(res)))
        return res

    def price_heston_cliquet_enqueue(self, opt: Option, sim: Sim, heston: Heston, cliquet: Cliquet, stats,
                                     samples=None) -> None:
        """Asynchronous: leaves {sum, sumsq, n_floored, n_capped, sum of the paths' average variance, n} in the device
        tensor `stats` (>= 6 doubles; finalize_stats)."""
        _check(self._L.mcamd_price_heston_cliquet_enqueue(self._h, C.byref(opt), C.byref(sim), C.byref(heston),
                                                          C.byref(cliquet), _ptr(samples), _ptr(stats)))

    def price_heston_barrier(self, opt: Option, sim: Sim, heston: Heston, barrier: Barrier, samples=None,
                             state=None) -> HestonBarrierResult:
        """Single-barrier option on the paths of price_heston (mcamd_price_heston_barrier); r, T, S0, K and the level B
        come from opt, opt.v is ignored, and heston.payoff must equal barrier.payoff.  samples: optional device tensor
        of n_paths_local values of the path precision that receives each path's undiscounted sample; state: optional
        device tensor of 3 x n_paths_local such values that receives S_T, then the raw final variance, then the
        survival weight (a knock-out path that was hit: NaN, NaN, 0)."""
        res = HestonBarrierResult()
        _check(self._L.mcamd_price_heston_barrier(self._h, C.byref(opt), C.byref(sim), C.byref(heston), C.byref(barrier),
                                                  _ptr(samples), _ptr(state), C.byref(res)))
        return res

    def price_heston_barrier_enqueue(self, opt: Option, sim: Sim, heston: Heston, barrier: Barrier, stats, samples=None,
                                     state=None) -> None:
        """Asynchronous: leaves {sum, sumsq, live_steps, truncated_steps, sum of v+ over the counted lane-steps, n} in
        the device tensor `stats` (>= 6 doubles; finalize_stats)."""
        _check(self._L.mcamd_price_heston_barrier_enqueue(self._h, C.byref(opt), C.byref(sim), C.byref(heston),
                                                          C.byref(barrier), _ptr(samples), _ptr(state), _ptr(stats)))

    def price_heston_smile(self, opt: Option, sim: Sim, heston: Heston, expiry_steps, strikes, state=None):
        """len(expiry_steps) x len(strikes) vanillas on one set of price_heston's paths (mcamd_price_heston_smile);
        heston.payoff holds for every node, opt.K, opt.v and opt.B are ignored.  state: optional device tensor of
        2 x n_expiries x n_paths_local values of the path precision that receives every path's spot at every expiry,
        expiry-major, then its raw variance there, expiry-major.  Returns (price, std_err, stats, res) as
        price_localvol_smile does: each node discounted to its own expiry, stats the 2 n_e n_K sums."""
        smile = make_smile(len(expiry_steps), len(strikes), heston.payoff, heston.q)
        steps, ks = _smile_arrays(smile, expiry_steps, strikes)
        return _smile_sync(opt, sim, smile, expiry_steps, lambda stats, res: self._L.mcamd_price_heston_smile(
            self._h, C.byref(opt), C.byref(sim), C.byref(heston), smile.n_expiries, smile.n_strikes, steps, ks, _ptr(state),
            stats, res))

    def price_heston_smile_enqueue(self, opt: Option, sim: Sim, heston: Heston, expiry_steps, strikes, stats,
                                   state=None) -> None:
        """Asynchronous: leaves the 2 n_e n_K sums and then n in the device tensor `stats` (>= 2 n_e n_K + 1 doubles;
        finalize_smile serves the sums)."""
        smile = make_smile(len(expiry_steps), len(strikes), heston.payoff, heston.q)
        steps, ks = _smile_arrays(smile, expiry_steps, strikes)
        _check(self._L.mcamd_price_heston_smile_enqueue(self._h, C.byref(opt), C.byref(sim), C.byref(heston),
                                                        smile.n_expiries, smile.n_strikes, steps, ks, _ptr(state),
                                                        _ptr(stats)))

    def price_localvol_greeks(self, opt: Option, sim: Sim, job: LocalVolGreeksJob, surface: "LocalVolSurface",
                              samples=None) -> LocalVolGreeks:
        """Price, delta, gamma, vega, bucketed vega, rho and dividend rho of a European option under a local-volatility
        surface from one walk of the paths (mcamd_price_localvol_greeks); opt.v is ignored.  samples: optional device
        tensor of (6 + n_vega_buckets) x n_paths_local doubles, estimator-major, that receives every path's
        undiscounted samples."""
        out = LocalVolGreeks()
        _check(self._L.mcamd_price_localvol_greeks(self._h, C.byref(opt), C.byref(sim), C.byref(job), surface._h,
                                                   _ptr(samples), C.byref(out)))
        return out

    def price_localvol_greeks_enqueue(self, opt: Option, sim: Sim, job: LocalVolGreeksJob, surface: "LocalVolSurface",
                                      stats, samples=None) -> None:
        """Asynchronous: leaves the 32-double record in the device tensor `stats` (finalize_localvol_greeks_stats)."""
        _check(self._L.mcamd_price_localvol_greeks_enqueue(self._h, C.byref(opt), C.byref(sim), C.byref(job), surface._h,
                                                           _ptr(samples), _ptr(stats)))

    def price_localvol_smile(self, opt: Option, sim: Sim, smile: Smile, expiry_steps, strikes,
                             surface: "LocalVolSurface", spots=None):
        """n_expiries x n_strikes vanillas on one set of local-volatility paths (mcamd_price_localvol_smile); opt.v and
        opt.K are ignored.  spots: optional device tensor of n_expiries x n_paths_local values of the path precision
        that receives every path's spot at every expiry, expiry-major.  Returns (price, std_err, stats, res): price
        and std_err as (n_expiries, n_strikes) numpy arrays, each node discounted to its own expiry; stats the
        2 n_e n_K sums (all sums, then all sums of squares) as a numpy array; res as the header describes it."""
        steps, ks = _smile_arrays(smile, expiry_steps, strikes)
        return _smile_sync(opt, sim, smile, expiry_steps, lambda stats, res: self._L.mcamd_price_localvol_smile(
            self._h, C.byref(opt), C.byref(sim), C.byref(smile), steps, ks, surface._h, _ptr(spots), stats, res))

    def price_localvol_smile_enqueue(self, opt: Option, sim: Sim, smile: Smile, expiry_steps, strikes,
                                     surface: "LocalVolSurface", stats, spots=None) -> None:
        """Asynchronous: leaves the 2 n_e n_K sums and then n in the device tensor `stats` (>= 2 n_e n_K + 1 doubles;
        finalize_smile serves the sums)."""
        steps, ks = _smile_arrays(smile, expiry_steps, strikes)
        _check(self._L.mcamd_price_localvol_smile_enqueue(self._h, C.byref(opt), C.byref(sim), C.byref(smile), steps, ks,
                                                          surface._h, _ptr(spots), _ptr(stats)))

    def price_lookback(self, opt: Option, sim: Sim, lookback: Lookback, samples=None) -> Result:
        """Lookback option (mcamd_price_lookback).  samples: optional device tensor of n_paths_local values of the path
        precision that receives each path's undiscounted sample."""
        res = Result()
        _check(self._L.mcamd_price_lookback(self._h, C.byref(opt), C.byref(sim), C.byref(lookback), _ptr(samples),
                                            C.byref(res)))
        return res

    def price_lookback_enqueue(self, opt: Option, sim: Sim, lookback: Lookback, stats, samples=None) -> None:
        """Asynchronous: leaves {sum, sumsq, 0, 0, 0, n} in the device tensor `stats` (>= 6 doubles; finalize_stats)."""
        _check(self._L.mcamd_price_lookback_enqueue(self._h, C.byref(opt), C.byref(sim), C.byref(lookback),
                                                    _ptr(samples), _ptr(stats)))

    def price_asian(self, opt: Option, sim: Sim, asian: Asian, samples=None) -> Result:
        """Asian option (mcamd_price_asian).  samples: optional device tensor of n_paths_local values of the path
        precision; receives the undiscounted sample of every path (never the control-adjusted value)."""
        res = Result()
        _check(self._L.mcamd_price_asian(self._h, C.byref(opt), C.byref(sim), C.byref(asian), _ptr(samples),
                                         C.byref(res)))
        return res

    def price_asian_enqueue(self, opt: Option, sim: Sim, asian: Asian, stats, samples=None) -> None:
        """Asynchronous: leaves {sum y, sum y^2, sum c, sum c^2, sum y c, n} in the device tensor `stats` (>= 6 doubles;
        finalize_stats, with control_variate=True for a controlled job)."""
        _check(self._L.mcamd_price_asian_enqueue(self._h, C.byref(opt), C.byref(sim), C.byref(asian), _ptr(samples),
                                                 _ptr(stats)))

    def price_autocall(self, opt: Option, sim: Sim, autocall: Autocall, samples=None) -> AutocallResult:
        """Worst-of autocallable note (mcamd_price_autocall): r and T come from opt.  samples: optional device tensor of
        n_paths_local values of the path precision that receives every path's sample, in maturity money."""
        res = AutocallResult()
        _check(self._L.mcamd_price_autocall(self._h, C.byref(opt), C.byref(sim), C.byref(autocall), _ptr(samples),
                                            C.byref(res)))
        return res

    def price_autocall_enqueue(self, opt: Option, sim: Sim, autocall: Autocall, stats, samples=None) -> None:
        """Asynchronous: leaves {sum, sumsq, n_called, sum_t_call, n_knocked_in, n} in the device tensor `stats`
        (>= 6 doubles; finalize_stats without the control variate)."""
        _check(self._L.mcamd_price_autocall_enqueue(self._h, C.byref(opt), C.byref(sim), C.byref(autocall),
                                                    _ptr(samples), _ptr(stats)))

    def price_autocall_localvol(self, opt: Option, sim: Sim, autocall: AutocallLocalVol, surfaces,
                                samples=None) -> AutocallResult:
        """Worst-of autocallable note under per-asset local-volatility surfaces (mcamd_price_autocall_localvol): r and T
        come from opt; surfaces: one LocalVolSurface per asset (the same one may appear several times).  samples:
        optional device tensor of n_paths_local values of the path precision that receives every path's sample."""
        res = AutocallResult()
        _check(self._L.mcamd_price_autocall_localvol(self._h, C.byref(opt), C.byref(sim), C.byref(autocall),
                                                     surface_array(surfaces), _ptr(samples), C.byref(res)))
        return res

    def price_autocall_localvol_enqueue(self, opt: Option, sim: Sim, autocall: AutocallLocalVol, surfaces, stats,
                                        samples=None) -> None:
        """Asynchronous: leaves {sum, sumsq, n_called, sum_t_call, n_knocked_in, n} in the device tensor `stats`
        (>= 6 doubles; finalize_stats without the control variate).  The surfaces must outlive the enqueued work."""
        _check(self._L.mcamd_price_autocall_localvol_enqueue(self._h, C.byref(opt), C.byref(sim), C.byref(autocall),
                                                             surface_array(surfaces), _ptr(samples), _ptr(stats)))

    def price_basket(self, opt: Option, sim: Sim, basket: Basket, samples=None) -> Result:
        """Basket, spread or rainbow option on correlated assets (mcamd_price_basket): r, T, K and the barrier level B
        come from opt.  samples: optional device tensor of n_paths_local values of the path precision that receives
        each path's undiscounted sample."""
        res = Result()
        _check(self._L.mcamd_price_basket(self._h, C.byref(opt), C.byref(sim), C.byref(basket), _ptr(samples),
                                          C.byref(res)))
        return res

    def price_basket_enqueue(self, opt: Option, sim: Sim, basket: Basket, stats, samples=None) -> None:
        """Asynchronous: leaves {sum, sumsq, 0, 0, 0, n} in the device tensor `stats` (>= 6 doubles; finalize_stats)."""
        _check(self._L.mcamd_price_basket_enqueue(self._h, C.byref(opt), C.byref(sim), C.byref(basket),
                                                  _ptr(samples), _ptr(stats)))

    def price_american(self, opt: Option, sim: Sim, am: American, work, coeffs: bool = False):
        """Least-squares Monte Carlo price of an American / Bermudan put or call (mcamd_price_american).  work: a device
        tensor of at least american_workspace_bytes(am, sim) bytes.  Returns the AmericanResult, and with coeffs=True
        also the (M, n_basis + 1) array of per-date coefficients and regressed flags."""
        res = AmericanResult()
        nb = am.n_basis or 3
        M = sim.n_steps // am.exercise_every if am.exercise_every else 0
        arr = (C.c_double * (M * (nb + 1)))() if coeffs and M > 0 else None
        nbytes = work.numel() * work.element_size() if work is not None else 0
        _check(self._L.mcamd_price_american(self._h, C.byref(opt), C.byref(sim), C.byref(am), _ptr(work), nbytes, arr,
                                            C.byref(res)))
        if not coeffs:
            return res
        import numpy as np
        return res, np.ctypeslib.as_array(arr).reshape(M, nb + 1).copy()

    def american_upper_bound(self, opt: Option, sim: Sim, am: American, dual: AmericanDual, coeffs, work,
                             cont=None) -> AmericanDualResult:
        """Andersen-Broadie dual (upper) bound of the exercise rule `coeffs` (mcamd_american_upper_bound): the
        (M, n_basis + 1) array price_american returns, or one of the caller's own.  work: a device tensor of at least
        american_dual_workspace_bytes(am, sim, dual) bytes; cont: optional device tensor of M * n_paths_local doubles
        that receives the continuation values Q[j, p]."""
        import numpy as np
        res = AmericanDualResult()
        table = None
        if coeffs is not None:
            table = np.ascontiguousarray(coeffs, dtype=np.float64)
            nb = am.n_basis or 3
            M = sim.n_steps // am.exercise_every if am.exercise_every else 0
            if table.size != M * (nb + 1):
                raise ValueError(f"coeffs holds {table.size} doubles; {M} dates x ({nb} + 1) expected")
        nbytes = work.numel() * work.element_size() if work is not None else 0
        _check(self._L.mcamd_american_upper_bound(
            self._h, C.byref(opt), C.byref(sim), C.byref(am), C.byref(dual),
            None if table is None else table.ctypes.data_as(C.POINTER(C.c_double)), _ptr(work), nbytes, _ptr(cont),
            C.byref(res)))
        return res

    def enqueued_kernel_ms(self, n_last: int):
        arr = (C.c_float * n_last)()
        _check(self._L.mcamd_enqueued_kernel_ms(self._h, n_last, arr))
        return list(arr)

    def simulate_trajectories(self, opt: Option, sim: Sim, traj, counts=None, payoffs=None,
                              layout=STEP_MAJOR) -> Result:
        res = Result()
        _check(self._L.mcamd_simulate_trajectories(self._h, C.byref(opt), C.byref(sim), layout, _ptr(traj),
                                                   _ptr(counts), _ptr(payoffs), C.byref(res)))
        return res

    def simulate_trajectories_enqueue(self, opt: Option, sim: Sim, traj, counts, payoffs, stats, layout=STEP_MAJOR) -> None:
        _check(self._L.mcamd_simulate_trajectories_enqueue(self._h, C.byref(opt), C.byref(sim), layout, _ptr(traj),
                                                           _ptr(counts), _ptr(payoffs), _ptr(stats)))

    def nmc_inner_enqueue(self, opt: Option, sim: Sim, prices, counts, point_prices, stats, layout=STEP_MAJOR,
                          variant=NMC_WAVE_PER_POINT) -> None:
        _check(self._L.mcamd_nmc_inner_enqueue(self._h, C.byref(opt), C.byref(sim), layout, variant, _ptr(prices),
                                               _ptr(counts), _ptr(point_prices), _ptr(stats)))

    def nmc_fused_enqueue(self, opt: Option, sim: Sim, outer_seed: int, prices, counts, point_prices, stats,
                          layout=STEP_MAJOR) -> None:
        _check(self._L.mcamd_nmc_fused_enqueue(self._h, C.byref(opt), C.byref(sim), outer_seed, layout, _ptr(prices),
                                               _ptr(counts), _ptr(point_prices), _ptr(stats)))

    def diag_store_pattern(self, n_paths_local: int, n_steps: int, precision: int, traj, payoffs=None) -> float:
        """kernel ms of the store kernel's pure store stream (diagnostic: the same-run HBM write ceiling)"""
        ms = C.c_float(0)
        _check(self._L.mcamd_diag_store_pattern(self._h, n_paths_local, n_steps, precision, _ptr(traj), _ptr(payoffs),
                                                C.byref(ms)))
        return ms.value

    def price_from_normals(self, opt: Option, sim: Sim, normals, payoffs=None) -> Result:
        res = Result()
        _check(self._L.mcamd_price_from_normals(self._h, C.byref(opt), C.byref(sim), _ptr(normals), _ptr(payoffs),
                                                C.byref(res)))
        return res

    def generate_normals(self, seed: int, n: int, precision: int, out) -> float:
        ms = C.c_float(0)
        _check(self._L.mcamd_generate_normals(self._h, seed, n, precision, _ptr(out), C.byref(ms)))
        return ms.value

    def reduce_sum(self, x, n: int, precision: int, variant: int = REDUCE_GRID_STRIDE):
        s, ms = C.c_double(0), C.c_float(0)
        _check(self._L.mcamd_reduce_sum(self._h, _ptr(x), n, precision, variant, C.byref(s), C.byref(ms)))
        return s.value, ms.value

    def reduce_partials(self, x, n: int, precision: int, variant: int, n_blocks: int):
        """one partial sum per workgroup (they add up to the complete sum) and the kernel's ms"""
        arr, ms = (C.c_double * n_blocks)(), C.c_float(0)
        _check(self._L.mcamd_reduce_partials(self._h, _ptr(x), n, precision, variant, n_blocks, arr, C.byref(ms)))
        return list(arr), ms.value

    def nmc_inner(self, opt: Option, sim: Sim, prices, counts, point_prices, layout=STEP_MAJOR,
                  variant=NMC_WAVE_PER_POINT) -> Result:
        res = Result()
        _check(self._L.mcamd_nmc_inner(self._h, C.byref(opt), C.byref(sim), layout, variant, _ptr(prices),
                                       _ptr(counts), _ptr(point_prices), C.byref(res)))
        return res

    def nmc_fused(self, opt: Option, sim: Sim, outer_seed: int, prices, counts, point_prices,
                  layout=STEP_MAJOR) -> Result:
        res = Result()
        _check(self._L.mcamd_nmc_fused(self._h, C.byref(opt), C.byref(sim), outer_seed, layout, _ptr(prices),
                                       _ptr(counts), _ptr(point_prices), C.byref(res)))
        return res


class LocalVolSurface:
    """Owns one mcamd_localvol_surface: the pair tables of a local-volatility surface in the memory of one context's
    device.  Immutable; several may be alive in one context."""

    def __init__(self, ctx: Context, grid_args, sigma):
        self._L = load()
        self._h = C.c_void_p()
        self.grid = grid_args if isinstance(grid_args, LocalVolGrid) else make_localvol_grid(*grid_args)
        _check(self._L.mcamd_localvol_surface_create(ctx._h, C.byref(self.grid), _sigma_array(self.grid, sigma),
                                                     C.byref(self._h)))

    def close(self):
        if self._h:
            self._L.mcamd_localvol_surface_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class Group:
    """Single-process multi-GPU group: one context per device + an RCCL communicator clique (mcamd_group_*)."""

    def __init__(self, n_devices: int = 0, devices=None):
        self._L = load()
        self._h = C.c_void_p()
        arr = (C.c_int * len(devices))(*devices) if devices else None
        _check(self._L.mcamd_group_create(len(devices) if devices else n_devices, arr, C.byref(self._h)))

    def close(self):
        if self._h:
            self._L.mcamd_group_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def size(self) -> int:
        n = C.c_int(0)
        _check(self._L.mcamd_group_size(self._h, C.byref(n)))
        return n.value

    def price_paths(self, opt: Option, sim: Sim) -> Result:
        res = Result()
        _check(self._L.mcamd_group_price_paths(self._h, C.byref(opt), C.byref(sim), C.byref(res)))
        return res

    def price_greeks(self, opt: Option, sim: Sim, method: int = GREEKS_AUTO) -> Greeks:
        out = Greeks()
        _check(self._L.mcamd_group_price_greeks(self._h, C.byref(opt), C.byref(sim), method, C.byref(out)))
        return out

    def shard(self, sim: Sim, i: int):
        """(first global path id, number of paths) device i of the group works on for this job."""
        lo, n = C.c_uint64(0), C.c_uint64(0)
        _check(self._L.mcamd_group_shard(self._h, C.byref(sim), i, C.byref(lo), C.byref(n)))
        return lo.value, n.value

    @staticmethod
    def _ptrs(per_device):
        """array of one device pointer per device (None: no such output)"""
        if per_device is None:
            return None
        return (C.c_void_p * len(per_device))(*[None if t is None else t.data_ptr() for t in per_device])

    def simulate_trajectories(self, opt: Option, sim: Sim, traj, counts=None, payoffs=None, layout=STEP_MAJOR) -> Result:
        res = Result()
        _check(self._L.mcamd_group_simulate_trajectories(self._h, C.byref(opt), C.byref(sim), layout, self._ptrs(traj),
                                                         self._ptrs(counts), self._ptrs(payoffs), C.byref(res)))
        return res

    def nmc_inner(self, opt: Option, sim: Sim, prices, counts, point_prices, layout=STEP_MAJOR,
                  variant=NMC_WAVE_PER_POINT) -> Result:
        res = Result()
        _check(self._L.mcamd_group_nmc_inner(self._h, C.byref(opt), C.byref(sim), layout, variant, self._ptrs(prices),
                                             self._ptrs(counts), self._ptrs(point_prices), C.byref(res)))
        return res

    def nmc_fused(self, opt: Option, sim: Sim, outer_seed: int, prices, counts, point_prices, layout=STEP_MAJOR) -> Result:
        res = Result()
        _check(self._L.mcamd_group_nmc_fused(self._h, C.byref(opt), C.byref(sim), outer_seed, layout, self._ptrs(prices),
                                             self._ptrs(counts), self._ptrs(point_prices), C.byref(res)))
        return res
