"""ctypes binding of the C ABI in include/mcamd.h (libmcamd.so).

Host-side plumbing only: device buffers and streams come from the caller (torch tensors'
data_ptr / torch.cuda.current_stream in the tests and bench).  Nothing here computes a price:
every call goes to the HIP library, and loading fails loudly if the library is missing.

The header is restated here once: the struct classes and the PROTOTYPES table.  tests/test_capi_header_cpu.py parses
include/mcamd.h and compares both with it, field by field and parameter by parameter.
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


class _Record(C.Structure):
    """a result struct of scalars: as_dict is its fields by name"""

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class Option(C.Structure):
    _fields_ = [("S0", C.c_double), ("T", C.c_double), ("K", C.c_double), ("r", C.c_double), ("v", C.c_double),
                ("B", C.c_double), ("P1", C.c_int32), ("P2", C.c_int32), ("use_window", C.c_int32),
                ("Ik", C.c_int32), ("Sk", C.c_double), ("Tk", C.c_int32), ("reserved", C.c_int32), ("dt", C.c_double)]


class Sim(C.Structure):
    _fields_ = [("n_paths", C.c_uint64), ("path_offset", C.c_uint64), ("n_paths_local", C.c_uint64),
                ("n_steps", C.c_uint32), ("n_paths_inner", C.c_uint32), ("seed", C.c_uint64),
                ("precision", C.c_int32), ("flags", C.c_int32)]


class Result(_Record):
    _fields_ = [("sum", C.c_double), ("sumsq", C.c_double), ("n", C.c_uint64), ("price", C.c_double),
                ("std_err", C.c_double), ("ci_lo", C.c_double), ("ci_hi", C.c_double), ("kernel_ms", C.c_float),
                ("total_ms", C.c_float), ("grid", C.c_uint32), ("block", C.c_uint32), ("sum_c", C.c_double),
                ("sum_cc", C.c_double), ("sum_yc", C.c_double), ("cv_beta", C.c_double), ("cv_rho", C.c_double),
                ("work_steps", C.c_double), ("live_steps", C.c_double)]


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


class AmericanResult(_Record):
    """mcamd_american_result: out-of-sample and in-sample estimates, raw shard sums, dates, timings."""
    _fields_ = [("price", C.c_double), ("std_err", C.c_double), ("ci_lo", C.c_double), ("ci_hi", C.c_double),
                ("sum", C.c_double), ("sumsq", C.c_double), ("n", C.c_uint64), ("in_sample_price", C.c_double),
                ("in_sample_std_err", C.c_double), ("in_sample_sum", C.c_double), ("in_sample_sumsq", C.c_double),
                ("n_train", C.c_uint64), ("n_early", C.c_uint64), ("sum_t_exercise", C.c_double),
                ("n_dates", C.c_uint32), ("n_regressed", C.c_uint32), ("immediate_exercise", C.c_int32),
                ("train_ms", C.c_float), ("price_ms", C.c_float), ("total_ms", C.c_float), ("grid", C.c_uint32),
                ("block", C.c_uint32), ("train_grid", C.c_uint32), ("reserved", C.c_int32)]


class AmericanDual(C.Structure):
    """mcamd_american_dual: the nested sample of mcamd_american_upper_bound."""
    _fields_ = [("n_inner", C.c_uint32), ("reserved", C.c_uint32), ("inner_seed", C.c_uint64)]


class AmericanDualResult(_Record):
    """mcamd_american_dual_result: the dual (upper) estimate, raw shard sums, lane-step counts, timings."""
    _fields_ = [("upper", C.c_double), ("std_err", C.c_double), ("ci_hi", C.c_double), ("sum", C.c_double),
                ("sumsq", C.c_double), ("n", C.c_uint64), ("sum_q0", C.c_double), ("work_steps", C.c_double),
                ("live_steps", C.c_double), ("n_dates", C.c_uint32), ("immediate_exercise", C.c_int32),
                ("outer_ms", C.c_float), ("inner_ms", C.c_float), ("scan_ms", C.c_float), ("total_ms", C.c_float),
                ("grid", C.c_uint32), ("block", C.c_uint32)]


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


class AutocallResult(_Record):
    """mcamd_autocall_result"""
    _fields_ = [("price", C.c_double), ("std_err", C.c_double), ("ci_lo", C.c_double), ("ci_hi", C.c_double),
                ("sum", C.c_double), ("sumsq", C.c_double), ("n", C.c_uint64), ("n_called", C.c_uint64),
                ("sum_t_call", C.c_double), ("n_knocked_in", C.c_uint64), ("work_steps", C.c_double),
                ("live_steps", C.c_double), ("kernel_ms", C.c_float), ("total_ms", C.c_float), ("grid", C.c_uint32),
                ("block", C.c_uint32)]


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


class CliquetResult(_Record):
    """mcamd_cliquet_result"""
    _fields_ = [("price", C.c_double), ("std_err", C.c_double), ("ci_lo", C.c_double), ("ci_hi", C.c_double),
                ("sum", C.c_double), ("sumsq", C.c_double), ("n", C.c_uint64), ("n_floored", C.c_uint64),
                ("n_capped", C.c_uint64), ("work_steps", C.c_double), ("kernel_ms", C.c_float), ("total_ms", C.c_float),
                ("grid", C.c_uint32), ("block", C.c_uint32)]


class Heston(C.Structure):
    """mcamd_heston: the payoff, the scheme (HESTON_FULL_TRUNCATION), the dividend yield and the model's parameters
    mcamd_price_heston prices a European option with."""
    _fields_ = [("payoff", C.c_int32), ("scheme", C.c_int32), ("q", C.c_double), ("v0", C.c_double),
                ("kappa", C.c_double), ("theta", C.c_double), ("xi", C.c_double), ("rho", C.c_double),
                ("reserved", C.c_double)]


class HestonResult(_Record):
    """mcamd_heston_result"""
    _fields_ = [("price", C.c_double), ("std_err", C.c_double), ("ci_lo", C.c_double), ("ci_hi", C.c_double),
                ("sum", C.c_double), ("sumsq", C.c_double), ("n", C.c_uint64), ("truncated_steps", C.c_double),
                ("mean_variance", C.c_double), ("work_steps", C.c_double), ("kernel_ms", C.c_float),
                ("total_ms", C.c_float), ("grid", C.c_uint32), ("block", C.c_uint32)]


class HestonCliquetResult(_Record):
    """mcamd_heston_cliquet_result: mcamd_cliquet_result's fields, then mcamd_heston_result's two diagnostics"""
    _fields_ = CliquetResult._fields_ + [("truncated_steps", C.c_double), ("mean_variance", C.c_double)]


class HestonBarrierResult(_Record):
    """mcamd_heston_barrier_result"""
    _fields_ = [("price", C.c_double), ("std_err", C.c_double), ("ci_lo", C.c_double), ("ci_hi", C.c_double),
                ("sum", C.c_double), ("sumsq", C.c_double), ("n", C.c_uint64), ("live_steps", C.c_double),
                ("work_steps", C.c_double), ("truncated_steps", C.c_double), ("mean_variance", C.c_double),
                ("kernel_ms", C.c_float), ("total_ms", C.c_float), ("grid", C.c_uint32), ("block", C.c_uint32)]


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


def _prototypes():
    """{name: (restype, argtypes)} of every function include/mcamd.h declares.  Device pointers and opaque handles are
    c_void_p (a torch data_ptr goes in as it is), host arrays and out-parameters POINTER(...)."""
    P, vp, u32, u64, i32, f32, f64 = C.POINTER, C.c_void_p, C.c_uint32, C.c_uint64, C.c_int, C.c_float, C.c_double
    pvp, pu32, pf32, pf64, res = P(vp), P(u32), P(f32), P(f64), P(Result)
    job = (vp, P(Option), P(Sim))   # the head of a pricing call: the context (or group), the option, the simulation
    table = {}

    def fn(name, *argtypes, restype=i32):
        table[name] = (restype, list(argtypes))

    def pair(name, *terms, result=Result):
        """a synchronous call that fills a result and its _enqueue form, which leaves device statistics instead"""
        fn(name, *job, *terms, P(result))
        fn(name + "_enqueue", *job, *terms, vp)

    fn("mcamd_abi_version")
    fn("mcamd_last_error", restype=C.c_char_p)
    fn("mcamd_build_id", restype=C.c_char_p)
    fn("mcamd_device_count", P(i32))
    fn("mcamd_ctx_create", i32, vp, pvp)
    fn("mcamd_ctx_destroy", vp)
    fn("mcamd_get_device_info", vp, P(DeviceInfo))
    fn("mcamd_device_malloc", vp, u64, pvp)
    fn("mcamd_device_free", vp, vp)
    fn("mcamd_memcpy_to_host", vp, vp, vp, u64)
    fn("mcamd_memcpy_to_device", vp, vp, vp, u64)
    fn("mcamd_enqueued_kernel_ms", vp, u32, pf32)
    fn("mcamd_diag_store_pattern", vp, u64, u32, i32, vp, vp, pf32)
    fn("mcamd_generate_normals", vp, u64, u64, i32, vp, pf32)
    fn("mcamd_reduce_sum", vp, vp, u64, i32, i32, pf64, pf32)
    fn("mcamd_reduce_partials", vp, vp, u64, i32, i32, u32, pf64, pf32)
    fn("mcamd_cpu_mc_f32", P(Option), u64, u32, u64, i32, pf32, pf32)

    # the paths of constant volatility: (ctx, opt, sim, the job's terms and device buffers, result or statistics)
    pair("mcamd_price_paths")
    pair("mcamd_simulate_trajectories", i32, vp, vp, vp)
    pair("mcamd_nmc_inner", i32, i32, vp, vp, vp)
    pair("mcamd_nmc_fused", u64, i32, vp, vp, vp)
    fn("mcamd_price_from_normals", *job, vp, vp, res)
    pair("mcamd_price_greeks", i32, result=Greeks)
    pair("mcamd_price_barrier", P(Barrier), vp)
    pair("mcamd_price_lookback", P(Lookback), vp)
    pair("mcamd_price_basket", P(Basket), vp)
    pair("mcamd_price_asian", P(Asian), vp)
    pair("mcamd_price_autocall", P(Autocall), vp, result=AutocallResult)
    fn("mcamd_american_workspace_bytes", P(American), P(Sim), P(u64))
    fn("mcamd_price_american", *job, P(American), vp, u64, pf64, P(AmericanResult))
    fn("mcamd_american_dual_workspace_bytes", P(American), P(Sim), P(AmericanDual), P(u64))
    fn("mcamd_american_upper_bound", *job, P(American), P(AmericanDual), pf64, vp, u64, vp, P(AmericanDualResult))

    # under a local-volatility surface
    fn("mcamd_localvol_surface_create", vp, P(LocalVolGrid), pf64, pvp)
    fn("mcamd_localvol_surface_destroy", vp)
    pair("mcamd_price_localvol", P(LocalVol), vp, vp)
    pair("mcamd_price_autocall_localvol", P(AutocallLocalVol), pvp, vp, result=AutocallResult)
    pair("mcamd_price_localvol_greeks", P(LocalVolGreeksJob), vp, vp, result=LocalVolGreeks)
    pair("mcamd_price_cliquet", P(Cliquet), vp, vp, result=CliquetResult)
    fn("mcamd_price_localvol_smile", *job, P(Smile), pu32, pf64, vp, vp, pf64, res)
    fn("mcamd_price_localvol_smile_enqueue", *job, P(Smile), pu32, pf64, vp, vp, vp)

    # under Heston
    pair("mcamd_price_heston", P(Heston), vp, vp, result=HestonResult)
    pair("mcamd_price_heston_cliquet", P(Heston), P(Cliquet), vp, result=HestonCliquetResult)
    pair("mcamd_price_heston_barrier", P(Heston), P(Barrier), vp, vp, result=HestonBarrierResult)
    fn("mcamd_price_heston_smile", *job, P(Heston), u32, u32, pu32, pf64, vp, pf64, res)
    fn("mcamd_price_heston_smile_enqueue", *job, P(Heston), u32, u32, pu32, pf64, vp, vp)

    # a group: the first argument is the group, the device buffers are host arrays of one pointer per device
    fn("mcamd_group_create", i32, P(i32), pvp)
    fn("mcamd_group_destroy", vp)
    fn("mcamd_group_size", vp, P(i32))
    fn("mcamd_group_ctx", vp, i32, pvp)
    fn("mcamd_group_shard", vp, P(Sim), i32, P(u64), P(u64))
    fn("mcamd_group_price_paths", *job, res)
    fn("mcamd_group_price_greeks", *job, i32, P(Greeks))
    fn("mcamd_group_simulate_trajectories", *job, i32, pvp, pvp, pvp, res)
    fn("mcamd_group_nmc_inner", *job, i32, i32, pvp, pvp, pvp, res)
    fn("mcamd_group_nmc_fused", *job, u64, i32, pvp, pvp, pvp, res)

    # host: statistics records into results
    fn("mcamd_finalize", f64, f64, u64, f64, f64, res)
    fn("mcamd_finalize_cv", pf64, u64, f64, f64, res)
    fn("mcamd_finalize_stats", pf64, f64, f64, i32, res)
    fn("mcamd_finalize_nmc_stats", pf64, res)
    fn("mcamd_finalize_greeks_stats", pf64, f64, f64, i32, P(Greeks))
    fn("mcamd_finalize_localvol_greeks_stats", pf64, f64, f64, u32, i32, P(LocalVolGreeks))
    fn("mcamd_finalize_smile", pf64, u64, P(Option), u32, P(Smile), pu32, pf64, pf64)

    # host: closed forms
    fn("mcamd_cnd_f32", f32, restype=f32)
    fn("mcamd_bs_call_f32", *[f32] * 5, restype=f32)
    fn("mcamd_bs_call_f64", *[f64] * 5, restype=f64)
    fn("mcamd_bs_greeks_f64", f64, f64, f64, f64, f64, pf64)
    fn("mcamd_bs_price_f64", f64, f64, f64, f64, f64, f64, i32, pf64)
    fn("mcamd_bs_implied_vol_f64", f64, f64, f64, f64, f64, i32, f64, pf64)
    fn("mcamd_barrier_price_f64", f64, f64, f64, f64, f64, f64, i32, i32, pf64)
    fn("mcamd_lookback_price_f64", f64, f64, f64, f64, f64, i32, i32, pf64)
    fn("mcamd_basket_geometric_price_f64", P(Basket), f64, f64, f64, pf64)
    fn("mcamd_exchange_price_f64", f64, f64, f64, f64, f64, f64, pf64)
    fn("mcamd_asian_geometric_price_f64", f64, f64, f64, f64, f64, u32, i32, i32, i32, pf64)
    fn("mcamd_autocall_single_date_price_f64", f64, f64, f64, f64, f64, f64, i32, pf64)
    fn("mcamd_localvol_sigma_f64", P(LocalVolGrid), pf64, u32, u32, f64, pf64)
    fn("mcamd_cliquet_price_f64", i32, f64, f64, f64, u32, u32, pf64, f64, f64, pf64)
    fn("mcamd_heston_price_f64", *[f64] * 10, i32, pf64)
    fn("mcamd_heston_cliquet_price_f64", i32, *[f64] * 8, u32, u32, f64, f64, pf64)
    return table


PROTOTYPES = _prototypes()
EXPORTS = list(PROTOTYPES)   # every symbol include/mcamd.h declares


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
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


def _check(rc: int):
    if rc != OK:
        raise McamdError(rc, load().mcamd_last_error().decode())


def _filled(fn, result, *args):
    """what the C function fn leaves in its last parameter: fn(*args, &out) on a fresh out = result(), checked.  A
    struct or scalar passed where the prototype says POINTER(its type) goes by reference, and None goes as NULL:
    ctypes does both from argtypes."""
    out = result()
    _check(getattr(load(), fn)(*args, out))
    return out


def _out_double(fn, *args) -> float:
    """the value a closed form leaves in its last parameter, a double *"""
    return _filled(fn, C.c_double, *args).value


def _doubles(values, n):
    """values as a C array of n doubles (fewer are padded with zeros; more are an IndexError)"""
    return (C.c_double * n)(*[float(x) for x in values])


def _fill_corr(table, corr, d):
    """the d x d correlations into a struct's table, whose rows are 8 apart"""
    for j in range(d):
        for k in range(d):
            table[8 * j + k] = float(corr[j][k])


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
    return _out_double("mcamd_barrier_price_f64", S0, K, B, T, r, sigma, kind, payoff)


def make_lookback(strike=LOOKBACK_FLOATING, payoff=PAYOFF_CALL, monitoring=MONITOR_CONTINUOUS) -> Lookback:
    return Lookback(strike, payoff, monitoring, 0)


def lookback_price_f64(S0, K, T, r, sigma, strike=LOOKBACK_FLOATING, payoff=PAYOFF_CALL) -> float:
    """closed form of the continuously monitored, newly issued lookback (Goldman-Sosin-Gatto, Conze-Viswanathan)"""
    return _out_double("mcamd_lookback_price_f64", S0, K, T, r, sigma, strike, payoff)


def make_basket(S0, v, w, corr, kind=BASKET_ARITHMETIC, payoff=PAYOFF_CALL, barrier=BASKET_NO_BARRIER) -> Basket:
    """S0, v, w: d values each (d = len(S0), at most BASKET_MAX_ASSETS); corr: d x d (nested sequences or an array)."""
    d = len(S0)
    if not 1 <= d <= BASKET_MAX_ASSETS or len(v) != d or len(w) != d or len(corr) != d or any(len(row) != d for row in corr):
        raise ValueError(f"a basket takes 1..{BASKET_MAX_ASSETS} assets and S0, v, w of d and corr of d x d values")
    b = Basket(d, kind, payoff, barrier)
    for j in range(d):
        b.S0[j], b.v[j], b.w[j] = float(S0[j]), float(v[j]), float(w[j])
    _fill_corr(b.corr, corr, d)
    return b


def basket_geometric_price_f64(basket: Basket, K, T, r) -> float:
    """closed form of the geometric basket (a lognormal); basket.payoff selects call or put"""
    return _out_double("mcamd_basket_geometric_price_f64", basket, K, T, r)


def exchange_price_f64(a_S1, b_S2, T, v1, v2, rho) -> float:
    """Margrabe's closed form of (a S1 - b S2)+, with a_S1 = a S1(0) and b_S2 = b S2(0)"""
    return _out_double("mcamd_exchange_price_f64", a_S1, b_S2, T, v1, v2, rho)


def make_asian(average=ASIAN_ARITHMETIC, strike=ASIAN_FIXED, payoff=PAYOFF_CALL, include_spot=0,
               control=ASIAN_CONTROL_NONE) -> Asian:
    return Asian(average, strike, payoff, include_spot, control, 0)


def asian_geometric_price_f64(S0, K, T, r, sigma, n_steps, include_spot=0, strike=ASIAN_FIXED, payoff=PAYOFF_CALL) -> float:
    """closed form of the discrete geometric-average option over the n_steps step ends (and t = 0 with include_spot)"""
    return _out_double("mcamd_asian_geometric_price_f64", S0, K, T, r, sigma, n_steps, include_spot, strike, payoff)


def _autocall_terms(cls, field, per_asset, corr, observe_every, call_level, coupon, ki_level, ki_monitoring,
                    call_step_down, first_call_date):
    """an Autocall or AutocallLocalVol: they differ in the per-asset field, v or q"""
    d = len(per_asset)
    if not 1 <= d <= BASKET_MAX_ASSETS or len(corr) != d or any(len(row) != d for row in corr):
        raise ValueError(f"an autocallable takes 1..{BASKET_MAX_ASSETS} assets, {field} of d and corr of d x d values")
    a = cls(d, ki_monitoring, observe_every, first_call_date)
    a.call_level, a.call_step_down, a.coupon, a.ki_level = call_level, call_step_down, coupon, ki_level
    getattr(a, field)[:d] = [float(x) for x in per_asset]
    _fill_corr(a.corr, corr, d)
    return a


def make_autocall(v, corr, observe_every=1, call_level=1.0, coupon=0.0, ki_level=0.0,
                  ki_monitoring=AUTOCALL_KI_NONE, call_step_down=0.0, first_call_date=1) -> Autocall:
    """v: d volatilities (d at most BASKET_MAX_ASSETS); corr: d x d (nested sequences or an array)."""
    return _autocall_terms(Autocall, "v", v, corr, observe_every, call_level, coupon, ki_level, ki_monitoring,
                           call_step_down, first_call_date)


def make_autocall_localvol(q, corr, observe_every=1, call_level=1.0, coupon=0.0, ki_level=0.0,
                           ki_monitoring=AUTOCALL_KI_NONE, call_step_down=0.0, first_call_date=1) -> AutocallLocalVol:
    """q: d dividend yields (d at most BASKET_MAX_ASSETS); corr: d x d (nested sequences or an array)."""
    return _autocall_terms(AutocallLocalVol, "q", q, corr, observe_every, call_level, coupon, ki_level, ki_monitoring,
                           call_step_down, first_call_date)


def surface_array(surfaces):
    """the host array of surface pointers the autocall calls under local volatility take: None stays NULL, and so does
    an entry that is None"""
    if surfaces is None:
        return None
    return (C.c_void_p * max(len(surfaces), 1))(*[None if s is None else s._h for s in surfaces])


def autocall_single_date_price_f64(T, r, sigma, call_level, coupon, ki_level=0.0, ki_monitoring=AUTOCALL_KI_NONE) -> float:
    """closed form of the autocallable on one asset with one date (no knock-in, or a knock-in at maturity)"""
    return _out_double("mcamd_autocall_single_date_price_f64", T, r, sigma, call_level, coupon, ki_level, ki_monitoring)


def make_localvol(payoff=PAYOFF_CALL, barrier=LOCALVOL_NO_BARRIER, monitoring=MONITOR_DISCRETE, q=0.0) -> LocalVol:
    return LocalVol(payoff, barrier, monitoring, 0, q)


def make_cliquet(kind=CLIQUET_SUM, reset_every=1, first_period=1, local_floor=-math.inf, local_cap=math.inf,
                 global_floor=-math.inf, global_cap=math.inf, q=0.0) -> Cliquet:
    return Cliquet(kind, reset_every, first_period, 0, local_floor, local_cap, global_floor, global_cap, q)


def cliquet_price(kind, T, r, q, period_vol, first_period=1, local_floor=-math.inf, local_cap=math.inf) -> float:
    """Closed form of a cliquet without a global clip where the volatility varies in time only
    (mcamd_cliquet_price_f64); period_vol: the rms volatility of each of the n_periods = len(period_vol) periods."""
    return _out_double("mcamd_cliquet_price_f64", kind, T, r, q, len(period_vol), first_period,
                       _doubles(period_vol, len(period_vol)), local_floor, local_cap)


def make_heston(payoff=PAYOFF_CALL, q=0.0, v0=0.04, kappa=2.0, theta=0.04, xi=0.3, rho=-0.7,
                scheme=HESTON_FULL_TRUNCATION) -> Heston:
    return Heston(payoff, scheme, q, v0, kappa, theta, xi, rho, 0.0)


def heston_price(S0, K, T, r, q, v0, kappa, theta, xi, rho, payoff=PAYOFF_CALL) -> float:
    """Closed form of a European option under Heston (mcamd_heston_price_f64): the model's price, which the
    full-truncation scheme of price_heston approaches at first order in the step."""
    return _out_double("mcamd_heston_price_f64", S0, K, T, r, q, v0, kappa, theta, xi, rho, payoff)


def heston_cliquet_price(kind, T, r, q, v0, kappa, theta, xi, rho, n_periods, first_period=1, local_floor=-math.inf,
                         local_cap=math.inf) -> float:
    """Closed form of an additive cliquet, a one-period compounding one or a discretely sampled variance swap under
    Heston, without a global clip (mcamd_heston_cliquet_price_f64): the model's price, through the forward
    characteristic function of the period returns."""
    return _out_double("mcamd_heston_cliquet_price_f64", kind, T, r, q, v0, kappa, theta, xi, rho, n_periods,
                       first_period, local_floor, local_cap)


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
    return _out_double("mcamd_localvol_sigma_f64", g, _sigma_array(g, sigma), n_steps, step, x)


def bs_price_f64(S0, K, T, r, q, sigma, payoff=PAYOFF_CALL) -> float:
    """Black-Scholes with a continuous dividend yield q"""
    return _out_double("mcamd_bs_price_f64", S0, K, T, r, q, sigma, payoff)


def bs_implied_vol(S0, K, T, r, q, price, payoff=PAYOFF_CALL) -> float:
    """the volatility at which bs_price_f64 gives `price` (mcamd_bs_implied_vol_f64); raises McamdError for a price
    that is not strictly inside the no-arbitrage bounds"""
    return _out_double("mcamd_bs_implied_vol_f64", S0, K, T, r, q, payoff, price)


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
    arr = _doubles(list(stats)[:2 * nodes], 2 * nodes)
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
    return _filled("mcamd_finalize", Result, sum_, sumsq, n, r, T)


def finalize_cv(sums, n, r, T) -> Result:
    return _filled("mcamd_finalize_cv", Result, _doubles(sums, 5), n, r, T)


def finalize_stats(stats6, r, T, control_variate=False) -> Result:
    return _filled("mcamd_finalize_stats", Result, _doubles(stats6, 6), r, T, int(control_variate))


def finalize_nmc_stats(stats6) -> Result:
    return _filled("mcamd_finalize_nmc_stats", Result, _doubles(stats6, 6))


def finalize_greeks_stats(stats16, r, T, theta_defined=True) -> Greeks:
    """Greeks of a (possibly all-reduced) 16-double record left by Context.price_greeks_enqueue."""
    return _filled("mcamd_finalize_greeks_stats", Greeks, _doubles(stats16, GREEKS_STATS), r, T, int(theta_defined))


def finalize_localvol_greeks_stats(stats32, r, T, n_vega_buckets=0, gamma_defined=True) -> LocalVolGreeks:
    """Greeks of a (possibly all-reduced) 32-double record left by Context.price_localvol_greeks_enqueue."""
    return _filled("mcamd_finalize_localvol_greeks_stats", LocalVolGreeks, _doubles(stats32, LOCALVOL_GREEKS_STATS),
                   r, T, n_vega_buckets, int(gamma_defined))


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


class _Handle:
    """Owns one opaque handle of the library (_h, on the loaded library _L); a subclass names the function that
    destroys it and creates the handle in its __init__."""
    _destroy = None

    def __init__(self):
        self._L = load()
        self._h = C.c_void_p()

    def close(self):
        if self._h:
            getattr(self._L, self._destroy)(self._h)
            self._h = C.c_void_p()

    def _close_quietly(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _sync(self, fn, result, *args):
        """a synchronous call: fn(handle, *args, &res) on a fresh result(), which it returns"""
        return _filled(fn, result, self._h, *args)

    def _enqueue(self, fn, *args):
        """an asynchronous call: fn(handle, *args), whose last argument is the device record it leaves"""
        _check(getattr(self._L, fn)(self._h, *args))


class Context(_Handle):
    """Owns one mcamd_ctx (one device, one stream)."""
    _destroy = "mcamd_ctx_destroy"
    __del__ = _Handle._close_quietly

    def __init__(self, device: int = 0, stream: int | None = None):
        super().__init__()
        _check(self._L.mcamd_ctx_create(device, C.c_void_p(stream) if stream else None, C.byref(self._h)))

    def device_info(self) -> DeviceInfo:
        return self._sync("mcamd_get_device_info", DeviceInfo)

    def price_paths(self, opt: Option, sim: Sim) -> Result:
        return self._sync("mcamd_price_paths", Result, opt, sim)

    def price_paths_enqueue(self, opt: Option, sim: Sim, stats) -> None:
        """Asynchronous: leaves {sum, sumsq, sum_c, sum_cc, sum_yc, n} in the device tensor `stats` (>= 6 doubles)."""
        self._enqueue("mcamd_price_paths_enqueue", opt, sim, _ptr(stats))

    def price_greeks(self, opt: Option, sim: Sim, method: int = GREEKS_AUTO) -> Greeks:
        return self._sync("mcamd_price_greeks", Greeks, opt, sim, method)

    def price_greeks_enqueue(self, opt: Option, sim: Sim, stats, method: int = GREEKS_AUTO) -> None:
        """Asynchronous: leaves the 16-double Greeks record in the device tensor `stats` (finalize_greeks_stats)."""
        self._enqueue("mcamd_price_greeks_enqueue", opt, sim, method, _ptr(stats))

    def price_barrier(self, opt: Option, sim: Sim, barrier: Barrier, samples=None) -> Result:
        """Single-barrier option (mcamd_price_barrier); opt.B is the level.  samples: optional device tensor of
        n_paths_local values of the path precision that receives each path's undiscounted sample."""
        return self._sync("mcamd_price_barrier", Result, opt, sim, barrier, _ptr(samples))

    def price_barrier_enqueue(self, opt: Option, sim: Sim, barrier: Barrier, stats, samples=None) -> None:
        """Asynchronous: leaves {sum, sumsq, 0, 0, 0, n} in the device tensor `stats` (>= 6 doubles; finalize_stats)."""
        self._enqueue("mcamd_price_barrier_enqueue", opt, sim, barrier, _ptr(samples), _ptr(stats))

    def localvol_surface(self, grid_args, sigma) -> "LocalVolSurface":
        """An immutable local-volatility surface on this context (mcamd_localvol_surface_create).  grid_args: a
        LocalVolGrid or its (n_t, n_x, x_min, x_max); sigma: n_t rows of n_x volatilities.  close() it (or use it as a
        context manager) before the context is closed."""
        return LocalVolSurface(self, grid_args, sigma)

    def price_localvol(self, opt: Option, sim: Sim, localvol: LocalVol, surface: "LocalVolSurface", samples=None) -> Result:
        """European or single-barrier option under a local-volatility surface (mcamd_price_localvol); opt.v is
        ignored, opt.B is the barrier level.  samples: optional device tensor of n_paths_local values of the path
        precision that receives each path's undiscounted sample."""
        return self._sync("mcamd_price_localvol", Result, opt, sim, localvol, surface._h, _ptr(samples))

    def price_localvol_enqueue(self, opt: Option, sim: Sim, localvol: LocalVol, surface: "LocalVolSurface", stats,
                               samples=None) -> None:
        """Asynchronous: leaves {sum, sumsq, 0, 0, 0, n} in the device tensor `stats` (>= 6 doubles; finalize_stats)."""
        self._enqueue("mcamd_price_localvol_enqueue", opt, sim, localvol, surface._h, _ptr(samples), _ptr(stats))

    def price_cliquet(self, opt: Option, sim: Sim, cliquet: Cliquet, surface: "LocalVolSurface",
                      samples=None) -> CliquetResult:
        """Cliquet, forward-start option or realized-variance swap on the paths of price_localvol
        (mcamd_price_cliquet); r, T and S0 come from opt, opt.v, opt.K and opt.B are ignored.  samples: optional device
        tensor of n_paths_local values of the path precision that receives each path's undiscounted sample."""
        return self._sync("mcamd_price_cliquet", CliquetResult, opt, sim, cliquet, surface._h, _ptr(samples))

    def price_cliquet_enqueue(self, opt: Option, sim: Sim, cliquet: Cliquet, surface: "LocalVolSurface", stats,
                              samples=None) -> None:
        """Asynchronous: leaves {sum, sumsq, n_floored, n_capped, 0, n} in the device tensor `stats` (>= 6 doubles;
        finalize_stats)."""
        self._enqueue("mcamd_price_cliquet_enqueue", opt, sim, cliquet, surface._h, _ptr(samples), _ptr(stats))

    def price_heston(self, opt: Option, sim: Sim, heston: Heston, samples=None, state=None) -> HestonResult:
        """European option under Heston stochastic volatility, full-truncation Euler in the log-price
        (mcamd_price_heston); r, T, S0 and K come from opt, opt.v and opt.B are ignored.  samples: optional device
        tensor of n_paths_local values of the path precision that receives each path's undiscounted sample; state:
        optional device tensor of 2 x n_paths_local such values that receives S_T, then the raw final variance."""
        return self._sync("mcamd_price_heston", HestonResult, opt, sim, heston, _ptr(samples), _ptr(state))

    def price_heston_enqueue(self, opt: Option, sim: Sim, heston: Heston, stats, samples=None, state=None) -> None:
        """Asynchronous: leaves {sum, sumsq, truncated_steps, sum of the paths' average variance, 0, n} in the device
        tensor `stats` (>= 6 doubles; finalize_stats)."""
        self._enqueue("mcamd_price_heston_enqueue", opt, sim, heston, _ptr(samples), _ptr(state), _ptr(stats))

    def price_heston_cliquet(self, opt: Option, sim: Sim, heston: Heston, cliquet: Cliquet,
                             samples=None) -> HestonCliquetResult:
        """Cliquet, forward-start option or realized-variance swap on the paths of price_heston
        (mcamd_price_heston_cliquet); r, T and S0 come from opt, opt.v, opt.K and opt.B are ignored, heston.payoff is
        not read and cliquet.q must equal heston.q.  samples: optional device tensor of n_paths_local values of the
        path precision that receives each path's undiscounted sample."""
        return self._sync("mcamd_price_heston_cliquet", HestonCliquetResult, opt, sim, heston, cliquet, _ptr(samples))

    def price_heston_cliquet_enqueue(self, opt: Option, sim: Sim, heston: Heston, cliquet: Cliquet, stats,
                                     samples=None) -> None:
        """Asynchronous: leaves {sum, sumsq, n_floored, n_capped, sum of the paths' average variance, n} in the device
        tensor `stats` (>= 6 doubles; finalize_stats)."""
        self._enqueue("mcamd_price_heston_cliquet_enqueue", opt, sim, heston, cliquet, _ptr(samples), _ptr(stats))

    def price_heston_barrier(self, opt: Option, sim: Sim, heston: Heston, barrier: Barrier, samples=None,
                             state=None) -> HestonBarrierResult:
        """Single-barrier option on the paths of price_heston (mcamd_price_heston_barrier); r, T, S0, K and the level B
        come from opt, opt.v is ignored, and heston.payoff must equal barrier.payoff.  samples: optional device tensor
        of n_paths_local values of the path precision that receives each path's undiscounted sample; state: optional
        device tensor of 3 x n_paths_local such values that receives S_T, then the raw final variance, then the
        survival weight (a knock-out path that was hit: NaN, NaN, 0)."""
        return self._sync("mcamd_price_heston_barrier", HestonBarrierResult, opt, sim, heston, barrier, _ptr(samples),
                          _ptr(state))

    def price_heston_barrier_enqueue(self, opt: Option, sim: Sim, heston: Heston, barrier: Barrier, stats, samples=None,
                                     state=None) -> None:
        """Asynchronous: leaves {sum, sumsq, live_steps, truncated_steps, sum of v+ over the counted lane-steps, n} in
        the device tensor `stats` (>= 6 doubles; finalize_stats)."""
        self._enqueue("mcamd_price_heston_barrier_enqueue", opt, sim, heston, barrier, _ptr(samples), _ptr(state),
                      _ptr(stats))

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
        self._enqueue("mcamd_price_heston_smile_enqueue", opt, sim, heston, smile.n_expiries, smile.n_strikes, steps, ks,
                      _ptr(state), _ptr(stats))

    def price_heston_greeks(self, opt: Option, sim: Sim, heston: Heston, job, samples=None):
        """Price, delta, gamma, rho, rho_q and the sensitivities to v0, kappa, theta, xi and rho of price_heston's option
        from one simulation on shared draws (mcamd_price_heston_greeks of include/mcamd_heston_greeks.h).  job:
        heston_greeks.make_job(...); returns a heston_greeks.HestonGreeks.  The binding lives in the module
        heston_greeks, imported here and not at the top: the structs of this module are those of mcamd.h."""
        from . import heston_greeks
        return heston_greeks.price(self, opt, sim, heston, job, samples)

    def price_heston_greeks_enqueue(self, opt: Option, sim: Sim, heston: Heston, job, stats, samples=None) -> None:
        """Asynchronous: leaves the 32-double record in the device tensor `stats` (heston_greeks.finalize_stats)."""
        from . import heston_greeks
        heston_greeks.enqueue(self, opt, sim, heston, job, stats, samples)

    def price_localvol_greeks(self, opt: Option, sim: Sim, job: LocalVolGreeksJob, surface: "LocalVolSurface",
                              samples=None) -> LocalVolGreeks:
        """Price, delta, gamma, vega, bucketed vega, rho and dividend rho of a European option under a local-volatility
        surface from one walk of the paths (mcamd_price_localvol_greeks); opt.v is ignored.  samples: optional device
        tensor of (6 + n_vega_buckets) x n_paths_local doubles, estimator-major, that receives every path's
        undiscounted samples."""
        return self._sync("mcamd_price_localvol_greeks", LocalVolGreeks, opt, sim, job, surface._h, _ptr(samples))

    def price_localvol_greeks_enqueue(self, opt: Option, sim: Sim, job: LocalVolGreeksJob, surface: "LocalVolSurface",
                                      stats, samples=None) -> None:
        """Asynchronous: leaves the 32-double record in the device tensor `stats` (finalize_localvol_greeks_stats)."""
        self._enqueue("mcamd_price_localvol_greeks_enqueue", opt, sim, job, surface._h, _ptr(samples), _ptr(stats))

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
        self._enqueue("mcamd_price_localvol_smile_enqueue", opt, sim, smile, steps, ks, surface._h, _ptr(spots),
                      _ptr(stats))

    def price_lookback(self, opt: Option, sim: Sim, lookback: Lookback, samples=None) -> Result:
        """Lookback option (mcamd_price_lookback).  samples: optional device tensor of n_paths_local values of the path
        precision that receives each path's undiscounted sample."""
        return self._sync("mcamd_price_lookback", Result, opt, sim, lookback, _ptr(samples))

    def price_lookback_enqueue(self, opt: Option, sim: Sim, lookback: Lookback, stats, samples=None) -> None:
        """Asynchronous: leaves {sum, sumsq, 0, 0, 0, n} in the device tensor `stats` (>= 6 doubles; finalize_stats)."""
        self._enqueue("mcamd_price_lookback_enqueue", opt, sim, lookback, _ptr(samples), _ptr(stats))

    def price_asian(self, opt: Option, sim: Sim, asian: Asian, samples=None) -> Result:
        """Asian option (mcamd_price_asian).  samples: optional device tensor of n_paths_local values of the path
        precision; receives the undiscounted sample of every path (never the control-adjusted value)."""
        return self._sync("mcamd_price_asian", Result, opt, sim, asian, _ptr(samples))

    def price_asian_enqueue(self, opt: Option, sim: Sim, asian: Asian, stats, samples=None) -> None:
        """Asynchronous: leaves {sum y, sum y^2, sum c, sum c^2, sum y c, n} in the device tensor `stats` (>= 6 doubles;
        finalize_stats, with control_variate=True for a controlled job)."""
        self._enqueue("mcamd_price_asian_enqueue", opt, sim, asian, _ptr(samples), _ptr(stats))

    def price_autocall(self, opt: Option, sim: Sim, autocall: Autocall, samples=None) -> AutocallResult:
        """Worst-of autocallable note (mcamd_price_autocall): r and T come from opt.  samples: optional device tensor of
        n_paths_local values of the path precision that receives every path's sample, in maturity money."""
        return self._sync("mcamd_price_autocall", AutocallResult, opt, sim, autocall, _ptr(samples))

    def price_autocall_enqueue(self, opt: Option, sim: Sim, autocall: Autocall, stats, samples=None) -> None:
        """Asynchronous: leaves {sum, sumsq, n_called, sum_t_call, n_knocked_in, n} in the device tensor `stats`
        (>= 6 doubles; finalize_stats without the control variate)."""
        self._enqueue("mcamd_price_autocall_enqueue", opt, sim, autocall, _ptr(samples), _ptr(stats))

    def price_autocall_localvol(self, opt: Option, sim: Sim, autocall: AutocallLocalVol, surfaces,
                                samples=None) -> AutocallResult:
        """Worst-of autocallable note under per-asset local-volatility surfaces (mcamd_price_autocall_localvol): r and T
        come from opt; surfaces: one LocalVolSurface per asset (the same one may appear several times).  samples:
        optional device tensor of n_paths_local values of the path precision that receives every path's sample."""
        return self._sync("mcamd_price_autocall_localvol", AutocallResult, opt, sim, autocall, surface_array(surfaces),
                          _ptr(samples))

    def price_autocall_localvol_enqueue(self, opt: Option, sim: Sim, autocall: AutocallLocalVol, surfaces, stats,
                                        samples=None) -> None:
        """Asynchronous: leaves {sum, sumsq, n_called, sum_t_call, n_knocked_in, n} in the device tensor `stats`
        (>= 6 doubles; finalize_stats without the control variate).  The surfaces must outlive the enqueued work."""
        self._enqueue("mcamd_price_autocall_localvol_enqueue", opt, sim, autocall, surface_array(surfaces),
                      _ptr(samples), _ptr(stats))

    def price_basket(self, opt: Option, sim: Sim, basket: Basket, samples=None) -> Result:
        """Basket, spread or rainbow option on correlated assets (mcamd_price_basket): r, T, K and the barrier level B
        come from opt.  samples: optional device tensor of n_paths_local values of the path precision that receives
        each path's undiscounted sample."""
        return self._sync("mcamd_price_basket", Result, opt, sim, basket, _ptr(samples))

    def price_basket_enqueue(self, opt: Option, sim: Sim, basket: Basket, stats, samples=None) -> None:
        """Asynchronous: leaves {sum, sumsq, 0, 0, 0, n} in the device tensor `stats` (>= 6 doubles; finalize_stats)."""
        self._enqueue("mcamd_price_basket_enqueue", opt, sim, basket, _ptr(samples), _ptr(stats))

    def price_american(self, opt: Option, sim: Sim, am: American, work, coeffs: bool = False):
        """Least-squares Monte Carlo price of an American / Bermudan put or call (mcamd_price_american).  work: a device
        tensor of at least american_workspace_bytes(am, sim) bytes.  Returns the AmericanResult, and with coeffs=True
        also the (M, n_basis + 1) array of per-date coefficients and regressed flags."""
        nb = am.n_basis or 3
        M = sim.n_steps // am.exercise_every if am.exercise_every else 0
        arr = (C.c_double * (M * (nb + 1)))() if coeffs and M > 0 else None
        nbytes = work.numel() * work.element_size() if work is not None else 0
        res = self._sync("mcamd_price_american", AmericanResult, opt, sim, am, _ptr(work), nbytes, arr)
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
        table = None
        if coeffs is not None:
            table = np.ascontiguousarray(coeffs, dtype=np.float64)
            nb = am.n_basis or 3
            M = sim.n_steps // am.exercise_every if am.exercise_every else 0
            if table.size != M * (nb + 1):
                raise ValueError(f"coeffs holds {table.size} doubles; {M} dates x ({nb} + 1) expected")
        nbytes = work.numel() * work.element_size() if work is not None else 0
        return self._sync("mcamd_american_upper_bound", AmericanDualResult, opt, sim, am, dual,
                          None if table is None else table.ctypes.data_as(C.POINTER(C.c_double)), _ptr(work), nbytes,
                          _ptr(cont))

    def enqueued_kernel_ms(self, n_last: int):
        arr = (C.c_float * n_last)()
        _check(self._L.mcamd_enqueued_kernel_ms(self._h, n_last, arr))
        return list(arr)

    def simulate_trajectories(self, opt: Option, sim: Sim, traj, counts=None, payoffs=None,
                              layout=STEP_MAJOR) -> Result:
        return self._sync("mcamd_simulate_trajectories", Result, opt, sim, layout, _ptr(traj), _ptr(counts),
                          _ptr(payoffs))

    def simulate_trajectories_enqueue(self, opt: Option, sim: Sim, traj, counts, payoffs, stats, layout=STEP_MAJOR) -> None:
        self._enqueue("mcamd_simulate_trajectories_enqueue", opt, sim, layout, _ptr(traj), _ptr(counts), _ptr(payoffs),
                      _ptr(stats))

    def nmc_inner_enqueue(self, opt: Option, sim: Sim, prices, counts, point_prices, stats, layout=STEP_MAJOR,
                          variant=NMC_WAVE_PER_POINT) -> None:
        self._enqueue("mcamd_nmc_inner_enqueue", opt, sim, layout, variant, _ptr(prices), _ptr(counts),
                      _ptr(point_prices), _ptr(stats))

    def nmc_fused_enqueue(self, opt: Option, sim: Sim, outer_seed: int, prices, counts, point_prices, stats,
                          layout=STEP_MAJOR) -> None:
        self._enqueue("mcamd_nmc_fused_enqueue", opt, sim, outer_seed, layout, _ptr(prices), _ptr(counts),
                      _ptr(point_prices), _ptr(stats))

    def diag_store_pattern(self, n_paths_local: int, n_steps: int, precision: int, traj, payoffs=None) -> float:
        """kernel ms of the store kernel's pure store stream (diagnostic: the same-run HBM write ceiling)"""
        return self._sync("mcamd_diag_store_pattern", C.c_float, n_paths_local, n_steps, precision, _ptr(traj),
                          _ptr(payoffs)).value

    def price_from_normals(self, opt: Option, sim: Sim, normals, payoffs=None) -> Result:
        return self._sync("mcamd_price_from_normals", Result, opt, sim, _ptr(normals), _ptr(payoffs))

    def generate_normals(self, seed: int, n: int, precision: int, out) -> float:
        return self._sync("mcamd_generate_normals", C.c_float, seed, n, precision, _ptr(out)).value

    def reduce_sum(self, x, n: int, precision: int, variant: int = REDUCE_GRID_STRIDE):
        s = C.c_double(0)
        ms = self._sync("mcamd_reduce_sum", C.c_float, _ptr(x), n, precision, variant, s)
        return s.value, ms.value

    def reduce_partials(self, x, n: int, precision: int, variant: int, n_blocks: int):
        """one partial sum per workgroup (they add up to the complete sum) and the kernel's ms"""
        arr = (C.c_double * n_blocks)()
        ms = self._sync("mcamd_reduce_partials", C.c_float, _ptr(x), n, precision, variant, n_blocks, arr)
        return list(arr), ms.value

    def nmc_inner(self, opt: Option, sim: Sim, prices, counts, point_prices, layout=STEP_MAJOR,
                  variant=NMC_WAVE_PER_POINT) -> Result:
        return self._sync("mcamd_nmc_inner", Result, opt, sim, layout, variant, _ptr(prices), _ptr(counts),
                          _ptr(point_prices))

    def nmc_fused(self, opt: Option, sim: Sim, outer_seed: int, prices, counts, point_prices,
                  layout=STEP_MAJOR) -> Result:
        return self._sync("mcamd_nmc_fused", Result, opt, sim, outer_seed, layout, _ptr(prices), _ptr(counts),
                          _ptr(point_prices))


class LocalVolSurface(_Handle):
    """Owns one mcamd_localvol_surface: the pair tables of a local-volatility surface in the memory of one context's
    device.  Immutable; several may be alive in one context."""
    _destroy = "mcamd_localvol_surface_destroy"
    __del__ = _Handle._close_quietly

    def __init__(self, ctx: Context, grid_args, sigma):
        super().__init__()
        self.grid = grid_args if isinstance(grid_args, LocalVolGrid) else make_localvol_grid(*grid_args)
        _check(self._L.mcamd_localvol_surface_create(ctx._h, C.byref(self.grid), _sigma_array(self.grid, sigma),
                                                     C.byref(self._h)))


class Group(_Handle):
    """Single-process multi-GPU group: one context per device + an RCCL communicator clique (mcamd_group_*)."""
    # no __del__, unlike Context and LocalVolSurface: the garbage collector must not tear RCCL down at interpreter
    # exit; a group ends with close() or its with block
    _destroy = "mcamd_group_destroy"

    def __init__(self, n_devices: int = 0, devices=None):
        super().__init__()
        arr = (C.c_int * len(devices))(*devices) if devices else None
        _check(self._L.mcamd_group_create(len(devices) if devices else n_devices, arr, C.byref(self._h)))

    def size(self) -> int:
        return self._sync("mcamd_group_size", C.c_int).value

    def price_paths(self, opt: Option, sim: Sim) -> Result:
        return self._sync("mcamd_group_price_paths", Result, opt, sim)

    def price_greeks(self, opt: Option, sim: Sim, method: int = GREEKS_AUTO) -> Greeks:
        return self._sync("mcamd_group_price_greeks", Greeks, opt, sim, method)

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
        return self._sync("mcamd_group_simulate_trajectories", Result, opt, sim, layout, self._ptrs(traj),
                          self._ptrs(counts), self._ptrs(payoffs))

    def nmc_inner(self, opt: Option, sim: Sim, prices, counts, point_prices, layout=STEP_MAJOR,
                  variant=NMC_WAVE_PER_POINT) -> Result:
        return self._sync("mcamd_group_nmc_inner", Result, opt, sim, layout, variant, self._ptrs(prices),
                          self._ptrs(counts), self._ptrs(point_prices))

    def nmc_fused(self, opt: Option, sim: Sim, outer_seed: int, prices, counts, point_prices, layout=STEP_MAJOR) -> Result:
        return self._sync("mcamd_group_nmc_fused", Result, opt, sim, outer_seed, layout, self._ptrs(prices),
                          self._ptrs(counts), self._ptrs(point_prices))
