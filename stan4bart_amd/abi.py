"""ctypes view of the C-ABI declared in ``include/stan4bart_amd.h``.

This is the Python stand-in for the R ``.Call`` shim (there is no R in this image): it marshals
numpy arrays into the plain structs of the C boundary, exactly as the R shim in
``INTEGRATION.md`` unpacks SEXPs.  The class is generic over the symbol prefix so that the test
suite can drive the CPU oracle (``orc_*``, test infrastructure only) through the very same code.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass, field
from fractions import Fraction
from typing import Callable, Optional, Sequence

import numpy as np

INTERFACE_VERSION = 6     # S4B_INTERFACE_VERSION of include/stan4bart_amd.h (tests/test_host_logic.py compares the two)
c_double_p = C.POINTER(C.c_double)
c_int32_p = C.POINTER(C.c_int32)
c_uint32_p = C.POINTER(C.c_uint32)


class BartControl(C.Structure):
    _fields_ = [("n_trees", C.c_int32), ("n_thin", C.c_int32), ("keep_trees", C.c_int32),
                ("node_capacity", C.c_int32),
                ("base", C.c_double), ("power", C.c_double), ("k", C.c_double), ("node_scale", C.c_double),
                ("birth_or_death_prob", C.c_double), ("swap_prob", C.c_double),
                ("change_prob", C.c_double), ("birth_prob", C.c_double),
                ("split_probs", c_double_p), ("use_quantiles", C.c_int32), ("interface_version", C.c_int32),
                ("k_hyper_df", C.c_double), ("k_hyper_scale", C.c_double)]


class BartData(C.Structure):
    _fields_ = [("n", C.c_int64), ("p", C.c_int32), ("reserved", C.c_int32),
                ("x", c_double_p), ("n_cuts", c_int32_p),
                ("n_test", C.c_int64), ("x_test", c_double_p)]


class StanData(C.Structure):
    _fields_ = [("N", C.c_int64), ("K", C.c_int32),
                ("is_binary", C.c_int32), ("has_intercept", C.c_int32), ("has_weights", C.c_int32),
                ("prior_dist", C.c_int32), ("prior_dist_for_aux", C.c_int32),
                ("X", c_double_p), ("y", c_double_p), ("weights", c_double_p),
                ("prior_scale", c_double_p), ("prior_mean", c_double_p), ("prior_df", c_double_p),
                ("prior_scale_for_aux", C.c_double), ("prior_mean_for_aux", C.c_double),
                ("prior_df_for_aux", C.c_double),
                ("t", C.c_int32), ("q", C.c_int32),
                ("len_theta_L", C.c_int32), ("len_concentration", C.c_int32),
                ("len_regularization", C.c_int32), ("reserved", C.c_int32),
                ("p", c_int32_p), ("l", c_int32_p),
                ("shape", c_double_p), ("scale", c_double_p),
                ("concentration", c_double_p), ("regularization", c_double_p),
                ("num_non_zero", C.c_int64),
                ("w", c_double_p), ("v", c_int32_p), ("u", c_int32_p),
                ("global_prior_df", C.c_double), ("global_prior_scale", C.c_double),
                ("slab_df", C.c_double), ("slab_scale", C.c_double), ("num_normals", c_int32_p)]


class StanControl(C.Structure):
    _fields_ = [("seed", C.c_uint32), ("skip", C.c_int32), ("init_r", C.c_double),
                ("adapt_gamma", C.c_double), ("adapt_delta", C.c_double),
                ("adapt_kappa", C.c_double), ("adapt_t0", C.c_double),
                ("adapt_init_buffer", C.c_uint32), ("adapt_term_buffer", C.c_uint32),
                ("adapt_window", C.c_uint32), ("reserved", C.c_uint32),
                ("stepsize", C.c_double), ("stepsize_jitter", C.c_double),
                ("max_treedepth", C.c_int32), ("hmc_mode", C.c_int32)]


CALLBACK = C.CFUNCTYPE(C.c_int, C.c_void_p, c_double_p, c_double_p, c_double_p, C.c_int32)
PROGRESS = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int32, C.c_int32, C.c_int32)


class CommonControl(C.Structure):
    _fields_ = [("warmup", C.c_int32), ("iter", C.c_int32), ("verbose", C.c_int32), ("refresh", C.c_int32),
                ("is_binary", C.c_int32), ("offset_type", C.c_int32), ("keep_fits", C.c_int32),
                ("device", C.c_int32),
                ("offset", c_double_p), ("bart_offset_init", c_double_p),
                ("sigma_init", C.c_double),
                ("callback", CALLBACK), ("callback_user", C.c_void_p)]


class Results(C.Structure):
    _fields_ = [("stan", c_double_p), ("bart_sigma", c_double_p), ("bart_train", c_double_p),
                ("bart_test", c_double_p), ("bart_varcount", c_int32_p), ("bart_k", c_double_p)]


class SummaryIn(C.Structure):          # s4b_summary_in
    _fields_ = [("x_test", c_double_p), ("n_test", C.c_int64), ("offset", c_double_p),
                ("n_dense", C.c_int32), ("n_ell", C.c_int32), ("n_ell_coef", C.c_int32), ("link", C.c_int32), ("n_weights", C.c_int32),
                ("route", C.c_int32), ("stage_nodes", C.c_int32), ("max_workgroups", C.c_int32),
                ("dense", c_double_p), ("dense_coef", c_double_p), ("ell_index", c_int32_p), ("ell_value", c_double_p), ("ell_coef", c_double_p),
                ("weights", c_double_p)]


class SummaryOut(C.Structure):         # s4b_summary_out
    _fields_ = [("mean", c_double_p), ("m2", c_double_p), ("average", c_double_p), ("num_samples", C.c_int64), ("info", C.c_int64 * 8)]


class PdIn(C.Structure):               # s4b_pd_in
    _fields_ = [("rows", SummaryIn), ("n_vars", C.c_int32), ("vars", C.c_int32 * 2), ("n_grid", C.c_int32), ("grid", c_double_p)]


class PdOut(C.Structure):              # s4b_pd_out
    _fields_ = [("pd", c_double_p), ("num_samples", C.c_int64), ("info", C.c_int64 * 8)]


class QuantileIn(C.Structure):         # s4b_quantile_in
    _fields_ = [("rows", SummaryIn), ("n_probs", C.c_int32), ("probs", c_double_p), ("n_peers", C.c_int32), ("peers", C.POINTER(C.c_void_p)),
                ("peer_dense_coef", C.POINTER(c_double_p)), ("peer_ell_coef", C.POINTER(c_double_p)), ("scratch_bytes", C.c_int64)]


class QuantileOut(C.Structure):        # s4b_quantile_out
    _fields_ = [("quantiles", c_double_p), ("num_samples", C.c_int64), ("info", C.c_int64 * 8)]


class ContrastIn(C.Structure):         # s4b_contrast_in
    _fields_ = [("rows", SummaryIn), ("x_test0", c_double_p), ("offset0", c_double_p), ("dense0", c_double_p), ("ell_index0", c_int32_p),
                ("ell_value0", c_double_p), ("n_probs", C.c_int32), ("probs", c_double_p), ("n_peers", C.c_int32), ("peers", C.POINTER(C.c_void_p)),
                ("peer_dense_coef", C.POINTER(c_double_p)), ("peer_ell_coef", C.POINTER(c_double_p)), ("scratch_bytes", C.c_int64)]


class ContrastOut(C.Structure):        # s4b_contrast_out
    _fields_ = [("mean", c_double_p), ("m2", c_double_p), ("average", c_double_p), ("quantiles", c_double_p), ("num_samples", C.c_int64),
                ("info", C.c_int64 * 8)]


class GroupsIn(C.Structure):           # s4b_groups_in
    _fields_ = [("arms", ContrastIn), ("n_arms", C.c_int32), ("level", c_int32_p), ("n_levels", C.c_int64), ("statistic", C.c_int32),
                ("has_threshold", C.c_int32), ("threshold", C.c_double), ("level_bytes", C.c_int64)]


class GroupsOut(C.Structure):          # s4b_groups_out
    _fields_ = [("mean", c_double_p), ("m2", c_double_p), ("quantiles", c_double_p), ("p_above", c_double_p), ("weight", c_double_p),
                ("count", C.POINTER(C.c_int64)), ("draws", c_double_p), ("num_samples", C.c_int64), ("info", C.c_int64 * 8)]


class ProjectionIn(C.Structure):       # s4b_projection_in
    _fields_ = [("arms", ContrastIn), ("n_arms", C.c_int32), ("n_columns", C.c_int32), ("design", c_double_p), ("has_threshold", C.c_int32),
                ("threshold", C.c_double), ("tol", C.c_double)]


class ProjectionOut(C.Structure):      # s4b_projection_out
    _fields_ = [("coef", c_double_p), ("r2", c_double_p), ("mean", c_double_p), ("m2", c_double_p), ("quantiles", c_double_p), ("p_above", c_double_p),
                ("weight", C.c_double), ("num_samples", C.c_int64), ("info", C.c_int64 * 8)]


class SpreadIn(C.Structure):           # s4b_spread_in
    _fields_ = [("arms", ContrastIn), ("n_arms", C.c_int32), ("n_thresholds", C.c_int32), ("thresholds", c_double_p), ("bin_index", C.c_int32)]


class SpreadOut(C.Structure):          # s4b_spread_out
    _fields_ = [("mean", c_double_p), ("m2", c_double_p), ("quantiles", c_double_p), ("draws", c_double_p), ("weight", C.c_double),
                ("num_samples", C.c_int64), ("info", C.c_int64 * 8)]


class PpdIn(C.Structure):              # s4b_ppd_in
    _fields_ = [("rows", SummaryIn), ("y", c_double_p), ("sigma", c_double_p), ("row_scale", c_double_p), ("noise_key", C.c_uint64),
                ("n_probs", C.c_int32), ("probs", c_double_p), ("n_peers", C.c_int32), ("peers", C.POINTER(C.c_void_p)),
                ("peer_dense_coef", C.POINTER(c_double_p)), ("peer_ell_coef", C.POINTER(c_double_p)), ("peer_sigma", C.POINTER(c_double_p)),
                ("scratch_bytes", C.c_int64)]


class CheckIn(C.Structure):            # s4b_check_in
    _fields_ = [("rows", SummaryIn), ("y", c_double_p), ("sigma", c_double_p), ("row_scale", c_double_p), ("noise_key", C.c_uint64),
                ("row_weights", c_double_p), ("n_thresholds", C.c_int32), ("thresholds", c_double_p), ("bin_index", C.c_int32),
                ("n_probs", C.c_int32), ("probs", c_double_p), ("n_peers", C.c_int32), ("peers", C.POINTER(C.c_void_p)),
                ("peer_dense_coef", C.POINTER(c_double_p)), ("peer_ell_coef", C.POINTER(c_double_p)), ("peer_sigma", C.POINTER(c_double_p)),
                ("scratch_bytes", C.c_int64)]


class CheckOut(C.Structure):           # s4b_check_out
    _fields_ = [("mean", c_double_p), ("m2", c_double_p), ("quantiles", c_double_p), ("draws", c_double_p), ("observed", c_double_p),
                ("weight", C.c_double), ("num_samples", C.c_int64), ("info", C.c_int64 * 8)]


class CurvesIn(C.Structure):           # s4b_curves_in
    _fields_ = [("rows", SummaryIn), ("n_vars", C.c_int32), ("vars", C.c_int32 * 2), ("n_grid", C.c_int32), ("grid", c_double_p),
                ("anchor", C.c_int32), ("n_probs", C.c_int32), ("probs", c_double_p), ("n_peers", C.c_int32),
                ("peers", C.POINTER(C.c_void_p)), ("peer_dense_coef", C.POINTER(c_double_p)), ("peer_ell_coef", C.POINTER(c_double_p)),
                ("scratch_bytes", C.c_int64)]


class CurvesOut(C.Structure):          # s4b_curves_out
    _fields_ = [("mean", c_double_p), ("m2", c_double_p), ("quantiles", c_double_p), ("p_max", c_double_p), ("p_min", c_double_p),
                ("range_mean", c_double_p), ("range_m2", c_double_p), ("range_quantiles", c_double_p), ("num_samples", C.c_int64),
                ("info", C.c_int64 * 8)]


class DescribeIn(C.Structure):         # s4b_describe_in
    _fields_ = [("arms", ContrastIn), ("n_arms", C.c_int32), ("n_hdi", C.c_int32), ("hdi_count", c_int32_p), ("n_thresholds", C.c_int32),
                ("thresholds", c_double_p)]


class DescribeOut(C.Structure):        # s4b_describe_out
    _fields_ = [("quantiles", c_double_p), ("median", c_double_p), ("hdi", c_double_p), ("hdi_start", c_int32_p), ("n_above", c_int32_p),
                ("n_below", c_int32_p), ("mad", c_double_p), ("num_samples", C.c_int64), ("info", C.c_int64 * 8)]


class SortedIn(C.Structure):           # s4b_sorted_in
    _fields_ = [("arms", ContrastIn), ("n_arms", C.c_int32), ("n_row_probs", C.c_int32), ("row_probs", c_double_p), ("n_cuts", C.c_int32),
                ("cut_rank", c_int32_p)]


class SortedOut(C.Structure):          # s4b_sorted_out
    _fields_ = [("mean", c_double_p), ("m2", c_double_p), ("quantiles", c_double_p), ("draws", c_double_p), ("n_above", c_int32_p),
                ("n_below", c_int32_p), ("num_samples", C.c_int64), ("info", C.c_int64 * 8)]


class PpdOut(C.Structure):             # s4b_ppd_out
    _fields_ = [("quantiles", c_double_p), ("lpd", c_double_p), ("lmean", c_double_p), ("lm2", c_double_p), ("pit", c_double_p),
                ("num_samples", C.c_int64), ("info", C.c_int64 * 8)]


class LooIn(C.Structure):              # s4b_loo_in
    _fields_ = [("rows", SummaryIn), ("y", c_double_p), ("sigma", c_double_p), ("row_scale", c_double_p), ("tail_len", C.c_int32),
                ("n_peers", C.c_int32), ("peers", C.POINTER(C.c_void_p)), ("peer_dense_coef", C.POINTER(c_double_p)),
                ("peer_ell_coef", C.POINTER(c_double_p)), ("peer_sigma", C.POINTER(c_double_p)), ("scratch_bytes", C.c_int64)]


class LooOut(C.Structure):             # s4b_loo_out
    _fields_ = [("elpd_loo", c_double_p), ("pareto_k", c_double_p), ("lpd", c_double_p), ("ess", c_double_p), ("num_samples", C.c_int64),
                ("tail_len", C.c_int32), ("info", C.c_int64 * 8)]


class ConvIn(C.Structure):             # s4b_conv_in
    _fields_ = [("rows", SummaryIn), ("quantity", C.c_int32), ("split", C.c_int32), ("y", c_double_p), ("sigma", c_double_p), ("row_scale", c_double_p),
                ("n_peers", C.c_int32), ("peers", C.POINTER(C.c_void_p)), ("peer_dense_coef", C.POINTER(c_double_p)),
                ("peer_ell_coef", C.POINTER(c_double_p)), ("peer_sigma", C.POINTER(c_double_p)), ("scratch_bytes", C.c_int64)]


class ConvOut(C.Structure):            # s4b_conv_out
    _fields_ = [("rhat", c_double_p), ("ess", c_double_p), ("mean", c_double_p), ("mcse", c_double_p), ("n_pairs", C.POINTER(C.c_int32)),
                ("num_samples", C.c_int64), ("n_chains", C.c_int32), ("chain_len", C.c_int32), ("info", C.c_int64 * 8)]


SUMMARY_ROUTES = {"auto": 0, "staged": 1, "global": 2}
SUMMARY_INFO = ("route", "rows_per_tile", "workgroups", "staging_bytes", "largest_draw_nodes", "launches", "device_bytes", "staging_nodes")
PD_INFO = SUMMARY_INFO[:7] + ("largest_affected", "total_affected")          # (the last two share info[7]: trees with a rule on a varied predictor)
QUANTILE_INFO = ("route", "rows_per_chunk", "chunks", "rows_per_sort", "padded_draws", "largest_draw_nodes", "launches", "device_bytes", "draws")
CONTRAST_INFO = ("route", "rows_per_chunk", "chunks", "launches", "device_bytes", "draws", "differing_columns", "largest_affected", "total_affected")
GROUPS_INFO = ("route", "rows_per_chunk", "chunks", "launches", "device_bytes", "draws", "edge_levels", "nan_levels")
GROUPS_STATISTICS = {"sum": 0, "mean": 1}
GROUPS_LEVEL_BYTES_MAX = 1 << 30       # S4B_GROUPS_LEVEL_BYTES_MAX: the level matrix (8 x levels x pooled draws) of one s4b_predict_groups call at most
PROJECTION_INFO = ("route", "rows_per_chunk", "chunks", "launches", "device_bytes", "draws", "deficient", "columns")
PROJECTION_COLUMNS_MAX = 32            # S4B_PROJECTION_COLUMNS_MAX: design columns of one s4b_predict_projection call at most
PROJECTION_SLAB = 128                  # S4B_PROJECTION_SLAB: rows per slab of the moments' fold
SPREAD_INFO = ("route", "rows_per_chunk", "chunks", "launches", "device_bytes", "draws", "thresholds", "zero_slabs")
SPREAD_THRESHOLDS_MAX = 64             # S4B_SPREAD_THRESHOLDS_MAX: thresholds of one s4b_predict_spread call at most
SPREAD_SLAB = 128                      # S4B_SPREAD_SLAB: rows per slab of the moments' and the bins' fold
SPREAD_BIN_INDEX = {"auto": 0, "compare": 1, "search": 2}
CHECK_INFO = SPREAD_INFO               # (s4b_check_out.info has s4b_spread_out.info's layout)
CURVES_INFO = QUANTILE_INFO[:7] + ("device_bytes", "largest_affected", "total_affected")          # (the last two share info[7], as in PD_INFO)
CURVES_OUTPUTS = ("mean", "m2", "quantiles", "p_max", "p_min", "range_mean", "range_m2", "range_quantiles")
CURVES_SCRATCH_MAX = 1 << 30           # S4B_CURVES_SCRATCH_MAX: the curves of 64 rows (8 x 64 x pooled draws x grid points) at most
DESCRIBE_INFO = ("route", "rows_per_chunk", "chunks", "launches", "device_bytes", "draws", "rows_per_sort", "padded_draws", "sort_lds_bytes")
DESCRIBE_OUTPUTS = ("quantiles", "median", "hdi", "hdi_start", "n_above", "n_below", "mad")
DESCRIBE_HDI_MAX = 8                   # S4B_DESCRIBE_HDI_MAX: window counts of one s4b_predict_describe call at most
DESCRIBE_THRESHOLDS_MAX = 32           # S4B_DESCRIBE_THRESHOLDS_MAX: thresholds of one s4b_predict_describe call at most
SORTED_INFO = ("route", "draws_per_block", "blocks", "launches", "device_bytes", "draws", "targets", "passes")
SORTED_OUTPUTS = ("mean", "m2", "quantiles", "draws", "n_above", "n_below")
SORTED_PROBS_MAX = 12                  # S4B_SORTED_PROBS_MAX: row probs of one s4b_predict_sorted call at most
SORTED_CUTS_MAX = 8                    # S4B_SORTED_CUTS_MAX: cut ranks of one s4b_predict_sorted call at most
PPD_INFO = QUANTILE_INFO               # (s4b_ppd_out.info has s4b_quantile_out.info's layout; rows_per_sort: rows per workgroup of k_ppd_rows)
LOO_INFO = QUANTILE_INFO               # (s4b_loo_out.info likewise; rows_per_sort: rows per workgroup of k_loo_rows)
LOO_OUTPUTS = ("elpd_loo", "pareto_k", "lpd", "ess")
CONV_INFO = QUANTILE_INFO              # (s4b_conv_out.info likewise; rows_per_sort: rows per workgroup of k_chain_rows)
CONV_OUTPUTS = ("rhat", "ess", "mean", "mcse", "n_pairs")
CONV_QUANTITIES = {"ev": 0, "lik": 1}
PD_GRID_MAX = 64                       # grid points per s4b_partial_dependence call


def _peer_tables(peers, draws, given, cols, what):
    """One C-ordered [peer's draws x cols] table per peer of a pooled call, as an array of pointers: (the array or None, the tables it points into).
    `draws(sampler)` is the peer's kept draw count."""
    if not cols or not peers or given is None:          # (tables missing though needed: the library refuses the call)
        return None, []
    if len(given) != len(peers):
        raise ValueError(f"{what} must hold one table per peer ({len(peers)})")
    held = []
    for x, (t, smp) in enumerate(zip(given, peers)):
        t = np.asarray(t)
        if t.shape != (draws(smp), cols):
            raise ValueError(f"{what}[{x}] must be [{draws(smp)} x {cols}], not shape {t.shape}")
        held.append(_f64(t, "C"))
    return (c_double_p * len(held))(*[_dp(t) for t in held]), held


def _dp(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(c_double_p)


def _ip(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(c_int32_p)


def _f64(a, order="F") -> np.ndarray:
    return np.require(np.asarray(a, dtype=np.float64), requirements=["A", "O"] + (["F"] if order == "F" else ["C"]))


def _i32(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.int32))


def ceil_fraction(fraction, count: int):
    """(the exact fraction, ceil(fraction x count)) in rational arithmetic on the decimal text of ``fraction``: in floating point 0.07 x 100 is
    7.000000000000001 and would give 8.  Shared by ``Stan4bartFit.hdi_draws`` and ``fraction_count``."""
    f = Fraction(repr(float(fraction)))
    return f, math.ceil(f * int(count))


def fraction_count(fraction, count: int) -> int:
    """The members m = ceil(fraction x count) of the top or bottom group of ``count`` rows for ``predict_sorted``, by ``ceil_fraction``: it needs
    0 < fraction < 1 and m < count."""
    f, m = ceil_fraction(fraction, count)
    if not 0 < f < 1:
        raise ValueError(f"a fraction of the rows must lie in (0, 1), not {fraction!r}")
    if not m < int(count):
        raise ValueError(f"the fraction {fraction!r} of {count} rows is all of them ({m}): the group must leave a row outside")
    return m


LATENT_MODES = {"exact": 0, "parallel": 1}      # bart_args latents -> s4b_set_latent_mode

def set_host_vector(lib, prefix: str, on: Optional[bool]) -> bool:
    """Process-wide: the host loops of a leapfrog in their AVX2 form (on) or their scalar form; both give the same bits.
    Returns what is in force (False on a CPU without AVX2 whatever was asked).  on = None changes nothing and only reports."""
    fn = getattr(lib, prefix + "set_host_vector")
    fn.restype, fn.argtypes = C.c_int, [C.c_int32, c_int32_p]
    eff = C.c_int32()
    if fn(-1 if on is None else int(bool(on)), C.byref(eff)) != 0:
        raise RuntimeError(getattr(lib, prefix + "last_error")().decode())
    return bool(eff.value)


@dataclass
class SamplerArgs:
    """The six argument objects of ``stan4bart_create`` (reference R/stan4bart_fit.R:42) as numpy/python."""
    # bart data / control / model
    x_bart: np.ndarray                      # n x p
    n_trees: int = 75
    n_cuts: int | Sequence[int] = 100
    n_thin: int = 1
    x_test: Optional[np.ndarray] = None
    base: float = 0.95
    power: float = 2.0
    k: float = 2.0
    node_scale: Optional[float] = None      # default 0.5 continuous / 3.0 binary
    keep_trees: bool = False
    node_capacity: int = 0
    proposal_probs: Sequence[float] = (0.5, 0.1, 0.4, 0.5)
    split_probs: Optional[Sequence[float]] = None     # cgm(split.probs): one positive weight per BART predictor, or None (uniform)
    use_quantiles: bool = False                       # dbartsControl(useQuantiles): cut points from the distinct values
    k_hyper: Optional[tuple] = None                   # normal(k = chi(degreesOfFreedom, scale)): (df, scale) -> k is sampled; `k` is where it starts
    latents: str = "exact"                            # probit latents: "exact" (R's stream, the reference's chain) or "parallel" (s4b_set_latent_mode 1)
    # stan data
    X: Optional[np.ndarray] = None          # n x K (already centred)
    y: Optional[np.ndarray] = None
    weights: Optional[np.ndarray] = None
    is_binary: bool = False
    prior_dist: int = 1
    prior_dist_for_aux: int = 3
    prior_scale: Optional[np.ndarray] = None
    prior_mean: Optional[np.ndarray] = None
    prior_df: Optional[np.ndarray] = None
    prior_scale_for_aux: float = 1.0
    prior_mean_for_aux: float = 0.0
    prior_df_for_aux: float = 1.0
    global_prior_df: float = 1.0            # hs / hs_plus
    global_prior_scale: float = 0.01
    slab_df: float = 4.0
    slab_scale: float = 2.5
    num_normals: Optional[Sequence[int]] = None   # product_normal
    p: Sequence[int] = ()
    l: Sequence[int] = ()
    shape: Sequence[float] = ()
    scale: Sequence[float] = ()
    concentration: Sequence[float] = ()
    regularization: Sequence[float] = ()
    w: Optional[np.ndarray] = None
    v: Optional[np.ndarray] = None
    u: Optional[np.ndarray] = None
    # stan control
    seed: int = 0
    skip: int = 1
    init_r: float = 2.0
    adapt_gamma: float = 0.05
    adapt_delta: float = 0.8
    adapt_kappa: float = 0.75
    adapt_t0: float = 10.0
    adapt_init_buffer: int = 75
    adapt_term_buffer: int = 50
    adapt_window: int = 25
    stepsize: float = 1.0
    stepsize_jitter: float = 0.0
    max_treedepth: int = 10
    hmc_mode: int = 0
    # common control
    warmup: int = 1000
    iter: int = 2000
    verbose: int = 0
    refresh: int = 0
    offset: Optional[np.ndarray] = None
    offset_type: int = 0
    bart_offset_init: Optional[np.ndarray] = None
    sigma_init: float = 1.0
    keep_fits: bool = True
    callback: Optional[Callable] = None
    device: int = 0
    extras: dict = field(default_factory=dict)


class Sampler:
    """One chain: wraps ``<prefix>create / run / disengage_adaptation / ... / free``."""

    def __init__(self, lib: C.CDLL, prefix: str, args: SamplerArgs, r_rng_state: np.ndarray):
        self._lib, self._pfx = lib, prefix
        self._bind()
        a = args
        self._keep = []  # keep numpy buffers alive for the duration of create()

        def keep(x):
            self._keep.append(x)
            return x

        xb = keep(_f64(a.x_bart))
        n, p = xb.shape
        ncuts = keep(_i32(np.broadcast_to(np.asarray(a.n_cuts), (p,))))
        xt = keep(_f64(a.x_test)) if a.x_test is not None and len(a.x_test) else None
        bd = BartData(n=n, p=p, reserved=0, x=_dp(xb), n_cuts=_ip(ncuts),
                      n_test=0 if xt is None else xt.shape[0], x_test=_dp(xt))
        ns = a.node_scale if a.node_scale is not None else (3.0 if a.is_binary else 0.5)
        pp = a.proposal_probs
        bc = BartControl(n_trees=a.n_trees, n_thin=a.n_thin, keep_trees=int(a.keep_trees),
                         node_capacity=a.node_capacity, base=a.base, power=a.power, k=a.k, node_scale=ns,
                         birth_or_death_prob=pp[0], swap_prob=pp[1], change_prob=pp[2], birth_prob=pp[3],
                         use_quantiles=int(bool(a.use_quantiles)), interface_version=INTERFACE_VERSION,
                         k_hyper_df=0.0 if a.k_hyper is None else float(a.k_hyper[0]),
                         k_hyper_scale=float("inf") if a.k_hyper is None else float(a.k_hyper[1]))
        self.k_modeled = a.k_hyper is not None
        if a.split_probs is not None:
            sp = keep(_f64(np.asarray(a.split_probs, dtype=np.float64)))
            if sp.shape != (xb.shape[1],):
                raise ValueError("split_probs needs one weight per BART predictor")
            bc.split_probs = _dp(sp)

        X = keep(_f64(a.X if a.X is not None else np.zeros((n, 0))))
        if X.ndim == 1:
            X = keep(_f64(X.reshape(n, 1)))
        K = X.shape[1]
        y = keep(_f64(a.y))
        t = len(a.p)
        q = int(sum(int(pi) * int(li) for pi, li in zip(a.p, a.l)))
        len_theta_L = int(sum(pi * (pi - 1) // 2 + pi for pi in a.p))
        ps = keep(_f64(a.prior_scale if a.prior_scale is not None else np.ones(K)))
        pm = keep(_f64(a.prior_mean if a.prior_mean is not None else np.zeros(K)))
        pdf = keep(_f64(a.prior_df if a.prior_df is not None else np.ones(K)))
        wts = keep(_f64(a.weights)) if a.weights is not None and len(a.weights) else None
        p_arr, l_arr = keep(_i32(a.p)), keep(_i32(a.l))
        shape, scale = keep(_f64(a.shape)), keep(_f64(a.scale))
        conc, reg = keep(_f64(a.concentration)), keep(_f64(a.regularization))
        w = keep(_f64(a.w if a.w is not None else np.zeros(0)))
        v = keep(_i32(a.v if a.v is not None else np.zeros(0)))
        u = keep(_i32(a.u if a.u is not None else np.zeros(n + 1)))
        sd = StanData(N=n, K=K, is_binary=int(a.is_binary), has_intercept=0, has_weights=int(wts is not None),
                      prior_dist=a.prior_dist, prior_dist_for_aux=a.prior_dist_for_aux,
                      X=_dp(X), y=_dp(y), weights=_dp(wts), prior_scale=_dp(ps), prior_mean=_dp(pm), prior_df=_dp(pdf),
                      prior_scale_for_aux=a.prior_scale_for_aux, prior_mean_for_aux=a.prior_mean_for_aux,
                      prior_df_for_aux=a.prior_df_for_aux, t=t, q=q, len_theta_L=len_theta_L,
                      len_concentration=len(conc), len_regularization=len(reg), reserved=0,
                      p=_ip(p_arr), l=_ip(l_arr), shape=_dp(shape), scale=_dp(scale),
                      concentration=_dp(conc), regularization=_dp(reg), num_non_zero=len(w),
                      w=_dp(w), v=_ip(v), u=_ip(u),
                      global_prior_df=a.global_prior_df, global_prior_scale=a.global_prior_scale, slab_df=a.slab_df,
                      slab_scale=a.slab_scale,
                      num_normals=_ip(keep(_i32(a.num_normals))) if a.num_normals is not None else None)
        sc = StanControl(seed=a.seed & 0xFFFFFFFF, skip=a.skip, init_r=a.init_r, adapt_gamma=a.adapt_gamma,
                         adapt_delta=a.adapt_delta, adapt_kappa=a.adapt_kappa, adapt_t0=a.adapt_t0,
                         adapt_init_buffer=a.adapt_init_buffer, adapt_term_buffer=a.adapt_term_buffer,
                         adapt_window=a.adapt_window, reserved=0, stepsize=a.stepsize,
                         stepsize_jitter=a.stepsize_jitter, max_treedepth=a.max_treedepth, hmc_mode=a.hmc_mode)
        off = keep(_f64(a.offset)) if a.offset is not None and len(a.offset) else None
        boi = keep(_f64(a.bart_offset_init)) if a.bart_offset_init is not None else None
        self._py_callback = a.callback
        self._cb = CALLBACK(self._trampoline) if a.callback is not None else CALLBACK()
        cc = CommonControl(warmup=a.warmup, iter=a.iter, verbose=a.verbose, refresh=a.refresh,
                           is_binary=int(a.is_binary), offset_type=a.offset_type, keep_fits=int(a.keep_fits),
                           device=a.device, offset=_dp(off), bart_offset_init=_dp(boi), sigma_init=a.sigma_init,
                           callback=self._cb, callback_user=None)
        st = np.ascontiguousarray(r_rng_state, dtype=np.uint32)
        assert st.shape == (625,)
        self._h = C.c_void_p()
        rc = self._f("create")(C.byref(bc), C.byref(bd), C.byref(sd), C.byref(sc), C.byref(cc),
                               st.ctypes.data_as(c_uint32_p), C.byref(self._h))
        self._check(rc)
        self._keep.clear()
        if a.latents not in LATENT_MODES:
            self.free()
            raise ValueError(f"latents must be one of {sorted(LATENT_MODES)}, not {a.latents!r}")
        if a.latents != "exact":
            try:
                self.set_latent_mode(LATENT_MODES[a.latents])
            except Exception:
                self.free()
                raise
        dims = (C.c_int64 * 5)()
        self._check(self._f("get_dims")(self._h, dims))
        self.num_pars, self.n, self.n_test, self.p, self.n_trees = (int(d) for d in dims)
        self.keep_fits = bool(a.keep_fits)
        self.K, self.q = int(K), int(q)
        self.callback_results: list = []
        self._pending_exc = None

    # ------------------------------------------------------------------ plumbing
    def _bind(self):
        """restype + argtypes of every entry point of include/stan4bart_amd.h (64-bit counts travel as c_int64)."""
        vp, i32, i64, dp, ip, up = C.c_void_p, C.c_int32, C.c_int64, c_double_p, c_int32_p, c_uint32_p
        sig = {
            "create": [C.POINTER(BartControl), C.POINTER(BartData), C.POINTER(StanData), C.POINTER(StanControl),
                       C.POINTER(CommonControl), up, C.POINTER(vp)],
            "run": [vp, i32, i32, i32, C.POINTER(Results)],
            "disengage_adaptation": [vp], "print_initial_summary": [vp],
            "get_parametric_mean": [vp, dp], "get_bart_data_range": [vp, dp],
            "get_r_rng_state": [vp, up], "set_r_rng_state": [vp, up],
            "get_dims": [vp, C.POINTER(i64)], "get_stan_par_names": [vp, C.c_char_p, C.c_size_t],
            "get_trees": [vp, i64, ip, ip, ip, ip, dp, C.POINTER(i64)],
            "get_kept_trees": [vp, i64, i64, ip, ip, ip, ip, ip, dp, C.POINTER(i64)],
            "get_kept_trees_indexed": [vp, ip, i64, ip, i64, i64, ip, ip, ip, ip, ip, dp, C.POINTER(i64)],
            "export_bart_state": [vp, vp, i64, C.POINTER(i64)],
            "create_stored_bart_sampler": [vp, i64, i32, C.POINTER(vp)],
            "predict_bart": [vp, dp, i64, dp, C.POINTER(i64)],
            "predict_bart_offset": [vp, dp, i64, dp, dp, C.POINTER(i64)], "print_trees": [vp, ip, i64, ip, i64],
            "get_state": [vp, vp, i64, C.POINTER(i64)], "set_state": [vp, vp, i64],
            "set_trace": [vp, i32], "get_trace": [vp, i64, ip, C.POINTER(i64)],
            "get_leaf_assignment": [vp, i32, ip], "get_counters": [vp, C.POINTER(i64)], "get_nuts_stats": [vp, dp],
            "set_nuts_helpers": [vp, i32], "get_nuts_runahead": [vp, C.POINTER(i64)],
            "profile_sweep": [vp, i32, dp], "profile_leapfrog": [vp, i32, dp],
            "set_progress": [vp, PROGRESS, vp], "set_device_sharing": [vp, i32],
            "set_tree_path": [vp, i32], "get_tree_path": [vp, ip], "get_fused_stats": [vp, C.POINTER(i64)], "get_sweep_stats": [vp, C.POINTER(i64)], "get_sweep_busy": [vp, C.POINTER(i64)], "get_sweep_spec": [vp, C.POINTER(i64)], "set_test_hook": [vp, i32, i64], "set_hmc_mode": [vp, i32], "get_hmc_mode": [vp, ip],
            "predict_summary": [vp, C.POINTER(SummaryIn), C.POINTER(SummaryOut)],
            "partial_dependence": [vp, C.POINTER(PdIn), C.POINTER(PdOut)],
            "predict_quantiles": [vp, C.POINTER(QuantileIn), C.POINTER(QuantileOut)],
            "predict_contrast": [vp, C.POINTER(ContrastIn), C.POINTER(ContrastOut)],
            "predict_groups": [vp, C.POINTER(GroupsIn), C.POINTER(GroupsOut)],
            "predict_projection": [vp, C.POINTER(ProjectionIn), C.POINTER(ProjectionOut)],
            "predict_spread": [vp, C.POINTER(SpreadIn), C.POINTER(SpreadOut)],
            "predict_check": [vp, C.POINTER(CheckIn), C.POINTER(CheckOut)],
            "predict_curves": [vp, C.POINTER(CurvesIn), C.POINTER(CurvesOut)],
            "predict_describe": [vp, C.POINTER(DescribeIn), C.POINTER(DescribeOut)],
            "predict_sorted": [vp, C.POINTER(SortedIn), C.POINTER(SortedOut)],
            "predict_ppd": [vp, C.POINTER(PpdIn), C.POINTER(PpdOut)],
            "predict_loo": [vp, C.POINTER(LooIn), C.POINTER(LooOut)],
            "predict_convergence": [vp, C.POINTER(ConvIn), C.POINTER(ConvOut)],
            "set_latent_mode": [vp, i32], "get_latent_mode": [vp, ip], "test_draw_latents": [vp], "test_hand_off": [vp, dp, dp, C.c_double, i32],
            "test_stan_sums": [vp, i32, dp, dp, ip, dp, C.POINTER(i64)],
            "test_sorted_select": [vp, dp, i64, i64, i64, i32, ip, dp, i32, ip, ip, ip, C.POINTER(i64)],
        }
        for name, argtypes in sig.items():
            fn = getattr(self._lib, self._pfx + name, None)
            if fn is None:          # optional entry points (the oracle exports the subset the tests drive)
                continue
            fn.restype = C.c_int
            fn.argtypes = argtypes
        getattr(self._lib, self._pfx + "last_error").restype = C.c_char_p
        getattr(self._lib, self._pfx + "last_error").argtypes = []
        getattr(self._lib, self._pfx + "free").restype = None
        getattr(self._lib, self._pfx + "free").argtypes = [vp]

    def _f(self, name):
        return getattr(self._lib, self._pfx + name)

    def _check(self, rc):
        if rc != 0:
            raise RuntimeError(self._f("last_error")().decode())

    def _trampoline(self, user, yhat_train, yhat_test, stan_pars, num_pars):
        tr = np.ctypeslib.as_array(yhat_train, shape=(self.n,)).copy()
        te = np.ctypeslib.as_array(yhat_test, shape=(self.n_test,)).copy() if self.n_test else None
        sp = np.ctypeslib.as_array(stan_pars, shape=(num_pars,)).copy()
        try:
            self.callback_results.append(self._py_callback(tr, te, sp))
        except BaseException as e:       # ctypes would swallow it: remember it, stop the run (non-zero return), re-raise after
            if self._pending_exc is None:
                self._pending_exc = e
            return 1
        return 0

    # ------------------------------------------------------------------ the .Call surface
    def run(self, num_iter: int, is_warmup: bool, results_type: int = 0) -> dict:
        """``stan4bart_run``: returns dict(stan=[num_pars x S], bart=dict(sigma, train, test, varcount))."""
        S = num_iter if self.keep_fits else 1
        stan = np.zeros((self.num_pars, S), order="F")
        sigma = np.zeros(S)
        train = np.zeros((self.n, S), order="F")
        test = np.zeros((self.n_test, S), order="F")
        varcount = np.zeros((self.p, S), dtype=np.int32, order="F")
        kdraws = np.zeros(S)
        res = Results(stan=_dp(stan), bart_sigma=_dp(sigma), bart_train=_dp(train),
                      bart_test=_dp(test) if self.n_test else None, bart_varcount=_ip(varcount),
                      bart_k=_dp(kdraws) if getattr(self, "k_modeled", False) else None)
        self.callback_results = []
        self._pending_exc = None
        rc = self._f("run")(self._h, num_iter, int(is_warmup), results_type, C.byref(res))
        if self._pending_exc is not None:           # an exception inside the per-iteration callback or the progress hook
            e, self._pending_exc = self._pending_exc, None
            raise e
        self._check(rc)
        out = {}
        if results_type in (0, 2):
            out["stan"] = stan
        if results_type in (0, 1):
            out["bart"] = dict(sigma=sigma, train=train, test=test, varcount=varcount)
            if getattr(self, "k_modeled", False):        # the reference's fifth result element (src/bart_util.cpp:17-26,75-76): only when k is modeled
                out["bart"]["k"] = kdraws
        if self._py_callback is not None:
            out["callback"] = list(self.callback_results)
        return out

    def disengage_adaptation(self):
        self._check(self._f("disengage_adaptation")(self._h))

    def print_initial_summary(self):
        self._check(self._f("print_initial_summary")(self._h))

    def get_parametric_mean(self) -> np.ndarray:
        out = np.zeros(self.n)
        self._check(self._f("get_parametric_mean")(self._h, _dp(out)))
        return out

    def get_bart_data_range(self) -> np.ndarray:
        out = np.zeros(2)
        self._check(self._f("get_bart_data_range")(self._h, _dp(out)))
        return out

    def get_r_rng_state(self) -> np.ndarray:
        st = np.zeros(625, dtype=np.uint32)
        self._check(self._f("get_r_rng_state")(self._h, st.ctypes.data_as(c_uint32_p)))
        return st

    def set_r_rng_state(self, st: np.ndarray):
        st = np.ascontiguousarray(st, dtype=np.uint32)
        self._check(self._f("set_r_rng_state")(self._h, st.ctypes.data_as(c_uint32_p)))

    def stan_par_names(self) -> list[str]:
        buf = C.create_string_buffer(64 * (self.num_pars + 8))
        self._check(self._f("get_stan_par_names")(self._h, buf, len(buf)))
        return buf.value.decode().split("\n")

    def get_trees(self) -> dict:
        """Flattened live trees (``stan4bart_getTrees(current = TRUE)`` layout)."""
        nn = C.c_int64()
        self._check(self._f("get_trees")(self._h, 0, None, None, None, None, None, C.byref(nn)))
        m = nn.value
        tree, nobs, var, split = (np.zeros(m, dtype=np.int32) for _ in range(4))
        value = np.zeros(m)
        self._check(self._f("get_trees")(self._h, m, _ip(tree), _ip(nobs), _ip(var), _ip(split), _dp(value), C.byref(nn)))
        return dict(tree=tree, n=nobs, var=var, split=split, value=value)

    def get_kept_trees(self, sample: int = -1) -> dict:
        """Flattened trees of the kept draws (``stan4bart_getTrees(current = FALSE)``; ``sample`` 0-based, -1 = all)."""
        nn = C.c_int64()
        self._check(self._f("get_kept_trees")(self._h, C.c_int64(sample), 0, None, None, None, None, None, None, C.byref(nn)))
        m = nn.value
        smp, tree, nobs, var, split = (np.zeros(m, dtype=np.int32) for _ in range(5))
        value = np.zeros(m)
        self._check(self._f("get_kept_trees")(self._h, C.c_int64(sample), m, _ip(smp), _ip(tree), _ip(nobs), _ip(var), _ip(split), _dp(value),
                                              C.byref(nn)))
        return dict(sample=smp, tree=tree, n=nobs, var=var, split=split, value=value)

    def get_kept_trees_indexed(self, sample_idx=None, tree_idx=None) -> dict:
        """``stan4bart_getTrees(sampleIndices, treeIndices)``: 0-based index vectors (None = all, in order)."""
        if not hasattr(self._lib, self._pfx + "get_kept_trees_indexed"):      # (the oracle exports the scalar form only)
            parts = [self.get_kept_trees(-1)] if sample_idx is None else [self.get_kept_trees(int(k)) for k in sample_idx]
            out = {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}
            if tree_idx is not None:
                order = np.concatenate([np.flatnonzero((out["sample"] == sm) & (out["tree"] == t)) for sm in (np.unique(out["sample"]) if sample_idx is None else sample_idx) for t in tree_idx] or [np.zeros(0, dtype=np.int64)])
                out = {k: v[order.astype(np.int64)] for k, v in out.items()}
            return out
        si = None if sample_idx is None else _i32(sample_idx)
        ti = None if tree_idx is None else _i32(tree_idx)
        args = (_ip(si), 0 if si is None else len(si), _ip(ti), 0 if ti is None else len(ti))
        nn = C.c_int64()
        self._check(self._f("get_kept_trees_indexed")(self._h, *args, 0, None, None, None, None, None, None, C.byref(nn)))
        m = nn.value
        smp, tree, nobs, var, split = (np.zeros(m, dtype=np.int32) for _ in range(5))
        value = np.zeros(m)
        self._check(self._f("get_kept_trees_indexed")(self._h, *args, m, _ip(smp), _ip(tree), _ip(nobs), _ip(var), _ip(split), _dp(value), C.byref(nn)))
        return dict(sample=smp, tree=tree, n=nobs, var=var, split=split, value=value)

    def print_trees(self, sample_idx=None, tree_idx=None):
        si = None if sample_idx is None else _i32(sample_idx)
        ti = None if tree_idx is None else _i32(tree_idx)
        self._check(self._f("print_trees")(self._h, _ip(si), 0 if si is None else len(si), _ip(ti), 0 if ti is None else len(ti)))

    def set_progress(self, fn):
        """``fn(iter, num_iter, is_warmup) -> bool`` (True cancels the run), or None."""
        self._progress_py = fn

        def hook(user, it, n, w):
            try:
                return int(bool(fn(it, n, bool(w))))
            except BaseException as e:   # cancel the run (non-zero) and re-raise once s4b_run has returned
                if self._pending_exc is None:
                    self._pending_exc = e
                return 1
        self._progress_c = PROGRESS(hook) if fn is not None else PROGRESS()
        self._check(self._f("set_progress")(self._h, self._progress_c, None))

    def set_device_sharing(self, chains: int):
        """Hint: ``chains`` samplers share this sampler's GPU (three or more: the tree update that leaves room for the others)."""
        fn = getattr(self._lib, self._pfx + "set_device_sharing", None)
        if fn is not None:          # (the CPU oracle has no such notion)
            self._check(fn(self._h, int(chains)))

    TREE_PATHS = {"auto": 0, "two-kernel": 1, "fused": 2, "persistent": 4, "stream": 5}

    def set_tree_path(self, path):
        """Device code of a tree update: "auto", "two-kernel" (k_tree + k_control), "fused" (k_step), "persistent" (k_sweep: one
        launch per sweep, the residual in registers) or "stream" (k_sweep_stream: the same launch with a streaming pass; on request
        only — it is slower than the other paths at every size)."""
        fn = getattr(self._lib, self._pfx + "set_tree_path", None)
        if fn is not None:          # (the CPU oracle has one path)
            self._check(fn(self._h, int(self.TREE_PATHS.get(path, path))))

    def get_tree_path(self):
        """(requested, in effect) as names."""
        fn = getattr(self._lib, self._pfx + "get_tree_path", None)
        if fn is None:
            return ("auto", "oracle")
        out = np.zeros(2, dtype=np.int32)
        self._check(fn(self._h, _ip(out)))
        names = {v: k for k, v in self.TREE_PATHS.items()}
        return (names[int(out[0])], names[int(out[1])])

    def set_hmc_mode(self, mode: int):
        self._check(self._f("set_hmc_mode")(self._h, int(mode)))

    def get_hmc_mode(self) -> int:
        fn = getattr(self._lib, self._pfx + "get_hmc_mode", None)
        if fn is None:
            return 1          # (the oracle evaluates the likelihood per leapfrog, like the reference)
        out = np.zeros(1, dtype=np.int32)
        self._check(fn(self._h, _ip(out)))
        return int(out[0])

    def set_latent_mode(self, mode: int):
        """How the probit latents are drawn: 0 exact (R's stream), 1 parallel (Philox, one thread per observation); before the first run."""
        fn = getattr(self._lib, self._pfx + "set_latent_mode", None)
        if fn is None:
            raise RuntimeError(f"this library ({self._pfx}*) has no set_latent_mode: it draws the probit latents from R's stream only")
        self._check(fn(self._h, int(mode)))

    def get_latent_mode(self) -> int:
        fn = getattr(self._lib, self._pfx + "get_latent_mode", None)
        if fn is None:
            return 0
        out = np.zeros(1, dtype=np.int32)
        self._check(fn(self._h, _ip(out)))
        return int(out[0])

    def get_fused_stats(self):
        """(evaluations of the fused O(N) Stan sums, evaluations repeated in plain doubles after a failed range check)"""
        out = (C.c_int64 * 2)()
        fn = getattr(self._lib, self._pfx + "get_fused_stats", None)
        if fn is not None:
            self._check(fn(self._h, out))
        return int(out[0]), int(out[1])

    def get_sweep_stats(self):
        """(sweeps run by the persistent kernel, of which handed over to k_step part-way) since creation."""
        fn = getattr(self._lib, self._pfx + "get_sweep_stats", None)
        if fn is None:
            return (0, 0)
        out = (C.c_int64 * 2)()
        self._check(fn(self._h, out))
        return (int(out[0]), int(out[1]))

    def get_sweep_spec(self):
        """(persistent launches that ran, tree updates decided inside them, steps published before their verdict, steps borne out) since creation."""
        fn = getattr(self._lib, self._pfx + "get_sweep_spec", None)
        if fn is None:
            return (0, 0, 0, 0)
        out = (C.c_int64 * 4)()
        self._check(fn(self._h, out))
        return tuple(int(v) for v in out)

    def set_test_hook(self, hook: int, value: int):
        """TEST HOOK (include/stan4bart_amd.h): hook 1, value k — every k-th persistent launch reports a busy device (0 = off)."""
        self._check(self._f("set_test_hook")(self._h, int(hook), int(value)))

    def test_draw_latents(self):
        """TEST ENTRY (include/stan4bart_amd.h): one draw of the probit latents from the current state (``set_state`` before, ``get_state``
        after), nothing else of a sweep: the exact draw in latent mode 0, the parallel draw (key and draw index of the state's tail) in mode 1."""
        self._check(self._f("test_draw_latents")(self._h))

    def test_hand_off(self, beta, b, sigma: float, update_scale: bool):
        """TEST ENTRY (include/stan4bart_amd.h): the Stan -> BART hand-off of one iteration for the given coefficients (BART's offset by the sampler's
        offset type, sigma, the rescaling with or without a new response scale) and nothing else; Stan's position and both generators stay."""
        beta, b = _f64(np.atleast_1d(beta)), _f64(np.atleast_1d(b))
        self._check(self._f("test_hand_off")(self._h, _dp(beta) if beta.size else None, _dp(b) if b.size else None, float(sigma), int(bool(update_scale))))

    STAN_SUMS_INFO = 18

    def test_stan_sums(self, mode: int, beta=None, b=None, set_exp=None):
        """TEST ENTRY (include/stan4bart_amd.h): one evaluation of the Stan block's O(N) sums.  ``mode`` -1: one leapfrog's evaluation with ``beta``,
        ``b`` (non-finite values allowed); 0..3: one Gibbs iteration's evaluation with that Stan-offset mode.  ``set_exp``: None or the three binary
        exponents of the fixed-point scales for this launch.  Returns (sums [1 + K + q]: ss, X'e, Z'e; info: dict of what the host's checks saw)."""
        K, q = self.K, self.q
        beta = _f64(np.zeros(K) if beta is None else np.atleast_1d(beta))
        b = _f64(np.zeros(q) if b is None else np.atleast_1d(b))
        if beta.size != K or b.size != q:
            raise ValueError(f"test_stan_sums: beta needs {K} entries and b {q}")
        ex = None if set_exp is None else np.ascontiguousarray(set_exp, dtype=np.int32)
        if ex is not None and ex.shape != (3,):
            raise ValueError("test_stan_sums: set_exp holds three exponents")
        sums = np.zeros(1 + K + q)
        info = (C.c_int64 * Sampler.STAN_SUMS_INFO)()
        self._check(self._f("test_stan_sums")(self._h, int(mode), _dp(beta) if K else None, _dp(b) if q else None, _ip(ex) if ex is not None else None, _dp(sums), info))
        v = [int(x) for x in info]
        return sums, dict(accepted=bool(v[0]), reject=v[1], exp_used=tuple(v[2:5]), exp_after=tuple(v[5:8]), mag=tuple(v[8:11]), exw=tuple(v[11:14]),
                          grid=v[14], fused=bool(v[15]), evals=v[16], fallbacks=v[17])

    def get_sweep_busy(self) -> int:
        """Persistent launches that found the device shared (roll call failed; their sweeps ran as k_step launches) since creation."""
        fn = getattr(self._lib, self._pfx + "get_sweep_busy", None)
        if fn is None:
            return 0
        out = C.c_int64(0)
        self._check(fn(self._h, C.byref(out)))
        return int(out.value)

    def set_trace(self, enable: bool):
        self._check(self._f("set_trace")(self._h, int(enable)))

    def get_trace(self, cap: int = 1 << 20) -> np.ndarray:
        nn = C.c_int64()
        out = np.zeros((cap, 5), dtype=np.int32)
        self._check(self._f("get_trace")(self._h, cap, _ip(out), C.byref(nn)))
        return out[: nn.value].copy()

    def get_leaf_assignment(self, tree: int) -> np.ndarray:
        out = np.zeros(self.n, dtype=np.int32)
        self._check(self._f("get_leaf_assignment")(self._h, tree, _ip(out)))
        return out

    def get_counters(self) -> np.ndarray:
        out = (C.c_int64 * 3)()
        self._check(self._f("get_counters")(self._h, out))
        return np.array(list(out), dtype=np.int64)

    def get_nuts_stats(self) -> dict:
        """Totals over all NUTS transitions since creation."""
        out = (C.c_double * 4)()
        self._check(self._f("get_nuts_stats")(self._h, out))
        return dict(transitions=int(out[0]), sum_treedepth=int(out[1]), sum_n_leapfrog=int(out[2]), divergent=int(out[3]))

    def set_nuts_helpers(self, n: int, wait: bool = False) -> None:
        """Run-ahead helper threads of the NUTS transition: 0 none, 1 the backward direction, 2 both (never called and S4B_NUTS_HELPERS unset: 1, and 2 where
        the process has the cores for it).  Same chain either way.
        wait (a test hook, not for use): the sampler's thread waits for a state its helper has not finished instead of computing it itself."""
        self._check(self._f("set_nuts_helpers")(self._h, int(n) | (16 if wait and n else 0)))

    def get_nuts_runahead(self) -> dict:
        """Run-ahead counters since creation."""
        out = (C.c_int64 * 4)()
        self._check(self._f("get_nuts_runahead")(self._h, out))
        return dict(taken=int(out[0]), not_ready=int(out[1]), unconsumed=int(out[2]), transitions_without_helper=int(out[3]))

    def predict_bart(self, x_test: np.ndarray, offset_test: Optional[np.ndarray] = None) -> np.ndarray:
        """``stan4bart_predictBART(x_test, offset_test)``: BART fit of every kept draw (keep_trees) at new rows, [n_test x samples]."""
        xt = _f64(x_test)
        ns = C.c_int64()
        self._check(self._f("predict_bart")(self._h, _dp(xt), xt.shape[0], None, C.byref(ns)))
        out = np.zeros((xt.shape[0], ns.value), order="F")
        if ns.value:
            if offset_test is not None:
                off = _f64(offset_test)
                if off.shape != (xt.shape[0],):
                    raise ValueError("length of offset_test must equal number of rows in x_test")
                self._check(self._f("predict_bart_offset")(self._h, _dp(xt), xt.shape[0], _dp(off), _dp(out), C.byref(ns)))
            else:
                self._check(self._f("predict_bart")(self._h, _dp(xt), xt.shape[0], _dp(out), C.byref(ns)))
        return out

    def predict_summary(self, x_test: np.ndarray, offset=None, dense=None, dense_coef=None, ell_index=None, ell_value=None, ell_coef=None,
                        link: int = 0, weights=None, route="auto", stage_nodes: int = 0, max_workgroups: int = 0) -> dict:
        """``s4b_predict_summary``: summaries of the kept draws' predictions at new rows, formed on the device without the [rows x draws] matrix.
        For row i and draw k, z = bart + offset[i] + dense[i] . dense_coef[k] + sum_e ell_value[i, e] * ell_coef[k, ell_index[i, e]] (index -1:
        padding), v = z (link 0) or Phi(z) (link 1).  dense [rows x M], dense_coef [draws x M], ell_index / ell_value [rows x E], ell_coef
        [draws x q], weights [G x rows] with G <= 8.  Returns dict(mean [rows], m2 [rows] = sum_k (v - mean)^2, average [draws x G] = weights @ v,
        draws, info: what the call did, SUMMARY_INFO)."""
        fn = getattr(self._lib, self._pfx + "predict_summary", None)
        if fn is None:
            raise RuntimeError(f"this library ({self._pfx}*) has no predict_summary")
        probe = SummaryOut()
        self._check(fn(self._h, None, C.byref(probe)))
        S = int(probe.num_samples)
        arg, keep, rows, G = self._summary_in(S, x_test, offset, dense, dense_coef, ell_index, ell_value, ell_coef, link, weights, route, stage_nodes,
                                              max_workgroups)
        mean, m2, avg = np.zeros(rows), np.zeros(rows), np.zeros((S, G))
        out = SummaryOut(mean=_dp(mean), m2=_dp(m2), average=_dp(avg) if avg.size else None)
        self.summary_info = dict(zip(SUMMARY_INFO, [0] * 8))
        rc = fn(self._h, C.byref(arg), C.byref(out))
        self.summary_info = dict(zip(SUMMARY_INFO, (int(v) for v in out.info)))          # (all zero after a refusal: nothing was launched)
        self._check(rc)
        return dict(mean=mean, m2=m2, average=avg, draws=int(out.num_samples), info=dict(self.summary_info))

    @staticmethod
    def _summary_in(S, x_test, offset, dense, dense_coef, ell_index, ell_value, ell_coef, link, weights, route, stage_nodes, max_workgroups):
        """The ``s4b_summary_in`` of a call on a sampler with S kept draws: (struct, the arrays it points into, rows, weight vectors)."""
        xt = _f64(x_test)
        if xt.ndim != 2:
            raise ValueError("x_test must be a matrix [rows x predictors]")
        rows = xt.shape[0]

        def table(a, first, what):
            if a is None:
                return None, 0
            a = np.asarray(a)
            if a.ndim != 2 or a.shape[0] != first:
                raise ValueError(f"{what} must have {first} rows, not shape {a.shape}")
            return a, a.shape[1]
        dense, M = table(dense, rows, "dense")
        dense_coef, Mc = table(dense_coef, S, "dense_coef")
        ell_index, E = table(ell_index, rows, "ell_index")
        ell_value, Ev = table(ell_value, rows, "ell_value")
        ell_coef, q = table(ell_coef, S, "ell_coef")
        if M != Mc:
            raise ValueError(f"dense has {M} columns, dense_coef {Mc}")
        if E != Ev:
            raise ValueError(f"ell_index has {E} columns, ell_value {Ev}")
        if weights is not None:
            weights = np.asarray(weights, dtype=np.float64)
            if weights.ndim != 2 or weights.shape[1] != rows:
                raise ValueError(f"weights must be [G x {rows}], not shape {weights.shape}")
        G = 0 if weights is None else weights.shape[0]
        off = None
        if offset is not None:
            off = _f64(offset)
            if off.shape != (rows,):
                raise ValueError("length of offset must equal number of rows in x_test")
        keep = dict(dense=None if not M else _f64(dense), dense_coef=None if not M else _f64(dense_coef, "C"),
                    ell_index=None if not E else np.asfortranarray(np.asarray(ell_index, dtype=np.int32)),
                    ell_value=None if not E else _f64(ell_value), ell_coef=None if not E else _f64(ell_coef, "C"),
                    weights=None if not G else _f64(weights, "C"))
        keep.update(x_test=xt, offset=off)
        arg = SummaryIn(x_test=_dp(xt), n_test=rows, offset=_dp(off), n_dense=M, n_ell=E, n_ell_coef=q if E else 0, link=int(link), n_weights=G,
                        route=int(SUMMARY_ROUTES.get(route, route)), stage_nodes=int(stage_nodes), max_workgroups=int(max_workgroups),
                        dense=_dp(keep["dense"]), dense_coef=_dp(keep["dense_coef"]), ell_index=_ip(keep["ell_index"]),
                        ell_value=_dp(keep["ell_value"]), ell_coef=_dp(keep["ell_coef"]), weights=_dp(keep["weights"]))
        return arg, keep, rows, G

    def partial_dependence(self, x_test: np.ndarray, vars, grid, offset=None, dense=None, dense_coef=None, ell_index=None, ell_value=None,
                           ell_coef=None, link: int = 0, weights=None, route="auto", stage_nodes: int = 0, max_workgroups: int = 0) -> dict:
        """``s4b_partial_dependence``: for every kept draw and every grid point the weighted row sum of the prediction with the BART predictors ``vars``
        (one index or two) set to the grid point's values, in one fused device call.  ``grid`` [G] or [G x len(vars)], G <= 64 (two predictors: the
        pairs of a joint grid, listed by the caller); ``weights`` None (1 / rows: the sample average) or [rows]; the other arguments as
        ``predict_summary`` takes them — the linear parts stay at the rows' own values.  Returns dict(pd [draws x G], draws, info: PD_INFO)."""
        fn = getattr(self._lib, self._pfx + "partial_dependence", None)
        if fn is None:
            raise RuntimeError(f"this library ({self._pfx}*) has no partial_dependence")
        probe = PdOut()
        self._check(fn(self._h, None, C.byref(probe)))
        S = int(probe.num_samples)
        vs = np.atleast_1d(np.asarray(vars, dtype=np.int64))
        if vs.ndim != 1 or len(vs) not in (1, 2):
            raise ValueError(f"vars must be one predictor index or two, not {vars!r}")
        gr = np.asarray(grid, dtype=np.float64)
        if gr.ndim == 1:
            gr = gr[:, None]
        if gr.ndim != 2 or gr.shape[1] != len(vs):
            raise ValueError(f"grid must be [G] or [G x {len(vs)}], not shape {np.shape(grid)}")
        gr = np.asfortranarray(gr)
        if weights is not None:
            weights = np.asarray(weights, dtype=np.float64)
            if weights.ndim == 1:
                weights = weights[None, :]
        rows_in, keep, rows, _ = self._summary_in(S, x_test, offset, dense, dense_coef, ell_index, ell_value, ell_coef, link, weights, route,
                                                   stage_nodes, max_workgroups)
        pd = np.zeros((S, gr.shape[0]))
        arg = PdIn(rows=rows_in, n_vars=len(vs), vars=(C.c_int32 * 2)(int(vs[0]), int(vs[-1]) if len(vs) > 1 else -1), n_grid=gr.shape[0], grid=_dp(gr))
        buf = pd if pd.size else np.zeros(1)          # (no draws or no grid point: refused by the library, which needs a pointer to tell the call from a query)
        out = PdOut(pd=_dp(buf))
        self.pd_info = dict(zip(PD_INFO, [0] * 9))
        rc = fn(self._h, C.byref(arg), C.byref(out))
        w = [int(v) for v in out.info]
        self.pd_info = dict(zip(PD_INFO, w[:7] + [w[7] >> 32, w[7] & 0xFFFFFFFF]))          # (all zero after a refusal: nothing was launched)
        self._check(rc)
        del keep, buf
        return dict(pd=pd, draws=int(out.num_samples), info=dict(self.pd_info))

    def predict_quantiles(self, x_test: np.ndarray, probs, peers=(), peer_dense_coef=None, peer_ell_coef=None, offset=None, dense=None, dense_coef=None,
                          ell_index=None, ell_value=None, ell_coef=None, link: int = 0, route="auto", stage_nodes: int = 0, scratch_bytes: int = 0) -> dict:
        """``s4b_predict_quantiles``: per row the ``probs`` quantiles (R's type 7, numpy's default) of ``predict_summary``'s value over the kept draws
        of this sampler and of ``peers`` (samplers or stored samplers of the same model: the chains of a fit), pooled in ONE device call, without the
        [rows x draws] matrix.  ``dense_coef`` / ``ell_coef`` are this sampler's tables, ``peer_dense_coef`` / ``peer_ell_coef`` lists of the
        peers' ([peer's draws x M], [peer's draws x q]); the other arguments as ``predict_summary`` takes them.  ``scratch_bytes`` limits the values
        held at once (fewer rows per chunk).  Returns dict(quantiles [Q x rows], draws: the pooled count, info: QUANTILE_INFO)."""
        fn = getattr(self._lib, self._pfx + "predict_quantiles", None)
        if fn is None:
            raise RuntimeError(f"this library ({self._pfx}*) has no predict_quantiles")

        def draws(smp):
            probe = QuantileOut()
            smp._check(fn(smp._h, None, C.byref(probe)))
            return int(probe.num_samples)
        pr = np.ascontiguousarray(np.atleast_1d(np.asarray(probs, dtype=np.float64)))
        if pr.ndim != 1:
            raise ValueError(f"probs must be a vector, not shape {pr.shape}")
        peers = list(peers)
        rows_in, keep, rows, _ = self._summary_in(draws(self), x_test, offset, dense, dense_coef, ell_index, ell_value, ell_coef, link, None, route,
                                                   stage_nodes, 0)

        pdc, hold_d = _peer_tables(peers, draws, peer_dense_coef, rows_in.n_dense, "peer_dense_coef")
        pec, hold_e = _peer_tables(peers, draws, peer_ell_coef, rows_in.n_ell_coef if rows_in.n_ell else 0, "peer_ell_coef")
        handles = (C.c_void_p * max(1, len(peers)))(*[p._h.value for p in peers])
        q = np.zeros((len(pr), rows))
        buf = q if q.size else np.zeros(1)          # (no prob: refused by the library, which needs a pointer to tell the call from a query)
        arg = QuantileIn(rows=rows_in, n_probs=len(pr), probs=_dp(pr), n_peers=len(peers), peers=handles if peers else None, peer_dense_coef=pdc,
                         peer_ell_coef=pec, scratch_bytes=int(scratch_bytes))
        out = QuantileOut(quantiles=_dp(buf))
        self.quantile_info = dict(zip(QUANTILE_INFO, [0] * 9))
        rc = fn(self._h, C.byref(arg), C.byref(out))
        w = [int(v) for v in out.info]
        self.quantile_info = dict(zip(QUANTILE_INFO, w[:3] + [w[3] >> 32, w[3] & 0xFFFFFFFF] + w[4:]))          # (all zero after a refusal: nothing was launched)
        self._check(rc)
        del keep, hold_d, hold_e, buf
        return dict(quantiles=q, draws=int(out.num_samples), info=dict(self.quantile_info))

    def predict_contrast(self, x_test: np.ndarray, x_test0=None, probs=(), peers=(), peer_dense_coef=None, peer_ell_coef=None, offset=None, offset0=None,
                         dense=None, dense0=None, dense_coef=None, ell_index=None, ell_index0=None, ell_value=None, ell_value0=None, ell_coef=None,
                         link: int = 0, weights=None, per_row: bool = True, route="auto", stage_nodes: int = 0, scratch_bytes: int = 0) -> dict:
        """``s4b_predict_contrast``: the paired contrast d = v(arm 1) - v(arm 0) of two arms over the same rows and the same draws, pooled over this
        sampler and ``peers`` as ``predict_quantiles`` pools them, summarised on the device.  ``x_test`` and the unsuffixed parts are arm 1;
        ``x_test0``, ``offset0``, ``dense0``, ``ell_index0``, ``ell_value0`` arm 0's row side, each None (arm 1's) or shaped as arm 1's; the
        coefficient tables are shared by the arms.  At most two BART columns may differ (in their bins).  ``weights`` [G x rows], G <= 8;
        ``probs`` up to 16; ``per_row`` False leaves mean and m2 out.  Returns dict(mean, m2 [rows] (None without per_row), average [draws x G],
        quantiles [Q x rows], draws: the pooled count, info: CONTRAST_INFO)."""
        fn = getattr(self._lib, self._pfx + "predict_contrast", None)
        if fn is None:
            raise RuntimeError(f"this library ({self._pfx}*) has no predict_contrast")

        def draws(smp):
            probe = ContrastOut()
            smp._check(fn(smp._h, None, C.byref(probe)))
            return int(probe.num_samples)
        arg, keep, rows, G, S, pr = self._contrast_in(draws, x_test, x_test0, probs, peers, peer_dense_coef, peer_ell_coef, offset, offset0, dense, dense0,
                                                      dense_coef, ell_index, ell_index0, ell_value, ell_value0, ell_coef, link, weights, route, stage_nodes,
                                                      scratch_bytes)
        mean, m2 = (np.zeros(rows), np.zeros(rows)) if per_row else (None, None)
        avg, q = np.zeros((S, G)), np.zeros((len(pr), rows))
        spare = np.zeros(1)          # (what a count beyond the library's limits would fill: refused there, which needs a pointer to tell the call from a query)
        out = ContrastOut(mean=_dp(mean), m2=_dp(m2), average=_dp(avg) if avg.size else (_dp(spare) if G else None),
                          quantiles=_dp(q) if q.size else (_dp(spare) if len(pr) else None))
        if not per_row and not G and not len(pr):
            out.average = _dp(spare)          # (nothing asked for: the library says so)
        self.contrast_info = dict(zip(CONTRAST_INFO, [0] * 9))
        rc = fn(self._h, C.byref(arg), C.byref(out))
        w = [int(v) for v in out.info]
        self.contrast_info = dict(zip(CONTRAST_INFO, w[:7] + [w[7] >> 32, w[7] & 0xFFFFFFFF]))          # (all zero after a refusal: nothing was launched)
        self._check(rc)
        del keep, spare
        return dict(mean=mean, m2=m2, average=avg, quantiles=q, draws=int(out.num_samples), info=dict(self.contrast_info))

    def _contrast_in(self, draws, x_test, x_test0, probs, peers, peer_dense_coef, peer_ell_coef, offset, offset0, dense, dense0, dense_coef, ell_index,
                     ell_index0, ell_value, ell_value0, ell_coef, link, weights, route, stage_nodes, scratch_bytes):
        """The ``s4b_contrast_in`` of a ``predict_contrast`` or ``predict_groups`` call; ``draws(sampler)`` is a sampler's kept draw count:
        (struct, what it points into, rows, weight vectors, pooled draws, probs)."""
        pr = np.ascontiguousarray(np.atleast_1d(np.asarray(probs, dtype=np.float64)))
        if pr.ndim != 1:
            raise ValueError(f"probs must be a vector, not shape {pr.shape}")
        peers = list(peers)
        own = draws(self)
        rows_in, keep, rows, G = self._summary_in(own, x_test, offset, dense, dense_coef, ell_index, ell_value, ell_coef, link, weights, route,
                                                   stage_nodes, 0)

        def arm0(a, cols, what, dtype=np.float64):
            """Arm 0's side of a part: [rows] (cols None) or [rows x cols], column-major; where arm 1 has no such part (cols 0) the array goes
            through as it is and the library refuses the call."""
            if a is None:
                return None
            a = np.asfortranarray(np.asarray(a, dtype=dtype))
            want = (rows,) if cols is None else (rows, cols or (a.shape[1] if a.ndim == 2 else 0))
            if a.shape != want:
                raise ValueError(f"{what} must have shape {want} like arm 1's, not {a.shape}")
            return a
        x0 = arm0(x_test0, keep["x_test"].shape[1], "x_test0")
        off0 = arm0(offset0, None, "offset0")
        d0 = arm0(dense0, rows_in.n_dense, "dense0")
        ix0 = arm0(ell_index0, rows_in.n_ell, "ell_index0", np.int32)
        ev0 = arm0(ell_value0, rows_in.n_ell, "ell_value0")

        pdc, hold_d = _peer_tables(peers, draws, peer_dense_coef, rows_in.n_dense, "peer_dense_coef")
        pec, hold_e = _peer_tables(peers, draws, peer_ell_coef, rows_in.n_ell_coef if rows_in.n_ell else 0, "peer_ell_coef")
        handles = (C.c_void_p * max(1, len(peers)))(*[p._h.value for p in peers])
        S = own + sum(draws(p) for p in peers)
        arg = ContrastIn(rows=rows_in, x_test0=_dp(x0), offset0=_dp(off0), dense0=_dp(d0), ell_index0=_ip(ix0), ell_value0=_dp(ev0), n_probs=len(pr),
                         probs=_dp(pr), n_peers=len(peers), peers=handles if peers else None, peer_dense_coef=pdc, peer_ell_coef=pec,
                         scratch_bytes=int(scratch_bytes))
        return arg, [keep, hold_d, hold_e, handles, pdc, pec, x0, off0, d0, ix0, ev0, pr], rows, G, S, pr

    def groups_draws(self) -> int:
        """The kept draws of this sampler, as ``s4b_predict_groups``' query form reports them."""
        probe = GroupsOut()
        self._check(self._f("predict_groups")(self._h, None, C.byref(probe)))
        return int(probe.num_samples)

    @staticmethod
    def group_order(labels):
        """The stable sort ``predict_groups`` applies to its rows: (order, sorted labels) with ``labels[order]`` non-decreasing and rows of equal
        label in their given order."""
        lab = np.asarray(labels)
        if lab.ndim != 1 or lab.dtype.kind not in "iu":
            raise ValueError("level must be a vector of integers")
        order = np.argsort(lab, kind="stable")
        return order, lab[order]

    def predict_groups(self, x_test: np.ndarray, level, n_levels: int, x_test0=None, n_arms: int = 1, statistic="mean", threshold=None, probs=(),
                       peers=(), peer_dense_coef=None, peer_ell_coef=None, offset=None, offset0=None, dense=None, dense0=None, dense_coef=None,
                       ell_index=None, ell_index0=None, ell_value=None, ell_value0=None, ell_coef=None, link: int = 0, weights=None,
                       outputs=("mean", "m2", "weight", "count"), route="auto", stage_nodes: int = 0, scratch_bytes: int = 0, level_bytes: int = 0,
                       presorted: bool = False) -> dict:
        """``s4b_predict_groups``: per level l of ``level`` (an integer in [0, n_levels) per row, in ANY order) and per pooled draw the weighted sum
        (``statistic`` "sum") or mean ("mean") of the rows' values — ``n_arms`` 1: ``predict_quantiles``' value, 2: ``predict_contrast``'s d, the
        arms given as there — and over the draws its mean, m2, the ``probs`` quantiles and, with a ``threshold``, the share of the draws strictly
        above it.  ``weights`` None (1) or [rows], non-negative.  The library wants the rows of a level contiguous: every row-side array is permuted
        here by a stable sort of ``level`` (``presorted`` True hands the rows down as they are; a decreasing label is then refused by the
        library).  ``outputs`` names what is formed besides quantiles (with probs) and p_above (with a threshold): any of "mean", "m2",
        "weight", "count", "draws" ([levels x pooled draws]).  ``level_bytes`` lowers the limit on 8 x levels x pooled draws
        (GROUPS_LEVEL_BYTES_MAX).  Returns a dict of the outputs in level order (None where not formed), ``draws_pooled`` and info: GROUPS_INFO."""
        fn = getattr(self._lib, self._pfx + "predict_groups", None)
        if fn is None:
            raise RuntimeError(f"this library ({self._pfx}*) has no predict_groups")

        def draws(smp):
            probe = GroupsOut()
            smp._check(fn(smp._h, None, C.byref(probe)))
            return int(probe.num_samples)
        unknown = set(outputs) - {"mean", "m2", "weight", "count", "draws"}
        if unknown:
            raise ValueError(f"unknown outputs {sorted(unknown)}")
        lab = np.asarray(level)
        if lab.ndim != 1 or lab.dtype.kind not in "iu" or len(lab) != np.shape(x_test)[0]:
            raise ValueError("level must hold one integer per row of x_test")
        if len(lab) and (lab.min() < -2 ** 31 or lab.max() >= 2 ** 31):
            raise ValueError("level does not fit 32 bits")
        L = int(n_levels)
        if weights is not None:
            weights = np.asarray(weights, dtype=np.float64)
            if weights.shape != (len(lab),):
                raise ValueError(f"weights must be [{len(lab)}], not shape {weights.shape}")
        if not presorted:          # the rows of a level next to one another, in their given order: every row-side array goes through the same permutation
            order, lab = self.group_order(lab)

            def rows_of(a):
                return None if a is None else np.asarray(a)[order]
            x_test, x_test0, offset, offset0, dense, dense0 = (rows_of(a) for a in (x_test, x_test0, offset, offset0, dense, dense0))
            ell_index, ell_index0, ell_value, ell_value0, weights = (rows_of(a) for a in (ell_index, ell_index0, ell_value, ell_value0, weights))
        lab = _i32(lab)
        w = None if weights is None else weights[None, :]
        arms, keep, rows, _, S, pr = self._contrast_in(draws, x_test, x_test0, probs, peers, peer_dense_coef, peer_ell_coef, offset, offset0, dense, dense0,
                                                       dense_coef, ell_index, ell_index0, ell_value, ell_value0, ell_coef, link, w, route, stage_nodes,
                                                       scratch_bytes)
        n = max(L, 1)
        res = dict(mean=np.zeros(n) if "mean" in outputs else None, m2=np.zeros(n) if "m2" in outputs else None,
                   quantiles=np.zeros((len(pr), n)) if len(pr) else None, p_above=np.zeros(n) if threshold is not None else None,
                   weight=np.zeros(n) if "weight" in outputs else None, count=np.zeros(n, dtype=np.int64) if "count" in outputs else None)
        # (a level matrix beyond the library's limit is refused there: no host array of that size is made for it)
        fits = 8 * n * S <= GROUPS_LEVEL_BYTES_MAX
        res["draws"] = np.zeros((n, S) if fits else 1) if "draws" in outputs else None
        spare = np.zeros(1)          # (nothing asked for: the library needs a pointer to tell the call from a query)
        arg = GroupsIn(arms=arms, n_arms=int(n_arms), level=_ip(lab), n_levels=L, statistic=int(GROUPS_STATISTICS.get(statistic, statistic)),
                       has_threshold=int(threshold is not None), threshold=0.0 if threshold is None else float(threshold), level_bytes=int(level_bytes))
        out = GroupsOut(mean=_dp(res["mean"]), m2=_dp(res["m2"]), quantiles=_dp(res["quantiles"]), p_above=_dp(res["p_above"]), weight=_dp(res["weight"]),
                        count=None if res["count"] is None else res["count"].ctypes.data_as(C.POINTER(C.c_int64)), draws=_dp(res["draws"]))
        if all(v is None for v in res.values()):
            out.weight = _dp(spare)
        self.groups_info = dict(zip(GROUPS_INFO, [0] * 8))
        rc = fn(self._h, C.byref(arg), C.byref(out))
        self.groups_info = dict(zip(GROUPS_INFO, (int(v) for v in out.info)))          # (all zero after a refusal: nothing was launched)
        self._check(rc)
        del keep, spare
        return dict(res, draws_pooled=int(out.num_samples), info=dict(self.groups_info))

    def describe_draws(self) -> int:
        """The kept draws of this sampler, as ``s4b_predict_describe``'s query form without an input reports them."""
        probe = DescribeOut()
        self._check(self._f("predict_describe")(self._h, None, C.byref(probe)))
        return int(probe.num_samples)

    def predict_describe(self, x_test: np.ndarray, x_test0=None, n_arms: int = 1, hdi_count=(), thresholds=(), probs=(), peers=(),
                         peer_dense_coef=None, peer_ell_coef=None, offset=None, offset0=None, dense=None, dense0=None, dense_coef=None,
                         ell_index=None, ell_index0=None, ell_value=None, ell_value0=None, ell_coef=None, link: int = 0, weights=None,
                         outputs=DESCRIBE_OUTPUTS, route="auto", stage_nodes: int = 0, scratch_bytes: int = 0) -> dict:
        """``s4b_predict_describe``: per row, from its pooled draws in sorted order x(0) <= ... <= x(S-1) — ``n_arms`` 1: ``predict_quantiles``' value,
        2: ``predict_contrast``'s d, the arms given as there — the ``probs`` type-7 quantiles [probs x rows], the median [rows], for every integer m of
        ``hdi_count`` (1 <= m <= S, at most DESCRIBE_HDI_MAX) the shortest window of m draws, hdi [counts x 2 x rows] and hdi_start [counts x rows] (the
        lowest start among the windows of the smallest width), for every threshold (at most DESCRIBE_THRESHOLDS_MAX, no NaN) the draws strictly above
        and strictly below it, n_above and n_below [thresholds x rows] int32, and the unscaled median absolute deviation mad [rows].  ``outputs``
        names what is formed, among DESCRIBE_OUTPUTS; an output whose count is 0 (quantiles without probs, hdi and hdi_start without hdi_count,
        n_above and n_below without thresholds) is left out.  ``outputs`` empty is the query: every check runs, nothing is launched and info holds the
        plan.  ``weights`` must stay None: there are no row weights.  Returns a dict of the outputs (None where not formed), ``draws`` (pooled) and
        info: DESCRIBE_INFO."""
        fn = getattr(self._lib, self._pfx + "predict_describe", None)
        if fn is None:
            raise RuntimeError(f"this library ({self._pfx}*) has no predict_describe")

        def draws(smp):
            probe = DescribeOut()
            smp._check(fn(smp._h, None, C.byref(probe)))
            return int(probe.num_samples)
        unknown = set(outputs) - set(DESCRIBE_OUTPUTS)
        if unknown:
            raise ValueError(f"outputs must be among {DESCRIBE_OUTPUTS}, not {sorted(unknown)}")
        cnt = np.atleast_1d(np.asarray(hdi_count))
        if cnt.ndim != 1 or (cnt.size and cnt.dtype.kind not in "iu"):
            raise ValueError("hdi_count must be a vector of integers")
        if cnt.size and (cnt.min() < -2 ** 31 or cnt.max() >= 2 ** 31):
            raise ValueError("hdi_count does not fit 32 bits")
        cnt = _i32(cnt)
        thr = np.ascontiguousarray(np.atleast_1d(np.asarray(thresholds, dtype=np.float64)))
        if thr.ndim != 1:
            raise ValueError(f"thresholds must be a vector, not shape {thr.shape}")
        w = None if weights is None else np.asarray(weights, dtype=np.float64)[None, :]
        arms, keep, rows, _, S, pr = self._contrast_in(draws, x_test, x_test0, probs, peers, peer_dense_coef, peer_ell_coef, offset, offset0, dense, dense0,
                                                       dense_coef, ell_index, ell_index0, ell_value, ell_value0, ell_coef, link, w, route, stage_nodes,
                                                       scratch_bytes)
        n, Q, M, T = max(rows, 1), len(pr), len(cnt), len(thr)
        shape = dict(quantiles=(Q, n), median=(n,), hdi=(M, 2, n), hdi_start=(M, n), n_above=(T, n), n_below=(T, n), mad=(n,))
        size = dict(quantiles=Q, hdi=M, hdi_start=M, n_above=T, n_below=T)
        res = {k: np.zeros(shape[k], dtype=np.int32 if k in ("hdi_start", "n_above", "n_below") else np.float64)
               if k in outputs and size.get(k, 1) > 0 else None for k in DESCRIBE_OUTPUTS}
        arg = DescribeIn(arms=arms, n_arms=int(n_arms), n_hdi=M, hdi_count=_ip(cnt) if M else None, n_thresholds=T, thresholds=_dp(thr) if T else None)
        out = DescribeOut(quantiles=_dp(res["quantiles"]), median=_dp(res["median"]), hdi=_dp(res["hdi"]), hdi_start=_ip(res["hdi_start"]),
                          n_above=_ip(res["n_above"]), n_below=_ip(res["n_below"]), mad=_dp(res["mad"]))
        self.describe_info = dict(zip(DESCRIBE_INFO, [0] * 9))
        rc = fn(self._h, C.byref(arg), C.byref(out))
        v = [int(x) for x in out.info]
        self.describe_info = dict(zip(DESCRIBE_INFO, v[:6] + [v[6] >> 32, v[6] & 0xFFFFFFFF, v[7]]))          # (all zero after a refusal: nothing was launched)
        self._check(rc)
        del keep
        return dict(res, draws=int(out.num_samples), info=dict(self.describe_info))

    def sorted_draws(self) -> int:
        """The kept draws of this sampler, as ``s4b_predict_sorted``'s query form without an input reports them."""
        probe = SortedOut()
        self._check(self._f("predict_sorted")(self._h, None, C.byref(probe)))
        return int(probe.num_samples)

    def predict_sorted(self, x_test: np.ndarray, x_test0=None, n_arms: int = 1, row_probs=(), top=(), bottom=(), cut_rank=(), probs=(), peers=(),
                       peer_dense_coef=None, peer_ell_coef=None, offset=None, offset0=None, dense=None, dense0=None, dense_coef=None,
                       ell_index=None, ell_index0=None, ell_value=None, ell_value0=None, ell_coef=None, link: int = 0, weights=None,
                       outputs=SORTED_OUTPUTS, route="auto", stage_nodes: int = 0, scratch_bytes: int = 0) -> dict:
        """``s4b_predict_sorted``: per pooled draw the order statistics of the rows' values ACROSS THE ROWS — ``n_arms`` 1: ``predict_quantiles``'
        value, 2: ``predict_contrast``'s d, the arms given as there.  ``row_probs`` (at most SORTED_PROBS_MAX, in [0, 1]): the type-7 quantiles
        across the rows, the rows ``sorted`` of the statistics matrix.  The cuts (at most SORTED_CUTS_MAX together), the rows ``cut`` behind them:
        for each fraction f of ``top``, 0 < f < 1, with m = ``fraction_count(f, rows)`` < rows, the rank rows - m - 1 — the m rows strictly above it
        are the top group of the draw; for each fraction of ``bottom`` the rank m — the m rows strictly below it are the bottom group; then the
        ranks of ``cut_rank`` as they are.  Over the draws the mean, m2 and the ``probs`` quantiles of every statistic; per cut and row the int32
        counts ``n_above`` and ``n_below`` of the draws in which the row lies strictly above / below the cut, and from them ``p_top``
        [top x rows] = n_above / draws and ``p_bottom`` [bottom x rows] = n_below / draws.  ``outputs`` names what is formed, among SORTED_OUTPUTS;
        an output whose count is 0 is left out; ``outputs`` empty is the query: every check runs, nothing is launched and info holds the plan.
        ``weights`` must stay None: ranks are unweighted.  Returns mean, m2 [Qr + J], quantiles [Q x (Qr + J)], draws [(Qr + J) x pooled draws]
        (None where not formed), n_above, n_below, p_top, p_bottom, cut_rank (all J ranks), top_count, bottom_count, row_probs, ``draws_pooled``
        and info: SORTED_INFO."""
        fn = getattr(self._lib, self._pfx + "predict_sorted", None)
        if fn is None:
            raise RuntimeError(f"this library ({self._pfx}*) has no predict_sorted")

        def draws(smp):
            probe = SortedOut()
            smp._check(fn(smp._h, None, C.byref(probe)))
            return int(probe.num_samples)
        unknown = set(outputs) - set(SORTED_OUTPUTS)
        if unknown:
            raise ValueError(f"outputs must be among {SORTED_OUTPUTS}, not {sorted(unknown)}")
        rp = np.ascontiguousarray(np.atleast_1d(np.asarray(row_probs, dtype=np.float64)))
        if rp.ndim != 1:
            raise ValueError(f"row_probs must be a vector, not shape {rp.shape}")
        n_rows = int(np.shape(x_test)[0])
        tc = [fraction_count(f, n_rows) for f in np.atleast_1d(np.asarray(top, dtype=np.float64))]
        bc = [fraction_count(f, n_rows) for f in np.atleast_1d(np.asarray(bottom, dtype=np.float64))]
        extra = np.atleast_1d(np.asarray(cut_rank))
        if extra.ndim != 1 or (extra.size and extra.dtype.kind not in "iu"):
            raise ValueError("cut_rank must be a vector of integers")
        if extra.size and (extra.min() < -2 ** 31 or extra.max() >= 2 ** 31):
            raise ValueError("cut_rank does not fit 32 bits")
        cuts = _i32(np.r_[[n_rows - m - 1 for m in tc], bc, extra].astype(np.int64))
        w = None if weights is None else np.asarray(weights, dtype=np.float64)[None, :]
        arms, keep, rows, _, S, pr = self._contrast_in(draws, x_test, x_test0, probs, peers, peer_dense_coef, peer_ell_coef, offset, offset0, dense, dense0,
                                                       dense_coef, ell_index, ell_index0, ell_value, ell_value0, ell_coef, link, w, route, stage_nodes,
                                                       scratch_bytes)
        n, Q, Qr, J = max(rows, 1), len(pr), len(rp), len(cuts)
        L = min(Qr, SORTED_PROBS_MAX) + min(J, SORTED_CUTS_MAX)          # (more are refused by the library: no array is sized by them)
        Jc = min(J, SORTED_CUTS_MAX)
        shape = dict(mean=(L,), m2=(L,), quantiles=(Q, L), draws=(L, S), n_above=(Jc, n), n_below=(Jc, n))
        size = dict(mean=L, m2=L, quantiles=Q * L, draws=L, n_above=Jc, n_below=Jc)
        res = {k: np.zeros(shape[k], dtype=np.int32 if k in ("n_above", "n_below") else np.float64) if k in outputs and size[k] > 0 else None
               for k in SORTED_OUTPUTS}
        arg = SortedIn(arms=arms, n_arms=int(n_arms), n_row_probs=Qr, row_probs=_dp(rp) if Qr else None, n_cuts=J, cut_rank=_ip(cuts) if J else None)
        out = SortedOut(mean=_dp(res["mean"]), m2=_dp(res["m2"]), quantiles=_dp(res["quantiles"]), draws=_dp(res["draws"]),
                        n_above=_ip(res["n_above"]), n_below=_ip(res["n_below"]))
        self.sorted_info = dict(zip(SORTED_INFO, [0] * 8))
        rc = fn(self._h, C.byref(arg), C.byref(out))
        self.sorted_info = dict(zip(SORTED_INFO, (int(v) for v in out.info)))          # (all zero after a refusal: nothing was launched)
        self._check(rc)
        del keep
        Sp = int(out.num_samples)
        nt, nb = len(tc), len(bc)
        p_top = res["n_above"][:nt].astype(np.int64) / Sp if res["n_above"] is not None else None
        p_bottom = res["n_below"][nt:nt + nb].astype(np.int64) / Sp if res["n_below"] is not None else None
        return dict(res, p_top=p_top, p_bottom=p_bottom, cut_rank=cuts.astype(np.int64), top_count=np.asarray(tc, dtype=np.int64),
                    bottom_count=np.asarray(bc, dtype=np.int64), row_probs=rp, draws_pooled=Sp, info=dict(self.sorted_info))

    def test_sorted_select(self, values, block_draws: int, ranks=(), cut_rank=(), outputs=("order_stats", "n_above", "n_below")) -> dict:
        """``s4b_test_sorted_select``: the selection and the count kernels of ``predict_sorted`` alone on ``values`` [n x S] in blocks of
        ``block_draws`` columns.  Returns order_stats [ranks x S], n_above, n_below [cuts x n] (None where not asked for or empty) and info."""
        fn = self._f("test_sorted_select")
        v = np.ascontiguousarray(np.asarray(values, dtype=np.float64))
        if v.ndim != 2:
            raise ValueError(f"values must be [n x S], not shape {v.shape}")
        n, S = v.shape
        rk, ct = _i32(np.atleast_1d(np.asarray(ranks, dtype=np.int64))), _i32(np.atleast_1d(np.asarray(cut_rank, dtype=np.int64)))
        R, J = len(rk), len(ct)
        ostat = np.zeros((R, S)) if "order_stats" in outputs and R else None
        above = np.zeros((J, n), dtype=np.int32) if "n_above" in outputs and J else None
        below = np.zeros((J, n), dtype=np.int32) if "n_below" in outputs and J else None
        info = np.zeros(8, dtype=np.int64)
        self._check(fn(self._h, _dp(v), n, S, int(block_draws), R, _ip(rk) if R else None, _dp(ostat), J, _ip(ct) if J else None, _ip(above), _ip(below),
                       info.ctypes.data_as(C.POINTER(C.c_int64))))
        return dict(order_stats=ostat, n_above=above, n_below=below,
                    info=dict(zip(("draws_per_workgroup", "draws_per_block", "blocks", "launches", "device_bytes", "draws", "targets", "passes"),
                                  (int(x) for x in info))))

    def projection_draws(self) -> int:
        """The kept draws of this sampler, as ``s4b_predict_projection``'s query form reports them."""
        probe = ProjectionOut()
        self._check(self._f("predict_projection")(self._h, None, C.byref(probe)))
        return int(probe.num_samples)

    @staticmethod
    def column_scales(design):
        """Per design column the power of two nearest 1 / rms of the column (1 for a column of zeros): multiplying by it is exact."""
        a = np.asarray(design, dtype=np.float64)
        rms = np.sqrt(np.mean(a * a, axis=0)) if a.shape[0] else np.ones(a.shape[1])
        ok = np.isfinite(rms) & (rms > 0.0)
        return np.where(ok, np.exp2(-np.rint(np.log2(np.where(ok, rms, 1.0)))), 1.0)

    def predict_projection(self, x_test: np.ndarray, design, x_test0=None, n_arms: int = 1, threshold=None, probs=(), tol: float = 1e-10,
                           scale_columns: bool = True, peers=(), peer_dense_coef=None, peer_ell_coef=None, offset=None, offset0=None, dense=None,
                           dense0=None, dense_coef=None, ell_index=None, ell_index0=None, ell_value=None, ell_value0=None, ell_coef=None,
                           link: int = 0, weights=None, route="auto", stage_nodes: int = 0, scratch_bytes: int = 0) -> dict:
        """``s4b_predict_projection``: per pooled draw the weighted least-squares coefficients of the rows' values — ``n_arms`` 1:
        ``predict_quantiles``' value, 2: ``predict_contrast``'s d, the arms given as there — on ``design`` [rows x K], K <= 32, taken as given (no
        intercept is added), the r2 of that fit, and over the draws the mean, m2, the ``probs`` quantiles and, with a ``threshold``, the share of the
        draws strictly above it, for every coefficient and (index K) for r2.  ``weights`` None (1) or [rows], non-negative.  ``scale_columns``:
        every design column is multiplied by the power of two nearest 1 / rms of the column before the call and coef, mean, quantiles (times the
        scale) and m2 (times its square) are scaled back after it.  That is exact — a power of two changes no significand — and removes scale
        disparities between the columns from the normal equations, on which ``tol`` acts, at no rounding cost; p_above of a scaled coefficient
        against a threshold other than 0 is counted here from the rescaled coef (the same strict count).  Returns coef [K x draws], r2 [draws], mean,
        m2 [K + 1], quantiles [Q x (K + 1)] or None, p_above [K + 1] or None, weight, scale [K], deficient (0 answered, 1 deficient design, 2 the
        weights sum to 0, 3 no rows: NaN in every floating output), ``draws_pooled`` and info: PROJECTION_INFO."""
        fn = getattr(self._lib, self._pfx + "predict_projection", None)
        if fn is None:
            raise RuntimeError(f"this library ({self._pfx}*) has no predict_projection")

        def draws(smp):
            probe = ProjectionOut()
            smp._check(fn(smp._h, None, C.byref(probe)))
            return int(probe.num_samples)
        A = np.asarray(design, dtype=np.float64)
        if A.ndim != 2 or A.shape[0] != np.shape(x_test)[0]:
            raise ValueError(f"design must be [{np.shape(x_test)[0]} x K], one row per row of x_test, not shape {A.shape}")
        K = A.shape[1]
        if weights is not None:
            weights = np.asarray(weights, dtype=np.float64)
            if weights.shape != (A.shape[0],):
                raise ValueError(f"weights must be [{A.shape[0]}], not shape {weights.shape}")
        scale = self.column_scales(A) if scale_columns else np.ones(K)
        A = np.ascontiguousarray(A * scale)          # (row-major; exact)
        w = None if weights is None else weights[None, :]
        arms, keep, rows, _, S, pr = self._contrast_in(draws, x_test, x_test0, probs, peers, peer_dense_coef, peer_ell_coef, offset, offset0, dense, dense0,
                                                       dense_coef, ell_index, ell_index0, ell_value, ell_value0, ell_coef, link, w, route, stage_nodes,
                                                       scratch_bytes)
        n = max(K, 1)
        res = dict(coef=np.zeros((n, S)), r2=np.zeros(S), mean=np.zeros(n + 1), m2=np.zeros(n + 1),
                   quantiles=np.zeros((len(pr), n + 1)) if len(pr) else None, p_above=np.zeros(n + 1) if threshold is not None else None)
        arg = ProjectionIn(arms=arms, n_arms=int(n_arms), n_columns=K, design=_dp(A), has_threshold=int(threshold is not None),
                           threshold=0.0 if threshold is None else float(threshold), tol=float(tol))
        out = ProjectionOut(coef=_dp(res["coef"]), r2=_dp(res["r2"]), mean=_dp(res["mean"]), m2=_dp(res["m2"]), quantiles=_dp(res["quantiles"]),
                            p_above=_dp(res["p_above"]))
        self.projection_info = dict(zip(PROJECTION_INFO, [0] * 8))
        rc = fn(self._h, C.byref(arg), C.byref(out))
        self.projection_info = dict(zip(PROJECTION_INFO, (int(v) for v in out.info)))          # (all zero after a refusal: nothing was launched)
        self._check(rc)
        del keep
        if np.any(scale != 1.0):          # back to the caller's columns: beta_j = scale_j x (the scaled column's coefficient)
            res["coef"] *= scale[:, None]
            res["mean"][:K] *= scale
            res["m2"][:K] *= scale * scale
            if res["quantiles"] is not None:
                res["quantiles"][:, :K] *= scale
            if threshold is not None and float(threshold) != 0.0 and not np.isnan(res["p_above"][0]):
                res["p_above"][:K] = (res["coef"] > float(threshold)).sum(axis=1) / float(S)
        return dict(res, weight=float(out.weight), scale=scale, deficient=int(out.info[6]), draws_pooled=int(out.num_samples),
                    info=dict(self.projection_info))

    def spread_draws(self) -> int:
        """The kept draws of this sampler, as ``s4b_predict_spread``'s query form reports them."""
        probe = SpreadOut()
        self._check(self._f("predict_spread")(self._h, None, C.byref(probe)))
        return int(probe.num_samples)

    @staticmethod
    def spread_names(n_thresholds: int):
        """The statistics of ``s4b_predict_spread``'s matrix in row order: 4 + 2 T names."""
        T = int(n_thresholds)
        return ["mean", "sd", "min", "max"] + [f"share_above[{j}]" for j in range(T)] + [f"part_above[{j}]" for j in range(T)]

    def predict_spread(self, x_test: np.ndarray, thresholds=(), x_test0=None, n_arms: int = 1, probs=(), peers=(), peer_dense_coef=None,
                       peer_ell_coef=None, offset=None, offset0=None, dense=None, dense0=None, dense_coef=None, ell_index=None, ell_index0=None,
                       ell_value=None, ell_value0=None, ell_coef=None, link: int = 0, weights=None, outputs=("mean", "m2", "draws"), route="auto",
                       stage_nodes: int = 0, scratch_bytes: int = 0, bin_index="auto") -> dict:
        """``s4b_predict_spread``: per pooled draw the spread of the rows' values ACROSS THE ROWS — ``n_arms`` 1: ``predict_quantiles``' value, 2:
        ``predict_contrast``'s d, the arms given as there: the weighted mean, the standard deviation (population form), the smallest and the largest
        value among the rows with weight, and for each of the T <= 64 strictly ascending ``thresholds`` (+-inf allowed) the share of the weight on
        the rows strictly above it and the part of the mean those rows contribute; over the draws the mean, m2 and the ``probs`` quantiles of each
        of these 4 + 2 T statistics.  ``weights`` None (1) or [rows], non-negative, not all 0.  ``outputs``: any of "mean", "m2", "draws" (the
        [(4 + 2 T) x pooled draws] matrix itself).  ``bin_index`` "auto", "compare" or "search": how the kernel finds a value's bin (the same
        result).  Returns names, mean, m2 [4 + 2 T], quantiles [Q x (4 + 2 T)] or None, draws or None, weight, thresholds, ``draws_pooled`` and
        info: SPREAD_INFO."""
        fn = getattr(self._lib, self._pfx + "predict_spread", None)
        if fn is None:
            raise RuntimeError(f"this library ({self._pfx}*) has no predict_spread")

        def draws(smp):
            probe = SpreadOut()
            smp._check(fn(smp._h, None, C.byref(probe)))
            return int(probe.num_samples)
        unknown = set(outputs) - {"mean", "m2", "draws"}
        if unknown:
            raise ValueError(f"unknown outputs {sorted(unknown)}")
        th = np.ascontiguousarray(np.atleast_1d(np.asarray(thresholds, dtype=np.float64)))
        if th.ndim != 1:
            raise ValueError(f"thresholds must be a vector, not shape {th.shape}")
        if isinstance(bin_index, str) and bin_index not in SPREAD_BIN_INDEX:
            raise ValueError(f"bin_index must be one of {', '.join(SPREAD_BIN_INDEX)}, not {bin_index!r}")
        n = np.shape(x_test)[0]
        if weights is not None:
            weights = np.asarray(weights, dtype=np.float64)
            if weights.shape != (n,):
                raise ValueError(f"weights must be [{n}], not shape {weights.shape}")
        w = None if weights is None else weights[None, :]
        arms, keep, rows, _, S, pr = self._contrast_in(draws, x_test, x_test0, probs, peers, peer_dense_coef, peer_ell_coef, offset, offset0, dense, dense0,
                                                       dense_coef, ell_index, ell_index0, ell_value, ell_value0, ell_coef, link, w, route, stage_nodes,
                                                       scratch_bytes)
        T = len(th)
        M = 4 + 2 * min(T, SPREAD_THRESHOLDS_MAX)          # (more thresholds are refused by the library: no array is sized by them)
        res = dict(mean=np.zeros(M) if "mean" in outputs else None, m2=np.zeros(M) if "m2" in outputs else None,
                   quantiles=np.zeros((len(pr), M)) if len(pr) else None, draws=np.zeros((M, S)) if "draws" in outputs else None)
        spare = np.zeros(M)          # (nothing asked for: the library needs a pointer to tell the call from a query)
        arg = SpreadIn(arms=arms, n_arms=int(n_arms), n_thresholds=T, thresholds=_dp(th) if T else None,
                       bin_index=int(SPREAD_BIN_INDEX.get(bin_index, bin_index)))
        out = SpreadOut(mean=_dp(res["mean"]), m2=_dp(res["m2"]), quantiles=_dp(res["quantiles"]), draws=_dp(res["draws"]))
        if all(v is None for v in res.values()):
            out.mean = _dp(spare)
        self.spread_info = dict(zip(SPREAD_INFO, [0] * 8))
        rc = fn(self._h, C.byref(arg), C.byref(out))
        self.spread_info = dict(zip(SPREAD_INFO, (int(v) for v in out.info)))          # (all zero after a refusal: nothing was launched)
        self._check(rc)
        del keep, spare
        return dict(res, names=self.spread_names(T), weight=float(out.weight), thresholds=th, draws_pooled=int(out.num_samples),
                    info=dict(self.spread_info))

    def check_draws(self) -> int:
        """The kept draws of this sampler, as ``s4b_predict_check``'s query form reports them."""
        probe = CheckOut()
        self._check(self._f("predict_check")(self._h, None, C.byref(probe)))
        return int(probe.num_samples)

    @staticmethod
    def check_names(n_thresholds: int):
        """The statistics of ``s4b_predict_check``'s matrix in row order: 7 + T names (``observed`` holds the first 5 + T)."""
        return ["mean", "sd", "m3", "min", "max"] + [f"share_above[{j}]" for j in range(int(n_thresholds))] + ["disc_rep", "disc_obs"]

    def predict_check(self, x_test: np.ndarray, y=None, thresholds=(), probs=(), sigma=None, row_scale=None, noise_key: int = 0, weights=None,
                      peers=(), peer_sigma=None, peer_dense_coef=None, peer_ell_coef=None, offset=None, dense=None, dense_coef=None, ell_index=None,
                      ell_value=None, ell_coef=None, link: int = 0, outputs=("mean", "m2", "observed"), route="auto", stage_nodes: int = 0,
                      scratch_bytes: int = 0, bin_index="auto") -> dict:
        """``s4b_predict_check``: posterior predictive checks over the kept draws of this sampler and of ``peers``, pooled in ONE device call as
        ``predict_ppd`` pools them.  Per pooled draw the statistics of the replicate y_rep ACROSS THE ROWS — link 0: z + sigma row_scale e, the bits
        ``predict_ppd`` sorts under the same ``noise_key``; link 1: 1 where a uniform of the same block is <= Phi(z) —: the weighted mean, sd, third
        central moment, min, max, the share of the weight strictly above each of the T <= 64 ascending ``thresholds`` (T = 0 under link 1), and
        the realised discrepancy of the replicate and of ``y`` [rows] (link 0: chi^2, link 1: deviance); over the draws the mean, m2 and ``probs``
        quantiles of each of these 7 + T series.  ``weights`` None (1) or [rows], non-negative, not all 0.  ``outputs``: any of "mean", "m2",
        "observed" (the first 5 + T statistics of ``y`` itself); the matrix ``draws`` [(7 + T) x pooled draws] is always returned.  Returns names,
        draws, observed, mean, m2, quantiles [Q x (7 + T)] or None, weight, thresholds, ``draws_pooled`` and info: CHECK_INFO."""
        fn = getattr(self._lib, self._pfx + "predict_check", None)
        if fn is None:
            raise RuntimeError(f"this library ({self._pfx}*) has no predict_check")

        def draws(smp):
            probe = CheckOut()
            smp._check(fn(smp._h, None, C.byref(probe)))
            return int(probe.num_samples)
        unknown = set(outputs) - {"mean", "m2", "observed"}
        if unknown:
            raise ValueError(f"unknown outputs {sorted(unknown)}")
        pr = np.ascontiguousarray(np.atleast_1d(np.asarray(probs, dtype=np.float64)))
        if pr.ndim != 1:
            raise ValueError(f"probs must be a vector, not shape {pr.shape}")
        th = np.ascontiguousarray(np.atleast_1d(np.asarray(thresholds, dtype=np.float64)))
        if th.ndim != 1:
            raise ValueError(f"thresholds must be a vector, not shape {th.shape}")
        if isinstance(bin_index, str) and bin_index not in SPREAD_BIN_INDEX:
            raise ValueError(f"bin_index must be one of {', '.join(SPREAD_BIN_INDEX)}, not {bin_index!r}")
        peers = list(peers)
        own = draws(self)
        rows_in, keep, rows, _ = self._summary_in(own, x_test, offset, dense, dense_coef, ell_index, ell_value, ell_coef, link, None, route,
                                                   stage_nodes, 0)

        def vector(a, n, what):
            if a is None:
                return None
            a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
            if a.shape != (n,):
                raise ValueError(f"{what} must have shape ({n},), not {a.shape}")
            return a

        pdc, hold_d = _peer_tables(peers, draws, peer_dense_coef, rows_in.n_dense, "peer_dense_coef")
        pec, hold_e = _peer_tables(peers, draws, peer_ell_coef, rows_in.n_ell_coef if rows_in.n_ell else 0, "peer_ell_coef")
        psg, hold_s = _peer_tables(peers, draws, None if peer_sigma is None else [np.asarray(t, dtype=np.float64).reshape(-1, 1) for t in peer_sigma], 1, "peer_sigma")
        handles = (C.c_void_p * max(1, len(peers)))(*[p._h.value for p in peers])
        yy, sg, rs, ww = vector(y, rows, "y"), vector(sigma, own, "sigma"), vector(row_scale, rows, "row_scale"), vector(weights, rows, "weights")
        S = own + sum(draws(p) for p in peers)
        T = len(th)
        Tc = min(T, SPREAD_THRESHOLDS_MAX)          # (more thresholds are refused by the library: no array is sized by them)
        M = 7 + Tc
        res = dict(draws=np.zeros((M, S)), observed=np.zeros(5 + Tc) if "observed" in outputs else None, mean=np.zeros(M) if "mean" in outputs else None,
                   m2=np.zeros(M) if "m2" in outputs else None, quantiles=np.zeros((len(pr), M)) if len(pr) else None)
        arg = CheckIn(rows=rows_in, y=_dp(yy), sigma=_dp(sg), row_scale=_dp(rs), noise_key=int(noise_key) & 0xFFFFFFFFFFFFFFFF, row_weights=_dp(ww),
                      n_thresholds=T, thresholds=_dp(th) if T else None, bin_index=int(SPREAD_BIN_INDEX.get(bin_index, bin_index)), n_probs=len(pr),
                      probs=_dp(pr), n_peers=len(peers), peers=handles if peers else None, peer_dense_coef=pdc, peer_ell_coef=pec, peer_sigma=psg,
                      scratch_bytes=int(scratch_bytes))
        out = CheckOut(mean=_dp(res["mean"]), m2=_dp(res["m2"]), quantiles=_dp(res["quantiles"]), draws=_dp(res["draws"]), observed=_dp(res["observed"]))
        self.check_info = dict(zip(CHECK_INFO, [0] * 8))
        rc = fn(self._h, C.byref(arg), C.byref(out))
        self.check_info = dict(zip(CHECK_INFO, (int(v) for v in out.info)))          # (all zero after a refusal: nothing was launched)
        self._check(rc)
        del keep, hold_d, hold_e, hold_s, yy, sg, rs, ww
        return dict(res, names=self.check_names(T), weight=float(out.weight), thresholds=th, draws_pooled=int(out.num_samples),
                    info=dict(self.check_info))

    def curves_draws(self) -> int:
        """The kept draws of this sampler, as ``s4b_predict_curves``' query form reports them."""
        probe = CurvesOut()
        self._check(self._f("predict_curves")(self._h, None, C.byref(probe)))
        return int(probe.num_samples)

    def predict_curves(self, x_test: np.ndarray, vars, grid, anchor=None, probs=(), outputs=CURVES_OUTPUTS, peers=(), peer_dense_coef=None,
                       peer_ell_coef=None, offset=None, dense=None, dense_coef=None, ell_index=None, ell_value=None, ell_coef=None, link: int = 0,
                       route="auto", stage_nodes: int = 0, scratch_bytes: int = 0) -> dict:
        """``s4b_predict_curves``: per row the response curve along the BART predictors ``vars`` (one index or two) — ``partial_dependence``'s value
        per row and grid point instead of averaged over the rows — over the kept draws of this sampler and of ``peers``, pooled in ONE device call
        as ``predict_quantiles`` pools them.  ``grid`` [G] or [G x len(vars)], G <= 64; ``anchor`` None or the grid index the curves are centred
        at (c = v - v at the anchor); ``probs`` up to 16; ``outputs`` names what is asked for (CURVES_OUTPUTS; the quantile outputs need probs);
        Returns dict(mean, m2, p_max, p_min [rows x G],
        quantiles [Q x rows x G], range_mean, range_m2 [rows], range_quantiles [Q x rows] (None where not asked for), draws: the pooled count,
        info: CURVES_INFO)."""
        fn = getattr(self._lib, self._pfx + "predict_curves", None)
        if fn is None:
            raise RuntimeError(f"this library ({self._pfx}*) has no predict_curves")

        def draws(smp):
            probe = CurvesOut()
            smp._check(fn(smp._h, None, C.byref(probe)))
            return int(probe.num_samples)
        unknown = set(outputs) - set(CURVES_OUTPUTS)
        if unknown:
            raise ValueError(f"outputs must be among {CURVES_OUTPUTS}, not {sorted(unknown)}")
        pr = np.ascontiguousarray(np.atleast_1d(np.asarray(probs, dtype=np.float64)))
        if pr.ndim != 1:
            raise ValueError(f"probs must be a vector, not shape {pr.shape}")
        vs = np.atleast_1d(np.asarray(vars, dtype=np.int64))
        if vs.ndim != 1 or len(vs) not in (1, 2):
            raise ValueError(f"vars must be one predictor index or two, not {vars!r}")
        gr = np.asarray(grid, dtype=np.float64)
        if gr.ndim == 1:
            gr = gr[:, None]
        if gr.ndim != 2 or gr.shape[1] != len(vs):
            raise ValueError(f"grid must be [G] or [G x {len(vs)}], not shape {np.shape(grid)}")
        gr = np.asfortranarray(gr)
        G = gr.shape[0]
        peers = list(peers)
        rows_in, keep, rows, _ = self._summary_in(draws(self), x_test, offset, dense, dense_coef, ell_index, ell_value, ell_coef, link, None, route,
                                                   stage_nodes, 0)
        pdc, hold_d = _peer_tables(peers, draws, peer_dense_coef, rows_in.n_dense, "peer_dense_coef")
        pec, hold_e = _peer_tables(peers, draws, peer_ell_coef, rows_in.n_ell_coef if rows_in.n_ell else 0, "peer_ell_coef")
        handles = (C.c_void_p * max(1, len(peers)))(*[p._h.value for p in peers])
        Q = len(pr)
        shapes = dict(mean=(rows, G), m2=(rows, G), quantiles=(Q, rows, G), p_max=(rows, G), p_min=(rows, G), range_mean=(rows,), range_m2=(rows,),
                      range_quantiles=(Q, rows))
        res = {k: (np.zeros(shapes[k]) if k in outputs else None) for k in CURVES_OUTPUTS}
        spare = np.zeros(1)          # (what a count beyond the library's limits would fill: refused there, which needs a pointer)
        ptr = {k: (None if v is None else _dp(v if v.size else spare)) for k, v in res.items()}
        arg = CurvesIn(rows=rows_in, n_vars=len(vs), vars=(C.c_int32 * 2)(int(vs[0]), int(vs[-1]) if len(vs) > 1 else -1), n_grid=G, grid=_dp(gr),
                       anchor=-1 if anchor is None else int(anchor), n_probs=Q, probs=_dp(pr),
                       n_peers=len(peers), peers=handles if peers else None, peer_dense_coef=pdc, peer_ell_coef=pec, scratch_bytes=int(scratch_bytes))
        out = CurvesOut(**ptr)
        self.curves_info = dict(zip(CURVES_INFO, [0] * 10))
        rc = fn(self._h, C.byref(arg), C.byref(out))
        w = [int(v) for v in out.info]
        self.curves_info = dict(zip(CURVES_INFO, w[:3] + [w[3] >> 32, w[3] & 0xFFFFFFFF] + w[4:7] + [w[7] >> 32, w[7] & 0xFFFFFFFF]))          # (all zero after a refusal)
        self._check(rc)
        del keep, hold_d, hold_e, spare
        return dict(res, draws=int(out.num_samples), info=dict(self.curves_info))

    def predict_ppd(self, x_test: np.ndarray, probs=(), y=None, sigma=None, row_scale=None, noise_key: int = 0, peers=(), peer_sigma=None,
                    peer_dense_coef=None, peer_ell_coef=None, offset=None, dense=None, dense_coef=None, ell_index=None, ell_value=None, ell_coef=None,
                    link: int = 0, lpd: bool = True, moments: bool = True, pit: Optional[bool] = None, route="auto", stage_nodes: int = 0,
                    scratch_bytes: int = 0) -> dict:
        """``s4b_predict_ppd``: the posterior predictive read-out per row over the kept draws of this sampler and of ``peers``, pooled in ONE device
        call as ``predict_quantiles`` pools them.  ``link`` names the response: 0 continuous, 1 binary.  Link 0: ``sigma`` [this sampler's draws]
        and ``peer_sigma`` (one vector per peer), ``row_scale`` [rows] or None (1); ``probs`` (up to 16, may be empty) gives the type-7 quantiles
        of y_rep = z + sigma row_scale e with e a pure function of (``noise_key``, row, pooled draw).  With ``y`` [rows] the scores: ``lpd``,
        ``moments`` (lmean and lm2 of the pointwise log-likelihood) and ``pit`` (None: under link 0 only), each left out where False.  The other
        arguments as ``predict_quantiles`` takes them.  Returns dict(quantiles [Q x rows], lpd, lmean, lm2, pit [rows] (None where not formed),
        draws: the pooled count, info: PPD_INFO)."""
        fn = getattr(self._lib, self._pfx + "predict_ppd", None)
        if fn is None:
            raise RuntimeError(f"this library ({self._pfx}*) has no predict_ppd")

        def draws(smp):
            probe = PpdOut()
            smp._check(fn(smp._h, None, C.byref(probe)))
            return int(probe.num_samples)
        pr = np.ascontiguousarray(np.atleast_1d(np.asarray(probs, dtype=np.float64)))
        if pr.ndim != 1:
            raise ValueError(f"probs must be a vector, not shape {pr.shape}")
        peers = list(peers)
        own = draws(self)
        rows_in, keep, rows, _ = self._summary_in(own, x_test, offset, dense, dense_coef, ell_index, ell_value, ell_coef, link, None, route,
                                                   stage_nodes, 0)

        def vector(a, n, what):
            if a is None:
                return None
            a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
            if a.shape != (n,):
                raise ValueError(f"{what} must have shape ({n},), not {a.shape}")
            return a

        pdc, hold_d = _peer_tables(peers, draws, peer_dense_coef, rows_in.n_dense, "peer_dense_coef")
        pec, hold_e = _peer_tables(peers, draws, peer_ell_coef, rows_in.n_ell_coef if rows_in.n_ell else 0, "peer_ell_coef")
        psg, hold_s = _peer_tables(peers, draws, None if peer_sigma is None else [np.asarray(t, dtype=np.float64).reshape(-1, 1) for t in peer_sigma], 1, "peer_sigma")
        handles = (C.c_void_p * max(1, len(peers)))(*[p._h.value for p in peers])
        yy, sg, rs = vector(y, rows, "y"), vector(sigma, own, "sigma"), vector(row_scale, rows, "row_scale")
        if pit is None:
            pit = int(link) == 0
        scored = yy is not None
        res = dict(quantiles=np.zeros((len(pr), rows)), lpd=np.zeros(rows) if scored and lpd else None, lmean=np.zeros(rows) if scored and moments else None,
                   lm2=np.zeros(rows) if scored and moments else None, pit=np.zeros(rows) if scored and pit else None)
        spare = np.zeros(1)          # (what a count beyond the library's limits would fill: refused there, which needs a pointer to tell the call from a query)
        arg = PpdIn(rows=rows_in, y=_dp(yy), sigma=_dp(sg), row_scale=_dp(rs), noise_key=int(noise_key) & 0xFFFFFFFFFFFFFFFF, n_probs=len(pr),
                    probs=_dp(pr), n_peers=len(peers), peers=handles if peers else None, peer_dense_coef=pdc, peer_ell_coef=pec, peer_sigma=psg,
                    scratch_bytes=int(scratch_bytes))
        out = PpdOut(quantiles=_dp(res["quantiles"]) if res["quantiles"].size else (_dp(spare) if len(pr) else None), lpd=_dp(res["lpd"]),
                     lmean=_dp(res["lmean"]), lm2=_dp(res["lm2"]), pit=_dp(res["pit"]))
        if not len(pr) and not any(res[k] is not None for k in ("lpd", "lmean", "pit")):
            out.quantiles = _dp(spare)          # (nothing asked for: the library says so)
        self.ppd_info = dict(zip(PPD_INFO, [0] * 9))
        rc = fn(self._h, C.byref(arg), C.byref(out))
        w = [int(v) for v in out.info]
        self.ppd_info = dict(zip(PPD_INFO, w[:3] + [w[3] >> 32, w[3] & 0xFFFFFFFF] + w[4:]))          # (all zero after a refusal: nothing was launched)
        self._check(rc)
        del keep, hold_d, hold_e, hold_s, spare, yy, sg, rs
        return dict(res, draws=int(out.num_samples), info=dict(self.ppd_info))

    def predict_loo(self, x_test: np.ndarray, y=None, sigma=None, row_scale=None, tail_len: int = 0, peers=(), peer_sigma=None, peer_dense_coef=None,
                    peer_ell_coef=None, offset=None, dense=None, dense_coef=None, ell_index=None, ell_value=None, ell_coef=None, link: int = 0,
                    outputs=LOO_OUTPUTS, route="auto", stage_nodes: int = 0, scratch_bytes: int = 0) -> dict:
        """``s4b_predict_loo``: PSIS-LOO of the responses ``y`` [rows] per row over the kept draws of this sampler and of ``peers``, pooled in ONE
        device call as ``predict_ppd`` pools them, with its ``link``, ``sigma`` / ``peer_sigma`` and ``row_scale``.  ``tail_len`` 0: the default
        min(ceil(S / 5), ceil(3 sqrt S)); else 5 .. min(S - 1, 1024).  ``outputs``: which of LOO_OUTPUTS are formed.  Returns dict(elpd_loo,
        pareto_k (+inf where no tail was fitted), lpd, ess [rows] (None where not asked for), draws: the pooled count, tail_len: the one used,
        info: LOO_INFO)."""
        fn = getattr(self._lib, self._pfx + "predict_loo", None)
        if fn is None:
            raise RuntimeError(f"this library ({self._pfx}*) has no predict_loo")

        def draws(smp):
            probe = LooOut()
            smp._check(fn(smp._h, None, C.byref(probe)))
            return int(probe.num_samples)
        outputs = tuple(outputs)
        self.loo_info = dict(zip(LOO_INFO, [0] * 9))
        if not outputs or not set(outputs) <= set(LOO_OUTPUTS):          # (no output pointer at all is the library's query form: refused here)
            raise ValueError(f"outputs must name at least one of {LOO_OUTPUTS}, not {outputs!r}")
        peers = list(peers)
        own = draws(self)
        rows_in, keep, rows, _ = self._summary_in(own, x_test, offset, dense, dense_coef, ell_index, ell_value, ell_coef, link, None, route,
                                                   stage_nodes, 0)

        def vector(a, n, what):
            if a is None:
                return None
            a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
            if a.shape != (n,):
                raise ValueError(f"{what} must have shape ({n},), not {a.shape}")
            return a

        pdc, hold_d = _peer_tables(peers, draws, peer_dense_coef, rows_in.n_dense, "peer_dense_coef")
        pec, hold_e = _peer_tables(peers, draws, peer_ell_coef, rows_in.n_ell_coef if rows_in.n_ell else 0, "peer_ell_coef")
        psg, hold_s = _peer_tables(peers, draws, None if peer_sigma is None else [np.asarray(t, dtype=np.float64).reshape(-1, 1) for t in peer_sigma], 1, "peer_sigma")
        handles = (C.c_void_p * max(1, len(peers)))(*[p._h.value for p in peers])
        yy, sg, rs = vector(y, rows, "y"), vector(sigma, own, "sigma"), vector(row_scale, rows, "row_scale")
        res = {k: (np.zeros(rows) if k in outputs else None) for k in LOO_OUTPUTS}
        spare = np.zeros(1)          # (no rows: what the library needs to tell the call from a query)
        arg = LooIn(rows=rows_in, y=_dp(yy), sigma=_dp(sg), row_scale=_dp(rs), tail_len=int(tail_len), n_peers=len(peers), peers=handles if peers else None,
                    peer_dense_coef=pdc, peer_ell_coef=pec, peer_sigma=psg, scratch_bytes=int(scratch_bytes))
        out = LooOut(**{k: _dp(v if v.size else spare) for k, v in res.items() if v is not None})
        self.loo_info = dict(zip(LOO_INFO, [0] * 9))
        rc = fn(self._h, C.byref(arg), C.byref(out))
        w = [int(v) for v in out.info]
        self.loo_info = dict(zip(LOO_INFO, w[:3] + [w[3] >> 32, w[3] & 0xFFFFFFFF] + w[4:]))          # (all zero after a refusal: nothing was launched)
        self._check(rc)
        del keep, hold_d, hold_e, hold_s, spare, yy, sg, rs
        return dict(res, draws=int(out.num_samples), tail_len=int(out.tail_len), info=dict(self.loo_info))

    def predict_convergence(self, x_test: np.ndarray, quantity="ev", split: bool = True, y=None, sigma=None, row_scale=None, peers=(), peer_sigma=None,
                            peer_dense_coef=None, peer_ell_coef=None, offset=None, dense=None, dense_coef=None, ell_index=None, ell_value=None,
                            ell_coef=None, link: int = 0, outputs=CONV_OUTPUTS, route="auto", stage_nodes: int = 0, scratch_bytes: int = 0) -> dict:
        """``s4b_predict_convergence``: split R-hat and the effective sample size per row with the chains kept apart — this sampler and every one of
        ``peers`` (each occurrence of a handle) is one chain, cut to the shortest and, with ``split``, halved.  ``quantity`` "ev" (0): the fitted
        value under ``link``; "lik" (1): the likelihood of ``y`` with ``predict_ppd``'s ``link``, ``sigma`` / ``peer_sigma`` and ``row_scale``.
        ``outputs``: which of CONV_OUTPUTS are formed.  Returns dict(rhat, ess, mean, mcse [rows] float64, n_pairs [rows] int32 (None where not
        asked for; NaN / -1 in a row without an answer), draws: the pooled count, chains, chain_len, info: CONV_INFO)."""
        fn = getattr(self._lib, self._pfx + "predict_convergence", None)
        if fn is None:
            raise RuntimeError(f"this library ({self._pfx}*) has no predict_convergence")

        def draws(smp):
            probe = ConvOut()
            smp._check(fn(smp._h, None, C.byref(probe)))
            return int(probe.num_samples)
        outputs = tuple(outputs)
        self.conv_info = dict(zip(CONV_INFO, [0] * 9))
        if not outputs or not set(outputs) <= set(CONV_OUTPUTS):          # (no output pointer at all is the library's query form: refused here)
            raise ValueError(f"outputs must name at least one of {CONV_OUTPUTS}, not {outputs!r}")
        if isinstance(quantity, str) and quantity not in CONV_QUANTITIES:          # (a number goes to the library as it is)
            raise ValueError(f"quantity must be one of {tuple(CONV_QUANTITIES)}, not {quantity!r}")
        peers = list(peers)
        own = draws(self)
        rows_in, keep, rows, _ = self._summary_in(own, x_test, offset, dense, dense_coef, ell_index, ell_value, ell_coef, link, None, route,
                                                   stage_nodes, 0)

        def vector(a, n, what):
            if a is None:
                return None
            a = np.ascontiguousarray(np.asarray(a, dtype=np.float64))
            if a.shape != (n,):
                raise ValueError(f"{what} must have shape ({n},), not {a.shape}")
            return a

        pdc, hold_d = _peer_tables(peers, draws, peer_dense_coef, rows_in.n_dense, "peer_dense_coef")
        pec, hold_e = _peer_tables(peers, draws, peer_ell_coef, rows_in.n_ell_coef if rows_in.n_ell else 0, "peer_ell_coef")
        psg, hold_s = _peer_tables(peers, draws, None if peer_sigma is None else [np.asarray(t, dtype=np.float64).reshape(-1, 1) for t in peer_sigma], 1, "peer_sigma")
        handles = (C.c_void_p * max(1, len(peers)))(*[p._h.value for p in peers])
        yy, sg, rs = vector(y, rows, "y"), vector(sigma, own, "sigma"), vector(row_scale, rows, "row_scale")
        res = {k: (np.zeros(rows, dtype=np.int32 if k == "n_pairs" else np.float64) if k in outputs else None) for k in CONV_OUTPUTS}
        spare = np.zeros(1)          # (no rows: what the library needs to tell the call from a query)
        arg = ConvIn(rows=rows_in, quantity=int(CONV_QUANTITIES.get(quantity, quantity)), split=int(bool(split)), y=_dp(yy), sigma=_dp(sg), row_scale=_dp(rs),
                     n_peers=len(peers), peers=handles if peers else None, peer_dense_coef=pdc, peer_ell_coef=pec, peer_sigma=psg,
                     scratch_bytes=int(scratch_bytes))
        ptr = {k: ((v if v.size else spare).ctypes.data_as(C.POINTER(C.c_int32)) if k == "n_pairs" else _dp(v if v.size else spare))
               for k, v in res.items() if v is not None}
        out = ConvOut(**ptr)
        rc = fn(self._h, C.byref(arg), C.byref(out))
        w = [int(v) for v in out.info]
        self.conv_info = dict(zip(CONV_INFO, w[:3] + [w[3] >> 32, w[3] & 0xFFFFFFFF] + w[4:]))          # (all zero after a refusal: nothing was launched)
        self._check(rc)
        del keep, hold_d, hold_e, hold_s, spare, yy, sg, rs
        return dict(res, draws=int(out.num_samples), chains=int(out.n_chains), chain_len=int(out.chain_len), info=dict(self.conv_info))

    def profile_leapfrog(self, n_evals: int = 10) -> dict:
        """Per-leapfrog O(N) sums of the hmc_mode 1 path timed with HIP events (measurement hook of the HIP library)."""
        out = (C.c_double * 8)()
        self._check(self._f("profile_leapfrog")(self._h, n_evals, out))
        return dict(kernels_us=out[0], with_fetch_us=out[1], launches=out[2], n=int(out[3]), algorithmic_bytes=out[4])

    def get_state(self) -> bytes:
        """``s4b_get_state``: the whole sampler state (NUTS + adaptation, trees, fits, offsets, both generators)."""
        size = C.c_int64()
        self._check(self._f("get_state")(self._h, None, 0, C.byref(size)))
        buf = C.create_string_buffer(size.value)
        self._check(self._f("get_state")(self._h, buf, size.value, C.byref(size)))
        return buf.raw[: size.value]

    def set_state(self, state: bytes):
        """``s4b_set_state``: resume from / be teacher-forced to a state produced by ``get_state`` of either implementation."""
        buf = C.create_string_buffer(state, len(state))
        self._check(self._f("set_state")(self._h, buf, len(state)))

    def export_bart_state(self) -> bytes:
        """``stan4bart_exportBARTState``: the kept trees + cut points + scales as one byte string."""
        size = C.c_int64()
        self._check(self._f("export_bart_state")(self._h, None, 0, C.byref(size)))
        buf = C.create_string_buffer(size.value)
        self._check(self._f("export_bart_state")(self._h, buf, size.value, C.byref(size)))
        return buf.raw[: size.value]

    def profile_sweep(self, n_sweeps: int = 1) -> dict:
        """Extra BART sweeps timed with HIP events on the sampler's stream (measurement hook of the HIP library)."""
        out = (C.c_double * 8)()
        self._check(self._f("profile_sweep")(self._h, n_sweeps, out))
        return dict(stats_us=out[0], control_us=out[1], apply_us=out[2], launches=[out[3], out[4], out[5]],
                    sweep_wall_us=out[6], n=int(out[7]))

    def free(self):
        if getattr(self, "_h", None) and self._h.value:
            self._f("free")(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class SweepGroup:
    """A sweep group (include/stan4bart_amd.h ``sweep_group_*``): samplers on one device whose solo tree sweeps (n <= 4 096) go out in one
    launch, one workgroup per member.  Members are driven from their own host threads; draws are those of the ungrouped samplers."""

    STAT_NAMES = ("launches", "batched_sweeps", "unbatched_sweeps", "timeouts")

    def __init__(self, lib: C.CDLL, prefix: str, device: int = 0, max_members: int = 16):
        self._lib, self._pfx = lib, prefix
        if getattr(lib, prefix + "sweep_group_create", None) is None:
            raise RuntimeError("this stan4bart_amd library has no sweep groups (sweep_group_create)")
        vp, i32, i64 = C.c_void_p, C.c_int32, C.c_int64
        for name, argtypes in {"sweep_group_create": [i32, i32, C.POINTER(vp)], "sweep_group_join": [vp, vp], "sweep_group_leave": [vp],
                               "sweep_group_stats": [vp, C.POINTER(i64)], "sweep_group_set_timeout": [vp, C.c_double],
                               "sweep_group_free": [vp]}.items():
            fn = getattr(lib, prefix + name)
            fn.restype, fn.argtypes = C.c_int, argtypes
        getattr(lib, prefix + "last_error").restype = C.c_char_p
        self._h = C.c_void_p()
        self._check(self._f("sweep_group_create")(int(device), int(max_members), C.byref(self._h)))

    def _f(self, name):
        return getattr(self._lib, self._pfx + name)

    def _check(self, rc):
        if rc != 0:
            raise RuntimeError(self._f("last_error")().decode())

    def join(self, sampler: "Sampler"):
        self._check(self._f("sweep_group_join")(self._h, sampler._h))

    def leave(self, sampler: "Sampler"):
        if getattr(sampler, "_h", None) and sampler._h.value:
            self._check(self._f("sweep_group_leave")(sampler._h))

    def set_timeout(self, seconds: float):
        """Longest wait of a member for the others (default 30 s): after it the members present launch without the straggler."""
        self._check(self._f("sweep_group_set_timeout")(self._h, float(seconds)))

    def stats(self) -> dict:
        out = (C.c_int64 * 4)()
        self._check(self._f("sweep_group_stats")(self._h, out))
        return dict(zip(self.STAT_NAMES, (int(v) for v in out)))

    def free(self):
        if getattr(self, "_h", None) and self._h.value:
            self._check(self._f("sweep_group_free")(self._h))
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class StoredSampler:
    """``stan4bart_createStoredBARTSampler`` (reference src/init.cpp:418-446, R/stan4bart_fit.R:572-580): a sampler rebuilt
    from an exported BART state — in another process, after the fitting sampler is gone — that predicts from the kept trees."""

    def __init__(self, lib: C.CDLL, prefix: str, state: bytes, device: int = 0):
        self._lib, self._pfx = lib, prefix
        self._h = C.c_void_p()
        Sampler._bind(self)
        buf = C.create_string_buffer(state, len(state))
        self._check(self._f("create_stored_bart_sampler")(buf, C.c_int64(len(state)), C.c_int32(device), C.byref(self._h)))

    _f = Sampler._f
    _check = Sampler._check
    predict_bart = Sampler.predict_bart
    predict_summary = Sampler.predict_summary
    _summary_in = staticmethod(Sampler._summary_in)
    partial_dependence = Sampler.partial_dependence
    predict_quantiles = Sampler.predict_quantiles
    predict_contrast = Sampler.predict_contrast
    _contrast_in = Sampler._contrast_in
    group_order = staticmethod(Sampler.group_order)
    groups_draws = Sampler.groups_draws
    predict_groups = Sampler.predict_groups
    column_scales = staticmethod(Sampler.column_scales)
    projection_draws = Sampler.projection_draws
    predict_projection = Sampler.predict_projection
    spread_draws = Sampler.spread_draws
    spread_names = staticmethod(Sampler.spread_names)
    predict_spread = Sampler.predict_spread
    check_draws = Sampler.check_draws
    check_names = staticmethod(Sampler.check_names)
    predict_check = Sampler.predict_check
    curves_draws = Sampler.curves_draws
    describe_draws = Sampler.describe_draws
    predict_describe = Sampler.predict_describe
    sorted_draws = Sampler.sorted_draws
    predict_sorted = Sampler.predict_sorted
    test_sorted_select = Sampler.test_sorted_select
    predict_curves = Sampler.predict_curves
    predict_ppd = Sampler.predict_ppd
    predict_loo = Sampler.predict_loo
    predict_convergence = Sampler.predict_convergence
    export_bart_state = Sampler.export_bart_state
    get_kept_trees = Sampler.get_kept_trees
    get_kept_trees_indexed = Sampler.get_kept_trees_indexed
    print_trees = Sampler.print_trees
    free = Sampler.free

    def get_trees(self):
        return self.get_kept_trees()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
