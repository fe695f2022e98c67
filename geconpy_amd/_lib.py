"""ctypes binding of libdsge_hip.so (C ABI declared in include/dsge_hip.h).

The library is the product path; there is NO fallback.  ``load()`` raises when the shared
object is missing and every compute call raises ``DsgeHipError`` when no gfx950 device is
present (the library itself refuses with DSGE_ERR_HIP).
"""
from __future__ import annotations

import ctypes as C
import os

PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG, "libdsge_hip.so")

ABI_VERSION = 19
ERR_INVALID, ERR_HIP, ERR_TOO_LARGE = 1, 2, 3
MAX_N = 64
MAX_N_CR = 64
MAX_N_GENSYS = 64
MAX_N_BIG = 96  # cycle reduction, selection and the fused solve + Kalman logp with a cycle-reduction solver (csrc/dsge_big.hpp)
MAX_P = 16
MAX_SEGMENTS = 8  # DSGE_MAX_SEGMENTS: segments of dsge_kalman_logp_segments_batched

ST_OK = 0
ST_NOT_CONVERGED = 1
ST_NAN = 2
ST_LYAP_FAIL = 4
ST_FILTER_NONFINITE = 8
ST_GENSYS_QZ_FAIL = 16
ST_GENSYS_TOO_BIG = 32
ST_GRAD_UNSUPPORTED = 64
ST_SECOND_ORDER_UNSUPPORTED = 128
ST_SMOOTHER_SINGULAR = 256
ST_COND_SINGULAR = 512
ST_SPECTRAL_SINGULAR = 1024
ST_ANTICIPATION_SINGULAR = 2048
ANT_PERFECT_FORESIGHT, ANT_NEWS = 0, 1  # DSGE_ANT_*: the information structures of dsge_anticipated_paths_batched
ANT_MAX_LEAD = 63
ST_CONSTRAINT_UNRESOLVED = 4096
OBC_NO_REGIME, OBC_SINGULAR, OBC_BEYOND_HORIZON, OBC_SKIPPED = 1, 2, 4, 8  # DSGE_OBC_*: the bits of a path of dsge_constrained_paths_batched
OBC_HORIZON_SHORT = 16  # a bit of a path of dsge_constrained_simulate_batched alone
OBC_MAX_HORIZON = 64

Q_DIAG_SHARED, Q_DIAG_BATCHED, Q_FULL_SHARED, Q_FULL_BATCHED = 0, 1, 2, 3
SOLVER_CYCLE_REDUCTION, SOLVER_GENSYS, SOLVER_BACKWARD_DIRECT, SOLVER_SCAN_CYCLE_REDUCTION = 0, 1, 2, 3
SOLVER_FLAG_ZERO_T_ON_FAILURE = 0x100  # include/dsge_hip.h: DSGE_SOLVER_FLAG_ZERO_T_ON_FAILURE
SOLVER_CODES = {
    "cycle_reduction": SOLVER_CYCLE_REDUCTION,
    "gensys": SOLVER_GENSYS,
    "backward_direct": SOLVER_BACKWARD_DIRECT,
    "scan_cycle_reduction": SOLVER_SCAN_CYCLE_REDUCTION,
}


class DsgeHipError(RuntimeError):
    code = None  # the library's return code (DSGE_ERR_*), when the error came from a call


class DsgeTooLargeError(DsgeHipError):
    """DSGE_ERR_TOO_LARGE: a well-formed call whose problem exceeds the entry point's on-chip capacity."""


class DsgeNoVerdictError(DsgeHipError):
    """``eu = [-3, -3, 0]``: gensys on a model with 65 .. 96 variables (solved by spectral division, csrc/dsge_big.hpp) whose draw
    is NOT certified regular -- not converged, a root within 2e-4 of the unit circle, a scale the reference's absolute tolerances
    would notice -- and there is no ordered QZ at that size to issue the reference's verdict ([1, 0, k], [0, 1, 0], [-2, -2, 0],
    or [1, 1, 0] for a regular draw close to the unit circle).  The reference never returns -3; the batched entry points report
    it per draw (status NOT_CONVERGED | GENSYS_TOO_BIG, T = R = 0), the single-model wrappers raise this."""


EU_NO_VERDICT = -3  # eu[0] = eu[1] = -3: see DsgeNoVerdictError


class GensysForward(C.Structure):
    """``dsge_gensys_forward`` of include/dsge_hip.h (addresses; 0 = not wanted)."""

    _fields_ = [("f_mat", C.c_void_p), ("f_wt", C.c_void_p), ("y_wt", C.c_void_p), ("loose", C.c_void_p),
                ("n_unstable", C.c_void_p), ("pi_raw", C.c_int32)]


# ---- the C ABI, by name ------------------------------------------------------------------------------------------------------
# entry -> its argument names in the order of include/dsge_hip.h (tests/test_abi_and_host.py compares both, names and kinds).  A
# name is an int, a double or a size_t when it is listed below, a pointer (double* / int32_t* / struct* / stream, passed as a raw
# host or device address) otherwise; a leading "*" marks the two names that are a pointer here and an int elsewhere.
_INTS = ("N T_len batch bound_batched c c_batched correlation cv_batched cv_paths d_batched device enable eps_batched "
         "eta_batched full_cov h_batched horizon k lag_step m max_iter mode n n_cond n_eta n_filter_hint n_grid n_groups n_lags "
         "n_lead n_lead_hint n_links n_out n_paths n_ret n_seg n_shock_steps n_state n_state_hint n_steps nnz p q_batched q_mode "
         "remainder reps s_batched shock solver w_batched x0_batched x0_paths z_batched z_selector_hint")
_KINDS = {**dict.fromkeys(_INTS.split(), C.c_int), **dict.fromkeys("jitter missing_fill rank_tol tol".split(), C.c_double),
          "scratch_limit_bytes": C.c_size_t}
_OBS = "Z z_batched d d_batched Hdiag h_batched"
_FILTER = f"T R Q q_mode {_OBS} y batch m k p T_len jitter missing_fill"
_FUSED = f"A B C D Q q_mode {_OBS} y batch n k p T_len solver tol max_iter jitter missing_fill"
_LOGP = f"{_FUSED} n_state_hint z_selector_hint n_lead_hint logp_out status_out"
_GRAD = f"A B C D q q_batched {_OBS} y batch n k p T_len solver tol max_iter jitter missing_fill"
_BARS = "logp_out status_out A_bar B_bar C_bar D_bar q_bar d_bar h_bar"
_PRUNED = "T R gyy gyu guu gss state_idx n_state"  # what the second-order entry returns, as it returns it
_PENCIL = "g0 g1 *c psi pi batch N k n_eta tol G1_out C_out impact_out gev_out eu_out status"
_DEVICE_ENTRIES = {
    "dsge_abi_version": "",
    "dsge_last_error": "",
    "dsge_device_count": "",
    "dsge_set_device": "device",
    "dsge_stream_synchronize": "stream",
    "dsge_options_init": "opt",
    "dsge_options_push": "opt",
    "dsge_options_pop": "",
    "dsge_forget_measured_shapes": "",
    "dsge_debug_cr_phases": "enable cycles_out",
    "dsge_debug_cr_fused_phases": "enable cycles_out",
    "dsge_debug_kalman_steady_steps": "steady_at_device",
    "dsge_debug_kalman_timeline": "timeline_device",
    "dsge_debug_kalman_phases": "enable cycles_out",
    "dsge_debug_big_phases": "enable cycles_out",
    "dsge_debug_gensys_phases": "A B C batch n tol n_lead_hint T_out eu_out status cycles_out",
    "dsge_debug_gensys_window_phases": "enable cycles_out",
    "dsge_debug_gensys_stage_ms": "enable ms_out",
    "dsge_debug_adjoint_refine": "mode",
    "dsge_debug_cr_static_rows": "mode",
    "dsge_debug_cr_refine": "mode",
    "dsge_debug_second_order_phases": "enable cycles_out",
    "dsge_debug_pruned_phases": "enable cycles_out",
    "dsge_debug_shock_decomp_phases": "enable cycles_out",
    "dsge_debug_condfc_phases": "enable cycles_out",
    "dsge_profile_pipeline": f"{_LOGP} reps ms_out stream",
    # every entry below has a host twin (``host_twin``)
    "dsge_cycle_reduction_batched": "A B C batch n max_iter tol T_out status n_iter stream",
    "dsge_scan_cycle_reduction_batched": "A B C batch n max_iter tol T_out status *n_steps stream",
    "dsge_gensys_batched": "A B C D batch n k tol n_lead_hint T_out R_out eu_out status stream",
    "dsge_gensys_pencil_batched": f"{_PENCIL} stream",
    "dsge_gensys_pencil_full_batched": f"{_PENCIL} forward stream",
    "dsge_bk_eigenvalues_batched": "A B C batch n tol eig_re eig_im n_eig n_forward n_unstable status stream",
    "dsge_selection_batched": "A B C D T batch n k R_out resid_out stream",
    "dsge_policy_adjoints_batched": "B C T T_bar batch n A_bar B_bar C_bar status stream",
    "dsge_selection_adjoints_batched": "B C T R R_bar batch n k B_bar C_bar D_bar T_bar stream",
    "dsge_policy_norms_batched": "A B C D T R state_mask batch n k det_norm_out stoch_norm_out stream",
    "dsge_backward_direct_batched": "A B D batch n k T_out R_out stream",
    "dsge_lyapunov_batched": "T R Q q_mode batch m k P0_out RQR_out status stream",
    "dsge_autocorrelation_batched": "T R Q q_mode Z Hdiag batch m k p n_lags lag_step correlation acf_out Sigma_out status stream",
    "dsge_kalman_logp_batched": f"{_FILTER} n_state_hint z_selector_hint logp_out status_io stream",
    "dsge_kalman_filter_outputs_batched": f"{_FILTER} ll_out a_pred_out a_filt_out p_pred_out p_filt_out full_cov status_io stream",
    "dsge_kalman_logp_segments_batched": (f"T R Q q_mode {_OBS} a0 P0 shift y seg_start n_seg batch m k p T_len jitter missing_fill "
                                          "logp_out ll_out a_last_out P_last_out status_io stream"),
    "dsge_kalman_smoother_batched": (f"{_FILTER} rank_tol scratch_limit_bytes ll_out a_smooth_out p_smooth_out eps_smooth_out "
                                     "full_cov status_io stream"),
    "dsge_kalman_smoother_segments_batched": (f"T R Q q_mode {_OBS} a0 P0 shift y seg_start n_seg batch m k p T_len jitter missing_fill "
                                              "rank_tol scratch_limit_bytes full_cov ll_out a_pred_out a_filt_out p_pred_out p_filt_out "
                                              "a_smooth_out p_smooth_out eps_smooth_out status_io stream"),
    "dsge_kalman_logp_segments_grad_batched": (f"T R Q q_mode {_OBS} a0 P0 shift y seg_start n_seg batch m k p T_len jitter missing_fill "
                                               "scratch_limit_bytes logp_out T_bar R_bar Q_bar Z_bar d_bar h_bar shift_bar a0_bar P0_bar "
                                               "status_io stream"),
    "dsge_simulation_smoother_batched": (f"{_FILTER} rank_tol scratch_limit_bytes x0 x0_batched eps eps_batched eta eta_batched "
                                         "n_paths ll_out x_out eps_out status_io stream"),
    "dsge_simulate_batched": "T R eps eps_batched x0 x0_batched status batch m k n_paths n_steps n_shock_steps x_out stream",
    "dsge_irf_batched": "T R S s_batched weights w_batched status batch m k c n_steps irf_out fevd_out stream",
    "dsge_forecast_batched": f"T R Q q_mode {_OBS} a0 P0 status batch m k p n_steps a_out p_out full_cov y_out f_out stream",
    "dsge_simulate_pruned_batched": (f"{_PRUNED} eps eps_batched xf0 xs0 x0_batched status batch n k n_paths n_steps n_shock_steps "
                                     "x_out xf_out xs_out stream"),
    "dsge_girf_pruned_batched": (f"{_PRUNED} S_imp s_batched c eps eps_batched xf0 xs0 x0_batched status batch n k n_paths n_steps "
                                 "n_shock_steps girf_out stream"),
    "dsge_shock_decomposition_batched": ("T R eps x group_of_shock n_groups var_idx n_out Z z_batched status batch m k p n_paths T_len "
                                         "remainder contrib_out obs_out stream"),
    "dsge_conditional_forecast_batched": ("T R Q q_mode Z z_batched d d_batched x0 x0_batched x0_paths eps eps_batched cond_t cond_j "
                                          "n_cond cond_val cv_batched cv_paths free_shock status_io batch m k p n_paths n_steps "
                                          "n_shock_steps rank_tol x_out eps_out obs_out stream"),
    "dsge_spectral_moments_batched": ("T R Q q_mode Z z_batched Hdiag h_batched gain batch m k p n_grid n_lags correlation rank_tol "
                                      "scratch_limit_bytes acov_out spectrum_out status_io stream"),
    "dsge_anticipated_paths_batched": ("B C T R eps eps_batched mode n_lead x0 x0_batched x0_paths Z z_batched d d_batched status_io "
                                       "batch n k p n_paths n_steps n_shock_steps rank_tol x_out w_out obs_out G_out stream"),
    "dsge_constrained_paths_batched": ("B C T R eps eps_batched x0 x0_batched x0_paths Z z_batched d d_batched c_row c_batched bound "
                                       "bound_batched shock horizon max_iter status_io batch n k p n_paths n_steps n_shock_steps rank_tol "
                                       "x_out w_out obs_out nu_out gap_out Mz_out path_status_out iters_out stream"),
    "dsge_constrained_simulate_batched": ("B C T R eps eps_batched x0 x0_batched x0_paths Z z_batched d d_batched c_row c_batched "
                                          "bound bound_batched shock horizon max_iter status_io batch n k p n_paths n_steps "
                                          "n_shock_steps rank_tol x_out obs_out gap_out shadow_out plan_out duration_out iters_out "
                                          "Mz_out path_status_out fail_step_out stream"),
    "dsge_solve_kalman_logp_batched": f"{_LOGP} T_out R_out resid_out n_iter_out stream",
    "dsge_solve_kalman_logp_batched_opt": f"opt {_LOGP} T_out R_out resid_out n_iter_out stream",
    "dsge_solve_kalman_logp_augmented_batched": (f"{_FUSED} m inv_var_order n_links link_rows link_cols n_state_hint z_selector_hint "
                                                 "n_lead_hint logp_out status_out T_aug_out R_aug_out resid_out stream"),
    "dsge_solve_kalman_logp_grad_batched": f"{_GRAD} n_filter_hint n_lead_hint {_BARS} stream",
    "dsge_solve_kalman_logp_grad_batched_opt": f"opt {_GRAD} n_filter_hint n_lead_hint {_BARS} stream",
    "dsge_solve_kalman_logp_grad_dense_z_batched": f"{_GRAD} n_state_hint n_lead_hint {_BARS} Z_bar stream",
    "dsge_second_order_logp_batched": ("A B C D hess_idx nnz hess_val q q_batched Z d Hdiag y batch n k p T_len solver tol max_iter "
                                       "jitter missing_fill state_idx n_state lead_idx n_lead ret_idx n_ret logp_out status_out "
                                       "T_out R_out gyy_out gyu_out guu_out gss_out stage_ms stream"),
}
_HOST_DROPS = {"dsge_second_order_logp_batched": 2}  # trailing arguments a host twin does not take: ``stream``; here ``stage_ms`` too


def host_twin(entry):
    """Name of the twin of a device entry that takes host pointers and stages through device memory."""
    return entry[:-4] + "_host_opt" if entry.endswith("_opt") else entry + "_host"


# name -> ((argument name, ctypes type), ...); every symbol include/dsge_hip.h declares must appear here
SIGNATURES = {name: tuple((w[1:], C.c_void_p) if w[0] == "*" else (w, _KINDS.get(w, C.c_void_p)) for w in sig.split())
              for name, sig in _DEVICE_ENTRIES.items()}
SIGNATURES.update({host_twin(name): SIGNATURES[name][:-_HOST_DROPS.get(name, 1)]
                   for name in _DEVICE_ENTRIES if "_batched" in name})
PROTOTYPES = {name: [kind for _, kind in sig] for name, sig in SIGNATURES.items()}  # name -> argtypes


class Options(C.Structure):
    """``dsge_options`` of include/dsge_hip.h: the kernel-variant switches and the filter conventions of ONE call (per call /
    per host thread; there is no process-wide mutable state since ABI 8)."""

    _fields_ = [
        ("struct_size", C.c_uint32),
        ("cr_compact", C.c_int32),
        ("cr_fused_selection", C.c_int32),
        ("cr_deflation", C.c_int32),
        ("cr_two_waves", C.c_int32),
        ("n_static_hint", C.c_int32),
        ("kalman_order", C.c_int32),
        ("kalman_tiny", C.c_int32),
        ("kalman_block", C.c_int32),
        ("kalman_mfma", C.c_int32),
        ("pipeline_chunks", C.c_int32),
        ("gensys_split", C.c_int32),
        ("kalman_steady_tol", C.c_double),
        ("kalman_nt_products", C.c_int32),
        ("cr_fused_deflation", C.c_int32),
        ("cr_four_waves", C.c_int32),
        ("gensys_real_stage", C.c_int32),
        ("gensys_pairs", C.c_int32),
        ("gensys_shape_cache", C.c_int32),
        ("kalman_narrow", C.c_int32),
        ("gensys_direct_blocks", C.c_int32),
        # ABI 8: conventions of the filter step (third party: pymc_extras)
        ("ll_constant", C.c_int32),
        ("mask_d", C.c_int32),
        ("joseph", C.c_int32),
        ("kalman_head_draws", C.c_int32),
        ("jitter_F", C.c_double),
        ("jitter_P", C.c_double),
        ("gensys_doubling", C.c_int32),
        ("kalman_grad_split", C.c_int32),
        ("reserved_", C.c_int32 * 2),
    ]


LL_CONSTANT = {"p": 0, "observed": 1, "one": 2}  # DSGE_LL_CONST_* (include/dsge_hip.h)


def filter_conventions(ll_constant="p", jitter_on_F=True, jitter_on_P=True, mask_d=False, joseph=True):
    """``dsge_options`` fields for one combination of the third-party conventions of the "standard" filter step, named as
    ``oracle.FilterConventions`` names them (so that the combination tests/test_oracle_kalman.py::test_pymc_extras_pin reports
    for a real pymc_extras install is pasted here verbatim): ``options=filter_conventions(ll_constant="one")``.  A jitter that
    is "on" is the call's ``jitter`` argument (``jitter_F = -1``), "off" is 0."""
    return {"ll_constant": LL_CONSTANT[ll_constant], "jitter_F": -1.0 if jitter_on_F else 0.0,
            "jitter_P": -1.0 if jitter_on_P else 0.0, "mask_d": int(bool(mask_d)), "joseph": int(bool(joseph))}


def make_options(options=None, **fields):
    """A ``dsge_options`` holding the compiled-in defaults with ``fields`` (or the dict ``options``) applied;
    an ``Options`` instance is passed through.  ``ll_constant`` also takes the names "p" / "observed" / "one"."""
    if isinstance(options, Options) and not fields:
        return options
    o = Options()
    check(load().dsge_options_init(C.addressof(o)))
    if isinstance(options, Options):
        C.memmove(C.addressof(o), C.addressof(options), C.sizeof(Options))
    elif options:
        fields = {**options, **fields}
    for name, value in fields.items():
        if name not in {f[0] for f in Options._fields_} or name in ("struct_size", "reserved_"):
            raise ValueError(f"unknown option {name!r}")
        if name == "ll_constant" and isinstance(value, str):
            value = LL_CONSTANT[value]
        setattr(o, name, value)
    return o


def opt_ptr(options):
    """(address or None, keep-alive object) for the ``*_opt`` entry points."""
    if options is None:
        return None, None
    o = make_options(options)
    return C.addressof(o), o


class options_scope:
    """``with options_scope(opts): ...`` -- every library call this THREAD makes inside uses ``opts``
    (dsge_options_push / dsge_options_pop); ``None`` is a no-op."""

    def __init__(self, options):
        self.options = None if options is None else make_options(options)

    def __enter__(self):
        if self.options is not None:
            check(load().dsge_options_push(C.addressof(self.options)))
        return self.options

    def __exit__(self, *exc):
        if self.options is not None:
            check(load().dsge_options_pop())
        return False


_lib = None


def load():
    """Load (once) and return the ctypes handle.  Loading does not touch the GPU."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise DsgeHipError(
            f"{LIB_PATH} is missing: build it with `python -m geconpy_amd.build` "
            "(there is no CPU fallback for the HIP engine)"
        )
    # One HIP runtime per process: the PyTorch-ROCm wheel bundles its own libamdhip64 (soname
    # libamdhip64.so.7, but linked by the name "libamdhip64.so").  If this library were loaded
    # first it would pull /opt/rocm's copy and a later `import torch` would load a SECOND
    # runtime, after which one of the two sees no device.  Importing torch first makes our
    # NEEDED libamdhip64.so.7 resolve to the runtime torch already loaded.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    for name, argtypes in PROTOTYPES.items():
        fn = getattr(lib, name)  # AttributeError here = header/library mismatch
        fn.argtypes = argtypes
        fn.restype = {"dsge_last_error": C.c_char_p}.get(name, C.c_int)
    if lib.dsge_abi_version() != ABI_VERSION:
        raise DsgeHipError("libdsge_hip ABI version mismatch")
    _lib = lib
    return lib


def check(rc):
    if rc != 0:
        msg = load().dsge_last_error()
        cls = DsgeTooLargeError if rc == ERR_TOO_LARGE else DsgeHipError
        err = cls(f"libdsge_hip call failed (code {rc}): {msg.decode() if msg else '?'}")
        err.code = rc
        raise err


_TO_C = {C.c_int: int, C.c_size_t: int, C.c_double: float}


def call(entry, *, host, stream=None, **named):
    """Call the device entry ``entry`` (``host=False``: ``stream`` is appended) or its host twin with the arguments given BY NAME,
    ordered by ``SIGNATURES``; a missing or an unknown name is a ``TypeError``, a non-zero return code raises (``check``).  What
    a host twin does not take (``stream``; second order: ``stage_ms``) may be passed to it as None only."""
    name = host_twin(entry) if host else entry
    sig = SIGNATURES[name]
    named["stream"] = stream
    if host:
        for dropped, _ in SIGNATURES[entry][len(sig):]:
            if named.pop(dropped, None) is not None:
                raise TypeError(f"{name} takes no {dropped}")
    names = {arg for arg, _ in sig}
    if named.keys() != names:
        raise TypeError(f"{name}: missing {sorted(names - named.keys())}, unknown {sorted(named.keys() - names)}")
    check(getattr(load(), name)(*[named[arg] if kind is C.c_void_p else _TO_C[kind](named[arg]) for arg, kind in sig]))


def device_count():
    return load().dsge_device_count()
