"""ctypes binding of the C ABI (include/dlm_engine.h).  Fails loudly when the HIP engine
library is missing or cannot be loaded: there is no CPU fallback in the product path."""
import ctypes
import os

HERE = os.path.dirname(os.path.abspath(__file__))
# DLM_ENGINE_LIB selects an alternative build of the same C ABI (kernel A/B experiments)
LIB_PATH = os.environ.get("DLM_ENGINE_LIB") or os.path.join(HERE, "libdlm_engine.so")

DLM_MEM_DEVICE, DLM_MEM_HOST = 0, 1
OPT_SMOOTHER_COMPAT_Q1 = 1 << 0
OPT_SVD_RAW_W_Q2 = 1 << 1
OPT_SVD_SAMPLER_Q9 = 1 << 2
OPT_FORCE_GENERIC = 1 << 3
OPT_STATS_OUTER = 1 << 4
OPT_ASYNC = 1 << 5
OPT_FFBS_SIMSMOOTH = 1 << 6
OPT_PACKED_SYM = 1 << 7
OPT_MODEL_UNCHANGED = 1 << 8
OPT_COUNT_STEPS = 1 << 9
OPT_TRUST_MODEL_UNCHANGED = 1 << 10
OPT_LOGLIK_LITERAL_Q7 = 1 << 11
OPT_STUDENTT_LITERAL = 1 << 12
OPT_NO_LANE = 1 << 16
OPT_NO_SAMPLER16 = 1 << 17
OPT_NO_WAVE = 1 << 18
OPT_FORCE_WAVE = 1 << 19
OPT_NO_SPARSE_F = 1 << 20
OPT_NO_SMALL_BATCH = 1 << 21
OPT_NO_STEADY = 1 << 22
OPT_NO_PIPE = 1 << 23
OPT_SHARED_COV = 1 << 24
OPT_SVD_PER_SERIES = 1 << 25
OPT_SAMPLER_PER_SERIES = 1 << 26
OPT_DRAW_EIG = 1 << 27
OPT_SMOOTHER_PER_SERIES = 1 << 28
OPT_NO_TABLE_REUSE = 1 << 29
OPT_TEST_FAIL_AFTER_TABLES = 1 << 30
TABLES_NONE, TABLES_BUILT, TABLES_REUSED, TABLES_SKIPPED = 0, 1, 2, 3   # dlm_last_table_reuse
ST_NONFINITE, ST_NOT_PD, ST_NOCONV = 1, 2, 4
COMM_ID_BYTES = 128
# dlm_pf_desc.family: the observation models of the particle filter (Dglm.scala:46-175, package.scala:13-28)
OBS_GAUSSIAN, OBS_POISSON, OBS_NEGBIN, OBS_ZIP, OBS_STUDENTT, OBS_BETA = range(6)
PF_MAX_D, PF_MIN_PARTICLES, PF_MAX_PARTICLES = 16, 64, 1024
PF_MAX_T = 0x1FFFFE           # DLM_PF_MAX_T: the Philox counter's slot field
PF_FORECAST_MAX_RANKS = 8     # dlm_pf_forecast_desc.n_ranks
# dlm_resample_desc.scheme: the ancestor step of the particle filter's resampling (dlm_pf_resampled)
RESAMPLE_MULTINOMIAL, RESAMPLE_STRATIFIED, RESAMPLE_SYSTEMATIC, RESAMPLE_METROPOLIS = range(4)
PF_MAX_MH_STEPS = 64          # DLM_PF_MAX_MH_STEPS: dlm_resample_desc.mh_steps under RESAMPLE_METROPOLIS

_dp = ctypes.POINTER(ctypes.c_double)
_ip = ctypes.POINTER(ctypes.c_int32)


class ModelDesc(ctypes.Structure):
    _fields_ = [("d", ctypes.c_int32), ("p", ctypes.c_int32), ("T", ctypes.c_int32), ("N", ctypes.c_int32),
                ("F", ctypes.c_void_p), ("f_stride", ctypes.c_int64),
                ("G", ctypes.c_void_p), ("n_g", ctypes.c_int32), ("g_index", ctypes.c_void_p),
                ("dt", ctypes.c_void_p)]


class ParamsDesc(ctypes.Structure):
    _fields_ = [("V", ctypes.c_void_p), ("v_stride", ctypes.c_int64),
                ("W", ctypes.c_void_p), ("w_stride", ctypes.c_int64),
                ("m0", ctypes.c_void_p), ("m0_stride", ctypes.c_int64),
                ("C0", ctypes.c_void_p), ("c0_stride", ctypes.c_int64),
                ("v_tstride", ctypes.c_int64), ("w_tstride", ctypes.c_int64)]


class StudentTPrior(ctypes.Structure):
    _fields_ = [("prior_nu_rate", ctypes.c_double), ("prop_nu_size", ctypes.c_double),
                ("prior_w_shape", ctypes.c_double), ("prior_w_scale", ctypes.c_double)]


class SvPrior(ctypes.Structure):
    """dlm_sv_prior: phi_update 0 = Gaussian(phi_a = mean, phi_b = sd) conjugate, 1 = Beta(phi_a, phi_b) prior with the Beta proposal."""
    _fields_ = [("phi_update", ctypes.c_int32), ("literal", ctypes.c_int32),
                ("phi_a", ctypes.c_double), ("phi_b", ctypes.c_double),
                ("mu_mean", ctypes.c_double), ("mu_sd", ctypes.c_double),
                ("sigma_shape", ctypes.c_double), ("sigma_scale", ctypes.c_double),
                ("prop_lambda", ctypes.c_double), ("prop_tau", ctypes.c_double)]


class SvOuPrior(ctypes.Structure):
    """dlm_sv_ou_prior: Beta(phi_a, phi_b) prior of the rate, Gaussian(mean, sd) of mu, InverseGamma(shape, scale) of sigma_eta ITSELF,
    the Beta proposal's (lambda, tau) and the two random walks' standard deviations."""
    _fields_ = [("literal", ctypes.c_int32),
                ("phi_a", ctypes.c_double), ("phi_b", ctypes.c_double),
                ("mu_mean", ctypes.c_double), ("mu_sd", ctypes.c_double),
                ("sigma_shape", ctypes.c_double), ("sigma_scale", ctypes.c_double),
                ("prop_lambda", ctypes.c_double), ("prop_tau", ctypes.c_double),
                ("delta_sigma", ctypes.c_double), ("delta_mu", ctypes.c_double)]


class FsvPrior(ctypes.Structure):
    """dlm_fsv_prior: Gaussian(beta_mean, beta_sd) prior of the free loadings (the standard deviation, as Breeze takes it),
    InverseGamma(sigma_shape, sigma_scale) of the observation variance sigma^2; literal = 1: the reference's arithmetic (Q27-Q30)."""
    _fields_ = [("literal", ctypes.c_int32),
                ("beta_mean", ctypes.c_double), ("beta_sd", ctypes.c_double),
                ("sigma_shape", ctypes.c_double), ("sigma_scale", ctypes.c_double)]


class PfDesc(ctypes.Structure):
    """dlm_pf_desc: the observation family (OBS_*), the number of particles (a multiple of 64, 64..1024), n0 (resample when ESS < n0;
    negative: floor(P / 5) as ParticleFilter.likelihood) and literal = 1: the reference's arithmetic (Q37-Q39)."""
    _fields_ = [("family", ctypes.c_int32), ("n_particles", ctypes.c_int32), ("n0", ctypes.c_int32), ("literal", ctypes.c_int32)]


class ResampleDesc(ctypes.Structure):
    """dlm_resample_desc: the scheme (RESAMPLE_*) and the steps of a Metropolis chain, 1..PF_MAX_MH_STEPS under RESAMPLE_METROPOLIS and 0
    under every other scheme."""
    _fields_ = [("scheme", ctypes.c_int32), ("mh_steps", ctypes.c_int32)]


class PfForecastDesc(ctypes.Structure):
    """dlm_pf_forecast_desc: the observation family (OBS_*), the number of particles, literal = 1 (Q38, Q39), the number of order statistics per
    time (0..PF_FORECAST_MAX_RANKS) and the Philox slot of the first forecast step."""
    _fields_ = [("family", ctypes.c_int32), ("n_particles", ctypes.c_int32), ("literal", ctypes.c_int32), ("n_ranks", ctypes.c_int32),
                ("slot_offset", ctypes.c_int64)]


FC_VAR, FC_LOGVAR, FC_IG_SCALE = range(3)   # DLM_FC_*: what the rows of pw and pv of dlm_pf_forecast_learned hold


class PfForecastLearnedDesc(ctypes.Structure):
    """dlm_pf_forecast_learned_desc: the observation family (OBS_*), the number of particles, var_kind (FC_*: the particles' rows are
    variances, log-variances or InverseGamma scales), the number of order statistics per time (0..PF_FORECAST_MAX_RANKS) and the Philox slot
    of the first forecast step."""
    _fields_ = [("family", ctypes.c_int32), ("n_particles", ctypes.c_int32), ("var_kind", ctypes.c_int32), ("n_ranks", ctypes.c_int32),
                ("slot_offset", ctypes.c_int64)]


def pf_forecast_learned_lds_bytes(d: int, n_particles: int) -> int:
    """pf_forecast_learned_lds_bytes of dlm_pf_forecast_learned.hip: the LDS dlm_pf_forecast_learned needs for (d, P)."""
    return (2 * d + 3) * n_particles * 8 + 4 * n_particles


class StorvikDesc(ctypes.Structure):
    """dlm_storvik_desc: dlm_pf_desc's fields (literal = 1: Q39 and Q43) and learn_v = 1: V is learned too (OBS_GAUSSIAN only)."""
    _fields_ = [("family", ctypes.c_int32), ("n_particles", ctypes.c_int32), ("n0", ctypes.c_int32), ("literal", ctypes.c_int32),
                ("learn_v", ctypes.c_int32)]


class LwDesc(ctypes.Structure):
    """dlm_lw_desc: dlm_storvik_desc's fields (literal = 1: Q39, Q50 and Q51; learn_v = 1: log V is learned too, for OBS_GAUSSIAN,
    OBS_STUDENTT and OBS_BETA) and the shrinkage a, 0 < a <= 1."""
    _fields_ = [("family", ctypes.c_int32), ("n_particles", ctypes.c_int32), ("n0", ctypes.c_int32), ("literal", ctypes.c_int32),
                ("learn_v", ctypes.c_int32), ("a", ctypes.c_double)]


class RbDesc(ctypes.Structure):
    """dlm_rb_desc: the number of particles, n0, literal = 1 (Q50, Q57 and Q58), learn_v = 1 (log V is learned too) and the shrinkage a,
    0 < a <= 1.  The family is Gaussian."""
    _fields_ = [("n_particles", ctypes.c_int32), ("n0", ctypes.c_int32), ("literal", ctypes.c_int32), ("learn_v", ctypes.c_int32),
                ("a", ctypes.c_double)]


class PgDesc(ctypes.Structure):
    """dlm_pg_desc: the observation family (OBS_*), the number of particles (the reference particle included), ancestor_sampling = 1
    (0: plain conditional SMC) and the bytes of engine workspace a launch may take (0: PG_WORKSPACE_CAP)."""
    _fields_ = [("family", ctypes.c_int32), ("n_particles", ctypes.c_int32), ("ancestor_sampling", ctypes.c_int32),
                ("workspace_cap", ctypes.c_int64)]


PG_WORKSPACE_CAP = 8 << 30   # DLM_PG_WORKSPACE_CAP
RB_LDS_BYTES = 160 * 1024   # the LDS of a workgroup on gfx950


def rb_lds_bytes(d: int, n_particles: int) -> int:
    """rb_lds_bytes of dlm_rb.hip: the LDS dlm_rb_batch needs for (d, P)."""
    tri = d * (d + 1) // 2
    return ((tri + 2 * d + 3) * n_particles + 64 * tri + 3 * d + 1) * 8 + 4 * n_particles


class MixtureDesc(ctypes.Structure):
    """dlm_mixture_desc: rows, components per row, times, dimension, the number of quantiles, and the row, component and time strides
    (in doubles) of f and of Q."""
    _fields_ = [("N", ctypes.c_int32), ("C", ctypes.c_int32), ("H", ctypes.c_int32), ("p", ctypes.c_int32), ("nq", ctypes.c_int32),
                ("f_nstride", ctypes.c_int64), ("f_cstride", ctypes.c_int64), ("f_tstride", ctypes.c_int64),
                ("q_nstride", ctypes.c_int64), ("q_cstride", ctypes.c_int64), ("q_tstride", ctypes.c_int64)]


SVPATH_MAX_H, SVPATH_MAX_R = 0x1FFFFF, 1024   # DLM_SVPATH_MAX_H, DLM_SVPATH_MAX_R (dlm_draws.h)
MIX_MAX_P, MIX_MAX_NQ, MIX_LDS_C, MIX_MAX_C = 64, 8, 4096, 1 << 30   # DLM_MIX_MAX_P, DLM_MIX_MAX_NQ, DLM_MIX_LDS_C, DLM_MIX_MAX_C (dlm_internal.h)


class Options(ctypes.Structure):
    _fields_ = [("flags", ctypes.c_uint32), ("mem", ctypes.c_int32),
                ("seed", ctypes.c_uint64), ("series_offset", ctypes.c_uint64)]


# every symbol include/dlm_engine.h declares: (name, restype, argtypes)
_V = ctypes.c_void_p
_MP, _PP, _OP = ctypes.POINTER(ModelDesc), ctypes.POINTER(ParamsDesc), ctypes.POINTER(Options)
SYMBOLS = [
    ("dlm_engine_create", ctypes.c_int, [ctypes.c_int, ctypes.POINTER(_V)]),
    ("dlm_engine_destroy", None, [_V]),
    ("dlm_last_error", ctypes.c_char_p, [_V]),
    ("dlm_version", ctypes.c_char_p, []),
    ("dlm_engine_set_stream", ctypes.c_int, [_V, _V]),
    ("dlm_engine_sync", ctypes.c_int, [_V]),
    ("dlm_last_variant", ctypes.c_char_p, [_V]),
    ("dlm_engine_wait_stream", ctypes.c_int, [_V, _V]),
    ("dlm_stream_wait_engine", ctypes.c_int, [_V, _V]),
    ("dlm_buffer_alloc", ctypes.c_int, [_V, ctypes.c_uint64, ctypes.POINTER(_V)]),
    ("dlm_buffer_free", ctypes.c_int, [_V, _V]),
    ("dlm_buffer_upload", ctypes.c_int, [_V, _V, ctypes.c_uint64, _V, ctypes.c_uint64]),
    ("dlm_buffer_download", ctypes.c_int, [_V, _V, ctypes.c_uint64, _V, ctypes.c_uint64]),
    ("dlm_buffer_fill", ctypes.c_int, [_V, _V, ctypes.c_uint64, ctypes.c_int, ctypes.c_uint64]),
    ("dlm_device_mem_info", ctypes.c_int, [_V, ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_uint64)]),
    ("dlm_packed_record_doubles", ctypes.c_int32, [ctypes.c_int32]),
    ("dlm_unpack_records", ctypes.c_int, [_V, ctypes.c_int32, ctypes.c_int64, _V, _OP, _V]),
    ("dlm_filter_batch", ctypes.c_int, [_V, _MP, _PP, _V, _OP, _V, _V, _V, _V]),
    ("dlm_loglik_batch", ctypes.c_int, [_V, _MP, _PP, _V, _OP, _V, _V]),
    ("dlm_simulate_batch", ctypes.c_int, [_V, _MP, _PP, _OP, _V, _V, _V]),
    ("dlm_dinvgamma_step_batch", ctypes.c_int, [_V, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _V, ctypes.c_double,
                                                ctypes.c_double, ctypes.c_double, ctypes.c_double, ctypes.c_uint64, _OP, _V, _V]),
    ("dlm_studentt_step_batch", ctypes.c_int, [_V, _MP, _V, _V, _V, ctypes.POINTER(StudentTPrior), _V, _V, ctypes.c_uint64, _OP,
                                               _V, _V, _V, _V, _V, _V, _V]),
    ("dlm_sv_mixture_batch", ctypes.c_int, [_V, ctypes.c_int32, ctypes.c_int32, _V, _V, ctypes.c_uint64, _OP, _V, _V, _V, _V]),
    ("dlm_sv_params_batch", ctypes.c_int, [_V, ctypes.c_int32, ctypes.c_int32, _V, _V, ctypes.POINTER(SvPrior), ctypes.c_uint64, _OP,
                                           _V, _V, _V]),
    ("dlm_sv_ou_params_batch", ctypes.c_int, [_V, ctypes.c_int32, ctypes.c_int32, _V, _V, _V, ctypes.POINTER(SvOuPrior), ctypes.c_uint64,
                                              _OP, _V, _V, _V]),
    ("dlm_sv_knots_batch", ctypes.c_int, [_V, ctypes.c_int32, ctypes.c_int32, _V, _V, ctypes.c_int32, _V, ctypes.c_int64, ctypes.c_uint64, _OP,
                                          _V, _V, _V]),
    ("dlm_fsv_factors_batch", ctypes.c_int, [_V, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _V, _V, _V, _V, ctypes.c_int32,
                                             ctypes.c_uint64, _OP, _V, _V]),
    ("dlm_fsv_loadings_batch", ctypes.c_int, [_V, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _V, _V, _V, _V,
                                              ctypes.POINTER(FsvPrior), ctypes.c_uint64, _OP, _V, _V, _V]),
    ("dlm_dlmfsv_center_batch", ctypes.c_int, [_V, _MP, _V, _V, _OP, _V, _V]),
    ("dlm_dlmfsv_impute_batch", ctypes.c_int, [_V, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _V, _V, _V, _V, ctypes.c_uint64, _OP,
                                               _V, _V]),
    ("dlm_dlmfsv_variance_batch", ctypes.c_int, [_V, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _V, _V, _V, _OP, _V, _V]),
    ("dlm_dlmfsvsys_innovations_batch", ctypes.c_int, [_V, _MP, _V, _OP, _V, _V]),
    ("dlm_pf_batch", ctypes.c_int, [_V, _MP, _PP, ctypes.POINTER(PfDesc), _V, _V, ctypes.c_uint64, _OP, _V, _V, _V, _V, _V, _V]),
    ("dlm_pf_resampled", ctypes.c_int, [_V, _MP, _PP, ctypes.POINTER(PfDesc), ctypes.POINTER(ResampleDesc), _V, _V, ctypes.c_uint64, _OP,
                                        _V, _V, _V, _V, _V, _V]),
    # (ranks is a HOST array whatever opts->mem is: a typed pointer, not one of the data pointers Engine._call turns into addresses)
    ("dlm_pf_forecast_particles", ctypes.c_int, [_V, _MP, _PP, ctypes.POINTER(PfForecastDesc), _V, _ip, _V, _V, _V, ctypes.c_uint64, _OP,
                                             _V, _V, _V, _V, _V, _V, _V, _V]),
    ("dlm_storvik_batch", ctypes.c_int, [_V, _MP, _PP, ctypes.POINTER(StorvikDesc), _V, ctypes.c_int64, _V, ctypes.c_int64, _V, _V, ctypes.c_uint64,
                                         _OP, _V, _V, _V, _V, _V, _V, _V, _V]),
    ("dlm_lw_batch", ctypes.c_int, [_V, _MP, _PP, ctypes.POINTER(LwDesc), _V, ctypes.c_int64, _V, ctypes.c_int64, _V, _V, ctypes.c_uint64,
                                    _OP, _V, _V, _V, _V, _V, _V, _V, _V, _V]),
    ("dlm_rb_batch", ctypes.c_int, [_V, _MP, _PP, ctypes.POINTER(RbDesc), _V, ctypes.c_int64, _V, ctypes.c_int64, _V, ctypes.c_uint64,
                                    _OP, _V, _V, _V, _V, _V, _V, _V, _V, _V, _V, _V]),
    # (ranks: a host array, as above)
    ("dlm_pf_forecast_learned", ctypes.c_int, [_V, _MP, _PP, ctypes.POINTER(PfForecastLearnedDesc), _V, _ip, _V, _V, _V, _V, _V, ctypes.c_int64,
                                               ctypes.c_uint64, _OP, _V, _V, _V, _V, _V, _V, _V, _V]),
    ("dlm_rb_state_draw", ctypes.c_int, [_V, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _V, _V, ctypes.c_int64, ctypes.c_uint64, _OP, _V, _V]),
    ("dlm_sv_paths", ctypes.c_int, [_V, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, ctypes.c_int32, _V, _V, ctypes.c_uint64, _OP, _V, _V]),
    # (probs is a HOST array whatever opts->mem is: a typed pointer, as ranks above)
    ("dlm_gaussian_mixture_summary", ctypes.c_int, [_V, ctypes.POINTER(MixtureDesc), _V, _V, ctypes.POINTER(ctypes.c_double), _OP, _V, _V, _V, _V]),
    ("dlm_pg_batch", ctypes.c_int, [_V, _MP, _PP, ctypes.POINTER(PgDesc), _V, _V, _V, ctypes.c_uint64, _OP, _V, _V, _V, _V, _V, _V, _V, _V]),
    ("dlm_ou_ffbs_batch", ctypes.c_int, [_V, ctypes.c_int32, ctypes.c_int32, _V, _V, _V, ctypes.c_int64, _V, ctypes.c_int64,
                                         _V, _OP, _V, _V, _V]),
    ("dlm_ar1_ffbs_batch", ctypes.c_int, [_V, ctypes.c_int32, ctypes.c_int32, _V, _V, ctypes.c_int64, _V, ctypes.c_int64,
                                          _V, _OP, _V, _V, _V]),
    ("dlm_smooth_batch", ctypes.c_int, [_V, _MP, _PP, _V, _OP, _V, _V]),
    ("dlm_filter_smooth_batch", ctypes.c_int, [_V, _MP, _PP, _V, _OP, _V, _V, _V]),
    ("dlm_last_timing", ctypes.c_int, [_V, ctypes.POINTER(ctypes.c_double * 2)]),
    ("dlm_last_counters", ctypes.c_int, [_V, ctypes.POINTER(ctypes.c_uint64 * 4)]),
    ("dlm_last_table_reuse", ctypes.c_int, [_V, ctypes.POINTER(ctypes.c_int32)]),
    ("dlm_ffbs_batch", ctypes.c_int, [_V, _MP, _PP, _V, _V, _OP, _V, _V, _V, _V, _V]),
    ("dlm_stats_len", ctypes.c_int32, [ctypes.c_int32, ctypes.c_int32, ctypes.c_uint32]),
    ("dlm_backward_sample_batch", ctypes.c_int, [_V, _MP, _PP, _V, _V, _V, _OP, _V, _V, _V, _V]),
    ("dlm_svd_filter_batch", ctypes.c_int, [_V, _MP, _PP, _V, _OP, _V, _V]),
    ("dlm_svd_ffbs_batch", ctypes.c_int, [_V, _MP, _PP, _V, _V, _OP, _V, _V, _V, _V]),
    ("dlm_stats_pool", ctypes.c_int, [_V, _V, ctypes.c_int32, ctypes.c_int32, _V, _OP]),
    ("dlm_comm_unique_id", ctypes.c_int, [ctypes.c_char_p]),
    ("dlm_comm_init_rank", ctypes.c_int, [_V, ctypes.c_int32, ctypes.c_int32, ctypes.c_char_p]),
    ("dlm_gibbs_suffstats_allreduce", ctypes.c_int, [_V, _V, ctypes.c_int64]),
]

_lib = None


class EngineLibraryMissing(RuntimeError):
    pass


def load():
    """Load libdlm_engine.so; raise EngineLibraryMissing if it is absent (no CPU fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch wheels bundle their own libamdhip64.so.7 / librccl.so.1.  Two HIP runtimes in one
    # process cannot both own the GPU, so when torch is installed it is imported first and
    # the engine library binds to the runtime torch has already loaded.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    if not os.path.exists(LIB_PATH):
        raise EngineLibraryMissing(
            f"{LIB_PATH} not found: build it with `python -m bayesian_dlms_amd.build` "
            "(hipcc, gfx950).  The engine has no CPU fallback.")
    lib = ctypes.CDLL(LIB_PATH)
    for name, res, args in SYMBOLS:
        fn = getattr(lib, name)  # AttributeError if the library does not export it
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib
