/*
 * dlm_engine.h -- C ABI of the MI355X batched Kalman filter / smoother / FFBS engine.
 *
 * This is the drop-in boundary.  The reference (jonnylaw/bayesian_dlms, Scala) has no
 * FFI/plugin interface: its seams are per-timestep closures (KalmanFilter.scala:32,
 * SvdFilter.scala:22, Smoothing.scala:114-116), far too fine for a JNI crossing.  The
 * boundary therefore sits one level up, at the whole-series calls, widened to a batch of
 * N independent series that share one model (`Dlm`) and one time grid.  Each entry point
 * names the reference call it replaces; the JNI / Scala binding is in INTEGRATION.md.
 *
 * Conventions (all citations relative to /root/reference/core/src/main/scala/dlm/model/):
 *  - fp64 everywhere; matrices column-major (Breeze `DenseMatrix.data`).
 *  - F is d x p and is used as F^T (KalmanFilter.scala:317).
 *  - A missing observation component (`None`, Dlm.scala:94) is NaN in `y`.
 *  - Outputs carry T+1 records; record 0 is the initial state at t0-1 (`.filter` keeps it,
 *    Filter.scala:41-45; KalmanFilter.initialiseState, KalmanFilter.scala:112-118).
 *  - A "state record" is d + d*d doubles: mean (d) then covariance (d x d, column-major).
 *  - The caller owns every buffer.  `opts->mem` says whether ALL data pointers of the call
 *    (descriptors' arrays, y, outputs, status) are device (HIP) pointers or host pointers;
 *    in host mode the engine stages H2D/D2H through its own workspace.
 *  - Return value: 0 = OK, negative = error (message via dlm_last_error).  Numerical trouble
 *    is reported per series in `status[N]` bit flags; the batch still completes.
 *  - An engine handle is not thread-safe; use one handle per thread / per GPU.
 */
#ifndef DLM_ENGINE_H
#define DLM_ENGINE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dlm_engine dlm_engine;

enum {
  DLM_OK = 0,
  DLM_ERR_ARG = -1,         /* bad argument / shape                                   */
  DLM_ERR_HIP = -2,         /* HIP runtime error                                      */
  DLM_ERR_UNSUPPORTED = -3, /* shape outside what the kernels cover   */
  DLM_ERR_RCCL = -4         /* RCCL error                                             */
};

enum { DLM_MEM_DEVICE = 0, DLM_MEM_HOST = 1 };

/* dlm_options.flags */
enum {
  DLM_OPT_SMOOTHER_COMPAT_Q1 = 1u << 0, /* literal Smoothing.scala:44 (J X J, no transpose) */
  DLM_OPT_SVD_RAW_W_Q2 = 1u << 1,       /* literal SvdFilter.filterDlm: raw W as sqrt(W)    */
  DLM_OPT_SVD_SAMPLER_Q9 = 1u << 2,     /* literal SvdSampler.step: sqrt(W) for sqrt(W)^-1  */
  DLM_OPT_FORCE_GENERIC = 1u << 3,      /* disable the specialised (MFMA) kernels           */
  DLM_OPT_STATS_OUTER = 1u << 4,        /* Gibbs stats: full outer product (GibbsWishart)   */
  DLM_OPT_ASYNC = 1u << 5,              /* do not synchronise the stream before returning   */
  DLM_OPT_FFBS_SIMSMOOTH = 1u << 6,     /* draw with the Durbin-Koopman simulation smoother */
  DLM_OPT_PACKED_SYM = 1u << 7,         /* state records leave PACKED: [mean (d) | lower triangle of the covariance by rows],
                                           dlm_packed_record_doubles(d) doubles per record (see below)              */
  /* A PROMISE of the caller, not a tuning knob -- results are WRONG if it is broken.  Device-memory calls only: F, G and the
   * time grid are bit for bit those of this engine's previous model-taking call, so its analysis of their structure is reused
   * (two stream round trips per call less).  The engine checks what it can without reading device memory (d, p, n_g, f_stride
   * and the path taken must agree, else it analyses afresh) and, unless DLM_OPT_TRUST_MODEL_UNCHANGED is also set, verifies
   * the promise with a 64-bit checksum of F, G, g_index and dt computed on the device (one tiny kernel per call; a mismatch
   * returns DLM_ERR_ARG).  Host-memory calls never need it: the engine compares the tables itself. */
  DLM_OPT_MODEL_UNCHANGED = 1u << 8,
  DLM_OPT_COUNT_STEPS = 1u << 9,        /* count the steps that took a short path (dlm_last_counters); costs a 32-byte memset per call */
  DLM_OPT_TRUST_MODEL_UNCHANGED = 1u << 10, /* with DLM_OPT_MODEL_UNCHANGED: skip the device checksum (callers that stage the tables themselves
                                         * and compare them on the host, as bayesian_dlms_amd/engine.py does)                     */
  DLM_OPT_LOGLIK_LITERAL_Q7 = 1u << 11, /* dlm_loglik_batch: KalmanFilter.likelihood as written (KalmanFilter.scala:299-306, what
                                         * MetropolisHastings.dlm evaluates): the transition density of the filtered means        */
  DLM_OPT_STUDENTT_LITERAL = 1u << 12,  /* dlm_studentt_step_batch: StudentT.step's arithmetic as written: v_t drawn
                                         * with the previous nu and theta_{t-1}, nu moved last, the proposal density at `to`, a
                                         * missing y_t drawn with shape (nu + 1) / 2, 0.5 log(pi nu sqrt(s)) in the log-likelihood */
  /* Kernel-selection overrides: measurements and tests only, results do not depend on them.           */
  DLM_OPT_NO_LANE = 1u << 16,           /* no lane-per-series kernels (d <= 5, p = 1)                                  */
  DLM_OPT_NO_SAMPLER16 = 1u << 17,      /* no register-tile backward sampler: the generic kernel                       */
  DLM_OPT_NO_WAVE = 1u << 18,           /* 16 <= d <= 48: the workgroup-per-series kernels instead of wave-per-series  */
  DLM_OPT_FORCE_WAVE = 1u << 19,        /* 16 <= d <= 48: wave-per-series kernels also for batches of <= 256 series    */
  DLM_OPT_NO_SPARSE_F = 1u << 20,       /* treat F as dense                                                            */
  DLM_OPT_NO_SMALL_BATCH = 1u << 21,    /* d <= 15: the throughput kernels also for batches that leave SIMDs idle      */
  DLM_OPT_NO_STEADY = 1u << 22,         /* d <= 15: every step recomputes the covariance recursion, also once it has settled */
  DLM_OPT_NO_PIPE = 1u << 23,           /* d <= 15, small batches: the output product's MFMAs in one block (as at full occupancy) */
  DLM_OPT_SVD_PER_SERIES = 1u << 25,    /* SVD filter: every series runs its own decompositions, also when the batch shares V, W, C0 and has no missing
                                           observation (by default they are then done once per call and shared: the same bits) */
  DLM_OPT_SAMPLER_PER_SERIES = 1u << 26, /* dlm_ffbs_batch, reference-form sampler: every series computes its own J_t, H_t and factors, also when the batch
                                           shares V, W, C0 on a regular grid (by default one wave computes them once per call and the series draw against
                                           its table: the same draws, bit for bit) */
  DLM_OPT_DRAW_EIG = 1u << 27,          /* dlm_ffbs_batch / dlm_backward_sample_batch, reference-form sampler: draw with the REFERENCE's factor, theta = h + E sqrt(Lambda) z from
                                           the symmetric eigendecomposition of H (MultivariateGaussianSvd.scala:13-22; eigenvalues ascending, the largest-|.| entry of each
                                           eigenvector positive -- LAPACK leaves the sign open), instead of the engine's lower Cholesky factor.  The same distribution,
                                           other draws; served by the general LDS kernel (d <= 53): for parity with the literal operation sequence, not for speed */
  DLM_OPT_SMOOTHER_PER_SERIES = 1u << 28, /* dlm_filter_smooth_batch with DLM_OPT_SMOOTHER_COMPAT_Q1, structured d <= 15, p = 1: every series computes its own J_t and
                                           S_t, also when the batch shares V, W, C0 on a regular grid (by default they are computed once per call and every series
                                           without a missing observation runs only its mean recursion: the same records, bit for bit) */
  DLM_OPT_NO_TABLE_REUSE = 1u << 29,    /* dlm_filter_smooth_batch through the shared RTS tables: by default the engine keeps the tables of the last call that made
                                           them and a later call whose d, T, F, G, V, W, C0 and semantics are byte for byte the same (compared on the device) uses them instead of
                                           making them again: the same records, bit for bit.  With this flag a call makes its tables afresh and keeps none (dlm_last_table_reuse) */
  DLM_OPT_TEST_FAIL_AFTER_TABLES = 1u << 30, /* TEST HOOK (tests/test_shared_sampler_gpu.py, test_shared_rts_gpu.py): dlm_ffbs_batch / dlm_filter_smooth_batch return DLM_ERR_UNSUPPORTED right after they have started the
                                           shared-factor tables and normals on the engine's auxiliary streams -- the error path that must leave the engine usable */
  DLM_OPT_SHARED_COV = 1u << 24         /* d <= 15, p = 1, regular grid, V, W, C0 shared by the batch: ONE wave runs the covariance recursions, every series
                                           only its mean recursions against their tables; a series with a missing observation runs its own recursion
                                           as always.  Bit for bit the results of the default kernels (tests/test_shared_cov_gpu.py) -- and, measured,
                                           no faster than them: opt-in (profiles/r03_notes.md) */
};

/* per-series status bits */
enum {
  DLM_ST_NONFINITE = 1, /* a non-finite value appeared in the state                        */
  DLM_ST_NOT_PD = 2,    /* a matrix that must be positive definite was not (Q, R or H)     */
  DLM_ST_NOCONV = 4     /* Jacobi SVD did not converge                                     */
};

/* The model, materialised on the host from the reference's closures
 * (`Dlm(f, g)`, Dlm.scala:14-15): F_t = f(time_t), G_k = g(dt_k) per distinct dt. */
typedef struct {
  int32_t d, p, T, N;
  const double *F;        /* [nF][d*p]; nF = 1 if f_stride == 0 else T                     */
  int64_t f_stride;       /* 0: time-invariant F; else F_t = F + t * f_stride (doubles)    */
  const double *G;        /* [n_g][d*d]                                                   */
  int32_t n_g;
  const int32_t *g_index; /* [T] table index of step t; NULL: all 0                        */
  const double *dt;       /* [T] time increments; NULL: all 1.0.  dt == 0 means "no        */
                          /* advance" exactly as KalmanFilter.advState (:279-280)          */
} dlm_model_desc;

/* `DlmParameters(v, w, m0, c0)` (Dlm.scala:36-39); a stride of 0 shares the array between
 * all series, otherwise series n reads base + n * stride (doubles).
 * Time-varying variances (the per-step V_t / W_t streams of StudentT.filter, StudentTGibbs.scala:100-136,
 * and of DlmFsvSystem.ffbs, DlmFsvSystem.scala:137-208): with v_tstride / w_tstride != 0 observation t (0-based) uses
 * V + n * v_stride + t * v_tstride and the transition INTO observation t uses W + n * w_stride + t * w_tstride
 * (T matrices each).  0 = time-invariant.  The SVD entry points take them too: step t then runs with the square roots
 * of V_t / W_t (DlmFsv.ffbsSvd, DlmFsv.scala:208-228; DlmFsvSystem.ffbsSvd, DlmFsvSystem.scala:176-208). */
typedef struct {
  const double *V;  int64_t v_stride;   /* p x p */
  const double *W;  int64_t w_stride;   /* d x d */
  const double *m0; int64_t m0_stride;  /* d     */
  const double *C0; int64_t c0_stride;  /* d x d */
  int64_t v_tstride;                    /* 0 or p * p */
  int64_t w_tstride;                    /* 0 or d * d */
} dlm_params_desc;

typedef struct {
  uint32_t flags;     /* DLM_OPT_*                                                        */
  int32_t mem;        /* DLM_MEM_DEVICE or DLM_MEM_HOST                                   */
  uint64_t seed;      /* Philox key for FFBS draws                                        */
  uint64_t series_offset; /* global index of series 0 of this call (multi-GPU shards       */
                          /* draw the same normals as a single-GPU run)                   */
} dlm_options;

/* ---- lifecycle ------------------------------------------------------------------- */
int dlm_engine_create(int device, dlm_engine **out);
void dlm_engine_destroy(dlm_engine *e);
const char *dlm_last_error(const dlm_engine *e);
const char *dlm_version(void);
/* Launch on a caller-owned hipStream_t (NULL = the engine's own stream).  The engine's workspaces are shared by its calls: a
 * change of stream first drains the work still in flight on the old one (DLM_OPT_ASYNC calls). */
int dlm_engine_set_stream(dlm_engine *e, void *hip_stream);
int dlm_engine_sync(dlm_engine *e);
/* Name of the kernel variant the last call dispatched to ("generic", "mfma16", ...). */
const char *dlm_last_variant(const dlm_engine *e);

/* ---- ordering against the caller's streams ------------------------------------------
 * The engine launches on its own stream.  A caller that produces inputs (or frees / reuses buffers) on another
 * HIP stream orders the two with events, without a host synchronisation:
 *   dlm_engine_wait_stream   work submitted to `hip_stream` so far completes before any later engine work starts;
 *   dlm_stream_wait_engine   engine work submitted so far completes before later work on `hip_stream` starts
 *                            (needed only after DLM_OPT_ASYNC calls: synchronous calls have drained the engine stream).
 * hip_stream == NULL means the legacy default stream (what `torch.cuda.current_stream()` is unless changed). */
int dlm_engine_wait_stream(dlm_engine *e, void *hip_stream);
int dlm_stream_wait_engine(dlm_engine *e, void *hip_stream);

/* ---- engine-owned device buffers ------------------------------------------------------
 * For callers without a device allocator of their own (the JVM through JNI, plain C / C++): allocate once, keep
 * inputs and results in HBM across calls (opts->mem = DLM_MEM_DEVICE, the measured path) and move only what is
 * needed.  A buffer is an ordinary HIP device pointer (arithmetic on it is allowed: base + offset is what the
 * descriptors take).  Upload / download are synchronous on return and ordered after all engine work submitted
 * before them; offsets and sizes in bytes.  Buffers still allocated are released by dlm_engine_destroy. */
int dlm_buffer_alloc(dlm_engine *e, uint64_t bytes, void **dev_ptr);
int dlm_buffer_free(dlm_engine *e, void *dev_ptr);
int dlm_buffer_upload(dlm_engine *e, void *dst_dev, uint64_t dst_offset, const void *src_host, uint64_t bytes);
int dlm_buffer_download(dlm_engine *e, const void *src_dev, uint64_t src_offset, void *dst_host, uint64_t bytes);
int dlm_buffer_fill(dlm_engine *e, void *dst_dev, uint64_t dst_offset, int byte_value, uint64_t bytes);
int dlm_device_mem_info(dlm_engine *e, uint64_t *free_bytes, uint64_t *total_bytes);

/* ---- packed symmetric records (DLM_OPT_PACKED_SYM) --------------------------------------
 * A packed state record is [mean (d) | C(0,0) | C(1,0) C(1,1) | C(2,0) ... C(d-1,d-1)] -- the lower triangle by
 * rows -- in a slot of dlm_packed_record_doubles(d) = d + d (d + 1) / 2 rounded up to even doubles (104 at d = 13
 * against 182 dense; the padding double, when there is one, is never written).  With the flag dlm_filter_batch writes `filt` and
 * dlm_filter_smooth_batch writes `filt` and `smooth` packed; algorithmic traffic of the fused pass drops from
 * 8p + 24 (d + d^2) to 8p + 24 (d + d (d + 1) / 2) bytes per series-step (2504 instead of 4376 at d = 13).  Served by the
 * structured d <= 15, p = 1 kernels (every model the reference can build at those sizes); other shapes, the Q1 literal
 * mode, prior records and dlm_smooth_batch return DLM_ERR_UNSUPPORTED -- use dense records there.
 * dlm_unpack_records expands [count] packed records into dense ones (host or device memory according to opts->mem). */
int32_t dlm_packed_record_doubles(int32_t d);
int dlm_unpack_records(dlm_engine *e, int32_t d, int64_t count, const double *packed, const dlm_options *opts,
                       double *dense);

/* ---- Kalman filter ----------------------------------------------------------------
 * Replaces KalmanFilter(KalmanFilter.advanceState(p, mod.g)).filter(mod, ys, p)
 * (KalmanFilter.scala:262-294, Filter.scala:41-45) for N series.
 *   y      [N][T][p]
 *   filt   [N][T+1][d+d*d]   (m_t, C_t)
 *   prior  [N][T+1][d+d*d]   (a_t, R_t)            optional (NULL)
 *   fq     [N][T+1][p+p*p]   (f_t, Q_t; record 0 NaN) optional (NULL)
 *   status [N]                                      optional (NULL) */
int dlm_filter_batch(dlm_engine *e, const dlm_model_desc *model, const dlm_params_desc *params,
                     const double *y, const dlm_options *opts, double *filt, double *prior,
                     double *fq, int32_t *status);

/* ---- RTS smoother -----------------------------------------------------------------
 * Replaces Smoothing.backwardsSmoother(mod)(kfStates) (Smoothing.scala:31-64).
 * Takes the filter records and recomputes a_{t+1}, R_{t+1} from (m_t, C_t) instead of
 * reading them back.  smooth [N][T+1][d+d*d] = (s_t, S_t). */
int dlm_smooth_batch(dlm_engine *e, const dlm_model_desc *model, const dlm_params_desc *params,
                     const double *filt, const dlm_options *opts, double *smooth, int32_t *status);

/* Simulation from the model on the device: Dlm.simulateRegular / simStep (Dlm.scala:245-292) over the model's time grid,
 *   x_0 ~ N(m0, C0);  x_t = G_t x_{t-1} + w_t, w_t ~ N(0, W dt_t);  y_t = F_t^T x_t + v_t, v_t ~ N(0, V).
 * Lower-Cholesky factors of C0, W, V (the reference draws through an eigen-factor: same distribution) on the Philox
 * stream (opts->seed, opts->series_offset + n, record t, i), i < d state noise, d <= i < d + p observation noise.
 * x [N][T+1][d] (record 0 = x_0) nullable; y [N][T][p]; status [N] nullable. */
int dlm_simulate_batch(dlm_engine* e, const dlm_model_desc* model, const dlm_params_desc* params,
                       const dlm_options* opts, double* x, double* y, int32_t* status);

/* GibbsSampling.dinvGammaStep on the device (Gibbs.scala:23-78, :134-151) for per-series parameters: from the
 * statistics [N][2p + d + 1] = [ssy | n | ss | T] of an FFBS call (without DLM_OPT_STATS_OUTER) draw
 *   V_jj ~ InverseGamma(alpha_v + n_j / 2, beta_v + ssy_j / 2),   W_ii ~ InverseGamma(alpha_w + T / 2, beta_w + ss_i / 2)
 * and write the dense diagonal matrices V_out [N][p*p], W_out [N][d*d] -- directly usable as the next call's
 * per-series parameters (v_stride = p*p, w_stride = d*d), so that a Gibbs iteration never leaves the GPU.
 * Marsaglia-Tsang Gamma draws on the Philox stream (opts->seed, opts->series_offset + n, iteration, component):
 * reproducible and shard-invariant; the reference's generator cannot be seeded, only the distribution compares. */
int dlm_dinvgamma_step_batch(dlm_engine* e, int32_t d, int32_t p, int32_t N, const double* stats, double alpha_v,
                             double beta_v, double alpha_w, double beta_w, uint64_t iteration, const dlm_options* opts,
                             double* V_out, double* W_out);

/* One step of the Student-t observation DLM's Gibbs sampler (StudentT.step, StudentTGibbs.scala:182-212) for N independent
 * chains, after the FFBS call of its state draw (dlm_ffbs_batch with the V_t stream v_t of the previous step and per-series W).
 * p = 1 (the reference's model is univariate; DLM_ERR_UNSUPPORTED otherwise).  model: F (time-varying allowed in the default
 * mode), d, T, N; G and the time grid are not read.  Inputs:
 *   y [N][T] (NaN = missing), theta [N][T+1][d] as dlm_ffbs_batch writes it, stats [N][dlm_stats_len(d, 1, 0)] of that call,
 *   scale_in [N] (s, the square of the Student-t scale), nu_in [N] (degrees of freedom, int32).
 * Default (corrected) order: W | theta, then nu | (theta, s) by Metropolis-Hastings with v_t marginalised, then v_t | (theta, nu, s),
 * then s | (v, nu):
 *   W_ii ~ InverseGamma(prior_w_shape + T / 2, prior_w_scale + ss_i / 2)       (dlm_dinvgamma_step_batch's stream: W_out is that call's)
 *   nu'  = Poisson(Gamma(r, nu / r)) + 1 (r = prop_nu_size), accepted against Poisson(prior_nu_rate) and the Student-t likelihood
 *   v_t  ~ InverseGamma((nu + 1) / 2, nu s / 2 + e_t^2 / 2),  e_t = y_t - F_t^T theta_t;  missing y_t: InverseGamma(nu / 2, nu s / 2)
 *   s    ~ Gamma(T nu / 2 + 1, 1 / (nu / 2 sum_t 1 / v_t))
 * DLM_OPT_STUDENTT_LITERAL: the reference's arithmetic; the caller passes the INITIAL (s, W) every step (Q10).
 * A literal call with a time-varying F is DLM_ERR_UNSUPPORTED (Q11 needs F at t0 - 1).
 * Outputs: v_out [N][T] (the next FFBS call's V stream: v_stride = T, v_tstride = 1), scale_out [N], nu_out [N], W_out [N][d*d]
 * (dense diagonal), accepted [N] (in / out: incremented on acceptance), loglik [N] (nullable: the Student-t log-likelihood at
 * nu_out and scale_in), status [N] (nullable).  scale_out may be scale_in and nu_out may be nu_in.  A series with nu_in < 1, s not
 * finite and positive, or a non-finite F^T theta_t gets DLM_ST_NONFINITE, NaN in its double outputs and nu_out = nu_in.
 * Draws: W on the dlm_dinvgamma_step_batch stream (components 1 + i), everything else on a Philox stream of its own keyed by
 * (opts->seed, opts->series_offset + n, iteration, slot): reproducible and independent of the sharding.  T < 2^21 - 4.
 * The call reads F only: it does not count as the "previous model-taking call" of DLM_OPT_MODEL_UNCHANGED. */
typedef struct { double prior_nu_rate, prop_nu_size, prior_w_shape, prior_w_scale; } dlm_studentt_prior;
int dlm_studentt_step_batch(dlm_engine* e, const dlm_model_desc* model, const double* y, const double* theta,
                            const double* stats, const dlm_studentt_prior* prior, const double* scale_in,
                            const int32_t* nu_in, uint64_t iteration, const dlm_options* opts, double* v_out,
                            double* scale_out, int32_t* nu_out, double* W_out, int32_t* accepted,
                            double* loglik, int32_t* status);

/* Scalar AR(1) state-space FFBS, one GPU lane per series: FilterAr.filterUnivariate / univariateSample / ffbs
 * (FilterAr.scala:15-82), the filter of the stochastic-volatility samplers (StochasticVolatility.scala:142-162,
 * FactorSv.scala:415-512):
 *   alpha_t = mu + phi (alpha_{t-1} - mu) + eta_t, eta_t ~ N(0, sigma_eta^2);   y_t = alpha_t + eps_t, eps_t ~ N(0, v_t)
 * y [N][T] (NaN = None); v: per-step observation variances, [N][T] with v_stride = T or one shared stream [T] with
 * v_stride = 0; sv: (phi, mu, sigma_eta) in SvParameters order, [N][3] with sv_stride = 3 or one shared triple with
 * sv_stride = 0; z [N][T+1] injected normals or NULL (Philox stream (seed, series_offset + n, t, 0));
 * filt [N][T+1][2] = (m_t, c_t) with record 0 = (mu, sigma_eta^2 / (1 - phi^2)), nullable;
 * theta [N][T+1] one draw per state, NULL = filter only; status [N] nullable.  opts->flags: DLM_OPT_ASYNC only. */
int dlm_ar1_ffbs_batch(dlm_engine* e, int32_t N, int32_t T, const double* y, const double* v, int64_t v_stride,
                       const double* sv, int64_t sv_stride, const double* z, const dlm_options* opts,
                       double* filt, double* theta, int32_t* status);

/* The Ornstein-Uhlenbeck variant of the above on an irregular time grid: FilterOu.filterUnivariate / univariateSample /
 * ffbs (FilterOu.scala:7-79).  times [T] observation times shared by the batch; sv = (phi, mu, sigma_eta) with phi > 0
 * the mean-reversion rate.  Literal reference behaviour: c0 = sigma * sigma / phi * phi (= sigma^2) and the initial
 * state sits at the first observation time (first dt = 0).  Everything else as dlm_ar1_ffbs_batch. */
int dlm_ou_ffbs_batch(dlm_engine* e, int32_t N, int32_t T, const double* times, const double* y, const double* v,
                      int64_t v_stride, const double* sv, int64_t sv_stride, const double* z, const dlm_options* opts,
                      double* filt, double* theta, int32_t* status);

/* Gibbs sampler of the stochastic-volatility model with AR(1) latent log-volatility (StochasticVolatility.sampleUni / sampleBeta,
 * StochasticVolatility.scala:269-341) for N independent chains: the two calls around dlm_ar1_ffbs_batch.
 *   y_t = eps_t exp(alpha_t / 2),  alpha_t = mu + phi (alpha_{t-1} - mu) + eta_t,  eta_t ~ N(0, sigma^2);
 *   log y_t^2 = alpha_t + log eps_t^2, log eps^2 approximated by the seven-component normal mixture (pi_j, m_j, v_j) of
 *   Kim, Shephard & Chib (StochasticVolatility.scala:42-44).
 * Chain state per series: alpha [T+1] (alpha[0] the state before the first observation, alpha[t+1] the state of y[t]: the theta of
 * dlm_ar1_ffbs_batch) and sv = (phi, mu, sigma) in SvParameters order.  One iteration:
 *   dlm_sv_mixture_batch   k_t | (y_t, alpha_t), ystar_t = log y_t^2 - m_{k_t}, v_t = v_{k_t}        (sampleKt, :112-140; :151-157)
 *   dlm_ar1_ffbs_batch     alpha | (ystar, v, sv)   with v_stride = T, sv_stride = 3                  (FilterAr, :160-161)
 *   dlm_sv_params_batch    phi, then mu given the new phi, then sigma given both                      (:276-283 / :294-299)
 *
 * dlm_sv_mixture_batch.  y [N][T] (NaN = missing), alpha [N][T+1] or NULL, ystar [N][T], v [N][T], k [N][T] int8 (nullable: the
 * indicators 0..6), status [N] (nullable).  Per element, with x = alpha[n][t+1]:
 *   lw_j = log pi_j + log N(log y_t^2 - m_j; x, v_j)  (a missing y_t: lw_j = log pi_j),  w_j = exp(lw_j - max lw),
 *   p_j = w_0 + ... + w_j in index order,  k = #{ j in 0..5 : u p_6 >= p_j },  u the [0, 1) uniform of the element.
 * A missing y_t keeps ystar_t = NaN and takes v_t = v_k of its prior draw.  alpha == NULL is the initial transform of
 * initialStateAr (StochVolKnots.scala:345-352): ystar = log y^2 + 1.27, v = pi^2 / 2, no draw, k not written.
 * Q20: an observed y_t whose log y_t^2 is not finite (y_t = 0, y_t^2 underflowing) would make every weight -inf and the draw NaN in the
 * reference; it is treated as missing and the series gets DLM_ST_NONFINITE (so does a series with a non-finite alpha).
 *
 * dlm_sv_params_batch.  alpha [N][T+1], sv_in [N][3], sv_out [N][3] (may be sv_in), accepted [N] (in / out: incremented when the
 * Beta proposal is accepted; nullable with phi_update = 0), status [N] (nullable).  prior->phi_update selects samplePhiConjugate
 * (StochVolKnots.scala:25-43; phi_a, phi_b = mean and STANDARD DEVIATION of the Gaussian prior, as Breeze takes them) or the
 * Beta-proposal Metropolis-Hastings samplePhi (:189-202; phi_a, phi_b = the Beta prior's a, b; prop_lambda, prop_tau: the reference
 * passes 100, 0.05).  Default arithmetic, over all T pairs (alpha_{t-1}, alpha_t), psi the prior's standard deviation:
 *   phi ~ N(mean, 1 / prec) restricted to (-1, 1),  prec = 1 / psi^2 + sum (alpha_{t-1} - mu)^2 / sigma^2,
 *         mean = (m / psi^2 + sum (alpha_{t-1} - mu)(alpha_t - mu) / sigma^2) / prec; by rejection, at most 1023 attempts -- after
 *         that phi stays and the series gets DLM_ST_NOT_PD;
 *   or  phi' ~ Beta(lambda phi + tau, lambda (1 - phi) + tau), accepted with the full Hastings ratio against
 *         Beta(a, b)(phi) N(alpha_0; mu, sigma^2 / (1 - phi^2)) prod_t N(alpha_t; mu + phi (alpha_{t-1} - mu), sigma^2);
 *   mu ~ N(mean, 1 / prec),  prec = 1 / psi^2 + T (1 - phi)^2 / sigma^2,  mean = (m / psi^2 + (1 - phi) / sigma^2 sum (alpha_t - phi alpha_{t-1})) / prec;
 *   sigma^2 ~ InverseGamma(shape + T / 2, scale + 1/2 sum (alpha_t - mu - phi (alpha_{t-1} - mu))^2),  sigma = sqrt.
 * The conjugate mode leaves the stationary density of alpha_0 out of its three conditionals (it is not conjugate); the Beta mode's
 * target has it.  prior->literal = 1 is the reference's arithmetic: `1 / sigma * sigma` (= 1) where 1 / sigma^2
 * belongs; the T - 1 pairs t = 2..T in every transition sum, but sum_{t=1..T} (alpha_t - mu)^2 in phi's precision; shape + (T + 1) / 2;
 * an unrestricted Gaussian phi (|phi| >= 1 makes the next dlm_ar1_ffbs_batch report DLM_ST_NOT_PD).
 * A series whose sv_in is not finite, whose sigma <= 0, whose phi lies outside (0, 1) in the Beta mode, or whose sums are not finite
 * gets DLM_ST_NONFINITE and NaN in sv_out.
 *
 * Draws: a Philox stream of their own keyed by (opts->seed, opts->series_offset + n, iteration, slot): slot t for k_t, six slots
 * at the top of the field for the scalar draws (Marsaglia-Tsang Gammas, Box-Muller normals): reproducible and independent of
 * the sharding.  Limits: N >= 1, 2 <= T < 2^21 - 8 (the reference throws on T = 1; the slot field), N T < 2^39; non-positive
 * standard deviations, shape, scale, Beta or proposal parameters and unknown modes are DLM_ERR_ARG.  opts: mem, seed,
 * series_offset, DLM_OPT_ASYNC. */
typedef struct {
  int32_t phi_update;            /* 0: Gaussian conjugate (sampleUni), 1: Beta-proposal MH (sampleBeta) */
  int32_t literal;               /* 1: the reference's arithmetic, Q16-Q19 */
  double phi_a, phi_b;           /* Gaussian(mean, sd) as Breeze takes it, or Beta(a, b) */
  double mu_mean, mu_sd;
  double sigma_shape, sigma_scale;
  double prop_lambda, prop_tau;  /* the reference passes 100, 0.05 */
} dlm_sv_prior;
int dlm_sv_mixture_batch(dlm_engine* e, int32_t N, int32_t T, const double* y, const double* alpha, uint64_t iteration,
                         const dlm_options* opts, double* ystar, double* v, int8_t* k, int32_t* status);
int dlm_sv_params_batch(dlm_engine* e, int32_t N, int32_t T, const double* alpha, const double* sv_in, const dlm_sv_prior* prior,
                        uint64_t iteration, const dlm_options* opts, double* sv_out, int32_t* accepted, int32_t* status);

/* The parameter step of the stochastic-volatility sampler whose log-volatility is an Ornstein-Uhlenbeck process observed at
 * arbitrary times (StochasticVolatility.sampleOu / stepOu, StochasticVolatility.scala:343-500) for N independent chains:
 *   y_i = eps_i exp(alpha_i / 2),  alpha(t + dt) | alpha(t) ~ N(mu + e^(-phi dt) (alpha(t) - mu), sigma^2 (1 - e^(-2 phi dt)) / (2 phi)),
 * phi > 0 the mean-reversion rate.  One iteration:
 *   dlm_sv_mixture_batch     as for the AR(1) sampler (it works per element and never sees the time grid)
 *   dlm_ou_ffbs_batch        alpha | (ystar, v, sv) on the grid `times`, v_stride = T, sv_stride = 3             (sampleStateOu, :433-452)
 *   dlm_sv_ou_params_batch   three Metropolis moves: phi, then sigma at the new phi, then mu at the new phi and sigma  (:459-478)
 *
 * times [T] shared by the batch; alpha [N][T+1] as dlm_ou_ffbs_batch writes its theta: alpha[0] and alpha[1] both sit at times[0]
 * (the reference's first dt is 0) and alpha[t] belongs to times[t-1], so the informative pairs are (alpha[t-1], alpha[t]), t = 2..T,
 * with dt_t = times[t-1] - times[t-2].  A pair with dt = 0 contributes nothing (ouLikelihood, :360-361); n counts the pairs with
 * dt > 0.  sv_in [N][3], sv_out [N][3] (may be sv_in), accepted [N][3] (in / out, REQUIRED: the acceptances of phi, sigma, mu are
 * added), status [N] (nullable).  With e_t = exp(-phi dt_t), g_t = -expm1(-2 phi dt_t), d_t = alpha[t] - mu0 (mu0 the incoming mu):
 *   log p(alpha | phi, mu, sigma) = -n/2 log 2 pi - n log sigma + n/2 log(2 phi) - L(phi) / 2 - phi Q(phi, mu) / sigma^2,
 *   L = sum log g_t,  A = sum (d_t - e_t d_{t-1})^2 / g_t,  B = sum (d_t - e_t d_{t-1})(1 - e_t) / g_t,  C = sum (1 - e_t)^2 / g_t,
 *   Q(phi, mu0 + delta) = A - 2 delta B + delta^2 C.
 * The row is read once: (L, A, B, C) at phi and at the proposed phi' are all the three moves need.  Each move accepts when
 * log u < Delta.  Default arithmetic:
 *   phi'   ~ Beta(lambda phi + tau, lambda (1 - phi) + tau) (rejected when it rounds to 0 or 1), prior Beta(phi_a, phi_b), target
 *            (a - 1) log phi + (b - 1) log(1 - phi) + n/2 log(2 phi) - L(phi) / 2 - phi A(phi) / sigma^2, with the full Hastings ratio;
 *   sigma' = sigma exp(delta_sigma z), prior InverseGamma(sigma_shape, sigma_scale) ON SIGMA ITSELF (priorSigma.logPdf(newSigma), :407;
 *            dlm_sv_params_batch's prior is on sigma^2), target -(shape + 1) log sigma - scale / sigma - n log sigma - phi A / sigma^2
 *            - log sigma - (alpha_0 - mu)^2 / (2 sigma^2), plus log(sigma' / sigma) for the log-normal walk;
 *   mu'    = mu + delta_mu z, prior Gaussian(mu_mean, mu_sd) (the STANDARD DEVIATION, as Breeze takes it), target
 *            -(mu - m)^2 / (2 s^2) - phi Q(phi, mu) / sigma^2 - (alpha_0 - mu)^2 / (2 sigma^2).
 * The terms in alpha_0 are log N(alpha_0; mu, sigma^2), the initial state as dlm_ou_ffbs_batch draws it (c0 = sigma^2).
 * prior->literal = 1 is the reference's arithmetic: plain Metropolis ratios for the two asymmetric proposals
 * and no term for the initial state.  Q22: the reference's stepOu passes lambda = 0.05 (it meant tau); lambda, tau, delta_sigma and
 * delta_mu are fields here, the signatures' defaults being 10, 0.05, 0.05, 0.05.  Q25: sigma and mu start from the incoming values
 * and see the new phi (and sigma), as stepOu has it.
 * A negative or non-finite step of `times` gives EVERY series DLM_ST_NONFINITE and NaN in sv_out.  A series whose sv_in is not
 * finite, whose phi lies outside (0, 1), whose sigma <= 0 or whose sums at its phi are not finite gets DLM_ST_NONFINITE and NaN in
 * sv_out; its counters stay.
 *
 * Draws: a Philox stream of its own (another key than dlm_sv_mixture_batch's), counter (opts->seed, opts->series_offset + n,
 * iteration, slot), seven slots at the top of the field (two Marsaglia-Tsang Gammas, two Box-Muller normals, three uniforms):
 * reproducible and independent of the sharding.  Limits: N >= 1, 2 <= T < 2^21 - 8; non-positive standard deviation, shape, scale,
 * Beta or proposal parameters and literal outside {0, 1} are DLM_ERR_ARG.  opts: mem, seed, series_offset, DLM_OPT_ASYNC. */
typedef struct {
  int32_t literal;                 /* 1: the reference's arithmetic, Q23-Q24 */
  double phi_a, phi_b;             /* Beta(a, b) prior of phi */
  double mu_mean, mu_sd;           /* Gaussian(mean, sd) as Breeze takes it */
  double sigma_shape, sigma_scale; /* InverseGamma prior of sigma (not sigma^2) */
  double prop_lambda, prop_tau;    /* the Beta proposal; the signature's defaults are 10, 0.05, stepOu passes 0.05, 0.05 (Q22) */
  double delta_sigma, delta_mu;    /* the random walks' standard deviations; the reference passes 0.05, 0.05 */
} dlm_sv_ou_prior;
int dlm_sv_ou_params_batch(dlm_engine* e, int32_t N, int32_t T, const double* times, const double* alpha, const double* sv_in,
                           const dlm_sv_ou_prior* prior, uint64_t iteration, const dlm_options* opts, double* sv_out,
                           int32_t* accepted, int32_t* status);

/* The knot block sampler of the AR(1) stochastic-volatility state (StochasticVolatilityKnots.sampleBlock / sampleState,
 * StochVolKnots.scala:74-176): one sweep over N independent chains, in place.  Where dlm_sv_mixture_batch + dlm_ar1_ffbs_batch leave the
 * posterior under the seven-component approximation of log eps^2 invariant, this sweep leaves the posterior of the model
 *   y_t = eps_t exp(alpha_t / 2),  alpha_t = mu + phi (alpha_{t-1} - mu) + eta_t,  eta_t ~ N(0, sigma^2)
 * itself invariant.  y [N][T] (NaN = missing); alpha [N][T+1], in and out, in the layout of dlm_ar1_ffbs_batch's theta (alpha[0] the
 * state before the first observation, state s >= 1 observes y[s-1]); sv = (phi, mu, sigma) [N][3] with sv_stride = 3 or one shared
 * triple with sv_stride = 0; knots [B+1] shared by the batch (as `times` is for the OU calls; they follow opts->mem and are read and
 * checked on the host before anything runs): knots[0] = 0, knots[B] = T + 1, strictly increasing, block i the states
 * alpha[knots[i] .. knots[i+1] - 1]; accepted [N] (in / out, nullable): incremented by the number of this call's accepted blocks;
 * status [N] (nullable).
 * One block, states lo..hi:
 *   forward   stepUni on ystar_s = log y_{s-1}^2 + 1.27 with v = pi^2 / 2, from the point mass (alpha[lo-1], 0); lo = 0: from the
 *             stationary record (mu, sigma^2 / (1 - phi^2)), alpha[0]'s own prior;
 *   backward  backStepUni from the fixed alpha[hi+1]; hi = T: from a draw of the last filtering distribution;
 *   accept    Metropolis.mAccept: Delta = sum_{s in block, s >= 1, y_{s-1} observed} [g(alpha'_s) - g(alpha_s)],
 *             g(a) = -1/2 (a + y^2 e^{-a}) + (ystar - a)^2 / pi^2; accepted when log u < Delta; a block that observes nothing always.
 * Sweep order: red-black -- the even blocks, then the odd blocks, each a launch with one GPU lane per (series, block); given the odd
 * blocks the even ones are conditionally independent (each reads alpha[lo-1] and alpha[hi+1] only), so this is a valid Gibbs scan.
 * An observed y whose log y^2 is not finite is treated as missing in the proposal and in Delta and the series gets DLM_ST_NONFINITE
 * (Q20).  A series with |phi| >= 1 or sigma <= 0 gets DLM_ST_NOT_PD, one with a non-finite alpha or mu DLM_ST_NONFINITE: its row of
 * alpha and its counter come back untouched.  There is no literal mode.
 * Draws: a Philox stream of its own, counter (opts->seed, opts->series_offset + n, iteration, slot): slot s holds the normal of state
 * s; the acceptance uniform of a block sits at the slot of its first state under which = 1.  Reproducible, independent of the sharding
 * and of how blocks map to wavefronts.  Limits (DLM_ERR_ARG): N >= 1, T >= 2, T + 1 < 2^21 - 8, 1 <= B <= T + 1, knots as above,
 * sv_stride 0 or 3, y / knots / sv / alpha required.  opts: mem, seed, series_offset, DLM_OPT_ASYNC. */
int dlm_sv_knots_batch(dlm_engine* e, int32_t N, int32_t T, const double* y, const int32_t* knots, int32_t B,
                       const double* sv, int64_t sv_stride, uint64_t iteration, const dlm_options* opts,
                       double* alpha, int32_t* accepted, int32_t* status);

/* The factor half of the factor stochastic-volatility Gibbs sampler (FactorSv.sampleAr, FactorSv.scala:546-562) for N independent
 * panels of p series, T times and k latent factors, 1 <= k <= 8, k <= p <= 64:
 *   y_t = beta f_t + eps_t,  eps_t ~ N(0, diag(v)),  f_{j,t} ~ N(0, exp(alpha_{j,t})),  alpha_j AR(1) with (phi, mu, sigma_eta)_j;
 *   beta p x k with beta_ii = 1, beta_ij = 0 for j > i, beta_ij ~ N(beta_mean, beta_sd^2) elsewhere;
 *   v = sigma^2 1_p,  sigma^2 ~ InverseGamma(sigma_shape, sigma_scale).
 * Layouts: y [N][T][p] (NaN = missing), f [N][k][T] (factor-major: viewed as [N k][T] it is the y of dlm_sv_mixture_batch; NaN where
 * the time is missing), alpha [N][k][T+1] (alpha[..][t+1] belongs to y[t]), sv [N][k][3], beta [N][p][k] row-major, v [N][p].
 * One iteration, in sampleStep's order:
 *   dlm_sv_mixture_batch, dlm_ar1_ffbs_batch, dlm_sv_params_batch on the N k factor series f (a missing factor is a missing
 *       observation); chain (n, j) is the series (series_offset + n) k + j of those calls.  Q31: the reference's sampleStep draws the
 *       state with the knot block sampler, which is not offered; this is its own alternative sampleVolatilityAr (:415-435);
 *   dlm_fsv_factors_batch    f_t | (y_t, beta, v, alpha_{t+1}) for every (n, t)                      (sampleFactors, :168-186)
 *   dlm_fsv_loadings_batch   sigma^2 | (y, f, beta_old), then beta | (y, f, sigma^2) row by row      (sampleSigmaUni, :516-541;
 *                                                                                                     sampleBeta / sampleBetaRow, :253-333)
 * A time t is OBSERVED when all p components of y_t are finite (encodePartiallyMissing, :150-157, treats a partially missing y_t as
 * wholly missing; both modes).  An unobserved time gets f_t = NaN and contributes to no sum.
 *
 * dlm_fsv_factors_batch.  For an observed time, with the Cholesky factor P_t = L L^T and z ~ N(0, I_k):
 *   P_t = beta^T diag(1 / v) beta + diag(exp(-alpha_{.,t+1})),   m_t = P_t^-1 beta^T diag(1 / v) y_t,
 *   f_t = m_t + L^-T z ~ N(m_t, P_t^-1);   literal = 1:  f_t = m_t + P_t^-1 z, of covariance P_t^-2 (Q27: rnorm, :222-232).
 * alpha == NULL is initialiseFactors (:571-590): the second term of P_t is the identity.  z_j is the Box-Muller normal of slot t,
 * attempt j of the stream below.  status [N] (nullable): DLM_ST_NOT_PD when a Cholesky pivot is not positive (that time is NaN);
 * DLM_ST_NONFINITE for a non-finite beta or a v that is not positive and finite -- the whole panel's f is NaN -- and for a non-finite
 * alpha_{j,t+1} or an exp(-alpha) that overflows -- that time is NaN.  Other panels are untouched.
 *
 * dlm_fsv_loadings_batch.  A time counts when y_t is observed and f_t is finite; over those times of a panel, n of them,
 *   S = sum f_t f_t^T,   c_i = sum f_t y_ti,   ssy = sum |y_t - beta_in f_t|^2,
 *   sigma^2 ~ InverseGamma(shape + n p / 2, scale + ssy / 2);  then for the rows i = 1 .. p - 1, q = min(i, k), S_q the leading block:
 *   beta_{i,0:q} ~ N(P^-1 r, P^-1),  P = S_q / sigma^2 + I / beta_sd^2,  r = (c_i - [i < k] S_{0:q,i}) / sigma^2 + beta_mean / beta_sd^2
 * (a row i < k regresses y_i - f_i on the earlier factors: its own loading is the fixed 1).  prior->literal = 1 is the reference's
 * arithmetic: InverseGamma(shape + n / 2, scale + ssy / (2 p)); P = S_q / sigma^2 + I beta_sd^2 and
 * r = c_i / sigma^2 (the prior variance where the precision belongs, no prior mean, f_i not removed); the draw P^-1 r + P^-1 z.
 * beta_out [N][p][k] gets its fixed ones and zeros too and may be beta_in; v_out [N][p] holds sigma^2 in every entry and may be v_in.
 * v_in is nullable.  status [N] (nullable): a panel without a counted time gets DLM_ST_NONFINITE and beta_out = beta_in, v_out = v_in
 * (NaN without v_in); sums that are not finite give DLM_ST_NONFINITE and NaN; a non-positive pivot DLM_ST_NOT_PD and NaN in that row.
 * The sums are taken in a fixed order without atomics: a panel's output depends on neither N nor its neighbours.
 *
 * Draws: a Philox stream of their own, counter (opts->seed, opts->series_offset + n, iteration, slot): slot t, attempt j for the
 * factors' normals; at the top of the field one slot for the Gamma of sigma^2 and one per row of beta (attempt j: its entry j).
 * Limits: N >= 1, 2 <= T < 2^21 - 64, N ceil(T / 256) < 2^31; k or p outside their limits, a non-positive beta_sd, shape or scale
 * and literal outside {0, 1} are DLM_ERR_ARG.  opts: mem, seed, series_offset, DLM_OPT_ASYNC. */
typedef struct {
  int32_t literal;                 /* 1: the reference's arithmetic, Q27-Q30 */
  double beta_mean, beta_sd;       /* Gaussian(mean, sd) as Breeze takes it */
  double sigma_shape, sigma_scale; /* InverseGamma prior of sigma^2 */
} dlm_fsv_prior;
int dlm_fsv_factors_batch(dlm_engine* e, int32_t N, int32_t T, int32_t p, int32_t k, const double* y, const double* beta,
                          const double* v, const double* alpha, int32_t literal, uint64_t iteration, const dlm_options* opts,
                          double* f, int32_t* status);
int dlm_fsv_loadings_batch(dlm_engine* e, int32_t N, int32_t T, int32_t p, int32_t k, const double* y, const double* f,
                           const double* beta_in, const double* v_in, const dlm_fsv_prior* prior, uint64_t iteration,
                           const dlm_options* opts, double* beta_out, double* v_out, int32_t* status);

/* The DLM whose observation noise is a factor stochastic-volatility process (DlmFsv.scala:64-318) for N independent panels:
 *   theta_0 ~ N(m0, C0),  theta_t = G theta_{t-1} + w_t,  w_t ~ N(0, W),  W diagonal;
 *   y_t = F_t^T theta_t + beta f_t + eps_t,  eps_t ~ N(0, diag(v)),  f_{j,t} ~ N(0, exp(alpha_{j,t}))   (the factor part as above).
 * The three calls here join dlm_ffbs_batch to the factor sampler's calls; one iteration, everything device-resident:
 *   1 dlm_dlmfsv_center_batch     r_t = y_t - F_t^T theta_{t+1}                                      (factorObs, DlmFsv.scala:173-185)
 *     dlm_dlmfsv_impute_batch     the missing components of a PARTIALLY missing r_t, drawn given its observed ones (Q34)
 *   2 dlm_fsv_factors_batch on r  f | r, alpha, beta, v
 *   3 dlm_sv_mixture_batch, dlm_ar1_ffbs_batch, dlm_sv_params_batch on f: alpha | f, then (phi, mu, sigma_eta) | alpha
 *   4 dlm_fsv_loadings_batch on (r, f): sigma^2, beta
 *   5 dlm_dlmfsv_variance_batch   V_t = beta diag(exp(alpha_{.,t+1})) beta^T + diag(v)               (DlmFsvSystem.calculateVariance, DlmFsvSystem.scala:126-131)
 *   6 dlm_ffbs_batch with params->V = that stream, v_stride = T p p, v_tstride = p p, per-panel W: theta | y, V_{1:T}, W (f integrated out)
 *   7 dlm_dinvgamma_step_batch on its statistics (W_out; V_out is not used): W | theta
 * In this order step 6 followed by the next step 2 is one joint draw of (theta, f).  DlmFsv.sampleStep runs 3, 2, 4, 5, 6, 7, whose
 * next step 3 conditions on the f drawn BEFORE theta was redrawn with f integrated out: not a valid sampler.
 * y[t] belongs to theta[t+1] and alpha[..][t+1].  A wholly missing y_t is missing for every step.  A PARTIALLY missing y_t is partially
 * observed for step 6; the factor calls take a time with any component missing as wholly missing, so the reference's steps 2-4 drop
 * observations that its step 6 uses and do not draw from their full conditionals (Q34).  dlm_dlmfsv_impute_batch completes such a time
 * first: with the factor draw that follows it is one joint draw of (the missing components, f_t) given the observed ones, and the
 * completed panel is what steps 2-4 read.  Without the call the iteration is the reference's.
 *
 * dlm_dlmfsv_center_batch.  model: d <= 64, p <= 64, T, N and F (d x p column-major; f_stride 0, or d p: the table of T); G and the
 * time grid are not read.  y, r [N][T][p]; theta [N][T+1][d] as dlm_ffbs_batch writes it.  r_ti = y_ti - sum_j F_ji theta_{t+1,j}, the
 * sum taken with j ascending; a NaN y_ti stays NaN.  status [N] (nullable): DLM_ST_NONFINITE for a panel with a theta_{t+1,j} that is
 * not finite.  r may be y.
 *
 * dlm_dlmfsv_variance_batch.  1 <= k <= 8, k <= p <= 64.  beta [N][p][k], v [N][p], alpha [N][k][T+1]; V [N][T][p p] gets
 *   V_t(i, j) = sum_l (beta_il beta_jl) exp(alpha_{l,t+1})  (l ascending)  + [i == j] v_i
 * for EVERY t, symmetric bit for bit.  status [N] (nullable): DLM_ST_NONFINITE for a panel with a beta or alpha that is not finite,
 * an exp(alpha) that overflows or a v that is not positive and finite (V is then what the arithmetic gives).
 *
 * dlm_dlmfsv_impute_batch.  r_in, r_out [N][T][p] (r_out may be r_in), beta, v, alpha as above.  A time with all or none of its
 * components finite is copied.  For any other, over its observed components i: P = sum_i beta_i beta_i^T / v_i + diag(exp(-alpha_{.,t+1})),
 * f = P^-1 sum_i beta_i r_ti / v_i + L^-T z (P = L L^T), and every missing r_ti = sum_j beta_ij f_j + sqrt(v_i) z_i.  Draws: a Philox
 * stream of its own, counter (opts->seed, opts->series_offset + n, iteration, slot t): attempt j for z_j, attempt 8 + i for z_i.
 * status [N] (nullable): DLM_ST_NONFINITE for a non-finite beta or a v that is not positive and finite (the panel is copied), and for a
 * non-finite alpha_{j,t+1} or an overflowing exp(-alpha) at a partially missing time; DLM_ST_NOT_PD for a pivot that is not positive
 * (that time is copied).  Limits and their codes: those of dlm_fsv_factors_batch.  opts: mem, seed, series_offset, DLM_OPT_ASYNC.
 *
 * The centring and the variance call draw nothing; a panel's output depends on neither N nor its neighbours in any of the three.
 * Their limits: N, T >= 1, T p < 2^31 - 4096, N ceil(T p / 256) < 2^31 and N ceil(T / 64) < 2^31 (DLM_ERR_ARG); d, p or k outside
 * their limits are DLM_ERR_UNSUPPORTED.  opts: mem, DLM_OPT_ASYNC. */
int dlm_dlmfsv_center_batch(dlm_engine* e, const dlm_model_desc* model, const double* y, const double* theta,
                            const dlm_options* opts, double* r, int32_t* status);
int dlm_dlmfsv_impute_batch(dlm_engine* e, int32_t N, int32_t T, int32_t p, int32_t k, const double* r_in, const double* beta,
                            const double* v, const double* alpha, uint64_t iteration, const dlm_options* opts, double* r_out,
                            int32_t* status);
int dlm_dlmfsv_variance_batch(dlm_engine* e, int32_t N, int32_t T, int32_t p, int32_t k, const double* beta, const double* v,
                              const double* alpha, const dlm_options* opts, double* V, int32_t* status);

/* The DLM whose SYSTEM noise is a factor stochastic-volatility process (DlmFsvSystem.scala:215-344) for N independent panels:
 *   theta_0 ~ N(m0, C0),  theta_t = G theta_{t-1} + beta f_t + eps_t,  eps_t ~ N(0, diag(v)),  f_{j,t} ~ N(0, exp(alpha_{j,t}));
 *   y_t = F_t^T theta_t + nu_t,  nu_t ~ N(0, V),  V diagonal   (beta d x k, v [d]: the factor part as above with p := d).
 * The call here and dlm_dlmfsv_variance_batch join dlm_ffbs_batch to the factor sampler's calls; one iteration, everything device-resident:
 *   1 dlm_dlmfsvsys_innovations_batch  w_t = theta_{t+1} - G theta_t                                 (factorState, DlmFsvSystem.scala:109-117)
 *   2 dlm_fsv_factors_batch on w (p := d)  f | w, alpha, beta, v
 *   3 dlm_sv_mixture_batch, dlm_ar1_ffbs_batch, dlm_sv_params_batch on f: alpha | f, then (phi, mu, sigma_eta) | alpha
 *   4 dlm_fsv_loadings_batch on (w, f): sigma^2, beta
 *   5 dlm_dlmfsv_variance_batch with p := d: W_t = beta diag(exp(alpha_{.,t+1})) beta^T + diag(v)   (calculateVariance, DlmFsvSystem.scala:126-131)
 *   6 dlm_ffbs_batch, the reference-form sampler, with params->W = that stream, w_stride = T d d, w_tstride = d d, per-panel diagonal V
 *     (v_stride = p p), statistics on: theta | y, W_{1:T}, V (f integrated out)
 *   7 dlm_dinvgamma_step_batch on its statistics (V_out; W_out is not used): V | theta, y  (sampleObservationMatrix, DlmFsvSystem.scala:246)
 * In this order step 6 followed by the next steps 1 and 2 is one joint draw of (theta, f).  DlmFsvSystem.sampleStep runs 1, 3, 2, 4, 5, 6,
 * 7, whose step 3 conditions on the f drawn BEFORE theta was redrawn with f integrated out: not a valid sampler.
 * w[t] belongs to alpha[..][t+1], as y[t] does in the calls above.  The innovations are never missing: nothing is completed here, and a
 * missing y is the state draw's business alone.
 *
 * dlm_dlmfsvsys_innovations_batch.  model: d <= 64, T, N and ONE G (d x d column-major, n_g = 1); F, p and the time grid are not read.
 * A g_index table or a dt array (an irregular grid) is DLM_ERR_UNSUPPORTED: the AR(1) volatility has no dt.  theta [N][T+1][d] as
 * dlm_ffbs_batch writes it; w [N][T][d] gets w_ti = theta_{t+1,i} - sum_j G_ij theta_{t,j}, the sum taken with j ascending from 0.
 * status [N] (nullable): DLM_ST_NONFINITE for a panel with a theta that is not finite (w is then what the arithmetic gives).  w must
 * not alias theta.  Draws nothing; a panel's output depends on neither N nor its neighbours.  Limits: N, T >= 1, T d < 2^31 - 4096,
 * N ceil(T d / 256) < 2^31 (DLM_ERR_ARG); d > 64 is DLM_ERR_UNSUPPORTED.  opts: mem, DLM_OPT_ASYNC. */
int dlm_dlmfsvsys_innovations_batch(dlm_engine* e, const dlm_model_desc* model, const double* theta, const dlm_options* opts,
                                    double* w, int32_t* status);

/* Bootstrap particle filter of a dynamic GENERALISED linear model (ParticleFilter.step / likelihood, ParticleFilter.scala:38-85, over the
 * observation models of Dglm.scala:46-175 and package.scala:13-28) for N independent series, P particles each, one wavefront per series:
 *   x_0,i = m0 + chol(C0) z,   x_t,i = G_t x_{t-1,i} + sqrt(dt_t) chol(W) z,   eta_t,i = F_t^T x_t,i,   y_t ~ family(eta_t,i, V).
 * p = 1 (every family reads y(0) and V(0,0)); d <= 16; P a multiple of 64, 64 <= P <= 1024; time-invariant V and W (v_tstride = w_tstride = 0);
 * T <= 2^21 - 2 (the Philox counter's slot field); the cloud lives in LDS, (d + 2.5) P + d^2 doubles of it, which every shape inside these
 * limits is granted on a device with 160 KB of LDS per workgroup; anything else is DLM_ERR_UNSUPPORTED.  V, W, m0, C0 per series or shared
 * through the strides of `params`; `model` as everywhere: F_t, the table of G, g_index, dt (dt == 0: no advance and no noise), NaN = missing y.
 * Families and what V(0,0) = v means (log-densities as the reference writes them):
 *   DLM_OBS_GAUSSIAN  N(eta, v)                                   DLM_OBS_POISSON   Poisson(exp(eta)) at y truncated to an integer (toInt)
 *   DLM_OBS_NEGBIN    mean exp(eta), size exp(v)                  DLM_OBS_ZIP       zero with probability expit(v), else Poisson(exp(eta)); |y| < 1e-5 is a zero
 *   DLM_OBS_STUDENTT  location eta, scale sqrt(v), obs_param[n] degrees of freedom (obs_param required, > 0)
 *   DLM_OBS_BETA      mean logisticFunction(1)(eta) (0 below -5, 1 above 5), variance v; parameters that are not positive give the particle
 *                     the weight 0 (the reference's Beta constructor throws, Q41)
 * Per step t, W_{-1,i} = 1 / P:  advance every particle; a missing y_t ends the step there (time does advance, Q38).  Otherwise
 *   l_i = log p(y_t | eta_t,i, v),  m = max l_i,  w_i = exp(l_i - m),  omega_i = W_{t-1,i} w_i,  s = sum omega_i,
 *   ll += m + log s,  W_t,i = omega_i / s,  ESS = floor(1 / sum W_t,i^2);  ESS < n0: multinomial resampling -- new particle i is a copy of the first j
 *   whose inclusive cumulative weight exceeds u_i times the last one, u_i an independent [0, 1) uniform -- and W_t,i = 1 / P.
 * pf->n0 < 0 stands for floor(P / 5) (ParticleFilter.likelihood); n0 = 0 never resamples, n0 > P always.
 * pf->literal = 1 is the reference's arithmetic: the weights of a step that did not resample are forgotten (W_{t-1,i}
 * = 1 / P at every step); with ONE G (n_g = 1) a missing step does not advance the time, so the next step advances the cloud over both
 * intervals again; the Student-t normaliser 0.5 log(pi nu scale).
 * Outputs: ll [N]; mean [N][T][d] (nullable) sum_i W_t,i x_t,i before any resampling; ess [N][T] (nullable; a missing step repeats the last
 * value, P before the first); cloud [N][d][P] and weights [N][P] (nullable) after the last step; status [N] (nullable).
 * A series whose m is not finite or whose s is not positive and finite gets DLM_ST_NONFINITE, one whose chol(W) or chol(C0) meets a pivot that
 * is not positive DLM_ST_NOT_PD; either has ll = -inf (a Metropolis step rejects it), NaN in mean and ess from that step on and in weights,
 * and does no further step.  The batch completes.
 * Draws: Philox streams of their own (DLM_KEY_PF, dlm_draws.h), counter (opts->seed, opts->series_offset + n, iteration, slot t, particle i):
 * block q gives the normals of the components 2 q and 2 q + 1, block 8 the resampling uniform.  Every sum runs in a fixed order without
 * atomics: a series' results depend on neither N nor its neighbours nor on how the batch is split.
 * opts: mem, seed, series_offset, DLM_OPT_ASYNC.  The call reads the model's tables and analyses nothing: it does not count as the "previous
 * model-taking call" of DLM_OPT_MODEL_UNCHANGED. */
enum { DLM_OBS_GAUSSIAN = 0, DLM_OBS_POISSON = 1, DLM_OBS_NEGBIN = 2, DLM_OBS_ZIP = 3, DLM_OBS_STUDENTT = 4, DLM_OBS_BETA = 5 };
typedef struct {
  int32_t family;       /* DLM_OBS_*                                                   */
  int32_t n_particles;  /* P                                                           */
  int32_t n0;           /* resample when ESS < n0; < 0: floor(P / 5)                   */
  int32_t literal;      /* 1: the reference's arithmetic, Q37-Q39                      */
} dlm_pf_desc;
int dlm_pf_batch(dlm_engine* e, const dlm_model_desc* model, const dlm_params_desc* params, const dlm_pf_desc* pf,
                 const double* obs_param, const double* y, uint64_t iteration, const dlm_options* opts, double* ll,
                 double* mean, double* ess, double* cloud, double* weights, int32_t* status);

/* dlm_pf_batch with the resampling scheme chosen (the `resample` argument of ParticleFilter(n, n0, resample), ParticleFilter.scala:26-30): every
 * argument, shape, limit, output, status and draw as in dlm_pf_batch, and one more descriptor.  Only the ANCESTOR step of a resampling differs;
 * the ESS test, the gather, W_t,i = 1 / P afterwards, ll, mean and ess are dlm_pf_batch's.  With cum_j the inclusive cumulative weights, their last
 * one `total`, anc(target) the first j with cum_j > target (P - 1 when none is) and u_i the [0, 1) uniform of block 8 of (slot t, particle i):
 *   DLM_RESAMPLE_MULTINOMIAL  anc_i = anc(u_i total): dlm_pf_batch, bit for bit (dlm_pf_batch IS this call with {DLM_RESAMPLE_MULTINOMIAL, 0})
 *   DLM_RESAMPLE_STRATIFIED   anc_i = anc(((i + u_i) / P) total): one uniform per stratum [i / P, (i + 1) / P)
 *   DLM_RESAMPLE_SYSTEMATIC   anc_i = anc(((i + u_0) / P) total): ONE uniform, particle 0's; the other P - 1 blocks of the step are not drawn
 *   DLM_RESAMPLE_METROPOLIS   mh_steps = b, 1 <= b <= 64; no cumulative weights.  Particle i starts at k = i; for s = 0 .. b - 1, with (u1, u2) the
 *                             uniforms of block 128 + s of (slot t, particle i): j = min(floor(u2 P), P - 1), and k moves to j when u1 W_k <= W_j
 *                             (a k of weight 0 always moves; there is no division).  anc_i is the last k.
 * The three unbiased schemes keep E[exp(ll)] = the likelihood exactly, for every P and n0 (the offspring counts have the means P W_j); stratified
 * and systematic resampling never have a larger variance of the offspring counts than multinomial, and every count N_j of a systematic step is
 * floor(P W_j) or that plus 1.  The reference's systematicResample is not followed (every index it returns is -1).
 * Metropolis resampling is BIASED for a finite b: a chain forgets its start at the rate 1 - 1 / (P max_j W_j) per step, so that after b steps the
 * ancestors still favour the particles' own indices and E[exp(ll)] is not the likelihood (DESIGN.md 4.27 has the measurements); it is the
 * reference's worked example (metropolisResampling(10), written here without its 0 / 0: Q76) and needs no collective operation, but a
 * particle-marginal Metropolis sampler must not be run on it.
 * DLM_ERR_ARG: resample == NULL, a scheme that is none of the four, mh_steps outside 1 .. 64 under DLM_RESAMPLE_METROPOLIS, mh_steps != 0 under
 * any other scheme; everything dlm_pf_batch answers.  dlm_last_variant: "pf-wave". */
enum { DLM_RESAMPLE_MULTINOMIAL = 0, DLM_RESAMPLE_STRATIFIED = 1, DLM_RESAMPLE_SYSTEMATIC = 2, DLM_RESAMPLE_METROPOLIS = 3 };
typedef struct {
  int32_t scheme;       /* DLM_RESAMPLE_*                                              */
  int32_t mh_steps;     /* b of DLM_RESAMPLE_METROPOLIS, 1 .. 64; 0 under the others   */
} dlm_resample_desc;
int dlm_pf_resampled(dlm_engine* e, const dlm_model_desc* model, const dlm_params_desc* params, const dlm_pf_desc* pf,
                           const dlm_resample_desc* resample, const double* obs_param, const double* y, uint64_t iteration,
                           const dlm_options* opts, double* ll, double* mean, double* ess, double* cloud, double* weights, int32_t* status);

/* Posterior-predictive forecast of a DGLM from a particle cloud (Dglm.forecastParticles, Dglm.scala:305-335): dlm_pf_batch's step, and at every
 * step one draw of the observation per particle, summarised where the draws are.  Shapes, limits, families and LDS as dlm_pf_batch; `model`
 * describes the H = model->T forecast steps (dt[0] the gap from the time of the cloud), y [N][H] with NaN = "forecast, do not update".
 * At entry: cloud0 == NULL draws the initial cloud from (m0, C0) exactly as dlm_pf_batch does (a prior-predictive simulation, or with
 * slot_offset = 0 the filter itself); cloud0 [N][d][P] starts from it, with equal weights when weights0 == NULL, else after ONE multinomial
 * resampling under weights0 [N][P] (non-negative, need not sum to 1), so that every later cloud has equal weights.
 * Per step h (Philox slot fc->slot_offset + h):
 *   1. advance the cloud as dlm_pf_batch does (same key, slot, blocks 0..7);  2. eta_i = F_h^T x_i;
 *   3. ytilde_i ~ family(eta_i, v), drawn EXACTLY (dlm_obs_draws.h; DESIGN.md 4.25: Poisson by inversion below a rate of 10 and Hoermann's PTRS from
 *      there on, NegBin as a Gamma mixture of it, ZIP, Student-t as a Gamma scale mixture, Beta from two Gammas), before any weighting;
 *   4. fmean[h] = (1 / P) sum_i ytilde_i in the fixed order of DESIGN.md 4.19;  5. draws[h][i] = ytilde_i when `draws` is given;
 *   6. the draws are sorted (a bitonic network in LDS) and fquant[h][j] = sorted[ranks[j]];
 *   7. y_h observed: weigh, ll += m + log s, mean[h] = the filtering mean, and ALWAYS resample with block 8 of the slot, as dlm_pf_batch does
 *      with n0 > P (Dglm.scala:322-328).  y_h NaN: mean[h] is the mean of the carried cloud and the step ends.
 * fc->literal as in dlm_pf_batch (Q38, Q39).  ranks is a HOST array of fc->n_ranks entries whatever opts->mem is.
 * A draw that is not finite, or a rate that is not finite or above 1e15 (Beta parameters that are not positive included, Q41), stops the series
 * with DLM_ST_NONFINITE; so do entry weights without a positive finite sum; the other statuses as dlm_pf_batch.  A stopped series has ll = -inf and
 * NaN in fmean, fquant, draws and mean from that step on.  The batch completes.
 * DLM_ERR_ARG: n_ranks outside 0..8, a rank outside [0, P), fquant missing with n_ranks > 0, fmean missing, weights0 without cloud0, slot_offset
 * < 0 and what dlm_pf_batch refuses so; DLM_ERR_UNSUPPORTED: slot_offset + H beyond 2^21 - 2 and the shapes dlm_pf_batch refuses.
 * Draws: DLM_KEY_PF, counter (opts->seed, opts->series_offset + n, iteration, slot, particle); the blocks are listed in dlm_draws.h.  Results
 * depend on neither N nor the neighbours nor how the batch is split.  opts: mem, seed, series_offset, DLM_OPT_ASYNC. */
typedef struct {
  int32_t family;       /* DLM_OBS_*                                                   */
  int32_t n_particles;  /* P                                                           */
  int32_t literal;      /* 1: the reference's arithmetic, Q38, Q39                     */
  int32_t n_ranks;      /* 0..8 order statistics per time                              */
  int64_t slot_offset;  /* step h draws from the Philox slot slot_offset + h           */
} dlm_pf_forecast_desc;
int dlm_pf_forecast_particles(dlm_engine* e, const dlm_model_desc* model, const dlm_params_desc* params, const dlm_pf_forecast_desc* fc,
                          const double* obs_param, const int32_t* ranks, const double* cloud0, const double* weights0, const double* y,
                          uint64_t iteration, const dlm_options* opts, double* fmean, double* fquant, double* draws, double* ll,
                          double* mean, double* cloud, double* weights, int32_t* status);

/* Storvik filter of a dynamic generalised linear model (StorvikFilter.step / filterTs, Storvik.scala:105-189; Storvik 2002): the particle
 * filter above with ONLINE PARAMETER LEARNING.  W is diagonal and unknown, W_kk ~ InverseGamma(prior_w[k][0], prior_w[k][1]) (shape, scale);
 * with sv->learn_v = 1 (DLM_OBS_GAUSSIAN only: the statistic is conjugate for the Gaussian family alone, any other family is DLM_ERR_ARG) so
 * is V ~ InverseGamma(prior_v[0], prior_v[1]); with learn_v = 0 V is params->V as in dlm_pf_batch and prior_v is not read.  params->W is
 * never read, params->V only with learn_v = 0.  prior_v_stride / prior_w_stride: doubles between the priors of consecutive series, 0 = one
 * prior for the batch.  Every particle carries the SCALES bw_k,i (k < d) and bv_i of its own posteriors; the shapes are the same for every
 * particle, aw_k = prior shape + 0.5 (advances so far), av = prior shape + 0.5 (observations so far).  Shapes and limits as dlm_pf_batch,
 * except the LDS: (2 d + 3.5) P + d^2 doubles, which d = 16 with P <= 512 and d <= 8 with P = 1024 are granted on a device with 160 KB per
 * workgroup; more is DLM_ERR_UNSUPPORTED (d = 16, P = 1024).  Per step t, W_{-1,i} = 1 / P:
 *   dt_t != 0:  w_k,i = bw_k,i / Gamma(aw_k, 1),  x'_k,i = (G_t x_i)_k + sqrt(dt_t w_k,i) z_k,i,  bw_k,i += 0.5 (x'_k,i - (G_t x_i)_k)^2 / dt_t;
 *               dt_t == 0: no advance, no draw, no update (the reference divides by zero, Q46);
 *   a missing y_t ends the step there: the means under the carried weights are written, the ESS repeats;
 *   v_i = bv_i / Gamma(av, 1) (learn_v) or V,  l_i = log p(y_t | F_t^T x'_i, v_i),  then m, omega_i, s, ll, W_t,i and the ESS as in dlm_pf_batch;
 *   learn_v:  bv_i += 0.5 (y_t - F_t^T x'_i)^2;
 *   ESS < n0: multinomial resampling as in dlm_pf_batch of the particle's WHOLE tuple (x_i, bw_.,i, bv_i), W_t,i = 1 / P.
 * The statistics are updated before the gather, on the particle that made the move (the reference pairs the states of two different
 * particles there, Q42: not offered).  sv->literal = 1: the weights of a step that did not resample are forgotten (Q43) and the Student-t
 * normaliser is Q39's.  ll estimates log p(y_1:T) with V and W integrated over their priors, without bias on the natural scale (the
 * reference's filter accumulates no likelihood, Q48).
 * Outputs: ll [N]; mean [N][T][d], ess [N][T], cloud [N][d][P], weights [N][P] (nullable) as dlm_pf_batch; scale_mean [N][T][d+1] (nullable)
 * sum_i W_t,i bw_k,i for k < d and sum_i W_t,i bv_i for k = d, before any resampling: divided by (shape - 1) the Rao-Blackwellised posterior
 * means of W_kk and V at time t; scales [N][d+1][P] (nullable) the rows bw_k and bv after the last step.  Without learn_v the entries k = d
 * are NaN.  status [N] (nullable): DLM_ST_NOT_PD for a chol(C0) that fails or a prior shape or scale that is not positive (NaN included),
 * DLM_ST_NONFINITE as in dlm_pf_batch; such a series has ll = -inf, NaN in mean, scale_mean and ess from the failing step on and in weights
 * and scales, and its neighbours are untouched.
 * Draws: the streams DLM_KEY_STORVIK (dlm_draws.h): a pure function of (opts->seed, opts->series_offset + n, iteration, t or the initial
 * slot, particle, what), what = a normal pair, the resampling uniform or attempt j of the Gamma of component k <= d.
 * opts: mem, seed, series_offset, DLM_OPT_ASYNC.  Like dlm_pf_batch the call does not count as the "previous model-taking call" of
 * DLM_OPT_MODEL_UNCHANGED. */
typedef struct {
  int32_t family;       /* DLM_OBS_*                                                   */
  int32_t n_particles;  /* P                                                           */
  int32_t n0;           /* resample when ESS < n0; < 0: floor(P / 5)                   */
  int32_t literal;      /* 1: the reference's arithmetic, Q39 and Q43                  */
  int32_t learn_v;      /* 1: V is learned too (DLM_OBS_GAUSSIAN only)                 */
} dlm_storvik_desc;
int dlm_storvik_batch(dlm_engine* e, const dlm_model_desc* model, const dlm_params_desc* params, const dlm_storvik_desc* sv,
                      const double* prior_v, int64_t prior_v_stride, const double* prior_w, int64_t prior_w_stride,
                      const double* obs_param, const double* y, uint64_t iteration, const dlm_options* opts, double* ll, double* mean,
                      double* ess, double* scale_mean, double* cloud, double* weights, double* scales, int32_t* status);

/* Liu-West filter of a dynamic generalised linear model (LiuAndWestFilter.step, LiuAndWest.scala:47-81; Liu & West 2001), and with a = 1 and
 * prior standard deviations of 0 the auxiliary particle filter for known parameters (AuxFilter.step, AuxFilter.scala:18-56): an auxiliary
 * particle filter whose particles carry their own LOG-VARIANCES psi_k,i -- k < d: log W_kk (W is diagonal, params->W is never read); k = d
 * with lw->learn_v = 1: log V.  learn_v is allowed for DLM_OBS_GAUSSIAN, DLM_OBS_STUDENTT and DLM_OBS_BETA, where v is a positive scale; any
 * other family with learn_v is DLM_ERR_ARG.  With learn_v = 0 V is params->V as in dlm_pf_batch and prior_v is not read.  The priors are
 * independent Gaussians on the log-variances: prior_w [d][2] = (mean, sd) of log W_kk, prior_v [2] = (mean, sd) of log V; prior_v_stride /
 * prior_w_stride: doubles between the priors of consecutive series, 0 = one prior for the batch.  sd = 0 makes the row a KNOWN variance
 * exp(mean): it is neither shrunk nor jittered and takes no draws.  lw->a is the shrinkage, 0 < a <= 1 (anything else, NaN included, is
 * DLM_ERR_ARG); h = sqrt(1 - a^2).  Shapes and limits as dlm_pf_batch, except the LDS: (2 d + 3.5) P + d^2 + d + 1 doubles, which d = 16 with
 * P <= 512 and d <= 8 with P = 1024 are granted on a device with 160 KB per workgroup; more is DLM_ERR_UNSUPPORTED (d = 16, P = 1024).
 *   x_0,i = m0 + chol(C0) z,   psi_k,i = mean_k + sd_k z',   W_{-1,i} = 1 / P.   Per step t, the learned rows being those with sd > 0:
 *   a missing y_t:  x'_k,i = (G_t x_i)_k + sqrt(dt_t exp psi_k,i) z_k,i (dt_t == 0: nothing, Q40); psi and the weights are carried, the outputs
 *               are written under the carried weights, the ESS repeats (the reference has no such branch, Q49).  Otherwise
 *   moments:    pbar_k = sum_i W_{t-1,i} psi_k,i,  s2_k = sum_i W_{t-1,i} (psi_k,i - pbar_k)^2;
 *   look-ahead: m_k,i = a psi_k,i + (1 - a) pbar_k,  mu_i = G_t x_i (dt_t == 0: x_i),  lambda_i = log p(y_t | F_t^T mu_i, exp m_d,i or V);
 *   stage 1:    omega_i = W_{t-1,i} exp(lambda_i - max lambda),  A = sum omega,  ll += max lambda + log A;  ALWAYS resampled: new particle j is a copy
 *               (x, m, lambda) of the first k whose inclusive cumulative omega exceeds u_j times the last one;
 *   propagate:  psi'_r,j = m_r,k + h sqrt(s2_r) z'_r,j,  x'_r,j = mu_r,k + sqrt(dt_t exp psi'_r,j) z_r,j (the state noise uses the NEW variances),
 *               l_j = log p(y_t | F_t^T x'_j, exp psi'_d,j or V) - lambda_k;
 *   stage 2:    m2 = max l,  w_j = exp(l_j - m2),  B = sum w,  ll += m2 + log(B / P),  W_t,j = w_j / B,  ESS = floor(1 / sum W_t,j^2);
 *               ESS < n0: multinomial resampling as in dlm_pf_batch of the WHOLE tuple (x_j, psi_.,j), W_t,j = 1 / P.
 * lw->n0 < 0 stands for floor(P / 5).  lw->literal = 1: s2_k is the unweighted n - 1 variance about the unweighted mean, whatever the weights
 * (varParameters, LiuAndWest.scala:51, Q50); l_j is not reduced by lambda_k (AuxFilter.scala:46, Q51); the Student-t normaliser is Q39's.
 * ll estimates log p(y_1:T) -- for a = 1 without bias on the natural scale, the variances integrated over their priors (the reference's
 * Liu-West filter accumulates no likelihood); for a < 1 the filter is an approximation.
 * Outputs: ll [N]; mean [N][T][d], ess [N][T], cloud [N][d][P], weights [N][P] (nullable) as dlm_pf_batch; psi_mean, psi_var [N][T][d+1]
 * (nullable): sum_j W_t,j psi'_k,j and sum_j W_t,j (psi'_k,j - psi_mean)^2, before the second stage's resampling; psi [N][d+1][P] (nullable)
 * the rows of psi after the last step.  Without learn_v the entries k = d are NaN.  status [N] (nullable): DLM_ST_NOT_PD for a chol(C0) that
 * fails, a prior sd that is negative or NaN or a prior mean that is not finite; DLM_ST_NONFINITE when a maximum is not finite or A or B is
 * not positive and finite; such a series has ll = -inf, NaN in mean, psi_mean, psi_var and ess from the failing step on and in weights and
 * psi, and its neighbours are untouched.
 * Draws: the streams DLM_KEY_LW (dlm_draws.h): a pure function of (opts->seed, opts->series_offset + n, iteration, t or the initial slot,
 * particle, block), block = a pair of state normals, the uniform of either stage, or a pair of the d + 1 log-variance normals.  Every sum
 * runs in a fixed order without atomics.
 * opts: mem, seed, series_offset, DLM_OPT_ASYNC.  Like dlm_pf_batch the call does not count as the "previous model-taking call" of
 * DLM_OPT_MODEL_UNCHANGED. */
typedef struct {
  int32_t family;       /* DLM_OBS_*                                                   */
  int32_t n_particles;  /* P                                                           */
  int32_t n0;           /* the second stage resamples when ESS < n0; < 0: floor(P / 5) */
  int32_t literal;      /* 1: the reference's arithmetic, Q39, Q50 and Q51             */
  int32_t learn_v;      /* 1: log V is learned too (Gaussian, Student-t, Beta)         */
  double a;             /* the shrinkage, 0 < a <= 1                                   */
} dlm_lw_desc;
int dlm_lw_batch(dlm_engine* e, const dlm_model_desc* model, const dlm_params_desc* params, const dlm_lw_desc* lw,
                 const double* prior_v, int64_t prior_v_stride, const double* prior_w, int64_t prior_w_stride,
                 const double* obs_param, const double* y, uint64_t iteration, const dlm_options* opts, double* ll, double* mean,
                 double* ess, double* psi_mean, double* psi_var, double* cloud, double* weights, double* psi, int32_t* status);

/* Rao-Blackwellised particle filter of a Gaussian DLM (RaoBlackwellFilter.scala; Liu & West 2001 with the state integrated out): the Liu-West
 * filter above whose particles carry, in place of a drawn state, the Kalman mean m_i [d] and covariance C_i [d][d] of the state GIVEN their own
 * log-variances psi_k,i -- k < d: log W_kk (W is diagonal, params->W is never read); k = d with rb->learn_v = 1: log V.  The family is
 * Gaussian, so there is no family and no obs_param.  With learn_v = 0 V is params->V (time-invariant) and prior_v is not read.  Priors,
 * strides, known rows (sd = 0) and rb->a (0 < a <= 1, else DLM_ERR_ARG; h = sqrt(1 - a^2)) as dlm_lw_batch.  With every variance known the
 * estimate IS the Kalman filter: ll the prediction-error log-likelihood, mean and cov the filtered moments, ESS = P, no Monte-Carlo error.
 * Shapes and limits as dlm_pf_batch (p = 1, d <= 16, P a multiple of 64 in 64 .. 1024, T <= 2^21 - 2), except the LDS:
 *   (d(d+1)/2 + 2 d + 3.5) P + 64 d(d+1)/2 + 3 d + 1 doubles
 * (the covariances dominate; the 64 d(d+1)/2 are one slot of predicted covariances).  On a device with 160 KB per workgroup that grants
 * P <= 1024 for d <= 3 (d = 3: 130,128 B), 896 for d = 4, 640 for d = 5, 512 for d = 6, 384 for d = 7, 320 for d = 8, 256 for d = 9,
 * 192 for d = 10, 128 for d = 11 and 12 and P = 64 for d = 13 .. 16 (d = 16: 157,832 B); more is DLM_ERR_UNSUPPORTED.
 *   m_0,i = m0,  C_0,i = C0 (its lower triangle is read),  psi_k,i = mean_k + sd_k z',  W_{-1,i} = 1 / P.  Per step t, learned rows: sd > 0;
 *   predict(m, C, psi) stands for  g = G_t^T F_t (dt_t == 0: F_t),  f = g^T m,  Q = g^T C g + dt_t sum_k F_t,k^2 exp psi_k + (exp psi_d or V),
 *   and N(y; f, Q) for -(1/2) log(2 pi Q) - (1/2) (y - f)^2 / Q:
 *   a missing y_t:  m_i <- G_t m_i,  C_i <- G_t C_i G_t^T + dt_t diag(exp psi_k,i) (dt_t == 0: nothing); psi and the weights are carried, the
 *               outputs are written under the carried weights, the ESS repeats (the reference has no such branch, Q60).  Otherwise
 *   moments:    pbar_k, s2_k and the shrinkage mshr_k,i = a psi_k,i + (1 - a) pbar_k as dlm_lw_batch;
 *   look-ahead: (f_i, Q_i) = predict(m_i, C_i, mshr_.,i),  lambda_i = N(y_t; f_i, Q_i): the predictive density of the Kalman step;
 *   stage 1:    omega_i = W_{t-1,i} exp(lambda_i - max lambda),  A = sum omega,  ll += max lambda + log A;  ALWAYS resampled: new particle j is a copy
 *               (m, C, mshr, lambda) of the first k whose inclusive cumulative omega exceeds u_j times the last one;
 *   propagate:  psi'_r,j = mshr_r,k + h sqrt(s2_r) z'_r,j (learned rows),  (f, Q) = predict(m_k, C_k, psi'_.,j),  l_j = N(y_t; f, Q) - lambda_k
 *               (variances that did not move -- a = 1, or every row known -- give l_j = 0 exactly: the same operations on the same numbers);
 *               a = G_t m_k,  R = G_t C_k G_t^T + dt_t diag(exp psi'_k,j) (dt_t == 0: m_k, C_k),  K = R F_t / Q,  m'_j = a + K (y_t - f),
 *               C'_j = (I - K F^T) R (I - K F^T)^T + K v K^T, the Joseph form (KalmanFilter.scala:89-90), its lower triangle kept;
 *   stage 2:    m2 = max l,  w_j = exp(l_j - m2),  B = sum w,  ll += m2 + log(B / P),  W_t,j = w_j / B,  ESS = floor(1 / sum W_t,j^2);
 *               ESS < n0: multinomial resampling as in dlm_pf_batch of the WHOLE tuple (m_j, C_j, psi_.,j), W_t,j = 1 / P.
 * rb->n0 < 0 stands for floor(P / 5).  rb->literal = 1 is the reference's arithmetic where it is a one-line switch: the look-ahead density is
 * N(y_t; f_i, exp mshr_d,i or V), at the predicted mean with the observation variance alone (RaoBlackwellFilter.scala:68-71, Q57); l_j is not
 * reduced by lambda_k (:54, Q58); s2_k is the unweighted n - 1 variance (Q50).  The reference's other departures (Q59-Q62) are not offered.
 * ll estimates log p(y_1:T) with the variances integrated over their priors -- for a = 1 without bias on the natural scale (the reference's
 * filter accumulates no likelihood, Q62); for a < 1 the filter is an approximation.
 * Outputs, all nullable but ll: ll [N]; mean [N][T][d] = sum_j W_t,j m_j; cov [N][T][d][d] = sum_j W_t,j (C_j + (m_j - mean)(m_j - mean)^T), the
 * mixture covariance, full and symmetric bit for bit; ess [N][T]; psi_mean, psi_var [N][T][d+1] as dlm_lw_batch (all of step t before the
 * second stage's resampling); after the last step means [N][d][P], covs [N][d(d+1)/2][P] (the lower triangle by rows: entry (r, c), c <= r,
 * in row r (r + 1) / 2 + c), weights [N][P], psi [N][d+1][P].  Without learn_v the entries k = d are NaN.  status [N] (nullable):
 * DLM_ST_NOT_PD for a prior sd that is negative or NaN, a prior mean that is not finite, or a Q that is not positive (NaN included) in the
 * first observed step, where C0 is first used; DLM_ST_NONFINITE when a maximum is not finite, or A, B or any other Q is not positive and
 * finite.  Such a series has ll = -inf, NaN in the per-step outputs from the failing step on and in means, covs, weights and psi, and its
 * neighbours are untouched bit for bit.
 * Draws: the streams DLM_KEY_RB (dlm_draws.h): a pure function of (opts->seed, opts->series_offset + n, iteration, t or the initial slot,
 * particle, block), block = the uniform of either stage or a pair of the d + 1 log-variance normals; there are no state draws.  Every sum
 * runs in a fixed order without atomics: a series' results depend on neither N nor its neighbours nor on how the
 * batch is split.
 * opts: mem, seed, series_offset, DLM_OPT_ASYNC.  Like dlm_pf_batch the call does not count as the "previous model-taking call" of
 * DLM_OPT_MODEL_UNCHANGED. */
typedef struct {
  int32_t n_particles;  /* P                                                           */
  int32_t n0;           /* the second stage resamples when ESS < n0; < 0: floor(P / 5) */
  int32_t literal;      /* 1: the reference's arithmetic, Q50, Q57 and Q58             */
  int32_t learn_v;      /* 1: log V is learned too                                     */
  double a;             /* the shrinkage, 0 < a <= 1                                   */
} dlm_rb_desc;
int dlm_rb_batch(dlm_engine* e, const dlm_model_desc* model, const dlm_params_desc* params, const dlm_rb_desc* rb,
                 const double* prior_v, int64_t prior_v_stride, const double* prior_w, int64_t prior_w_stride,
                 const double* y, uint64_t iteration, const dlm_options* opts, double* ll, double* mean, double* cov,
                 double* ess, double* psi_mean, double* psi_var, double* means, double* covs, double* weights, double* psi,
                 int32_t* status);

/* Posterior-predictive forecast of a DGLM from the cloud of a LEARNING filter -- dlm_storvik_batch, dlm_lw_batch, and dlm_rb_batch after
 * dlm_rb_state_draw below --, whose particles carry their own variances: dlm_pf_forecast_particles' step with a diagonal state noise
 * w_k,i and an observation scale v_i PER PARTICLE, so that the band keeps the parameter uncertainty the filter was run to obtain.  A pure
 * forecast: nothing is observed, weighted or resampled after the entry, and there is no likelihood; to fold in test-period observations, run
 * the filter over them first and forecast from the cloud it leaves.  `model` describes the H = model->T forecast steps (dt[0] the gap from
 * the time of the cloud) as for dlm_pf_forecast_particles; shapes and families as dlm_pf_batch (p = 1, d <= 16, P a multiple of 64 in
 * 64 .. 1024).  LDS: (2 d + 3.5) P doubles (the cloud, the standard deviations of the state noise, the observation scale, the weights, the
 * row of the draws, the ancestors), which d = 16 with P <= 512 and d <= 8 with P = 1024 are granted on a device with 160 KB per workgroup;
 * more is DLM_ERR_UNSUPPORTED (d = 16, P = 1024), before any launch.  params: V alone is read, and only when pv == NULL (every particle
 * takes v = V[n * v_stride], as the family takes it); W, m0 and C0 are never read.
 * At entry: cloud0 [N][d][P]; the rows pw [N][d][P] of the state variances and pv [N][P] of the observation scale (nullable); weights0
 * [N][P] (nullable: equal weights), non-negative with a positive finite sum, else DLM_ST_NONFINITE: ONE multinomial resampling of the
 * whole tuple (x_i, pw_i, pv_i) with the draws dlm_pf_forecast_particles uses there.  Then the rows become variances by fc->var_kind:
 *   DLM_FC_VAR       they are variances;
 *   DLM_FC_LOGVAR    the variance is exp(row): the rows of `psi` of dlm_lw_batch and dlm_rb_batch;
 *   DLM_FC_IG_SCALE  the rows are the InverseGamma scales of dlm_storvik_batch (`scales`), shapes [d + 1] (V's last, read with pv only) at
 *                    n * shapes_stride (0: shared) their shapes: w_k,i = pw_k,i / Gamma(shape_k, 1), and v_i likewise, drawn ONCE per
 *                    particle after the resampling and held for the whole horizon (the parameters are static).
 * A variance that is not finite or is negative, a zero one under DLM_FC_IG_SCALE or in pv, or a shape that is not positive and finite
 * gives DLM_ST_NOT_PD for that series alone (a zero DLM_FC_VAR / DLM_FC_LOGVAR row of pw is a known, noiseless component).  v of
 * DLM_OBS_NEGBIN and DLM_OBS_ZIP is no variance (a log size, a logit) and of DLM_OBS_POISSON is not read: there it has to be finite only,
 * and pv is taken under DLM_FC_VAR alone.
 * Per step h (Philox slot fc->slot_offset + h):
 *   1. dt_h != 0: x'_k,i = (G_h x_i)_k + sqrt(dt_h) (sqrt(w_k,i) z_k,i), z the state normals of dlm_pf_batch (DLM_KEY_PF, blocks 0..7): a cloud
 *      whose particles all carry diag(W) and V reproduces dlm_pf_forecast_particles with that W and every y NaN bit for bit;
 *   2. eta_i = F_h^T x'_i;  3. ytilde_i ~ family(eta_i, v_i), the exact samplers of dlm_pf_forecast_particles;
 *   4. fmean[h], draws[h][i], the sort, fquant[h][j] = sorted[ranks[j]] and mean[h] (the equal-weight mean of the cloud) as there.
 * ranks is a HOST array of fc->n_ranks entries whatever opts->mem is.  After the last step: cloud [N][d][P]; var_w [N][d][P] and var_v
 * [N][P], the variances the steps used (written at entry: the Gamma draws can be seen); status [N].  Every output but fmean is nullable.
 * A draw or rate that is not finite stops the series with DLM_ST_NONFINITE and NaN in fmean, fquant, draws and mean from that step on; a
 * series stopped at entry has NaN in var_w and var_v too, and with DLM_ST_NOT_PD in cloud.  The batch completes, the neighbours untouched.
 * DLM_ERR_ARG: cloud0, pw or fmean missing; shapes missing with DLM_FC_IG_SCALE; a var_kind that is none of the three; pv given for
 * DLM_OBS_NEGBIN or DLM_OBS_ZIP under DLM_FC_LOGVAR or DLM_FC_IG_SCALE; params->V missing without pv; n_ranks outside 0..8, a rank outside
 * [0, P), fquant missing with n_ranks > 0; slot_offset < 0; a time-varying V (v_tstride != 0) without pv; shapes_stride neither 0 nor >= d + 1;
 * DLM_OBS_STUDENTT without obs_param.  DLM_ERR_UNSUPPORTED: the shapes above, slot_offset + H beyond 2^21 - 2.
 * Draws: DLM_KEY_PF as dlm_pf_forecast_particles (counter (opts->seed, opts->series_offset + n, iteration, slot, particle)), the Gammas
 * under DLM_KEY_FCL at the slot slot_offset (dlm_draws.h).  Results depend on neither N nor the neighbours nor how the batch is split.
 * opts: mem, seed, series_offset, DLM_OPT_ASYNC.  Like dlm_pf_batch the call does not count as the "previous model-taking call" of
 * DLM_OPT_MODEL_UNCHANGED. */
enum { DLM_FC_VAR = 0, DLM_FC_LOGVAR = 1, DLM_FC_IG_SCALE = 2 };
typedef struct {
  int32_t family;       /* DLM_OBS_*                                                   */
  int32_t n_particles;  /* P                                                           */
  int32_t var_kind;     /* DLM_FC_*: what the rows of pw and pv hold                   */
  int32_t n_ranks;      /* 0..8 order statistics per time                              */
  int64_t slot_offset;  /* step h draws from the Philox slot slot_offset + h           */
} dlm_pf_forecast_learned_desc;
int dlm_pf_forecast_learned(dlm_engine* e, const dlm_model_desc* model, const dlm_params_desc* params, const dlm_pf_forecast_learned_desc* fc,
                            const double* obs_param, const int32_t* ranks, const double* cloud0, const double* weights0, const double* pw,
                            const double* pv, const double* shapes, int64_t shapes_stride, uint64_t iteration, const dlm_options* opts,
                            double* fmean, double* fquant, double* draws, double* mean, double* cloud, double* var_w, double* var_v,
                            int32_t* status);

/* A state per particle from the Kalman moments dlm_rb_batch leaves: cloud [N][d][P], x_i = m_i + chol(C_i) z_i from means [N][d][P] and
 * covs [N][d(d+1)/2][P] (the lower triangles by rows), so that dlm_pf_forecast_learned can forecast from the Rao-Blackwellised filter
 * (with its weights and psi; the draw comes BEFORE that call's entry resampling -- either order is valid, this one keeps one entry form).
 * One wavefront per series, a particle's factor in its thread's registers, the Cholesky in the order of operations of the particle
 * filters' own; no LDS.  d <= 16, P a multiple of 64 in 64 .. 1024 (DLM_ERR_UNSUPPORTED otherwise); N, d >= 1, 0 <= slot <= 2^21 - 1,
 * means, covs and cloud required (DLM_ERR_ARG).  A pivot that is not positive (NaN included) in any particle gives the WHOLE series
 * DLM_ST_NOT_PD and NaN in its cloud; nothing else is touched.  Draws: DLM_KEY_RB, counter (opts->seed, opts->series_offset + n, iteration,
 * slot, particle), blocks DLM_RB_BLOCK_STATE + q (dlm_draws.h), which no step of dlm_rb_batch uses: slot = the number of steps filtered
 * is the natural choice.  opts: mem, seed, series_offset, DLM_OPT_ASYNC. */
int dlm_rb_state_draw(dlm_engine* e, int32_t d, int32_t N, int32_t P, const double* means, const double* covs, int64_t slot,
                      uint64_t iteration, const dlm_options* opts, double* cloud, int32_t* status);

/* Posterior-predictive forecasts of the factor stochastic-volatility models (FactorSv, DlmFsv, DlmFsvSystem).  A posterior
 * draw's forecast is, given a future log-volatility path, Gaussian: the two calls here make the paths and summarise the mixture over draws
 * and paths; dlm_dlmfsv_variance_batch (with T = H) and dlm_filter_batch (on all-NaN data, want fq) stand between them.
 *
 * dlm_sv_paths: alpha [N][R][k][H+1], R paths of the k AR(1) log-volatilities of every row -- viewed as [N R][k][H+1] the alpha of
 * dlm_dlmfsv_variance_batch with T = H.  Entry 0 of a path is its start: alpha0 [N][k], or with alpha0 == NULL a draw from the stationary
 * law N(mu, sigma^2 / (1 - phi^2)); entry h = 1 .. H is alpha_h = mu + phi (alpha_{h-1} - mu) + sigma z (StochasticVolatility.stepState;
 * sv [N][k][3] = (phi, mu, sigma_eta), sigma_eta a standard deviation).  One lane per (row, path), the k chains in registers.  Draws:
 * DLM_KEY_SVPATH + j (dlm_draws.h), counter (opts->seed, opts->series_offset + n, iteration, slot h (0: the stationary start), path r):
 * a pure function of those, so the first 64 paths of an R = 128 call are the R = 64 call bit for bit and a row's paths depend on neither
 * N nor the sharding.  1 <= k <= 8, R a multiple of 64 in 64 .. 1024 (DLM_ERR_UNSUPPORTED otherwise); N >= 1, 1 <= H <= 2^21 - 1, sv and
 * alpha required (DLM_ERR_ARG).  A row with a non-finite sv or alpha0: DLM_ST_NONFINITE; else with |phi| >= 1 or sigma <= 0:
 * DLM_ST_NOT_PD; its paths are NaN, other rows untouched.  opts: mem, seed, series_offset, DLM_OPT_ASYNC. */
int dlm_sv_paths(dlm_engine* e, int32_t N, int32_t k, int32_t H, int32_t R, const double* sv, const double* alpha0, uint64_t iteration,
                 const dlm_options* opts, double* alpha, int32_t* status);

/* dlm_gaussian_mixture_summary: for N rows, H times and the equal-weight mixture of C Gaussians N(f_c, Q_c) of dimension p at each,
 *   mean [N][H][p]      sum_c f_c / C
 *   cov  [N][H][p p]    sum_c (Q_c + f_c f_c^T) / C - mean mean^T, the total predictive covariance, symmetric bit for bit
 *   quant [N][H][p][nq] the exact quantiles at probs [nq] of the marginal mixture sum_c N(f_c,i, Q_c,ii) / C
 * Component c of row n at time h is read at f + n f_nstride + c f_cstride + h f_tstride (p doubles; f == NULL: 0) and Q + n q_nstride +
 * c q_cstride + h q_tstride (p p doubles, symmetric), strides in doubles, so nothing is repacked: with rec = p + p p,
 *   the fq records [N C][H+1][rec] of dlm_filter_batch:   f = fq + rec, Q = fq + rec + p (record 0 skipped), nstride = C (H + 1) rec,
 *                                                         cstride = (H + 1) rec, tstride = rec for both
 *   a variance stream [N C][H][p p]:                      f = NULL, Q = the stream, q_nstride = C H p p, q_cstride = H p p, q_tstride = p p
 * Sums run over c ascending in a fixed order, without atomics: a row's result depends on neither N nor its neighbours (dlm_fsv_forecast.hip
 * has the order).  QUANTILES: the mixture's CDF F is solved by bisection safeguarding Newton.  The bracket starts at
 * [min f - (|z| + 1) max s, max f + (|z| + 1) max s], z = normcdfinv(prob), s = sqrt(2 Q_ii); every evaluation moves the end on its side, so
 * the computed F(lo) < prob <= F(hi) throughout.  STOPPING RULE: an exact hit F(x) == prob returns x; otherwise the search ends when hi is the
 * double next to lo and returns hi, so |F(q) - prob| <= density(q) spacing(q) + the rounding of the computed F (below C 2^-52).  No Monte
 * Carlo.  A cell's (f_c,i, s_c) pairs are held in LDS up to C = 4096; beyond that they are packed once into an engine workspace of at most
 * DLM_MIXTURE_WORKSPACE_CAP bytes per launch.  1 <= C <= 2^30 (tested to 2^20; the kernels index the components with an int), p <= 64
 * (DLM_ERR_UNSUPPORTED), 0 <= nq <= 8 with every prob
 * inside (0, 1), N H p < 2^31, strides >= 0, Q, mean, cov required, probs and quant with nq > 0 (DLM_ERR_ARG).  probs is a HOST array
 * whatever opts->mem.  With DLM_MEM_HOST an f and a Q that lie inside one buffer (the fq layout) are staged as ONE range.  A Q_c,ii that is not positive and finite gives the row DLM_ST_NOT_PD, a non-finite f_c,i DLM_ST_NONFINITE; mean_i,
 * the quantiles of cell i and row and column i of cov are NaN.  opts: mem, DLM_OPT_ASYNC. */
#define DLM_MIXTURE_WORKSPACE_CAP (1ll << 30)
typedef struct {
  int32_t N, C, H, p;   /* rows, components per row, times, dimension                  */
  int32_t nq;           /* 0..8 quantiles per cell                                     */
  int64_t f_nstride, f_cstride, f_tstride;   /* in doubles; not read with f == NULL    */
  int64_t q_nstride, q_cstride, q_tstride;
} dlm_mixture_desc;
int dlm_gaussian_mixture_summary(dlm_engine* e, const dlm_mixture_desc* mx, const double* f, const double* Q, const double* probs,
                                 const dlm_options* opts, double* mean, double* cov, double* quant, int32_t* status);

/* Particle Gibbs for a dynamic generalised linear model: ONE draw of the state path x_{0:T} | y, V, W of every series by conditional SMC
 * with ancestor sampling (Andrieu, Doucet & Holenstein 2010; Lindsten, Jordan & Schoen 2014).  It is what ParticleGibbs.scala aims at; the
 * reference's own step is not a valid kernel, so there is no literal mode.  The kernel leaves the law of
 * x_{0:T} | y invariant for ANY P >= 2: started from a draw of it, `path` is a draw of it.  Shapes and limits as dlm_pf_batch (p = 1,
 * d <= 16, P a multiple of 64 in 64 .. 1024, time-invariant V and W, T <= 2^21 - 2, the six families); LDS: dlm_pf_batch's plus d doubles.
 * The path convention is dlm_ffbs_batch's: ref, path [N][T+1][d], record 0 is the state before the first step, y[t] belongs to record
 * t + 1.  Particle P - 1 is the reference particle.  W_{-1,i} = 1 / P;
 *   x_0,i = m0 + chol(C0) z (i < P - 1),  x_0,P-1 = ref_0;   then for t = 0 .. T - 1 -- EVERY step resamples, as ParticleGibbs.step does:
 *   a_t,i (i < P - 1): the first j whose inclusive running sum of W_{t-1} exceeds u_i times the last one;
 *   a_t,P-1: with pg->ancestor_sampling and dt_t != 0 drawn the same way from omega_j = W_{t-1,j} exp(q_j - max q),
 *            q_j = -0.5 |L^-1 (ref_{t+1} - G_t x_t,j)|^2 / dt_t, L = chol(W);  otherwise P - 1 (dt_t = 0: no advance, ref_{t+1} is not read);
 *   x_{t+1,i} = G_t x_{t,a_t,i} + sqrt(dt_t) L z (i < P - 1), x_{t+1,P-1} = ref_{t+1}   (dt_t = 0: x_{t+1,i} = x_{t,a_t,i} for every i);
 *   a missing y_t: W_t,i = 1 / P.  Otherwise l_i = log p(y_t | F_t^T x_{t+1,i}, v), m = max l_i, w_i = exp(l_i - m), s = sum w_i,
 *   ll += m + log(s / P), W_t,i = w_i / s;
 *   at the end k_T ~ W_{T-1} by the same search, path_t = x_t,k_t, k_{t-1} = a_{t-1,k_t}.
 * The trace-back needs the clouds x_t [T+1][d][P] and the ancestors a_t [T][P] of every step: they go to HBM as whole rows of P, into the
 * `clouds` / `ancestors` outputs when they are given and otherwise into an engine workspace of (T + 1) d P doubles + T P int32 a series.
 * A workspace above pg->workspace_cap bytes (0: DLM_PG_WORKSPACE_CAP = 8 GiB) is avoided by splitting the batch into launches of whole
 * series; one series always runs.  A series' results depend on neither N nor its neighbours nor on the split.
 * Outputs: ll [N] (the conditional filter's likelihood estimate; a diagnostic, NOT an unbiased estimate); path [N][T+1][d], which may be
 * the array `ref` itself; stats [N][dlm_stats_len(d, 1, 0)] = [ssy | n | ss (d) | T] of the drawn path in dlm_ffbs_batch's layout --
 * ss_i = sum over the steps with dt_t != 0 of (path_{t+1} - G_t path_t)_i^2 / dt_t, ssy and n over the observed y_t for DLM_OBS_GAUSSIAN
 * and 0 otherwise -- so that dlm_dinvgamma_step_batch is the parameter step.  Nullable traces: path_index [N][T+1] (int32, the k_t);
 * clouds [N][T+1][d][P] and ancestors [N][T][P] (int32), given together or not at all (DLM_ERR_ARG); step_weights [N][T][P] (the W_t).
 * status [N] (nullable): DLM_ST_NOT_PD for a chol(C0) or chol(W) that meets a pivot that is not positive; DLM_ST_NONFINITE for a
 * non-finite entry of `ref` that is read, a maximum that is not finite or a sum that is not positive and finite (the ancestor-sampling
 * sum included).  Such a series has ll = -inf and NaN in path and stats (its traces are what the kernel had written by then); its
 * neighbours are untouched and the batch completes.
 * Draws: the streams DLM_KEY_PG (dlm_draws.h), a pure function of (opts->seed, opts->series_offset + n, iteration, slot t or the initial
 * slot, particle, block): blocks q < 8 the state normals of a free particle, then one block each for a free particle's ancestor uniform,
 * the reference's ancestor uniform and the final index.  Every sum runs in a fixed order without atomics.
 * opts: mem, seed, series_offset, DLM_OPT_ASYNC.  Like dlm_pf_batch the call does not count as the "previous model-taking call" of
 * DLM_OPT_MODEL_UNCHANGED. */
#define DLM_PG_WORKSPACE_CAP (8ll << 30)
typedef struct {
  int32_t family;             /* DLM_OBS_*                                                   */
  int32_t n_particles;        /* P, the reference particle included                          */
  int32_t ancestor_sampling;  /* 1: the reference's ancestor is drawn; 0: plain conditional SMC */
  int64_t workspace_cap;      /* bytes of engine workspace a launch may take; 0: DLM_PG_WORKSPACE_CAP */
} dlm_pg_desc;
int dlm_pg_batch(dlm_engine* e, const dlm_model_desc* model, const dlm_params_desc* params, const dlm_pg_desc* pg,
                 const double* obs_param, const double* y, const double* ref, uint64_t iteration, const dlm_options* opts,
                 double* ll, double* path, double* stats, int32_t* path_index, double* clouds, int32_t* ancestors,
                 double* step_weights, int32_t* status);

/* Per-series log-likelihood by the prediction-error decomposition,
 *   loglik[n] = sum_t log N(y_t^obs ; f_t^obs, Q_t^obs),
 * i.e. KalmanFilter.conditionalLikelihood (KalmanFilter.scala:138-153) summed over the series (steps with no observed
 * component contribute 0).  It is the filter recursion with one scalar reduction per series and no record output, for
 * the callers that evaluate a bank of parameter sets (MetropolisHastings.scala:126-137, RaoBlackwellFilter.scala:43-57;
 * SURVEY 8f #2): params strides select per-series parameters.  loglik [N]; status [N] as for dlm_filter_batch.
 *
 * DLM_OPT_LOGLIK_LITERAL_Q7 selects what the reference's `KalmanFilter.likelihood` (KalmanFilter.scala:299-306) -- the
 * function MetropolisHastings.dlm calls (MetropolisHastings.scala:134, :205) -- really computes: it filters and then
 * sums the TRANSITION density of the filtered means (KalmanFilter.logLikelihood, :175-183),
 *   loglik[n] = sum_{t=1..T} log N(m_t ; g(dt_t) m_{t-1}, W dt_t),     m_0 = the initial state at t0 - 1,
 * with Breeze's MultivariateGaussian.logPdf (Cholesky of W dt).  Every consecutive pair counts, also across a missing
 * observation.  W must be positive definite and every dt > 0 (Breeze's cholesky throws otherwise: here loglik[n] = NaN and
 * DLM_ST_NOT_PD); a W_t stream (w_tstride != 0) is DLM_ERR_UNSUPPORTED (the reference passes the time-invariant p.w).
 * The call filters into an engine workspace of N (T + 1) (d + d^2) doubles first. */
int dlm_loglik_batch(dlm_engine* e, const dlm_model_desc* model, const dlm_params_desc* params,
                     const double* y, const dlm_options* opts, double* loglik, int32_t* status);

/* ---- fused filter + smoother (the headline metric path) ----------------------------
 * KalmanFilter(...).filter followed by Smoothing.backwardsSmoother (KalmanFilter.scala:262-294, Smoothing.scala:57-64)
 * in one call.  filt may be NULL when only the smoothed moments are wanted: the filtered records then stay in an
 * engine workspace (stored packed -- mean + lower triangle -- on the structured d <= 15 path, which cuts the traffic
 * of both passes). */
int dlm_filter_smooth_batch(dlm_engine *e, const dlm_model_desc *model,
                            const dlm_params_desc *params, const double *y,
                            const dlm_options *opts, double *filt, double *smooth,
                            int32_t *status);

/* Device time of the forward (ms[0]) and backward (ms[1]) kernels of the LAST dlm_filter_smooth_batch, dlm_ffbs_batch,
 * dlm_backward_sample_batch, dlm_svd_filter_batch or dlm_svd_ffbs_batch call, from HIP events recorded on the
 * engine's stream around them (a part that did not run reads 0). */
int dlm_last_timing(dlm_engine *e, double ms[2]);

/* Step counters of the LAST call made with DLM_OPT_COUNT_STEPS (synchronises the engine's stream):
 *   out[0]  steps of the forward kernel that took its steady-state (mean-only) path, summed over the series
 *   out[1]  the same for the backward kernel
 *   out[2]  series served by the shared-covariance kernels
 *   out[3]  series of the same call that ran their own covariance recursion (a missing observation)
 * `bench.py` reports out[0..1] / (N T) as `steady_fraction`. */
int dlm_last_counters(dlm_engine *e, uint64_t out[4]);

/* What the LAST dlm_filter_smooth_batch call did about the shared RTS tables (synchronises the engine's stream): */
enum {
  DLM_TABLES_NONE = 0,     /* the call did not go through the shared tables (last variant other than "sparse16-rts-shared") */
  DLM_TABLES_BUILT = 1,    /* it made them (and, without DLM_OPT_NO_TABLE_REUSE, kept them for the next call)              */
  DLM_TABLES_REUSED = 2,   /* it found the kept tables' key equal to its own, byte for byte, and made none                  */
  DLM_TABLES_SKIPPED = 3   /* most of its series had a missing observation: no tables, the kept ones untouched              */
};
int dlm_last_table_reuse(dlm_engine *e, int32_t *out);

/* ---- FFBS + Gibbs sufficient statistics --------------------------------------------
 * Replaces Smoothing.ffbsDlm (Smoothing.scala:173-180) and, when `stats` is given, the
 * sums inside GibbsSampling.sampleObservationMatrix / sampleSystemMatrix
 * (Gibbs.scala:23-78) or GibbsWishart.sampleSystemMatrix (GibbsWishart.scala:16-35).
 *   filt_ws [N][T+1][d+d*d]  the forward pass's records (the caller's to read afterwards); NULL: not wanted -- the engine keeps
 *                            them in a workspace of its own, and where the batch shares V, W, C0 on a regular grid (d <= 15) it
 *                            does not produce them at all: a mean-only forward pass against one covariance table
 *   z       [N][T+1][d]      injected standard normals; NULL = Philox4x32-10 stream
 *                            keyed by (opts->seed, opts->series_offset + n, t, i)
 *   theta   [N][T+1][d]      the draw                     optional
 *   cond    [N][T+1][d+d*d]  conditional (h_t, H_t)       optional
 *   stats   [N][L]           L = dlm_stats_len(d, p, flags):
 *                            [ssy(p) | n(p) | ss(d) | T]            (d-Inverse-Gamma)
 *                            [ssy(p) | n(p) | outer(d*d) | T]       (DLM_OPT_STATS_OUTER)
 * DLM_OPT_FFBS_SIMSMOOTH: draw theta = E[x | y - y+] + x+ with (x+, y+) simulated from the model
 * (Durbin & Koopman 2002): the same distribution as FFBS without a d x d factorisation per step
 * (fast paths: d <= 15, p = 1, structured G, regular grid; or 16 <= d <= 48, p <= 32; otherwise the
 * flag is ignored).  Normals: d + p per record (state noise, then observation noise), so injected z is
 * [N][T+1][d+p]; `cond` is not produced.
 * The draw uses the lower Cholesky factor of H_t (theta = h + L z); the reference's eigSym
 * factor has LAPACK-defined signs and an unseedable RNG, so draw-level parity with Breeze is
 * not defined -- see DESIGN.md. */
int dlm_ffbs_batch(dlm_engine *e, const dlm_model_desc *model, const dlm_params_desc *params,
                   const double *y, const double *z, const dlm_options *opts, double *filt_ws,
                   double *theta, double *cond, double *stats, int32_t *status);
int32_t dlm_stats_len(int32_t d, int32_t p, uint32_t flags);

/* Backward sampling only, from existing filter records (Smoothing.sampleDlm,
 * Smoothing.scala:164-165). */
int dlm_backward_sample_batch(dlm_engine *e, const dlm_model_desc *model,
                              const dlm_params_desc *params, const double *y, const double *filt,
                              const double *z, const dlm_options *opts, double *theta,
                              double *cond, double *stats, int32_t *status);

/* ---- SVD (square-root) filter / sampler -------------------------------------------
 * Replaces SvdFilter.filterDlm (SvdFilter.scala:158-161) and SvdSampler.ffbsDlm
 * (SvdSampler.scala:79-82).  svd_rec [N][T+1][d + d + d*d] = (m_t, dc_t, uc_t) with
 * C_t = uc diag(dc^2) uc^T.  The sampler's backward step uses sqrt(W)^-1 / sqrt(dt_t) (the reference's step leaves dt out: DESIGN.md 2,
 * Q26; DLM_OPT_SVD_SAMPLER_Q9 keeps the literal factor).  d <= 48, p <= 32 (DLM_ERR_UNSUPPORTED beyond): one wavefront per series, the
 * decompositions in LDS; models with d, p <= 16 keep fourteen series per CU, larger ones one. */
int dlm_svd_filter_batch(dlm_engine *e, const dlm_model_desc *model,
                         const dlm_params_desc *params, const double *y,
                         const dlm_options *opts, double *svd_rec, int32_t *status);
int dlm_svd_ffbs_batch(dlm_engine *e, const dlm_model_desc *model, const dlm_params_desc *params,
                       const double *y, const double *z, const dlm_options *opts,
                       double *svd_ws, double *theta, double *stats, int32_t *status);

/* ---- pooled-parameter Gibbs: reduce over series, then over GPUs --------------------
 * dlm_stats_pool sums stats [N][L] over the N series of this shard into pooled[L] (device).
 * dlm_comm_* wrap RCCL (one rank per engine / GPU); dlm_gibbs_suffstats_allreduce is one
 * ncclAllReduce(sum, fp64) of `count` doubles in place.  The only collective on the path. */
int dlm_stats_pool(dlm_engine *e, const double *stats, int32_t N, int32_t L, double *pooled,
                   const dlm_options *opts);
#define DLM_COMM_ID_BYTES 128
int dlm_comm_unique_id(uint8_t id[DLM_COMM_ID_BYTES]);
int dlm_comm_init_rank(dlm_engine *e, int32_t nranks, int32_t rank,
                       const uint8_t id[DLM_COMM_ID_BYTES]);
int dlm_gibbs_suffstats_allreduce(dlm_engine *e, double *stats_dev, int64_t count);

#ifdef __cplusplus
}
#endif
#endif /* DLM_ENGINE_H */
