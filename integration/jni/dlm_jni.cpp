// JNI glue between the Scala shim (integration/scala/Batched.scala) and the C ABI (include/dlm_engine.h): one native
// method of class com.github.jonnylaw.dlm.gpu.Native per export, nothing else.
//
// Neither a JDK nor <jni.h> exists in the build container or on the GPU box.  The file is therefore checked two ways:
// tests/cpp/jni_glue_check.cpp compiles it against a small functional stand-in for the JNI calls it uses
// (tests/cpp/jni_stub/jni.h) and drives every entry point on the GPU; tests/test_integration_sources.py checks that every
// dlm_* export is bound here and declared @native in Batched.scala.  Build where a JDK is present:
//   g++ -O2 -fPIC -shared -I$JAVA_HOME/include -I$JAVA_HOME/include/linux -Iinclude integration/jni/dlm_jni.cpp
//       -Lbayesian_dlms_amd -ldlm_engine -o libdlm_jni.so
//
// Conventions
//   * Every bulk array crosses as a raw ADDRESS (jlong): a device pointer from bufferAlloc (opts.mem = DLM_MEM_DEVICE, the
//     measured path -- results stay in HBM and are fetched with bufferDownload) or the address of a direct
//     java.nio buffer obtained with Native.address (opts.mem = DLM_MEM_HOST).  0 = NULL.  Nothing is copied through
//     Get<Primitive>ArrayElements.
//   * The three descriptors cross as small long[] arrays in the field order of the C structs:
//       model  = {d, p, T, N, F, fStride, G, nG, gIndex, dt}                                   (dlm_model_desc)
//       params = {V, vStride, W, wStride, m0, m0Stride, C0, c0Stride, vTStride, wTStride}      (dlm_params_desc)
//       opts   = {flags, mem, seed, seriesOffset}                                              (dlm_options)
//   * A non-zero return code becomes a RuntimeException carrying dlm_last_error (Breeze throws on singular systems, the
//     engine reports numerical trouble per series in `status` instead; argument and HIP errors throw).
#if __has_include(<jni.h>)
#include <jni.h>
#include <cstdint>
#include <cstring>
#include "dlm_engine.h"

namespace {
template <class T> T* ptr(jlong a) { return reinterpret_cast<T*>(static_cast<uintptr_t>(a)); }
dlm_engine* eng(jlong h) { return ptr<dlm_engine>(h); }

// returns true when an exception is now pending (the caller returns at once)
bool throw_if(JNIEnv* env, dlm_engine* e, int rc) {
  if (rc == DLM_OK) return false;
  jclass cls = env->FindClass("java/lang/RuntimeException");
  if (cls) env->ThrowNew(cls, e ? dlm_last_error(e) : "dlm engine error");
  return true;
}
bool throw_arg(JNIEnv* env, const char* msg) {
  jclass cls = env->FindClass("java/lang/IllegalArgumentException");
  if (cls) env->ThrowNew(cls, msg);
  return true;
}

struct Desc { dlm_model_desc m; dlm_params_desc q; dlm_options o; };

bool read_opts(JNIEnv* env, jlongArray opts, dlm_options& o) {
  if (!opts || env->GetArrayLength(opts) != 4) return !throw_arg(env, "opts must be long[4] = {flags, mem, seed, seriesOffset}");
  jlong v[4];
  env->GetLongArrayRegion(opts, 0, 4, v);
  o.flags = static_cast<uint32_t>(v[0]); o.mem = static_cast<int32_t>(v[1]);
  o.seed = static_cast<uint64_t>(v[2]); o.series_offset = static_cast<uint64_t>(v[3]);
  return true;
}
bool read_desc(JNIEnv* env, jlongArray model, jlongArray params, jlongArray opts, Desc& d) {
  std::memset(&d, 0, sizeof d);
  if (!model || env->GetArrayLength(model) != 10) return !throw_arg(env, "model must be long[10] = {d, p, T, N, F, fStride, G, nG, gIndex, dt}");
  if (!params || env->GetArrayLength(params) != 10) return !throw_arg(env, "params must be long[10] = {V, vStride, W, wStride, m0, m0Stride, C0, c0Stride, vTStride, wTStride}");
  jlong m[10], q[10];
  env->GetLongArrayRegion(model, 0, 10, m);
  env->GetLongArrayRegion(params, 0, 10, q);
  d.m.d = static_cast<int32_t>(m[0]); d.m.p = static_cast<int32_t>(m[1]); d.m.T = static_cast<int32_t>(m[2]); d.m.N = static_cast<int32_t>(m[3]);
  d.m.F = ptr<const double>(m[4]); d.m.f_stride = m[5]; d.m.G = ptr<const double>(m[6]); d.m.n_g = static_cast<int32_t>(m[7]);
  d.m.g_index = ptr<const int32_t>(m[8]); d.m.dt = ptr<const double>(m[9]);
  d.q.V = ptr<const double>(q[0]); d.q.v_stride = q[1]; d.q.W = ptr<const double>(q[2]); d.q.w_stride = q[3];
  d.q.m0 = ptr<const double>(q[4]); d.q.m0_stride = q[5]; d.q.C0 = ptr<const double>(q[6]); d.q.c0_stride = q[7];
  d.q.v_tstride = q[8]; d.q.w_tstride = q[9];
  return read_opts(env, opts, d.o);
}
}  // namespace

extern "C" {

// ---- lifecycle --------------------------------------------------------------------------------------------------
JNIEXPORT jlong JNICALL Java_com_github_jonnylaw_dlm_gpu_Native_engineCreate(JNIEnv* env, jobject, jint device) {
  dlm_engine* e = nullptr;
  if (dlm_engine_create(device, &e) != DLM_OK) {
    jclass cls = env->FindClass("java/lang/RuntimeException");
    if (cls) env->ThrowNew(cls, "dlm_engine_create failed: no usable HIP device");
    return 0;
  }
  return static_cast<jlong>(reinterpret_cast<uintptr_t>(e));
}
JNIEXPORT void JNICALL Java_com_github_jonnylaw_dlm_gpu_Native_engineDestroy(JNIEnv*, jobject, jlong h) { dlm_engine_destroy(eng(h)); }
JNIEXPORT jstring JNICALL Java_com_github_jonnylaw_dlm_gpu_Native_lastError(JNIEnv* env, jobject, jlong h) { return env->NewStringUTF(dlm_last_error(eng(h))); }
JNIEXPORT jstring JNICALL Java_com_github_jonnylaw_dlm_gpu_Native_version(JNIEnv* env, jobject) { return env->NewStringUTF(dlm_version()); }
JNIEXPORT jstring JNICALL Java_com_github_jonnylaw_dlm_gpu_Native_lastVariant(JNIEnv* env, jobject, jlong h) { return env->NewStringUTF(dlm_last_variant(eng(h))); }
JNIEXPORT void JNICALL Java_com_github_jonnylaw_dlm_gpu_Native_engineSetStream(JNIEnv* env, jobject, jlong h, jlong stream) {
  throw_if(env, eng(h), dlm_engine_set_stream(eng(h), ptr<void>(stream)));
}
JNIEXPORT void JNICALL Java_com_github_jonnylaw_dlm_gpu_Native_engineSync(JNIEnv* env, jobject, jlong h) { throw_if(env, eng(h), dlm_engine_sync(eng(h))); }
JNIEXPORT void JNICALL Java_com_github_jonnylaw_dlm_gpu_Native_engineWaitStream(JNIEnv* env, jobject, jlong h, jlong stream) {
  throw_if(env, eng(h), dlm_engine_wait_stream(eng(h), ptr<void>(stream)));
}
JNIEXPORT void JNICALL Java_com_github_jonnylaw_dlm_gpu_Native_streamWaitEngine(JNIEnv* env, jobject, jlong h, jlong stream) {
  throw_if(env, eng(h), dlm_stream_wait_engine(eng(h), ptr<void>(stream)));
}
// {forward ms, backward ms} of the last fused call
JNIEXPORT jdoubleArray JNICALL Java_com_github_jonnylaw_dlm_gpu_Native_lastTiming(JNIEnv* env, jobject, jlong h) {
  double ms[2] = {0.0, 0.0};
  if (throw_if(env, eng(h), dlm_last_timing(eng(h), ms))) return nullptr;
  jdoubleArray out = env->NewDoubleArray(2);
  if (out) env->SetDoubleArrayRegion(out, 0, 2, ms);
  return out;
}
// {forward steady steps, backward steady steps, series on the shared-covariance path, series on their own recursion} of the last
// call made with DLM_OPT_COUNT_STEPS
JNIEXPORT jlongArray JNICALL Java_com_github_jonnylaw_dlm_gpu_Native_lastCounters(JNIEnv* env, jobject, jlong h) {
  uint64_t c[4] = {0, 0, 0, 0};
  if (throw_if(env, eng(h), dlm_last_counters(eng(h), c))) return nullptr;
  jlong v[4] = {static_cast<jlong>(c[0]), static_cast<jlong>(c[1]), static_cast<jlong>(c[2]), static_cast<jlong>(c[3])};
  jlongArray out = env->NewLongArray(4);
  if (out) env->SetLongArrayRegion(out, 0, 4, v);
  return out;
}

// DLM_TABLES_* of the last filterSmooth call: 0 not through the shared RTS tables, 1 built, 2 reused, 3 skipped
JNIEXPORT jint JNICALL Java_com_github_jonnylaw_dlm_gpu_Native_lastTableReuse(JNIEnv* env, jobject, jlong h) {
  int32_t v = 0;
  if (throw_if(env, eng(h), dlm_last_table_reuse(eng(h), &v))) return 0;
  return static_cast<jint>(v);
}

// ---- engine-owned device buffers ----------------------------------------------------------------------------------
// address of a direct java.nio buffer (host mode, and the host side of upload / download)
JNIEXPORT jlong JNICALL Java_com_github_jonnylaw_dlm_gpu_Native_address(JNIEnv* env, jobject, jobject directBuffer) {
  void* a = directBuffer ? env->GetDirectBufferAddress(directBuffer) : nullptr;
  if (directBuffer && !a) { throw_arg(env, "not a direct buffer"); return 0; }
  return static_cast<jlong>(reinterpret_cast<uintptr_t>(a));
}
JNIEXPORT jlong JNICALL Java_com_github_jonnylaw_dlm_gpu_Native_bufferAlloc(JNIEnv* env, jobject, jlong h, jlong bytes) {
  void* p = nullptr;
  if (bytes <= 0) { throw_arg(env, "bufferAlloc: bytes must be positive"); return 0; }
  if (throw_if(env, eng(h), dlm_buffer_alloc(eng(h), static_cast<uint64_t>(bytes), &p))) return 0;
  return static_cast<jlong>(reinterpret_cast<uintptr_t>(p));
}
JNIEXPORT void JNICALL Java_com_github_jonnylaw_dlm_gpu_Native_bufferFree(JNIEnv* env, jobject, jlong h, jlong dev) {
  throw_if(env, eng(h), dlm_buffer_free(eng(h), ptr<void>(dev)));
}
JNIEXPORT void JNICALL Java_com_github_jonnylaw_dlm_gpu_Native_bufferUpload(JNIEnv* env, jobject, jlong h, jlong dstDev, jlong dstOffset, jlong srcHost, jlong bytes) {
  if (dstOffset < 0 || bytes < 0) { throw_arg(env, "bufferUpload: negative offset or size"); return; }
  throw_if(env, eng(h), dlm_buffer_upload(eng(h), ptr<void>(dstDev), static_cast<uint64_t>(dstOffset), ptr<const void>(srcHost), static_cast<uint64_t>(bytes)));
}
JNIEXPORT void JNICALL Java_com_github_jonnylaw_dlm_gpu_Native_bufferDownload(JNIEnv* env, jobject, jlong h, jlong srcDev, jlong srcOffset, jlong dstHost, jlong bytes) {
  if (srcOffset < 0 || bytes < 0) { throw_arg(env, "bufferDownload: negative offset or size"); return; }
  throw_if(env, eng(h), dlm_buffer_download(eng(h), ptr<const void>(srcDev), static_cast<uint64_t>(srcOffset), ptr<void>(dstHost), static_cast<uint64_t>(bytes)));
}
JNIEXPORT void JNICALL Java_com_github_jonnylaw_dlm_gpu_Native_bufferFill(JNIEnv* env, jobject, jlong h, jlong dstDev, jlong dstOffset, jint byteValue, jlong bytes) {
  if (dstOffset < 0 || bytes < 0) { throw_arg(env, "bufferFill: negative offset or size"); return; }
  throw_if(env, eng(h), dlm_buffer_fill(eng(h), ptr<void>(dstDev), static_cast<uint64_t>(dstOffset), byteValue, static_cast<uint64_t>(bytes)));
}
// {free bytes, total bytes}
JNIEXPORT jlongArray JNICALL Java_com_github_jonnylaw_dlm_gpu_Native_deviceMemInfo(JNIEnv* env, jobject, jlong h) {
  uint64_t f = 0, t = 0;
  if (throw_if(env, eng(h), dlm_device_mem_info(eng(h), &f, &t))) return nullptr;
  jlong v[2] = {static_cast<jlong>(f), static_cast<jlong>(t)};
  jlongArray out = env->NewLongArray(2);
  if (out) env->SetLongArrayRegion(out, 0, 2, v);
  return out;
}
JNIEXPORT jint JNICALL Java_com_github_jonnylaw_dlm_gpu_Native_packedRecordDoubles(JNIEnv*, jobject, jint d) { return dlm_packed_record_doubles(d); }
JNIEXPORT void JNICALL Java_com_github_jonnylaw_dlm_gpu_Native_unpackRecords(JNIEnv* env, jobject, jlong h, jint d, jlong count, jlong packed, jlongArray opts, jlong dense) {
  dlm_options o{};
  if (!read_opts(env, opts, o)) return;
  throw_if(env, eng(h), dlm_unpack_records(eng(h), d, count, ptr<const double>(packed), &o, ptr<double>(dense)));
}

// ---- Kalman filter: KalmanFilter(advanceState(p, mod.g)).filter / filterDlm (KalmanFilter.scala:262-294) ---------------
JNIEXPORT void JNICALL Java_com_github_jonnylaw_dlm_gpu_Native_filter(JNIEnv* env, jobject, jlong h, jlongArray model, jlongArray params, jlongArray opts,
                                                                      jlong y, jlong filt, jlong prior, jlong fq, jlong status) {
  Desc d;
  if (!read_desc(env, model, params, opts, d)) return;
  throw_if(env, eng(h), dlm_filter_batch(eng(h), &d.m, &d.q, ptr<const double>(y), &d.o, ptr<double>(filt), ptr<double>(prior), ptr<double>(fq), ptr<int32_t>(status)));
}
// ---- RTS smoother: Smoothing.backwardsSmoother (Smoothing.scala:31-64) --------------------------------------------------
JNIEXPORT void JNICALL Java_com_github_jonnylaw_dlm_gpu_Native_smooth(JNIEnv* env, jobject, jlong h, jlongArray model, jlongArray params, jlongArray opts,
                                                                      jlong filt, jlong smooth, jlong status) {
  Desc d;
  if (!read_desc(env, model, params, opts, d)) return;
  throw_if(env, eng(h), dlm_smooth_batch(eng(h), &d.m, &d.q, ptr<const double>(filt), &d.o, ptr<double>(smooth), ptr<int32_t>(status)));
}
// ---- fused filter + smoother (the metric path) --------------------------------------------------------------------------
JNIEXPORT void JNICALL Java_com_github_jonnylaw_dlm_gpu_Native_filterSmooth(JNIEnv* env, jobject, jlong h, jlongArray model, jlongArray params, jlongArray opts,
                                                                            jlong y, jlong filt, jlong smooth, jlong status) {
  Desc d;
  if (!read_desc(env, model, params, opts, d)) return;
  throw_if(env, eng(h), dlm_filter_smooth_batch(eng(h), &d.m, &d.q, ptr<const double>(y), &d.o, ptr<double>(filt), ptr<double>(smooth), ptr<int32_t>(status)));
}
// ---- log-likelihood: sum of KalmanFilter.conditionalLikelihood (KalmanFilter.scala:138-153) --------------------------------
JNIEXPORT void JNICALL Java_com_github_jonnylaw_dlm_gpu_Native_loglik(JNIEnv* env, jobject, jlong h, jlongArray model, jlongArray params, jlongArray opts,
                                                                      jlong y, jlong loglik, jlong status) {
  Desc d;
  if (!read_desc(env, model, params, opts, d)) return;
  throw_if(env, eng(h), dlm_loglik_batch(eng(h), &d.m, &d.q, ptr<const double>(y), &d.o, ptr<double>(loglik), ptr<int32_t>(status)));
}
// ---- Dlm.simulateRegular (Dlm.scala:245-292) -------------------------------------------------------------------------------
JNIEXPORT void JNICALL Java_com_github_jonnylaw_dlm_gpu_Native_simulate(JNIEnv* env, jobject, jlong h, jlongArray model, jlongArray params, jlongArray opts,
                                                                        jlong x, jlong y, jlong status) {
  Desc d;
  if (!read_desc(env, model, params, opts, d)) return;
  throw_if(env, eng(h), dlm_simulate_batch(eng(h), &d.m, &d.q, &d.o, ptr<double>(x), ptr<double>(y), ptr<int32_t>(status)));
}
// ---- FFBS + Gibbs sufficient statistics: Smoothing.ffbsDlm (Smoothing.scala:173-180), sums of Gibbs.scala:23-78 ---------------
JNIEXPORT void JNICALL Java_com_github_jonnylaw_dlm_gpu_Native_ffbs(JNIEnv* env, jobject, jlong h, jlongArray model, jlongArray params, jlongArray opts,
                                                                    jlong y, jlong z, jlong filtWs, jlong theta, jlong cond, jlong stats, jlong status) {
  Desc d;
  if (!read_desc(env, model, params, opts, d)) return;
  throw_if(env, eng(h), dlm_ffbs_batch(eng(h), &d.m, &d.q, ptr<const double>(y), ptr<const double>(z), &d.o, ptr<double>(filtWs), ptr<double>(theta),
                                       ptr<double>(cond), ptr<double>(stats), ptr<int32_t>(status)));
}
JNIEXPORT jint JNICALL Java_com_github_jonnylaw_dlm_gpu_Native_statsLen(JNIEnv*, jobject, jint d, jint p, jint flags) {
  return dlm_stats_len(d, p, static_cast<uint32_t>(flags));
}
// ---- Smoothing.sampleDlm (Smoothing.scala:164-165): backward sampling from existing filter records ---------------------------
JNIEXPORT void JNICALL Java_com_github_jonnylaw_dlm_gpu_Native_backwardSample(JNIEnv* env, jobject, jlong h, jlongArray model, jlongArray params, jlongArray opts,
                                                                              jlong y, jlong filt, jlong z, jlong theta, jlong cond, jlong stats, jlong status) {
  Desc d;
  if (!read_desc(env, model, params, opts, d)) return;
  throw_if(env, eng(h), dlm_backward_sample_batch(eng(h), &d.m, &d.q, ptr<const double>(y), ptr<const double>(filt), ptr<const double>(z), &d.o, ptr<double>(theta),
                                                  ptr<double>(cond), ptr<double>(stats), ptr<int32_t>(status)));
}
// ---- SvdFilter.filterDlm (SvdFilter.scala:158-161), SvdSampler.ffbsDlm (SvdSampler.scala:79-82) ---------------------------------
JNIEXPORT void JNICALL Java_com_github_jonnylaw_dlm_gpu_Native_svdFilter(JNIEnv* env, jobject, jlong h, jlongArray model, jlongArray params, jlongArray opts,
                                                                         jlong y, jlong svdRec, jlong status) {
  Desc d;
  if (!read_desc(env, model, params, opts, d)) return;
  throw_if(env, eng(h), dlm_svd_filter_batch(eng(h), &d.m, &d.q, ptr<const double>(y), &d.o, ptr<double>(svdRec), ptr<int32_t>(status)));
}
JNIEXPORT void JNICALL Java_com_github_jonnylaw_dlm_gpu_Native_svdFfbs(JNIEnv* env, jobject, jlong h, jlongArray model, jlongArray params, jlongArray opts,
                                                                       jlong y, jlong z, jlong svdWs, jlong theta, jlong stats, jlong status) {
  Desc d;
  if (!read_desc(env, model, params, opts, d)) return;
  throw_if(env, eng(h), dlm_svd_ffbs_batch(eng(h), &d.m, &d.q, ptr<const double>(y), ptr<const double>(z), &d.o, ptr<double>(svdWs), ptr<double>(theta),
                                           ptr<double>(stats), ptr<int32_t>(status)));
}
// ---- GibbsSampling.dinvGammaStep on the device (Gibbs.scala:23-78, :134-151) -------------------------------------------------------
JNIEXPORT void JNICALL Java_com_github_jonnylaw_dlm_gpu_Native_dinvgammaStep(JNIEnv* env, jobject, jlong h, jint d, jint p, jint n, jlong stats, jdouble alphaV, jdouble betaV,
                                                                             jdouble alphaW, jdouble betaW, jlong iteration, jlongArray opts, jlong vOut, jlong wOut) {
  dlm_options o{};
  if (!read_opts(env, opts, o)) return;
  throw_if(env, eng(h), dlm_dinvgamma_step_batch(eng(h), d, p, n, ptr<const double>(stats), alphaV, betaV, alphaW, betaW, static_cast<uint64_t>(iteration), &o,
                                                 ptr<double>(vOut), ptr<double>(wOut)));
}
// ---- StudentT.step on the device (StudentTGibbs.scala:182-212), after the FFBS call of its state draw --------------------------------
// The prior crosses as four doubles (dlm_studentt_prior's field order); model = the usual long[10] (F, d, T, N are read).
JNIEXPORT void JNICALL Java_com_github_jonnylaw_dlm_gpu_Native_studenttStep(JNIEnv* env, jobject, jlong h, jlongArray model, jlong y, jlong theta, jlong stats,
                                                                            jdouble priorNuRate, jdouble propNuSize, jdouble priorWShape, jdouble priorWScale,
                                                                            jlong scaleIn, jlong nuIn, jlong iteration, jlongArray opts, jlong vOut,
                                                                            jlong scaleOut, jlong nuOut, jlong wOut, jlong accepted, jlong loglik, jlong status) {
  if (!model || env->GetArrayLength(model) != 10) { throw_arg(env, "model must be long[10] = {d, p, T, N, F, fStride, G, nG, gIndex, dt}"); return; }
  jlong m[10];
  env->GetLongArrayRegion(model, 0, 10, m);
  dlm_model_desc md{};
  md.d = static_cast<int32_t>(m[0]); md.p = static_cast<int32_t>(m[1]); md.T = static_cast<int32_t>(m[2]); md.N = static_cast<int32_t>(m[3]);
  md.F = ptr<const double>(m[4]); md.f_stride = m[5]; md.G = ptr<const double>(m[6]); md.n_g = static_cast<int32_t>(m[7]);
  md.g_index = ptr<const int32_t>(m[8]); md.dt = ptr<const double>(m[9]);
  dlm_options o{};
  if (!read_opts(env, opts, o)) return;
  const dlm_studentt_prior pr{priorNuRate, propNuSize, priorWShape, priorWScale};
  throw_if(env, eng(h), dlm_studentt_step_batch(eng(h), &md, ptr<const double>(y), ptr<const double>(theta), ptr<const double>(stats), &pr,
                                                ptr<const double>(scaleIn), ptr<const int32_t>(nuIn), static_cast<uint64_t>(iteration), &o,
                                                ptr<double>(vOut), ptr<double>(scaleOut), ptr<int32_t>(nuOut), ptr<double>(wOut),
                                                ptr<int32_t>(accepted), ptr<double>(loglik), ptr<int32_t>(status)));
}
// ---- scalar AR(1) / OU FFBS: FilterAr (FilterAr.scala:15-82), FilterOu (FilterOu.scala:7-79) ------------------------------------------
JNIEXPORT void JNICALL Java_com_github_jonnylaw_dlm_gpu_Native_ar1Ffbs(JNIEnv* env, jobject, jlong h, jint n, jint t, jlong y, jlong v, jlong vStride, jlong sv, jlong svStride,
                                                                       jlong z, jlongArray opts, jlong filt, jlong theta, jlong status) {
  dlm_options o{};
  if (!read_opts(env, opts, o)) return;
  throw_if(env, eng(h), dlm_ar1_ffbs_batch(eng(h), n, t, ptr<const double>(y), ptr<const double>(v), vStride, ptr<const double>(sv), svStride, ptr<const double>(z), &o,
                                           ptr<double>(filt), ptr<double>(theta), ptr<int32_t>(status)));
}
JNIEXPORT void JNICALL Java_com_github_jonnylaw_dlm_gpu_Native_ouFfbs(JNIEnv* env, jobject, jlong h, jint n, jint t, jlong times, jlong y, jlong v, jlong vStride, jlong sv,
                                                                      jlong svStride, jlong z, jlongArray opts, jlong filt, jlong theta, jlong status) {
  dlm_options o{};
  if (!read_opts(env, opts, o)) return;
  throw_if(env, eng(h), dlm_ou_ffbs_batch(eng(h), n, t, ptr<const double>(times), ptr<const double>(y), ptr<const double>(v), vStride, ptr<const double>(sv), svStride,
                                          ptr<const double>(z), &o, ptr<double>(filt), ptr<double>(theta), ptr<int32_t>(status)));
}
// ---- the AR(1) stochastic-volatility sampler around ar1Ffbs (StochasticVolatility.scala:112-157, :189-252; StochVolKnots.scala:25-43) ----
// alpha = 0: the initial transform of initialStateAr.  The prior crosses as scalars in dlm_sv_prior's field order.
JNIEXPORT void JNICALL Java_com_github_jonnylaw_dlm_gpu_Native_svMixture(JNIEnv* env, jobject, jlong h, jint n, jint t, jlong y, jlong alpha, jlong iteration, jlongArray opts,
                                                                         jlong ystar, jlong v, jlong k, jlong status) {
  dlm_options o{};
  if (!read_opts(env, opts, o)) return;
  throw_if(env, eng(h), dlm_sv_mixture_batch(eng(h), n, t, ptr<const double>(y), ptr<const double>(alpha), static_cast<uint64_t>(iteration), &o, ptr<double>(ystar),
                                             ptr<double>(v), ptr<int8_t>(k), ptr<int32_t>(status)));
}
JNIEXPORT void JNICALL Java_com_github_jonnylaw_dlm_gpu_Native_svParams(JNIEnv* env, jobject, jlong h, jint n, jint t, jlong alpha, jlong svIn, jint phiUpdate, jint literal,
                                                                        jdouble phiA, jdouble phiB, jdouble muMean, jdouble muSd, jdouble sigmaShape, jdouble sigmaScale,
                                                                        jdouble propLambda, jdouble propTau, jlong iteration, jlongArray opts, jlong svOut, jlong accepted,
                                                                        jlong status) {
  dlm_options o{};
  if (!read_opts(env, opts, o)) return;
  const dlm_sv_prior pr{phiUpdate, literal, phiA, phiB, muMean, muSd, sigmaShape, sigmaScale, propLambda, propTau};
  throw_if(env, eng(h), dlm_sv_params_batch(eng(h), n, t, ptr<const double>(alpha), ptr<const double>(svIn), &pr, static_cast<uint64_t>(iteration), &o, ptr<double>(svOut),
                                            ptr<int32_t>(accepted), ptr<int32_t>(status)));
}
// ---- the OU stochastic-volatility sampler's parameter step after ouFfbs (StochasticVolatility.scala:350-431, :459-478): the prior, the
// proposal's (lambda, tau) and the walks' standard deviations cross as scalars in dlm_sv_ou_prior's field order; accepted is [N][3]
JNIEXPORT void JNICALL Java_com_github_jonnylaw_dlm_gpu_Native_svOuParams(JNIEnv* env, jobject, jlong h, jint n, jint t, jlong times, jlong alpha, jlong svIn, jint literal,
                                                                          jdouble phiA, jdouble phiB, jdouble muMean, jdouble muSd, jdouble sigmaShape, jdouble sigmaScale,
                                                                          jdouble propLambda, jdouble propTau, jdouble deltaSigma, jdouble deltaMu, jlong iteration,
                                                                          jlongArray opts, jlong svOut, jlong accepted, jlong status) {
  dlm_options o{};
  if (!read_opts(env, opts, o)) return;
  const dlm_sv_ou_prior pr{literal, phiA, phiB, muMean, muSd, sigmaShape, sigmaScale, propLambda, propTau, deltaSigma, deltaMu};
  throw_if(env, eng(h), dlm_sv_ou_params_batch(eng(h), n, t, ptr<const double>(times), ptr<const double>(alpha), ptr<const double>(svIn), &pr, static_cast<uint64_t>(iteration),
                                               &o, ptr<double>(svOut), ptr<int32_t>(accepted), ptr<int32_t>(status)));
}
// ---- the knot block sampler of the AR(1) stochastic-volatility state (StochVolKnots.scala:74-176): one red-black sweep over alpha in place; knots [B+1] int32 shared by
// the batch (0 = knots[0] < ... < knots[B] = T + 1, placed as opts' mem says); svStride 3 or 0 (one shared triple); accepted = 0, status = 0: none
JNIEXPORT void JNICALL Java_com_github_jonnylaw_dlm_gpu_Native_svKnots(JNIEnv* env, jobject, jlong h, jint n, jint t, jlong y, jlong knots, jint b, jlong sv, jlong svStride,
                                                                       jlong iteration, jlongArray opts, jlong alpha, jlong accepted, jlong status) {
  dlm_options o{};
  if (!read_opts(env, opts, o)) return;
  throw_if(env, eng(h), dlm_sv_knots_batch(eng(h), n, t, ptr<const double>(y), ptr<const int32_t>(knots), b, ptr<const double>(sv), static_cast<int64_t>(svStride),
                                           static_cast<uint64_t>(iteration), &o, ptr<double>(alpha), ptr<int32_t>(accepted), ptr<int32_t>(status)));
}
// ---- the factor half of the factor stochastic-volatility sampler (FactorSv.scala:168-186, :253-333, :516-541) around the factor chains'
// svMixture / ar1Ffbs / svParams calls; alpha = 0: initialiseFactors; vIn = 0: none.  The prior crosses as scalars in dlm_fsv_prior's field order.
JNIEXPORT void JNICALL Java_com_github_jonnylaw_dlm_gpu_Native_fsvFactors(JNIEnv* env, jobject, jlong h, jint n, jint t, jint p, jint k, jlong y, jlong beta, jlong v, jlong alpha,
                                                                          jint literal, jlong iteration, jlongArray opts, jlong f, jlong status) {
  dlm_options o{};
  if (!read_opts(env, opts, o)) return;
  throw_if(env, eng(h), dlm_fsv_factors_batch(eng(h), n, t, p, k, ptr<const double>(y), ptr<const double>(beta), ptr<const double>(v), ptr<const double>(alpha), literal,
                                              static_cast<uint64_t>(iteration), &o, ptr<double>(f), ptr<int32_t>(status)));
}
JNIEXPORT void JNICALL Java_com_github_jonnylaw_dlm_gpu_Native_fsvLoadings(JNIEnv* env, jobject, jlong h, jint n, jint t, jint p, jint k, jlong y, jlong f, jlong betaIn, jlong vIn,
                                                                           jint literal, jdouble betaMean, jdouble betaSd, jdouble sigmaShape, jdouble sigmaScale, jlong iteration,
                                                                           jlongArray opts, jlong betaOut, jlong vOut, jlong status) {
  dlm_options o{};
  if (!read_opts(env, opts, o)) return;
  const dlm_fsv_prior pr{literal, betaMean, betaSd, sigmaShape, sigmaScale};
  throw_if(env, eng(h), dlm_fsv_loadings_batch(eng(h), n, t, p, k, ptr<const double>(y), ptr<const double>(f), ptr<const double>(betaIn), ptr<const double>(vIn), &pr,
                                               static_cast<uint64_t>(iteration), &o, ptr<double>(betaOut), ptr<double>(vOut), ptr<int32_t>(status)));
}
// ---- the DLM with factor stochastic-volatility noise (DlmFsv.scala:173-185; DlmFsvSystem.scala:126-131): the centred panel for the factor calls above, the missing components of its partially missing times (rOut may be rIn) and the V_t stream for
// ffbs.  The centring reads d, p, T, N and F of the model (model[4] = F, model[5] = f_stride, as make_model lays them out); status = 0: none.
JNIEXPORT void JNICALL Java_com_github_jonnylaw_dlm_gpu_Native_dlmFsvCenter(JNIEnv* env, jobject, jlong h, jlongArray model, jlong y, jlong theta, jlongArray opts, jlong r, jlong status) {
  if (!model || env->GetArrayLength(model) != 10) { throw_arg(env, "model must be long[10] = {d, p, T, N, F, fStride, G, nG, gIndex, dt}"); return; }
  jlong m[10];
  env->GetLongArrayRegion(model, 0, 10, m);
  dlm_model_desc md{};
  md.d = static_cast<int32_t>(m[0]); md.p = static_cast<int32_t>(m[1]); md.T = static_cast<int32_t>(m[2]); md.N = static_cast<int32_t>(m[3]);
  md.F = ptr<const double>(m[4]); md.f_stride = m[5];
  dlm_options o{};
  if (!read_opts(env, opts, o)) return;
  throw_if(env, eng(h), dlm_dlmfsv_center_batch(eng(h), &md,ptr<const double>(y), ptr<const double>(theta), &o, ptr<double>(r), ptr<int32_t>(status)));
}
JNIEXPORT void JNICALL Java_com_github_jonnylaw_dlm_gpu_Native_dlmFsvImpute(JNIEnv* env, jobject, jlong h, jint n, jint t, jint p, jint k, jlong rIn, jlong beta, jlong v, jlong alpha, jlong iteration,
                                                                            jlongArray opts, jlong rOut, jlong status) {
  dlm_options o{};
  if (!read_opts(env, opts, o)) return;
  throw_if(env, eng(h), dlm_dlmfsv_impute_batch(eng(h), n, t, p, k, ptr<const double>(rIn), ptr<const double>(beta), ptr<const double>(v), ptr<const double>(alpha), static_cast<uint64_t>(iteration), &o,
                                                ptr<double>(rOut), ptr<int32_t>(status)));
}
JNIEXPORT void JNICALL Java_com_github_jonnylaw_dlm_gpu_Native_dlmFsvVariance(JNIEnv* env, jobject, jlong h, jint n, jint t, jint p, jint k, jlong beta, jlong v, jlong alpha, jlongArray opts,
                                                                              jlong vOut, jlong status) {
  dlm_options o{};
  if (!read_opts(env, opts, o)) return;
  throw_if(env, eng(h), dlm_dlmfsv_variance_batch(eng(h), n, t, p, k, ptr<const double>(beta), ptr<const double>(v), ptr<const double>(alpha), &o, ptr<double>(vOut), ptr<int32_t>(status)));
}
// ---- the DLM with factor stochastic-volatility SYSTEM noise (DlmFsvSystem.scala:109-117): w = theta_{t+1} - G theta_t for the factor calls above (p := d); dlmFsvVariance then writes the W_t stream for
// ffbs.  Reads d, T, N and G of the model (model[6] = G, model[7] = nG, model[8] = gIndex, model[9] = dt, as make_model lays them out; a gIndex or dt is refused); status = 0: none.
JNIEXPORT void JNICALL Java_com_github_jonnylaw_dlm_gpu_Native_dlmFsvSysInnovations(JNIEnv* env, jobject, jlong h, jlongArray model, jlong theta, jlongArray opts, jlong w, jlong status) {
  if (!model || env->GetArrayLength(model) != 10) { throw_arg(env, "model must be long[10] = {d, p, T, N, F, fStride, G, nG, gIndex, dt}"); return; }
  jlong m[10];
  env->GetLongArrayRegion(model, 0, 10, m);
  dlm_model_desc md{};
  md.d = static_cast<int32_t>(m[0]); md.p = static_cast<int32_t>(m[1]); md.T = static_cast<int32_t>(m[2]); md.N = static_cast<int32_t>(m[3]);
  md.G = ptr<const double>(m[6]); md.n_g = static_cast<int32_t>(m[7]); md.g_index = ptr<const int32_t>(m[8]); md.dt = ptr<const double>(m[9]);
  dlm_options o{};
  if (!read_opts(env, opts, o)) return;
  throw_if(env, eng(h), dlm_dlmfsvsys_innovations_batch(eng(h), &md, ptr<const double>(theta), &o, ptr<double>(w), ptr<int32_t>(status)));
}
// ---- bootstrap particle filter of a dynamic generalised linear model (ParticleFilter.scala:38-85; Dglm.scala:46-175): the log-likelihood estimate of every series, and on request the filtering means, the
// effective sample sizes, the final cloud and its weights (0: not wanted).  dlm_pf_desc crosses as scalars in its field order; obsParam = 0: none (required by the Student-t family).
JNIEXPORT void JNICALL Java_com_github_jonnylaw_dlm_gpu_Native_particleFilter(JNIEnv* env, jobject, jlong h, jlongArray model, jlongArray params, jlongArray opts, jint family, jint nParticles, jint n0,
                                                                              jint literal, jlong obsParam, jlong y, jlong iteration, jlong ll, jlong mean, jlong ess, jlong cloud, jlong weights,
                                                                              jlong status) {
  Desc d;
  if (!read_desc(env, model, params, opts, d)) return;
  const dlm_pf_desc pf{family, nParticles, n0, literal};
  throw_if(env, eng(h), dlm_pf_batch(eng(h), &d.m, &d.q, &pf, ptr<const double>(obsParam), ptr<const double>(y), static_cast<uint64_t>(iteration), &d.o, ptr<double>(ll), ptr<double>(mean),
                                     ptr<double>(ess), ptr<double>(cloud), ptr<double>(weights), ptr<int32_t>(status)));
}
// ---- particleFilter with the resampling scheme chosen (the `resample` argument of ParticleFilter(n, n0, resample)): dlm_resample_desc crosses as scalars in its field order behind dlm_pf_desc's; scheme 0..3 =
// multinomial (particleFilter bit for bit), stratified, systematic, Metropolis with mhSteps = 1..64 chain steps (biased: not for a particle-marginal sampler); mhSteps = 0 under every other scheme.
JNIEXPORT void JNICALL Java_com_github_jonnylaw_dlm_gpu_Native_particleFilterResampled(JNIEnv* env, jobject, jlong h, jlongArray model, jlongArray params, jlongArray opts, jint family, jint nParticles,
                                                                                       jint n0, jint literal, jint scheme, jint mhSteps, jlong obsParam, jlong y, jlong iteration, jlong ll, jlong mean,
                                                                                       jlong ess, jlong cloud, jlong weights, jlong status) {
  Desc d;
  if (!read_desc(env, model, params, opts, d)) return;
  const dlm_pf_desc pf{family, nParticles, n0, literal};
  const dlm_resample_desc rs{scheme, mhSteps};
  throw_if(env, eng(h), dlm_pf_resampled(eng(h), &d.m, &d.q, &pf, &rs, ptr<const double>(obsParam), ptr<const double>(y), static_cast<uint64_t>(iteration), &d.o, ptr<double>(ll),
                                               ptr<double>(mean), ptr<double>(ess), ptr<double>(cloud), ptr<double>(weights), ptr<int32_t>(status)));
}
// ---- posterior-predictive forecast of a dynamic generalised linear model from a particle cloud (Dglm.forecastParticles, Dglm.scala:297-331): the model describes the H forecast steps, y [N][H] with NaN =
// "forecast, do not update".  dlm_pf_forecast_desc crosses as scalars (family, nParticles, literal, slotOffset) and ranks, a long[] of at most 8 order statistics in [0, nParticles) (null or empty: none), which
// the engine reads on the host.  cloud0 [N][d][nParticles] (0: drawn from (m0, C0)), weights0 [N][nParticles] (0: equal).  fmean [N][H] and ll [N] are required; fquant [N][H][ranks.length] with ranks; draws
// [N][H][nParticles], mean [N][H][d], cloud, weights and status are optional (0).
JNIEXPORT void JNICALL Java_com_github_jonnylaw_dlm_gpu_Native_particleForecast(JNIEnv* env, jobject, jlong h, jlongArray model, jlongArray params, jlongArray opts, jint family, jint nParticles, jint literal,
                                                                                jlong slotOffset, jlongArray ranks, jlong obsParam, jlong cloud0, jlong weights0, jlong y, jlong iteration, jlong fmean,
                                                                                jlong fquant, jlong draws, jlong ll, jlong mean, jlong cloud, jlong weights, jlong status) {
  Desc d;
  if (!read_desc(env, model, params, opts, d)) return;
  const jsize nRanks = ranks ? env->GetArrayLength(ranks) : 0;
  if (nRanks > 8) { throw_arg(env, "particleForecast: at most 8 ranks"); return; }
  jlong rk[8] = {0};
  int32_t rk32[8] = {0};
  if (nRanks) env->GetLongArrayRegion(ranks, 0, nRanks, rk);
  for (jsize j = 0; j < nRanks; ++j) {
    if (rk[j] < 0 || rk[j] >= nParticles) { throw_arg(env, "particleForecast: a rank must satisfy 0 <= rank < nParticles"); return; }
    rk32[j] = static_cast<int32_t>(rk[j]);
  }
  const dlm_pf_forecast_desc fc{family, nParticles, literal, static_cast<int32_t>(nRanks), static_cast<int64_t>(slotOffset)};
  throw_if(env, eng(h), dlm_pf_forecast_particles(eng(h), &d.m, &d.q, &fc, ptr<const double>(obsParam), rk32, ptr<const double>(cloud0), ptr<const double>(weights0), ptr<const double>(y),
                                                  static_cast<uint64_t>(iteration), &d.o, ptr<double>(fmean), ptr<double>(fquant), ptr<double>(draws), ptr<double>(ll), ptr<double>(mean), ptr<double>(cloud),
                                                  ptr<double>(weights), ptr<int32_t>(status)));
}
// ---- Storvik filter of a dynamic generalised linear model (Storvik.scala:105-189): the particle filter above with the diagonal of W -- and with learnV = 1 (Gaussian family) V -- learned online from
// InverseGamma priors: priorV [2] = (shape, scale), priorW [d][2], strides in doubles (0: one prior for the batch).  dlm_storvik_desc crosses as scalars in its field order; scaleMean [N][T][d+1] and
// scales [N][d+1][nParticles] are optional (0) like the outputs of particleFilter.
JNIEXPORT void JNICALL Java_com_github_jonnylaw_dlm_gpu_Native_storvikFilter(JNIEnv* env, jobject, jlong h, jlongArray model, jlongArray params, jlongArray opts, jint family, jint nParticles, jint n0,
                                                                             jint literal, jint learnV, jlong priorV, jlong priorVStride, jlong priorW, jlong priorWStride, jlong obsParam, jlong y,
                                                                             jlong iteration, jlong ll, jlong mean, jlong ess, jlong scaleMean, jlong cloud, jlong weights, jlong scales, jlong status) {
  Desc d;
  if (!read_desc(env, model, params, opts, d)) return;
  const dlm_storvik_desc sv{family, nParticles, n0, literal, learnV};
  throw_if(env, eng(h), dlm_storvik_batch(eng(h), &d.m, &d.q, &sv, ptr<const double>(priorV), static_cast<int64_t>(priorVStride), ptr<const double>(priorW), static_cast<int64_t>(priorWStride),
                                          ptr<const double>(obsParam), ptr<const double>(y), static_cast<uint64_t>(iteration), &d.o, ptr<double>(ll), ptr<double>(mean), ptr<double>(ess),
                                          ptr<double>(scaleMean), ptr<double>(cloud), ptr<double>(weights), ptr<double>(scales), ptr<int32_t>(status)));
}
// ---- Liu-West filter of a dynamic generalised linear model (LiuAndWest.scala:47-81; with a = 1 and prior sds of 0 the auxiliary particle filter of AuxFilter.scala): every particle carries its own
// log-variances, Gaussian priors on them: priorV [2] = (mean, sd) of log V, priorW [d][2] of log W_kk, strides in doubles (0: one prior for the batch).  dlm_lw_desc crosses as scalars in its field
// order; psiMean, psiVar [N][T][d+1] and psi [N][d+1][nParticles] are optional (0) like the outputs of particleFilter.
JNIEXPORT void JNICALL Java_com_github_jonnylaw_dlm_gpu_Native_lwFilter(JNIEnv* env, jobject, jlong h, jlongArray model, jlongArray params, jlongArray opts, jint family, jint nParticles, jint n0,
                                                                        jint literal, jint learnV, jdouble a, jlong priorV, jlong priorVStride, jlong priorW, jlong priorWStride, jlong obsParam, jlong y,
                                                                        jlong iteration, jlong ll, jlong mean, jlong ess, jlong psiMean, jlong psiVar, jlong cloud, jlong weights, jlong psi,
                                                                        jlong status) {
  Desc d;
  if (!read_desc(env, model, params, opts, d)) return;
  const dlm_lw_desc lw{family, nParticles, n0, literal, learnV, a};
  throw_if(env, eng(h), dlm_lw_batch(eng(h), &d.m, &d.q, &lw, ptr<const double>(priorV), static_cast<int64_t>(priorVStride), ptr<const double>(priorW), static_cast<int64_t>(priorWStride),
                                     ptr<const double>(obsParam), ptr<const double>(y), static_cast<uint64_t>(iteration), &d.o, ptr<double>(ll), ptr<double>(mean), ptr<double>(ess),
                                     ptr<double>(psiMean), ptr<double>(psiVar), ptr<double>(cloud), ptr<double>(weights), ptr<double>(psi), ptr<int32_t>(status)));
}
// ---- Rao-Blackwellised filter of a Gaussian DLM (RaoBlackwellFilter.scala): the Liu-West filter whose particles carry the Kalman mean and covariance of the state given their own log-variances.
// Priors and strides as lwFilter; dlm_rb_desc crosses as scalars in its field order; every output but ll is optional (0): mean [N][T][d], cov [N][T][d][d], ess [N][T], psiMean, psiVar [N][T][d+1],
// means [N][d][nParticles], covs [N][d(d+1)/2][nParticles], weights [N][nParticles], psi [N][d+1][nParticles], status [N].
JNIEXPORT void JNICALL Java_com_github_jonnylaw_dlm_gpu_Native_rbFilter(JNIEnv* env, jobject, jlong h, jlongArray model, jlongArray params, jlongArray opts, jint nParticles, jint n0, jint literal,
                                                                        jint learnV, jdouble a, jlong priorV, jlong priorVStride, jlong priorW, jlong priorWStride, jlong y, jlong iteration, jlong ll,
                                                                        jlong mean, jlong cov, jlong ess, jlong psiMean, jlong psiVar, jlong means, jlong covs, jlong weights, jlong psi, jlong status) {
  Desc d;
  if (!read_desc(env, model, params, opts, d)) return;
  const dlm_rb_desc rb{nParticles, n0, literal, learnV, a};
  throw_if(env, eng(h), dlm_rb_batch(eng(h), &d.m, &d.q, &rb, ptr<const double>(priorV), static_cast<int64_t>(priorVStride), ptr<const double>(priorW), static_cast<int64_t>(priorWStride),
                                     ptr<const double>(y), static_cast<uint64_t>(iteration), &d.o, ptr<double>(ll), ptr<double>(mean), ptr<double>(cov), ptr<double>(ess), ptr<double>(psiMean),
                                     ptr<double>(psiVar), ptr<double>(means), ptr<double>(covs), ptr<double>(weights), ptr<double>(psi), ptr<int32_t>(status)));
}
// ---- posterior-predictive forecast from the cloud of a learning filter (storvikFilter's cloud / weights / scales, lwFilter's and -- after rbStateDraw -- rbFilter's cloud / weights / psi): particleForecast
// with a diagonal state noise pw [N][d][nParticles] and an observation scale pv [N][nParticles] (0: params' V) per particle, read by varKind (0 variances, 1 log-variances, 2 InverseGamma scales with
// shapes [d+1] at a stride of shapesStride doubles, 0: shared).  A pure forecast: model describes the H steps, there is no y.  dlm_pf_forecast_learned_desc crosses as scalars; ranks as in particleForecast;
// every output but fmean is optional (0).
JNIEXPORT void JNICALL Java_com_github_jonnylaw_dlm_gpu_Native_particleForecastLearned(JNIEnv* env, jobject, jlong h, jlongArray model, jlongArray params, jlongArray opts, jint family, jint nParticles,
                                                                                       jint varKind, jlong slotOffset, jlongArray ranks, jlong obsParam, jlong cloud0, jlong weights0, jlong pw, jlong pv,
                                                                                       jlong shapes, jlong shapesStride, jlong iteration, jlong fmean, jlong fquant, jlong draws, jlong mean, jlong cloud,
                                                                                       jlong varW, jlong varV, jlong status) {
  Desc d;
  if (!read_desc(env, model, params, opts, d)) return;
  const jsize nRanks = ranks ? env->GetArrayLength(ranks) : 0;
  if (nRanks > 8) { throw_arg(env, "particleForecastLearned: at most 8 ranks"); return; }
  jlong rk[8] = {0};
  int32_t rk32[8] = {0};
  if (nRanks) env->GetLongArrayRegion(ranks, 0, nRanks, rk);
  for (jsize j = 0; j < nRanks; ++j) {
    if (rk[j] < 0 || rk[j] >= nParticles) { throw_arg(env, "particleForecastLearned: a rank must satisfy 0 <= rank < nParticles"); return; }
    rk32[j] = static_cast<int32_t>(rk[j]);
  }
  const dlm_pf_forecast_learned_desc fc{family, nParticles, varKind, static_cast<int32_t>(nRanks), static_cast<int64_t>(slotOffset)};
  throw_if(env, eng(h), dlm_pf_forecast_learned(eng(h), &d.m, &d.q, &fc, ptr<const double>(obsParam), rk32, ptr<const double>(cloud0), ptr<const double>(weights0), ptr<const double>(pw),
                                                ptr<const double>(pv), ptr<const double>(shapes), static_cast<int64_t>(shapesStride), static_cast<uint64_t>(iteration), &d.o, ptr<double>(fmean),
                                                ptr<double>(fquant), ptr<double>(draws), ptr<double>(mean), ptr<double>(cloud), ptr<double>(varW), ptr<double>(varV), ptr<int32_t>(status)));
}
// ---- a state per particle from the Kalman moments rbFilter leaves: cloud [N][d][nParticles], x_i = m_i + chol(C_i) z_i, the normals from the Philox slot `slot` of the filter's stream
JNIEXPORT void JNICALL Java_com_github_jonnylaw_dlm_gpu_Native_rbStateDraw(JNIEnv* env, jobject, jlong h, jint d, jint n, jint nParticles, jlong means, jlong covs, jlong slot, jlong iteration,
                                                                           jlongArray opts, jlong cloud, jlong status) {
  dlm_options o{};
  if (!read_opts(env, opts, o)) return;
  throw_if(env, eng(h), dlm_rb_state_draw(eng(h), d, n, nParticles, ptr<const double>(means), ptr<const double>(covs), static_cast<int64_t>(slot), static_cast<uint64_t>(iteration), &o,
                                          ptr<double>(cloud), ptr<int32_t>(status)));
}
// ---- posterior-predictive forecasts of the factor stochastic-volatility models: nPaths future log-volatility paths per row, alpha [N][nPaths][k][H+1] from sv [N][k][3] and the starts alpha0 [N][k]
// (0: the stationary law); status is optional (0)
JNIEXPORT void JNICALL Java_com_github_jonnylaw_dlm_gpu_Native_svPaths(JNIEnv* env, jobject, jlong h, jint n, jint k, jint horizon, jint nPaths, jlong sv, jlong alpha0, jlong iteration, jlongArray opts,
                                                                       jlong alpha, jlong status) {
  dlm_options o{};
  if (!read_opts(env, opts, o)) return;
  throw_if(env, eng(h), dlm_sv_paths(eng(h), n, k, horizon, nPaths, ptr<const double>(sv), ptr<const double>(alpha0), static_cast<uint64_t>(iteration), &o, ptr<double>(alpha), ptr<int32_t>(status)));
}
// ---- ... and the summary of the Gaussian mixture over draws and paths: mean [N][H][p], cov [N][H][p p], quant [N][H][p][nProbs] of the c components per row read through the (row, component,
// time) strides fStrides / qStrides (three longs each, in doubles); f = 0: zero means; probs is a HOST address of nProbs doubles (a direct buffer's) whatever opts' mem; dlm_mixture_desc crosses as scalars and the two arrays
JNIEXPORT void JNICALL Java_com_github_jonnylaw_dlm_gpu_Native_gaussianMixtureSummary(JNIEnv* env, jobject, jlong h, jint n, jint c, jint horizon, jint p, jlongArray fStrides, jlongArray qStrides, jlong f,
                                                                                      jlong q, jlong probs, jint nProbs, jlongArray opts, jlong mean, jlong cov, jlong quant, jlong status) {
  dlm_options o{};
  if (!read_opts(env, opts, o)) return;
  if (nProbs < 0 || nProbs > 8 || (nProbs && !probs)) { throw_arg(env, "gaussianMixtureSummary: 0 <= nProbs <= 8, and probs is a host address with nProbs > 0"); return; }
  if (!fStrides || !qStrides || env->GetArrayLength(fStrides) != 3 || env->GetArrayLength(qStrides) != 3) { throw_arg(env, "gaussianMixtureSummary: fStrides and qStrides hold three strides each"); return; }
  jlong fs[3], qs[3];
  env->GetLongArrayRegion(fStrides, 0, 3, fs);
  env->GetLongArrayRegion(qStrides, 0, 3, qs);
  const dlm_mixture_desc mx{n, c, horizon, p, nProbs, fs[0], fs[1], fs[2], qs[0], qs[1], qs[2]};
  throw_if(env, eng(h), dlm_gaussian_mixture_summary(eng(h), &mx, ptr<const double>(f), ptr<const double>(q), ptr<const double>(probs), &o, ptr<double>(mean), ptr<double>(cov), ptr<double>(quant), ptr<int32_t>(status)));
}
// ---- particle Gibbs for a dynamic generalised linear model (what ParticleGibbs.scala aims at): one conditional-SMC sweep with ancestor sampling per series, the new state path [N][T+1][d] given the path
// `ref` (path may be ref), with the statistics [N][d+3] dinvgammaStep takes.  dlm_pg_desc crosses as scalars in its field order (workspaceCap = 0: the default cap); obsParam = 0: none; pathIndex
// [N][T+1] int32, clouds [N][T+1][d][nParticles] with ancestors [N][T][nParticles] int32, stepWeights [N][T][nParticles] and status are optional (0).
JNIEXPORT void JNICALL Java_com_github_jonnylaw_dlm_gpu_Native_pgSweep(JNIEnv* env, jobject, jlong h, jlongArray model, jlongArray params, jlongArray opts, jint family, jint nParticles,
                                                                       jint ancestorSampling, jlong workspaceCap, jlong obsParam, jlong y, jlong ref, jlong iteration, jlong ll, jlong path, jlong stats,
                                                                       jlong pathIndex, jlong clouds, jlong ancestors, jlong stepWeights, jlong status) {
  Desc d;
  if (!read_desc(env, model, params, opts, d)) return;
  const dlm_pg_desc pg{family, nParticles, ancestorSampling, static_cast<int64_t>(workspaceCap)};
  throw_if(env, eng(h), dlm_pg_batch(eng(h), &d.m, &d.q, &pg, ptr<const double>(obsParam), ptr<const double>(y), ptr<const double>(ref), static_cast<uint64_t>(iteration), &d.o, ptr<double>(ll),
                                     ptr<double>(path), ptr<double>(stats), ptr<int32_t>(pathIndex), ptr<double>(clouds), ptr<int32_t>(ancestors), ptr<double>(stepWeights), ptr<int32_t>(status)));
}
// ---- pooled-parameter Gibbs: reduce over series, then over GPUs (RCCL) ---------------------------------------------------------------
JNIEXPORT void JNICALL Java_com_github_jonnylaw_dlm_gpu_Native_statsPool(JNIEnv* env, jobject, jlong h, jlong stats, jint n, jint l, jlong pooled, jlongArray opts) {
  dlm_options o{};
  if (!read_opts(env, opts, o)) return;
  throw_if(env, eng(h), dlm_stats_pool(eng(h), ptr<const double>(stats), n, l, ptr<double>(pooled), &o));
}
JNIEXPORT jbyteArray JNICALL Java_com_github_jonnylaw_dlm_gpu_Native_commUniqueId(JNIEnv* env, jobject) {
  uint8_t id[DLM_COMM_ID_BYTES];
  if (dlm_comm_unique_id(id) != DLM_OK) {
    jclass cls = env->FindClass("java/lang/RuntimeException");
    if (cls) env->ThrowNew(cls, "dlm_comm_unique_id failed (RCCL)");
    return nullptr;
  }
  jbyteArray out = env->NewByteArray(DLM_COMM_ID_BYTES);
  if (out) env->SetByteArrayRegion(out, 0, DLM_COMM_ID_BYTES, reinterpret_cast<const jbyte*>(id));
  return out;
}
JNIEXPORT void JNICALL Java_com_github_jonnylaw_dlm_gpu_Native_commInitRank(JNIEnv* env, jobject, jlong h, jint nranks, jint rank, jbyteArray id) {
  if (!id || env->GetArrayLength(id) != DLM_COMM_ID_BYTES) { throw_arg(env, "commInitRank: id must be the byte[128] of commUniqueId"); return; }
  uint8_t raw[DLM_COMM_ID_BYTES];
  env->GetByteArrayRegion(id, 0, DLM_COMM_ID_BYTES, reinterpret_cast<jbyte*>(raw));
  throw_if(env, eng(h), dlm_comm_init_rank(eng(h), nranks, rank, raw));
}
JNIEXPORT void JNICALL Java_com_github_jonnylaw_dlm_gpu_Native_gibbsSuffstatsAllreduce(JNIEnv* env, jobject, jlong h, jlong statsDev, jlong count) {
  throw_if(env, eng(h), dlm_gibbs_suffstats_allreduce(eng(h), ptr<double>(statsDev), count));
}

}  // extern "C"
#endif  // __has_include(<jni.h>)
