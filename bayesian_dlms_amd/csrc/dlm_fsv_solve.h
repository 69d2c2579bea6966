// The small SPD solve-and-draw of the factor stochastic-volatility kernels (dlm_fsv.hip: k_fsv_factors, k_fsv_loadings; dlm_dlmfsv.hip:
// k_dlmfsv_impute), defined here ONCE; dlm_fsv.hip's header describes the factorisation and the two draws.
#pragma once
#include "dlm_internal.h"

namespace dlm {

// x <- P^-1 x + (L^-T z, or P^-1 z with lit); P: the lower triangle packed by rows, overwritten by L.  false: a pivot was not positive
template <int K>
__device__ __forceinline__ bool fsv_solve_draw(double (&P)[K * (K + 1) / 2], double (&x)[K], const double (&z)[K], bool lit) {
  bool ok = true;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    double s = P[j * (j + 1) / 2 + j];
#pragma unroll
    for (int m = 0; m < j; ++m) s = s - P[j * (j + 1) / 2 + m] * P[j * (j + 1) / 2 + m];
    ok = ok && s > 0.0;
    const double d = sqrt(s);
    P[j * (j + 1) / 2 + j] = d;
#pragma unroll
    for (int i = j + 1; i < K; ++i) {
      double e = P[i * (i + 1) / 2 + j];
#pragma unroll
      for (int m = 0; m < j; ++m) e = e - P[i * (i + 1) / 2 + m] * P[j * (j + 1) / 2 + m];
      P[i * (i + 1) / 2 + j] = e / d;
    }
  }
#pragma unroll
  for (int i = 0; i < K; ++i) {
    double s = lit ? x[i] + z[i] : x[i];
#pragma unroll
    for (int m = 0; m < i; ++m) s = s - P[i * (i + 1) / 2 + m] * x[m];
    x[i] = s / P[i * (i + 1) / 2 + i];
  }
#pragma unroll
  for (int i = K - 1; i >= 0; --i) {
    double s = lit ? x[i] : x[i] + z[i];
#pragma unroll
    for (int m = i + 1; m < K; ++m) s = s - P[m * (m + 1) / 2 + i] * x[m];
    x[i] = s / P[i * (i + 1) / 2 + i];
  }
  return ok;
}

}  // namespace dlm
