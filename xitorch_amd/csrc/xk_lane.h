// xitorch_amd :: lane-level and scalar device helpers shared by the kernels outside the three panel-product files:
// wave-uniform values in scalar registers, v_readlane, the Newton-refined reciprocal and what is built on it, the
// integer hash of the deterministic start vectors, the floating-point limits.  (xk_common.h keeps the wave reductions.)
#pragma once
#include "xk_common.h"

namespace xk {

template <typename T> struct Limits;
template <> struct Limits<double> { static constexpr double eps = 2.220446049250313e-16; static constexpr double tiny = 2.2250738585072014e-308; };
template <> struct Limits<float> { static constexpr float eps = 1.1920929e-07f; static constexpr float tiny = 1.17549435e-38f; };

// a value every lane of the wave holds identically, moved to scalar registers
__device__ __forceinline__ float wave_uniform(float v) {
  return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v)));
}
__device__ __forceinline__ double wave_uniform(double v) {
  const int lo = __builtin_amdgcn_readfirstlane(__double2loint(v));
  const int hi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
  return __hiloint2double(hi, lo);
}

// wave-uniform lane index -> v_readlane (scalar result, no LDS crossbar trip like a variable-index shuffle)
__device__ __forceinline__ double readlane(double v, int l) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), l);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), l);
  return __hiloint2double(hi, lo);
}
__device__ __forceinline__ float readlane(float v, int l) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}
// element r (0-based, wave-uniform) of a vector distributed as slot[t] of lane l <-> element l + 64 t
template <typename T, int NT>
__device__ __forceinline__ T dist_get(const T (&v)[NT], int r) {
  const int t = r >> 6, l = r & 63;
  T out = T(0);
#pragma unroll
  for (int u = 0; u < NT; ++u)
    if (u == t) out = readlane(v[u], l);            // t is wave-uniform: a scalar branch per slot
  return out;
}

// reciprocal to ~1-2 ulp: hardware estimate + Newton steps (a full IEEE division costs ~4x as much on the
// sequential critical paths of the Sturm count and of the triangular solves)
__device__ __forceinline__ double rcp_nr(double x) {
  double r = __builtin_amdgcn_rcp(x);
  r = fma(fma(-x, r, 1.0), r, r);
  r = fma(fma(-x, r, 1.0), r, r);
  return r;
}
__device__ __forceinline__ float rcp_nr(float x) {
  float r = __builtin_amdgcn_rcpf(x);
  r = fmaf(fmaf(-x, r, 1.0f), r, r);
  return r;
}
// Householder reflector of x = (alpha, rest), sigma = |rest|^2: (I - tau v v^T) x = beta e1, v = (1, rest * scale)
template <typename T>
__device__ __forceinline__ void house(T alpha, T sigma, T& tau, T& beta, T& scale) {
  tau = T(0); beta = alpha; scale = T(0);
  if (!(sigma == T(0))) {                                   // (a NaN must poison the result, not be skipped)
    const T nrm = sqrt(alpha * alpha + sigma);
    beta = alpha >= T(0) ? -nrm : nrm;
    tau = (beta - alpha) * rcp_nr(beta);
    scale = rcp_nr(alpha - beta);
  }
}

__device__ __forceinline__ unsigned hash32(unsigned x) {
  x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
  return x;
}

}  // namespace xk
