// xitorch_amd :: what the two FSAI build kernels (xk_fsai.hip, xk_fsai_lu.hip) share: the element algebra, real and
// interleaved complex, and the wave-level ordering of wave-private LDS.
#pragma once
#include "xk_common.h"

namespace xk {

template <typename T> struct alignas(2 * sizeof(T)) fz { T re, im; };

// the element algebra of the kernels, real and interleaved complex
template <typename E> struct FsaiEl;
template <typename T> struct FsaiReal {
  typedef T real;
  static __device__ __forceinline__ T zero() { return T(0); }
  static __device__ __forceinline__ T from_re(T a) { return a; }
  static __device__ __forceinline__ T re(T a) { return a; }
  static __device__ __forceinline__ T add(T a, T b) { return a + b; }
  static __device__ __forceinline__ T msub(T acc, T a, T b) { return acc - a * b; }      // acc - a conj(b)
  static __device__ __forceinline__ T msubu(T acc, T a, T b) { return acc - a * b; }     // acc - a b
  static __device__ __forceinline__ T div_re(T a, T d) { return a / d; }
  static __device__ __forceinline__ T div(T a, T b) { return a / b; }
  static __device__ __forceinline__ T conj(T a) { return a; }
  static __device__ __forceinline__ T abs1(T a) { return fabs(a); }                      // |re| + |im|
  static __device__ __forceinline__ bool is_zero(T a) { return a == T(0); }
  static __device__ __forceinline__ bool finite(T a) { return isfinite(a); }
  static __device__ __forceinline__ T bcast(T a, int src) { return __shfl(a, src, 64); }
};
template <> struct FsaiEl<double> : FsaiReal<double> {};
template <> struct FsaiEl<float> : FsaiReal<float> {};
template <typename T> struct FsaiEl<fz<T>> {
  typedef T real;
  typedef fz<T> E;
  static __device__ __forceinline__ E zero() { return {T(0), T(0)}; }
  static __device__ __forceinline__ E from_re(T a) { return {a, T(0)}; }
  static __device__ __forceinline__ T re(E a) { return a.re; }
  static __device__ __forceinline__ E add(E a, E b) { return {a.re + b.re, a.im + b.im}; }
  static __device__ __forceinline__ E msub(E acc, E a, E b) {                              // acc - a conj(b)
    return {acc.re - (a.re * b.re + a.im * b.im), acc.im - (a.im * b.re - a.re * b.im)};
  }
  static __device__ __forceinline__ E msubu(E acc, E a, E b) {                             // acc - a b
    return {acc.re - (a.re * b.re - a.im * b.im), acc.im - (a.im * b.re + a.re * b.im)};
  }
  static __device__ __forceinline__ E div_re(E a, T d) { return {a.re / d, a.im / d}; }
  static __device__ __forceinline__ E div(E a, E b) {                                      // Smith: no |b|^2 is formed
    if (fabs(b.re) >= fabs(b.im)) {
      const T r = b.im / b.re, d = b.re + b.im * r;
      return {(a.re + a.im * r) / d, (a.im - a.re * r) / d};
    }
    const T r = b.re / b.im, d = b.re * r + b.im;
    return {(a.re * r + a.im) / d, (a.im * r - a.re) / d};
  }
  static __device__ __forceinline__ E conj(E a) { return {a.re, -a.im}; }
  static __device__ __forceinline__ T abs1(E a) { return fabs(a.re) + fabs(a.im); }
  static __device__ __forceinline__ bool is_zero(E a) { return a.re == T(0) && a.im == T(0); }
  static __device__ __forceinline__ bool finite(E a) { return isfinite(a.re) && isfinite(a.im); }
  static __device__ __forceinline__ E bcast(E a, int src) { return {__shfl(a.re, src, 64), __shfl(a.im, src, 64)}; }
};

// LDS written by one lane is read by another lane of the same wave: order the accesses (no workgroup barrier)
__device__ __forceinline__ void fsai_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

}  // namespace xk
