// xitorch_amd :: the complex pair of the kernels that work on interleaved (re, im) storage (xk_krylov.hip's complex
// family, xk_herm_davidson.hip).  T is the underlying real type; element i of an array p sits at p[2 i], p[2 i + 1].
#pragma once
#include "xk_common.h"

namespace xk {

template <typename T> struct cx { T re, im; };
template <typename T> __device__ __forceinline__ cx<T> cmul(cx<T> a, cx<T> b) {
  return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re};
}
template <typename T> __device__ __forceinline__ cx<T> cmulc(cx<T> a, cx<T> b) {   // conj(a) b
  return {a.re * b.re + a.im * b.im, a.re * b.im - a.im * b.re};
}
template <typename T> __device__ __forceinline__ void cfma(cx<T>& acc, cx<T> a, cx<T> b) {   // acc += a b
  acc.re = fma(a.re, b.re, fma(-a.im, b.im, acc.re));
  acc.im = fma(a.re, b.im, fma(a.im, b.re, acc.im));
}
template <typename T> __device__ __forceinline__ void cfmac(cx<T>& acc, cx<T> a, cx<T> b) {  // acc += conj(a) b
  acc.re = fma(a.re, b.re, fma(a.im, b.im, acc.re));
  acc.im = fma(a.re, b.im, fma(-a.im, b.re, acc.im));
}
template <typename T> __device__ __forceinline__ cx<T> cdiv(cx<T> a, cx<T> b) {
  const T d = b.re * b.re + b.im * b.im;
  return {(a.re * b.re + a.im * b.im) / d, (a.im * b.re - a.re * b.im) / d};
}
// `_safedenom` of the reference (xitorch/_impls/linalg/solve.py:437-439): an exact complex zero becomes eps + 0i
template <typename T> __device__ __forceinline__ cx<T> csafe(cx<T> v, T eps) {
  return (v.re == T(0) && v.im == T(0)) ? cx<T>{eps, T(0)} : v;
}
template <typename T> __device__ __forceinline__ cx<T> cld(const T* p, long i) { return {p[2 * i], p[2 * i + 1]}; }
template <typename T> __device__ __forceinline__ void cst(T* p, long i, cx<T> v) { p[2 * i] = v.re; p[2 * i + 1] = v.im; }

}  // namespace xk
