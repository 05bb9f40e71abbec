// xitorch_amd :: the block layout of the fused Krylov step kernels, defined once for xk_krylov.hip (CG, BiCGStab),
// xk_minres.hip and xk_lsmr.hip; xk_gmres.hip and xk_gmres_c.hip take the partial pitch from here.
//
// Every system (batch member x column; S of them) is one length-N vector of a padded (S, ld) array, cut into
// nblk <= KRY_MAX_PART blocks of 256 threads (block_range).  Loads and stores are 16 B vectors.  Reductions are
// two-stage in a fixed order: a producer writes one partial per block (block_partial), a consumer re-reduces the
// partials of its system (reduce_partials, reduce_partials_d).  No atomics: repeated runs give identical bits.
#pragma once
#include "xk_common.h"

namespace xk {

constexpr int KRY_MAX_PART = 64;   // partial sums per system, and the pitch of every partial array

// each block handles the contiguous element range [lo, hi) of system s
__device__ __forceinline__ void block_range(int N, int nblk, int blk, int vn, int& lo, int& hi) {
  const int chunks = (N + vn - 1) / vn;                 // in 16 B vectors
  const int per = (chunks + nblk - 1) / nblk;
  lo = blk * per * vn;
  hi = lo + per * vn;
  const int npad = chunks * vn;
  if (hi > npad) hi = npad;
  if (lo > npad) lo = npad;
}

// the kernel has T, N, ld, nblk; the grid is XK_KRY_GRID(S, nblk)
#define XK_KRY_PROLOGUE                                    \
  typedef typename Vec16<T>::type VT;                      \
  constexpr int VN = Vec16<T>::n;                          \
  const int s = blockIdx.x / nblk;                         \
  const int blk = blockIdx.x - s * nblk;                   \
  int lo, hi;                                              \
  block_range(N, nblk, blk, VN, lo, hi);                   \
  const long base = (long)s * ld;
#define XK_KRY_LOOP for (int j = lo + threadIdx.x * VN; j < hi; j += 256 * VN)
#define XK_KRY_LD(p) (*reinterpret_cast<const VT*>((p) + base + j))
#define XK_KRY_LDNT(p) (ld_stream(reinterpret_cast<const VT*>((p) + base + j)))
#define XK_KRY_ST(p, val) (*reinterpret_cast<VT*>((p) + base + j) = (val))
// (the entry point has `stream`)
#define XK_KRY_GRID(S, nblk) dim3((unsigned)((long)(S) * (nblk))), dim3(256), 0, (hipStream_t)stream

// sum of the `nblk` partials of system s in the vector type (all threads of the block get the value)
template <typename T>
__device__ __forceinline__ T reduce_partials(const T* __restrict__ part, int s, int nblk, T* sh) {
  if (threadIdx.x < 64) {
    T v = (int)threadIdx.x < nblk ? part[(long)s * KRY_MAX_PART + threadIdx.x] : T(0);
    v = wave_sum(v);
    if (threadIdx.x == 0) *sh = v;
  }
  __syncthreads();
  const T r = *sh;
  __syncthreads();
  return r;
}

// the same in double; pstride = 2 takes the real parts of (re, im) pairs (the partials of xk_kry_dots_c*)
template <typename T>
__device__ __forceinline__ double reduce_partials_d(const T* __restrict__ part, int s, int nblk, int pstride,
                                                    double* sh) {
  if (threadIdx.x < 64) {
    double v = (int)threadIdx.x < nblk ? (double)part[((long)s * KRY_MAX_PART + threadIdx.x) * pstride] : 0.0;
    v = wave_sum(v);
    if (threadIdx.x == 0) *sh = v;
  }
  __syncthreads();
  const double r = *sh;
  __syncthreads();
  return r;
}

// the sums `w` of the block's four waves (wave_sum of the per-thread values) added in a fixed order and written by
// thread 0 to partial `blk` of system s; sh4 may not be reused before the next barrier
template <typename T>
__device__ __forceinline__ void block_partial(T w, T* part, int s, int blk, T* sh4) {
  if ((threadIdx.x & 63) == 0) sh4[threadIdx.x >> 6] = w;
  __syncthreads();
  if (threadIdx.x == 0) part[(long)s * KRY_MAX_PART + blk] = (sh4[0] + sh4[1]) + (sh4[2] + sh4[3]);
}
// block sum of the per-thread `v` into that partial, with the barrier after which sh4 serves the next sum
template <typename T>
__device__ __forceinline__ void block_store_partial(T v, T* __restrict__ part, int s, int blk, T* sh4) {
  block_partial(wave_sum(v), part, s, blk, sh4);
  __syncthreads();
}

}  // namespace xk
