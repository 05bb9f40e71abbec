// xitorch_amd :: block layout shared by the fused Krylov step kernels (xk_krylov.hip, xk_minres.hip).
#pragma once
#include "xk_common.h"

namespace xk {

constexpr int KRY_MAX_PART = 64;   // partial sums per system

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

}  // namespace xk
