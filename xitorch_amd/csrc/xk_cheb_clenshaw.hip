// xitorch_amd :: the Clenshaw step of a Chebyshev band-pass filter (Li, Xi, Vecharynski, Yang, Saad, SIAM J. Sci.
// Comput. 38 (2016) A2512), the one pass over the block between two operator applies of symeig(mode="nearest").
//
// An extension (the reference has no interior eigensolver); a sibling of xk_cheb.hip, whose device code it leaves
// alone.  Panels are the (Bt, p, ld) arrays of _panel.py.  For every operator b, column c and n < N
//
//   out[b,c,n] = ((alpha[b] * AY[b,c,n] + beta[b] * Y[b,c,n]) + gamma[b] * Yprev[b,c,n]) + delta[b] * X0[b,c,n]
//
// with (alpha, beta, gamma, delta) = coef[b, 0..3], a DEVICE array of doubles.  In the Clenshaw recurrence
// b_k = (2/e)(A - c) b_{k+1} - b_{k+2} + c_k X the fourth term carries the filter's coefficient times the unfiltered
// block, so the filtered block is assembled without a second accumulator panel: 5 Bt p N s bytes per step (4 where
// gamma = 0) instead of the 7 of two three-term steps.
//
// Every clause of xk_cheb_step's contract holds.  The coefficients are real for all four dtypes: the complex entry
// points run the real kernels on the interleaved storage with N, pitches and batch strides doubled.  f64 / c128
// evaluate in double; f32 / c64 round each coefficient ONCE to float and evaluate in float.  The sum is taken left to
// right as written; products may be contracted into FMAs.  gamma[b] == 0.0 exactly (+0 or -0): Yprev[b] is NOT read
// and may hold NaN / Inf; alpha, beta and delta get no such treatment.  out may be Yprev itself (same pointer, pitch
// and batch stride: every lane reads the elements it writes before it writes them) or an array apart from it.  out
// must not share memory with AY, Y or X0 and its own rows must not overlap: XK_ERR_ARG, nothing launched.  Only
// out[b, c, :N] is written: a vector that straddles N is finished element by element, pads are never touched.
//
// Launch shape of cheb_step: a workgroup of 256 lanes owns one chunk of CLEN_UNR x 256 vectors of one row, grid =
// Bt * p * chunks; each lane issues its 3 or 4 x CLEN_UNR non-temporal 16 B loads back to back, a scheduling fence
// keeps them ahead of the arithmetic, then CLEN_UNR stores.  Any other layout (a base off 16 B, a pitch or stride off
// the vector) takes the scalar form: same grid, same arithmetic, one element per load.  The four coefficients of a
// row are wave-uniform.  All stores are ordinary vector-memory stores.
#include "xk_common.h"
#include "xk_lane.h"

namespace xk {

constexpr int CLEN_UNR = 4;                        // 16 B vectors per lane and array: 16 loads in flight, no scratch

template <typename T, bool VEC>
__global__ __launch_bounds__(256) void cheb_clenshaw_kernel(
    const T* __restrict__ AY, const T* __restrict__ Y, const T* Yp, const T* __restrict__ X0, T* out,
    const double* __restrict__ coef, int p, int N, long ldA, long sA, long ldY, long sY, long ldP, long sP, long ldX,
    long sX, long ldO, long sO, int nchunk) {
  typedef typename Vec16<T>::type VT;
  constexpr int VN = Vec16<T>::n;
  constexpr int CH = 256 * VN * CLEN_UNR;          // elements of a chunk
  const int row = blockIdx.x / nchunk;
  const int chunk = blockIdx.x - row * nchunk;
  const int b = row / p;
  const int c = row - b * p;
  const T al = wave_uniform((T)coef[4 * (long)b + 0]);
  const T be = wave_uniform((T)coef[4 * (long)b + 1]);
  const T ga = wave_uniform((T)coef[4 * (long)b + 2]);
  const T de = wave_uniform((T)coef[4 * (long)b + 3]);
  const bool prev = ga != T(0);                    // (-0.0 compares equal to 0: not read either)
  const T* a_ = AY + (long)b * sA + (long)c * ldA;
  const T* y_ = Y + (long)b * sY + (long)c * ldY;
  const T* q_ = Yp + (long)b * sP + (long)c * ldP;
  const T* x_ = X0 + (long)b * sX + (long)c * ldX;
  T* o_ = out + (long)b * sO + (long)c * ldO;
  const long j0 = (long)chunk * CH;
  if (VEC) {
    VT av[CLEN_UNR], yv[CLEN_UNR], qv[CLEN_UNR], xv[CLEN_UNR];
    bool full[CLEN_UNR];
#pragma unroll
    for (int u = 0; u < CLEN_UNR; ++u) {
      const long j = j0 + ((long)u * 256 + threadIdx.x) * VN;
      full[u] = j + VN <= (long)N;
      if (full[u]) {
        av[u] = ld_stream(reinterpret_cast<const VT*>(a_ + j));
        yv[u] = ld_stream(reinterpret_cast<const VT*>(y_ + j));
        xv[u] = ld_stream(reinterpret_cast<const VT*>(x_ + j));
      }
    }
    if (prev) {
#pragma unroll
      for (int u = 0; u < CLEN_UNR; ++u) {
        const long j = j0 + ((long)u * 256 + threadIdx.x) * VN;
        if (full[u]) qv[u] = ld_stream(reinterpret_cast<const VT*>(q_ + j));
      }
    }
    __builtin_amdgcn_sched_barrier(0);             // all loads of the lane are in flight before the first use
#pragma unroll
    for (int u = 0; u < CLEN_UNR; ++u) {
      const long j = j0 + ((long)u * 256 + threadIdx.x) * VN;
      if (full[u]) {
        VT r;
        if (prev) {
#pragma unroll
          for (int e = 0; e < VN; ++e) r[e] = ((al * av[u][e] + be * yv[u][e]) + ga * qv[u][e]) + de * xv[u][e];
        } else {
#pragma unroll
          for (int e = 0; e < VN; ++e) r[e] = (al * av[u][e] + be * yv[u][e]) + de * xv[u][e];
        }
        *reinterpret_cast<VT*>(o_ + j) = r;
      } else if (j < (long)N) {                    // the vector that straddles N: element by element, pads untouched
        for (long n = j; n < (long)N; ++n) {
          T r = al * a_[n] + be * y_[n];
          if (prev) r += ga * q_[n];
          r += de * x_[n];
          o_[n] = r;
        }
      }
    }
  } else {
#pragma unroll 4
    for (int i = 0; i < VN * CLEN_UNR; ++i) {
      const long n = j0 + (long)i * 256 + threadIdx.x;
      if (n < (long)N) {
        T r = al * a_[n] + be * y_[n];
        if (prev) r += ga * q_[n];
        r += de * x_[n];
        o_[n] = r;
      }
    }
  }
}

// byte range [lo, hi) a (Bt, p, ld) panel of N-element rows touches (strides >= 0)
static inline void clen_range(const void* base, long ld, long sB, int Bt, int p, int N, size_t esz, uintptr_t& lo,
                              uintptr_t& hi) {
  lo = (uintptr_t)base;
  hi = lo + (size_t)((long)(Bt - 1) * sB + (long)(p - 1) * ld + N) * esz;
}

template <typename T>
static int cheb_clenshaw(const T* AY, long ldA, long sA, const T* Y, long ldY, long sY, const T* Yp, long ldP, long sP,
                         const T* X0, long ldX, long sX, T* out, long ldO, long sO, const double* coef, int Bt, int p,
                         int N, hipStream_t st) {
  constexpr int VN = Vec16<T>::n;
  if (Bt <= 0 || p <= 0 || N <= 0 || !AY || !Y || !Yp || !X0 || !out || !coef) return XK_ERR_ARG;
  if (ldA < N || ldY < N || ldP < N || ldX < N || ldO < N || sA < 0 || sY < 0 || sP < 0 || sX < 0 || sO < 0)
    return XK_ERR_ARG;
  // the rows of out must not overlap each other (several workgroups would write the same elements): the pitch covers
  // a row (checked above) and the batch stride a whole member
  if (Bt > 1 && sO < (long)(p - 1) * ldO + N) return XK_ERR_ARG;
  uintptr_t olo, ohi, lo, hi;
  clen_range(out, ldO, sO, Bt, p, N, sizeof(T), olo, ohi);
  clen_range(AY, ldA, sA, Bt, p, N, sizeof(T), lo, hi);
  if (olo < hi && lo < ohi) return XK_ERR_ARG;
  clen_range(Y, ldY, sY, Bt, p, N, sizeof(T), lo, hi);
  if (olo < hi && lo < ohi) return XK_ERR_ARG;
  clen_range(X0, ldX, sX, Bt, p, N, sizeof(T), lo, hi);
  if (olo < hi && lo < ohi) return XK_ERR_ARG;
  clen_range(Yp, ldP, sP, Bt, p, N, sizeof(T), lo, hi);
  const bool same = (const T*)out == Yp && ldO == ldP && sO == sP;
  if (!same && olo < hi && lo < ohi) return XK_ERR_ARG;
  const long nchunk = ((long)N + 256L * VN * CLEN_UNR - 1) / (256L * VN * CLEN_UNR);
  const long grid = (long)Bt * p * nchunk;
  if (grid > 0x7fffffffL) return XK_ERR_ARG;
  auto ok = [](const void* q, long ld, long s) { return !((uintptr_t)q & 15) && ld % VN == 0 && s % VN == 0; };
  const bool vec = ok(AY, ldA, sA) && ok(Y, ldY, sY) && ok(Yp, ldP, sP) && ok(X0, ldX, sX) && ok(out, ldO, sO);
  if (vec)
    hipLaunchKernelGGL((cheb_clenshaw_kernel<T, true>), dim3((unsigned)grid), dim3(256), 0, st, AY, Y, Yp, X0, out,
                       coef, p, N, ldA, sA, ldY, sY, ldP, sP, ldX, sX, ldO, sO, (int)nchunk);
  else
    hipLaunchKernelGGL((cheb_clenshaw_kernel<T, false>), dim3((unsigned)grid), dim3(256), 0, st, AY, Y, Yp, X0, out,
                       coef, p, N, ldA, sA, ldY, sY, ldP, sP, ldX, sX, ldO, sO, (int)nchunk);
  XK_LAUNCH_CHECK();
  return XK_OK;
}

}  // namespace xk

extern "C" {

// MUL = 1: real panels;  MUL = 2: interleaved complex ones (N, pitches and batch strides in complex elements)
#define XK_DEFINE_CLENSHAW(SUF, T, MUL)                                                                            \
  int xk_cheb_clenshaw_##SUF(const T* AY, long ldA, long sA, const T* Y, long ldY, long sY, const T* Yprev,        \
                             long ldP, long sP, const T* X0, long ldX, long sX, T* out, long ldO, long sO,         \
                             const double* coef, int Bt, int p, int N, void* stream) {                             \
    if (N <= 0 || N > 0x7fffffff / MUL) return XK_ERR_ARG;                                                         \
    return xk::cheb_clenshaw<T>(AY, ldA * MUL, sA * MUL, Y, ldY * MUL, sY * MUL, Yprev, ldP * MUL, sP * MUL, X0,   \
                                ldX * MUL, sX * MUL, out, ldO * MUL, sO * MUL, coef, Bt, p, N * MUL,               \
                                (hipStream_t)stream);                                                              \
  }

XK_DEFINE_CLENSHAW(f64, double, 1)
XK_DEFINE_CLENSHAW(f32, float, 1)
XK_DEFINE_CLENSHAW(c128, double, 2)
XK_DEFINE_CLENSHAW(c64, float, 2)

}  // extern "C"
