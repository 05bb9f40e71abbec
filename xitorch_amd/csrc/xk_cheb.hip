// xitorch_amd :: the three-term step of a Chebyshev filter (Zhou, Saad, Tiago, Chelikowsky, J. Comput. Phys. 219
// (2006) 172), the one pass over the block between two operator applies of Chebyshev-filtered subspace iteration.
//
// An extension (the reference has no filtered subspace iteration).  Panels are the (Bt, p, ld) arrays of _panel.py:
// Bt operators, p vectors each, every vector a contiguous run of N elements, ld >= N.  For every operator b, column c
// and n < N
//
//   out[b,c,n] = alpha[b] * AY[b,c,n] + beta[b] * Y[b,c,n] + gamma[b] * Yprev[b,c,n]
//
// with (alpha, beta, gamma) = coef[b, 0..2], a DEVICE array of doubles: the driver computes the coefficient table of a
// whole filter with a handful of torch ops and no step of the filter synchronises with the host.  The coefficients are
// real for all four dtypes, so the complex entry points run the real kernels on the interleaved (re, im) storage with
// N, ld and the batch stride doubled, as xk_minres_* do.
//
// Arithmetic: the f64 / c128 forms evaluate in double.  The f32 / c64 forms round each coefficient ONCE to float and
// evaluate in float (the storage precision).  The sum is taken left to right, (alpha*ay + beta*y) + gamma*yp; the
// compiler may contract products into FMAs, which only removes roundings.  When gamma[b] == 0.0 exactly (+0 or -0: the
// first step of a filter) Yprev[b] is NOT read and may hold NaN / Inf; alpha and beta get no such treatment.
//
// out may be Yprev itself (same pointer, pitch and batch stride: the ring of the driver overwrites its oldest panel;
// every lane reads the elements it writes before it writes them) or an array apart from it.  out must not share
// memory with AY or Y: the entry points compare the address ranges and return XK_ERR_ARG without launching anything;
// so does an out whose own rows overlap (a batch stride below (p - 1) * pitch + N with Bt > 1, a pitch below N).
// Only out[b, c, :N] is written: a vector that straddles N is finished element by element, pads are never touched.
//
// A pure stream, 4 Bt p N s bytes (3 Bt p N s on a first step).  Vector form (every base 16 B aligned, every pitch and
// batch stride a multiple of the 16 B vector — the rule of DESIGN.md section 3.0, always true of pad_len panels): a
// workgroup of 256 lanes owns one chunk of 4 x 256 vectors of one row, grid = Bt * p * chunks so a narrow block still
// fills the device; each lane issues its 8 (first step) or 12 non-temporal 16 B loads back to back, a scheduling fence
// keeps them ahead of the arithmetic, then 4 stores.  Any other layout takes the scalar form: same grid, same
// arithmetic, one element per load.  The three coefficients of a row are wave-uniform (readfirstlane).  All stores are
// ordinary vector-memory stores.
#include "xk_common.h"
#include "xk_lane.h"

namespace xk {

constexpr int CHEB_UNR = 4;                        // 16 B vectors per lane and array

template <typename T, bool VEC>
__global__ __launch_bounds__(256) void cheb_step_kernel(
    const T* __restrict__ AY, const T* __restrict__ Y, const T* Yp, T* out, const double* __restrict__ coef,
    int p, int N, long ldA, long sA, long ldY, long sY, long ldP, long sP, long ldO, long sO, int nchunk) {
  typedef typename Vec16<T>::type VT;
  constexpr int VN = Vec16<T>::n;
  constexpr int CH = 256 * VN * CHEB_UNR;          // elements of a chunk
  const int row = blockIdx.x / nchunk;
  const int chunk = blockIdx.x - row * nchunk;
  const int b = row / p;
  const int c = row - b * p;
  const T al = wave_uniform((T)coef[3 * (long)b + 0]);
  const T be = wave_uniform((T)coef[3 * (long)b + 1]);
  const T ga = wave_uniform((T)coef[3 * (long)b + 2]);
  const bool prev = ga != T(0);                    // (-0.0 compares equal to 0: not read either)
  const T* a_ = AY + (long)b * sA + (long)c * ldA;
  const T* y_ = Y + (long)b * sY + (long)c * ldY;
  const T* q_ = Yp + (long)b * sP + (long)c * ldP;
  T* o_ = out + (long)b * sO + (long)c * ldO;
  const long j0 = (long)chunk * CH;
  if (VEC) {
    VT av[CHEB_UNR], yv[CHEB_UNR], qv[CHEB_UNR];
    bool full[CHEB_UNR];
#pragma unroll
    for (int u = 0; u < CHEB_UNR; ++u) {
      const long j = j0 + ((long)u * 256 + threadIdx.x) * VN;
      full[u] = j + VN <= (long)N;
      if (full[u]) {
        av[u] = ld_stream(reinterpret_cast<const VT*>(a_ + j));
        yv[u] = ld_stream(reinterpret_cast<const VT*>(y_ + j));
      }
    }
    if (prev) {
#pragma unroll
      for (int u = 0; u < CHEB_UNR; ++u) {
        const long j = j0 + ((long)u * 256 + threadIdx.x) * VN;
        if (full[u]) qv[u] = ld_stream(reinterpret_cast<const VT*>(q_ + j));
      }
    }
    __builtin_amdgcn_sched_barrier(0);             // all loads of the lane are in flight before the first use
#pragma unroll
    for (int u = 0; u < CHEB_UNR; ++u) {
      const long j = j0 + ((long)u * 256 + threadIdx.x) * VN;
      if (full[u]) {
        VT r;
        if (prev) {
#pragma unroll
          for (int e = 0; e < VN; ++e) r[e] = (al * av[u][e] + be * yv[u][e]) + ga * qv[u][e];
        } else {
#pragma unroll
          for (int e = 0; e < VN; ++e) r[e] = al * av[u][e] + be * yv[u][e];
        }
        *reinterpret_cast<VT*>(o_ + j) = r;
      } else if (j < (long)N) {                    // the vector that straddles N: element by element, pads untouched
        for (long n = j; n < (long)N; ++n) {
          T r = al * a_[n] + be * y_[n];
          if (prev) r += ga * q_[n];
          o_[n] = r;
        }
      }
    }
  } else {
#pragma unroll 4
    for (int i = 0; i < VN * CHEB_UNR; ++i) {
      const long n = j0 + (long)i * 256 + threadIdx.x;
      if (n < (long)N) {
        T r = al * a_[n] + be * y_[n];
        if (prev) r += ga * q_[n];
        o_[n] = r;
      }
    }
  }
}

// byte range [lo, hi) a (Bt, p, ld) panel of N-element rows touches (strides >= 0)
static inline void cheb_range(const void* base, long ld, long sB, int Bt, int p, int N, size_t esz, uintptr_t& lo,
                              uintptr_t& hi) {
  lo = (uintptr_t)base;
  hi = lo + (size_t)((long)(Bt - 1) * sB + (long)(p - 1) * ld + N) * esz;
}

template <typename T>
static int cheb_step(const T* AY, long ldA, long sA, const T* Y, long ldY, long sY, const T* Yp, long ldP, long sP,
                     T* out, long ldO, long sO, const double* coef, int Bt, int p, int N, hipStream_t st) {
  constexpr int VN = Vec16<T>::n;
  if (Bt <= 0 || p <= 0 || N <= 0 || !AY || !Y || !Yp || !out || !coef) return XK_ERR_ARG;
  if (ldA < N || ldY < N || ldP < N || ldO < N || sA < 0 || sY < 0 || sP < 0 || sO < 0) return XK_ERR_ARG;
  // the rows of out must not overlap each other (several workgroups would write the same elements): the pitch covers
  // a row (checked above) and the batch stride a whole member
  if (Bt > 1 && sO < (long)(p - 1) * ldO + N) return XK_ERR_ARG;
  uintptr_t olo, ohi, lo, hi;
  cheb_range(out, ldO, sO, Bt, p, N, sizeof(T), olo, ohi);
  cheb_range(AY, ldA, sA, Bt, p, N, sizeof(T), lo, hi);
  if (olo < hi && lo < ohi) return XK_ERR_ARG;
  cheb_range(Y, ldY, sY, Bt, p, N, sizeof(T), lo, hi);
  if (olo < hi && lo < ohi) return XK_ERR_ARG;
  cheb_range(Yp, ldP, sP, Bt, p, N, sizeof(T), lo, hi);
  const bool same = (const T*)out == Yp && ldO == ldP && sO == sP;
  if (!same && olo < hi && lo < ohi) return XK_ERR_ARG;
  const long nchunk = ((long)N + 256L * VN * CHEB_UNR - 1) / (256L * VN * CHEB_UNR);
  const long grid = (long)Bt * p * nchunk;
  if (grid > 0x7fffffffL) return XK_ERR_ARG;
  auto ok = [](const void* q, long ld, long s) { return !((uintptr_t)q & 15) && ld % VN == 0 && s % VN == 0; };
  const bool vec = ok(AY, ldA, sA) && ok(Y, ldY, sY) && ok(Yp, ldP, sP) && ok(out, ldO, sO);
  if (vec)
    hipLaunchKernelGGL((cheb_step_kernel<T, true>), dim3((unsigned)grid), dim3(256), 0, st, AY, Y, Yp, out, coef, p, N,
                       ldA, sA, ldY, sY, ldP, sP, ldO, sO, (int)nchunk);
  else
    hipLaunchKernelGGL((cheb_step_kernel<T, false>), dim3((unsigned)grid), dim3(256), 0, st, AY, Y, Yp, out, coef, p,
                       N, ldA, sA, ldY, sY, ldP, sP, ldO, sO, (int)nchunk);
  XK_LAUNCH_CHECK();
  return XK_OK;
}

}  // namespace xk

extern "C" {

// MUL = 1: real panels;  MUL = 2: interleaved complex ones (N, pitches and batch strides in complex elements)
#define XK_DEFINE_CHEB(SUF, T, MUL)                                                                              \
  int xk_cheb_step_##SUF(const T* AY, long ldA, long sA, const T* Y, long ldY, long sY, const T* Yprev, long ldP, \
                         long sP, T* out, long ldO, long sO, const double* coef, int Bt, int p, int N,           \
                         void* stream) {                                                                         \
    if (N <= 0 || N > 0x7fffffff / MUL) return XK_ERR_ARG;                                                       \
    return xk::cheb_step<T>(AY, ldA * MUL, sA * MUL, Y, ldY * MUL, sY * MUL, Yprev, ldP * MUL, sP * MUL, out,    \
                            ldO * MUL, sO * MUL, coef, Bt, p, N * MUL, (hipStream_t)stream);                     \
  }

XK_DEFINE_CHEB(f64, double, 1)
XK_DEFINE_CHEB(f32, float, 1)
XK_DEFINE_CHEB(c128, double, 2)
XK_DEFINE_CHEB(c64, float, 2)

}  // extern "C"
