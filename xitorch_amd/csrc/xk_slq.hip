// xitorch_amd :: stochastic Lanczos quadrature: the quadratic forms z^H f(A) z of a Hermitian operator by Gauss
// quadrature on the Lanczos tridiagonal (Golub & Meurant, "Matrices, Moments and Quadrature"; Ubaru, Chen & Saad,
// SIAM J. Matrix Anal. Appl. 38 (2017) 1075 for the trace estimator built on them).
//
// An extension (the reference has no logdet / trace of a matrix function).  Lanczos started on z runs on the
// UN-normalised vectors r2 = beta_k v_k (the norm is folded into the consumer, as xk_minres.hip and xk_lsmr.hip do: no
// scaling pass, and the host never reads a norm); only the three vectors r1, r2 and W = A r2 exist, whatever the step
// count: no basis is stored and nothing is reorthogonalised (the quadrature of the finite-precision Lanczos matrix
// stays accurate).  The layout is the one xk_kry_layout.h defines: every system (batch member x probe) is one vector
// of a padded (S, ld) array, cut into nblk <= 64 blocks (block_range), reductions are two-stage in a fixed order (one
// partial per block, the consumers re-reduce the partials of their system in double: reduce_partials_d), loads and
// stores are 16 B vectors, 256 threads, no atomics: repeated runs give identical bits.
//
// Per-system scalar state, ALWAYS in double whatever the vector type, double-buffered: SQ_NST doubles per system and
// slot, state[(slot * S + s) * SQ_NST + i]; a launch of step k reads slot k & 1 and writes slot (k + 1) & 1, so no
// block reads a scalar another block of the same launch is writing (the discipline of xk_minres.hip).  For the same
// reason the partials of |y|^2 ping-pong: a step reads Pin (those of the step before) and writes Pout.
//
//   i = 0 beta     the norm of the Lanczos vector the last step ran on (after xk_slq_init: beta_1 = |z|)
//       1 oldb     the norm before that (0: after the first step and before it; the r1 term is then absent)
//       2 flag     0 running, 1 frozen by a breakdown (an invariant subspace has been found: the quadrature over the
//                  m x m matrix is exact), 2 frozen: z = 0 (m = 0, every quadratic form is 0)
//       3 m        steps recorded: alpha_1 .. alpha_m in Tal[s, 0 .. m), beta_1 .. beta_m in Tbe[s, 0 .. m); the Jacobi
//                  matrix is diag(Tal[s, :m]) with the off-diagonal Tbe[s, 1 .. m) (Tbe[s, 0] = |z| is not part of it)
//       4 tnorm    running maximum of the absolute row sums |alpha_j| + beta_j + beta_{j+1} of that matrix
//       5 rowp     |alpha_m| + beta_m (beta_m only when it is part of the matrix): the last row, short of its beta_{m+1}
//       6 znorm2   |z|^2
//       7 alpha    alpha_m (a record; nothing reads it back)
//
// Breakdown.  A step first forms the norm beta of the vector it is to run on, from the partials the step before wrote.
// With tnorm updated by the row this beta completes, the system is frozen when beta <= SQ_BREAK * eps_T * tnorm, eps_T
// the machine epsilon of the vector type and SQ_BREAK = 64: the rounding errors of y = W / beta - ... (three terms, a
// few roundings each, every term of size at most |A| |v|) leave at most about 12 eps_T |A| of a vector that is zero in
// exact arithmetic, and |A| <= tnorm up to the Lanczos error, so 64 eps_T tnorm catches every such remainder with a
// factor 5 to spare, while a beta that small against |A| (8e-6 in single, 1.4e-14 in double precision) changes the
// quadrature by its square.  The test is `<=`, so an exactly zero beta is frozen here and never reaches a division.
// A frozen system returns block-uniformly before any store to its vectors, partials or T rows; only its state is
// carried from slot to slot.
//
// All Lanczos scalars of a Hermitian operator are REAL, so on interleaved (re, im) storage the vector arithmetic of a
// complex system of order N is that of a real one of order 2N: the complex entry points are the real kernels with
// N -> 2N; they differ only in where the inner products come from: xk_kry_dots_c* writes (re, im) pairs of the
// conjugated products, of which the real part is taken (pstride = 2).
//
//   xk_slq_init   beta_1 = sqrt(<z, z>) from the xk_kry_dots partials Pb, r2 = z, the start state in slot k & 1
//   xk_slq_step   alpha = sum Pa / beta^2 (Pa: the xk_kry_dots partials of <r2, W>, W = A r2),
//                 y = W / beta - (alpha / beta) r2 - (beta / oldb) r1 written over r1 (the caller swaps r1 and r2),
//                 Pout <- block partials of |y|^2, alpha and beta into Tal[s, m], Tbe[s, m], slot (k + 1) & 1
//   xk_slq_quad   one lane per system: eigenvalues theta and squared first eigenvector components tau^2 of the m x m
//                 Jacobi matrix by implicit QL with the first row of the rotations carried along (Golub & Welsch,
//                 Math. Comp. 23 (1969) 221), then |z|^2 sum tau_k^2 f(theta_k).  d, e and the row live in LDS as
//                 [step][lane], so the lanes of a wave hit different banks; 3 * 8 * nsteps bytes per lane, and the
//                 workgroup is 64, 32 or 16 lanes so that it never takes more than 48 KB (nsteps = 128: 16 lanes).
#include "xk_common.h"
#include "xk_kry_layout.h"
#include "xk_lane.h"

namespace xk {

constexpr int SQ_NST = 8;
constexpr int SQ_MAX_STEPS = 128;
constexpr double SQ_BREAK = 64.0;
constexpr int SQ_QL_SWEEPS = 60;              // implicit QL iterations allowed per eigenvalue
enum { SQ_BETA = 0, SQ_OLDB, SQ_FLAG, SQ_M, SQ_TNORM, SQ_ROWP, SQ_ZNORM2, SQ_ALPHA };
enum { SQ_FN_LOG = 0, SQ_FN_INV, SQ_FN_SQRT, SQ_FN_INVSQRT, SQ_FN_EXP, SQ_FN_IDENTITY, SQ_FN_COUNT };

template <typename T> struct SqEps;
template <> struct SqEps<double> { static constexpr double v = 2.220446049250313e-16; };
template <> struct SqEps<float> { static constexpr double v = 1.1920928955078125e-07; };

// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void slq_init_kernel(
    const T* __restrict__ z, T* __restrict__ r2, const T* __restrict__ Pb, double* __restrict__ state, int S, int N,
    long ld, int nblk, int pstride, int k) {
  __shared__ double sh;
  XK_KRY_PROLOGUE
  const double bb = reduce_partials_d(Pb, s, nblk, pstride, &sh);
  XK_KRY_LOOP { XK_KRY_ST(r2, XK_KRY_LDNT(z)); }
  if (blk == 0 && threadIdx.x == 0) {
    double* st = state + ((long)(k & 1) * S + s) * SQ_NST;
    const double beta = sqrt(bb);                                         // (a NaN stays a NaN)
    st[SQ_BETA] = beta;   st[SQ_OLDB] = 0.0;  st[SQ_FLAG] = bb == 0.0 ? 2.0 : 0.0;  st[SQ_M] = 0.0;
    st[SQ_TNORM] = 0.0;   st[SQ_ROWP] = 0.0;  st[SQ_ZNORM2] = bb;                   st[SQ_ALPHA] = 0.0;
  }
}

// y = W / beta - (alpha / beta) r2 - (beta / oldb) r1, written over r1; partials of |y|^2; alpha, beta into T
template <typename T>
__global__ __launch_bounds__(256) void slq_step_kernel(
    const T* __restrict__ W, const T* __restrict__ r2, T* __restrict__ r1, const T* __restrict__ Pa,
    const T* __restrict__ Pin, T* __restrict__ Pout, double* __restrict__ state, double* __restrict__ Tal,
    double* __restrict__ Tbe, int S, int N, long ld, int nblk, int pstride, int nsteps, int k) {
  __shared__ double sh;
  __shared__ T sh4[4];
  XK_KRY_PROLOGUE
  const double* st = state + ((long)(k & 1) * S + s) * SQ_NST;
  double* so = state + ((long)((k + 1) & 1) * S + s) * SQ_NST;
  const bool writer = blk == 0 && threadIdx.x == 0;
  const double md = st[SQ_M];
  if (st[SQ_FLAG] != 0.0 || !(md >= 0.0 && md < (double)nsteps)) {   // frozen (or T is full): carry the state over
    if (writer) {
#pragma unroll
      for (int i = 0; i < SQ_NST; ++i) so[i] = st[i];
    }
    return;
  }
  const int m = (int)md;
  const bool first = m == 0;
  const double oldb = first ? 0.0 : st[SQ_BETA];
  const double beta = first ? st[SQ_BETA] : sqrt(reduce_partials_d(Pin, s, nblk, 1, &sh));
  const double tnorm = fmax(st[SQ_TNORM], st[SQ_ROWP] + (first ? 0.0 : beta));
  if (!first && beta <= SQ_BREAK * SqEps<T>::v * tnorm) {           // breakdown: freeze, nothing else is written
    if (writer) {
#pragma unroll
      for (int i = 0; i < SQ_NST; ++i) so[i] = st[i];
      so[SQ_FLAG] = 1.0;
      so[SQ_TNORM] = tnorm;
    }
    return;
  }
  const double alpha = reduce_partials_d(Pa, s, nblk, pstride, &sh) / (beta * beta);
  const T c0 = wave_uniform((T)(1.0 / beta));
  const T c2 = wave_uniform((T)(alpha / beta));
  T acc = T(0);
  if (!first) {
    const T c1 = wave_uniform((T)(beta / oldb));
    XK_KRY_LOOP {
      const VT wv = XK_KRY_LDNT(W);
      const VT r2v = XK_KRY_LD(r2);
      VT y = XK_KRY_LD(r1);
#pragma unroll
      for (int q = 0; q < VN; ++q) y[q] = (wv[q] * c0 - c2 * r2v[q]) - c1 * y[q];
#pragma unroll
      for (int q = 0; q < VN; ++q) acc += y[q] * y[q];
      XK_KRY_ST(r1, y);
    }
  } else {
    XK_KRY_LOOP {
      const VT wv = XK_KRY_LDNT(W);
      const VT r2v = XK_KRY_LD(r2);
      VT y;
#pragma unroll
      for (int q = 0; q < VN; ++q) y[q] = wv[q] * c0 - c2 * r2v[q];
#pragma unroll
      for (int q = 0; q < VN; ++q) acc += y[q] * y[q];
      XK_KRY_ST(r1, y);
    }
  }
  block_partial(wave_sum(acc), Pout, s, blk, sh4);
  if (writer) {
    Tal[(long)s * nsteps + m] = alpha;
    Tbe[(long)s * nsteps + m] = beta;
    so[SQ_BETA] = beta;     so[SQ_OLDB] = oldb;   so[SQ_FLAG] = 0.0;                 so[SQ_M] = md + 1.0;
    so[SQ_TNORM] = tnorm;   so[SQ_ROWP] = fabs(alpha) + (first ? 0.0 : beta);
    so[SQ_ZNORM2] = st[SQ_ZNORM2];                so[SQ_ALPHA] = alpha;
  }
}

// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ double sq_fn(int fn, double param, double x) {
  switch (fn) {
    case SQ_FN_LOG: return log(x);
    case SQ_FN_INV: return 1.0 / x;
    case SQ_FN_SQRT: return sqrt(x);
    case SQ_FN_INVSQRT: return 1.0 / sqrt(x);
    case SQ_FN_EXP: return exp(param * x);
    default: return x;
  }
}

// one lane per system; d, e, w: LDS arrays [nsteps][L] (L = blockDim.x lanes)
__global__ __launch_bounds__(64) void slq_quad_kernel(const double* __restrict__ Tal, const double* __restrict__ Tbe,
                                const double* __restrict__ state, double* __restrict__ theta,
                                double* __restrict__ weight, double* __restrict__ out, int* __restrict__ flag, int S,
                                int nsteps, int k, int fn, double param) {
  extern __shared__ double sq_lds[];
  const int L = blockDim.x, lane = threadIdx.x;
  const int s = blockIdx.x * L + lane;
  if (s >= S) return;
  double* d = sq_lds + lane;
  double* e = d + (long)nsteps * L;
  double* w = e + (long)nsteps * L;
#define D_(i) d[(i) * L]
#define E_(i) e[(i) * L]
#define W_(i) w[(i) * L]
  const double* st = state + ((long)(k & 1) * S + s) * SQ_NST;
  const double md = st[SQ_M];
  const int m = md >= 0.0 ? (md < (double)nsteps ? (int)md : nsteps) : 0;      // (a NaN count: 0)
  const double zz = st[SQ_ZNORM2];
  for (int i = 0; i < m; ++i) {
    D_(i) = Tal[(long)s * nsteps + i];
    E_(i) = i + 1 < m ? Tbe[(long)s * nsteps + i + 1] : 0.0;
    W_(i) = i == 0 ? 1.0 : 0.0;
  }
  int bad = 0;
  constexpr double EPS = 2.220446049250313e-16;
  for (int l = 0; l < m; ++l) {
    int iter = 0;
    while (true) {
      int mm = l;
      for (; mm < m - 1; ++mm) {
        const double dd = fabs(D_(mm)) + fabs(D_(mm + 1));
        if (!(fabs(E_(mm)) > EPS * dd)) break;
      }
      if (mm == l) break;
      if (iter++ == SQ_QL_SWEEPS) { bad = 2; break; }
      const double el = E_(l);
      double g = (D_(l + 1) - D_(l)) / (2.0 * el);
      double r = hypot(g, 1.0);
      g = D_(mm) - D_(l) + el / (g + copysign(r, g));
      double sn = 1.0, cs = 1.0, p = 0.0;
      int i = mm - 1;
      for (; i >= l; --i) {
        double f = sn * E_(i);
        const double b = cs * E_(i);
        r = hypot(f, g);
        E_(i + 1) = r;
        if (r == 0.0) {                                  // recover from underflow
          D_(i + 1) -= p;
          E_(mm) = 0.0;
          break;
        }
        sn = f / r;
        cs = g / r;
        g = D_(i + 1) - p;
        r = (D_(i) - g) * sn + 2.0 * cs * b;
        p = sn * r;
        D_(i + 1) = g + p;
        g = cs * r - b;
        f = W_(i + 1);                                   // the first row of the accumulated rotations
        W_(i + 1) = sn * W_(i) + cs * f;
        W_(i) = cs * W_(i) - sn * f;
      }
      if (r == 0.0 && i >= l) continue;
      D_(l) -= p;
      E_(l) = g;
      E_(mm) = 0.0;
    }
    if (bad) break;
  }
  const bool needpos = fn <= SQ_FN_INVSQRT;
  double sum = 0.0;
  for (int i = 0; i < nsteps; ++i) {
    double th = 0.0, wt = 0.0;
    if (i < m) {
      th = D_(i);
      wt = W_(i) * W_(i);
      if (needpos && !(th > 0.0)) bad |= 1;
      sum += wt * sq_fn(fn, param, th);
    }
    theta[(long)s * nsteps + i] = th;
    weight[(long)s * nsteps + i] = wt;
  }
#undef D_
#undef E_
#undef W_
  out[s] = bad ? (double)NAN : zz * sum;
  flag[s] = bad;
}

// lanes per workgroup of xk_slq_quad: the largest of 64, 32, 16 whose three [nsteps][L] double arrays fit 48 KB
static int sq_quad_lanes(int nsteps) {
  int L = 64;
  while (L > 16 && (long)3 * 8 * nsteps * L > 48 * 1024) L >>= 1;
  return L;
}

// host-side argument checks shared by the entry points: nothing is launched unless they pass
static int sq_check(int S, long N, long ld, int nblk, int k, int elem, int vn) {
  if (S < 0 || N <= 0 || k < 0 || nblk < 1 || nblk > KRY_MAX_PART) return XK_ERR_ARG;
  const long npad = (N + vn - 1) / vn * vn;
  if (npad > 2147483647L) return XK_ERR_ARG;          // the kernels index a system with ints (complex: 2 N elements)
  if (ld < npad) return XK_ERR_ARG;
  if ((ld * elem) % 16 != 0) return XK_ERR_UNSUPPORTED;
  return XK_OK;
}
static bool sq_misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

}  // namespace xk

extern "C" {

int xk_slq_state_len(void) { return xk::SQ_NST; }

#define XK_SQ_CHECK                                                                                            \
  {                                                                                                            \
    const int rc__ = xk::sq_check(S, (long)N * MUL, ld * MUL, nblk, k, (int)sizeof(T_), 16 / (int)sizeof(T_)); \
    if (rc__ != XK_OK) return rc__;                                                                            \
  }

// MUL = 1: real systems;  MUL = 2: interleaved complex ones (N, ld in complex elements; Pb, Pa hold (re, im) pairs)
#define XK_DEFINE_SLQ(SUF, T, MUL_)                                                                            \
  int xk_slq_init_##SUF(const T* z, T* r2, const T* Pb, double* state, int S, int N, long ld, int nblk, int k, \
                        void* stream) {                                                                        \
    typedef T T_;                                                                                              \
    constexpr int MUL = MUL_;                                                                                  \
    XK_SQ_CHECK                                                                                                \
    if (!z || !r2 || !Pb || !state || z == r2) return XK_ERR_ARG;                                              \
    if (xk::sq_misaligned(z) || xk::sq_misaligned(r2)) return XK_ERR_UNSUPPORTED;                              \
    if (S == 0) return XK_OK;                                                                                  \
    hipLaunchKernelGGL((xk::slq_init_kernel<T>), XK_KRY_GRID(S, nblk), z, r2, Pb, state, S, N * MUL, ld * MUL, \
                       nblk, MUL, k);                                                                          \
    XK_LAUNCH_CHECK();                                                                                         \
    return XK_OK;                                                                                              \
  }                                                                                                            \
  int xk_slq_step_##SUF(const T* W, const T* r2, T* r1, const T* Pa, const T* Pin, T* Pout, double* state,     \
                        double* Tal, double* Tbe, int S, int N, long ld, int nblk, int nsteps, int k,          \
                        void* stream) {                                                                        \
    typedef T T_;                                                                                              \
    constexpr int MUL = MUL_;                                                                                  \
    XK_SQ_CHECK                                                                                                \
    if (nsteps < 1 || nsteps > xk::SQ_MAX_STEPS) return XK_ERR_ARG;                                            \
    if (!W || !r2 || !r1 || !Pa || !Pin || !Pout || !state || !Tal || !Tbe) return XK_ERR_ARG;                 \
    if (W == r2 || W == r1 || r2 == r1 || Pin == Pout || Pa == Pout || Tal == Tbe) return XK_ERR_ARG;          \
    if (xk::sq_misaligned(W) || xk::sq_misaligned(r2) || xk::sq_misaligned(r1)) return XK_ERR_UNSUPPORTED;     \
    if (S == 0) return XK_OK;                                                                                  \
    hipLaunchKernelGGL((xk::slq_step_kernel<T>), XK_KRY_GRID(S, nblk), W, r2, r1, Pa, Pin, Pout, state, Tal,   \
                       Tbe, S, N * MUL, ld * MUL, nblk, MUL, nsteps, k);                                       \
    XK_LAUNCH_CHECK();                                                                                         \
    return XK_OK;                                                                                              \
  }

XK_DEFINE_SLQ(f64, double, 1)
XK_DEFINE_SLQ(f32, float, 1)
XK_DEFINE_SLQ(c128, double, 2)
XK_DEFINE_SLQ(c64, float, 2)

int xk_slq_quad(const double* Tal, const double* Tbe, const double* state, double* theta, double* weight,
                double* out, int* flag, int S, int nsteps, int k, int fn, double param, void* stream) {
  if (S < 0 || k < 0 || nsteps < 1 || nsteps > xk::SQ_MAX_STEPS || fn < 0 || fn >= xk::SQ_FN_COUNT)
    return XK_ERR_ARG;
  if (!Tal || !Tbe || !state || !theta || !weight || !out || !flag) return XK_ERR_ARG;
  if (theta == weight || Tal == theta || Tal == weight || Tbe == theta || Tbe == weight || Tal == Tbe)
    return XK_ERR_ARG;
  if (S == 0) return XK_OK;
  const int L = xk::sq_quad_lanes(nsteps);
  const size_t lds = (size_t)3 * 8 * nsteps * L;
  hipLaunchKernelGGL(xk::slq_quad_kernel, dim3((unsigned)((S + L - 1) / L)), dim3(L), lds, (hipStream_t)stream, Tal,
                     Tbe, state, theta, weight, out, flag, S, nsteps, k, fn, param);
  XK_LAUNCH_CHECK();
  return XK_OK;
}

}  // extern "C"
