// xitorch_amd :: f(A) B for a Hermitian operator by two-pass Lanczos (Lanczos-FA without a stored basis; Druskin &
// Knizhnerman, USSR Comput. Math. Math. Phys. 29 (1989) 112; Musco, Musco & Sidford, SODA 2018 for its behaviour in
// finite precision; the two-pass form: Frommer & Simoncini, "Matrix functions", 2008, section 4).
//
// An extension (the reference has no matrix function of an operator).  Pass 1 is the run of xk_slq.hip on a start
// vector b: the Lanczos scalars alpha_k, beta_k of the UN-normalised recurrence in Tal, Tbe (S, nsteps), the step count
// m and |b|^2 in the state.  The small problem: with T = Q Theta Q^T the Jacobi matrix of a system,
//   f(A) b ~ V_m f(T) e_1 |b| = sum_k c_k v_k,      c = |b| Q f(Theta) Q^T e_1,
// and r2_k = beta_k v_k is the vector pass 1 ran on in step k, so X = sum_k (c_k / beta_k) r2_k.  Pass 2 replays the
// recurrence from the stored scalars and accumulates X; it has no inner products, no partial sums and no state of its
// own.  Nothing is reorthogonalised, so the replayed vectors must be pass 1's BIT FOR BIT: xk_fnm_step forms c0, c1, c2
// from the same doubles by the same expressions and casts as slq_step_kernel and evaluates y by the same expression.
//
//   xk_fnm_eig     one wave per system: eigenvalues theta and the WHOLE eigenvector matrix of the m x m Jacobi matrix by
//                  the implicit QL of slq_quad_kernel with the rotation product accumulated.  The rotation scalars are
//                  the same in every lane (d and e live in LDS, every lane computes and stores the same numbers); lane
//                  i owns rows i and i + 64 of Q.  Q is kept in the caller's global array Qt (S, nsteps, nsteps),
//                  COLUMN-major ([col][row]: Qt[s, k, j] = component j of eigenvector k), so a rotation of columns i,
//                  i + 1 is two unit-stride accesses of the wave: 128 KB per system at nsteps = 128 do not fit the
//                  64 KB of LDS a workgroup gets by default, the array is an output anyway (xk_fnm_coeff reads it) and
//                  at these sizes it stays in L2.  A sweep walks the columns downwards and carries the upper column of
//                  every rotation in registers: one load and one store per rotation and row, and no lane ever reads an
//                  entry another lane wrote.
//   xk_fnm_coeff   C[s, j] = |b_s| sum_k Q[j, k] f_k Q[0, k], k ascending; one thread per row j.  f_k is a named
//                  function of theta_k (the codes of xk_slq_quad) or, fn = -1, the caller's fvals; tail[s] =
//                  |C[s, m-4 : m]| / |C[s, : m]|, summed by one thread in index order.
//   xk_fnm_step    step k of pass 2 on the XK_KRY_* layout: X += (C[s, k] / beta_k) r2, then the Lanczos vector of step
//                  k + 1 over r1 (the caller swaps r1 and r2).  Six array passes (read W, r2, r1, X; write r1, X), 16 B
//                  accesses, W non-temporal; no reductions, no atomics, no LDS.
#include "xk_common.h"
#include "xk_kry_layout.h"
#include "xk_lane.h"

namespace xk {

// The state layout, the function codes, the step and QL sweep caps and fnm_fn below restate SQ_NST, SQ_MAX_STEPS,
// SQ_QL_SWEEPS, the SQ_* enums and sq_fn of xk_slq.hip, which keeps them to itself.  tests/test_fnm_abi.py compares the
// two source files entry by entry (and the state length with xk_slq_state_len()); moving them into one header is left
// to a change that may touch xk_slq.hip.
constexpr int FN_NST = 8;
constexpr int FN_MAX_STEPS = 128;
constexpr int FN_QL_SWEEPS = 60;
enum { FN_ST_FLAG = 2, FN_ST_M = 3, FN_ST_ZNORM2 = 6 };
enum { FN_LOG = 0, FN_INV, FN_SQRT, FN_INVSQRT, FN_EXP, FN_IDENTITY, FN_COUNT };

__device__ __forceinline__ int fnm_count(const double* st, int nsteps) {
  const double md = st[FN_ST_M];
  return md >= 0.0 ? (md < (double)nsteps ? (int)md : nsteps) : 0;            // (a NaN count: 0)
}

// ---------------------------------------------------------------------------------------------
// grid S, one wave each.  d, e: the tridiagonal, the same numbers written by every lane (wave-uniform control flow).
// THE WORKGROUP MUST STAY ONE WAVE (64 threads: __launch_bounds__(64) here, dim3(64) in xk_fnm_eig): the 64 lanes store
// identical values into the same LDS words with no barrier, which is sound only because they do so in the lockstep of
// one wave; a second wave would read d and e in the middle of the first one's sweep.
__global__ __launch_bounds__(64) void fnm_eig_kernel(const double* __restrict__ Tal, const double* __restrict__ Tbe,
                                                     const double* __restrict__ state, double* __restrict__ theta,
                                                     double* __restrict__ Qt, int* __restrict__ flag, int S, int nsteps,
                                                     int k) {
  __shared__ double d[FN_MAX_STEPS + 1], e[FN_MAX_STEPS + 1];
  const int s = blockIdx.x, lane = threadIdx.x;
  const int m = fnm_count(state + ((long)(k & 1) * S + s) * FN_NST, nsteps);
  double* Q = Qt + (long)s * nsteps * nsteps;
  const int ra = lane, rb = lane + 64;                    // the rows of this lane
  const bool oka = ra < m, okb = rb < m;
  for (int c = 0; c < nsteps; ++c) {                      // Q = I on the leading m x m block, 0 elsewhere
    if (ra < nsteps) Q[(long)c * nsteps + ra] = (c == ra && oka) ? 1.0 : 0.0;
    if (rb < nsteps) Q[(long)c * nsteps + rb] = (c == rb && okb) ? 1.0 : 0.0;
  }
  for (int i = 0; i < m; ++i) {
    d[i] = Tal[(long)s * nsteps + i];
    e[i] = i + 1 < m ? Tbe[(long)s * nsteps + i + 1] : 0.0;
  }
  int bad = 0;
  constexpr double EPS = 2.220446049250313e-16;
  for (int l = 0; l < m; ++l) {
    int iter = 0;
    while (true) {
      int mm = l;
      for (; mm < m - 1; ++mm) {
        const double dd = fabs(d[mm]) + fabs(d[mm + 1]);
        if (!(fabs(e[mm]) > EPS * dd)) break;
      }
      if (mm == l) break;
      if (iter++ == FN_QL_SWEEPS) { bad = 2; break; }
      const double el = e[l];
      double g = (d[l + 1] - d[l]) / (2.0 * el);
      double r = hypot(g, 1.0);
      g = d[mm] - d[l] + el / (g + copysign(r, g));
      double sn = 1.0, cs = 1.0, p = 0.0;
      double qa = oka ? Q[(long)mm * nsteps + ra] : 0.0;  // the carried column: i + 1 of the rotation to come
      double qb = okb ? Q[(long)mm * nsteps + rb] : 0.0;
      int i = mm - 1;
      for (; i >= l; --i) {
        double f = sn * e[i];
        const double b = cs * e[i];
        r = hypot(f, g);
        e[i + 1] = r;
        if (r == 0.0) {                                   // recover from underflow
          d[i + 1] -= p;
          e[mm] = 0.0;
          break;
        }
        sn = f / r;
        cs = g / r;
        g = d[i + 1] - p;
        r = (d[i] - g) * sn + 2.0 * cs * b;
        p = sn * r;
        d[i + 1] = g + p;
        g = cs * r - b;
        double* qi = Q + (long)i * nsteps;                // columns i, i + 1 of the accumulated rotations
        if (oka) {
          const double lo = qi[ra];
          qi[nsteps + ra] = sn * lo + cs * qa;
          qa = cs * lo - sn * qa;
        }
        if (okb) {
          const double lo = qi[rb];
          qi[nsteps + rb] = sn * lo + cs * qb;
          qb = cs * lo - sn * qb;
        }
      }
      if (oka) Q[(long)(i + 1) * nsteps + ra] = qa;       // the carried column comes to rest
      if (okb) Q[(long)(i + 1) * nsteps + rb] = qb;
      if (r == 0.0 && i >= l) continue;
      d[l] -= p;
      e[l] = g;
      e[mm] = 0.0;
    }
    if (bad) break;
  }
  for (int i = lane; i < nsteps; i += 64) theta[(long)s * nsteps + i] = i < m ? d[i] : 0.0;
  if (lane == 0) flag[s] = bad;
}

__device__ __forceinline__ double fnm_fn(int fn, double param, double x) {
  switch (fn) {
    case FN_LOG: return log(x);
    case FN_INV: return 1.0 / x;
    case FN_SQRT: return sqrt(x);
    case FN_INVSQRT: return 1.0 / sqrt(x);
    case FN_EXP: return exp(param * x);
    default: return x;
  }
}

// grid S, 128 threads: thread j owns row j of Q.  CP = 1: C (S, nsteps); CP = 2: (re, im) pairs
template <int CP>
__global__ __launch_bounds__(128) void fnm_coeff_kernel(const double* __restrict__ Qt, const double* __restrict__ theta,
                                                        const double* __restrict__ state,
                                                        const double* __restrict__ fvals, double* __restrict__ C,
                                                        double* __restrict__ tail, int* __restrict__ flag, int S,
                                                        int nsteps, int k, int fn, double param) {
  __shared__ double sq[FN_MAX_STEPS];
  const int s = blockIdx.x, j = threadIdx.x;
  const double* st = state + ((long)(k & 1) * S + s) * FN_NST;
  const int m = fnm_count(st, nsteps);
  const double bnorm = sqrt(st[FN_ST_ZNORM2]);
  const double* Q = Qt + (long)s * nsteps * nsteps;
  const double* th = theta + (long)s * nsteps;
  const bool needpos = fn >= 0 && fn <= FN_INVSQRT;
  int bad = flag[s] & 2;                                  // (what xk_fnm_eig left)
  double cr = 0.0, ci = 0.0;
  for (int kk = 0; kk < m; ++kk) {                        // every thread sees every node: `bad` is block-uniform
    const double x = th[kk];
    double fr, fi = 0.0;
    if (fn < 0) {
      fr = fvals[((long)s * nsteps + kk) * CP];
      if (CP == 2) fi = fvals[((long)s * nsteps + kk) * CP + 1];
    } else {
      if (needpos && !(x > 0.0)) bad |= 1;
      fr = fnm_fn(fn, param, x);
    }
    if (j < m) {
      const double w = Q[(long)kk * nsteps + j] * Q[(long)kk * nsteps];
      cr += w * fr;
      if (CP == 2) ci += w * fi;
    }
  }
  cr *= bnorm;
  ci *= bnorm;
  if (bad && j < m) cr = ci = (double)NAN;
  if (j < nsteps) {
    C[((long)s * nsteps + j) * CP] = j < m ? cr : 0.0;
    if (CP == 2) C[((long)s * nsteps + j) * CP + 1] = j < m ? ci : 0.0;
  }
  sq[j] = j < m ? cr * cr + ci * ci : 0.0;
  __syncthreads();
  if (j == 0) {
    double all = 0.0, last4 = 0.0;
    for (int i = 0; i < m; ++i) {
      all += sq[i];
      if (i >= m - 4) last4 += sq[i];
    }
    tail[s] = m > 4 ? sqrt(last4 / all) : 0.0;            // (C = 0 or NaN: NaN, as the coefficients themselves)
    flag[s] = bad;
  }
}

// ---------------------------------------------------------------------------------------------
// X += (cr + i ci) a on one 16 B vector; complex entries are (re, im) pairs of the real vector
template <typename T, bool CPLX, typename VT, int VN>
__device__ __forceinline__ void fnm_axpy(VT& x, const VT& a, T cr, T ci) {
  if constexpr (!CPLX) {
#pragma unroll
    for (int q = 0; q < VN; ++q) x[q] += cr * a[q];
  } else {
#pragma unroll
    for (int q = 0; q < VN; q += 2) {
      x[q] = (x[q] + cr * a[q]) - ci * a[q + 1];
      x[q + 1] = (x[q + 1] + cr * a[q + 1]) + ci * a[q];
    }
  }
}

template <typename T, bool CPLX>
__global__ __launch_bounds__(256) void fnm_step_kernel(
    const T* __restrict__ W, const T* __restrict__ r2, T* __restrict__ r1, T* __restrict__ X,
    const double* __restrict__ C, const double* __restrict__ Tal, const double* __restrict__ Tbe,
    const double* __restrict__ state, int S, int N, long ld, int nblk, int nsteps, int k, int kstate, int last) {
  XK_KRY_PROLOGUE
  const double* st = state + ((long)(kstate & 1) * S + s) * FN_NST;
  const double md = st[FN_ST_M];
  if (st[FN_ST_FLAG] == 2.0 || !(md > (double)k)) return;         // b = 0, or past the system's last step: nothing
  const long tk = (long)s * nsteps + k;
  const double beta = Tbe[tk], alpha = Tal[tk];
  constexpr int CP = CPLX ? 2 : 1;
  const T xr = wave_uniform((T)(C[tk * CP] / beta));
  const T xi = CPLX ? wave_uniform((T)(C[tk * CP + 1] / beta)) : T(0);
  if (last || !(md > (double)(k + 1))) {                          // the system's last vector: X only
    XK_KRY_LOOP {
      const VT r2v = XK_KRY_LD(r2);
      VT xv = XK_KRY_LD(X);
      fnm_axpy<T, CPLX, VT, VN>(xv, r2v, xr, xi);
      XK_KRY_ST(X, xv);
    }
    return;
  }
  // (as slq_step_kernel forms them)
  const T c0 = wave_uniform((T)(1.0 / beta));
  const T c2 = wave_uniform((T)(alpha / beta));
  if (k > 0) {
    const double oldb = Tbe[tk - 1];
    const T c1 = wave_uniform((T)(beta / oldb));
    XK_KRY_LOOP {
      const VT wv = XK_KRY_LDNT(W);
      const VT r2v = XK_KRY_LD(r2);
      VT y = XK_KRY_LD(r1);
      VT xv = XK_KRY_LD(X);
#pragma unroll
      for (int q = 0; q < VN; ++q) y[q] = (wv[q] * c0 - c2 * r2v[q]) - c1 * y[q];
      fnm_axpy<T, CPLX, VT, VN>(xv, r2v, xr, xi);
      XK_KRY_ST(r1, y);
      XK_KRY_ST(X, xv);
    }
  } else {
    XK_KRY_LOOP {
      const VT wv = XK_KRY_LDNT(W);
      const VT r2v = XK_KRY_LD(r2);
      VT xv = XK_KRY_LD(X);
      VT y;
#pragma unroll
      for (int q = 0; q < VN; ++q) y[q] = wv[q] * c0 - c2 * r2v[q];
      fnm_axpy<T, CPLX, VT, VN>(xv, r2v, xr, xi);
      XK_KRY_ST(r1, y);
      XK_KRY_ST(X, xv);
    }
  }
}

// host-side argument checks (those of xk_slq.hip): nothing is launched unless they pass
static int fnm_check(int S, long N, long ld, int nblk, int k, int elem, int vn) {
  if (S < 0 || N <= 0 || k < 0 || nblk < 1 || nblk > KRY_MAX_PART) return XK_ERR_ARG;
  const long npad = (N + vn - 1) / vn * vn;
  if (npad > 2147483647L) return XK_ERR_ARG;          // the kernels index a system with ints (complex: 2 N elements)
  if (ld < npad) return XK_ERR_ARG;
  if ((ld * elem) % 16 != 0) return XK_ERR_UNSUPPORTED;
  return XK_OK;
}
static bool fnm_misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

}  // namespace xk

extern "C" {

// MUL = 1: real systems;  MUL = 2: interleaved complex ones (N, ld in complex elements; C holds (re, im) pairs)
#define XK_DEFINE_FNM(SUF, T, MUL)                                                                             \
  int xk_fnm_step_##SUF(const T* W, const T* r2, T* r1, T* X, const double* C, const double* Tal,              \
                        const double* Tbe, const double* state, int S, int N, long ld, int nblk, int nsteps,   \
                        int k, int kstate, int last, void* stream) {                                           \
    const int rc = xk::fnm_check(S, (long)N * MUL, ld * MUL, nblk, k, (int)sizeof(T), 16 / (int)sizeof(T));    \
    if (rc != XK_OK) return rc;                                                                                \
    if (nsteps < 1 || nsteps > xk::FN_MAX_STEPS || k >= nsteps || kstate < 0) return XK_ERR_ARG;               \
    if (xk_slq_state_len() != xk::FN_NST) return XK_ERR_UNSUPPORTED; /* the state is xk_slq.hip's */           \
    if (!W) last = 1;                                                                                          \
    if (!r2 || !X || !C || !Tal || !Tbe || !state || (!last && !r1)) return XK_ERR_ARG;                        \
    if (r2 == X || (const T*)r1 == r2 || r1 == X || (W && (W == r2 || W == r1 || W == X)) || Tal == Tbe)        \
      return XK_ERR_ARG;                                                                                       \
    if (xk::fnm_misaligned(W) || xk::fnm_misaligned(r2) || xk::fnm_misaligned(r1) || xk::fnm_misaligned(X))    \
      return XK_ERR_UNSUPPORTED;                                                                               \
    if (S == 0) return XK_OK;                                                                                  \
    hipLaunchKernelGGL((xk::fnm_step_kernel<T, MUL == 2>), XK_KRY_GRID(S, nblk), W, r2, r1, X, C, Tal, Tbe,    \
                       state, S, N * MUL, ld * MUL, nblk, nsteps, k, kstate, last ? 1 : 0);                    \
    XK_LAUNCH_CHECK();                                                                                         \
    return XK_OK;                                                                                              \
  }

XK_DEFINE_FNM(f64, double, 1)
XK_DEFINE_FNM(f32, float, 1)
XK_DEFINE_FNM(c128, double, 2)
XK_DEFINE_FNM(c64, float, 2)

int xk_fnm_eig(const double* Tal, const double* Tbe, const double* state, double* theta, double* Qt, int* flag, int S,
               int nsteps, int k, void* stream) {
  if (S < 0 || k < 0 || nsteps < 1 || nsteps > xk::FN_MAX_STEPS) return XK_ERR_ARG;
  if (xk_slq_state_len() != xk::FN_NST) return XK_ERR_UNSUPPORTED;          // the state is xk_slq.hip's
  if (!Tal || !Tbe || !state || !theta || !Qt || !flag) return XK_ERR_ARG;
  if (Tal == Tbe || theta == Tal || theta == Tbe || Qt == Tal || Qt == Tbe || Qt == theta) return XK_ERR_ARG;
  if (S == 0) return XK_OK;
  hipLaunchKernelGGL(xk::fnm_eig_kernel, dim3((unsigned)S), dim3(64), 0, (hipStream_t)stream, Tal, Tbe, state, theta,
                     Qt, flag, S, nsteps, k);
  XK_LAUNCH_CHECK();
  return XK_OK;
}

int xk_fnm_coeff(const double* Qt, const double* theta, const double* state, const double* fvals, double* C,
                 double* tail, int* flag, int S, int nsteps, int k, int fn, double param, int cplx, void* stream) {
  if (S < 0 || k < 0 || nsteps < 1 || nsteps > xk::FN_MAX_STEPS || fn < -1 || fn >= xk::FN_COUNT) return XK_ERR_ARG;
  if (xk_slq_state_len() != xk::FN_NST) return XK_ERR_UNSUPPORTED;          // the state is xk_slq.hip's
  if (!Qt || !theta || !state || !C || !tail || !flag || (fn < 0 && !fvals)) return XK_ERR_ARG;
  if (C == Qt || C == theta || C == fvals || C == tail || tail == theta || tail == Qt) return XK_ERR_ARG;
  if (S == 0) return XK_OK;
  if (cplx)
    hipLaunchKernelGGL(xk::fnm_coeff_kernel<2>, dim3((unsigned)S), dim3(128), 0, (hipStream_t)stream, Qt, theta, state,
                       fvals, C, tail, flag, S, nsteps, k, fn, param);
  else
    hipLaunchKernelGGL(xk::fnm_coeff_kernel<1>, dim3((unsigned)S), dim3(128), 0, (hipStream_t)stream, Qt, theta, state,
                       fvals, C, tail, flag, S, nsteps, k, fn, param);
  XK_LAUNCH_CHECK();
  return XK_OK;
}

}  // extern "C"
