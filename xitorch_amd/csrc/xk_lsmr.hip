// xitorch_amd :: LSMR step kernels (Fong & Saunders, SIAM J. Sci. Comput. 33 (2011) 2950) for least squares with a
// rectangular operator A (m x n):  min |A x - b|^2 + damp^2 |x|^2.
//
// An extension (the reference has no lstsq).  Golub-Kahan bidiagonalisation of A started on b,
//     beta_{k+1} u_{k+1} = A v_k - alpha_k u_k,      alpha_{k+1} v_{k+1} = A^H u_{k+1} - beta_{k+1} v_k,
// carried on the UN-normalised vectors uh_k = beta_k u_k and vh_k = alpha_k v_k (the norm is folded into the consumer,
// as xk_minres.hip does: no scaling pass, and the host never reads a norm), two plane rotations per step (plus the
// damping rotation) and the three-vector update of the paper's Algorithm.  The layout is the one xk_kry_layout.h
// defines (shared with xk_krylov.hip and xk_minres.hip): every system (batch member x column) is one vector of a padded
// (S, ld) array, cut into nblk <= 64 blocks (block_range), reductions are two-stage in a fixed order (one partial per
// block, the consumers re-reduce the partials of their system in double: reduce_partials_d), loads and stores are
// 16 B vectors, 256 threads, no atomics: repeated runs give identical bits.
//
// Per-system scalar state, ALWAYS in double whatever the vector type, double-buffered: LS_NST doubles per system and
// slot, state[(slot * S + s) * LS_NST + i]; a launch of step k reads slot k & 1 and xk_lsmr_update writes slot
// (k + 1) & 1, so no block reads a scalar another block of the same launch is writing.
//
//   i = 0 alpha     alpha_k = |vh_k| (0: start, no vh yet: xk_lsmr_bidiag does not read y, xk_lsmr_update only
//                   sets up the recurrence: h = vh / alpha_1)
//       1 beta      beta_k = |uh_k|
//       2 alphabar, 3 zetabar, 4 rho, 5 rhobar, 6 cbar, 7 sbar, 8 zeta        the rotations of the Algorithm
//       9 betadd, 10 betad, 11 rhodold, 12 tautildeold, 13 thetatilde, 14 d   the |r| recurrence (section 5)
//      15 normA2 (sum of the squared bidiagonal entries), 16 maxrbar, 17 minrbar, 18 itn (steps of this recurrence)
//      19 flag      0 running, 1 S1 (|rbar| <= btol |b| + atol |A| |x|; also b = 0), 2 S2 (|Abar^H rbar| <= atol |A|
//                   |rbar|), 3 S3 (cond(Abar) >= conlim), 4 alpha_{k+1} = 0 (A^H u = 0: the least-squares solution is
//                   reached), 5 beta_{k+1} = 0 (A v - alpha u = 0: the system is consistent and solved)
//      20 normb, 21 normr, 22 normar = |zetabar|, 23 normA, 24 condA, 25 normx   the estimates of the step
//      26 alpha_1 = |A^H b| / |b| <= |A|_2
//
// normA, the |A| of the stopping rules, is the Frobenius norm of the bidiagonal (sqrt(normA2)) CAPPED by an estimate
// of |A|_2: in exact arithmetic the former never exceeds |A|_F, but once the Lanczos vectors lose orthogonality every
// ghost copy of a converged singular value adds to it and it grows without bound, relaxing S1 and S2 with it.  The
// cap is sqrt(maxrbar^2 - damp^2) (rhobar is a diagonal entry of a triangular factor of [B_k; damp I], so
// rhobar^2 <= |A|_2^2 + damp^2; ghosts do not inflate a 2-norm), at least alpha_1: normA <= |A|_F also in floating point.
//
// |x| is not estimated by a recurrence: xk_lsmr_update sums |x_{k+1}|^2 into block partials while it writes x, and the
// NEXT step's stopping test reads them, so S1 sees |x_k| for |x_{k+1}| (|x_k| grows monotonically: the test is the
// stricter one).
//
// All scalars are REAL even for a complex operator, so on interleaved (re, im) storage the vector arithmetic of a
// complex system of order N is that of a real one of order 2N: the complex entry points are the real kernels with
// N -> 2N.
//
//   xk_lsmr_init     beta_1 = sqrt(sum Pb), uh = b, state slot k & 1 (alpha = 0: start), beta_1 = 0 freezes (flag 1)
//   xk_lsmr_bidiag   y <- Op / nu_x - (nu_x / nu_y) y with nu_x = sqrt(sum Pin) (the norm of the vector Op was applied
//                    to, from the partials the previous half wrote) and nu_y from the state (half 0, the u half:
//                    beta; half 1, the v half: alpha, 0 = y is not read); Pout <- block partials of |y|^2;
//                    nu_x = 0: y is left alone and the partials are 0 (the following update freezes the system)
//   xk_lsmr_update   beta_{k+1}, alpha_{k+1} from the partials, the rotations, hbar <- h - c1 hbar, x <- x + c2 hbar,
//                    h <- vh / alpha_{k+1} - c3 h in one pass, the estimates and the stop code into slot (k + 1) & 1,
//                    run[s * 64] <- 1 (running) / 0 for xk_kry_status (nblk = 1, stop = 0.5)
#include "xk_common.h"
#include "xk_kry_layout.h"
#include "xk_lane.h"

namespace xk {

constexpr int LS_NST = 27;
enum { LS_ALPHA = 0, LS_BETA, LS_ALPHABAR, LS_ZETABAR, LS_RHO, LS_RHOBAR, LS_CBAR, LS_SBAR, LS_ZETA, LS_BETADD,
       LS_BETAD, LS_RHODOLD, LS_TAUTILDEOLD, LS_THETATILDE, LS_D, LS_NORMA2, LS_MAXRBAR, LS_MINRBAR, LS_ITN, LS_FLAG,
       LS_NORMB, LS_NORMR, LS_NORMAR, LS_NORMA, LS_CONDA, LS_NORMX, LS_ALPHA1 };

__device__ __forceinline__ double ls_div(double a, double b) { return b == 0.0 ? 0.0 : a / b; }

// block sum of the per-thread `acc`, written by thread 0 to dst (fixed order: wave butterflies, then four waves).
// block_partial of xk_kry_layout.h is the same sum; it forms the address of the partial in thread 0 alone, this one
// takes it formed by every thread, and with the other the compiler allocates the registers of both kernels below
// differently, so this form stays.
template <typename T>
__device__ __forceinline__ void ls_block_partial(T acc, T* sh4, T* dst) {
  acc = wave_sum(acc);
  if ((threadIdx.x & 63) == 0) sh4[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) *dst = (sh4[0] + sh4[1]) + (sh4[2] + sh4[3]);
}

// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void lsmr_init_kernel(
    const T* __restrict__ b, T* __restrict__ uh, const T* __restrict__ Pb, double* __restrict__ state,
    T* __restrict__ run, int S, int N, long ld, int nblk, int k) {
  __shared__ double sh;
  XK_KRY_PROLOGUE
  const double bb = reduce_partials_d(Pb, s, nblk, 1, &sh);
  const double beta = sqrt(bb);                                           // (a NaN stays a NaN)
  XK_KRY_LOOP { XK_KRY_ST(uh, XK_KRY_LDNT(b)); }
  if (blk == 0 && threadIdx.x == 0) {
    double* st = state + ((long)(k & 1) * S + s) * LS_NST;
#pragma unroll
    for (int i = 0; i < LS_NST; ++i) st[i] = 0.0;
    st[LS_BETA] = beta;
    st[LS_NORMB] = beta;
    st[LS_NORMR] = beta;
    st[LS_FLAG] = beta == 0.0 ? 1.0 : 0.0;
    run[(long)s * KRY_MAX_PART] = beta == 0.0 ? T(0) : T(1);
  }
}

// y <- Op / nu_x - (nu_x / nu_y) y; partials of |y|^2
template <typename T>
__global__ __launch_bounds__(256) void lsmr_bidiag_kernel(
    const T* __restrict__ Op, T* __restrict__ y, const T* __restrict__ Pin, T* __restrict__ Pout,
    const double* __restrict__ state, int half, int S, int N, long ld, int nblk, int nblk_in, int k) {
  __shared__ double sh;
  __shared__ T sh4[4];
  XK_KRY_PROLOGUE
  const double* st = state + ((long)(k & 1) * S + s) * LS_NST;
  if (st[LS_FLAG] != 0.0) return;                      // frozen system: nothing is written (block-uniform)
  const double nux = sqrt(reduce_partials_d(Pin, s, nblk_in, 1, &sh));
  const double nuy = half == 0 ? st[LS_BETA] : st[LS_ALPHA];
  T acc = T(0);
  if (nux == 0.0) {                                    // breakdown: y stays, |y|^2 = 0 tells the update
    if (threadIdx.x == 0) Pout[(long)s * KRY_MAX_PART + blk] = T(0);
    return;
  }
  const T c0 = wave_uniform((T)(1.0 / nux));
  if (nuy != 0.0) {
    const T c1 = wave_uniform((T)(nux / nuy));
    XK_KRY_LOOP {
      const VT ov = XK_KRY_LDNT(Op);
      VT yv = XK_KRY_LD(y);
#pragma unroll
      for (int q = 0; q < VN; ++q) yv[q] = ov[q] * c0 - c1 * yv[q];
#pragma unroll
      for (int q = 0; q < VN; ++q) acc += yv[q] * yv[q];
      XK_KRY_ST(y, yv);
    }
  } else {
    XK_KRY_LOOP {
      VT yv = XK_KRY_LDNT(Op);
#pragma unroll
      for (int q = 0; q < VN; ++q) yv[q] = yv[q] * c0;
#pragma unroll
      for (int q = 0; q < VN; ++q) acc += yv[q] * yv[q];
      XK_KRY_ST(y, yv);
    }
  }
  ls_block_partial(acc, sh4, Pout + (long)s * KRY_MAX_PART + blk);
}

// rotations + hbar, x, h in one pass + estimates + stop code
template <typename T>
__global__ __launch_bounds__(256) void lsmr_update_kernel(
    const T* __restrict__ vh, T* __restrict__ h, T* __restrict__ hbar, T* __restrict__ x,
    const T* __restrict__ Pu, const T* __restrict__ Pv, const T* __restrict__ Pxin, T* __restrict__ Pxout,
    double* __restrict__ state, T* __restrict__ run, int S, int N, long ld, int nblk, int nblk_u, int k,
    double damp, double atol, double btol, double conlim) {
  __shared__ double sh;
  __shared__ T sh4[4];
  XK_KRY_PROLOGUE
  const double* st = state + ((long)(k & 1) * S + s) * LS_NST;
  double* so = state + ((long)((k + 1) & 1) * S + s) * LS_NST;
  const bool writer = blk == 0 && threadIdx.x == 0;
  if (st[LS_FLAG] != 0.0) {                            // frozen: carry the state over, touch nothing else
    if (writer) {
#pragma unroll
      for (int i = 0; i < LS_NST; ++i) so[i] = st[i];
    }
    return;
  }
  const double alpha = sqrt(reduce_partials_d(Pv, s, nblk, 1, &sh));
  const double beta0 = st[LS_BETA];
  if (st[LS_ALPHA] == 0.0) {                           // start: alpha_1 = |A^H b| / beta_1, h = v_1; x, hbar stay
    const T ia = wave_uniform(alpha == 0.0 ? T(0) : (T)(1.0 / alpha));
    XK_KRY_LOOP {
      VT vv = XK_KRY_LDNT(vh);
#pragma unroll
      for (int q = 0; q < VN; ++q) vv[q] = vv[q] * ia;
      XK_KRY_ST(h, vv);
    }
    if (writer) {
#pragma unroll
      for (int i = 0; i < LS_NST; ++i) so[i] = 0.0;
      so[LS_ALPHA] = alpha;           so[LS_BETA] = beta0;       so[LS_ALPHABAR] = alpha;
      so[LS_ZETABAR] = alpha * beta0; so[LS_RHO] = 1.0;          so[LS_RHOBAR] = 1.0;
      so[LS_CBAR] = 1.0;              so[LS_BETADD] = beta0;     so[LS_RHODOLD] = 1.0;
      so[LS_NORMA2] = alpha * alpha;  so[LS_MINRBAR] = 1e100;    so[LS_FLAG] = alpha == 0.0 ? 4.0 : 0.0;
      so[LS_NORMB] = st[LS_NORMB];    so[LS_NORMR] = beta0;      so[LS_NORMAR] = alpha * beta0;
      so[LS_NORMA] = alpha;           so[LS_CONDA] = 1.0;        so[LS_ALPHA1] = alpha;
      run[(long)s * KRY_MAX_PART] = alpha == 0.0 ? T(0) : T(1);
    }
    return;
  }
  const double beta = sqrt(reduce_partials_d(Pu, s, nblk_u, 1, &sh));
  const double normx = sqrt(reduce_partials_d(Pxin, s, nblk, 1, &sh));
  // the damping rotation, then the two plane rotations of the Algorithm
  const double alphabar = st[LS_ALPHABAR], zetabar = st[LS_ZETABAR], rhoold = st[LS_RHO], rhobarold = st[LS_RHOBAR];
  const double cbar = st[LS_CBAR], sbar = st[LS_SBAR], zetaold = st[LS_ZETA];
  const double alphahat = sqrt(alphabar * alphabar + damp * damp);
  const double chat = alphahat == 0.0 ? 1.0 : alphabar / alphahat, shat = ls_div(damp, alphahat);
  const double rho = sqrt(alphahat * alphahat + beta * beta);
  const double c = rho == 0.0 ? 1.0 : alphahat / rho, sn = ls_div(beta, rho);
  const double thetanew = sn * alpha, alphabar_n = c * alpha;
  const double thetabar = sbar * rho, rhotemp = cbar * rho;
  const double rhobar = sqrt(rhotemp * rhotemp + thetanew * thetanew);
  const double cbar_n = rhobar == 0.0 ? 1.0 : rhotemp / rhobar, sbar_n = ls_div(thetanew, rhobar);
  const double zeta = cbar_n * zetabar, zetabar_n = -sbar_n * zetabar;
  const T c1 = wave_uniform((T)ls_div(thetabar * rho, rhoold * rhobarold));
  const T c2 = wave_uniform((T)ls_div(zeta, rho * rhobar));
  const T c3 = wave_uniform((T)ls_div(thetanew, rho));
  const T ia = wave_uniform(alpha == 0.0 ? T(0) : (T)(1.0 / alpha));
  T acc = T(0);
  XK_KRY_LOOP {
    const VT vv = XK_KRY_LDNT(vh);
    VT hv = XK_KRY_LD(h);
    VT hb = XK_KRY_LD(hbar);
    VT xv = XK_KRY_LD(x);
#pragma unroll
    for (int q = 0; q < VN; ++q) {
      hb[q] = hv[q] - c1 * hb[q];
      xv[q] = xv[q] + c2 * hb[q];
      hv[q] = vv[q] * ia - c3 * hv[q];
      acc += xv[q] * xv[q];
    }
    XK_KRY_ST(hbar, hb);
    XK_KRY_ST(x, xv);
    XK_KRY_ST(h, hv);
  }
  ls_block_partial(acc, sh4, Pxout + (long)s * KRY_MAX_PART + blk);
  if (writer) {
    // |rbar| (section 5 of the paper)
    const double betadd = st[LS_BETADD], betad = st[LS_BETAD], rhodold = st[LS_RHODOLD];
    const double tautildeold = st[LS_TAUTILDEOLD], thetatildeold = st[LS_THETATILDE];
    const double betaacute = chat * betadd, betacheck = -shat * betadd;
    const double betahat = c * betaacute, betadd_n = -sn * betaacute;
    const double rhotildeold = sqrt(rhodold * rhodold + thetabar * thetabar);
    const double ctildeold = rhotildeold == 0.0 ? 1.0 : rhodold / rhotildeold, stildeold = ls_div(thetabar, rhotildeold);
    const double thetatilde = stildeold * rhobar, rhodold_n = ctildeold * rhobar;
    const double betad_n = -stildeold * betad + ctildeold * betahat;
    const double tautildeold_n = ls_div(zetaold - thetatildeold * tautildeold, rhotildeold);
    const double taud = ls_div(zeta - thetatilde * tautildeold_n, rhodold_n);
    const double d_n = st[LS_D] + betacheck * betacheck;
    const double dt = betad_n - taud;
    const double normr = sqrt(d_n + dt * dt + betadd_n * betadd_n);
    // |A|_F of the bidiagonal, cond(Abar)
    const double na2 = st[LS_NORMA2] + beta * beta;
    const double itn = st[LS_ITN];
    const double maxrbar = fmax(st[LS_MAXRBAR], rhobarold);
    const double two2 = maxrbar * maxrbar - damp * damp;
    const double normA = fmin(sqrt(na2), fmax(sqrt(fmax(two2, 0.0)), st[LS_ALPHA1]));
    const double minrbar = itn >= 1.0 ? fmin(st[LS_MINRBAR], rhobarold) : st[LS_MINRBAR];
    const double condA = ls_div(fmax(maxrbar, rhotemp), fmin(minrbar, rhotemp));
    const double normar = fabs(zetabar_n);
    const double normb = st[LS_NORMB];
    double code = 0.0;
    if (condA >= conlim) code = 3.0;
    if (normar <= atol * normA * normr) code = 2.0;
    if (normr <= btol * normb + atol * normA * normx) code = 1.0;
    if (alpha == 0.0) code = 4.0;
    if (beta == 0.0) code = 5.0;
    so[LS_ALPHA] = alpha;          so[LS_BETA] = beta;            so[LS_ALPHABAR] = alphabar_n;
    so[LS_ZETABAR] = zetabar_n;    so[LS_RHO] = rho;              so[LS_RHOBAR] = rhobar;
    so[LS_CBAR] = cbar_n;          so[LS_SBAR] = sbar_n;          so[LS_ZETA] = zeta;
    so[LS_BETADD] = betadd_n;      so[LS_BETAD] = betad_n;        so[LS_RHODOLD] = rhodold_n;
    so[LS_TAUTILDEOLD] = tautildeold_n; so[LS_THETATILDE] = thetatilde; so[LS_D] = d_n;
    so[LS_NORMA2] = na2 + alpha * alpha; so[LS_MAXRBAR] = maxrbar; so[LS_MINRBAR] = minrbar;
    so[LS_ITN] = itn + 1.0;        so[LS_FLAG] = code;            so[LS_NORMB] = normb;
    so[LS_NORMR] = normr;          so[LS_NORMAR] = normar;        so[LS_NORMA] = normA;
    so[LS_CONDA] = condA;          so[LS_NORMX] = normx;          so[LS_ALPHA1] = st[LS_ALPHA1];
    run[(long)s * KRY_MAX_PART] = code == 0.0 ? T(1) : T(0);
  }
}

// host-side argument checks shared by the entry points: nothing is launched unless they pass
static int ls_check(int S, long N, long ld, int nblk, int k, int elem, int vn) {
  if (S < 0 || N <= 0 || k < 0 || nblk < 1 || nblk > KRY_MAX_PART) return XK_ERR_ARG;
  const long npad = (N + vn - 1) / vn * vn;
  if (ld < npad) return XK_ERR_ARG;
  if ((ld * elem) % 16 != 0) return XK_ERR_UNSUPPORTED;
  return XK_OK;
}
static bool ls_misaligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

}  // namespace xk

extern "C" {

int xk_lsmr_state_len(void) { return xk::LS_NST; }

#define XK_LS_CHECK                                                                                            \
  {                                                                                                            \
    const int rc__ = xk::ls_check(S, (long)N * MUL, ld * MUL, nblk, k, (int)sizeof(T_), 16 / (int)sizeof(T_)); \
    if (rc__ != XK_OK) return rc__;                                                                            \
  }

// MUL = 1: real systems;  MUL = 2: interleaved complex ones (N, ld in complex elements)
#define XK_DEFINE_LSMR(SUF, T, MUL_)                                                                           \
  int xk_lsmr_init_##SUF(const T* b, T* uh, const T* Pb, double* state, T* run, int S, int N, long ld,         \
                         int nblk, int k, void* stream) {                                                      \
    typedef T T_;                                                                                              \
    constexpr int MUL = MUL_;                                                                                  \
    XK_LS_CHECK                                                                                                \
    if (!b || !uh || !Pb || !state || !run) return XK_ERR_ARG;                                                 \
    if (xk::ls_misaligned(b) || xk::ls_misaligned(uh)) return XK_ERR_UNSUPPORTED;                              \
    if (S == 0) return XK_OK;                                                                                  \
    hipLaunchKernelGGL((xk::lsmr_init_kernel<T>), XK_KRY_GRID(S, nblk), b, uh, Pb, state, run, S, N * MUL,     \
                       ld * MUL, nblk, k);                                                                     \
    XK_LAUNCH_CHECK();                                                                                         \
    return XK_OK;                                                                                              \
  }                                                                                                            \
  int xk_lsmr_bidiag_##SUF(const T* Op, T* y, const T* Pin, T* Pout, const double* state, int half, int S,     \
                           int N, long ld, int nblk, int nblk_in, int k, void* stream) {                       \
    typedef T T_;                                                                                              \
    constexpr int MUL = MUL_;                                                                                  \
    XK_LS_CHECK                                                                                                \
    if (nblk_in < 1 || nblk_in > xk::KRY_MAX_PART || half < 0 || half > 1) return XK_ERR_ARG;                  \
    if (!Op || !y || !Pin || !Pout || !state || Pin == Pout || Op == y) return XK_ERR_ARG;                     \
    if (xk::ls_misaligned(Op) || xk::ls_misaligned(y)) return XK_ERR_UNSUPPORTED;                              \
    if (S == 0) return XK_OK;                                                                                  \
    hipLaunchKernelGGL((xk::lsmr_bidiag_kernel<T>), XK_KRY_GRID(S, nblk), Op, y, Pin, Pout, state, half, S,    \
                       N * MUL, ld * MUL, nblk, nblk_in, k);                                                   \
    XK_LAUNCH_CHECK();                                                                                         \
    return XK_OK;                                                                                              \
  }                                                                                                            \
  int xk_lsmr_update_##SUF(const T* vh, T* h, T* hbar, T* x, const T* Pu, const T* Pv, const T* Pxin,          \
                           T* Pxout, double* state, T* run, int S, int N, long ld, int nblk, int nblk_u,       \
                           int k, double damp, double atol, double btol, double conlim, void* stream) {        \
    typedef T T_;                                                                                              \
    constexpr int MUL = MUL_;                                                                                  \
    XK_LS_CHECK                                                                                                \
    if (nblk_u < 1 || nblk_u > xk::KRY_MAX_PART || !(damp >= 0.0)) return XK_ERR_ARG;                          \
    if (!vh || !h || !hbar || !x || !Pu || !Pv || !Pxin || !Pxout || !state || !run) return XK_ERR_ARG;        \
    if (Pxin == Pxout || vh == h || vh == hbar || vh == x || h == hbar || h == x || hbar == x)                 \
      return XK_ERR_ARG;                                                                                       \
    if (xk::ls_misaligned(vh) || xk::ls_misaligned(h) || xk::ls_misaligned(hbar) || xk::ls_misaligned(x))      \
      return XK_ERR_UNSUPPORTED;                                                                               \
    if (S == 0) return XK_OK;                                                                                  \
    hipLaunchKernelGGL((xk::lsmr_update_kernel<T>), XK_KRY_GRID(S, nblk), vh, h, hbar, x, Pu, Pv, Pxin, Pxout, \
                       state, run, S, N * MUL, ld * MUL, nblk, nblk_u, k, damp, atol, btol, conlim);           \
    XK_LAUNCH_CHECK();                                                                                         \
    return XK_OK;                                                                                              \
  }

XK_DEFINE_LSMR(f64, double, 1)
XK_DEFINE_LSMR(f32, float, 1)
XK_DEFINE_LSMR(c128, double, 2)
XK_DEFINE_LSMR(c64, float, 2)

}  // extern "C"
