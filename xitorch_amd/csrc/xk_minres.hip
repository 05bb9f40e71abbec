// xitorch_amd :: MINRES step kernels (Paige & Saunders 1975) for Hermitian, possibly indefinite or singular systems.
//
// An extension (the reference has no MINRES): Lanczos tridiagonalisation of the (preconditioned) operator, one Givens
// rotation per step to keep the tridiagonal's QR factors, and the three-term recurrence of the search directions
// w_k = (v_k - eps_k w_{k-2} - delta_k w_{k-1}) / gamma_k that follows from  W R = V.  The layout is the one
// xk_kry_layout.h defines (shared with xk_krylov.hip and xk_lsmr.hip): every system (batch member x column) is one
// length-N vector of a padded (S, ld) array, each system is cut into nblk <= 64 blocks (block_range), reductions are
// two-stage in a fixed order (one partial per block, the consumers re-reduce the partials of their system in double:
// reduce_partials_d), loads and stores are 16 B vectors.
//
// Per-system scalar state, ALWAYS in double whatever the vector type, double-buffered: MR_NST doubles per system and
// slot, state[(slot * S + s) * MR_NST + i]; a launch of iteration k reads slot k & 1 and (xk_minres_update only)
// writes slot (k + 1) & 1, so no block reads a scalar another block of the same launch is writing.
//
//   i = 0 beta     beta_k: norm of the un-normalised Lanczos vector r2 (sqrt <r2, P r2> with a preconditioner)
//       1 oldb     beta_{k-1} (0: first step, the r1 term is absent and r1 is not read)
//       2 cs, 3 sn the last Givens rotation (start: -1, 0)
//       4 dbar     the rotated, not yet eliminated sub-diagonal entry;  5 epsln: the entry two above the diagonal
//       6 phibar   the recurrence residual norm |b - A x_k|
//       7 flag     0 running, 1 frozen by beta = 0 (exact convergence), 2 frozen: <r2, P r2> < 0 (the preconditioner
//                  is not positive definite), 3 frozen: gamma = 0 (the Krylov space holds no further descent)
//       8 alpha, 9 gamma, 10 delta, 11 phi   of the step that wrote the slot (records; nothing reads them back)
//
// All Lanczos and rotation scalars of a Hermitian operator are REAL, so on interleaved (re, im) storage the vector
// arithmetic of a complex system of order N is that of a real one of order 2N; the complex entry points are the real
// kernels on the interleaved storage and differ only in where the inner products come from: xk_kry_dots_c* writes
// (re, im) pairs of the conjugated products, of which the real part is taken (pstride = 2).
//
//   xk_minres_init     beta_1 = sqrt(<b, y0>), v = y0 / beta_1, state slot k & 1, phibar^2 for xk_kry_status
//   xk_minres_lanczos  y = Av - (alpha/beta) r2 - (beta/oldb) r1, written over r1 (the caller swaps r1 and r2);
//                      block partials of |y|^2
//   xk_minres_update   beta_new from the partials, the new rotation, w <- (v - epsln w1 - delta w2) / gamma written over
//                      w1 (the caller rotates the ring), x += phi w, v <- y / beta_new, state slot (k + 1) & 1,
//                      phibar^2 where xk_kry_status reads |r|^2
#include "xk_common.h"
#include "xk_kry_layout.h"

namespace xk {

constexpr int MR_NST = 12;
enum { MR_BETA = 0, MR_OLDB, MR_CS, MR_SN, MR_DBAR, MR_EPSLN, MR_PHIBAR, MR_FLAG, MR_ALPHA, MR_GAMMA, MR_DELTA, MR_PHI };

// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void minres_init_kernel(
    const T* __restrict__ y0, T* __restrict__ v, const T* __restrict__ Pb, double* __restrict__ state,
    T* __restrict__ phi2, int S, int N, long ld, int nblk, int pstride, int k) {
  __shared__ double sh;
  XK_KRY_PROLOGUE
  const double bb = reduce_partials_d(Pb, s, nblk, pstride, &sh);
  const double beta = bb > 0.0 ? sqrt(bb) : (bb < 0.0 ? 0.0 : bb);      // (a NaN stays a NaN)
  const double flag = bb < 0.0 ? 2.0 : (bb == 0.0 ? 1.0 : 0.0);
  const T sc = flag == 0.0 ? (T)(1.0 / beta) : T(0);
  XK_KRY_LOOP {
    VT yv = XK_KRY_LD(y0);
#pragma unroll
    for (int q = 0; q < VN; ++q) yv[q] = flag == 0.0 ? yv[q] * sc : T(0);
    XK_KRY_ST(v, yv);
  }
  if (blk == 0 && threadIdx.x == 0) {
    double* st = state + ((long)(k & 1) * S + s) * MR_NST;
    st[MR_BETA] = beta;  st[MR_OLDB] = 0.0;  st[MR_CS] = -1.0;  st[MR_SN] = 0.0;
    st[MR_DBAR] = 0.0;   st[MR_EPSLN] = 0.0; st[MR_PHIBAR] = beta; st[MR_FLAG] = flag;
    st[MR_ALPHA] = 0.0;  st[MR_GAMMA] = 0.0; st[MR_DELTA] = 0.0;  st[MR_PHI] = 0.0;
    phi2[(long)s * KRY_MAX_PART] = flag == 2.0 ? (T)INFINITY : (T)(beta * beta);
  }
}

// y = Av - (alpha/beta) r2 - (beta/oldb) r1, written over r1; partials of |y|^2 (Pbeta may be NULL)
template <typename T>
__global__ __launch_bounds__(256) void minres_lanczos_kernel(
    const T* __restrict__ Av, const T* __restrict__ r2, T* __restrict__ r1, const T* __restrict__ Palpha,
    const double* __restrict__ state, T* __restrict__ Pbeta, int S, int N, long ld, int nblk, int pstride, int k) {
  __shared__ double sh;
  __shared__ T sh4[4];
  XK_KRY_PROLOGUE
  const double* st = state + ((long)(k & 1) * S + s) * MR_NST;
  if (st[MR_FLAG] != 0.0) return;                      // frozen system: nothing is written (block-uniform)
  const double alpha = reduce_partials_d(Palpha, s, nblk, pstride, &sh);
  const double beta = st[MR_BETA], oldb = st[MR_OLDB];
  const T c2 = (T)(alpha / beta);
  const bool has1 = oldb != 0.0;
  const T c1 = has1 ? (T)(beta / oldb) : T(0);
  T acc = T(0);
  XK_KRY_LOOP {
    const VT av = XK_KRY_LD(Av);
    const VT r2v = XK_KRY_LD(r2);
    VT y;
    if (has1) {
      const VT r1v = XK_KRY_LD(r1);
#pragma unroll
      for (int q = 0; q < VN; ++q) y[q] = (av[q] - c2 * r2v[q]) - c1 * r1v[q];
    } else {
#pragma unroll
      for (int q = 0; q < VN; ++q) y[q] = av[q] - c2 * r2v[q];
    }
#pragma unroll
    for (int q = 0; q < VN; ++q) acc += y[q] * y[q];
    XK_KRY_ST(r1, y);
  }
  if (Pbeta != nullptr) block_partial(wave_sum(acc), Pbeta, s, blk, sh4);
}

// rotation + direction ring + solution + next Lanczos vector; y = r2 (no preconditioner) or P r2
template <typename T>
__global__ __launch_bounds__(256) void minres_update_kernel(
    T* __restrict__ v, const T* __restrict__ y, T* __restrict__ w1, const T* __restrict__ w2, T* __restrict__ x,
    const T* __restrict__ Palpha, const T* __restrict__ Pbeta, double* __restrict__ state, T* __restrict__ phi2,
    int S, int N, long ld, int nblk, int pstride_a, int pstride_b, int k) {
  __shared__ double sh;
  XK_KRY_PROLOGUE
  const double* st = state + ((long)(k & 1) * S + s) * MR_NST;
  double* so = state + ((long)((k + 1) & 1) * S + s) * MR_NST;
  const bool writer = blk == 0 && threadIdx.x == 0;
  if (st[MR_FLAG] != 0.0) {                            // frozen: carry the state over, touch nothing else
    if (writer) {
#pragma unroll
      for (int i = 0; i < MR_NST; ++i) so[i] = st[i];
    }
    return;
  }
  const double alpha = reduce_partials_d(Palpha, s, nblk, pstride_a, &sh);
  const double bb = reduce_partials_d(Pbeta, s, nblk, pstride_b, &sh);
  const double beta = st[MR_BETA], cs = st[MR_CS], sn = st[MR_SN], dbar = st[MR_DBAR], phibar = st[MR_PHIBAR];
  const double oldeps = st[MR_EPSLN];
  if (bb < 0.0) {                                      // <r2, P r2> < 0: not a positive definite preconditioner
    if (writer) {
#pragma unroll
      for (int i = 0; i < MR_NST; ++i) so[i] = st[i];
      so[MR_FLAG] = 2.0;
      phi2[(long)s * KRY_MAX_PART] = (T)INFINITY;
    }
    return;
  }
  const double bnew = sqrt(bb);
  const double delta = cs * dbar + sn * alpha;
  const double gbar = sn * dbar - cs * alpha;
  const double gamma = sqrt(gbar * gbar + bnew * bnew);
  if (gamma == 0.0) {                                  // no descent left in the Krylov space: keep x, freeze
    if (writer) {
#pragma unroll
      for (int i = 0; i < MR_NST; ++i) so[i] = st[i];
      so[MR_FLAG] = 3.0;
    }
    return;
  }
  const double csn = gbar / gamma, snn = bnew / gamma;
  const double phi = csn * phibar, phibar_n = snn * phibar;
  const bool done = bnew == 0.0;                       // exact convergence: no division by a replaced zero
  const T te = (T)oldeps, td = (T)delta, tg = (T)(1.0 / gamma), tp = (T)phi;
  const T tb = done ? T(0) : (T)(1.0 / bnew);
  XK_KRY_LOOP {
    VT vv = XK_KRY_LD(v);
    const VT w1v = XK_KRY_LD(w1);
    const VT w2v = XK_KRY_LD(w2);
    VT xv = XK_KRY_LD(x);
    const VT yv = XK_KRY_LD(y);
    VT w;
#pragma unroll
    for (int q = 0; q < VN; ++q) {
      w[q] = ((vv[q] - te * w1v[q]) - td * w2v[q]) * tg;
      xv[q] += tp * w[q];
      vv[q] = done ? T(0) : yv[q] * tb;
    }
    XK_KRY_ST(w1, w);
    XK_KRY_ST(x, xv);
    XK_KRY_ST(v, vv);
  }
  if (writer) {
    so[MR_BETA] = bnew;       so[MR_OLDB] = beta;        so[MR_CS] = csn;       so[MR_SN] = snn;
    so[MR_DBAR] = -cs * bnew; so[MR_EPSLN] = sn * bnew;  so[MR_PHIBAR] = phibar_n;
    so[MR_FLAG] = done ? 1.0 : 0.0;
    so[MR_ALPHA] = alpha;     so[MR_GAMMA] = gamma;      so[MR_DELTA] = delta;  so[MR_PHI] = phi;
    phi2[(long)s * KRY_MAX_PART] = (T)(phibar_n * phibar_n);
  }
}

}  // namespace xk

extern "C" {

int xk_minres_state_len(void) { return xk::MR_NST; }

#define XK_MR_CHECK                                                                       \
  if (S < 0 || N < 0 || k < 0 || nblk < 1 || nblk > xk::KRY_MAX_PART) return XK_ERR_ARG;  \
  if (S == 0 || N == 0) return XK_OK;

// MUL = 1, PS = 1: real systems;  MUL = 2, PS = 2: interleaved complex ones (N, ld in complex elements)
#define XK_DEFINE_MINRES(SUF, T, MUL, PS)                                                                   \
  int xk_minres_init_##SUF(const T* y0, T* v, const T* Pb, double* state, T* phi2, int S, int N, long ld,   \
                           int nblk, int k, void* stream) {                                                 \
    XK_MR_CHECK                                                                                             \
    hipLaunchKernelGGL((xk::minres_init_kernel<T>), XK_KRY_GRID(S, nblk), y0, v, Pb, state, phi2, S,        \
                       N * MUL, ld * MUL, nblk, PS, k);                                                     \
    XK_LAUNCH_CHECK();                                                                                      \
    return XK_OK;                                                                                           \
  }                                                                                                         \
  int xk_minres_lanczos_##SUF(const T* Av, const T* r2, T* r1, const T* Palpha, const double* state,        \
                              T* Pbeta, int S, int N, long ld, int nblk, int k, void* stream) {             \
    XK_MR_CHECK                                                                                             \
    hipLaunchKernelGGL((xk::minres_lanczos_kernel<T>), XK_KRY_GRID(S, nblk), Av, r2, r1, Palpha, state,     \
                       Pbeta, S, N * MUL, ld * MUL, nblk, PS, k);                                           \
    XK_LAUNCH_CHECK();                                                                                      \
    return XK_OK;                                                                                           \
  }                                                                                                         \
  int xk_minres_update_##SUF(T* v, const T* y, T* w1, const T* w2, T* x, const T* Palpha, const T* Pbeta,   \
                             int beta_is_dot, double* state, T* phi2, int S, int N, long ld, int nblk,      \
                             int k, void* stream) {                                                         \
    XK_MR_CHECK                                                                                             \
    hipLaunchKernelGGL((xk::minres_update_kernel<T>), XK_KRY_GRID(S, nblk), v, y, w1, w2, x, Palpha, Pbeta, \
                       state, phi2, S, N * MUL, ld * MUL, nblk, PS, beta_is_dot ? PS : 1, k);               \
    XK_LAUNCH_CHECK();                                                                                      \
    return XK_OK;                                                                                           \
  }

XK_DEFINE_MINRES(f64, double, 1, 1)
XK_DEFINE_MINRES(f32, float, 1, 1)
XK_DEFINE_MINRES(c128, double, 2, 2)
XK_DEFINE_MINRES(c64, float, 2, 2)

}  // extern "C"
