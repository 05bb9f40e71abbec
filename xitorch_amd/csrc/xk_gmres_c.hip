// xitorch_amd :: GMRES on COMPLEX operators (complex128 = _c128, complex64 = _c64): the basis kernels and the
// device-side Hessenberg / Givens state of native_krylov.gmres for complex dtypes.  The real kernels are in
// xk_gmres.hip (state) and xk_dense.hip / xk_basis.hip (the K1 Gram product and xk_lincomb the real driver uses);
// neither has a complex form, and a Gram product of a complex basis needs the conjugate of the basis.
//
// Complex data is INTERLEAVED (re, im) storage (torch.view_as_real of a complex tensor); T is the underlying real
// type; every pointer offset, pitch, stride and length counts whole COMPLEX elements (as in xk_kry_*_c*, xk_csr_mm_c*).
// A 16 B vector holds CV = 1 complex128 or 2 complex64 elements.  One system is one (batch member, column) pair; the S
// systems advance in lock step.  An Arnoldi step (basis q_0 .. q_k, w = A q_k stored in basis row k+1) is
//
//   xk_gmres_gram_c    c1[i] = <q_i, w> = sum_n conj(q_i[n]) w[n], i <= k                    (CGS pass 1)
//   xk_lincomb_c       w <- w - sum_i c1[i] q_i                                              (projection 1)
//   xk_gmres_gram_c    c2[i] = <q_i, w1>, i <= k, and entry k+1 = |w1|^2 (imaginary part exactly 0)   (CGS pass 2)
//   xk_gmres_step_c    h[j,k] = c1[j] + c2[j], h[k+1,k] = sqrt(|w1|^2 - sum |c2[j]|^2) (real, >= 0), previous rotations
//                      replayed on the column, new rotation, rotated right-hand side g, est2 = |g[k+1]|^2, 1 / h[k+1,k]
//   xk_gmres_finish_c  q_{k+1} = (w1 - sum_j c2[j] q_j) / h[k+1,k]   in place             (projection 2 + normalisation)
//
// and an iterate is  xk_gmres_solve_c (R y = g, back substitution)  +  xk_lincomb_c (x = Q y).
//
// ROTATION CONVENTION.  For the pair (a, b), a = the rotated h[k,k] (complex), b = h[k+1,k] >= 0 (real):
//     cs = |a| / sqrt(|a|^2 + b^2)  (real),   sn = (a / |a|) b / sqrt(|a|^2 + b^2)  (complex);   a = 0:  cs = 0, sn = 1
// and the unitary G = [cs, sn; -conj(sn), cs] is applied from the LEFT:  G [a; b] = [(a/|a|) sqrt(|a|^2 + b^2); 0]
// (for a = 0: [b; 0]), g[k] <- cs g[k], g[k+1] = -conj(sn) g[k].  The diagonal of R carries the phase of a.
//
// State (double whatever the vector type): R (S, cap+1, cap) complex, row-major per system, only i <= j meaningful;
// sn (S, cap) complex; g (S, cap+1) complex; cs (S, cap) REAL.
//
// Reductions have a fixed shape and no atomics: xk_gmres_gram_c cuts every vector into fixed
// tiles of 256 lanes x 4 vectors of 16 B; a workgroup owns one tile of one system, keeps its piece of w in registers,
// streams the matching piece of every basis row once, reduces each row over the wave (vector precision) and over its 4
// waves (double) and writes ONE double pair per (system, tile, row) into the caller's scratch; a second kernel folds
// the tiles in a fixed order in double.  Loads are unconditional from clamped addresses; what a lane beyond the vector
// loaded is multiplied by a zeroed w.
#include "xk_common.h"
#include "xk_kry_layout.h"

namespace xk {

constexpr int GRAM_U = 4;           // 16 B vectors of w a lane keeps in registers
constexpr int GRAM_ROWS = 64;       // basis rows between two cross-wave folds

template <typename T> struct GramTile { static constexpr int value = 256 * GRAM_U * (Vec16<T>::n / 2); };

template <typename T>
__global__ __launch_bounds__(256) void gmres_gram_c_kernel(const T* __restrict__ Q, const T* __restrict__ w,
                                                           double* __restrict__ part, int N, int kq, long ldq, long sQ,
                                                           long sw, int nblk) {
  typedef typename Vec16<T>::type VT;
  constexpr int VN = Vec16<T>::n;
  constexpr int CV = VN / 2;
  __shared__ double sh[4][GRAM_ROWS][2];
  const int s = blockIdx.x / nblk;
  const int blk = blockIdx.x - s * nblk;
  const int npad = (N + CV - 1) / CV * CV;                 // (complex64: an odd N reads one pad element, which is 0)
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  long off[GRAM_U];
  VT wv[GRAM_U];
  T n2 = T(0);
  const T* ws = w + 2 * (long)s * sw;
#pragma unroll
  for (int u = 0; u < GRAM_U; ++u) {
    const int j = blk * GramTile<T>::value + (u * 256 + (int)threadIdx.x) * CV;
    const bool in = j < npad;
    off[u] = 2 * (long)(in ? j : npad - CV);               // clamped: always a whole vector inside [0, npad)
    VT v = *reinterpret_cast<const VT*>(ws + off[u]);
#pragma unroll
    for (int e = 0; e < VN; ++e) {
      v[e] = in ? v[e] : T(0);
      n2 += v[e] * v[e];
    }
    wv[u] = v;
  }
  const T* Qs = Q + 2 * (long)s * sQ;
  double* ps = part + ((long)s * nblk + blk) * (long)(kq + 1) * 2;
  for (int i0 = 0; i0 <= kq; i0 += GRAM_ROWS) {           // rows 0 .. kq-1: the basis; "row" kq: the norm entry
    const int i1 = i0 + GRAM_ROWS < kq + 1 ? i0 + GRAM_ROWS : kq + 1;
    const int iq = i1 < kq ? i1 : kq;
    int i = i0;
    for (; i + 2 <= iq; i += 2) {                         // two rows per trip: eight 16 B loads in flight per lane
      const T* qi = Qs + 2 * (long)i * ldq;
      VT qa[GRAM_U], qb[GRAM_U];
#pragma unroll
      for (int u = 0; u < GRAM_U; ++u) qa[u] = *reinterpret_cast<const VT*>(qi + off[u]);
#pragma unroll
      for (int u = 0; u < GRAM_U; ++u) qb[u] = *reinterpret_cast<const VT*>(qi + 2 * ldq + off[u]);
      T ra = T(0), ia = T(0), rb = T(0), ib = T(0);
#pragma unroll
      for (int u = 0; u < GRAM_U; ++u)
#pragma unroll
        for (int c = 0; c < CV; ++c) {                     // conj(q) * w
          ra += qa[u][2 * c] * wv[u][2 * c] + qa[u][2 * c + 1] * wv[u][2 * c + 1];
          ia += qa[u][2 * c] * wv[u][2 * c + 1] - qa[u][2 * c + 1] * wv[u][2 * c];
          rb += qb[u][2 * c] * wv[u][2 * c] + qb[u][2 * c + 1] * wv[u][2 * c + 1];
          ib += qb[u][2 * c] * wv[u][2 * c + 1] - qb[u][2 * c + 1] * wv[u][2 * c];
        }
      ra = wave_sum(ra);
      ia = wave_sum(ia);
      rb = wave_sum(rb);
      ib = wave_sum(ib);
      if (lane == 0) {
        sh[wave][i - i0][0] = (double)ra;
        sh[wave][i - i0][1] = (double)ia;
        sh[wave][i + 1 - i0][0] = (double)rb;
        sh[wave][i + 1 - i0][1] = (double)ib;
      }
    }
    if (i < iq) {
      const T* qi = Qs + 2 * (long)i * ldq;
      VT qa[GRAM_U];
#pragma unroll
      for (int u = 0; u < GRAM_U; ++u) qa[u] = *reinterpret_cast<const VT*>(qi + off[u]);
      T ra = T(0), ia = T(0);
#pragma unroll
      for (int u = 0; u < GRAM_U; ++u)
#pragma unroll
        for (int c = 0; c < CV; ++c) {
          ra += qa[u][2 * c] * wv[u][2 * c] + qa[u][2 * c + 1] * wv[u][2 * c + 1];
          ia += qa[u][2 * c] * wv[u][2 * c + 1] - qa[u][2 * c + 1] * wv[u][2 * c];
        }
      ra = wave_sum(ra);
      ia = wave_sum(ia);
      if (lane == 0) { sh[wave][i - i0][0] = (double)ra; sh[wave][i - i0][1] = (double)ia; }
    }
    if (i1 == kq + 1) {
      const T t = wave_sum(n2);
      if (lane == 0) { sh[wave][kq - i0][0] = (double)t; sh[wave][kq - i0][1] = 0.0; }
    }
    __syncthreads();
    if ((int)threadIdx.x < 2 * (i1 - i0)) {
      const int r = threadIdx.x >> 1, c = threadIdx.x & 1;
      ps[(long)(i0 + r) * 2 + c] = (sh[0][r][c] + sh[1][r][c]) + (sh[2][r][c] + sh[3][r][c]);
    }
    __syncthreads();
  }
}

// c[s, i] = sum over the tiles, lane l takes tiles l, l + 64, ... in order, then the fixed wave tree; one wave per (s, i)
template <typename T>
__global__ __launch_bounds__(64) void gmres_gram_c_fold_kernel(const double* __restrict__ part, T* __restrict__ c,
                                                               long sc, int kq, int nblk) {
  const int s = blockIdx.x / (kq + 1);
  const int i = blockIdx.x - s * (kq + 1);
  const double* ps = part + (long)s * nblk * (long)(kq + 1) * 2 + (long)i * 2;
  double re = 0.0, im = 0.0;
  for (int b = threadIdx.x; b < nblk; b += 64) {
    const d2 v = *reinterpret_cast<const d2*>(ps + (long)b * (kq + 1) * 2);
    re += v[0];
    im += v[1];
  }
  re = wave_sum(re);
  im = wave_sum(im);
  if (threadIdx.x == 0) {
    T* o = c + 2 * ((long)s * sc + i);
    o[0] = (T)re;
    o[1] = i == kq ? T(0) : (T)im;
  }
}

// Out[b, c, :] = beta Out + alpha sum_{a<k} C[b, c, a] V[b, a, :]; one lane owns 16 B of one output row
template <typename T>
__global__ __launch_bounds__(256) void lincomb_c_kernel(const T* __restrict__ V, const T* __restrict__ C, T* Out, int k,
                                                        int N, long ldv, long sV, long sC, long sCc, long ldo, long sO,
                                                        T alpha, T beta, int col_tiles) {
  typedef typename Vec16<T>::type VT;
  constexpr int VN = Vec16<T>::n;
  constexpr int CV = VN / 2;
  const int b = blockIdx.x / col_tiles;
  const int ct = blockIdx.x - b * col_tiles;
  const int c = blockIdx.y;
  const int j = (ct * 256 + threadIdx.x) * CV;
  if (j >= N) return;
  const T* Vb = V + 2 * ((long)b * sV + j);
  const T* Cb = C + 2 * ((long)b * sC + (long)c * sCc);
  VT acc;
#pragma unroll
  for (int e = 0; e < VN; ++e) acc[e] = T(0);
  int a = 0;
  for (; a + 4 <= k; a += 4) {
    VT v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = *reinterpret_cast<const VT*>(Vb + 2 * (long)(a + u) * ldv);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const T cr = Cb[2 * (a + u)], ci = Cb[2 * (a + u) + 1];
#pragma unroll
      for (int q = 0; q < CV; ++q) {
        acc[2 * q] += cr * v[u][2 * q] - ci * v[u][2 * q + 1];
        acc[2 * q + 1] += cr * v[u][2 * q + 1] + ci * v[u][2 * q];
      }
    }
  }
  for (; a < k; ++a) {
    const VT v0 = *reinterpret_cast<const VT*>(Vb + 2 * (long)a * ldv);
    const T cr = Cb[2 * a], ci = Cb[2 * a + 1];
#pragma unroll
    for (int q = 0; q < CV; ++q) {
      acc[2 * q] += cr * v0[2 * q] - ci * v0[2 * q + 1];
      acc[2 * q + 1] += cr * v0[2 * q + 1] + ci * v0[2 * q];
    }
  }
  T* Ob = Out + 2 * ((long)b * sO + (long)c * ldo + j);
  VT o;
  if (beta != T(0)) {
    o = *reinterpret_cast<const VT*>(Ob);
#pragma unroll
    for (int e = 0; e < VN; ++e) o[e] = beta * o[e] + alpha * acc[e];
  } else {
#pragma unroll
    for (int e = 0; e < VN; ++e) o[e] = alpha * acc[e];
  }
  *reinterpret_cast<VT*>(Ob) = o;
}

template <typename T>
__global__ __launch_bounds__(64) void gmres_step_c_kernel(
    const T* __restrict__ c1, long sc1, const T* __restrict__ c2n, long sc2, int k, int cap,
    double* __restrict__ R, double* __restrict__ cs, double* __restrict__ sn, double* __restrict__ g,
    T* __restrict__ inv_hn, T* __restrict__ est2, int S) {
  const int s = blockIdx.x * 64 + threadIdx.x;
  if (s >= S) return;
  const T* a1 = c1 + 2 * (long)s * sc1;
  const T* a2 = c2n + 2 * (long)s * sc2;
  double* Rs = R + 2 * (long)s * (cap + 1) * cap;
  double* css = cs + (long)s * cap;
  double* sns = sn + 2 * (long)s * cap;
  double* gs = g + 2 * (long)s * (cap + 1);
  // h[k+1,k]^2 = |w1|^2 - sum |c2[j]|^2 (orthonormal Q; c2 is rounding-sized next to w1: no cancellation)
  double n2 = (double)a2[2 * (k + 1)];
  for (int j = 0; j <= k; ++j) {
    const double cr = (double)a2[2 * j], ci = (double)a2[2 * j + 1];
    n2 -= cr * cr + ci * ci;
  }
  const double hn = n2 > 0.0 ? sqrt(n2) : 0.0;
  // column k of the Hessenberg, h[j,k] = c1[j] + c2[j], with the previous rotations applied on the fly
  double pr = (double)a1[0] + (double)a2[0], pi = (double)a1[1] + (double)a2[1];
  for (int j = 0; j < k; ++j) {
    const double nr = (double)a1[2 * (j + 1)] + (double)a2[2 * (j + 1)];
    const double ni = (double)a1[2 * (j + 1) + 1] + (double)a2[2 * (j + 1) + 1];
    const double c = css[j], tr = sns[2 * j], ti = sns[2 * j + 1];
    Rs[2 * ((long)j * cap + k)] = c * pr + (tr * nr - ti * ni);
    Rs[2 * ((long)j * cap + k) + 1] = c * pi + (tr * ni + ti * nr);
    const double qr = -(tr * pr + ti * pi) + c * nr;        // -conj(t) * prev + c * nxt
    const double qi = -(tr * pi - ti * pr) + c * ni;
    pr = qr;
    pi = qi;
  }
  const double b = hn;
  const double ma = sqrt(pr * pr + pi * pi);                // |a|
  const double den = sqrt(ma * ma + b * b);
  double c, tr, ti, rr, ri;
  if (ma > 0.0) {
    const double ur = pr / ma, ui = pi / ma;                // a / |a|
    c = ma / den;
    tr = ur * b / den;
    ti = ui * b / den;
    rr = ur * den;                                          // G [a; b] = [(a/|a|) den; 0]
    ri = ui * den;
  } else {
    c = 0.0; tr = 1.0; ti = 0.0; rr = b; ri = 0.0;
  }
  css[k] = c;
  sns[2 * k] = tr;
  sns[2 * k + 1] = ti;
  Rs[2 * ((long)k * cap + k)] = rr;
  Rs[2 * ((long)k * cap + k) + 1] = ri;
  const double gr = gs[2 * k], gi = gs[2 * k + 1];
  gs[2 * k] = c * gr;
  gs[2 * k + 1] = c * gi;
  const double hr = -(tr * gr + ti * gi), hi = -(tr * gi - ti * gr);      // -conj(sn) * g[k]
  gs[2 * (k + 1)] = hr;
  gs[2 * (k + 1) + 1] = hi;
  inv_hn[s] = hn > 0.0 ? (T)(1.0 / hn) : T(0);
  est2[(long)s * KRY_MAX_PART] = (T)(hr * hr + hi * hi);
}

// q[k+1] = (w1 - sum_{j<=k} c2[j] q[j]) * inv_hn, in place in basis row k+1 (which holds w1).  Lane owns 16 B.
template <typename T>
__global__ __launch_bounds__(256) void gmres_finish_c_kernel(T* __restrict__ Q, const T* __restrict__ c2n, long sc2,
                                                             const T* __restrict__ inv_hn, int N, int k, long ldq,
                                                             long sQ, int col_tiles) {
  typedef typename Vec16<T>::type VT;
  constexpr int VN = Vec16<T>::n;
  constexpr int CV = VN / 2;
  const int s = blockIdx.x / col_tiles;
  const int ct = blockIdx.x - s * col_tiles;
  const int j0 = (ct * 256 + threadIdx.x) * CV;
  if (j0 >= N) return;
  T* Qs = Q + 2 * ((long)s * sQ + j0);
  const T* cc = c2n + 2 * (long)s * sc2;
  VT acc;
#pragma unroll
  for (int e = 0; e < VN; ++e) acc[e] = T(0);
  int j = 0;
  for (; j + 4 <= k + 1; j += 4) {
    VT q[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) q[u] = *reinterpret_cast<const VT*>(Qs + 2 * (long)(j + u) * ldq);
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const T cr = cc[2 * (j + u)], ci = cc[2 * (j + u) + 1];
#pragma unroll
      for (int e = 0; e < CV; ++e) {
        acc[2 * e] += cr * q[u][2 * e] - ci * q[u][2 * e + 1];
        acc[2 * e + 1] += cr * q[u][2 * e + 1] + ci * q[u][2 * e];
      }
    }
  }
  for (; j <= k; ++j) {
    const VT q0 = *reinterpret_cast<const VT*>(Qs + 2 * (long)j * ldq);
    const T cr = cc[2 * j], ci = cc[2 * j + 1];
#pragma unroll
    for (int e = 0; e < CV; ++e) {
      acc[2 * e] += cr * q0[2 * e] - ci * q0[2 * e + 1];
      acc[2 * e + 1] += cr * q0[2 * e + 1] + ci * q0[2 * e];
    }
  }
  const T sc = inv_hn[s];
  VT w = *reinterpret_cast<const VT*>(Qs + 2 * (long)(k + 1) * ldq);
#pragma unroll
  for (int e = 0; e < VN; ++e) w[e] = (w[e] - acc[e]) * sc;
  *reinterpret_cast<VT*>(Qs + 2 * (long)(k + 1) * ldq) = w;
}

// back substitution R y = g (upper triangular kd x kd, complex), one wave per system, y in LDS (16 B per entry); a zero
// pivot (breakdown: the Krylov space of that system is exhausted) gives y_i = 0
template <typename T>
__global__ __launch_bounds__(64) void gmres_solve_c_kernel(const double* __restrict__ R, const double* __restrict__ g,
                                                           T* __restrict__ y, long sy, int kd, int cap) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double* ys = reinterpret_cast<double*>(smem);
  const int s = blockIdx.x;
  const int lane = threadIdx.x;
  const double* Rs = R + 2 * (long)s * (cap + 1) * cap;
  const double* gs = g + 2 * (long)s * (cap + 1);
  for (int i = kd - 1; i >= 0; --i) {
    double pr = 0.0, pi = 0.0;
    for (int j = i + 1 + lane; j < kd; j += 64) {
      const double rr = Rs[2 * ((long)i * cap + j)], ri = Rs[2 * ((long)i * cap + j) + 1];
      const double yr = ys[2 * j], yi = ys[2 * j + 1];
      pr += rr * yr - ri * yi;
      pi += rr * yi + ri * yr;
    }
    const double tr = wave_sum(pr), ti = wave_sum(pi);
    if (lane == 0) {
      const double dr = Rs[2 * ((long)i * cap + i)], di = Rs[2 * ((long)i * cap + i) + 1];
      const double d2n = dr * dr + di * di;
      const double nr = gs[2 * i] - tr, ni = gs[2 * i + 1] - ti;
      ys[2 * i] = d2n != 0.0 ? (nr * dr + ni * di) / d2n : 0.0;           // (n conj(d)) / |d|^2
      ys[2 * i + 1] = d2n != 0.0 ? (ni * dr - nr * di) / d2n : 0.0;
    }
    __syncthreads();
  }
  for (int j = lane; j < kd; j += 64) {
    y[2 * ((long)s * sy + j)] = (T)ys[2 * j];
    y[2 * ((long)s * sy + j) + 1] = (T)ys[2 * j + 1];
  }
}

}  // namespace xk

extern "C" {

#define XK_DEFINE_GMRESC(SUF, T)                                                                                 \
  int xk_gmres_gram_##SUF(const T* Q, const T* w, T* c, double* scratch, int S, int N, int kq, long ldq, long sQ, \
                          long sw, long sc, int nblk, void* stream) {                                            \
    if (S < 0 || N < 0 || kq < 0) return XK_ERR_ARG;                                                             \
    if (S == 0) return XK_OK;                                                                                    \
    constexpr int CV = xk::Vec16<T>::n / 2;                                                                      \
    constexpr int TILE = xk::GramTile<T>::value;                                                                 \
    if (nblk != (N + TILE - 1) / TILE) return XK_ERR_ARG;                                                        \
    const long npad = (long)((N + CV - 1) / CV) * CV;                                                            \
    if ((ldq % CV) || (sQ % CV) || (sw % CV) || ((uintptr_t)Q & 15) || ((uintptr_t)w & 15) ||                    \
        ((uintptr_t)scratch & 15) || (kq > 0 && ldq < npad) || (S > 1 && sw < npad))                             \
      return XK_ERR_UNSUPPORTED;                                                                                 \
    if ((long)S * nblk > 2147483647L || (long)S * (kq + 1) > 2147483647L) return XK_ERR_UNSUPPORTED;             \
    if (N > 0) { /* N == 0: no tile, the fold alone writes the empty sums (zeros), like the other entry points */ \
      hipLaunchKernelGGL((xk::gmres_gram_c_kernel<T>), dim3((unsigned)((long)S * nblk)), dim3(256), 0,           \
                         (hipStream_t)stream, Q, w, scratch, N, kq, ldq, sQ, sw, nblk);                          \
      XK_LAUNCH_CHECK();                                                                                         \
    }                                                                                                            \
    hipLaunchKernelGGL((xk::gmres_gram_c_fold_kernel<T>), dim3((unsigned)((long)S * (kq + 1))), dim3(64), 0,     \
                       (hipStream_t)stream, scratch, c, sc, kq, nblk);                                           \
    XK_LAUNCH_CHECK();                                                                                           \
    return XK_OK;                                                                                                \
  }                                                                                                              \
  int xk_lincomb_##SUF(const T* V, const T* C, T* Out, int B, int k, int N, int P, long ldv, long sV, long sC,   \
                       long sCc, long ldo, long sO, double alpha, double beta, void* stream) {                   \
    if (B < 0 || k < 0 || N < 0 || P < 0 || P > 65535) return XK_ERR_ARG;                                        \
    if (B == 0 || N == 0 || P == 0) return XK_OK;                                                                \
    constexpr int CV = xk::Vec16<T>::n / 2;                                                                      \
    const long npad = (long)((N + CV - 1) / CV) * CV;                                                            \
    if ((ldv % CV) || (sV % CV) || (ldo % CV) || (sO % CV) || ((uintptr_t)V & 15) || ((uintptr_t)Out & 15) ||    \
        (k > 1 && ldv < npad) || (P > 1 && ldo < npad))                                                          \
      return XK_ERR_UNSUPPORTED;                                                                                 \
    const int ct = (N + 256 * CV - 1) / (256 * CV);                                                              \
    if ((long)B * ct > 2147483647L) return XK_ERR_UNSUPPORTED;                                                   \
    hipLaunchKernelGGL((xk::lincomb_c_kernel<T>), dim3((unsigned)((long)B * ct), (unsigned)P), dim3(256), 0,     \
                       (hipStream_t)stream, V, C, Out, k, N, ldv, sV, sC, sCc, ldo, sO, (T)alpha, (T)beta, ct);  \
    XK_LAUNCH_CHECK();                                                                                           \
    return XK_OK;                                                                                                \
  }                                                                                                              \
  int xk_gmres_step_##SUF(const T* c1, long sc1, const T* c2n, long sc2, int k, int cap, double* R, double* cs,   \
                          double* sn, double* g, T* inv_hn, T* est2, int S, void* stream) {                      \
    if (S < 0 || k < 0 || cap <= 0 || k >= cap) return XK_ERR_ARG;                                               \
    if (S == 0) return XK_OK;                                                                                    \
    hipLaunchKernelGGL((xk::gmres_step_c_kernel<T>), dim3((S + 63) / 64), dim3(64), 0, (hipStream_t)stream, c1,  \
                       sc1, c2n, sc2, k, cap, R, cs, sn, g, inv_hn, est2, S);                                    \
    XK_LAUNCH_CHECK();                                                                                           \
    return XK_OK;                                                                                                \
  }                                                                                                              \
  int xk_gmres_finish_##SUF(T* Q, const T* c2n, long sc2, const T* inv_hn, int S, int N, int k, long ldq,        \
                            long sQ, void* stream) {                                                             \
    if (S < 0 || N < 0 || k < 0) return XK_ERR_ARG;                                                              \
    if (S == 0 || N == 0) return XK_OK;                                                                          \
    constexpr int CV = xk::Vec16<T>::n / 2;                                                                      \
    if ((ldq % CV) || (sQ % CV) || ((uintptr_t)Q & 15) || ldq < (long)((N + CV - 1) / CV) * CV)                   \
      return XK_ERR_UNSUPPORTED;                                                                                 \
    const int ct = (N + 256 * CV - 1) / (256 * CV);                                                              \
    if ((long)S * ct > 2147483647L) return XK_ERR_UNSUPPORTED;                                                   \
    hipLaunchKernelGGL((xk::gmres_finish_c_kernel<T>), dim3((unsigned)((long)S * ct)), dim3(256), 0,             \
                       (hipStream_t)stream, Q, c2n, sc2, inv_hn, N, k, ldq, sQ, ct);                             \
    XK_LAUNCH_CHECK();                                                                                           \
    return XK_OK;                                                                                                \
  }                                                                                                              \
  int xk_gmres_solve_##SUF(const double* R, const double* g, T* y, long sy, int S, int kd, int cap,              \
                           void* stream) {                                                                       \
    if (S < 0 || kd < 0 || cap <= 0 || kd > cap) return XK_ERR_ARG;                                              \
    if (S == 0 || kd == 0) return XK_OK;                                                                         \
    if (kd > 4096) return XK_ERR_UNSUPPORTED;     /* y of one system lives in LDS (64 KiB, 16 B per entry) */    \
    hipLaunchKernelGGL((xk::gmres_solve_c_kernel<T>), dim3(S), dim3(64), (size_t)kd * 2 * sizeof(double),        \
                       (hipStream_t)stream, R, g, y, sy, kd, cap);                                               \
    XK_LAUNCH_CHECK();                                                                                           \
    return XK_OK;                                                                                                \
  }

XK_DEFINE_GMRESC(c128, double)
XK_DEFINE_GMRESC(c64, float)

}  // extern "C"
