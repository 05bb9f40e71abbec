// xitorch_amd :: block Davidson for complex Hermitian operators (complex128 = _c128, complex64 = _c64).
//
// The real driver's chain (xk_chain.hip, xk_eigh_tri.hip) restated for complex data; the operator-panel product and the
// tall Gram / projection products stay on the real K1 kernels through the interleaved storage
// (kernels.dense_mm_complex).  Complex arrays are interleaved (re, im) pairs of the element type T; all strides below
// count COMPLEX elements.  Three stages:
//
//   herm_eigh_kernel     Rayleigh–Ritz of the k x k Hermitian T (the zhetrd / dstebz / dstein / zunmtr route, the
//                        complex counterpart of K3t): complex Householder reflectors chosen so that the sub-diagonal is
//                        real (zlarfg), bisection on the real tridiagonal (xk_tridiag.h), inverse iteration on it
//                        (real), back-transformation by the complex reflectors.  One workgroup per matrix; the packed
//                        lower triangle lives in LDS, each reflector in the column it eliminates.
//   herm_ritz_kernel     X = Y^T V, R = Y^T AV - diag(lam) Y^T MV, Tn = -R, max|R| per member and over the batch
//                        (integer max on the bit patterns: order-independent and NaN-propagating)
//   herm_gram_chol_kernel + herm_cholqr_apply_kernel
//                        CholeskyQR of a q-vector block in the (M-)inner product: G = W^H M W in a fixed summation
//                        order, G (+ shift_rel trace G) = R^H R, W <- W R^-1 (and MW <- MW R^-1)
#include "xk_common.h"
#include "xk_complex.h"
#include "xk_lane.h"
#include "xk_tridiag.h"

namespace xk {

constexpr int HERM_MAXK = 128;      // order of the Rayleigh–Ritz matrix served by herm_eigh_kernel
constexpr int HERM_MAXP = 16;       // wanted pairs per call
constexpr int HERM_THREADS = 256;
constexpr int HERM_RITZ_PC = 16;    // columns of Y per launch of herm_ritz_kernel
constexpr int HERM_CHOL_MAXQ = 32;  // block width of the CholeskyQR kernels
constexpr int HERM_CHOL_CH = 32;    // vector elements per LDS chunk of the Gram kernel

__device__ __forceinline__ int pk(int i, int c) { return i * (i + 1) / 2 + c; }   // packed lower triangle, c <= i

// bit pattern of a non-negative value widened to double: integer max over these is the max of the values, with a NaN
// (positive after fabs) above everything
__device__ __forceinline__ unsigned long long herm_key(double a) { return (unsigned long long)__double_as_longlong(a); }

}  // namespace xk

// LDS of herm_eigh_kernel in elements of T: packed triangle (complex), v, w, tau (complex n each), d, e, e^2, 16
// eigenvalues, 16 scratch, Z (p x n real eigenvectors of the tridiagonal matrix)
static long herm_eigh_lds_elems(long n, long p) {
  return n * (n + 1) + 6 * n + 3 * n + xk::HERM_MAXP + 16 + p * n;
}

namespace xk {

// ---------------------------------------------------------------------------------------------------------------------
// Rayleigh–Ritz: lowest / uppermost p eigenpairs of the Hermitian T[b] (lower triangle read, imaginary part of the
// diagonal ignored, like zheevd).  lam (B, p) ascending, Y (B, p, n) complex with Y[b, j] the j-th eigenvector;
// info[b] = 1 when the self-check fails (the caller repeats that member on the library).  ws: 5 n p elements of T per
// member (the LU factors of the inverse iteration: at n = 128 they do not fit next to the packed triangle).
template <typename T>
__global__ __launch_bounds__(HERM_THREADS) void herm_eigh_kernel(
    const T* __restrict__ Tin, T* __restrict__ lam_out, T* __restrict__ Y_out, int* __restrict__ info_out,
    T* __restrict__ ws, int n, int p, int uppest, long ldt, long sT) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  T* S = reinterpret_cast<T*>(smem);                  // n (n+1) / 2 complex: packed lower triangle
  T* vv = S + (long)n * (n + 1);                      // n complex: Householder vector over rows j+1.. (vv[0] = 1)
  T* ww = vv + 2 * n;                                 // n complex: w = tau A v
  T* tau = ww + 2 * n;                                // n complex
  T* dd = tau + 2 * n;                                // n diagonal of the tridiagonal matrix
  T* ee = dd + n;                                     // n sub-diagonal (ee[i] = (i+1, i))
  T* e2 = ee + n;                                     // n squares
  T* lamv = e2 + n;                                   // HERM_MAXP eigenvalues
  T* red = lamv + HERM_MAXP;                          // 16 scratch scalars
  T* Z = red + 16;                                    // p x n
  const int b = blockIdx.x;
  const int tid = threadIdx.x, nt = blockDim.x;
  const int lane = tid & 63, nw = nt >> 6;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const T* Tb = Tin + 2 * (long)b * sT;
  T* lu = ws + (long)b * 5 * n * p;
  const T eps = Limits<T>::eps;

  // (the diagonal is taken as real here, as zhetd2 does: an imaginary part handed over must not reach w = tau A22 v)
  for (int i = wave; i < n; i += nw)
    for (int c = lane; c <= i; c += 64) {
      cx<T> a = cld(Tb, (long)i * ldt + c);
      if (c == i) a.im = T(0);
      cst(S, pk(i, c), a);
    }
  __syncthreads();

  // ---- 1. Householder tridiagonalisation (zhetd2, lower): A <- H_j^H A H_j, H_j = I - tau_j v v^H -----------------
  // Three barriers per step: wave 0 forms the reflector | all threads form w = tau A22 v | all waves form
  // K = -tau/2 (w^H v) themselves (same data, same operations: the same number) and apply A22 -= v q^H + q v^H,
  // q = w + K v.
  for (int j = 0; j + 1 < n; ++j) {
    if (wave == 0) {
      // zlarfg on column j below the diagonal: H^H (alpha, x) = (beta, 0) with beta real
      const int i0 = j + 1 + lane, i1 = i0 + 64;
      const cx<T> x0 = i0 < n ? cld(S, pk(i0, j)) : cx<T>{T(0), T(0)};
      const cx<T> x1 = i1 < n ? cld(S, pk(i1, j)) : cx<T>{T(0), T(0)};
      const T sigma = wave_sum_dpp((lane > 0 ? x0.re * x0.re + x0.im * x0.im : T(0)) + x1.re * x1.re + x1.im * x1.im);
      const T ar = readlane(x0.re, 0), ai = readlane(x0.im, 0);
      cx<T> tj = {T(0), T(0)}, sc = {T(0), T(0)};
      T beta = ar;
      if (!(sigma == T(0) && ai == T(0))) {           // (a NaN column must poison the result, not be skipped)
        const T nrm = sqrt(ar * ar + ai * ai + sigma);
        beta = ar >= T(0) ? -nrm : nrm;
        tj = {(beta - ar) / beta, -ai / beta};
        const T dr = ar - beta, den = dr * dr + ai * ai;   // 1 / (alpha - beta)
        sc = {dr / den, -ai / den};
      }
      const cx<T> v0 = lane == 0 ? cx<T>{T(1), T(0)} : cmul(x0, sc);
      const cx<T> v1 = cmul(x1, sc);
      if (i0 < n) cst(vv, lane, v0);
      if (i1 < n) cst(vv, lane + 64, v1);
      // column j is not read again by the reduction: park the reflector there for the back-transformation
      if (lane > 0 && i0 < n) cst(S, pk(i0, j), v0);
      if (i1 < n) cst(S, pk(i1, j), v1);
      if (lane == 0) {
        cst(tau, j, tj);
        ee[j] = beta;
        dd[j] = S[2 * pk(j, j)];
      }
    }
    __syncthreads();
    const cx<T> tj = cld(tau, j);
    const int m = n - j - 1;                          // order of the trailing block (rows / columns j+1 ..)
    const bool active = tj.re != T(0) || tj.im != T(0);
    if (active) {
      // w = tau A22 v: two threads per row (adjacent lanes, combined by a shuffle); A[i][c] = S(i, c) for c <= i,
      // conj(S(c, i)) above the diagonal
      const int r = tid >> 1, h = tid & 1;
      cx<T> acc = {T(0), T(0)};
      if (r < m) {
        const int i = j + 1 + r;
        for (int c = j + 1 + h; c < n; c += 2) {
          const cx<T> v = cld(vv, c - j - 1);
          if (c <= i) cfma(acc, cld(S, pk(i, c)), v);
          else cfmac(acc, cld(S, pk(c, i)), v);
        }
      }
      acc.re += __shfl_xor(acc.re, 1, 64);
      acc.im += __shfl_xor(acc.im, 1, 64);
      if (r < m && h == 0) cst(ww, r, cmul(tj, acc));
    }
    __syncthreads();
    if (active) {
      // K = -tau/2 (w^H v) (real in exact arithmetic; kept complex like zhetd2)
      cx<T> dp = {T(0), T(0)};
      for (int r = lane; r < m; r += 64) cfmac(dp, cld(ww, r), cld(vv, r));
      dp.re = wave_sum_dpp(dp.re);
      dp.im = wave_sum_dpp(dp.im);
      const cx<T> K = cmul(cx<T>{T(-0.5) * tj.re, T(-0.5) * tj.im}, dp);
      for (int i = j + 1 + wave; i < n; i += nw) {
        const int ri = i - j - 1;
        const cx<T> vi = cld(vv, ri);
        cx<T> qi = cld(ww, ri);
        cfma(qi, K, vi);
        for (int c = j + 1 + lane; c <= i; c += 64) {
          const int rc = c - j - 1;
          const cx<T> vc = cld(vv, rc);
          cx<T> qc = cld(ww, rc);
          cfma(qc, K, vc);
          // A[i][c] -= v_i conj(q_c) + q_i conj(v_c)
          cx<T> a = cld(S, pk(i, c));
          const cx<T> t1 = cmulc(qc, vi), t2 = cmulc(vc, qi);
          a.re -= t1.re + t2.re;
          a.im -= t1.im + t2.im;
          cst(S, pk(i, c), a);
        }
      }
    }
    __syncthreads();
  }
  if (tid == 0) {
    dd[n - 1] = S[2 * pk(n - 1, n - 1)];
    ee[n - 1] = T(0);
  }
  __syncthreads();
  if (tid < n) e2[tid] = ee[tid] * ee[tid];
  __syncthreads();

  // ---- 2. bisection (dstebz): wave w -> wanted eigenvalue number w (ascending) --------------------------------------
  T gl = T(INFINITY), gu = T(-INFINITY), emax = T(0);
  for (int i = lane; i < n; i += 64) {
    const T rr = (i > 0 ? fabs(ee[i - 1]) : T(0)) + (i < n - 1 ? fabs(ee[i]) : T(0));
    gl = fmin(gl, dd[i] - rr);
    gu = fmax(gu, dd[i] + rr);
    emax = fmax(emax, e2[i]);
  }
  gl = -wave_max(-gl);
  gu = wave_max(gu);
  emax = wave_max(emax);
  const T tnorm = fmax(fabs(gl), fabs(gu));
  const T pivmin = Limits<T>::tiny * fmax(T(1), emax);
  for (int w = wave; w < p; w += nw) {
    const int target = (uppest ? n - p + w : w) + 1;
    const T lamw = tri_bisect_wave<T>(dd, e2, n, target, gl, gu, tnorm, pivmin, eps, lane);
    if (lane == 0) lamv[w] = lamw;
  }
  __syncthreads();
  if (tid == 0) {
    red[15] = T(0);                                   // "an iterate was annihilated" flag of step 3
    for (int j = 1; j < p; ++j) lamv[j] = fmax(lamv[j], lamv[j - 1]);
  }
  __syncthreads();

  // ---- 3. inverse iteration (dstein) on the real tridiagonal: lane j of wave 0 owns eigenvalue j -------------------
  // LU factors in `ws`, index [a][i][j]: the p lanes read consecutive addresses
  const T pfloor = eps * tnorm + pivmin;
#define AT(a, i) lu[((long)(a) * n + (i)) * p + j]
  if (tid < p) {
    const int j = tid;
    T shift = lamv[j];
    for (int q = j - 1; q >= 0; --q) {                // coincident eigenvalues get distinct shifts
      if (lamv[j] - lamv[q] < T(10) * eps * tnorm) shift += T(10) * eps * tnorm; else break;
    }
    // LU with partial pivoting (dgttrf); AT(1, .) holds the reciprocal pivots
    T dcur = dd[0] - shift, ucur = n > 1 ? ee[0] : T(0);
    for (int i = 0; i + 1 < n; ++i) {
      const T li = ee[i];
      const T dn = dd[i + 1] - shift;
      const T un = (i + 2 < n) ? ee[i + 1] : T(0);
      if (fabs(dcur) >= fabs(li)) {
        if (fabs(dcur) < pfloor) dcur = dcur < T(0) ? -pfloor : pfloor;
        const T inv = T(1) / dcur;
        const T fact = li * inv;
        AT(0, i) = fact; AT(1, i) = inv; AT(2, i) = ucur; AT(3, i) = T(0); AT(4, i) = T(0);
        dcur = dn - fact * ucur;
        ucur = un;
      } else {
        const T inv = T(1) / li;
        const T fact = dcur * inv;
        AT(0, i) = fact; AT(1, i) = inv; AT(2, i) = dn; AT(3, i) = un; AT(4, i) = T(1);
        dcur = ucur - fact * dn;
        ucur = -fact * un;
      }
    }
    if (fabs(dcur) < pfloor) dcur = dcur < T(0) ? -pfloor : pfloor;
    AT(1, n - 1) = T(1) / dcur;
    T* z = Z + (long)j * n;
    for (int i = 0; i < n; ++i) {                     // deterministic pseudo-random start in (-1, 1)
      const unsigned hh = hash32((unsigned)(i * 131 + j * 7919 + 12345));
      z[i] = T((int)(hh & 0xffffff) - 0x800000) / T(0x800000);
    }
  }
  __syncthreads();
  for (int it = 0; it < 3; ++it) {
    if (tid < p) {
      const int j = tid;
      T* z = Z + (long)j * n;
      T cur = z[0];
      for (int i = 0; i + 1 < n; ++i) {               // forward substitution with the recorded interchanges
        const T nxt = z[i + 1];
        const T l = AT(0, i);
        if (AT(4, i) == T(0)) { z[i] = cur; cur = nxt - l * cur; }
        else { z[i] = nxt; cur = cur - l * nxt; }
      }
      T zp1 = cur * AT(1, n - 1), zp2 = T(0);         // back substitution
      z[n - 1] = zp1;
      for (int i = n - 2; i >= 0; --i) {
        const T t = (z[i] - AT(2, i) * zp1 - AT(3, i) * zp2) * AT(1, i);
        z[i] = t;
        zp2 = zp1; zp1 = t;
      }
    }
    __syncthreads();
    // scale, modified Gram–Schmidt against every previous vector, normalise: wave 0, lanes over the vector
    if (wave == 0) {
      for (int j = 0; j < p; ++j) {
        T* zj = Z + (long)j * n;
        T mx = T(0);
        for (int i = lane; i < n; i += 64) mx = fmax(mx, fabs(zj[i]));
        mx = wave_max(mx);
        const T s = (mx > T(0) && mx < T(INFINITY)) ? T(1) / mx : T(1);
        for (int i = lane; i < n; i += 64) zj[i] *= s;
        for (int q = j - 1; q >= 0; --q) {
          const T* zq = Z + (long)q * n;
          T d = T(0);
          for (int i = lane; i < n; i += 64) d += zq[i] * zj[i];
          d = wave_sum_dpp(d);
          for (int i = lane; i < n; i += 64) zj[i] -= d * zq[i];
        }
        T nn = T(0);
        for (int i = lane; i < n; i += 64) nn += zj[i] * zj[i];
        nn = wave_sum_dpp(nn);
        const T inv = nn > T(0) ? T(1) / sqrt(nn) : T(0);
        if (lane == 0 && !(nn > T(0) && nn < T(INFINITY))) red[15] = T(1);
        for (int i = lane; i < n; i += 64) zj[i] *= inv;
      }
    }
    __syncthreads();
  }
#undef AT

  // ---- 4. self-check on the tridiagonal level: residuals, orthonormality, scale range ---------------------------
  if (wave == 0) {
    T worst = T(0), orth = T(0);
    int bad = 0;                                      // fmax / comparisons drop NaN: tracked explicitly
    for (int j = 0; j < p; ++j) {
      const T* zj = Z + (long)j * n;
      const T lam = lamv[j];
      T r = T(0);
      for (int i = lane; i < n; i += 64) {
        T t = (dd[i] - lam) * zj[i];
        if (i > 0) t += ee[i - 1] * zj[i - 1];
        if (i < n - 1) t += ee[i] * zj[i + 1];
        if (!(fabs(t) < T(INFINITY))) bad = 1;
        r = fmax(r, fabs(t));
      }
      worst = fmax(worst, wave_max(r));
      for (int q = 0; q <= j; ++q) {
        const T* zq = Z + (long)q * n;
        T d = T(0);
        for (int i = lane; i < n; i += 64) d += zq[i] * zj[i];
        d = wave_sum_dpp(d);
        const T dev = fabs(q == j ? d - T(1) : d);
        if (!(dev < T(INFINITY))) bad = 1;
        orth = fmax(orth, dev);
      }
    }
    bad = __any(bad) ? 1 : 0;
    if (!(tnorm < T(INFINITY))) bad = 1;
    if (!tri_scale_in_range(tnorm)) bad = 1;        // (xk_tridiag.h: outside it the reduction is not safe)
    if (red[15] != T(0)) bad = 1;
    if (lane == 0) {
      const T tol = T(100) * eps * tnorm + T(8) * pivmin;
      info_out[b] = (worst <= tol && orth <= T(32) * eps * n && !bad) ? 0 : 1;
    }
  }
  __syncthreads();

  // ---- 5. back-transformation y = H_0 ... H_{n-2} z (zunmtr), one wave per vector ----------------------------------
  for (int j = wave; j < p; j += nw) {
    const T* zj = Z + (long)j * n;
    cx<T> y0 = {lane < n ? zj[lane] : T(0), T(0)};
    cx<T> y1 = {lane + 64 < n ? zj[lane + 64] : T(0), T(0)};
    for (int r = n - 2; r >= 0; --r) {
      const cx<T> tr = cld(tau, r);
      if (tr.re == T(0) && tr.im == T(0)) continue;
      // v_r: rows <= r are 0, row r+1 is 1, rows > r+1 in column r of the packed triangle
      const int i0 = lane, i1 = lane + 64;
      const cx<T> v0 = (i0 >= n || i0 <= r) ? cx<T>{T(0), T(0)}
                       : (i0 == r + 1 ? cx<T>{T(1), T(0)} : cld(S, pk(i0, r)));
      const cx<T> v1 = (i1 >= n || i1 <= r) ? cx<T>{T(0), T(0)}
                       : (i1 == r + 1 ? cx<T>{T(1), T(0)} : cld(S, pk(i1, r)));
      cx<T> d = {T(0), T(0)};
      cfmac(d, v0, y0);
      cfmac(d, v1, y1);
      d.re = wave_sum_dpp(d.re);
      d.im = wave_sum_dpp(d.im);
      const cx<T> td = cmul(tr, d);                   // y -= tau (v^H y) v
      const cx<T> u0 = cmul(td, v0), u1 = cmul(td, v1);
      y0.re -= u0.re; y0.im -= u0.im;
      y1.re -= u1.re; y1.im -= u1.im;
    }
    T* Yb = Y_out + 2 * ((long)b * p + j) * n;
    if (lane < n) cst(Yb, lane, y0);
    if (lane + 64 < n) cst(Yb, lane + 64, y1);
    if (lane == 0) lam_out[(long)b * p + j] = lamv[j];
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Fused Ritz step for columns [c0, c0 + pc) (pc <= HERM_RITZ_PC): one thread per vector element, V / AV / MV read once
//   X[c] = sum_a Y[a, c] V[a],  R[c] = sum_a Y[a, c] (AV[a] - lam_c MV[a]),  Tn[c] = -R[c]
//   status[1 + b] = max(status[1 + b], max |R|),  status[0] = max over the batch   (bit patterns, atomic integer max)
template <typename T>
__global__ __launch_bounds__(256) void herm_ritz_kernel(
    const T* __restrict__ V, const T* __restrict__ AV, const T* __restrict__ MV, const T* __restrict__ Y,
    const T* __restrict__ lam, T* __restrict__ X, T* __restrict__ Tn, double* __restrict__ status, int k, int N,
    int c0, int pc, long ldv, long sV, long ldav, long sAV, long ldmv, long sMV, long sY, long sYa, long sYc,
    long sL, long ldx, long sX, long ldtn, long sTn) {
  constexpr int PC = HERM_RITZ_PC;
  const int b = blockIdx.y;
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  const bool live = n < N;
  const int nn = live ? n : 0;
  const T* Vb = V + 2 * (long)b * sV;
  const T* AVb = AV + 2 * (long)b * sAV;
  const T* MVb = MV != nullptr ? MV + 2 * (long)b * sMV : nullptr;
  const T* Yb = Y + 2 * ((long)b * sY + (long)c0 * sYc);
  cx<T> x[PC], ax[PC], mx[PC];
#pragma unroll
  for (int c = 0; c < PC; ++c) { x[c] = {T(0), T(0)}; ax[c] = {T(0), T(0)}; mx[c] = {T(0), T(0)}; }
  for (int a = 0; a < k; ++a) {
    const cx<T> v = cld(Vb, (long)a * ldv + nn);
    const cx<T> av = cld(AVb, (long)a * ldav + nn);
    const cx<T> mv = MVb != nullptr ? cld(MVb, (long)a * ldmv + nn) : v;
#pragma unroll
    for (int c = 0; c < PC; ++c) {
      if (c < pc) {
        const cx<T> y = cld(Yb, (long)a * sYa + (long)c * sYc);
        cfma(x[c], y, v);
        cfma(ax[c], y, av);
        if (MVb != nullptr) cfma(mx[c], y, mv);
      }
    }
  }
  double rmax = 0.0;
#pragma unroll
  for (int c = 0; c < PC; ++c) {
    if (c < pc) {
      const T l = lam[(long)b * sL + c0 + c];
      const cx<T> m = MVb != nullptr ? mx[c] : x[c];
      const cx<T> r = {ax[c].re - l * m.re, ax[c].im - l * m.im};
      if (live) {
        cst(X + 2 * ((long)b * sX + (long)(c0 + c) * ldx), n, x[c]);
        cst(Tn + 2 * ((long)b * sTn + (long)(c0 + c) * ldtn), n, cx<T>{-r.re, -r.im});
        const double mod = (double)sqrt(r.re * r.re + r.im * r.im);
        rmax = herm_key(fabs(mod)) > herm_key(rmax) ? fabs(mod) : rmax;
      }
    }
  }
  unsigned long long key = herm_key(rmax);
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    const unsigned long long o = __shfl_xor(key, s, 64);
    key = o > key ? o : key;
  }
  if ((threadIdx.x & 63) == 0) {
    atomicMax(reinterpret_cast<unsigned long long*>(status + 1 + b), key);
    atomicMax(reinterpret_cast<unsigned long long*>(status), key);
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Gram + Cholesky of a q-vector block, one workgroup per member:
//   G[i][j] = sum_n conj(W[i, n]) MW[j, n]   (upper triangle; every entry summed in a fixed order)
//   G += shift_rel trace(G) I (shift_rel > 0),  G = R^H R,  Rinv[b] = R^-1 (q x q complex, row-major)
// info[b] = index + 1 of the first non-positive pivot when info[b] is still 0 (sticky); the pivot is then taken as 1.
template <typename T>
__global__ __launch_bounds__(256) void herm_gram_chol_kernel(
    const T* __restrict__ W, const T* __restrict__ MW, T* __restrict__ Rinv, int* __restrict__ info, int q, int N,
    long ldw, long sW, long ldmw, long sMW, T shift_rel) {
  constexpr int QM = HERM_CHOL_MAXQ, CH = HERM_CHOL_CH;
  constexpr int NE = QM * (QM + 1) / 2;
  constexpr int EPT = (NE + 255) / 256;               // Gram entries per thread
  __shared__ cx<T> Wc[QM][CH + 1];
  __shared__ cx<T> Mc[QM][CH + 1];
  __shared__ cx<T> G[QM][QM + 1];                  // Gram matrix; row j becomes row j of R at Cholesky step j
  __shared__ int bad_sh;
  const int b = blockIdx.x;
  const int tid = threadIdx.x;
  const T* Wb = W + 2 * (long)b * sW;
  const T* Mb = MW != nullptr ? MW + 2 * (long)b * sMW : Wb;
  const long ldm = MW != nullptr ? ldmw : ldw;
  const int ne = q * (q + 1) / 2;
  int ei[EPT], ej[EPT];
  cx<T> g[EPT];
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    g[e] = {T(0), T(0)};
    const int idx = tid + e * 256;
    int i = 0, rem = idx;                              // entry idx -> (i, j), row i holding q - i entries
    while (i < q && rem >= q - i) { rem -= q - i; ++i; }
    ei[e] = idx < ne ? i : 0;
    ej[e] = idx < ne ? i + rem : 0;
  }
  for (int n0 = 0; n0 < N; n0 += CH) {
    for (int t = tid; t < q * CH; t += 256) {
      const int a = t / CH, c = t - a * CH;
      const bool ok = n0 + c < N;
      Wc[a][c] = ok ? cld(Wb, (long)a * ldw + n0 + c) : cx<T>{T(0), T(0)};
      Mc[a][c] = ok ? cld(Mb, (long)a * ldm + n0 + c) : cx<T>{T(0), T(0)};
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
      if (tid + e * 256 < ne) {
        for (int c = 0; c < CH; ++c) cfmac(g[e], Wc[ei[e]][c], Mc[ej[e]][c]);
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int e = 0; e < EPT; ++e) {
    if (tid + e * 256 < ne) G[ei[e]][ej[e]] = g[e];
  }
  if (tid == 0) bad_sh = 0;
  __syncthreads();
  if (tid == 0 && shift_rel > T(0)) {                  // shifted CholeskyQR: G + (shift_rel trace G) I
    T tr = T(0);
    for (int c = 0; c < q; ++c) tr += G[c][c].re;
    for (int c = 0; c < q; ++c) G[c][c].re += shift_rel * tr;
  }
  __syncthreads();
  // right-looking Cholesky in place, thread c owns column c
  for (int j = 0; j < q; ++j) {
    T d = G[j][j].re;
    if (!(d > T(0))) {
      if (tid == 0 && bad_sh == 0) bad_sh = j + 1;
      d = T(1);
    }
    const T rjj = sqrt(d);
    __syncthreads();
    if (tid < q && tid >= j) {
      const int c = tid;
      G[j][c] = c == j ? cx<T>{rjj, T(0)} : cx<T>{G[j][c].re / rjj, G[j][c].im / rjj};
    }
    __syncthreads();
    if (tid < q && tid > j) {
      const int c = tid;
      const cx<T> rjc = G[j][c];
      for (int r = j + 1; r <= c; ++r) {               // G[r][c] -= conj(R[j][r]) R[j][c]
        const cx<T> t = cmulc(G[j][r], rjc);
        G[r][c].re -= t.re;
        G[r][c].im -= t.im;
      }
    }
    __syncthreads();
  }
  // R^-1 column by column (thread c): R w = e_c by back substitution
  if (tid < q) {
    const int c = tid;
    T* Rb = Rinv + 2 * (long)b * q * q;
    for (int r = q - 1; r >= 0; --r) {
      cx<T> s = {r == c ? T(1) : T(0), T(0)};
      if (r <= c) {
        for (int m = r + 1; m <= c; ++m) {
          const cx<T> t = cmul(G[r][m], cld(Rb, (long)m * q + c));
          s.re -= t.re;
          s.im -= t.im;
        }
        const T inv = T(1) / G[r][r].re;
        s.re *= inv;
        s.im *= inv;
      } else {
        s = {T(0), T(0)};
      }
      cst(Rb, (long)r * q + c, s);
    }
  }
  if (tid == 0 && bad_sh != 0 && info[b] == 0) info[b] = bad_sh;
}

// W[c, n] <- sum_{a <= c} Rinv[a][c] W[a, n] in place (and the same for MW), one thread per element n
template <typename T>
__global__ __launch_bounds__(256) void herm_cholqr_apply_kernel(
    T* __restrict__ W, T* __restrict__ MW, const T* __restrict__ Rinv, int q, int N, long ldw, long sW, long ldmw,
    long sMW) {
  constexpr int QM = HERM_CHOL_MAXQ;
  const int b = blockIdx.y;
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= N) return;
  const T* Rb = Rinv + 2 * (long)b * q * q;
  for (int pass = 0; pass < (MW != nullptr ? 2 : 1); ++pass) {
    T* P = pass == 0 ? W + 2 * (long)b * sW : MW + 2 * (long)b * sMW;
    const long ld = pass == 0 ? ldw : ldmw;
    cx<T> w[QM];
#pragma unroll
    for (int a = 0; a < QM; ++a) w[a] = a < q ? cld(P, (long)a * ld + n) : cx<T>{T(0), T(0)};
#pragma unroll
    for (int c = 0; c < QM; ++c) {
      if (c < q) {
        cx<T> s = {T(0), T(0)};
#pragma unroll
        for (int a = 0; a <= c; ++a) cfma(s, cld(Rb, (long)a * q + c), w[a]);
        cst(P, (long)c * ld + n, s);
      }
    }
  }
}

}  // namespace xk

extern "C" {

long xk_herm_eigh_lds_bytes(int k, int p, int elem_size) {
  return herm_eigh_lds_elems(k, p) * elem_size + 64;
}

long xk_herm_eigh_workspace_elems(int B, int k, int p) { return 5L * B * k * p; }

#define XK_DEFINE_HERM(SUF, T)                                                                                         \
  int xk_herm_eigh_##SUF(const T* Tin, T* lam, T* Y, int* info, T* ws, long ws_elems, int B, int k, int p,           \
                         int uppest, long ldt, long sT, void* stream) {                                               \
    if (B < 0 || k < 1 || p < 1 || p > k || k > xk::HERM_MAXK || p > xk::HERM_MAXP || ldt < k) return XK_ERR_ARG;   \
    if (B == 0) return XK_OK;                                                                                         \
    if (ws == nullptr || ws_elems < xk_herm_eigh_workspace_elems(B, k, p)) return XK_ERR_ARG;                         \
    const long lds = xk_herm_eigh_lds_bytes(k, p, (int)sizeof(T));                                                    \
    if (lds > 160 * 1024) return XK_ERR_UNSUPPORTED;                                                                  \
    hipError_t e = hipFuncSetAttribute((const void*)xk::herm_eigh_kernel<T>,                                          \
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                         \
    if (e != hipSuccess) return (int)e;                                                                               \
    hipLaunchKernelGGL((xk::herm_eigh_kernel<T>), dim3(B), dim3(xk::HERM_THREADS), (size_t)lds, (hipStream_t)stream, \
                       Tin, lam, Y, info, ws, k, p, uppest, ldt, sT);                                                 \
    XK_LAUNCH_CHECK();                                                                                                \
    return XK_OK;                                                                                                     \
  }                                                                                                                   \
  int xk_herm_ritz_##SUF(const T* V, const T* AV, const T* MV, const T* Y, const T* lam, T* X, T* Tn,               \
                         double* status, int B, int k, int N, int p, long ldv, long sV, long ldav, long sAV,          \
                         long ldmv, long sMV, long sY, long sYa, long sYc, long sL, long ldx, long sX, long ldtn,     \
                         long sTn, void* stream) {                                                                    \
    if (B < 0 || k < 1 || N < 1 || p < 1 || B > 65535) return XK_ERR_ARG;                                             \
    if (ldv < N || ldav < N || (MV != nullptr && ldmv < N) || ldx < N || ldtn < N) return XK_ERR_ARG;                 \
    if (B == 0) return XK_OK;                                                                                         \
    hipError_t e = hipMemsetAsync(status, 0, sizeof(double) * (size_t)(B + 1), (hipStream_t)stream);                 \
    if (e != hipSuccess) return (int)e;                                                                               \
    for (int c0 = 0; c0 < p; c0 += xk::HERM_RITZ_PC) {                                                                \
      const int pc = p - c0 < xk::HERM_RITZ_PC ? p - c0 : xk::HERM_RITZ_PC;                                           \
      hipLaunchKernelGGL((xk::herm_ritz_kernel<T>), dim3((N + 255) / 256, B), dim3(256), 0, (hipStream_t)stream,      \
                         V, AV, MV, Y, lam, X, Tn, status, k, N, c0, pc, ldv, sV, ldav, sAV, ldmv, sMV, sY, sYa, sYc, \
                         sL, ldx, sX, ldtn, sTn);                                                                     \
      XK_LAUNCH_CHECK();                                                                                              \
    }                                                                                                                 \
    return XK_OK;                                                                                                     \
  }                                                                                                                   \
  int xk_herm_cholqr_##SUF(T* W, T* MW, T* Rinv, int* info, int B, int q, int N, long ldw, long sW, long ldmw,      \
                           long sMW, double shift_rel, void* stream) {                                                \
    if (B < 0 || q < 1 || q > xk::HERM_CHOL_MAXQ || N < 1 || ldw < N || (MW != nullptr && ldmw < N) || B > 65535)     \
      return XK_ERR_ARG;                                                                                              \
    if (B == 0) return XK_OK;                                                                                         \
    hipLaunchKernelGGL((xk::herm_gram_chol_kernel<T>), dim3(B), dim3(256), 0, (hipStream_t)stream, W, MW, Rinv,      \
                       info, q, N, ldw, sW, ldmw, sMW, (T)shift_rel);                                                 \
    XK_LAUNCH_CHECK();                                                                                                \
    hipLaunchKernelGGL((xk::herm_cholqr_apply_kernel<T>), dim3((N + 255) / 256, B), dim3(256), 0,                    \
                       (hipStream_t)stream, W, MW, Rinv, q, N, ldw, sW, ldmw, sMW);                                   \
    XK_LAUNCH_CHECK();                                                                                                \
    return XK_OK;                                                                                                     \
  }

XK_DEFINE_HERM(c128, double)
XK_DEFINE_HERM(c64, float)

}  // extern "C"
