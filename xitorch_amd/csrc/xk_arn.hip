// xitorch_amd :: kernels of the Krylov-Schur Arnoldi iteration for non-Hermitian eigenpairs, eigs(method="arnoldi")
// (Stewart, SIAM J. Matrix Anal. Appl. 23 (2001) 601).  An extension (the reference has Hermitian eigensolvers only).
//
// The Arnoldi step reuses xk_gkl_sweep_* (CGS2 in three passes over the basis).  Two kernels are new:
//
// xk_arn_finish  — xk_gkl_finish (same fixed-order sums of a sweep's partials, same norm, same breakdown flag) with one
//   more output: the dots also go into a column of the device-resident Hessenberg matrix H, stored (accumulate = 0) or
//   added (accumulate = 1).  The Arnoldi column is c1 + c2 of the two projecting passes; the norm goes to H[j+1, j].
//
// xk_arn_schur   — everything a restart needs from the m x m Rayleigh quotient B = H[:m, :m] (m <= 48) and beta =
//   H[m, m-1], one workgroup of ONE wave per member, all arithmetic in complex double whatever the operator's dtype:
//     1. power-of-two scaling by max |B_ij| (exact); a non-finite entry sets a flag and nothing else is written
//     2. Householder reduction to Hessenberg form, accumulated into Z (B after a restart is a full block plus a row)
//     3. single-shift complex QR: Givens rotations, Wilkinson shift, exceptional shifts at iterations 10 and 20 of a
//        block, at most 30 m iterations in all  ->  B = Z T Z^H, T upper triangular
//     4. ranking of diag(T) by `which`; for a real operator conjugate partners share their key and stay adjacent
//        (positive imaginary part first), and a cut at `keep` that separates partners moves by one
//     5. the selected eigenvalues are brought to the leading positions by adjacent swaps (one Givens rotation each)
//     6. Ritz vectors of the leading neig eigenvalues by back substitution in T, y = Z x, res = |beta| |y[m-1]|
//     7. restart coefficients: complex Q = Z[:, :keep'], Hnext = T[:keep', :keep'], spike beta Z[m-1, :keep'];  real: a
//        REAL orthonormal Q spanning the same space (column-pivoted Gram-Schmidt, every projection applied twice, on
//        [Re Z_k | Im Z_k]), Hnext = Q^T B Q, spike beta Q[m-1, :]
//   LDS: three 48 x 49 complex-double arrays (T, Z and a scratch; the pitch of 49 skews the rows over the banks so
//   that "lane = row" phases are conflict-free) = 110.25 KiB, plus < 4 KiB of bookkeeping, of the 160 KiB of a CU.
//   The wave alternates between phases in which lane j owns column j (rotations from the left) and phases in which
//   lane i owns row i (rotations from the right): every sum is a serial loop of one lane, there is no cross-lane
//   reduction and no atomic, so a repeat call returns the same bits.
//
// The member algorithm is written as a sequence of lane-parallel phases (ARN_LANES) with wave-uniform control flow
// between them; with XK_ARN_HOST defined the same text compiles as plain C++ with the lanes as a loop.
// All stores are ordinary vector-memory stores.
#include "xk_arn_check.h"
#include <float.h>
#include <math.h>
#ifndef XK_ARN_HOST
#include "xk_common.h"
#define ARN_HD __device__ __forceinline__
#define ARN_LANES(l) for (int l = (int)threadIdx.x, once_ = 1; once_; once_ = 0)
#define ARN_SYNC() __syncthreads()
#define ARN_SHARED __shared__
#else
#define ARN_HD static inline
#define ARN_LANES(l) for (int l = 0; l < 64; ++l)
#define ARN_SYNC() ((void)0)
#define ARN_SHARED static
#endif

namespace xk {

constexpr int ARN_LD = ARN_MAX_ROWS + 1;           // pitch (complex elements) of the LDS arrays
constexpr int ARN_LDR = 2 * ARN_LD;                // the same pitch in doubles (the real views)
constexpr int ARN_STATUS = 8;                      // ints per member in `status`
constexpr int ARN_FLAG_NONFINITE = 1, ARN_FLAG_QR_LIMIT = 2, ARN_FLAG_NOT_CLOSED = 4, ARN_FLAG_KEEP_MOVED = 8;

struct cd { double re, im; };
ARN_HD cd cmk(double re, double im) { cd r; r.re = re; r.im = im; return r; }
ARN_HD cd cadd(cd a, cd b) { return cmk(a.re + b.re, a.im + b.im); }
ARN_HD cd csub(cd a, cd b) { return cmk(a.re - b.re, a.im - b.im); }
ARN_HD cd cmul(cd a, cd b) { return cmk(a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re); }
ARN_HD cd cmulc(cd a, cd b) { return cmk(a.re * b.re + a.im * b.im, a.re * b.im - a.im * b.re); }   // conj(a) b
ARN_HD cd cconj(cd a) { return cmk(a.re, -a.im); }
ARN_HD cd cscl(cd a, double s) { return cmk(a.re * s, a.im * s); }
ARN_HD double cabs1(cd a) { return fabs(a.re) + fabs(a.im); }
ARN_HD double cabs2(cd a) { return hypot(a.re, a.im); }
ARN_HD cd cdivd(cd a, cd b) {                      // Smith's division: no overflow in |b|^2
  if (fabs(b.re) >= fabs(b.im)) {
    const double r = b.im / b.re, d = b.re + b.im * r;
    return cmk((a.re + a.im * r) / d, (a.im - a.re * r) / d);
  }
  const double r = b.re / b.im, d = b.re * r + b.im;
  return cmk((a.re * r + a.im) / d, (a.im * r - a.re) / d);
}
ARN_HD cd csqrtd(cd a) {
  const double r = cabs2(a);
  if (r == 0.0) return cmk(0.0, 0.0);
  if (a.re >= 0.0) {
    const double t = sqrt(0.5 * (r + a.re));
    return cmk(t, a.im / (2.0 * t));
  }
  const double t = sqrt(0.5 * (r - a.re));
  return cmk(fabs(a.im) / (2.0 * t), a.im >= 0.0 ? t : -t);
}
// Givens rotation [c s; -conj(s) c] (c real) that maps (a, b) to (r, 0)
ARN_HD void givens(cd a, cd b, double& c, cd& s) {
  const double na = cabs2(a), nb = cabs2(b);
  if (nb == 0.0) { c = 1.0; s = cmk(0.0, 0.0); return; }
  if (na == 0.0) { c = 0.0; s = cscl(cconj(b), 1.0 / nb); return; }
  const double r = hypot(na, nb);
  c = na / r;
  s = cscl(cmul(cscl(a, 1.0 / na), cconj(b)), 1.0 / r);
}
ARN_HD double rank_key(cd lam, int which) {
  switch (which) {
    case 0: return cabs2(lam);
    case 1: return lam.re;
    case 2: return -lam.re;
    case 3: return lam.im;
    default: return -lam.im;
  }
}

// element (r, c) of member b of H (Bt, m + 1, m) row-major: real doubles, or interleaved complex
template <bool CPLX>
ARN_HD cd h_load(const double* Hb, int m, int r, int c) {
  if (CPLX) return cmk(Hb[2 * ((long)r * m + c)], Hb[2 * ((long)r * m + c) + 1]);
  return cmk(Hb[(long)r * m + c], 0.0);
}

#ifndef XK_ARN_HOST
template <bool CPLX>
__global__ __launch_bounds__(64) void arn_schur_kernel(
    const double* __restrict__ H, int m, int neig, int keep, const int* __restrict__ keep_add, int which, double tol,
    double u, const int* __restrict__ brk, double* __restrict__ theta, double* __restrict__ Y, double* __restrict__ res,
    double* __restrict__ Q, double* __restrict__ Hnext, int* __restrict__ status) {
  const int b = blockIdx.x;
#else
template <bool CPLX>
void arn_schur_member(const double* H, int m, int neig, int keep, const int* keep_add, int which, double tol, double u,
                      const int* brk, double* theta, double* Y, double* res, double* Q, double* Hnext, int* status,
                      int b) {
#endif
  ARN_SHARED cd T[ARN_MAX_ROWS * ARN_LD], Z[ARN_MAX_ROWS * ARN_LD], S[ARN_MAX_ROWS * ARN_LD];
  ARN_SHARED cd vv[ARN_MAX_ROWS], lam[ARN_MAX_ROWS];
  ARN_SHARED double rowa[64], rowb[64], key[ARN_MAX_ROWS], cn[2 * ARN_MAX_ROWS];
  ARN_SHARED int partner[ARN_MAX_ROWS], rk[ARN_MAX_ROWS], posrk[ARN_MAX_ROWS], used[2 * ARN_MAX_ROWS],
      qcol[ARN_MAX_ROWS], cflag[ARN_MAX_ROWS];
  constexpr int EL = CPLX ? 2 : 1;
  const double EPS = DBL_EPSILON;
  const double* Hb = H + (long)b * (m + 1) * m * EL;
  int* st = status + (long)b * ARN_STATUS;
  const int brkcode = brk ? brk[b] : -1;

  // ---- 1. load, finite check, scaling
  ARN_LANES(l) {
    double mx = 0.0, bad = 0.0;
    if (l < m) {
      for (int c = 0; c < m; ++c) {
        const cd v = h_load<CPLX>(Hb, m, l, c);
        T[l * ARN_LD + c] = v;
        Z[l * ARN_LD + c] = cmk(l == c ? 1.0 : 0.0, 0.0);
        mx = fmax(mx, fmax(fabs(v.re), fabs(v.im)));
        if (!(fabs(v.re) <= DBL_MAX) || !(fabs(v.im) <= DBL_MAX)) bad = 1.0;
      }
    }
    rowa[l] = mx;
    rowb[l] = bad;
  }
  ARN_SYNC();
  const cd beta = h_load<CPLX>(Hb, m, m, m - 1);
  double mx = 0.0;
  bool bad = !(cabs1(beta) <= DBL_MAX);
  for (int i = 0; i < m; ++i) {
    mx = fmax(mx, rowa[i]);
    bad = bad || rowb[i] != 0.0;
  }
  ARN_SYNC();
  if (bad) {
    ARN_LANES(l) if (l == 0) {
      st[0] = 0; st[1] = 0; st[2] = ARN_FLAG_NONFINITE; st[3] = 0; st[4] = brkcode; st[5] = 0; st[6] = 0; st[7] = 0;
    }
    return;
  }
  const int ex = mx > 0.0 ? ilogb(mx) : 0;
  const double sc = scalbn(1.0, -ex), isc = scalbn(1.0, ex);       // max |B_ij| * sc in [1, 2)
  ARN_LANES(l) {
    double ss = 0.0;
    if (l < m)
      for (int c = 0; c < m; ++c) {
        const cd v = cscl(T[l * ARN_LD + c], sc);
        T[l * ARN_LD + c] = v;
        ss += v.re * v.re + v.im * v.im;
      }
    rowa[l] = ss;
  }
  ARN_SYNC();
  double fro = 0.0;
  for (int i = 0; i < m; ++i) fro += rowa[i];
  fro = sqrt(fro);                                                 // |B|_F of the scaled matrix
  ARN_SYNC();

  // ---- 2. Householder reduction to Hessenberg form, T <- P T P, Z <- Z P with P = I - 2 v v^H
  for (int k = 0; k + 2 < m; ++k) {
    double sigma = 0.0;
    for (int i = k + 2; i < m; ++i) {
      const cd v = T[i * ARN_LD + k];
      sigma += v.re * v.re + v.im * v.im;
    }
    if (sigma == 0.0) continue;                                    // the column is in Hessenberg form already
    const cd x0 = T[(k + 1) * ARN_LD + k];
    const double a0 = cabs2(x0), nx = sqrt(a0 * a0 + sigma);
    const cd ph = a0 > 0.0 ? cscl(x0, 1.0 / a0) : cmk(1.0, 0.0);
    const cd alpha = cscl(ph, -nx);
    const cd v0 = csub(x0, alpha);
    const double vn = sqrt(v0.re * v0.re + v0.im * v0.im + sigma), ivn = 1.0 / vn;
    ARN_SYNC();
    ARN_LANES(l) if (l > k && l < m) vv[l] = cscl(l == k + 1 ? v0 : T[l * ARN_LD + k], ivn);
    ARN_SYNC();
    ARN_LANES(j) if (j >= k && j < m) {
      if (j == k) {
        T[(k + 1) * ARN_LD + k] = alpha;
        for (int i = k + 2; i < m; ++i) T[i * ARN_LD + k] = cmk(0.0, 0.0);
      } else {
        cd w = cmk(0.0, 0.0);
        for (int i = k + 1; i < m; ++i) w = cadd(w, cmulc(vv[i], T[i * ARN_LD + j]));
        w = cscl(w, 2.0);
        for (int i = k + 1; i < m; ++i) T[i * ARN_LD + j] = csub(T[i * ARN_LD + j], cmul(vv[i], w));
      }
    }
    ARN_SYNC();
    ARN_LANES(i) if (i < m) {
      cd w = cmk(0.0, 0.0), wz = cmk(0.0, 0.0);
      for (int j = k + 1; j < m; ++j) {
        w = cadd(w, cmul(T[i * ARN_LD + j], vv[j]));
        wz = cadd(wz, cmul(Z[i * ARN_LD + j], vv[j]));
      }
      w = cscl(w, 2.0);
      wz = cscl(wz, 2.0);
      for (int j = k + 1; j < m; ++j) {
        const cd vc = cconj(vv[j]);
        T[i * ARN_LD + j] = csub(T[i * ARN_LD + j], cmul(w, vc));
        Z[i * ARN_LD + j] = csub(Z[i * ARN_LD + j], cmul(wz, vc));
      }
    }
    ARN_SYNC();
  }

  // ---- 3. single-shift QR iteration on the Hessenberg matrix (rotation k of a sweep is kept in vv[k], rowa[k])
  int ihi = m - 1, its = 0, total = 0, qr_fail = 0;
  const int limit = 30 * m;
  while (ihi >= 1) {
    int lo;
    for (lo = ihi; lo >= 1; --lo) {
      double s = cabs1(T[(lo - 1) * ARN_LD + lo - 1]) + cabs1(T[lo * ARN_LD + lo]);
      if (s == 0.0) s = fro;
      if (cabs1(T[lo * ARN_LD + lo - 1]) <= EPS * s) break;
    }
    ARN_SYNC();
    if (lo >= 1) {
      ARN_LANES(l) if (l == 0) T[lo * ARN_LD + lo - 1] = cmk(0.0, 0.0);
      ARN_SYNC();
    }
    if (lo == ihi) {
      --ihi;
      its = 0;
      continue;
    }
    if (total >= limit) {
      qr_fail = 1;
      break;
    }
    ++its;
    ++total;
    cd mu;
    {
      const cd a = T[(ihi - 1) * ARN_LD + ihi - 1], bb = T[(ihi - 1) * ARN_LD + ihi];
      const cd c = T[ihi * ARN_LD + ihi - 1], d = T[ihi * ARN_LD + ihi];
      if (its == 10 || its == 20) {
        mu = cadd(d, cmk(0.75 * cabs1(c), 0.0));                   // exceptional shift
      } else {
        const cd delta = cscl(csub(a, d), 0.5), bc = cmul(bb, c);
        const cd disc = csqrtd(cadd(cmul(delta, delta), bc));
        const cd d1 = cadd(delta, disc), d2 = csub(delta, disc);
        const cd den = cabs1(d1) >= cabs1(d2) ? d1 : d2;
        mu = cabs1(den) == 0.0 ? d : csub(d, cdivd(bc, den));      // the eigenvalue of the trailing 2 x 2 nearer d
      }
    }
    ARN_SYNC();
    ARN_LANES(l) if (l >= lo && l <= ihi) T[l * ARN_LD + l] = csub(T[l * ARN_LD + l], mu);
    ARN_SYNC();
    for (int k = lo; k < ihi; ++k) {
      double c;
      cd s;
      givens(T[k * ARN_LD + k], T[(k + 1) * ARN_LD + k], c, s);
      ARN_SYNC();
      ARN_LANES(q) if (q >= k && q < m) {
        const cd x = T[k * ARN_LD + q], y = T[(k + 1) * ARN_LD + q];
        T[k * ARN_LD + q] = cadd(cscl(x, c), cmul(s, y));
        T[(k + 1) * ARN_LD + q] = q == k ? cmk(0.0, 0.0) : csub(cscl(y, c), cmulc(s, x));
        if (q == k) {
          rowa[k] = c;
          vv[k] = s;
        }
      }
      ARN_SYNC();
    }
    ARN_LANES(i) if (i < m) {
      for (int k = lo; k < ihi; ++k) {
        const double c = rowa[k];
        const cd s = vv[k];
        if (i <= k + 1) {
          const cd x = T[i * ARN_LD + k], y = T[i * ARN_LD + k + 1];
          T[i * ARN_LD + k] = cadd(cscl(x, c), cmulc(s, y));
          T[i * ARN_LD + k + 1] = csub(cscl(y, c), cmul(x, s));
        }
        const cd x = Z[i * ARN_LD + k], y = Z[i * ARN_LD + k + 1];
        Z[i * ARN_LD + k] = cadd(cscl(x, c), cmulc(s, y));
        Z[i * ARN_LD + k + 1] = csub(cscl(y, c), cmul(x, s));
      }
    }
    ARN_SYNC();
    ARN_LANES(l) if (l >= lo && l <= ihi) T[l * ARN_LD + l] = cadd(T[l * ARN_LD + l], mu);
    ARN_SYNC();
  }
  if (qr_fail) {
    ARN_LANES(l) if (l == 0) {
      st[0] = 0; st[1] = total; st[2] = ARN_FLAG_QR_LIMIT; st[3] = 0; st[4] = brkcode; st[5] = 0; st[6] = 0; st[7] = 0;
    }
    return;
  }

  // ---- 4. ranking.  Real operator: an eigenvalue and the nearest one of opposite imaginary part, if it is its
  // conjugate to 1e-6 relative, are partners: they share the larger key and the smaller index as tie-breaker
  ARN_LANES(l) if (l < m) {
    lam[l] = T[l * ARN_LD + l];
    partner[l] = -1;
  }
  ARN_SYNC();
  if (!CPLX) {
    ARN_LANES(l) if (l == 0) {
      for (int i = 0; i < m; ++i) {
        if (partner[i] >= 0 || lam[i].im == 0.0) continue;
        int best = -1;
        double bd = 0.0;
        for (int j = 0; j < m; ++j) {
          if (j == i || partner[j] >= 0 || !(lam[j].im * lam[i].im < 0.0)) continue;
          const double d = cabs2(csub(lam[j], cconj(lam[i])));
          if (best < 0 || d < bd) {
            best = j;
            bd = d;
          }
        }
        if (best >= 0 && bd <= 1e-6 * fmax(cabs2(lam[i]), cabs2(lam[best]))) {
          partner[i] = best;
          partner[best] = i;
        }
      }
    }
    ARN_SYNC();
  }
  ARN_LANES(l) if (l < m) {
    double kv = rank_key(lam[l], which);
    if (partner[l] >= 0) kv = fmax(kv, rank_key(lam[partner[l]], which));
    key[l] = kv;
  }
  ARN_SYNC();
  ARN_LANES(i) if (i < m) {
    const int li = partner[i] >= 0 && partner[i] < i ? partner[i] : i;
    int r = 0;
    for (int j = 0; j < m; ++j) {
      if (j == i) continue;
      const int lj = partner[j] >= 0 && partner[j] < j ? partner[j] : j;
      bool before;
      if (key[j] != key[i]) before = key[j] > key[i];
      else if (lj != li) before = lj < li;
      else if (lam[j].im != lam[i].im) before = lam[j].im > lam[i].im;
      else before = j < i;
      r += before ? 1 : 0;
    }
    rk[i] = r;
    posrk[i] = r;
  }
  ARN_SYNC();
  ARN_LANES(i) if (i < m) qcol[rk[i]] = i;                           // (qcol as the inverse permutation, for the cut)
  ARN_SYNC();
  int kp = keep + (keep_add ? keep_add[b] : 0), flags = 0;
  if (kp > m - 1) kp = m - 1;
  if (!CPLX) {
    if (partner[qcol[kp - 1]] == qcol[kp]) ++kp;                     // the cut separates partners
    if (kp > m - 1) {
      kp = m - 1;
      if (partner[qcol[kp - 1]] == qcol[kp]) --kp;
    }
  }
  if (kp != keep) flags |= ARN_FLAG_KEEP_MOVED;
  ARN_SYNC();

  // ---- 5. reordering: the eigenvalue of rank p to position p, p < keep', by adjacent swaps
  for (int p = 0; p < kp; ++p) {
    int c = p;
    while (c < m && posrk[c] != p) ++c;
    for (int k = c - 1; k >= p; --k) {
      const cd a = T[k * ARN_LD + k], bb = T[(k + 1) * ARN_LD + k + 1], x = T[k * ARN_LD + k + 1];
      const cd y = csub(bb, a);
      const double r = hypot(cabs2(x), cabs2(y));
      ARN_SYNC();
      if (r > 0.0) {
        const double ir = 1.0 / r;
        const cd g11 = cscl(x, ir), g21 = cscl(y, ir), g12 = cscl(cconj(y), -ir), g22 = cscl(cconj(x), ir);
        ARN_LANES(q) if (q >= k && q < m) {
          const cd tk = T[k * ARN_LD + q], tk1 = T[(k + 1) * ARN_LD + q];
          T[k * ARN_LD + q] = cadd(cmulc(g11, tk), cmulc(g21, tk1));
          T[(k + 1) * ARN_LD + q] = cadd(cmulc(g12, tk), cmulc(g22, tk1));
        }
        ARN_SYNC();
        ARN_LANES(i) if (i < m) {
          if (i <= k + 1) {
            const cd tk = T[i * ARN_LD + k], tk1 = T[i * ARN_LD + k + 1];
            T[i * ARN_LD + k] = cadd(cmul(tk, g11), cmul(tk1, g21));
            T[i * ARN_LD + k + 1] = cadd(cmul(tk, g12), cmul(tk1, g22));
          }
          const cd zk = Z[i * ARN_LD + k], zk1 = Z[i * ARN_LD + k + 1];
          Z[i * ARN_LD + k] = cadd(cmul(zk, g11), cmul(zk1, g21));
          Z[i * ARN_LD + k + 1] = cadd(cmul(zk, g12), cmul(zk1, g22));
        }
        ARN_SYNC();
      }
      ARN_LANES(l) if (l == 0) {
        T[(k + 1) * ARN_LD + k] = cmk(0.0, 0.0);
        const int t = posrk[k];
        posrk[k] = posrk[k + 1];
        posrk[k + 1] = t;
      }
      ARN_SYNC();
    }
  }
  double* thb = theta + (long)b * m * 2;
  ARN_LANES(l) if (l < m) {
    const cd v = cscl(T[l * ARN_LD + l], isc);
    thb[2 * posrk[l]] = v.re;
    thb[2 * posrk[l] + 1] = v.im;
  }

  // ---- 6. Ritz vectors of the leading neig eigenvalues (lane i: eigenvalue i), residual estimates, convergence
  const double smin = fmax(EPS * fro, DBL_MIN);
  const double nbeta = cabs2(beta);
  double* Yb = Y + (long)b * m * neig * 2;
  ARN_LANES(i) if (i < neig) {
    const cd li = T[i * ARN_LD + i];
    S[i * ARN_LD + i] = cmk(1.0, 0.0);
    for (int r = i - 1; r >= 0; --r) {
      cd acc = cmk(0.0, 0.0);
      for (int c = r + 1; c <= i; ++c) acc = cadd(acc, cmul(T[r * ARN_LD + c], S[c * ARN_LD + i]));
      cd den = csub(T[r * ARN_LD + r], li);
      if (cabs1(den) < smin) den = cmk(smin, 0.0);
      S[r * ARN_LD + i] = cdivd(cmk(-acc.re, -acc.im), den);
    }
    double n2 = 0.0;
    for (int r = 0; r < m; ++r) {
      cd y = cmk(0.0, 0.0);
      for (int c = 0; c <= i; ++c) y = cadd(y, cmul(Z[r * ARN_LD + c], S[c * ARN_LD + i]));
      Yb[2 * ((long)r * neig + i)] = y.re;
      Yb[2 * ((long)r * neig + i) + 1] = y.im;
      n2 += y.re * y.re + y.im * y.im;
    }
    const double inv = 1.0 / sqrt(n2);
    cd last = cmk(0.0, 0.0);
    for (int r = 0; r < m; ++r) {
      last = cmk(Yb[2 * ((long)r * neig + i)] * inv, Yb[2 * ((long)r * neig + i) + 1] * inv);
      Yb[2 * ((long)r * neig + i)] = last.re;
      Yb[2 * ((long)r * neig + i) + 1] = last.im;
    }
    const double rs = nbeta * cabs2(last);
    res[(long)b * neig + i] = rs;
    cflag[i] = rs <= tol * fmax(cabs2(li) * isc, u * fro * isc) ? 1 : 0;
  }
  ARN_SYNC();
  int nconv = 0;
  for (int i = 0; i < neig; ++i) nconv += cflag[i];
  ARN_SYNC();

  // ---- 7. restart coefficients
  double* Qb = Q + (long)b * m * m * EL;
  double* Hn = Hnext + (long)b * (m + 1) * m * EL;
  if (CPLX) {
    ARN_LANES(j) if (j < m) {
      for (int i = 0; i < m; ++i) {
        const cd q = j < kp ? Z[i * ARN_LD + j] : cmk(0.0, 0.0);
        Qb[2 * ((long)i * m + j)] = q.re;
        Qb[2 * ((long)i * m + j) + 1] = q.im;
      }
      for (int i = 0; i <= m; ++i) {
        cd h = cmk(0.0, 0.0);
        if (j < kp && i <= j) h = cscl(T[i * ARN_LD + j], isc);
        if (j < kp && i == kp) h = cmul(beta, Z[(m - 1) * ARN_LD + j]);
        Hn[2 * ((long)i * m + j)] = h.re;
        Hn[2 * ((long)i * m + j) + 1] = h.im;
      }
    }
  } else {
    double* Sr = reinterpret_cast<double*>(S);
    double* Tr = reinterpret_cast<double*>(T);
    double* Wr = reinterpret_cast<double*>(Z);
    const int ncol = 2 * kp;
    ARN_SYNC();
    ARN_LANES(i) {
      if (i < m)
        for (int c = 0; c < kp; ++c) {
          Sr[i * ARN_LDR + c] = Z[i * ARN_LD + c].re;
          Sr[i * ARN_LDR + kp + c] = Z[i * ARN_LD + c].im;
        }
      used[i] = 0;
      if (i + 64 < 2 * ARN_MAX_ROWS) used[i + 64] = 0;
    }
    ARN_SYNC();
    int nq = 0;
    for (int c = 0; c <= kp; ++c) {                                // (the last round only measures what is left)
      ARN_LANES(l) {
        for (int col = l; col < ncol; col += 64) {
          double n2 = -1.0;
          if (!used[col]) {
            n2 = 0.0;
            for (int i = 0; i < m; ++i) n2 += Sr[i * ARN_LDR + col] * Sr[i * ARN_LDR + col];
          }
          cn[col] = n2;
        }
      }
      ARN_SYNC();
      int p = 0;
      for (int col = 1; col < ncol; ++col)
        if (cn[col] > cn[p]) p = col;
      const double pn2 = ncol > 0 ? cn[p] : 0.0;                   // (keep' = 0: there are no columns)
      ARN_SYNC();
      if (c == kp) {
        if (pn2 > 1e-16) flags |= ARN_FLAG_NOT_CLOSED;             // a column longer than 1e-8 is left: not closed
        break;
      }
      if (!(pn2 > 1e-28)) {                                        // (cannot happen for kp independent columns)
        flags |= ARN_FLAG_NOT_CLOSED;
        break;
      }
      const double ipn = 1.0 / sqrt(pn2);
      ARN_LANES(i) {
        if (i < m) Sr[i * ARN_LDR + p] *= ipn;
        if (i == 0) {
          used[p] = 1;
          qcol[c] = p;
        }
      }
      ARN_SYNC();
      ARN_LANES(l) {
        for (int col = l; col < ncol; col += 64) {
          if (used[col]) continue;
          for (int pass = 0; pass < 2; ++pass) {
            double d = 0.0;
            for (int i = 0; i < m; ++i) d += Sr[i * ARN_LDR + p] * Sr[i * ARN_LDR + col];
            for (int i = 0; i < m; ++i) Sr[i * ARN_LDR + col] -= d * Sr[i * ARN_LDR + p];
          }
        }
      }
      ARN_SYNC();
      nq = c + 1;
    }
    // Hnext = Q^T B Q from the scaled B (reloaded into T's storage), W = B Q into Z's storage
    ARN_LANES(i) if (i < m)
      for (int c = 0; c < m; ++c) Tr[i * ARN_LDR + c] = Hb[(long)i * m + c] * sc;
    ARN_SYNC();
    ARN_LANES(j) if (j < nq) {
      const int col = qcol[j];
      for (int i = 0; i < m; ++i) {
        double w = 0.0;
        for (int k = 0; k < m; ++k) w += Tr[i * ARN_LDR + k] * Sr[k * ARN_LDR + col];
        Wr[i * ARN_LDR + j] = w;
      }
    }
    ARN_SYNC();
    ARN_LANES(j) if (j < m) {
      for (int i = 0; i < m; ++i) Qb[(long)i * m + j] = j < nq ? Sr[i * ARN_LDR + qcol[j]] : 0.0;
      for (int a = 0; a <= m; ++a) {
        double h = 0.0;
        if (j < nq && a < nq) {
          const int col = qcol[a];
          for (int i = 0; i < m; ++i) h += Sr[i * ARN_LDR + col] * Wr[i * ARN_LDR + j];
          h *= isc;
        }
        if (j < nq && a == kp) h = beta.re * Sr[(m - 1) * ARN_LDR + qcol[j]];
        Hn[(long)a * m + j] = h;
      }
    }
  }
  ARN_LANES(l) if (l == 0) {
    st[0] = nconv; st[1] = total; st[2] = flags; st[3] = kp; st[4] = brkcode; st[5] = 0; st[6] = 0; st[7] = 0;
  }
}

#ifndef XK_ARN_HOST
__global__ __launch_bounds__(256) void arn_finish_kernel(
    const double* __restrict__ part, int nval, int nchunk, double* __restrict__ coef, long sC, double* __restrict__ nrm,
    double* __restrict__ rnrm, double* hcol, long sHb, long sHr, int cplx, int accumulate, double* dst, long sdst,
    double* smax, double u, int* brk, int code) {
  const int b = blockIdx.x;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const double* pb = part + (long)b * nval * nchunk;
  for (int r = wv; r < nval; r += 4) {             // (wave-uniform; the sums are those of xk_gkl_finish, bit for bit)
    double s = 0.0;
    for (int c = lane; c < nchunk; c += 64) s += pb[(long)r * nchunk + c];
    s = wave_sum(s);
    if (lane != 0) continue;
    if (r < nval - 1) {
      if (coef) coef[(long)b * sC + r] = s;
      if (hcol) {
        double* h = hcol + (long)b * sHb + (cplx ? (long)(r >> 1) * sHr + (r & 1) : (long)r * sHr);
        *h = accumulate ? *h + s : s;
      }
      continue;
    }
    double norm = sqrt(s > 0.0 ? s : 0.0);
    const double big = smax ? smax[b] : 0.0;
    const bool bad = !(s == s) || !(norm > u * big) || !(norm <= DBL_MAX);
    if (bad) {
      if (brk && brk[b] < 0) brk[b] = code;
      nrm[b] = 0.0;
      rnrm[b] = 0.0;
      norm = 0.0;
    } else {
      nrm[b] = norm;
      rnrm[b] = 1.0 / norm;
      if (smax && norm > big) smax[b] = norm;
    }
    if (dst) dst[(long)b * sdst] = norm;
  }
}
#endif

}  // namespace xk

#ifndef XK_ARN_HOST
extern "C" {

int xk_arn_max_rows(void) { return xk::ARN_MAX_ROWS; }
int xk_arn_status_words(void) { return xk::ARN_STATUS; }

int xk_arn_finish(const double* part, int Bt, int nval, int nchunk, double* coef, long sC, double* nrm, double* rnrm,
                  double* hcol, long sHb, long sHr, int cplx, int accumulate, double* dst, long sdst, double* smax,
                  double u, int* brk, int code, void* stream) {
  const int rc = xk::arn_finish_check(part, Bt, nval, nchunk, coef, sC, nrm, rnrm, hcol, sHb, sHr, cplx, accumulate,
                                      sdst, u);
  if (rc != XK_OK) return rc;
  hipLaunchKernelGGL(xk::arn_finish_kernel, dim3((unsigned)Bt), dim3(256), 0, (hipStream_t)stream, part, nval, nchunk,
                     coef, sC, nrm, rnrm, hcol, sHb, sHr, cplx, accumulate, dst, sdst, smax, u, brk, code);
  XK_LAUNCH_CHECK();
  return XK_OK;
}

int xk_arn_schur(const double* H, int Bt, int m, int neig, int keep, const int* keep_add, int which, int cplx,
                 double tol, double u, const int* brk, double* theta, double* Y, double* res, double* Q, double* Hnext,
                 int* status, void* stream) {
  const int rc = xk::arn_schur_check(H, Bt, m, neig, keep, which, cplx, tol, u, theta, Y, res, Q, Hnext, status);
  if (rc != XK_OK) return rc;
  if (cplx)
    hipLaunchKernelGGL((xk::arn_schur_kernel<true>), dim3((unsigned)Bt), dim3(64), 0, (hipStream_t)stream, H, m, neig,
                       keep, keep_add, which, tol, u, brk, theta, Y, res, Q, Hnext, status);
  else
    hipLaunchKernelGGL((xk::arn_schur_kernel<false>), dim3((unsigned)Bt), dim3(64), 0, (hipStream_t)stream, H, m, neig,
                       keep, keep_add, which, tol, u, brk, theta, Y, res, Q, Hnext, status);
  XK_LAUNCH_CHECK();
  return XK_OK;
}

}  // extern "C"
#endif
