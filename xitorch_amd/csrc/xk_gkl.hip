// xitorch_amd :: kernels of the Golub-Kahan-Lanczos bidiagonalisation with thick restart, svd(method="gkl")
// (Baglama & Reichel, SIAM J. Sci. Comput. 27 (2005) 19; full reorthogonalisation as in Larsen's PROPACK).
//
// An extension (the reference's svd goes through symeig of A^H A).  Three kernels:
//
// xk_gkl_sweep_*  — one pass of classical Gram-Schmidt of ONE new vector per batch member against j rows of a basis
//   panel Q (Bt, cap, ld) (rows are vectors).  For every member b and n < N
//
//     dst[b,n] = s_b * ( w[b,n] - sum_{i<j} c[b,i] Q[b,i,n] ),        s_b = scale ? scale[b] : 1,
//
//   (the sum is skipped when coef is null) and, from the SAME tile of Q held in registers, the partial sums over the
//   chunk of  conj(Q[b,i,:]) . dst[b,:]  (i < j)  and of  |dst[b,:]|^2.  The update is local per element, so the
//   coefficients of the previous pass are applied and those of the next pass are accumulated in one read of the basis:
//   CGS2 costs three sweeps and no temporaries.  dst may be w itself.  The tile: a workgroup of four waves owns a
//   chunk of 64 16 B vectors of the vector; wave v holds rows v, v + 4, ... (up to 16 rows = 64 VGPRs) of that chunk,
//   all of its non-temporal 16 B loads issued before the first use.  The partial updates of the four waves are added
//   through LDS in the fixed order wave 0..3 in double; the dots are reduced over the wave by the vector-ALU butterfly
//   and written as doubles part[b, r, chunk], r < nval = j (x 2 for complex: re, im) + 1 (the sum of squares).  No
//   atomics: a repeat call gives the same bits.  Lanes whose vector straddles N, and layouts that break the 16 B rule
//   (base, pitch or batch stride not a multiple of 16 B), go element by element; pads are never written.
//
// xk_gkl_finish   — adds the partials of one sweep in a fixed order (lane l takes chunks l, l + 64, ...; then the
//   butterfly), writes the coefficients for the next sweep, norm = sqrt(sum of squares) and 1 / norm, stores the norm
//   (the alpha or beta of the step) straight into the device-resident projected matrix, keeps the running maximum of
//   the norms (a lower estimate of sigma_max) and flags a breakdown — norm <= u * that maximum, or not a number — by
//   writing the step code into brk[b] (first breakdown of the cycle only); a broken-down member gets norm = 1/norm = 0.
//
// xk_gkl_bsvd     — SVD of the projected matrices (Bt, n, n), n <= 64, real for all dtypes, in double: one-sided
//   (Hestenes) Jacobi on the columns in LDS, one workgroup per member, 32 disjoint column pairs per round (8 lanes a
//   pair), round-robin ordering; columns no longer than eps |B|_F are null columns and are not rotated.  It never forms
//   B^T B.  LDS: W and V, 2 * 64 * 64 * 8 B = 64 KiB, plus < 1 KiB of
//   bookkeeping; a workgroup may declare up to 160 KiB on gfx950, so two workgroups fit a CU.  Epilogue: null columns
//   (sigma <= n eps sigma_max) get an orthonormal completion, the triplets are sorted in the order the mode wants,
//   res[i] = |beta * P[n - 1, i]|, the status word {converged among the first k, sweeps, sweep-limit flag, breakdown
//   code} and the projected matrix of the restarted basis (diag(sigma[:keep]) plus the arrow beta * P[n - 1, :keep]).
//
// All stores are ordinary vector-memory stores.
#include "xk_common.h"
#include <float.h>

namespace xk {

constexpr int GKL_MAX_ROWS = 64;                   // rows of the basis one sweep reads
constexpr int GKL_CHUNK_VEC = 64;                  // 16 B vectors of the new vector per workgroup (one per lane)
constexpr int GKL_BSVD_MAX = 64;                   // order of the projected matrix
constexpr int GKL_BSVD_SWEEPS = 40;

template <typename T, bool CP, int RW>
__global__ __launch_bounds__(256) void gkl_sweep_kernel(
    const T* __restrict__ Q, long ldQ, long sQ, const T* w, long sW, T* dst, long sD, const double* __restrict__ coef,
    long sC, const double* __restrict__ scale, double* __restrict__ part, int j, int N, int nchunk, int vec) {
  typedef typename Vec16<T>::type VT;
  constexpr int VN = Vec16<T>::n;
  __shared__ double sacc[4][VN][64];
  const int chunk = blockIdx.x, b = blockIdx.y;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long n0 = ((long)chunk * GKL_CHUNK_VEC + lane) * VN;
  const bool full = vec && n0 + VN <= (long)N;
  const T* Qb = Q + (long)b * sQ;
  const T* wb = w + (long)b * sW;
  VT q[RW], x;
#pragma unroll
  for (int t = 0; t < RW; ++t) {
    const int row = wv + 4 * t;
    if (row < j) {
      const T* qr = Qb + (long)row * ldQ;
      if (full) {
        q[t] = ld_stream(reinterpret_cast<const VT*>(qr + n0));
      } else {
#pragma unroll
        for (int e = 0; e < VN; ++e) q[t][e] = n0 + e < (long)N ? qr[n0 + e] : T(0);
      }
    } else {
#pragma unroll
      for (int e = 0; e < VN; ++e) q[t][e] = T(0);
    }
  }
  if (full) {
    x = *reinterpret_cast<const VT*>(wb + n0);
  } else {
#pragma unroll
    for (int e = 0; e < VN; ++e) x[e] = n0 + e < (long)N ? wb[n0 + e] : T(0);
  }
  __builtin_amdgcn_sched_barrier(0);               // every load of the lane is in flight before the first use
  double xd[VN];
#pragma unroll
  for (int e = 0; e < VN; ++e) xd[e] = (double)x[e];
  __syncthreads();                                 // dst may be w: every wave holds its copy of w before wave 0 stores
  if (coef != nullptr && j > 0) {
    double acc[VN];
#pragma unroll
    for (int e = 0; e < VN; ++e) acc[e] = 0.0;
    const double* cb = coef + (long)b * sC;
#pragma unroll
    for (int t = 0; t < RW; ++t) {
      const int row = wv + 4 * t;
      if (row < j) {
        if (CP) {
          const double cr = cb[2 * row], ci = cb[2 * row + 1];
#pragma unroll
          for (int e = 0; e < VN; e += 2) {
            acc[e] += cr * (double)q[t][e] - ci * (double)q[t][e + 1];
            acc[e + 1] += cr * (double)q[t][e + 1] + ci * (double)q[t][e];
          }
        } else {
          const double c = cb[row];
#pragma unroll
          for (int e = 0; e < VN; ++e) acc[e] += c * (double)q[t][e];
        }
      }
    }
#pragma unroll
    for (int e = 0; e < VN; ++e) sacc[wv][e][lane] = acc[e];
    __syncthreads();
#pragma unroll
    for (int e = 0; e < VN; ++e) xd[e] -= ((sacc[0][e][lane] + sacc[1][e][lane]) + sacc[2][e][lane]) + sacc[3][e][lane];
  }
  const double s = scale != nullptr ? scale[b] : 1.0;
#pragma unroll
  for (int e = 0; e < VN; ++e) {
    x[e] = (T)(s * xd[e]);                         // rounded once to the storage type; the dots see what is stored
    xd[e] = (double)x[e];
  }
  double* pb = part + (long)b * (CP ? 2 * j + 1 : j + 1) * nchunk + chunk;
#pragma unroll
  for (int t = 0; t < RW; ++t) {
    const int row = wv + 4 * t;
    if (row < j) {                                 // (wave-uniform)
      if (CP) {
        double re = 0.0, im = 0.0;
#pragma unroll
        for (int e = 0; e < VN; e += 2) {
          re += (double)q[t][e] * xd[e] + (double)q[t][e + 1] * xd[e + 1];
          im += (double)q[t][e] * xd[e + 1] - (double)q[t][e + 1] * xd[e];
        }
        re = wave_sum(re);
        im = wave_sum(im);
        if (lane == 0) {
          pb[(long)(2 * row) * nchunk] = re;
          pb[(long)(2 * row + 1) * nchunk] = im;
        }
      } else {
        double d = 0.0;
#pragma unroll
        for (int e = 0; e < VN; ++e) d += (double)q[t][e] * xd[e];
        d = wave_sum(d);
        if (lane == 0) pb[(long)row * nchunk] = d;
      }
    }
  }
  if (wv == 0) {
    double ss = 0.0;
#pragma unroll
    for (int e = 0; e < VN; ++e) ss += xd[e] * xd[e];
    ss = wave_sum(ss);
    if (lane == 0) pb[(long)(CP ? 2 * j : j) * nchunk] = ss;
    T* db = dst + (long)b * sD;
    if (full) {
      *reinterpret_cast<VT*>(db + n0) = x;
    } else {
#pragma unroll
      for (int e = 0; e < VN; ++e)
        if (n0 + e < (long)N) db[n0 + e] = x[e];
    }
  }
}

// N, ldQ, sQ, sW, sD in REAL elements (the complex entry points double them); ncoef doubles per member in coef
template <typename T, bool CP>
static int gkl_sweep(const T* Q, long ldQ, long sQ, const T* w, long sW, T* dst, long sD, const double* coef, long sC,
                     const double* scale, double* part, long part_len, int Bt, int j, int N, hipStream_t st) {
  constexpr int VN = Vec16<T>::n;
  if (Bt <= 0 || Bt > 65535 || N <= 0 || j < 0 || j > GKL_MAX_ROWS || !w || !dst || !part) return XK_ERR_ARG;
  if (j > 0 && (!Q || ldQ < N || sQ < 0)) return XK_ERR_ARG;
  if (sW < 0 || sD < 0 || sC < 0) return XK_ERR_ARG;
  const int ncoef = CP ? 2 * j : j;
  if (Bt > 1 && (sD < N || (coef && sC < ncoef))) return XK_ERR_ARG;
  // dst against w and against rows [0, j) of Q.  Panels of one batch stride (the driver's: dst is a slot of the panel
  // that holds Q) interleave their members, so the footprints are compared member by member: those of member 0, both
  // inside one window of the common stride.  Any other layout: the whole address ranges must lie apart.
  auto apart = [&](const T* a, long sa, long la, const T* d, long sd, long ldn) {
    const uintptr_t alo = (uintptr_t)a, dlo = (uintptr_t)d;
    const uintptr_t aend = alo + (size_t)((long)(Bt - 1) * sa + la) * sizeof(T);
    const uintptr_t dend = dlo + (size_t)((long)(Bt - 1) * sd + ldn) * sizeof(T);
    if (!(alo < dend && dlo < aend)) return true;                    // the whole ranges lie apart
    if (Bt > 1 && sa != sd) return false;
    const uintptr_t ahi = alo + (size_t)la * sizeof(T), dhi = dlo + (size_t)ldn * sizeof(T);
    if (alo < dhi && dlo < ahi) return false;                        // the footprints of member 0 meet
    const uintptr_t lo = alo < dlo ? alo : dlo, hi = ahi > dhi ? ahi : dhi;
    return Bt == 1 || hi - lo <= (size_t)sd * sizeof(T);             // ... and fit one window of the common stride
  };
  const bool inplace = (const T*)dst == w && (sD == sW || Bt == 1);
  if (!inplace && !apart(w, sW, N, dst, sD, N)) return XK_ERR_ARG;
  if (j > 0 && !apart(Q, sQ, (long)(j - 1) * ldQ + N, dst, sD, N)) return XK_ERR_ARG;
  const long chunk_el = (long)GKL_CHUNK_VEC * VN;
  const long nchunk = ((long)N + chunk_el - 1) / chunk_el;
  if (nchunk > 0x7fffffffL || part_len < (long)Bt * (ncoef + 1) * nchunk) return XK_ERR_ARG;
  auto ok = [](const void* p, long ld, long s) { return !((uintptr_t)p & 15) && ld % VN == 0 && s % VN == 0; };
  const int vec = (j == 0 || ok(Q, ldQ, sQ)) && ok(w, 0, sW) && ok(dst, 0, sD);
  const dim3 grid((unsigned)nchunk, (unsigned)Bt);
  if (j <= 16)
    hipLaunchKernelGGL((gkl_sweep_kernel<T, CP, 4>), grid, dim3(256), 0, st, Q, ldQ, sQ, w, sW, dst, sD, coef, sC,
                       scale, part, j, N, (int)nchunk, vec);
  else
    hipLaunchKernelGGL((gkl_sweep_kernel<T, CP, 16>), grid, dim3(256), 0, st, Q, ldQ, sQ, w, sW, dst, sD, coef, sC,
                       scale, part, j, N, (int)nchunk, vec);
  XK_LAUNCH_CHECK();
  return XK_OK;
}

__global__ __launch_bounds__(256) void gkl_finish_kernel(
    const double* __restrict__ part, int nval, int nchunk, double* __restrict__ coef, long sC, double* __restrict__ nrm,
    double* __restrict__ rnrm, double* dst, long sdst, double* smax, double u, int* brk, int code) {
  const int b = blockIdx.x;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const double* pb = part + (long)b * nval * nchunk;
  for (int r = wv; r < nval; r += 4) {             // (wave-uniform)
    double s = 0.0;
    for (int c = lane; c < nchunk; c += 64) s += pb[(long)r * nchunk + c];
    s = wave_sum(s);
    if (lane != 0) continue;
    if (r < nval - 1) {
      if (coef) coef[(long)b * sC + r] = s;
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

__global__ __launch_bounds__(256) void gkl_bsvd_kernel(
    const double* __restrict__ Bm, const double* __restrict__ beta, const double* __restrict__ smax_in,
    const int* __restrict__ brk, int n, int k, int keep, int descending, double tol, double* __restrict__ sigma,
    double* __restrict__ P, double* __restrict__ Qo, double* __restrict__ res, int* __restrict__ status,
    double* __restrict__ Bnext) {
  __shared__ double W[GKL_BSVD_MAX * GKL_BSVD_MAX], V[GKL_BSVD_MAX * GKL_BSVD_MAX];
  __shared__ double sg[GKL_BSVD_MAX];
  __shared__ int rnk[GKL_BSVD_MAX], nul[GKL_BSVD_MAX];
  __shared__ int s_rot, s_conv;
  const int b = blockIdx.x, tid = threadIdx.x;
  const double* Bb = Bm + (long)b * n * n;
  for (int idx = tid; idx < n * n; idx += 256) {
    const int r = idx / n, c = idx - r * n;
    W[c * n + r] = Bb[idx];                        // column-major: a column is a contiguous run
    V[c * n + r] = r == c ? 1.0 : 0.0;
  }
  if (tid == 0) s_conv = 0;
  __syncthreads();
  // columns no longer than eps |B|_F are null columns (below the n eps sigma_max of the epilogue, which replaces their
  // left vectors by the completion) and are left alone: in a rank-deficient B with zero rows such a column is rounding
  // noise inside the span of the others, never orthogonal to them relative to its own length; chasing it shrinks it by
  // about eps per sweep until its squared norm underflows and every later rotation is the identity
  if (tid < n) {
    double s = 0.0;
    for (int i = 0; i < n; ++i) s += W[tid * n + i] * W[tid * n + i];
    sg[tid] = s;
  }
  __syncthreads();
  double fro2 = 0.0;
  for (int i = 0; i < n; ++i) fro2 += sg[i];
  const double dnull = DBL_EPSILON * sqrt(fro2);
  __syncthreads();
  const int m = n + (n & 1);
  const int g = tid >> 3, l = tid & 7;
  const double tolj = sqrt((double)n) * DBL_EPSILON;
  int sweeps = 0, hit_limit = 1;
  while (sweeps < GKL_BSVD_SWEEPS) {
    if (tid == 0) s_rot = 0;
    __syncthreads();
    bool rotated = false;
    for (int r = 0; r < m - 1; ++r) {
      int p = 0, q = 0;
      bool valid = false;
      if (g < m / 2) {
        p = (r + g) % (m - 1);
        q = g == 0 ? m - 1 : (r + (m - 1) - g) % (m - 1);
        if (p > q) {
          const int t = p;
          p = q;
          q = t;
        }
        valid = q < n;
      }
      double a = 0.0, d = 0.0, c = 0.0;
      if (valid)
        for (int i = l; i < n; i += 8) {
          const double wp = W[p * n + i], wq = W[q * n + i];
          a += wp * wp;
          d += wq * wq;
          c += wp * wq;
        }
#pragma unroll
      for (int msk = 1; msk <= 4; msk <<= 1) {
        a += shfl_xor_t(a, msk);
        d += shfl_xor_t(d, msk);
        c += shfl_xor_t(c, msk);
      }
      const double sa = sqrt(a), sd = sqrt(d);
      double t = 0.0;
      if (valid && c != 0.0 && sa > dnull && sd > dnull && fabs(c) > tolj * sa * sd) {
        const double zeta = (d - a) / (2.0 * c);
        t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
      }
      if (t != 0.0) {                              // (t == 0: the rotation is the identity, nothing left to do)
        rotated = true;
        const double cs = 1.0 / sqrt(1.0 + t * t), sn = cs * t;
        for (int i = l; i < n; i += 8) {
          const double wp = W[p * n + i], wq = W[q * n + i];
          W[p * n + i] = cs * wp - sn * wq;
          W[q * n + i] = sn * wp + cs * wq;
          const double vp = V[p * n + i], vq = V[q * n + i];
          V[p * n + i] = cs * vp - sn * vq;
          V[q * n + i] = sn * vp + cs * vq;
        }
      }
      __syncthreads();
    }
    ++sweeps;
    if (rotated) atomicOr(&s_rot, 1);
    __syncthreads();
    const int any = s_rot;
    __syncthreads();
    if (!any) {
      hit_limit = 0;
      break;
    }
  }
  // singular values, null columns, normalisation of the left vectors
  if (tid < n) {
    double s = 0.0;
    for (int i = 0; i < n; ++i) s += W[tid * n + i] * W[tid * n + i];
    sg[tid] = sqrt(s);
  }
  __syncthreads();
  double smax = 0.0;
  for (int i = 0; i < n; ++i) smax = sg[i] > smax ? sg[i] : smax;
  if (tid < n) {
    const int isnull = !(sg[tid] > (double)n * DBL_EPSILON * smax);
    nul[tid] = isnull;
    const double inv = isnull ? 0.0 : 1.0 / sg[tid];
    for (int i = 0; i < n; ++i) W[tid * n + i] *= inv;
  }
  __syncthreads();
  // orthonormal completion of the null columns: unit vectors, two Gram-Schmidt passes against the columns in place
  // (wave 0; lane = row, so a lane reads and writes its own row only and the sums are bit-identical on all lanes)
  if (tid < 64) {
    const bool inr = tid < n;
    for (int i = 0; i < n; ++i) {
      if (!nul[i]) continue;                       // (uniform: nul is not written in this loop)
      for (int cand = 0; cand < n; ++cand) {
        double x = (inr && tid == cand) ? 1.0 : 0.0;
        for (int pass = 0; pass < 2; ++pass)
          for (int c = 0; c < n; ++c) {
            if (c == i || (nul[c] && c > i)) continue;
            const double wc = inr ? W[c * n + tid] : 0.0;
            const double dd = wave_sum(wc * x);
            x -= dd * wc;
          }
        const double nr = sqrt(wave_sum(x * x));
        // (with r columns in place the best unit vector keeps (n - r) / n >= 1 / n of its squared length)
        if (nr * nr * 2.0 * (double)n >= 1.0) {
          if (inr) W[i * n + tid] = x / nr;
          break;
        }
      }
    }
  }
  __syncthreads();
  if (tid < n) {
    const double si = sg[tid];
    int rk = 0;
    for (int i = 0; i < n; ++i) {
      const double sj = sg[i];
      const bool before = descending ? (sj > si || (sj == si && i < tid)) : (sj < si || (sj == si && i < tid));
      rk += before ? 1 : 0;
    }
    rnk[tid] = rk;
  }
  __syncthreads();
  const double big_in = smax_in ? smax_in[b] : 0.0;
  const double scale = smax > big_in ? smax : big_in;
  const double bt = beta ? beta[b] : 0.0;
  for (int idx = tid; idx < n * n; idx += 256) {
    const int c = idx / n, r = idx - c * n;
    P[(long)b * n * n + (long)r * n + rnk[c]] = W[c * n + r];
    Qo[(long)b * n * n + (long)r * n + rnk[c]] = V[c * n + r];
    if (Bnext) Bnext[(long)b * n * n + idx] = 0.0;
  }
  __syncthreads();                                 // (Bnext is zero before the entries below are written)
  if (tid < n) {
    const int rk = rnk[tid];
    const double rho = bt * W[tid * n + n - 1];
    sigma[(long)b * n + rk] = sg[tid];
    res[(long)b * n + rk] = fabs(rho);
    if (rk < k && fabs(rho) <= tol * scale) atomicAdd(&s_conv, 1);
    if (Bnext && rk < keep) {
      Bnext[(long)b * n * n + (long)rk * n + rk] = sg[tid];
      if (keep < n) Bnext[(long)b * n * n + (long)rk * n + keep] = rho;
    }
  }
  __syncthreads();
  if (tid == 0) {
    status[4 * b + 0] = s_conv;
    status[4 * b + 1] = sweeps;
    status[4 * b + 2] = hit_limit;
    status[4 * b + 3] = brk ? brk[b] : -1;
  }
}

}  // namespace xk

extern "C" {

int xk_gkl_max_rows(void) { return xk::GKL_MAX_ROWS; }
int xk_gkl_bsvd_max(void) { return xk::GKL_BSVD_MAX; }
// elements (of the entry point's own element type) of one chunk of the new vector
int xk_gkl_chunk_elems(int elem_bytes) {
  if (elem_bytes != 4 && elem_bytes != 8 && elem_bytes != 16) return XK_ERR_ARG;
  return xk::GKL_CHUNK_VEC * 16 / elem_bytes;
}

// MUL = 1: real vectors;  MUL = 2: interleaved complex ones (N, pitches and strides in complex elements)
#define XK_DEFINE_GKL(SUF, T, CP, MUL)                                                                               \
  int xk_gkl_sweep_##SUF(const T* Q, long ldQ, long sQ, const T* w, long sW, T* dst, long sD, const double* coef,    \
                         long sC, const double* scale, double* part, long part_len, int Bt, int j, int N,           \
                         void* stream) {                                                                             \
    if (N <= 0 || N > 0x7fffffff / MUL) return XK_ERR_ARG;                                                           \
    return xk::gkl_sweep<T, CP>(Q, ldQ * MUL, sQ * MUL, w, sW * MUL, dst, sD * MUL, coef, sC, scale, part, part_len, \
                                Bt, j, N * MUL, (hipStream_t)stream);                                                \
  }

XK_DEFINE_GKL(f64, double, false, 1)
XK_DEFINE_GKL(f32, float, false, 1)
XK_DEFINE_GKL(c128, double, true, 2)
XK_DEFINE_GKL(c64, float, true, 2)

int xk_gkl_finish(const double* part, int Bt, int nval, int nchunk, double* coef, long sC, double* nrm, double* rnrm,
                  double* dst, long sdst, double* smax, double u, int* brk, int code, void* stream) {
  if (Bt <= 0 || nval <= 0 || nchunk <= 0 || !part || !nrm || !rnrm || sC < 0 || sdst < 0 || !(u >= 0.0)) return XK_ERR_ARG;
  if (nval > 2 * xk::GKL_MAX_ROWS + 1 || (Bt > 1 && coef && sC < nval - 1)) return XK_ERR_ARG;
  hipLaunchKernelGGL(xk::gkl_finish_kernel, dim3((unsigned)Bt), dim3(256), 0, (hipStream_t)stream, part, nval, nchunk,
                     coef, sC, nrm, rnrm, dst, sdst, smax, u, brk, code);
  XK_LAUNCH_CHECK();
  return XK_OK;
}

int xk_gkl_bsvd(const double* Bm, const double* beta, const double* smax, const int* brk, int Bt, int n, int k,
                int keep, int descending, double tol, double* sigma, double* P, double* Q, double* res, int* status,
                double* Bnext, void* stream) {
  if (Bt <= 0 || n <= 0 || n > xk::GKL_BSVD_MAX || k < 0 || k > n || keep < 0 || keep > n || !(tol >= 0.0))
    return XK_ERR_ARG;
  if (!Bm || !sigma || !P || !Q || !res || !status) return XK_ERR_ARG;
  if (Bnext && (Bnext == Bm || keep >= n)) return XK_ERR_ARG;
  hipLaunchKernelGGL(xk::gkl_bsvd_kernel, dim3((unsigned)Bt), dim3(256), 0, (hipStream_t)stream, Bm, beta, smax, brk, n,
                     k, keep, descending ? 1 : 0, tol, sigma, P, Q, res, status, Bnext);
  XK_LAUNCH_CHECK();
  return XK_OK;
}

}  // extern "C"
