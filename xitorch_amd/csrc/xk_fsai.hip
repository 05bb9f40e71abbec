// xitorch_amd :: factorised sparse approximate inverse (FSAI) of a Hermitian CSR operator: the build of G.
//
//   xk_fsai_build   row i of G on its columns S_i (sorted, i last, m = |S_i| <= 32):
//                     A_JJ = A[S_i, S_i] = L L^H,  L^H z = e_m,  G[i, S_i] = conj(z)
//                   so that diag(G A G^H) = 1 and (G A)[i, j] = 0 for j in S_i, j != i  (DESIGN.md §3.11).
//
// Work distribution.  One wavefront per (row, batch member), four per workgroup; the members of one row are
// neighbouring waves, so they re-read the row's indices right after one another.  The rows are independent: no wave
// reads what another one writes, there is no workgroup barrier anywhere (a wave whose index is past the last row
// leaves at once, and m differs from wave to wave), and every loop runs to a count read before it starts
// (m <= 32, or a row length of A clipped to the stored entry count).
//
//   gather     for local row r the wave walks the stored entries of row S_i[r] of A in storage order, 64 at a time
//              (one coalesced load, then one lane broadcast per entry); lane c <= r adds an entry to A_JJ[r, c] when
//              its column is S_i[c].  S_i is sorted, so these are entries of A's LOWER triangle only: whatever is
//              stored above the diagonal is never matched.  Duplicates add up in storage order, entries of
//              S_i x S_i that A does not store stay zero, the imaginary part of a diagonal entry is dropped.
//   Cholesky   left-looking, lane r owns row r of the packed lower triangle in wave-private LDS (528 elements per
//              wave: 33.8 KB per workgroup for complex128); column k: s_r = A[r,k] - sum_{t<k} L[r,t] conj(L[k,t]),
//              pivot d = s_k (broadcast), L[k,k] = sqrt(d), L[r,k] = s_r / L[k,k].
//   solve      L^H z = e_m column by column from the last: z_t = acc_t / L[t,t], acc_c -= conj(L[t,c]) z_t (c < t).
//
// Fallback.  A pivot that is <= 0 or not finite (a NaN anywhere in A_JJ ends in one), or a z that is not finite,
// makes the row the Jacobi row: G[i,i] = 1 / sqrt(|a_ii|), or 1 when a_ii is 0 or not finite, zeros elsewhere, and
// one integer atomicAdd on nfail[member].  All sums have a fixed order, all stores are plain vector stores: the
// result is bit-identical from run to run.
#include "xk_fsai_el.h"

namespace xk {

constexpr int FSAI_MAX = 32;                                   // longest row of G
constexpr int FSAI_TRI = FSAI_MAX * (FSAI_MAX + 1) / 2;        // packed lower triangle, elements
constexpr int FSAI_WAVES = 4;                                  // waves (rows) per workgroup

__device__ __forceinline__ int fsai_tri(int r) { return r * (r + 1) / 2; }

template <typename E>
__global__ __launch_bounds__(64 * FSAI_WAVES) void fsai_build_kernel(
    const int* __restrict__ a_ptr, const int* __restrict__ a_idx, const E* __restrict__ a_val, long sV, int a_nnz,
    const int* __restrict__ g_ptr, const int* __restrict__ g_idx, E* __restrict__ g_val, long sG, int g_nnz,
    int* __restrict__ nfail, int N, int B) {
  typedef FsaiEl<E> X;
  typedef typename X::real R;
  __shared__ E tri[FSAI_WAVES][FSAI_TRI];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long w = (long)blockIdx.x * FSAI_WAVES + wv;
  if (w >= (long)N * B) return;                     // the whole wave leaves; nothing below waits for another wave
  const int row = (int)(w / B), b = (int)(w % B);
  E* L = tri[wv];
  const int g0 = g_ptr[row];
  const int m = g_ptr[row + 1] - g0;
  if (g0 < 0 || m < 1 || m > FSAI_MAX || (long)g0 + m > g_nnz) {
    // not a row this kernel serves (the caller checks the pattern once): nothing is read or written, it is counted
    if (lane == 0) atomicAdd(nfail + b, 1);
    return;
  }
  const E* Ab = a_val + (long)b * sV;
  E* Gb = g_val + (long)b * sG + g0;
  const int sc = lane < m ? g_idx[g0 + lane] : -1;             // lane c holds S_i[c]

  // ---- gather the lower triangle of A_JJ, row by row
  R aii = R(0);
  for (int r = 0; r < m; ++r) {
    const int j = __shfl(sc, r, 64);
    int k0 = 0, k1 = 0;
    if (j >= 0 && j < N) {
      k0 = a_ptr[j];
      k1 = a_ptr[j + 1];
    }
    if (k0 < 0) k0 = 0;
    if (k1 > a_nnz) k1 = a_nnz;
    E acc = X::zero();
    for (int kb = k0; kb < k1; kb += 64) {
      const int k = kb + lane;
      int myc = -1;
      E myv = X::zero();
      if (k < k1) {
        myc = a_idx[k];
        myv = Ab[k];
      }
      const int n = (k1 - kb) < 64 ? (k1 - kb) : 64;
      for (int t = 0; t < n; ++t) {
        const int col = __shfl(myc, t, 64);
        const E v = X::bcast(myv, t);
        if (lane <= r && col == sc) acc = X::add(acc, v);
      }
    }
    if (lane == r) acc = X::from_re(X::re(acc));               // a diagonal entry counts with its real part
    if (lane <= r) L[fsai_tri(r) + lane] = acc;
    if (r == m - 1) aii = __shfl(X::re(acc), m - 1, 64);
  }

  // ---- Cholesky A_JJ = L L^H in place, column by column
  bool fail = false;
  for (int k = 0; k < m; ++k) {
    fsai_wave_sync();
    E s = X::zero();
    if (lane >= k && lane < m) {
      const E* Lr = L + fsai_tri(lane);
      const E* Lk = L + fsai_tri(k);
      s = Lr[k];
      for (int t = 0; t < k; ++t) s = X::msub(s, Lr[t], Lk[t]);
    }
    const R d = __shfl(X::re(s), k, 64);
    if (!(d > R(0)) || !isfinite(d)) {                         // the same d in every lane: the wave leaves together
      fail = true;
      break;
    }
    const R piv = sqrt(d);
    if (lane == k) L[fsai_tri(k) + k] = X::from_re(piv);
    else if (lane > k && lane < m) L[fsai_tri(lane) + k] = X::div_re(s, piv);
  }

  // ---- L^H z = e_m
  E z = X::zero();
  if (!fail) {
    fsai_wave_sync();
    E acc = lane == m - 1 ? X::from_re(R(1)) : X::zero();
    for (int t = m - 1; t >= 0; --t) {
      E zt = X::zero();
      if (lane == t) {
        z = X::div_re(acc, X::re(L[fsai_tri(t) + t]));
        zt = z;
      }
      zt = X::bcast(zt, t);
      if (lane < t) acc = X::msub(acc, zt, L[fsai_tri(t) + lane]);
    }
    if (__ballot(lane < m && !X::finite(z)) != 0ull) fail = true;
  }

  if (!fail) {
    if (lane < m) Gb[lane] = lane == m - 1 ? X::from_re(X::re(z)) : X::conj(z);
    return;
  }
  const R a = fabs(aii);
  const R gd = (a > R(0) && isfinite(a)) ? R(1) / sqrt(a) : R(1);
  if (lane < m) Gb[lane] = lane == m - 1 ? X::from_re(gd) : X::zero();
  if (lane == 0) atomicAdd(nfail + b, 1);
}

template <typename E>
static int fsai_build(const int* a_ptr, const int* a_idx, const void* a_val, long sV, int a_nnz, const int* g_ptr,
                      const int* g_idx, void* g_val, long sG, int g_nnz, int* nfail, int N, int B, hipStream_t st) {
  if (!a_ptr || !a_idx || !a_val || !g_ptr || !g_idx || !g_val || !nfail) return XK_ERR_ARG;
  if (N <= 0 || B <= 0 || sV < 0 || sG < 0 || a_nnz < 0 || g_nnz < N) return XK_ERR_ARG;
  if (B > 1 && (sG < g_nnz || (sV != 0 && sV < a_nnz))) return XK_ERR_ARG;      // members overlap
  // G must not be written over the values it is built from
  const uintptr_t a0 = (uintptr_t)a_val, a1 = a0 + sizeof(E) * (size_t)((long)(B - 1) * sV + a_nnz);
  const uintptr_t g0 = (uintptr_t)g_val, g1 = g0 + sizeof(E) * (size_t)((long)(B - 1) * sG + g_nnz);
  if (g0 < a1 && a0 < g1) return XK_ERR_ARG;
  const long nblk = ((long)N * B + FSAI_WAVES - 1) / FSAI_WAVES;
  if (nblk > 0x7fffffffL) return XK_ERR_UNSUPPORTED;
  hipError_t e = hipMemsetAsync(nfail, 0, sizeof(int) * (size_t)B, st);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL((fsai_build_kernel<E>), dim3((unsigned)nblk), dim3(64 * FSAI_WAVES), 0, st, a_ptr, a_idx,
                     (const E*)a_val, sV, a_nnz, g_ptr, g_idx, (E*)g_val, sG, g_nnz, nfail, N, B);
  XK_LAUNCH_CHECK();
  return XK_OK;
}

}  // namespace xk

extern "C" {

int xk_fsai_max_row(void) { return xk::FSAI_MAX; }

#define XK_DEFINE_FSAI(SUF, T, E)                                                                                \
  int xk_fsai_build_##SUF(const int* a_ptr, const int* a_idx, const T* a_val, long sV, int a_nnz,                \
                          const int* g_ptr, const int* g_idx, T* g_val, long sG, int g_nnz, int* nfail, int N,   \
                          int B, void* stream) {                                                                 \
    return xk::fsai_build<E>(a_ptr, a_idx, a_val, sV, a_nnz, g_ptr, g_idx, g_val, sG, g_nnz, nfail, N, B,        \
                             (hipStream_t)stream);                                                               \
  }

XK_DEFINE_FSAI(f64, double, double)
XK_DEFINE_FSAI(f32, float, float)
/* complex: interleaved (re, im), strides and counts in whole complex elements */
XK_DEFINE_FSAI(c128, double, xk::fz<double>)
XK_DEFINE_FSAI(c64, float, xk::fz<float>)

}  // extern "C"
