// xitorch_amd :: unsymmetric factorised sparse approximate inverse (FSAI) of a CSR operator: the build of G_L and G_U.
//
//   xk_fsai_lu_build   row i on its columns S_i (sorted, i last, m = |S_i| <= 32), A_SS = A[S_i, S_i] (both triangles):
//                        A_SS u = e_m,  A_SS^T g = e_m  (one LU with partial pivoting serves both)
//                        G_L[i, S_i] = g / g_m  (unit diagonal),   G_U[S_i, i] = u,  stored as W = G_U^H: W[i, S_i] = conj(u)
//                      so that (G_L A)[i, j] = 0 and (A G_U)[j, i] = 0 for j in S_i, j != i, and diag(G_L A G_U) = 1
//                      (DESIGN.md §3.18).
//
// Work distribution: that of xk_fsai_build.  One wavefront per (row, batch member), the members of one row in
// neighbouring waves.  The rows are independent: no wave reads what another one writes, there is no workgroup barrier
// (a wave whose index is past the last row leaves at once, and m differs from wave to wave), and every loop runs to a
// count read before it starts (m <= 32, or a row length of A clipped to the stored entry count).
//
//   gather     for local row r the wave walks the stored entries of row S_i[r] of A in storage order, 64 at a time (one
//              coalesced load, then one lane broadcast per entry); lane c < m adds an entry to A_SS[r, c] when its
//              column is S_i[c] -- for every r, so both triangles of the block are filled.  Duplicates add up in storage
//              order, entries of S_i x S_i that A does not store stay zero, nothing is made real.
//   LU         right-looking with partial pivoting, lane r owns row r.  Column k: the pivot is the not-yet-used row with
//              the largest |re| + |im| (ties: the lowest row; a magnitude that is not a number counts as infinite, so it
//              is taken at once and ends the row in the fallback), found by a wave reduction and recorded per lane as
//              `pos` (the step at which the lane's row was used, m while it is free).  No rows move.  The free lanes
//              store their multiplier in place and subtract it times the pivot row (read as a broadcast).
//   solves     A_SS u = e_m: forward through the multipliers in pivot order, back through U column by column.
//              A_SS^T g = e_m: forward through U^T (lane c holds component c, the pivot row is read across the lanes),
//              back through L^T, which leaves g_r in the lane that owns row r.
//
// The block in LDS.  The full m x m block is wave-private, row r at element offset r * 33.  Lane r reads and writes
// element (r, k) for one k at a time, so the lanes' addresses are 33 elements apart.  The LDS has 64 banks of 4 B; a
// 4-byte access is served in two groups of 32 lanes on bank (a/4) mod 32, an 8-byte read in two groups of 32 on
// (a/4) mod 64, a 16-byte read in four groups of 16 on (a/4) mod 64 (MI355X LDS table).  With a stride of 32 elements
// lane r's dword address is 32 r, 64 r or 128 r (4-, 8-, 16-byte elements): one bank for every lane, a 32-way (16-way
// for complex128) conflict on every access of the factorisation.  With 33 it is 33 r, 66 r = 2 r, 132 r = 4 r modulo
// the bank count: the 32 (16) lanes of a group cover 32 x 1, 32 x 2 or 16 x 4 distinct banks, and the same holds for
// the stores (groups of 16 lanes x 2 banks and 8 lanes x 4 banks modulo 32).  The pivot row is read at one address by
// every lane (a broadcast) and, in the transposed solve, across consecutive elements: no conflict either.
//   33 * 32 elements per wave: 4.1 KB (float32), 8.3 KB (float64, complex64), 16.5 KB (complex128).  Four waves of
// complex128 would be 66 KB, over the 64 KB of static LDS, so the kernel runs 32 / sizeof(element) waves per workgroup,
// four at the most: 4 / 4 / 4 / 2 waves, 16.5 / 33 / 33 / 33 KB.
//
// Fallback.  A pivot that is exactly zero or not finite, a u or g that is not finite, or g_m == 0 gives
// G_L[i, .] = e_i and G_U[., i] = e_i / a_ii (e_i when a_ii, duplicates summed, is zero or not finite), and one integer
// atomicAdd on nfail[member].  All sums have a fixed order, all stores are plain vector stores: the result is
// bit-identical from run to run.
#include "xk_fsai_el.h"

namespace xk {

constexpr int FSAI_LU_MAX = 32;                                // longest row of G_L / W
constexpr int FSAI_LU_LD = FSAI_LU_MAX + 1;                    // row stride of the block in LDS, elements (odd: see above)
constexpr int FSAI_LU_BLK = FSAI_LU_MAX * FSAI_LU_LD;          // elements per wave
template <typename E> struct FsaiLuWaves {                     // waves (rows) per workgroup
  static constexpr int value = 32 / (int)sizeof(E) > 4 ? 4 : 32 / (int)sizeof(E);
};
static_assert(FsaiLuWaves<fz<double>>::value * FSAI_LU_BLK * sizeof(fz<double>) <= 65536, "static LDS");
static_assert(FsaiLuWaves<double>::value * FSAI_LU_BLK * sizeof(double) <= 65536, "static LDS");

// The block algorithm, stated once: LU with partial pivoting of the m x m block Ab (lane r owns row r, row stride
// FSAI_LU_LD, wave-private LDS) and the two solves from it.  On return lane c < m holds u_c (A u = e_m) and g_c
// (A^T g = e_m).  False, in every lane alike, when a pivot is exactly zero or not finite.
template <typename E>
__device__ __forceinline__ bool fsai_lu_block(E* Ab, int m, int lane, E& u_out, E& g_out) {
  typedef FsaiEl<E> X;
  typedef typename X::real R;
  E* mine = Ab + lane * FSAI_LU_LD;                            // (only dereferenced by lanes < m)
  int pos = m;                                                 // the step that used this lane's row; m: still free
  for (int k = 0; k < m; ++k) {
    fsai_wave_sync();
    const bool cand = lane < m && pos == m;
    E v = X::zero();
    R mag = R(-1);
    if (cand) {
      v = mine[k];
      mag = X::abs1(v);
      if (!(mag == mag)) mag = INFINITY;
    }
    int who = lane;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
      const R om = shfl_xor_t(mag, s);
      const int ow = __shfl_xor(who, s, 64);
      if (om > mag || (om == mag && ow < who)) {
        mag = om;
        who = ow;
      }
    }
    const E piv = X::bcast(v, who);                            // the same in every lane: the wave leaves together
    if (X::is_zero(piv) || !X::finite(piv)) return false;
    if (lane == who) {
      pos = k;
    } else if (cand) {
      const E l = X::div(v, piv);
      mine[k] = l;
      const E* prow = Ab + who * FSAI_LU_LD;
      for (int c = k + 1; c < m; ++c) mine[c] = X::msubu(mine[c], l, prow[c]);
    }
  }
  fsai_wave_sync();
  const R one = R(1);

  // ---- A u = e_m.  L y = P e_m in pivot order: the lane used at step k holds y_k once the steps before k are done
  E acc = lane == m - 1 ? X::from_re(one) : X::zero();
  for (int k = 0; k < m; ++k) {
    const int p = __ffsll((unsigned long long)__ballot(pos == k)) - 1;
    const E yk = X::bcast(acc, p);
    if (lane < m && pos > k) acc = X::msubu(acc, mine[k], yk);
  }
  // U x = y, column by column from the last; lane c keeps x_c
  E u = X::zero();
  for (int c = m - 1; c >= 0; --c) {
    const int p = __ffsll((unsigned long long)__ballot(pos == c)) - 1;
    E xc = X::zero();
    if (lane == p) xc = X::div(acc, mine[c]);
    xc = X::bcast(xc, p);
    if (lane == c) u = xc;
    if (lane < m && pos < c) acc = X::msubu(acc, mine[c], xc);
  }

  // ---- A^T g = e_m.  U^T z = e_m: lane c holds component c, z_k lands in the lane whose row was used at step k
  acc = lane == m - 1 ? X::from_re(one) : X::zero();
  E w = X::zero();
  for (int k = 0; k < m; ++k) {
    const int p = __ffsll((unsigned long long)__ballot(pos == k)) - 1;
    const E* prow = Ab + p * FSAI_LU_LD;
    E zk = X::zero();
    if (lane == k) zk = X::div(acc, prow[k]);
    zk = X::bcast(zk, k);
    if (lane == p) w = zk;
    if (lane > k && lane < m) acc = X::msubu(acc, prow[lane], zk);
  }
  // L^T w = z from the last step back; what is left in the lane that owns row r is g_r (g = P^T w)
  for (int t = m - 1; t >= 1; --t) {
    const int p = __ffsll((unsigned long long)__ballot(pos == t)) - 1;
    const E wt = X::bcast(w, p);
    if (lane < m && pos < t) w = X::msubu(w, Ab[p * FSAI_LU_LD + pos], wt);
  }
  u_out = u;
  g_out = w;
  return true;
}

template <typename E>
__global__ __launch_bounds__(64 * FsaiLuWaves<E>::value) void fsai_lu_build_kernel(
    const int* __restrict__ a_ptr, const int* __restrict__ a_idx, const E* __restrict__ a_val, long sV, int a_nnz,
    const int* __restrict__ g_ptr, const int* __restrict__ g_idx, E* __restrict__ gl_val, E* __restrict__ w_val,
    long sG, int g_nnz, int* __restrict__ nfail, int N, int B) {
  typedef FsaiEl<E> X;
  typedef typename X::real R;
  constexpr int WAVES = FsaiLuWaves<E>::value;
  __shared__ E blk[WAVES][FSAI_LU_BLK];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long w = (long)blockIdx.x * WAVES + wv;
  if (w >= (long)N * B) return;                     // the whole wave leaves; nothing below waits for another wave
  const int row = (int)(w / B), b = (int)(w % B);
  E* Ab = blk[wv];
  const int g0 = g_ptr[row];
  const int m = g_ptr[row + 1] - g0;
  if (g0 < 0 || m < 1 || m > FSAI_LU_MAX || (long)g0 + m > g_nnz) {
    // not a row this kernel serves (the caller checks the pattern once): nothing is read or written, it is counted
    if (lane == 0) atomicAdd(nfail + b, 1);
    return;
  }
  const E* Av = a_val + (long)b * sV;
  E* GLb = gl_val + (long)b * sG + g0;
  E* Wb = w_val + (long)b * sG + g0;
  const int sc = lane < m ? g_idx[g0 + lane] : -1;             // lane c holds S_i[c]

  // ---- gather the whole block A_SS, row by row
  E aii = X::zero();
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
        myv = Av[k];
      }
      const int n = (k1 - kb) < 64 ? (k1 - kb) : 64;
      for (int t = 0; t < n; ++t) {
        const int col = __shfl(myc, t, 64);
        const E v = X::bcast(myv, t);
        if (lane < m && col == sc) acc = X::add(acc, v);
      }
    }
    if (lane < m) Ab[r * FSAI_LU_LD + lane] = acc;
    if (r == m - 1) aii = X::bcast(acc, m - 1);
  }

  E u = X::zero(), g = X::zero();
  bool ok = fsai_lu_block<E>(Ab, m, lane, u, g);
  if (ok) {
    const E gm = X::bcast(g, m - 1);
    if (__ballot(lane < m && !(X::finite(u) && X::finite(g))) != 0ull || X::is_zero(gm)) {
      ok = false;
    } else {
      g = X::div(g, gm);
    }
  }
  if (ok) {
    if (lane < m) {
      GLb[lane] = lane == m - 1 ? X::from_re(R(1)) : g;
      Wb[lane] = X::conj(u);
    }
    return;
  }
  E d = X::from_re(R(1));
  if (!X::is_zero(aii) && X::finite(aii)) d = X::div(d, aii);
  if (lane < m) {
    GLb[lane] = lane == m - 1 ? X::from_re(R(1)) : X::zero();
    Wb[lane] = lane == m - 1 ? X::conj(d) : X::zero();
  }
  if (lane == 0) atomicAdd(nfail + b, 1);
}

template <typename E>
static int fsai_lu_build(const int* a_ptr, const int* a_idx, const void* a_val, long sV, int a_nnz, const int* g_ptr,
                         const int* g_idx, void* gl_val, void* w_val, long sG, int g_nnz, int* nfail, int N, int B,
                         hipStream_t st) {
  if (!a_ptr || !a_idx || !a_val || !g_ptr || !g_idx || !gl_val || !w_val || !nfail) return XK_ERR_ARG;
  if (N <= 0 || B <= 0 || sV < 0 || sG < 0 || a_nnz < 0 || g_nnz < N) return XK_ERR_ARG;
  if (B > 1 && (sG < g_nnz || (sV != 0 && sV < a_nnz))) return XK_ERR_ARG;      // members overlap
  // neither factor may be written over the values it is built from, nor over the other factor
  const uintptr_t a0 = (uintptr_t)a_val, a1 = a0 + sizeof(E) * (size_t)((long)(B - 1) * sV + a_nnz);
  const size_t gbytes = sizeof(E) * (size_t)((long)(B - 1) * sG + g_nnz);
  const uintptr_t l0 = (uintptr_t)gl_val, l1 = l0 + gbytes, w0 = (uintptr_t)w_val, w1 = w0 + gbytes;
  if ((l0 < a1 && a0 < l1) || (w0 < a1 && a0 < w1) || (l0 < w1 && w0 < l1)) return XK_ERR_ARG;
  constexpr int WAVES = FsaiLuWaves<E>::value;
  const long nblk = ((long)N * B + WAVES - 1) / WAVES;
  if (nblk > 0x7fffffffL) return XK_ERR_UNSUPPORTED;
  hipError_t e = hipMemsetAsync(nfail, 0, sizeof(int) * (size_t)B, st);
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL((fsai_lu_build_kernel<E>), dim3((unsigned)nblk), dim3(64 * WAVES), 0, st, a_ptr, a_idx,
                     (const E*)a_val, sV, a_nnz, g_ptr, g_idx, (E*)gl_val, (E*)w_val, sG, g_nnz, nfail, N, B);
  XK_LAUNCH_CHECK();
  return XK_OK;
}

}  // namespace xk

extern "C" {

int xk_fsai_lu_max_row(void) { return xk::FSAI_LU_MAX; }

#define XK_DEFINE_FSAI_LU(SUF, T, E)                                                                              \
  int xk_fsai_lu_build_##SUF(const int* a_ptr, const int* a_idx, const T* a_val, long sV, int a_nnz,             \
                             const int* g_ptr, const int* g_idx, T* gl_val, T* w_val, long sG, int g_nnz,        \
                             int* nfail, int N, int B, void* stream) {                                           \
    return xk::fsai_lu_build<E>(a_ptr, a_idx, a_val, sV, a_nnz, g_ptr, g_idx, gl_val, w_val, sG, g_nnz, nfail,   \
                                N, B, (hipStream_t)stream);                                                      \
  }

XK_DEFINE_FSAI_LU(f64, double, double)
XK_DEFINE_FSAI_LU(f32, float, float)
/* complex: interleaved (re, im), strides and counts in whole complex elements */
XK_DEFINE_FSAI_LU(c128, double, xk::fz<double>)
XK_DEFINE_FSAI_LU(c64, float, xk::fz<float>)

}  // extern "C"
