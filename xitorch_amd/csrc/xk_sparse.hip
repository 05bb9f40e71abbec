// xitorch_amd :: CSR sparse operator apply and its values gradient.
//
//   xk_csr_mm     Y[b,c,i] = sum_{k in row i} val[b, perm ? perm[k] : k] * X[b,c,idx[k]]
//   xk_csr_sddmm  G[b,k]   = sum_c U[b,c,row_of[k]] * W[b,c,col[k]]
// and, further down, the same two on interleaved complex data (_c128 / _c64): the value conjugated on request as
// it is loaded (the adjoint apply), conj(W) in the gradient.
//
// One sparsity pattern is shared by the whole batch.  The transposed operator is the same product on the
// CSC view of the pattern (ptr = column pointers, idx = row indices) with perm[k] = the CSR position of the
// k-th CSC entry, so the values are never copied and swapped values stay valid.
//
// Row mapping.  The host bins the output rows by length once (xitorch_amd/linop.py, _CsrView) and calls
// one launch per non-empty bin; inside a bin every row is served by a group of W lanes:
//   bin 0: len <= 4      W = 1    (diagonals, empty rows)
//   bin 1: len <= 32     W = 8    (stencils, uniform random patterns)
//   bin 2: len <= 1024   W = 64   (one wave per row)
//   bin 3: longer        split into segments of CSR_SEG entries, one workgroup per segment; the segment sums
//                        go to a scratch array and a second launch adds them per row in segment order
// so no lane walks more than ~16 entries of a long row and a full row of a power-law pattern spreads over
// len / CSR_SEG workgroups.  Lane l of a group takes the entries k = start + l, start + l + W, ... and the
// partial sums meet in a fixed-shape tree: the summation order depends on the pattern only, so repeated
// calls are bit-identical (no atomics).  The batch loop sits inside the group, so the other members re-read
// a row's indices right after the first one did (meant to hit in cache; not verified by counters).
// X is gathered element-wise straight from the panel vectors.  Only scalar loads: there is
// no alignment requirement.
//
// XK_CSR_PROBE_INTERLEAVED (measurement builds only, never shipped): X is read as an interleaved (Nin, C)
// array per batch member, X[b, j*ldx + c], for the gather-form comparison of scripts/sparse_bench.py.
#include "xk_common.h"

#ifdef XK_CSR_PROBE_INTERLEAVED
#define XK_CSR_X(c, j) Xb[(long)(j) * ldx + (c)]
#else
#define XK_CSR_X(c, j) Xb[(long)(c) * ldx + (j)]
#endif

namespace xk {

constexpr int CSR_NBINS = 4;
constexpr int CSR_SEG = 4096;        // entries of a long row per workgroup (16 per lane)
#ifdef XK_CSR_PROBE_INTERLEAVED
constexpr bool CSR_INTERLEAVED = true;
#else
constexpr bool CSR_INTERLEAVED = false;
#endif

// partial sums of the W lanes of a group -> lane 0 of the group (fixed order; all 64 lanes participate)
template <typename T, int W>
__device__ __forceinline__ T group_sum(T v) {
  if (W >= 64) v += shfl_xor_t(v, 32);
  if (W >= 32) v += shfl_xor_t(v, 16);
  if (W >= 16) v += lane_partner<8>(v);
  if (W >= 8) v += lane_partner<4>(v);
  if (W >= 4) v += lane_partner<2>(v);
  if (W >= 2) v += lane_partner<1>(v);
  return v;
}

template <typename T, int C, int W>
__global__ __launch_bounds__(256) void csr_mm_kernel(
    const int* __restrict__ ptr, const int* __restrict__ idx, const int* __restrict__ perm,
    const T* __restrict__ val, long sV, const int* __restrict__ rows, int nrows, const T* __restrict__ X,
    T* __restrict__ Y, int B, long ldx, long sX, long ldy, long sY) {
  const long g = ((long)blockIdx.x * 256 + threadIdx.x) / W;
  const int lane = threadIdx.x % W;
  const bool live = g < nrows;
  const int row = live ? rows[g] : 0;
  const long k0 = live ? ptr[row] : 0;
  const long k1 = live ? ptr[row + 1] : 0;
  for (int b = 0; b < B; ++b) {
    const T* Vb = val + (long)b * sV;
    const T* Xb = X + (long)b * sX;
    T acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = T(0);
    for (long k = k0 + lane; k < k1; k += W) {
      const int j = idx[k];
      const T v = Vb[perm ? perm[k] : k];
#pragma unroll
      for (int c = 0; c < C; ++c) acc[c] += v * XK_CSR_X(c, j);
    }
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = group_sum<T, W>(acc[c]);
    if (live && lane == 0) {
      T* Yb = Y + (long)b * sY + row;
#pragma unroll
      for (int c = 0; c < C; ++c) Yb[(long)c * ldy] = acc[c];
    }
  }
}

// long rows, pass 1: one workgroup per segment s (of long row q = seg_q[s]); its 256 partial sums are folded
// by a fixed tree and written to part[(b*C + c)*nseg + s]
template <typename T, int C>
__global__ __launch_bounds__(256) void csr_mm_seg_kernel(
    const int* __restrict__ ptr, const int* __restrict__ idx, const int* __restrict__ perm,
    const T* __restrict__ val, long sV, const int* __restrict__ rows, const int* __restrict__ seg_q,
    const int* __restrict__ seg_off, int nseg, const T* __restrict__ X, T* __restrict__ part, int B, long ldx,
    long sX) {
  __shared__ T wsum[C][4];
  const int s = blockIdx.x;
  const int q = seg_q[s];
  const int row = rows[q];
  const long k0 = (long)ptr[row] + (long)(s - seg_off[q]) * CSR_SEG;
  const long kend = ptr[row + 1];
  const long k1 = k0 + CSR_SEG < kend ? k0 + CSR_SEG : kend;
  const int wave = threadIdx.x / 64, wl = threadIdx.x % 64;
  for (int b = 0; b < B; ++b) {
    const T* Vb = val + (long)b * sV;
    const T* Xb = X + (long)b * sX;
    T acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = T(0);
    for (long k = k0 + threadIdx.x; k < k1; k += 256) {
      const int j = idx[k];
      const T v = Vb[perm ? perm[k] : k];
#pragma unroll
      for (int c = 0; c < C; ++c) acc[c] += v * XK_CSR_X(c, j);
    }
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = group_sum<T, 64>(acc[c]);
    if (wl == 0) {
#pragma unroll
      for (int c = 0; c < C; ++c) wsum[c][wave] = acc[c];
    }
    __syncthreads();
    if (threadIdx.x < C) {
      const int c = threadIdx.x;
      part[((long)b * C + c) * nseg + s] = (wsum[c][0] + wsum[c][1]) + (wsum[c][2] + wsum[c][3]);
    }
    __syncthreads();
  }
}

// long rows, pass 2: Y[b,c,row_q] = sum of the row's segment sums in segment order (one thread per (b, c, q))
template <typename T>
__global__ __launch_bounds__(256) void csr_mm_seg_fold_kernel(
    const int* __restrict__ rows, const int* __restrict__ seg_off, int nlong, int nseg, const T* __restrict__ part,
    T* __restrict__ Y, int B, int C, long ldy, long sY) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long)B * C * nlong) return;
  const int q = (int)(t % nlong);
  const long bc = t / nlong;
  const int c = (int)(bc % C), b = (int)(bc / C);
  const T* p = part + bc * nseg;
  T acc = T(0);
  for (int s = seg_off[q]; s < seg_off[q + 1]; ++s) acc += p[s];
  Y[(long)b * sY + (long)c * ldy + rows[q]] = acc;
}

template <typename T, int C>
static int csr_launch(const int* ptr, const int* idx, const int* perm, const T* val, long sV, const int* rows,
                      const int* bin_off, const int* seg_q, const int* seg_off, int nseg, T* ws, const T* Xc,
                      T* Yc, int B, long ldx, long sX, long ldy, long sY, hipStream_t st) {
  for (int bin = 0; bin < CSR_NBINS; ++bin) {
    const int n = bin_off[bin + 1] - bin_off[bin];
    if (n <= 0) continue;
    const int* r = rows + bin_off[bin];
    if (bin == 3) {
      hipLaunchKernelGGL((csr_mm_seg_kernel<T, C>), dim3((unsigned)nseg), dim3(256), 0, st, ptr, idx, perm, val, sV,
                         r, seg_q, seg_off, nseg, Xc, ws, B, ldx, sX);
      XK_LAUNCH_CHECK();
      const long nt = (long)B * C * n;
      hipLaunchKernelGGL((csr_mm_seg_fold_kernel<T>), dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, st, r,
                         seg_off, n, nseg, (const T*)ws, Yc, B, C, ldy, sY);
    } else {
      const int W = bin == 0 ? 1 : (bin == 1 ? 8 : 64);
      const dim3 grid((unsigned)(((long)n * W + 255) / 256));
#define XK_CSR_GO(WW)                                                                                            \
  hipLaunchKernelGGL((csr_mm_kernel<T, C, WW>), grid, dim3(256), 0, st, ptr, idx, perm, val, sV, r, n, Xc, Yc, B, \
                     ldx, sX, ldy, sY)
      if (W == 1) XK_CSR_GO(1);
      else if (W == 8) XK_CSR_GO(8);
      else XK_CSR_GO(64);
#undef XK_CSR_GO
    }
    XK_LAUNCH_CHECK();
  }
  return XK_OK;
}

template <typename T>
static int csr_mm(const int* ptr, const int* idx, const int* perm, const T* val, long sV, const int* rows,
                  const int* bin_off, const int* seg_q, const int* seg_off, int nseg, T* ws, const T* X, T* Y, int B,
                  int C, long ldx, long sX, long ldy, long sY, hipStream_t st) {
  for (int c0 = 0; c0 < C; c0 += 8) {
    const int pc = (C - c0) >= 8 ? 8 : (C - c0);
#ifdef XK_CSR_PROBE_INTERLEAVED
    const T* Xc = X + c0;
#else
    const T* Xc = X + (long)c0 * ldx;
#endif
    T* Yc = Y + (long)c0 * ldy;
    int rc = XK_ERR_UNSUPPORTED;
    switch (pc) {
#define XK_CASE(CC)                                                                                                  \
  case CC:                                                                                                           \
    rc = csr_launch<T, CC>(ptr, idx, perm, val, sV, rows, bin_off, seg_q, seg_off, nseg, ws, Xc, Yc, B, ldx, sX, ldy, \
                           sY, st);                                                                                  \
    break;
      XK_CASE(1) XK_CASE(2) XK_CASE(3) XK_CASE(4) XK_CASE(5) XK_CASE(6) XK_CASE(7) XK_CASE(8)
#undef XK_CASE
    }
    if (rc != XK_OK) return rc;
  }
  return XK_OK;
}

// values gradient: one thread per stored entry, batch members and columns summed in a fixed order
template <typename T>
__global__ __launch_bounds__(256) void csr_sddmm_kernel(
    const int* __restrict__ row_of, const int* __restrict__ col, const T* __restrict__ U, const T* __restrict__ W,
    T* __restrict__ G, int nnz, int B, int C, long ldu, long sU, long ldw, long sW, long sG) {
  const long k = (long)blockIdx.x * 256 + threadIdx.x;
  if (k >= nnz) return;
  const int i = row_of[k], j = col[k];
  for (int b = 0; b < B; ++b) {
    const T* Ub = U + (long)b * sU + i;
    const T* Wb = W + (long)b * sW + j;
    T a = T(0);
    for (int c = 0; c < C; ++c) a += Ub[(long)c * ldu] * Wb[(long)c * ldw];
    G[(long)b * sG + k] = a;
  }
}

// ------------------------------------------------------------------------------------------------ complex
// The same mapping on interleaved (re, im) elements of component type T.  One element is one naturally aligned
// 2*sizeof(T) load (16 B for complex128, 8 B for complex64); values, panels and outputs are addressed by whole
// elements, so every slice of a complex array is aligned.  conj_val conjugates the value as it is loaded (the
// adjoint apply on the CSC view); re and im of a sum go through the same group_sum tree, so the order of the
// additions is the real kernel's.
template <typename T> struct alignas(2 * sizeof(T)) cel { T re, im; };

template <typename T> __device__ __forceinline__ void cel_fma(cel<T>& acc, cel<T> a, cel<T> b) {   // acc += a b
  acc.re += a.re * b.re - a.im * b.im;
  acc.im += a.re * b.im + a.im * b.re;
}
template <typename T> __device__ __forceinline__ cel<T> cel_add(cel<T> a, cel<T> b) {
  return {a.re + b.re, a.im + b.im};
}
template <typename T, int W> __device__ __forceinline__ cel<T> cel_group_sum(cel<T> v) {
  return {group_sum<T, W>(v.re), group_sum<T, W>(v.im)};
}

template <typename T, int C, int W>
__global__ __launch_bounds__(256) void csr_mm_c_kernel(
    const int* __restrict__ ptr, const int* __restrict__ idx, const int* __restrict__ perm,
    const cel<T>* __restrict__ val, long sV, int conj_val, const int* __restrict__ rows, int nrows,
    const cel<T>* __restrict__ X, cel<T>* __restrict__ Y, int B, long ldx, long sX, long ldy, long sY) {
  const long g = ((long)blockIdx.x * 256 + threadIdx.x) / W;
  const int lane = threadIdx.x % W;
  const bool live = g < nrows;
  const int row = live ? rows[g] : 0;
  const long k0 = live ? ptr[row] : 0;
  const long k1 = live ? ptr[row + 1] : 0;
  for (int b = 0; b < B; ++b) {
    const cel<T>* Vb = val + (long)b * sV;
    const cel<T>* Xb = X + (long)b * sX;
    cel<T> acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = {T(0), T(0)};
    for (long k = k0 + lane; k < k1; k += W) {
      const int j = idx[k];
      cel<T> v = Vb[perm ? perm[k] : k];
      if (conj_val) v.im = -v.im;
#pragma unroll
      for (int c = 0; c < C; ++c) cel_fma(acc[c], v, Xb[(long)c * ldx + j]);
    }
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = cel_group_sum<T, W>(acc[c]);
    if (live && lane == 0) {
      cel<T>* Yb = Y + (long)b * sY + row;
#pragma unroll
      for (int c = 0; c < C; ++c) Yb[(long)c * ldy] = acc[c];
    }
  }
}

template <typename T, int C>
__global__ __launch_bounds__(256) void csr_mm_c_seg_kernel(
    const int* __restrict__ ptr, const int* __restrict__ idx, const int* __restrict__ perm,
    const cel<T>* __restrict__ val, long sV, int conj_val, const int* __restrict__ rows,
    const int* __restrict__ seg_q, const int* __restrict__ seg_off, int nseg, const cel<T>* __restrict__ X,
    cel<T>* __restrict__ part, int B, long ldx, long sX) {
  __shared__ cel<T> wsum[C][4];
  const int s = blockIdx.x;
  const int q = seg_q[s];
  const int row = rows[q];
  const long k0 = (long)ptr[row] + (long)(s - seg_off[q]) * CSR_SEG;
  const long kend = ptr[row + 1];
  const long k1 = k0 + CSR_SEG < kend ? k0 + CSR_SEG : kend;
  const int wave = threadIdx.x / 64, wl = threadIdx.x % 64;
  for (int b = 0; b < B; ++b) {
    const cel<T>* Vb = val + (long)b * sV;
    const cel<T>* Xb = X + (long)b * sX;
    cel<T> acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = {T(0), T(0)};
    for (long k = k0 + threadIdx.x; k < k1; k += 256) {
      const int j = idx[k];
      cel<T> v = Vb[perm ? perm[k] : k];
      if (conj_val) v.im = -v.im;
#pragma unroll
      for (int c = 0; c < C; ++c) cel_fma(acc[c], v, Xb[(long)c * ldx + j]);
    }
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = cel_group_sum<T, 64>(acc[c]);
    if (wl == 0) {
#pragma unroll
      for (int c = 0; c < C; ++c) wsum[c][wave] = acc[c];
    }
    __syncthreads();
    if (threadIdx.x < C) {
      const int c = threadIdx.x;
      part[((long)b * C + c) * nseg + s] =
          cel_add(cel_add(wsum[c][0], wsum[c][1]), cel_add(wsum[c][2], wsum[c][3]));
    }
    __syncthreads();
  }
}

template <typename T>
__global__ __launch_bounds__(256) void csr_mm_c_seg_fold_kernel(
    const int* __restrict__ rows, const int* __restrict__ seg_off, int nlong, int nseg,
    const cel<T>* __restrict__ part, cel<T>* __restrict__ Y, int B, int C, long ldy, long sY) {
  const long t = (long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long)B * C * nlong) return;
  const int q = (int)(t % nlong);
  const long bc = t / nlong;
  const int c = (int)(bc % C), b = (int)(bc / C);
  const cel<T>* p = part + bc * nseg;
  cel<T> acc = {T(0), T(0)};
  for (int s = seg_off[q]; s < seg_off[q + 1]; ++s) acc = cel_add(acc, p[s]);
  Y[(long)b * sY + (long)c * ldy + rows[q]] = acc;
}

template <typename T, int C>
static int csr_c_launch(const int* ptr, const int* idx, const int* perm, const cel<T>* val, long sV, int conj_val,
                        const int* rows, const int* bin_off, const int* seg_q, const int* seg_off, int nseg,
                        cel<T>* ws, const cel<T>* Xc, cel<T>* Yc, int B, long ldx, long sX, long ldy, long sY,
                        hipStream_t st) {
  for (int bin = 0; bin < CSR_NBINS; ++bin) {
    const int n = bin_off[bin + 1] - bin_off[bin];
    if (n <= 0) continue;
    const int* r = rows + bin_off[bin];
    if (bin == 3) {
      hipLaunchKernelGGL((csr_mm_c_seg_kernel<T, C>), dim3((unsigned)nseg), dim3(256), 0, st, ptr, idx, perm, val,
                         sV, conj_val, r, seg_q, seg_off, nseg, Xc, ws, B, ldx, sX);
      XK_LAUNCH_CHECK();
      const long nt = (long)B * C * n;
      hipLaunchKernelGGL((csr_mm_c_seg_fold_kernel<T>), dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, st, r,
                         seg_off, n, nseg, (const cel<T>*)ws, Yc, B, C, ldy, sY);
    } else {
      const int W = bin == 0 ? 1 : (bin == 1 ? 8 : 64);
      const dim3 grid((unsigned)(((long)n * W + 255) / 256));
#define XK_CSR_GO(WW)                                                                                          \
  hipLaunchKernelGGL((csr_mm_c_kernel<T, C, WW>), grid, dim3(256), 0, st, ptr, idx, perm, val, sV, conj_val, r, \
                     n, Xc, Yc, B, ldx, sX, ldy, sY)
      if (W == 1) XK_CSR_GO(1);
      else if (W == 8) XK_CSR_GO(8);
      else XK_CSR_GO(64);
#undef XK_CSR_GO
    }
    XK_LAUNCH_CHECK();
  }
  return XK_OK;
}

// 8 columns per pass for both complex types: 16 accumulator components per lane
template <typename T>
static int csr_mm_c(const int* ptr, const int* idx, const int* perm, const cel<T>* val, long sV, int conj_val,
                    const int* rows, const int* bin_off, const int* seg_q, const int* seg_off, int nseg, cel<T>* ws,
                    const cel<T>* X, cel<T>* Y, int B, int C, long ldx, long sX, long ldy, long sY, hipStream_t st) {
  for (int c0 = 0; c0 < C; c0 += 8) {
    const int pc = (C - c0) >= 8 ? 8 : (C - c0);
    const cel<T>* Xc = X + (long)c0 * ldx;
    cel<T>* Yc = Y + (long)c0 * ldy;
    int rc = XK_ERR_UNSUPPORTED;
    switch (pc) {
#define XK_CASE(CC)                                                                                              \
  case CC:                                                                                                       \
    rc = csr_c_launch<T, CC>(ptr, idx, perm, val, sV, conj_val, rows, bin_off, seg_q, seg_off, nseg, ws, Xc, Yc, \
                             B, ldx, sX, ldy, sY, st);                                                           \
    break;
      XK_CASE(1) XK_CASE(2) XK_CASE(3) XK_CASE(4) XK_CASE(5) XK_CASE(6) XK_CASE(7) XK_CASE(8)
#undef XK_CASE
    }
    if (rc != XK_OK) return rc;
  }
  return XK_OK;
}

// values gradient, complex: G[b,k] = sum_c U[b,c,row_of[k]] conj(W[b,c,col[k]]), one thread per stored entry
template <typename T>
__global__ __launch_bounds__(256) void csr_sddmm_c_kernel(
    const int* __restrict__ row_of, const int* __restrict__ col, const cel<T>* __restrict__ U,
    const cel<T>* __restrict__ W, cel<T>* __restrict__ G, int nnz, int B, int C, long ldu, long sU, long ldw,
    long sW, long sG) {
  const long k = (long)blockIdx.x * 256 + threadIdx.x;
  if (k >= nnz) return;
  const int i = row_of[k], j = col[k];
  for (int b = 0; b < B; ++b) {
    const cel<T>* Ub = U + (long)b * sU + i;
    const cel<T>* Wb = W + (long)b * sW + j;
    cel<T> a = {T(0), T(0)};
    for (int c = 0; c < C; ++c) {
      cel<T> w = Wb[(long)c * ldw];
      w.im = -w.im;
      cel_fma(a, Ub[(long)c * ldu], w);
    }
    G[(long)b * sG + k] = a;
  }
}

}  // namespace xk

extern "C" {

int xk_csr_seg_len(void) { return xk::CSR_SEG; }

#define XK_DEFINE_SPARSE(SUF, T)                                                                                \
  int xk_csr_mm_##SUF(const int* ptr, const int* idx, const int* perm, const T* val, long sV, const int* rows,   \
                      const int* bin_off, const int* seg_q, const int* seg_off, int nseg, T* ws, const T* X,    \
                      T* Y, int B, int Mout, int Nin, int C, long ldx, long sX, long ldy, long sY,              \
                      void* stream) {                                                                           \
    if (B < 0 || Mout < 0 || Nin < 0 || C < 0 || sV < 0 || sX < 0 || sY < 0 || nseg < 0) return XK_ERR_ARG;    \
    if (B == 0 || Mout == 0 || C == 0) return XK_OK;                                                            \
    if (!bin_off || bin_off[0] != 0 || bin_off[xk::CSR_NBINS] != Mout) return XK_ERR_ARG;                      \
    for (int q = 0; q < xk::CSR_NBINS; ++q)                                                                     \
      if (bin_off[q + 1] < bin_off[q]) return XK_ERR_ARG;                                                       \
    if (bin_off[4] > bin_off[3] && (nseg < bin_off[4] - bin_off[3] || !seg_q || !seg_off || !ws))              \
      return XK_ERR_ARG;                                                                                        \
    if (ldy < Mout || (!xk::CSR_INTERLEAVED && ldx < Nin)) return XK_ERR_UNSUPPORTED;                          \
    if (B > 1 && sY < (long)C * ldy) return XK_ERR_UNSUPPORTED;  /* overlapping outputs */                      \
    return xk::csr_mm<T>(ptr, idx, perm, val, sV, rows, bin_off, seg_q, seg_off, nseg, ws, X, Y, B, C, ldx, sX, \
                         ldy, sY, (hipStream_t)stream);                                                         \
  }                                                                                                             \
  int xk_csr_sddmm_##SUF(const int* row_of, const int* col, const T* U, const T* W, T* G, int nnz, int B,        \
                         int M, int N, int C, long ldu, long sU, long ldw, long sW, long sG, void* stream) {     \
    if (nnz < 0 || B < 0 || M < 0 || N < 0 || C < 0 || sU < 0 || sW < 0 || sG < 0) return XK_ERR_ARG;           \
    if (nnz == 0 || B == 0) return XK_OK;                                                                       \
    if (C > 0 && (ldu < M || ldw < N)) return XK_ERR_UNSUPPORTED;                                               \
    if (B > 1 && sG < nnz) return XK_ERR_UNSUPPORTED;                                                           \
    if (C == 0) {                                                                                               \
      for (int b = 0; b < B; ++b) {                                                                             \
        hipError_t e = hipMemsetAsync(G + (long)b * sG, 0, sizeof(T) * (size_t)nnz, (hipStream_t)stream);      \
        if (e != hipSuccess) return (int)e;                                                                     \
      }                                                                                                         \
      return XK_OK;                                                                                             \
    }                                                                                                           \
    hipLaunchKernelGGL((xk::csr_sddmm_kernel<T>), dim3((unsigned)(((long)nnz + 255) / 256)), dim3(256), 0,      \
                       (hipStream_t)stream, row_of, col, U, W, G, nnz, B, C, ldu, sU, ldw, sW, sG);             \
    XK_LAUNCH_CHECK();                                                                                          \
    return XK_OK;                                                                                               \
  }

XK_DEFINE_SPARSE(f64, double)
XK_DEFINE_SPARSE(f32, float)

/* complex: pointers to interleaved (re, im), every count, pitch and stride in whole complex elements */
#define XK_DEFINE_SPARSE_C(SUF, T)                                                                               \
  int xk_csr_mm_##SUF(const int* ptr, const int* idx, const int* perm, const T* val, long sV, const int* rows,    \
                      const int* bin_off, const int* seg_q, const int* seg_off, int nseg, T* ws, const T* X,     \
                      T* Y, int B, int Mout, int Nin, int C, long ldx, long sX, long ldy, long sY, int conj_val, \
                      void* stream) {                                                                            \
    typedef xk::cel<T> E;                                                                                        \
    if (B < 0 || Mout < 0 || Nin < 0 || C < 0 || sV < 0 || sX < 0 || sY < 0 || nseg < 0) return XK_ERR_ARG;     \
    if (B == 0 || Mout == 0 || C == 0) return XK_OK;                                                             \
    if (!bin_off || bin_off[0] != 0 || bin_off[xk::CSR_NBINS] != Mout) return XK_ERR_ARG;                       \
    for (int q = 0; q < xk::CSR_NBINS; ++q)                                                                      \
      if (bin_off[q + 1] < bin_off[q]) return XK_ERR_ARG;                                                        \
    if (bin_off[4] > bin_off[3] && (nseg < bin_off[4] - bin_off[3] || !seg_q || !seg_off || !ws))               \
      return XK_ERR_ARG;                                                                                         \
    if (ldy < Mout || ldx < Nin) return XK_ERR_UNSUPPORTED;                                                      \
    if (B > 1 && sY < (long)C * ldy) return XK_ERR_UNSUPPORTED;  /* overlapping outputs */                       \
    return xk::csr_mm_c<T>(ptr, idx, perm, (const E*)val, sV, conj_val ? 1 : 0, rows, bin_off, seg_q, seg_off,   \
                           nseg, (E*)ws, (const E*)X, (E*)Y, B, C, ldx, sX, ldy, sY, (hipStream_t)stream);       \
  }                                                                                                              \
  int xk_csr_sddmm_##SUF(const int* row_of, const int* col, const T* U, const T* W, T* G, int nnz, int B,         \
                         int M, int N, int C, long ldu, long sU, long ldw, long sW, long sG, void* stream) {      \
    typedef xk::cel<T> E;                                                                                        \
    if (nnz < 0 || B < 0 || M < 0 || N < 0 || C < 0 || sU < 0 || sW < 0 || sG < 0) return XK_ERR_ARG;            \
    if (nnz == 0 || B == 0) return XK_OK;                                                                        \
    if (C > 0 && (ldu < M || ldw < N)) return XK_ERR_UNSUPPORTED;                                                \
    if (B > 1 && sG < nnz) return XK_ERR_UNSUPPORTED;                                                            \
    if (C == 0) {                                                                                                \
      for (int b = 0; b < B; ++b) {                                                                              \
        hipError_t e = hipMemsetAsync((E*)G + (long)b * sG, 0, sizeof(E) * (size_t)nnz, (hipStream_t)stream);   \
        if (e != hipSuccess) return (int)e;                                                                      \
      }                                                                                                          \
      return XK_OK;                                                                                              \
    }                                                                                                            \
    hipLaunchKernelGGL((xk::csr_sddmm_c_kernel<T>), dim3((unsigned)(((long)nnz + 255) / 256)), dim3(256), 0,     \
                       (hipStream_t)stream, row_of, col, (const E*)U, (const E*)W, (E*)G, nnz, B, C, ldu, sU,   \
                       ldw, sW, sG);                                                                             \
    XK_LAUNCH_CHECK();                                                                                           \
    return XK_OK;                                                                                                \
  }

XK_DEFINE_SPARSE_C(c128, double)
XK_DEFINE_SPARSE_C(c64, float)

}  // extern "C"
