/* xitorch_amd — C ABI of the MI355X (gfx950) native hot path.
 *
 * One shared library, libxitorch_amd.so, built by `__graft_entry__.build()`
 * with `hipcc --offload-arch=gfx950 -shared -fPIC`.  The reference (xitorch,
 * pure Python) has no FFI; these entry points sit *under* its three Python
 * plug-in contracts (operator / method / functional) and are
 * what a reference-side binding would call (INTEGRATION.md shows the ctypes
 * stubs).  Each function names the reference code it replaces.
 *
 * Conventions
 *  - extern "C", plain pointers and sizes; no torch types.
 *  - every function returns int: 0 ok, <0 argument/shape error
 *    (XK_ERR_ARG=-1, XK_ERR_UNSUPPORTED=-2), >0 a hipError_t passed through.
 *  - all pointers are DEVICE pointers, borrowed for the duration of the
 *    stream-ordered work; nothing is allocated on behalf of the caller — a
 *    `*_workspace_elems` query precedes calls that need scratch.
 *  - every launch goes to the `stream` argument (a hipStream_t passed as
 *    void*; NULL = the default stream).  No hidden global state: nothing in
 *    the library is process-wide and writable — launch shapes and measurement
 *    switches are ARGUMENTS (0 = the shipped default), the only objects with a
 *    lifetime are the ones the caller creates and hands back (CU-masked streams,
 *    RCCL communicators).  Two threads / two devices of one process share nothing.
 *  - PANEL-MAJOR vectors: a block of P vectors of length N is stored (P, N),
 *    pitch `ld*` between vectors, `s*` between batch members.  This is the
 *    reference's "Fortran order" (N, P) view (_utils/tensor.py:21-32).
 *  - `_f64` / `_f32` suffix = element type.
 */
#ifndef XITORCH_AMD_H
#define XITORCH_AMD_H

#ifdef __cplusplus
extern "C" {
#endif

#define XK_OK 0
#define XK_ERR_ARG (-1)
#define XK_ERR_UNSUPPORTED (-2)

/* library/ABI version (bumped when a signature changes) */
int xk_abi_version(void);

/* ---- CU-masked stream (no reference counterpart: the reference runs everything on one stream) ----
 * Creates a HIP stream whose kernels may use all but `reserve_cus` compute units of `device`
 * (hipExtStreamCreateWithCUMask).  The eigensolver launches the HBM-bound panel product on it so that the
 * latency-bound small kernels of the other half of the batch find free CUs (linalg.symeig davidson,
 * option overlap).  The caller owns the stream (xk_stream_destroy). */
/* measurement utility: read bytes/pitch_bytes rows of pitch_bytes (16 B multiples, 16 B aligned) of device memory once
 * in the panel kernels' tile walk, no arithmetic; `scratch`: >= 4 KiB of device memory or NULL.  Timed by the caller
 * (bench.py: the practical streaming ceiling of the operator batch) */
int xk_stream_read(const void* src, long bytes, long pitch_bytes, void* scratch, void* stream);
int xk_stream_create_cu_masked(int device, int reserve_cus, void** stream_out);
/* the same with the bits to clear chosen by `pattern`: 0 = the last reserve_cus bits of the linear mask (what
 * xk_stream_create_cu_masked does), 1 = every (units / reserve_cus)-th bit */
int xk_stream_create_cu_masked_pattern(int device, int reserve_cus, int pattern, void** stream_out);
/* measurement utility: `workgroups` one-wave workgroups on `stream`, each spinning `spin_cycles`; hist16[x] = workgroups
 * that ran on XCD x, units128[8 x + w] = bit set of the (SE, SH, CU) ids seen there (device memory, zeroed by the call) */
int xk_probe_xcc(unsigned* hist16, unsigned* units128, int workgroups, int spin_cycles, void* stream);
int xk_stream_destroy(void* stream);

/* ---- K1: batched dense operator-panel product --------------------------------
 * trans=0:  Y[b,c,i] = sum_j A[b,i,j] X[b,c,j]     i<M, j<N
 * trans=1:  Y[b,c,j] = sum_i A[b,i,j] X[b,c,i]
 * Replaces MatrixLinearOperator._mv/_mm/_rmv/_rmm (xitorch/_core/linop.py:692-702)
 * on the eigensolver panel product (xitorch/_impls/linalg/symeig.py:163,221) and
 * the Krylov operator apply (xitorch/_impls/linalg/solve.py:571-572).  Passing a
 * basis (B,k,N) as A computes Gram / Rayleigh blocks (symeig.py:170,
 * _utils/tensor.py:15).
 * A: (B,M,N) row-major, row pitch lda, batch pitch sA (sA=0 broadcasts one operator).
 * ws: scratch for trans=1 of xk_dense_mm_workspace_elems() elements (may be NULL for trans=0).
 * rows_hint: 0 = auto (tuning knob: rows per wave 4/8/16); stagger: 1 = de-phase row sweeps. */
long xk_dense_mm_workspace_elems(int B, int M, int N, int P, int trans);
int xk_dense_mm_f64(const double* A, const double* X, double* Y, double* ws, long ws_elems,
                    int B, int M, int N, int P, long lda, long sA, long ldx, long sX,
                    long ldy, long sY, int trans, int rows_hint, int stagger, void* stream);
int xk_dense_mm_f32(const float* A, const float* X, float* Y, float* ws, long ws_elems,
                    int B, int M, int N, int P, long lda, long sA, long ldx, long sX,
                    long ldy, long sY, int trans, int rows_hint, int stagger, void* stream);

/* ---- K1s: the same product for EXACTLY symmetric storage, reading only the upper triangle ------
 * Y[b,c,:] = A_b X[b,c,:] with A_b == A_b^T bit for bit (the caller's promise): every tile on or
 * above the diagonal is streamed once and feeds both y_I += A_IJ x_J and y_J += A_IJ^T x_I, i.e.
 * about half the HBM traffic of xk_dense_mm.  Used for the eigensolver panel product
 * (xitorch/_impls/linalg/symeig.py:163,221; symeig requires a Hermitian operator, linalg/symeig.py:103).
 * N must be a multiple of the 16 B vector width; ws: xk_dense_symm_workspace_elems(B,N,P,sizeof(T)). */
long xk_dense_symm_workspace_elems(int B, int N, int P, int elem_size);
/* Results are run-to-run bit-identical: the four waves of a workgroup add into the LDS row accumulator in a fixed
 * order (phase rotation with barriers), partial slots are folded in a fixed order.
 * opts (results never depend on the launch shape chosen through it, only — for bits 5, 8..15 and 2/3 — on the fixed
 * summation order of the partial slots): bit 0 plain instead of non-temporal stores of the row / column partials, bit 1
 * plain instead of non-temporal loads in the fold, bits 8..15 column slabs per workgroup run (0 = 1; row partials per row
 * tile = ceil(slabs / run), at most 64); bit 2: 512-row tiles (fp64), bit 3: 1024-row tiles — without either the library
 * picks 512 rows for fp64 launches of fewer than 2200 workgroups (<= 16 operators of order 16384: +1 %);
 * bit 4 (round 5): RESIDENT launch — bits 16..27 workgroups (0 = two per compute unit of the device) take the runs from a
 * queue (the last 64 bytes of `ws`, reset by the call in stream order) until it is empty: bit-identical to the
 * one-workgroup-per-run launch; a second resident launch on another stream moves into the slots this one's tail frees
 * (the eigensolver's two batch groups: 217.6 -> 211.9 ms per BASELINE configs[1] call);
 * bit 5 (round 5, fp64 only): 8-wave workgroups on 2048 x 2048 tiles, one workgroup per compute unit (with bit 4: half
 * the bits-16..27 count) — half the partial-sum bytes; worth it from ~8 tiles per compute unit alone on the device, ~2
 * inside the pipeline (-> 206.7 ms).  The Python host picks bits 4 / 5 per launch (xitorch_amd.kernels.k1s_auto_opts). */
int xk_dense_symm_f64(const double* A, const double* X, double* Y, double* ws, long ws_elems, int B,
                      int N, int P, long lda, long sA, long ldx, long sX, long ldy, long sY, int opts, void* stream);
int xk_dense_symm_f32(const float* A, const float* X, float* Y, float* ws, long ws_elems, int B, int N,
                      int P, long lda, long sA, long ldx, long sX, long ldy, long sY, int opts, void* stream);
/* The two halves of the call above as separate launches (P <= 6): the tile kernel leaves per-slab / per-row-tile
 * partial sums in `ws`, the fold adds them into Y.  The eigensolver's two-group pipeline runs the tile kernels of
 * both groups back to back on one (CU-masked) stream and each fold on its group's own stream, off that
 * critical path; `ws` must stay untouched between the two calls, and both take the same `opts`. */
int xk_dense_symm_tiles_f64(const double* A, const double* X, double* ws, long ws_elems, int B, int N, int P,
                            long lda, long sA, long ldx, long sX, int opts, void* stream);
int xk_dense_symm_tiles_f32(const float* A, const float* X, float* ws, long ws_elems, int B, int N, int P,
                            long lda, long sA, long ldx, long sX, int opts, void* stream);
int xk_dense_symm_fold_f64(double* Y, const double* ws, long ws_elems, int B, int N, int P, long ldy, long sY,
                           int opts, void* stream);
int xk_dense_symm_fold_f32(float* Y, const float* ws, long ws_elems, int B, int N, int P, long ldy, long sY,
                           int opts, void* stream);

/* ---- K1sw: the same product (exactly symmetric storage, upper triangle streamed once) for WIDE panels on the matrix
 * cores: 9 <= P <= 16 columns, fp32 — BASELINE configs[4]'s 16-column eigen-block (xitorch/_core/linop.py:695-696 inside
 * _impls/linalg/symeig.py:163,221).  Every 64-row x 128-byte sub-tile on or above the diagonal is loaded once, turned
 * through LDS per wave and feeds y_I += A_IJ x_J and y_J += A_IJ^T x_I through v_mfma_f32_16x16x4_f32; row / column sums
 * leave as partials in `ws` (one wave = one 512-row x 256-column tile, no atomics, no block barriers) and a fold adds the
 * slots that exist in fixed order: run-to-run bit-identical.  N must be a multiple of 64; the 64 x 64 diagonal blocks are
 * read whole.  ws: xk_dense_symm_wide_workspace_elems(B, N).  _tiles / _fold: the two launches separately (the
 * eigensolver's two-group pipeline), `ws` untouched in between.  opts: 0 = one wave per tile (above); 1 = the
 * workgroup-cooperative form (three waves per SIMD, four 128-column strips per workgroup sharing their row sums
 * through LDS; + 2 = raised wave priority around its MFMA block; 3 is what the Python host passes: 3.58 ms against 3.97 ms
 * for 8 x 32768^2, profiles/r04_k1sw_forms.jsonl); + 4 (round 5, with 1): resident launch — bits 16..27 workgroups (0 =
 * three per compute unit) take the super-tiles from a queue in the last 64 bytes of `ws` (reset by the call), bit-identical
 * to opts 1 / 3; + 8 (round 6, with 1, not with 2 / 4; 9 is what the Python host passes): the column part straight from the
 * load registers (a load = 4 rows x 256 B in the column part's B-operand layout), the row part through ds_write_b128 /
 * ds_read_b128 one block behind, a ring of four 16 x 64 blocks = 16 KB in flight per wave, two waves per SIMD — same
 * work split, partial slots and fold as opts 1: 3.62 -> 2.94 ms for 8 x 32768^2 (profiles/r06_k1sw_forms.json).
 * _tiles and _fold of one product take the same opts. */
long xk_dense_symm_wide_workspace_elems(int B, int N);
int xk_dense_symm_wide_f32(const float* A, const float* X, float* Y, float* ws, long ws_elems, int B, int N, int P,
                           long lda, long sA, long ldx, long sX, long ldy, long sY, int opts, void* stream);
int xk_dense_symm_wide_tiles_f32(const float* A, const float* X, float* ws, long ws_elems, int B, int N, int P,
                                 long lda, long sA, long ldx, long sX, int opts, void* stream);
int xk_dense_symm_wide_fold_f32(float* Y, const float* ws, long ws_elems, int B, int N, int P, long ldy, long sY,
                                int opts, void* stream);

/* ---- K1w: wide panels on the matrix cores (MFMA) --------------------------------------------
 * Y[b,c,n] = sum_i A[b,i,n] Xrm[b,i,c]  (= A^T X; = A X for a Hermitian operator), c < P <= 32, in ONE
 * pass over A (v_mfma_f32_32x32x2_f32 / v_mfma_f64_16x16x4_f64, exact FMA chains).  Xrm is ROW-major
 * (B, M, PP) with PP = xk_dense_wide_padded_width(P) zero-padded columns; Y panel-major (B, P, N).
 * Requires N % 128 == 0 (fp32) / N % 32 == 0 (fp64).  Many-column torch.matmul(mat, x) of
 * MatrixLinearOperator._mm/_rmm (xitorch/_core/linop.py:695-702), e.g. solve with ncols = 50
 * (benchmarks/benchmarks_solve.py:11-15). */
long xk_dense_wide_workspace_elems(int B, int M, int N, int P, int elem_size);
int xk_dense_wide_padded_width(int P, int elem_size);
int xk_dense_wide_f32(const float* A, const float* Xrm, float* Y, float* ws, long ws_elems, int B, int M,
                      int N, int P, long lda, long sA, long ldxr, long sXr, long ldy, long sY, void* stream);
int xk_dense_wide_f64(const double* A, const double* Xrm, double* Y, double* ws, long ws_elems, int B, int M,
                      int N, int P, long lda, long sA, long ldxr, long sXr, long ldy, long sY, void* stream);

/* ---- K1wr: wide panels in the ROW orientation (no transposed copy, no MFMA) -----------------------
 * Y[b,c,i] = sum_j A[b,i,j] X[b,c,j], any P (32 columns per pass over A): `torch.matmul(mat, x)` of a
 * non-Hermitian MatrixLinearOperator with many right-hand sides (xitorch/_core/linop.py:695-696;
 * benchmarks/benchmarks_solve.py:11-15; the BiCGStab / GMRES applies of a multi-RHS solve,
 * _impls/linalg/solve.py:278,284).  Coalesced 64-row sub-tiles are turned through LDS so that every lane walks
 * along its own row with wave-uniform (scalar) panel values: no cross-lane reduction.  X, Y panel-major;
 * requires N, lda, ldx multiples of the 16 B vector width (else XK_ERR_UNSUPPORTED: use xk_dense_mm).
 * ws: xk_dense_rows_wide_workspace_elems() elements (0 when the contraction is not split). */
long xk_dense_rows_wide_workspace_elems(int B, int M, int N, int P, int elem_size);
int xk_dense_rows_wide_f64(const double* A, const double* X, double* Y, double* ws, long ws_elems, int B, int M,
                           int N, int P, long lda, long sA, long ldx, long sX, long ldy, long sY, void* stream);
int xk_dense_rows_wide_f32(const float* A, const float* X, float* Y, float* ws, long ws_elems, int B, int M, int N,
                           int P, long lda, long sA, long ldx, long sX, long ldy, long sY, void* stream);

/* ---- basis maintenance of the block eigensolver (K2/K4/K5/K6) ------------------------------
 * Panels must be PADDED: pitch a multiple of 16 B and >= N rounded up to 16 B, pads zero.
 *
 * xk_lincomb:  Out[b,c,:] = beta*Out[b,c,:] + alpha * sum_{a<k} C[b,a,c] V[b,a,:]
 *   C element (b,a,c) at C[b*sC + a*sCa + c*sCc].  Replaces the Ritz rotations `V @ Y`
 *   (xitorch/_impls/linalg/symeig.py:178,181) and the projection step standing in for the full
 *   CholeskyQR `tallqr` (xitorch/_utils/tensor.py:15-18). */
int xk_lincomb_f64(const double* V, const double* C, double* Out, int B, int k, int N, int P,
                   long ldv, long sV, long sC, long sCa, long sCc, long ldo, long sO,
                   double alpha, double beta, void* stream);
int xk_lincomb_f32(const float* V, const float* C, float* Out, int B, int k, int N, int P,
                   long ldv, long sV, long sC, long sCa, long sCc, long ldo, long sO,
                   double alpha, double beta, void* stream);
/* xk_ritz_residual (fused K4/K5, symeig.py:178-188,207):
 *   X[b,c,:] = sum_a Y[b,a,c] V[b,a,:];  AX likewise from AV;  Tn[b,c,:] = -(AX - lam[b,c] X);
 *   rmax[b] = max(rmax[b], max |AX - lam X|)  (caller zeroes rmax; NaN is reported as +inf). */
int xk_ritz_residual_f64(const double* V, const double* AV, const double* Y, const double* lam,
                         double* X, double* Tn, double* rmax, int B, int k, int N, int P,
                         long ldv, long sV, long ldav, long sAV, long sY, long sYa, long sYc,
                         long sLam, long ldx, long sX, long ldt, long sT, void* stream);
int xk_ritz_residual_f32(const float* V, const float* AV, const float* Y, const float* lam,
                         float* X, float* Tn, float* rmax, int B, int k, int N, int P,
                         long ldv, long sV, long ldav, long sAV, long sY, long sYa, long sYc,
                         long sLam, long ldx, long sX, long ldt, long sT, void* stream);
/* xk_panel_chol: G[b] (P x P, pitch ldg) = R^T R, W[b] = R^-1 compact (B,P,P) row-major; info[b] =
 *   1+index of the first non-positive pivot, 0 if none (tensor.py:16-17; P <= 32). */
int xk_panel_chol_f64(const double* G, double* W, int* info, int B, int P, long ldg, long sG, void* stream);
int xk_panel_chol_f32(const float* G, float* W, int* info, int B, int P, long ldg, long sG, void* stream);
/* xk_panel_transform: in place Tp[b,c,:] <- sum_{a<=c} W[b,a,c] Tp[b,a,:]  (tensor.py:18). */
int xk_panel_transform_f64(double* Tp, const double* W, int B, int P, int N, long ldt, long sT, void* stream);
int xk_panel_transform_f32(float* Tp, const float* W, int B, int P, int N, long ldt, long sT, void* stream);

/* ---- Davidson diagonal preconditioner (extension; the reference's davidson has none, `t = -resid`,
 * xitorch/_impls/linalg/symeig.py:206-207) ------------------------------------------------------
 * t[b,c,n] /= (d[b,n] - lam[b,c]*m[b,n]) with |denominator| >= floor (sign kept); m == NULL: identity.
 * t: (B,P,ld) panel, d/m: (B,N) with batch strides sD/sM (0 broadcasts), lam: (B,>=P) unit stride. */
int xk_diag_precond_f64(double* t, const double* d, const double* m, const double* lam, int B, int N, int P,
                        long ldt, long sT, long sD, long sM, long sLam, double floor_, void* stream);
int xk_diag_precond_f32(float* t, const float* d, const float* m, const float* lam, int B, int N, int P,
                        long ldt, long sT, long sD, long sM, long sLam, double floor_, void* stream);

/* ---- group status of a Davidson step in one launch (native_eig._Group.small; the reference reads
 * `resid.abs().max()` on the host, symeig.py:190-197): status[0] = max_b rmax[b] (NaN if any is NaN),
 * status[1] = max_b info[b] (panel Cholesky flags), status[2] = max_b flag[b] (K3t self-check; flag may be NULL);
 * orth (B, may be NULL): the a-posteriori guard values left by xk_ritz_guard: status[4] = max_b orth[b] (NaN counts as
 * infinite), orth is re-zeroed; status then has 5 doubles (status[3], the chain's condition estimate, is not written) */
int xk_group_status_f64(const double* rmax, const int* info, const int* flag, double* orth, double* status, int B,
                        void* stream);
int xk_group_status_f32(const float* rmax, const int* info, const int* flag, float* orth, double* status, int B,
                        void* stream);

/* ---- K3: batched small symmetric eigensolver (LDS-resident parallel Jacobi) -----------------
 * Lowest (uppest=0) / uppermost (uppest=1) p eigenpairs of B symmetric k x k matrices (lower
 * triangle read, pitch ldt, batch pitch sT), eigenvalues ascending: lam (B,p), Y (B,p,k) with
 * Y[b,c,:] the c-th eigenvector.  Replaces torch.linalg.eigh + _take_eigpairs
 * (symeig.py:174-175, 255-264).  k <= 128, p <= 16.  ws: xk_small_eigh_workspace_elems elements.
 * sweeps[b]: Jacobi sweeps taken (== max_sweeps: not converged); there is no other failure flag.
 * Scale-safe: each matrix is scaled inside the kernel by the exact power of two that brings max|T| to
 * [1, 2) and lam is scaled back, so any finite T whose entries are representable gives the same relative
 * accuracy (and in-range T the same bits as without the scaling); a zero matrix returns lam = 0 with unit
 * vectors; the result for a matrix that holds a NaN or an infinity is undefined. */
long xk_small_eigh_workspace_elems(int B, int k, int max_sweeps);
int xk_small_eigh_f64(const double* T, double* lam, double* Y, double* ws, long ws_elems, int* sweeps,
                      int B, int k, int p, int uppest, int max_sweeps, long ldt, long sT, void* stream);
int xk_small_eigh_f32(const float* T, float* lam, float* Y, float* ws, long ws_elems, int* sweeps,
                      int B, int k, int p, int uppest, int max_sweeps, long ldt, long sT, void* stream);

/* ---- K3t: the same p eigenpairs by Householder tridiagonalisation + bisection + inverse iteration ------
 * (the LAPACK dsyevx route), one workgroup per matrix, LDS-resident: the O(k^3) work is ONE tridiagonalisation
 * instead of ~8 Jacobi sweeps over the whole matrix, which is what the Davidson loop — interested in p << k
 * pairs only (symeig.py:174-175, 255-264) — needs.  Same outputs as xk_small_eigh_*; info[b] != 0 flags a
 * batch member whose result failed the kernel's residual / orthogonality check (caller re-runs on the Jacobi
 * kernel).  Returns XK_ERR_UNSUPPORTED when xk_small_eigh_tri_lds_bytes(k, p, elem_size) exceeds 160 KiB.
 * threads: workgroup size, a multiple of 64 in [64, 1024], 0 = the measured default (512); profile: NULL, or a device
 * buffer of >= 8 int64 that receives the cycle counter at the phase boundaries of block 0 (measurements). */
long xk_small_eigh_tri_lds_bytes(int k, int p, int elem_size);
int xk_small_eigh_tri_f64(const double* T, double* lam, double* Y, int* info, int B, int k, int p, int uppest,
                          long ldt, long sT, int threads, long long* profile, void* stream);
int xk_small_eigh_tri_f32(const float* T, float* lam, float* Y, int* info, int B, int k, int p, int uppest, long ldt,
                          long sT, int threads, long long* profile, void* stream);

/* ---- banded operator (DIA storage) -------------------------------------------------------------
 * band (B, 2*hb+1, N), band[b,d,i] = A_b[i, i+d-hb]; entries outside the matrix are ignored.
 * trans=0: Y[b,c,i] = sum_d band[b,d,i] X[b,c,i+d-hb];  trans=1: the transposed operator.
 * sBand = 0 broadcasts one operator over the batch.  Operator of BASELINE configs[2]; in the
 * reference a user writes it as a custom `_mv` (cf. ALarge, xitorch/_tests/test_linop_fcns.py:129-150). */
int xk_banded_mm_f64(const double* band, const double* X, double* Y, int B, int N, int hb, int C,
                     long sBand, long ldx, long sX, long ldy, long sY, int trans, void* stream);
int xk_banded_mm_f32(const float* band, const float* X, float* Y, int B, int N, int hb, int C,
                     long sBand, long ldx, long sX, long ldy, long sY, int trans, void* stream);

/* ---- CSR sparse operator (one pattern shared by the batch) ---------------------------------------
 * xk_csr_mm:    Y[b,c,i] = sum_{ptr[i] <= k < ptr[i+1]} val[b*sV + (perm ? perm[k] : k)] X[b,c,idx[k]]
 *   for the Mout rows listed in rows[0 .. Mout): rows is a permutation of 0 .. Mout-1 grouped into 4 bins by row
 *   length, bin q = rows[bin_off[q] .. bin_off[q+1]) (bin_off: HOST array of 5 ints, bin_off[4] = Mout).  Bins 0-2
 *   are served by 1 / 8 / 64 lanes per row; the rows of bin 3 (nlong = bin_off[4] - bin_off[3]) are cut into
 *   segments of xk_csr_seg_len() entries: long row q owns segments seg_off[q] .. seg_off[q+1] (seg_off: nlong+1
 *   device ints), seg_q[s] = the long row of segment s (nseg device ints), and ws (device, >= B * min(C, 8) * nseg
 *   elements) holds the segment sums, added per row in segment order.  The transposed operator is the same call on
 *   the CSC view (ptr = column pointers, idx = row indices, perm = CSR position of each CSC entry).  Fixed summation
 *   order, no atomics.  sV = 0 broadcasts one set of values over the batch.  X (B, C, ldx >= Nin),
 *   Y (B, C, ldy >= Mout) panel-major; only the Mout leading entries of each Y vector are written.
 * xk_csr_sddmm: G[b,k] = sum_c U[b,c,row_of[k]] W[b,c,col[k]]  (the values gradient; transposed apply: swap U and
 *   W; batch dims the values lack are folded into the columns by the caller).  U (B, C, ldu >= M),
 *   W (B, C, ldw >= N).  Indices are int32 and must be in range (checked once by the operator). */
int xk_csr_seg_len(void);
int xk_csr_mm_f64(const int* ptr, const int* idx, const int* perm, const double* val, long sV, const int* rows,
                  const int* bin_off, const int* seg_q, const int* seg_off, int nseg, double* ws, const double* X,
                  double* Y, int B, int Mout, int Nin, int C, long ldx, long sX, long ldy, long sY, void* stream);
int xk_csr_mm_f32(const int* ptr, const int* idx, const int* perm, const float* val, long sV, const int* rows,
                  const int* bin_off, const int* seg_q, const int* seg_off, int nseg, float* ws, const float* X,
                  float* Y, int B, int Mout, int Nin, int C, long ldx, long sX, long ldy, long sY, void* stream);
int xk_csr_sddmm_f64(const int* row_of, const int* col, const double* U, const double* W, double* G, int nnz, int B,
                     int M, int N, int C, long ldu, long sU, long ldw, long sW, long sG, void* stream);
int xk_csr_sddmm_f32(const int* row_of, const int* col, const float* U, const float* W, float* G, int nnz, int B,
                     int M, int N, int C, long ldu, long sU, long ldw, long sW, long sG, void* stream);
/* Complex values (c128 / c64): the same two products on interleaved (re, im) data, the same row bins, segments and
 *   fixed summation order (re and im go through the same tree).  val, ws, X, Y, U, W, G point to interleaved complex;
 *   sV, ldx, sX, ldy, sY, ldu, sU, ldw, sW, sG and the size of ws count WHOLE COMPLEX ELEMENTS.  Every element is
 *   read and written as one 16-byte (c128) / 8-byte (c64) access, so the base pointers must be aligned to one complex
 *   element; a slice of a complex array always is, and there is no alignment contract beyond that.
 * xk_csr_mm_c*:    Y[b,c,i] = sum_k op(val[b*sV + (perm ? perm[k] : k)]) X[b,c,idx[k]], op = conj when conj_val != 0.
 *   A x is the CSR view with conj_val = 0, A^H x the CSC view with conj_val = 1 (the values are never copied).
 * xk_csr_sddmm_c*: G[b,k] = sum_c U[b,c,row_of[k]] conj(W[b,c,col[k]])  (the values gradient "gy x^H" sampled at the
 *   pattern; adjoint apply: U = x, W = grad y). */
int xk_csr_mm_c128(const int* ptr, const int* idx, const int* perm, const double* val, long sV, const int* rows,
                   const int* bin_off, const int* seg_q, const int* seg_off, int nseg, double* ws, const double* X,
                   double* Y, int B, int Mout, int Nin, int C, long ldx, long sX, long ldy, long sY, int conj_val,
                   void* stream);
int xk_csr_mm_c64(const int* ptr, const int* idx, const int* perm, const float* val, long sV, const int* rows,
                  const int* bin_off, const int* seg_q, const int* seg_off, int nseg, float* ws, const float* X,
                  float* Y, int B, int Mout, int Nin, int C, long ldx, long sX, long ldy, long sY, int conj_val,
                  void* stream);
int xk_csr_sddmm_c128(const int* row_of, const int* col, const double* U, const double* W, double* G, int nnz, int B,
                      int M, int N, int C, long ldu, long sU, long ldw, long sW, long sG, void* stream);
int xk_csr_sddmm_c64(const int* row_of, const int* col, const float* U, const float* W, float* G, int nnz, int B,
                     int M, int N, int C, long ldu, long sU, long ldw, long sW, long sG, void* stream);

/* ---- operator gradients of the implicit backward passes (streaming writes) -----------------------
 * The backward of solve / symeig / rootfinder ends with a VJP through the operator apply
 * (`loss = -A.mm(x)`; `autograd.grad(loss, params, v)`: xitorch/linalg/solve.py:188-195,
 * linalg/symeig.py:374-379, optimize/rootfinder.py:352-362); in the reference that is torch's matmul / slice
 * backward.  U, W panel-major (B, C, N), pitches ld*, batch pitches s*.
 * xk_banded_grad:  G[b,d,i] (+)= sum_c U[b,c,i] W[b,c,i+d-hb]   (DIA band gradient; trans apply: swap U and W)
 * xk_dense_outer:  G[b,i,j] (+)= sum_c U[b,c,i] W[b,c,j]        (i < M, j < N, row pitch ldg)
 * accumulate = 1 adds into G. */
int xk_banded_grad_f64(const double* U, const double* W, double* G, int B, int N, int hb, int C, long ldu,
                       long sU, long ldw, long sW, long sG, int accumulate, void* stream);
int xk_banded_grad_f32(const float* U, const float* W, float* G, int B, int N, int hb, int C, long ldu, long sU,
                       long ldw, long sW, long sG, int accumulate, void* stream);
int xk_dense_outer_f64(const double* U, const double* W, double* G, int B, int M, int N, int C, long ldu,
                       long sU, long ldw, long sW, long ldg, long sG, int accumulate, void* stream);
int xk_dense_outer_f32(const float* U, const float* W, float* G, int B, int M, int N, int C, long ldu, long sU,
                       long ldw, long sW, long ldg, long sG, int accumulate, void* stream);

/* ---- fused Krylov-loop kernels (K7-K9, K11; xitorch/_impls/linalg/solve.py:143-180, 272-314) ----
 * Vectors are (S, ld) arrays: S systems (batch member x column), pitch ld (16 B multiple, pads 0).
 * P* are partial-sum buffers (S, xk_kry_max_partials()); nblk <= that many blocks per system.
 * Per-system scalars (rho, alpha, omega) are device arrays of S elements.  eps = the reference's
 * `_safedenom` replacement of exact zeros (solve.py:437-439). */
int xk_kry_max_partials(void);
/* P1[s] <- partials of <x1,y1>, P2[s] (optional) <- <x2,y2>; if E != NULL first y1 -= E[s]*shiftz */
int xk_kry_dots_f64(const double* x1, double* y1, const double* x2, const double* y2, const double* shiftz,
                    const double* E, double* P1, double* P2, int S, int N, long ld, int nblk, void* stream);
int xk_kry_dots_f32(const float* x1, float* y1, const float* x2, const float* y2, const float* shiftz,
                    const float* E, float* P1, float* P2, int S, int N, long ld, int nblk, void* stream);
/* p = r + beta (p - omega v), beta = rho_new/safe(rho_old) * alpha/safe(omega); rho_store <- rho_new
 * (rho_old and rho_store must be different arrays); first=1: p = r  (solve.py:273-276) */
int xk_bicg_p_f64(const double* r, double* p, const double* v, const double* Prho_new, const double* rho_old,
                  const double* alpha, const double* omega, double* rho_store, int S, int N, long ld,
                  int nblk, double eps, int first, void* stream);
int xk_bicg_p_f32(const float* r, float* p, const float* v, const float* Prho_new, const float* rho_old,
                  const float* alpha, const float* omega, float* rho_store, int S, int N, long ld,
                  int nblk, double eps, int first, void* stream);
/* s = r - alpha v, alpha = rho / safe(<r0,v>)  (solve.py:279,282) */
int xk_bicg_s_f64(const double* r, const double* v, double* s, const double* rho, const double* Pr0v,
                  double* alpha_store, int S, int N, long ld, int nblk, double eps, void* stream);
int xk_bicg_s_f32(const float* r, const float* v, float* s, const float* rho, const float* Pr0v,
                  float* alpha_store, int S, int N, long ld, int nblk, double eps, void* stream);
/* omega = <Kt,Ks>/safe(<Kt,Kt>); xout = x + alpha*yd + omega*zd; unless skip_r: r = s - omega t and
 * Prr <- |r|^2, Prho <- <r0,r>  (solve.py:286-297) */
int xk_bicg_final_f64(const double* x, double* xout, const double* yd, const double* zd, const double* s,
                      const double* t, double* r, const double* r0, const double* alpha, const double* Pts,
                      const double* Ptt, double* omega_store, double* Prr, double* Prho, int S, int N,
                      long ld, int nblk, double eps, int skip_r, void* stream);
int xk_bicg_final_f32(const float* x, float* xout, const float* yd, const float* zd, const float* s,
                      const float* t, float* r, const float* r0, const float* alpha, const float* Pts,
                      const float* Ptt, float* omega_store, float* Prr, float* Prho, int S, int N,
                      long ld, int nblk, double eps, int skip_r, void* stream);
/* r = b - y; Prr <- |r|^2; Prho (optional) <- <r0,r> (or |r|^2 when r0 is NULL)  (solve.py:148-149, 290-291) */
int xk_kry_resid_f64(const double* b, const double* y, double* r, const double* r0, double* Prr,
                     double* Prho, int S, int N, long ld, int nblk, void* stream);
int xk_kry_resid_f32(const float* b, const float* y, float* r, const float* r0, float* Prr, float* Prho,
                     int S, int N, long ld, int nblk, void* stream);
/* alpha = <r,z>/safe(<p,Ap>); xout = x + alpha p; unless skip_r: r -= alpha Ap, Prr <- |r|^2  (solve.py:144-155) */
int xk_cg_update_f64(const double* x, double* xout, const double* p, const double* Ap, double* r,
                     const double* Prz, const double* PpAp, double* Prr, int S, int N, long ld, int nblk,
                     double eps, int skip_r, void* stream);
int xk_cg_update_f32(const float* x, float* xout, const float* p, const float* Ap, float* r, const float* Prz,
                     const float* PpAp, float* Prr, int S, int N, long ld, int nblk, double eps, int skip_r,
                     void* stream);
/* p = z + beta p, beta = <r,z>_new / safe(<r,z>_old)  (solve.py:171-173) */
int xk_cg_p_f64(const double* z, double* p, const double* Prz_new, const double* Prz_old, int S, int N,
                long ld, int nblk, double eps, void* stream);
int xk_cg_p_f32(const float* z, float* p, const float* Prz_new, const float* Prz_old, int S, int N, long ld,
                int nblk, double eps, void* stream);
/* rnorm[s] = sqrt(sum Prr[s,:]); status[0] = max_s rnorm (NaN -> +inf), status[1] = #{s: !(rnorm < stop[s])}
 * (the stopping test of solve.py:157,166,301,310 — read back once per iteration) */
int xk_kry_status_f64(const double* Prr, const double* stop, double* rnorm, double* status, int S, int nblk,
                      void* stream);
int xk_kry_status_f32(const float* Prr, const float* stop, float* rnorm, double* status, int S, int nblk,
                      void* stream);

/* ---- K3g: the same p wanted eigenpairs for Rayleigh-Ritz matrices of order 129 .. 1536 (xk_eigh_big.hip) ---------
 * torch.linalg.eigh + _take_eigpairs (symeig.py:174-175, 255-264) once the un-restarted basis (symeig.py:132-135) has
 * outgrown the LDS-resident kernels: Householder tridiagonalisation of the upper triangle of a work copy in global
 * memory, k - 1 launches (one per step, look-ahead form) over several workgroups per matrix; then bisection / inverse
 * iteration / self-check in LDS like K3t and the back-transformation from the reflectors parked in the work copy, one
 * workgroup per matrix.  The whole sequence is enqueued on `stream` by one call.  Only the lower triangle of T is read.
 * ws: xk_small_eigh_big_workspace_elems(B, k, wg) elements (work copies + the steps' hand-over blocks).
 * wg: workgroups per matrix of the step kernels, 0 = automatic (by batch and order), 1 .. 32; threads: 0 = 512, or 256.
 * lam (B, p) ascending, Y (B, p, k) eigenvectors, info[b] != 0 -> redo that call on the library solver.
 * xk_small_eigh_big_batch(k, p, elem_size): shifts factorised at a time (> 0) when the problem fits the 160 KiB of
 * LDS, 0 when it does not.  8 <= k <= 1536 (r06: beyond 1024 with 24 column slots per lane; r05: beyond 768 with 16 column slots per lane in 256-thread workgroups, or the two-stage form below where its band fits: fp32), p <= 256 (r06; 64 before) (also the solver for MORE THAN 16 wanted pairs at any order: wide
 * eigen-blocks, thick restarts; the batch of vectors in work lives in LDS, finished ones in the rows of Y).
 * algo: 1 = the form above; 2 = the TWO-STAGE form (xk_eigh_band.hip: dense -> band of 16 sub-diagonals by block
 * reflectors, two launches per 16 columns; band -> tridiagonal by bulge chasing in LDS, one workgroup per matrix, sweeps
 * pipelined three steps apart; eigenvectors back through both stages, one workgroup per vector), XK_ERR_UNSUPPORTED when
 * the band of order k does not fit the LDS (fp64: k <= 614); 3 = the PERSISTENT form (r06, xk_eigh_persist.hip: the whole
 * Householder reduction in ONE launch of one workgroup per matrix, the trailing block of order <= 256 (fp64) / 384 (fp32)
 * resident in the registers of its eight waves, one barrier per step; larger orders start with k - 256 / k - 384 step
 * launches of form 1 and hand over); 0 = the measured choice (form 3 up to 64 .. 128 orders beyond its register limit,
 * by batch; the two-stage form beyond where it fits; else form 1).  Every form is bit-reproducible; the forms differ in
 * rounding. */
int xk_small_eigh_big_batch(int k, int p, int elem_size);
long xk_small_eigh_big_workspace_elems(int B, int k, int wg);
int xk_small_eigh_big_f64(const double* T, double* lam, double* Y, double* ws, long ws_elems, int* info, int B, int k,
                          int p, int uppest, long ldt, long sT, int wg, int threads, int algo, void* stream);
int xk_small_eigh_big_f32(const float* T, float* lam, float* Y, float* ws, long ws_elems, int* info, int B, int k,
                          int p, int uppest, long ldt, long sT, int wg, int threads, int algo, void* stream);

/* ---- Davidson chain: one C call per stage of an iteration (xitorch/_impls/linalg/symeig.py:160-223) -------------
 * The stages between two operator-panel products are two to eight small launches each; issued from C++ they cost a
 * few microseconds of host time instead of an interpreter round trip per launch (what bounds small per-GPU batches).
 * xk_davidson_ritz: xk_ritz_residual + the group status {max_b rmax (NaN-propagating), max_b info, max_b flag} as
 *   three doubles (+ a fourth, max_b cond, when cond is given; cond is re-zeroed; + a fifth, max_b orth, when orth is
 *   given: xk_ritz_guard of the Ritz block X just formed, folded and re-zeroed); rmax is left zeroed for the next
 *   step (symeig.py:178-197).  flag, cond and orth may be NULL.  Gs: scratch >= B*P*P and ws:
 *   xk_dense_mm_workspace_elems(B, P, N, P, 0), both only read when orth is given and P > 8.
 * xk_ritz_guard: the a-posteriori check that stands where the reference's whole-basis CholeskyQR makes a wrong
 *   answer impossible (tallqr of [V, t] every iteration, _utils/tensor.py:8-19, symeig.py:207-223): orth[b] =
 *   max(orth[b], max_{c,d} |<X_c, (M X)_d> - delta_cd|) over the P rows of the Ritz block X (B, P, ldx) and M X
 *   (B, P, ldm; NULL: X itself).  Two copies of one eigenpair in a block give 1, a healthy block rounding level; the
 *   Davidson driver never returns (and never restarts from) a block above its threshold.  P <= 8: one kernel, the
 *   panels are read once; wider: Gram on K1 into Gs (>= B*P*P) + one wave per member.
 * xk_davidson_orth: rows [k0, k0+q) of the basis V (B, cap, ldv) against rows [0, k0): block Gram-Schmidt
 *   (C[b,c,a] = <V_a, t_c>, t_c -= sum_a C V_a) and CholeskyQR of the q rows — for q <= 8 in ONE kernel (Gram,
 *   Cholesky, inverse, transform; one workgroup per batch member) — i.e. tallqr of [V, t] restricted to the new block
 *   (_utils/tensor.py:8-19, symeig.py:207-220).  passes = 0: CholeskyQR only; 1: projection, CholeskyQR; >= 2:
 *   [projection, CholeskyQR] per pass with the FIRST CholeskyQR shifted (Gram + 11 (N q + q (q + 1)) u trace I): the
 *   order that keeps nearly dependent panels (Gram spectrum over 15 decades) positive definite and orthogonal to V.
 *   cond (B, may be NULL; q <= 8 only): cond[b] = max(cond[b], (largest / smallest pivot)^2 of the raw panel's
 *   CholeskyQR) — the squared condition estimate by which the Davidson driver decides when ONE pass stops being safe.  C: scratch >= B*q*max(k0,q), W: scratch B*q*q, info[b] sticky
 *   index+1 of a non-positive pivot, ws: xk_dense_mm_workspace_elems(B, cap, N, q, 0).  Any q: panels wider than
 *   32 are taken 32 rows at a time, each chunk against everything before it (twice), then among itself.
 * xk_davidson_extend_t: Tn[b,c,a] = <V_a, (AV)_{k0+c}> for a < k0+q, written to T[b, k0+c, a] and mirrored to
 *   T[b, a, k0+c] (symeig.py:170 restricted to the new rows / columns).  Tn: scratch >= B*q*(k0+q). */
int xk_davidson_ritz_f64(const double* V, const double* AV, const double* Y, const double* lam, double* X, double* Tn,
                         double* rmax, const int* info, const int* flag, double* cond, double* orth, double* status,
                         int B, int k, int N, int P, long ldv, long sV, long ldav, long sAV, long sY, long sYa,
                         long sYc, long sLam, long ldx, long sX, long ldt, long sT, double* Gs, long gs_elems,
                         double* ws, long ws_elems, void* stream);
int xk_davidson_ritz_f32(const float* V, const float* AV, const float* Y, const float* lam, float* X, float* Tn,
                         float* rmax, const int* info, const int* flag, float* cond, float* orth, double* status, int B,
                         int k, int N, int P, long ldv, long sV, long ldav, long sAV, long sY, long sYa, long sYc,
                         long sLam, long ldx, long sX, long ldt, long sT, float* Gs, long gs_elems, float* ws,
                         long ws_elems, void* stream);
int xk_ritz_guard_f64(const double* X, const double* MX, double* orth, int B, int N, int P, long ldx, long sX,
                      long ldm, long sM, double* Gs, long gs_elems, double* ws, long ws_elems, void* stream);
int xk_ritz_guard_f32(const float* X, const float* MX, float* orth, int B, int N, int P, long ldx, long sX, long ldm,
                      long sM, float* Gs, long gs_elems, float* ws, long ws_elems, void* stream);
int xk_davidson_orth_f64(double* V, int B, int N, int k0, int q, long ldv, long sV, double* C, double* W, int* info,
                         double* cond, double* ws, long ws_elems, int passes, void* stream);
int xk_davidson_orth_f32(float* V, int B, int N, int k0, int q, long ldv, long sV, float* C, float* W, int* info,
                         float* cond, float* ws, long ws_elems, int passes, void* stream);
int xk_davidson_extend_t_f64(const double* V, const double* AV, double* T, double* Tn, int B, int N, int k0, int q,
                             long ldv, long sV, long ldav, long sAV, long ldt, long sT, double* ws, long ws_elems,
                             void* stream);
int xk_davidson_extend_t_f32(const float* V, const float* AV, float* T, float* Tn, int B, int N, int k0, int q,
                             long ldv, long sV, long ldav, long sAV, long ldt, long sT, float* ws, long ws_elems,
                             void* stream);

/* ---- GMRES: per-system Hessenberg / Givens state on the device (xitorch/_impls/linalg/solve.py:326-433) ----------
 * The reference fills one Hessenberg column per iteration by modified Gram-Schmidt (:390-394) and solves the
 * (k+1) x k least-squares problem from scratch with torch.linalg.lstsq (:403) on every pass of its Python loop.
 * Here the S = batch x columns systems keep their state on the device, always in double:
 *   R  (S, cap+1, cap) row-major per system: the rotated (triangularised) Hessenberg, R[i][j] meaningful for i <= j
 *   cs, sn (S, cap): Givens rotations;  g (S, cap+1): rotated right-hand side, g[:,0] = |r0| set by the caller.
 * xk_gmres_step: column k from the two Gram passes of the CGS2 orthogonalisation — c1[s, 0..k] = <q_j, w>,
 *   c2n[s, 0..k] = <q_j, w1> with w1 = w - Q c1 and c2n[s, k+1] = <w1, w1> (strides sc1 / sc2 between systems) —
 *   h[j,k] = c1 + c2, h[k+1,k] = sqrt(<w1,w1> - |c2|^2); replays rotations 0..k-1, creates rotation k, updates g;
 *   inv_hn[s] = 1 / h[k+1,k] (0 on breakdown); est2[s * xk_kry_max_partials()] = g[k+1]^2, i.e. a one-partial |r|^2
 *   array for xk_kry_status: the least-squares residual norm, equal to :414-415's explicit one in exact arithmetic.
 * xk_gmres_finish: basis row k+1 (holding w1) <- (w1 - sum_{j<=k} c2n[j] q_j) * inv_hn   (:392,396-398).
 * xk_gmres_solve: y[s, 0..kd) = R^-1 g (back substitution; zero pivots give 0) — what :403 returns; kd <= 8192. */
int xk_gmres_step_f64(const double* c1, long sc1, const double* c2n, long sc2, int k, int cap, double* R, double* cs,
                      double* sn, double* g, double* inv_hn, double* est2, int S, void* stream);
int xk_gmres_step_f32(const float* c1, long sc1, const float* c2n, long sc2, int k, int cap, double* R, double* cs,
                      double* sn, double* g, float* inv_hn, float* est2, int S, void* stream);
int xk_gmres_finish_f64(double* Q, const double* c2n, long sc2, const double* inv_hn, int S, int N, int k, long ldq,
                        long sQ, void* stream);
int xk_gmres_finish_f32(float* Q, const float* c2n, long sc2, const float* inv_hn, int S, int N, int k, long ldq,
                        long sQ, void* stream);
int xk_gmres_solve_f64(const double* R, const double* g, double* y, long sy, int S, int kd, int cap, void* stream);
int xk_gmres_solve_f32(const double* R, const double* g, float* y, long sy, int S, int kd, int cap, void* stream);

/* ---- GMRES for COMPLEX systems (extension: the reference's gmres is real-only; xk_gmres_c.hip) --------------------
 * Complex data is INTERLEAVED (re, im) storage; every pitch, stride and length counts whole COMPLEX elements.  A 16 B
 * vector holds CV = 1 complex128 / 2 complex64 elements; pitches and strides must be multiples of CV, base pointers 16 B
 * aligned, and the pad [N, round_up(N, CV)) of every vector zero (else XK_ERR_UNSUPPORTED where it can be checked).
 * xk_gmres_gram: c[s, i] = sum_n conj(Q[s, i, n]) w[s, n] for i < kq (Q: sQ between systems, ldq between rows; w: sw
 *   between systems; c: sc between systems) and c[s, kq] = (|w_s|^2, exactly 0).  Fixed-shape reduction without atomics
 *   (repeated calls are bit-identical): every vector is cut into tiles of 1024 * CV elements, nblk MUST be
 *   ceil(N / (1024 * CV)) (else XK_ERR_ARG; N == 0: nblk == 0 and c[s, 0..kq] = 0), scratch holds
 *   S * nblk * (kq + 1) * 2 doubles.  Products and wave sums in
 *   the vector's precision, everything above a wave in double.
 * xk_lincomb: Out[b, c, :] = beta Out[b, c, :] + alpha sum_{a<k} C[b, c, a] V[b, a, :], complex C (sC between batch
 *   members, sCc between output rows, a contiguous: the "ca" layout), REAL alpha / beta; c < P.
 * xk_gmres_step / _finish / _solve: as the real kernels above with complex c1, c2n (c2n[s, k+1] = (|w1|^2, 0)), Q, y and
 *   state R (S, cap+1, cap), sn (S, cap), g (S, cap+1) COMPLEX double, cs (S, cap) REAL double; inv_hn and est2 are
 *   real (est2 = |g[k+1]|^2 for xk_kry_status_f64/_f32).  Rotation k for a = rotated h[k,k], b = h[k+1,k] >= 0:
 *   cs = |a| / sqrt(|a|^2 + b^2), sn = (a / |a|) b / sqrt(|a|^2 + b^2) (a = 0: cs = 0, sn = 1), and
 *   [cs, sn; -conj(sn), cs] is applied from the left.  xk_gmres_solve: kd <= 4096 (else XK_ERR_UNSUPPORTED). */
int xk_gmres_gram_c128(const double* Q, const double* w, double* c, double* scratch, int S, int N, int kq, long ldq,
                       long sQ, long sw, long sc, int nblk, void* stream);
int xk_gmres_gram_c64(const float* Q, const float* w, float* c, double* scratch, int S, int N, int kq, long ldq,
                      long sQ, long sw, long sc, int nblk, void* stream);
int xk_lincomb_c128(const double* V, const double* C, double* Out, int B, int k, int N, int P, long ldv, long sV,
                    long sC, long sCc, long ldo, long sO, double alpha, double beta, void* stream);
int xk_lincomb_c64(const float* V, const float* C, float* Out, int B, int k, int N, int P, long ldv, long sV,
                   long sC, long sCc, long ldo, long sO, double alpha, double beta, void* stream);
int xk_gmres_step_c128(const double* c1, long sc1, const double* c2n, long sc2, int k, int cap, double* R, double* cs,
                       double* sn, double* g, double* inv_hn, double* est2, int S, void* stream);
int xk_gmres_step_c64(const float* c1, long sc1, const float* c2n, long sc2, int k, int cap, double* R, double* cs,
                      double* sn, double* g, float* inv_hn, float* est2, int S, void* stream);
int xk_gmres_finish_c128(double* Q, const double* c2n, long sc2, const double* inv_hn, int S, int N, int k, long ldq,
                         long sQ, void* stream);
int xk_gmres_finish_c64(float* Q, const float* c2n, long sc2, const float* inv_hn, int S, int N, int k, long ldq,
                        long sQ, void* stream);
int xk_gmres_solve_c128(const double* R, const double* g, double* y, long sy, int S, int kd, int cap, void* stream);
int xk_gmres_solve_c64(const double* R, const double* g, float* y, long sy, int S, int kd, int cap, void* stream);

/* ---- the same fused Krylov kernels for COMPLEX systems (complex64 = _c64, complex128 = _c128) ----------
 * The reference runs cg / bicgstab on complex operators with conjugated inner products
 * (xitorch/_impls/linalg/solve.py:441-445; _tests/test_linop_fcns.py:474-524, 631-676).  Pointers address
 * INTERLEAVED (re, im) storage (torch.view_as_real of a complex panel); N and ld count complex elements; the
 * per-system scalars (rho, alpha, omega, E) are (S, 2) arrays; partials of complex products are
 * (S, xk_kry_max_partials(), 2); |r|^2 partials (Prr) stay real (S, xk_kry_max_partials()) and are consumed by
 * xk_kry_status_f32/_f64.  <x, y> = sum conj(x) y; xk_kry_dots_c*: conj1 = 1 stores conj(<x1,y1>) = <y1,x1>
 * in P1 (BiCGStab's omega = <t, s> / <t, t>, solve.py:286, with the shift applied to y1 = t). */
int xk_kry_dots_c128(const double* x1, double* y1, const double* x2, const double* y2, const double* shiftz,
                     const double* E, double* P1, double* P2, int S, int N, long ld, int nblk, int conj1, void* stream);
int xk_kry_dots_c64(const float* x1, float* y1, const float* x2, const float* y2, const float* shiftz, const float* E,
                    float* P1, float* P2, int S, int N, long ld, int nblk, int conj1, void* stream);
int xk_bicg_p_c128(const double* r, double* p, const double* v, const double* Prho_new, const double* rho_old,
                   const double* alpha, const double* omega, double* rho_store, int S, int N, long ld, int nblk,
                   double eps, int first, void* stream);
int xk_bicg_p_c64(const float* r, float* p, const float* v, const float* Prho_new, const float* rho_old,
                  const float* alpha, const float* omega, float* rho_store, int S, int N, long ld, int nblk, double eps,
                  int first, void* stream);
int xk_bicg_s_c128(const double* r, const double* v, double* s, const double* rho, const double* Pr0v,
                   double* alpha_store, int S, int N, long ld, int nblk, double eps, void* stream);
int xk_bicg_s_c64(const float* r, const float* v, float* s, const float* rho, const float* Pr0v, float* alpha_store,
                  int S, int N, long ld, int nblk, double eps, void* stream);
int xk_bicg_final_c128(const double* x, double* xout, const double* yd, const double* zd, const double* s,
                       const double* t, double* r, const double* r0, const double* alpha, const double* Pts,
                       const double* Ptt, double* omega_store, double* Prr, double* Prho, int S, int N, long ld,
                       int nblk, double eps, int skip_r, void* stream);
int xk_bicg_final_c64(const float* x, float* xout, const float* yd, const float* zd, const float* s, const float* t,
                      float* r, const float* r0, const float* alpha, const float* Pts, const float* Ptt,
                      float* omega_store, float* Prr, float* Prho, int S, int N, long ld, int nblk, double eps,
                      int skip_r, void* stream);
int xk_kry_resid_c128(const double* b, const double* y, double* r, const double* r0, double* Prr, double* Prho,
                      int S, int N, long ld, int nblk, void* stream);
int xk_kry_resid_c64(const float* b, const float* y, float* r, const float* r0, float* Prr, float* Prho, int S, int N,
                     long ld, int nblk, void* stream);
int xk_cg_update_c128(const double* x, double* xout, const double* p, const double* Ap, double* r, const double* Prz,
                      const double* PpAp, double* Prr, int S, int N, long ld, int nblk, double eps, int skip_r,
                      void* stream);
int xk_cg_update_c64(const float* x, float* xout, const float* p, const float* Ap, float* r, const float* Prz,
                     const float* PpAp, float* Prr, int S, int N, long ld, int nblk, double eps, int skip_r,
                     void* stream);
int xk_cg_p_c128(const double* z, double* p, const double* Prz_new, const double* Prz_old, int S, int N, long ld,
                 int nblk, double eps, void* stream);
int xk_cg_p_c64(const float* z, float* p, const float* Prz_new, const float* Prz_old, int S, int N, long ld, int nblk,
                double eps, void* stream);

/* ---- MINRES step kernels (extension: Paige & Saunders 1975; Hermitian indefinite / consistent singular systems) ----
 * Same (S, ld) vectors, block partials and nblk as the fused Krylov kernels above; _c128 / _c64 address interleaved
 * (re, im) storage with N and ld in complex elements.  The per-system scalars (Lanczos alpha / beta, the Givens
 * rotation, dbar / epsln, phibar, a flag) are DOUBLES whatever the vector type: state is (2, S, xk_minres_state_len())
 * doubles, iteration k reads slot k & 1 and xk_minres_update writes slot (k + 1) & 1.  Entry i of a slot: 0 beta,
 * 1 previous beta, 2 cs, 3 sn, 4 dbar, 5 epsln, 6 phibar, 7 flag (0 running; frozen: 1 beta = 0, exact convergence;
 * 2 <r2, P r2> < 0, the preconditioner is not positive definite; 3 gamma = 0), 8..11 alpha, gamma, delta, phi of the
 * step that wrote the slot.  Frozen systems are never written again (their state is carried from slot to slot).
 * Palpha, Pb (and Pbeta with beta_is_dot = 1) are partials written by xk_kry_dots of the same suffix — (re, im)
 * pairs for the complex suffixes, of which the real part is used; Pbeta with beta_is_dot = 0 are the real partials
 * xk_minres_lanczos writes.  phi2[s * xk_kry_max_partials()] receives phibar^2 (+inf with flag 2): a one-partial
 * |r|^2 array for xk_kry_status (nblk = 1).
 * xk_minres_init: beta = sqrt(<b, y0>) from Pb (y0 = b, or P b with a preconditioner); v = y0 / beta; slot k & 1.
 * xk_minres_lanczos: r1 <- Av - (alpha / beta) r2 - (beta / previous beta) r1 (the caller swaps r1 and r2; r1 is not
 *   read on a first step); Pbeta (may be NULL) <- partials of |r1|^2.
 * xk_minres_update: beta_new = sqrt(sum Pbeta); rotation; w1 <- (v - epsln w1 - delta w2) / gamma (the caller rotates
 *   the ring); x += phi w1; v <- y / beta_new (y = the new r2, or P r2), v <- 0 when beta_new = 0. */
int xk_minres_state_len(void);
int xk_minres_init_f64(const double* y0, double* v, const double* Pb, double* state, double* phi2, int S, int N, long ld,
                       int nblk, int k, void* stream);
int xk_minres_lanczos_f64(const double* Av, const double* r2, double* r1, const double* Palpha, const double* state,
                          double* Pbeta, int S, int N, long ld, int nblk, int k, void* stream);
int xk_minres_update_f64(double* v, const double* y, double* w1, const double* w2, double* x, const double* Palpha,
                         const double* Pbeta, int beta_is_dot, double* state, double* phi2, int S, int N, long ld,
                         int nblk, int k, void* stream);
int xk_minres_init_f32(const float* y0, float* v, const float* Pb, double* state, float* phi2, int S, int N, long ld,
                       int nblk, int k, void* stream);
int xk_minres_lanczos_f32(const float* Av, const float* r2, float* r1, const float* Palpha, const double* state,
                          float* Pbeta, int S, int N, long ld, int nblk, int k, void* stream);
int xk_minres_update_f32(float* v, const float* y, float* w1, const float* w2, float* x, const float* Palpha,
                         const float* Pbeta, int beta_is_dot, double* state, float* phi2, int S, int N, long ld,
                         int nblk, int k, void* stream);
int xk_minres_init_c128(const double* y0, double* v, const double* Pb, double* state, double* phi2, int S, int N, long ld,
                       int nblk, int k, void* stream);
int xk_minres_lanczos_c128(const double* Av, const double* r2, double* r1, const double* Palpha, const double* state,
                          double* Pbeta, int S, int N, long ld, int nblk, int k, void* stream);
int xk_minres_update_c128(double* v, const double* y, double* w1, const double* w2, double* x, const double* Palpha,
                         const double* Pbeta, int beta_is_dot, double* state, double* phi2, int S, int N, long ld,
                         int nblk, int k, void* stream);
int xk_minres_init_c64(const float* y0, float* v, const float* Pb, double* state, float* phi2, int S, int N, long ld,
                       int nblk, int k, void* stream);
int xk_minres_lanczos_c64(const float* Av, const float* r2, float* r1, const float* Palpha, const double* state,
                          float* Pbeta, int S, int N, long ld, int nblk, int k, void* stream);
int xk_minres_update_c64(float* v, const float* y, float* w1, const float* w2, float* x, const float* Palpha,
                         const float* Pbeta, int beta_is_dot, double* state, float* phi2, int S, int N, long ld,
                         int nblk, int k, void* stream);

/* ---- Chebyshev filter step (extension: Zhou, Saad, Tiago, Chelikowsky 2006; symeig method "chebfsi") ----------
 * Panels are (Bt, p, ld*) arrays: Bt operators, p vectors each, every vector a contiguous run of N elements; each of
 * the four panels has its own pitch ld* >= N and batch stride s* >= 0 (elements; complex elements for _c128 / _c64,
 * which address interleaved (re, im) storage).  For every b < Bt, c < p, n < N
 *     out[b,c,n] = coef[3b] * AY[b,c,n] + coef[3b+1] * Y[b,c,n] + coef[3b+2] * Yprev[b,c,n]
 * coef: (Bt, 3) DOUBLES on the device (alpha, beta, gamma per operator, real for every suffix), read by the kernel:
 * no host synchronisation.  _f64 / _c128 evaluate in double; _f32 / _c64 round each coefficient once to float and
 * evaluate in float; the sum is (alpha AY + beta Y) + gamma Yprev, products may be contracted into FMAs.
 * gamma == 0.0 exactly (either sign): Yprev[b] is not read (it may hold NaN / Inf) — the first step of a filter.
 * out may BE Yprev (same pointer, pitch and batch stride) or lie apart from it.  XK_ERR_ARG, nothing launched, nothing
 * written: the address range of out intersects that of AY or Y (or that of a Yprev it is not identical to), N <= 0,
 * Bt <= 0, p <= 0, a pitch below N, a negative stride, a NULL pointer, rows of out that overlap each other (Bt > 1 and
 * sO < (p - 1) * ldO + N).  Only out[b, c, :N] is written (pads stay).
 * Every base 16 B aligned and every pitch / batch stride a multiple of the 16 B vector: vector form (16 B non-temporal
 * loads, 4 per lane and array in flight); any other layout: scalar form, same result contract.  4 Bt p N s bytes. */
int xk_cheb_step_f64(const double* AY, long ldA, long sA, const double* Y, long ldY, long sY, const double* Yprev,
                     long ldP, long sP, double* out, long ldO, long sO, const double* coef, int Bt, int p, int N,
                     void* stream);
int xk_cheb_step_f32(const float* AY, long ldA, long sA, const float* Y, long ldY, long sY, const float* Yprev,
                     long ldP, long sP, float* out, long ldO, long sO, const double* coef, int Bt, int p, int N,
                     void* stream);
int xk_cheb_step_c128(const double* AY, long ldA, long sA, const double* Y, long ldY, long sY, const double* Yprev,
                      long ldP, long sP, double* out, long ldO, long sO, const double* coef, int Bt, int p, int N,
                      void* stream);
int xk_cheb_step_c64(const float* AY, long ldA, long sA, const float* Y, long ldY, long sY, const float* Yprev,
                     long ldP, long sP, float* out, long ldO, long sO, const double* coef, int Bt, int p, int N,
                     void* stream);

/* ---- Clenshaw step of a Chebyshev band-pass filter (extension: Li, Xi, Vecharynski, Yang, Saad 2016; symeig
 * mode "nearest"; new symbols only) ----
 * Panels as for xk_cheb_step: (Bt, p, ld*) arrays, each of the five with its own pitch ld* >= N and batch stride
 * s* >= 0 (elements; complex elements for _c128 / _c64, which address interleaved (re, im) storage).  For every
 * b < Bt, c < p, n < N
 *     out[b,c,n] = ((coef[4b] * AY[b,c,n] + coef[4b+1] * Y[b,c,n]) + coef[4b+2] * Yprev[b,c,n]) + coef[4b+3] * X0[b,c,n]
 * coef: (Bt, 4) DOUBLES on the device (alpha, beta, gamma, delta per operator, real for every suffix), read by the
 * kernel: no host synchronisation.  _f64 / _c128 evaluate in double; _f32 / _c64 round each coefficient once to float
 * and evaluate in float; the sum is taken left to right as written, products may be contracted into FMAs.
 * gamma == 0.0 exactly (either sign): Yprev[b] is not read (it may hold NaN / Inf) and its term is absent.
 * out may BE Yprev (same pointer, pitch and batch stride) or lie apart from it.  XK_ERR_ARG, nothing launched, nothing
 * written: the address range of out intersects that of AY, Y or X0 (or that of a Yprev it is not identical to),
 * N <= 0, Bt <= 0, p <= 0, a pitch below N, a negative stride, a NULL pointer, rows of out that overlap each other
 * (Bt > 1 and sO < (p - 1) * ldO + N).  Only out[b, c, :N] is written (pads stay).  All stores are ordinary vector
 * stores.  Every base 16 B aligned and every pitch / batch stride a multiple of the 16 B vector: vector form (16 B
 * non-temporal loads, 4 per lane and array in flight); any other layout: scalar form, same result contract.
 * 5 Bt p N s bytes (4 where gamma == 0). */
int xk_cheb_clenshaw_f64(const double* AY, long ldA, long sA, const double* Y, long ldY, long sY, const double* Yprev,
                         long ldP, long sP, const double* X0, long ldX, long sX, double* out, long ldO, long sO,
                         const double* coef, int Bt, int p, int N, void* stream);
int xk_cheb_clenshaw_f32(const float* AY, long ldA, long sA, const float* Y, long ldY, long sY, const float* Yprev,
                         long ldP, long sP, const float* X0, long ldX, long sX, float* out, long ldO, long sO,
                         const double* coef, int Bt, int p, int N, void* stream);
int xk_cheb_clenshaw_c128(const double* AY, long ldA, long sA, const double* Y, long ldY, long sY, const double* Yprev,
                          long ldP, long sP, const double* X0, long ldX, long sX, double* out, long ldO, long sO,
                          const double* coef, int Bt, int p, int N, void* stream);
int xk_cheb_clenshaw_c64(const float* AY, long ldA, long sA, const float* Y, long ldY, long sY, const float* Yprev,
                         long ldP, long sP, const float* X0, long ldX, long sX, float* out, long ldO, long sO,
                         const double* coef, int Bt, int p, int N, void* stream);

/* ---- LOBPCG: the in-place rotation of the three panel stacks (extension: symeig method "lobpcg"; new symbols only) --
 * S, AS and (may be NULL) MS are (Bt, rows, ld*) stacks [X | P | W] of the driver: every row a contiguous run of N
 * elements, pitch ld* >= N, stack stride s* (elements; complex elements for _c128 / _c64, interleaved storage).
 * C: coefficients in the panels' dtype, C[b,a,c] at C[b * sC + a * sCa + c * sCc], plain (NOT conjugated: the caller
 * passes eigenvector columns).  lam: DOUBLES on the device, lam[b * sLam + c], c < w, read by the kernel and rounded
 * once by the 32-bit forms.  For every b < Bt and n < N, with w <= q <= k <= xk_lobpcg_max_rows():
 *     stack[b,c,n] <- sum_{a<k} C[b,a,c] * stack[b,a,n],   c < q,   for stack = S, MS, AS         (in place)
 *     S[b,q+c,n]   <- AS'[b,c,n] - lam[b,c] * (MS ? MS' : S')[b,c,n],   c < w                    (the residual)
 *     Pnorm[(b * w + c) * nblk + blk] <- sum over column chunk blk of |S[b,q+c,n]|^2   (doubles, fixed order)
 *     Pmax[b * nblk + blk] <- max over chunk blk and c < w of |S[b,q+c,n]| (complex: the modulus; NaN is kept)
 * nblk = xk_lobpcg_blocks(N, element bytes): chunks of 256 16 B vectors; it depends on N and the dtype only.
 * Rows [q, q+w) of AS and MS, every row >= q + w and everything at n >= N are left alone; rows >= k are not read.
 * Sums accumulate in the panels' real type in the order a = 0, 1, ...; no atomics, a repeat call gives the same bits.
 * A workgroup owns its columns outright and loads all k rows of them before it stores: there is no second copy.
 * XK_ERR_ARG, nothing launched: NULL S / AS / C / lam / Pnorm / Pmax; Bt, N or w <= 0; q < w, q > k, k above
 * xk_lobpcg_max_rows(); a pitch below N; a stack stride below (q + w) * pitch.
 * Every base 16 B aligned and every pitch / stack stride a multiple of the 16 B vector: vector form; any other layout:
 * scalar form, same result contract. */
int xk_lobpcg_max_rows(void);
int xk_lobpcg_blocks(int N, int elem_bytes);
int xk_lobpcg_rotate_f64(double* S, long ldS, long sS, double* AS, long ldA, long sA, double* MS, long ldM, long sM,
                         const double* C, long sC, long sCa, long sCc, const double* lam, long sLam, double* Pnorm,
                         double* Pmax, int Bt, int N, int k, int q, int w, void* stream);
int xk_lobpcg_rotate_f32(float* S, long ldS, long sS, float* AS, long ldA, long sA, float* MS, long ldM, long sM,
                         const float* C, long sC, long sCa, long sCc, const double* lam, long sLam, double* Pnorm,
                         double* Pmax, int Bt, int N, int k, int q, int w, void* stream);
int xk_lobpcg_rotate_c128(double* S, long ldS, long sS, double* AS, long ldA, long sA, double* MS, long ldM, long sM,
                          const double* C, long sC, long sCa, long sCc, const double* lam, long sLam, double* Pnorm,
                          double* Pmax, int Bt, int N, int k, int q, int w, void* stream);
int xk_lobpcg_rotate_c64(float* S, long ldS, long sS, float* AS, long ldA, long sA, float* MS, long ldM, long sM,
                         const float* C, long sC, long sCa, long sCc, const double* lam, long sLam, double* Pnorm,
                         double* Pmax, int Bt, int N, int k, int q, int w, void* stream);

/* ---- Golub-Kahan-Lanczos bidiagonalisation with thick restart (extension: svd method "gkl"; new symbols only, ABI stays 2) -
 * xk_gkl_sweep: one Gram-Schmidt pass of one new vector per member against j <= xk_gkl_max_rows() rows of a basis
 *   panel Q (Bt, cap, ldQ), rows are vectors (elements; complex elements for _c128 / _c64, interleaved storage):
 *       dst[b,n] = s_b * ( w[b,n] - sum_{i<j} c[b,i] Q[b,i,n] ),  n < N,   s_b = scale ? scale[b] : 1
 *   c[b,i] = coef[b * sC + i] (real) or coef[b * sC + 2i] + i coef[b * sC + 2i + 1] (complex), DOUBLES on the device;
 *   coef NULL: no sum.  From the same read of Q it writes the partial sums over each chunk of xk_gkl_chunk_elems()
 *   elements of conj(Q[b,i,:]) . dst[b,:] and of |dst[b,:]|^2 (of the values as stored) as doubles
 *       part[(b * nval + r) * nchunk + chunk],  r < nval = j (complex: 2j; re, im interleaved) + 1 (sum of squares),
 *   nchunk = ceil(N / chunk elements); part_len (doubles) must hold Bt * nval * nchunk.  The update is evaluated in
 *   double and rounded once.  No atomics: a repeat call returns the same bits.  dst may BE w (same pointer and
 *   stride) or lie apart from it; it must not touch rows [0, j) of Q (a slot of the panel that holds Q is fine: with
 *   one batch stride for both, the footprints are compared member by member).  XK_ERR_ARG, nothing launched: Bt <= 0 or
 *   > 65535, N <= 0, j < 0 or beyond the row cap, NULL w / dst / part (Q with j > 0), ldQ < N, a negative stride,
 *   Bt > 1 with sD < N or sC below the coefficients of a member, overlapping ranges as above, a short part.
 *   Bases 16 B aligned and pitch / strides multiples of the 16 B vector: 16 B non-temporal loads of the basis, all
 *   issued before the first use; otherwise element by element.  Only dst[b, :N] is written.
 * xk_gkl_finish: adds the partials of one sweep in a fixed order; coef[b * sC + r] = sum_r for r < nval - 1 (coef
 *   may be NULL), nrm[b] = sqrt(sum of squares), rnrm[b] = its reciprocal, dst[b * sdst] = the norm (dst may be
 *   NULL; the alpha / beta slot of the projected matrix), smax[b] = max(smax[b], norm) (may be NULL).  Breakdown —
 *   norm <= u * smax[b] (the value before this call), or not finite —: norm and reciprocal are written as 0 and, when
 *   brk is given and brk[b] < 0, brk[b] = code.
 * xk_gkl_bsvd: SVD Bm[b] = P diag(sigma) Q^T of (Bt, n, n) row-major real matrices, n <= xk_gkl_bsvd_max(), by
 *   one-sided Jacobi in double (never through Bm^T Bm).  sigma (Bt, n) descending (descending != 0) or ascending,
 *   P, Q (Bt, n, n) row-major with the vectors as COLUMNS, orthonormal also where sigma is null, res[b,i] =
 *   |beta[b] P[b, n-1, i]| (beta NULL: 0), status[4b..] = {number of i < k with res <= tol * max(sigma_max, smax[b]),
 *   Jacobi sweeps, 1 if the sweep limit was hit, brk[b] (brk NULL: -1)}.  Bnext (may be NULL; not Bm; keep < n): the
 *   projected matrix of the restarted basis, diag(sigma[:keep]) and column keep = beta * P[n-1, :keep]. */
int xk_gkl_max_rows(void);
int xk_gkl_bsvd_max(void);
int xk_gkl_chunk_elems(int elem_bytes);
int xk_gkl_sweep_f64(const double* Q, long ldQ, long sQ, const double* w, long sW, double* dst, long sD,
                     const double* coef, long sC, const double* scale, double* part, long part_len, int Bt, int j,
                     int N, void* stream);
int xk_gkl_sweep_f32(const float* Q, long ldQ, long sQ, const float* w, long sW, float* dst, long sD,
                     const double* coef, long sC, const double* scale, double* part, long part_len, int Bt, int j,
                     int N, void* stream);
int xk_gkl_sweep_c128(const double* Q, long ldQ, long sQ, const double* w, long sW, double* dst, long sD,
                      const double* coef, long sC, const double* scale, double* part, long part_len, int Bt, int j,
                      int N, void* stream);
int xk_gkl_sweep_c64(const float* Q, long ldQ, long sQ, const float* w, long sW, float* dst, long sD,
                     const double* coef, long sC, const double* scale, double* part, long part_len, int Bt, int j,
                     int N, void* stream);
int xk_gkl_finish(const double* part, int Bt, int nval, int nchunk, double* coef, long sC, double* nrm, double* rnrm,
                  double* dst, long sdst, double* smax, double u, int* brk, int code, void* stream);
int xk_gkl_bsvd(const double* Bm, const double* beta, const double* smax, const int* brk, int Bt, int n, int k,
                int keep, int descending, double tol, double* sigma, double* P, double* Q, double* res, int* status,
                double* Bnext, void* stream);

/* ---- Krylov-Schur Arnoldi for non-Hermitian eigenpairs (extension: linalg.eigs; new symbols only, ABI stays 2) ------
 * The Arnoldi step orthogonalises with xk_gkl_sweep_* above.  The projected matrix H is (Bt, m + 1, m) row-major
 * DOUBLES on the device: real for real operators, interleaved (re, im) for complex ones (cplx != 0).
 * xk_arn_finish: xk_gkl_finish — the same fixed-order sums, norm, reciprocal, running maximum and breakdown flag, bit
 *   for bit — with one more output: when hcol is given, sum_r (r < nval - 1) is also stored (accumulate == 0) or added
 *   (accumulate == 1) at hcol[b * sHb + r * sHr] (real) or hcol[b * sHb + (r / 2) * sHr + r % 2] (cplx: r runs over
 *   re, im pairs), strides in doubles: the column j of H, hcol = &H[0, 0, j], sHr = m (2 m for cplx).  The Arnoldi
 *   column is the sum of the coefficients of the two projecting passes; dst = &H[0, j + 1, j] receives the norm.
 *   XK_ERR_ARG: what xk_gkl_finish refuses, cplx / accumulate not 0 or 1, cplx with an even nval, sHr below one
 *   entry, Bt > 1 with members of the column overlapping.
 * xk_arn_schur: one workgroup per member, complex double in LDS, m <= xk_arn_max_rows().  With B = H[b, :m, :m] and
 *   beta = H[b, m, m - 1]: Schur form B = Z T Z^H (Householder reduction to Hessenberg form, single-shift QR with
 *   Wilkinson and exceptional shifts, at most 30 m iterations), the eigenvalues ranked by which (0 largest modulus, 1
 *   largest real part, 2 smallest real part, 3 largest imaginary part, 4 smallest imaginary part; 3 and 4 for cplx
 *   only) and the first keep' brought to the leading positions of T.  keep' = keep + keep_add[b] (keep_add may be
 *   NULL), moved by one when the cut would separate a complex-conjugate pair of a real B (partners share their rank,
 *   positive imaginary part first), never above m - 1.  Outputs: theta (Bt, m) complex, in rank order; Y (Bt, m, neig)
 *   complex, unit Ritz vectors of the first neig (columns); res (Bt, neig) = |beta| |Y[m - 1, i]|; Q (Bt, m, m) in
 *   H's element type, the restart coefficients in columns < keep' (the rest 0): Z[:, :keep'] for cplx, for a real B a
 *   REAL orthonormal basis of the same space (column-pivoted Gram-Schmidt, applied twice, of [Re Z | Im Z]); Hnext
 *   (Bt, m + 1, m), not H: Q^H B Q in the leading block, beta Q[m - 1, :keep'] in row keep', 0 elsewhere; status
 *   (Bt, xk_arn_status_words()) = {number of i < neig with res <= tol * max(|theta_i|, u |B|_F), QR iterations, flags,
 *   keep', brk[b] (brk NULL: -1), 0, 0, 0}.  Flags: 1 a non-finite entry (nothing else is written), 2 the QR
 *   iteration limit was hit (nothing else is written), 4 the real basis does not close under conjugation (a column
 *   longer than 1e-8 is left after keep' vectors: call again with keep_add[b] one larger), 8 keep' != keep.
 *   XK_ERR_ARG: m < 2 or beyond the cap, not 1 <= neig <= keep <= m - 1, which out of range, a null output. */
int xk_arn_max_rows(void);
int xk_arn_status_words(void);
int xk_arn_finish(const double* part, int Bt, int nval, int nchunk, double* coef, long sC, double* nrm, double* rnrm,
                  double* hcol, long sHb, long sHr, int cplx, int accumulate, double* dst, long sdst, double* smax,
                  double u, int* brk, int code, void* stream);
int xk_arn_schur(const double* H, int Bt, int m, int neig, int keep, const int* keep_add, int which, int cplx,
                 double tol, double u, const int* brk, double* theta, double* Y, double* res, double* Q, double* Hnext,
                 int* status, void* stream);

/* ---- factorised sparse approximate inverse of a Hermitian CSR operator (extension: linalg.fsai; new symbols only, ABI
 * stays 2) -----------------------------------------------------------------------------------------------------------
 * xk_fsai_build: the values of the lower-triangular G with G A G^H ~ I on a given pattern.  Row i of G has the columns
 *   S_i = g_idx[g_ptr[i] .. g_ptr[i+1]): ascending, unique, all <= i, i itself LAST, 1 <= |S_i| <= xk_fsai_max_row().
 *   With A_JJ = A[S_i, S_i] = L L^H and L^H z = e_m the row is conj(z): diag(G A G^H) = 1, (G A)[i, j] = 0 for j in
 *   S_i other than i, G[i,i] real positive.  Of A (CSR a_ptr (N+1), a_idx, values a_val[b * sV + k], sV = 0 broadcasts
 *   one set over the batch) only the entries with column <= row are read and A is taken as Hermitian; duplicates add
 *   up in storage order, columns need not be sorted, the imaginary part of a diagonal entry is ignored.  a_nnz / g_nnz:
 *   the stored entries per member of A / of G (the kernel reads and writes no index beyond them).
 *   G values g_val[b * sG + k].  One wavefront per (row, member), no floating-point atomics: bit-reproducible.
 *   A row whose A_JJ is not numerically positive definite (a pivot <= 0 or not finite, or a solution that is not
 *   finite) becomes the Jacobi row, G[i,i] = 1 / sqrt(|a_ii|) (1 when a_ii is 0 or not finite), zeros elsewhere, and is
 *   counted in nfail[b] (B ints, zeroed by the call).  A row of the pattern outside the limits above is left
 *   unwritten and counted as well: the caller checks the pattern.
 *   XK_ERR_ARG (decided on the host, before any launch): a null pointer, N <= 0, B <= 0, a negative stride or count,
 *   g_nnz < N, members of G (or of A with sV != 0) that overlap, g_val overlapping a_val.
 *   Complex (_c128 / _c64): interleaved (re, im); strides and counts in whole complex elements. */
int xk_fsai_max_row(void);
int xk_fsai_build_f64(const int* a_ptr, const int* a_idx, const double* a_val, long sV, int a_nnz, const int* g_ptr,
                      const int* g_idx, double* g_val, long sG, int g_nnz, int* nfail, int N, int B, void* stream);
int xk_fsai_build_f32(const int* a_ptr, const int* a_idx, const float* a_val, long sV, int a_nnz, const int* g_ptr,
                      const int* g_idx, float* g_val, long sG, int g_nnz, int* nfail, int N, int B, void* stream);
int xk_fsai_build_c128(const int* a_ptr, const int* a_idx, const double* a_val, long sV, int a_nnz, const int* g_ptr,
                       const int* g_idx, double* g_val, long sG, int g_nnz, int* nfail, int N, int B, void* stream);
int xk_fsai_build_c64(const int* a_ptr, const int* a_idx, const float* a_val, long sV, int a_nnz, const int* g_ptr,
                      const int* g_idx, float* g_val, long sG, int g_nnz, int* nfail, int N, int B, void* stream);

/* ---- unsymmetric factorised sparse approximate inverse of a CSR operator (extension: linalg.fsai_lu; new symbols only,
 * ABI stays 2) --------------------------------------------------------------------------------------------------------
 * xk_fsai_lu_build: the values of the two triangular factors with G_L A G_U ~ I on ONE lower-triangular pattern.  Row i
 *   has the columns S_i = g_idx[g_ptr[i] .. g_ptr[i+1]): ascending, unique, all <= i, i itself LAST,
 *   1 <= |S_i| <= xk_fsai_lu_max_row().  With A_SS = A[S_i, S_i] (both triangles as stored), A_SS u = e_m and
 *   A_SS^T g = e_m from one LU with partial pivoting (pivot: the largest |re| + |im|, ties to the lowest row):
 *   gl_val holds row i of G_L = g / g_m (unit diagonal), w_val row i of W = G_U^H = conj(u), so that
 *   (G_L A)[i, j] = 0 and (A G_U)[j, i] = 0 for j in S_i other than i and diag(G_L A G_U) = 1.  The preconditioner is
 *   P x = G_U (G_L x) = W^H (G_L x), its adjoint P^H x = G_L^H (W x): xk_csr_mm twice.
 *   Of A (CSR a_ptr (N+1), a_idx, values a_val[b * sV + k], sV = 0 broadcasts one set over the batch) every stored
 *   entry is read; duplicates add up in storage order, columns need not be sorted, nothing is made real.  a_nnz /
 *   g_nnz: the stored entries per member of A / of each factor (no index beyond them is read or written).  Factor
 *   values gl_val[b * sG + k], w_val[b * sG + k].  One wavefront per (row, member), no floating-point atomics:
 *   bit-reproducible.
 *   A row with a pivot that is exactly zero or not finite, a u or g that is not finite, or g_m = 0 becomes
 *   G_L[i, .] = e_i, G_U[., i] = e_i / a_ii (e_i when a_ii, duplicates summed, is zero or not finite) and is counted in
 *   nfail[b] (B ints, zeroed by the call).  A row of the pattern outside the limits above is left unwritten and
 *   counted as well: the caller checks the pattern.
 *   XK_ERR_ARG (decided on the host, before any launch): a null pointer, N <= 0, B <= 0, a negative stride or count,
 *   g_nnz < N, members of a factor (or of A with sV != 0) that overlap, gl_val or w_val overlapping a_val or each other.
 *   Complex (_c128 / _c64): interleaved (re, im); strides and counts in whole complex elements. */
int xk_fsai_lu_max_row(void);
int xk_fsai_lu_build_f64(const int* a_ptr, const int* a_idx, const double* a_val, long sV, int a_nnz, const int* g_ptr,
                         const int* g_idx, double* gl_val, double* w_val, long sG, int g_nnz, int* nfail, int N, int B,
                         void* stream);
int xk_fsai_lu_build_f32(const int* a_ptr, const int* a_idx, const float* a_val, long sV, int a_nnz, const int* g_ptr,
                         const int* g_idx, float* gl_val, float* w_val, long sG, int g_nnz, int* nfail, int N, int B,
                         void* stream);
int xk_fsai_lu_build_c128(const int* a_ptr, const int* a_idx, const double* a_val, long sV, int a_nnz, const int* g_ptr,
                          const int* g_idx, double* gl_val, double* w_val, long sG, int g_nnz, int* nfail, int N, int B,
                          void* stream);
int xk_fsai_lu_build_c64(const int* a_ptr, const int* a_idx, const float* a_val, long sV, int a_nnz, const int* g_ptr,
                         const int* g_idx, float* gl_val, float* w_val, long sG, int g_nnz, int* nfail, int N, int B,
                         void* stream);

/* ---- block Davidson for COMPLEX Hermitian operators (complex64 = _c64, complex128 = _c128; ABI 2) --------------
 * The reference's davidson (xitorch/_impls/linalg/symeig.py:100-227) uses unconjugated transposes and is real-only;
 * these are the complex counterparts of K3t / xk_ritz_residual / the panel CholeskyQR, with conjugate transposes.
 * Pointers address INTERLEAVED (re, im) storage; every stride and length counts COMPLEX elements; lam is real.
 * The tall products (V^H W, V C, V^H AW, W^H AW) run on the real K1 kernels through the interleaved storage.
 *
 * xk_herm_eigh: lowest (uppest = 0) / uppermost p eigenpairs of the Hermitian T[b] (B, k, k), lower triangle read,
 *   imaginary part of the diagonal ignored: lam (B, p) ascending, Y (B, p, k) with Y[b, j] the j-th eigenvector,
 *   info[b] = 1 when the self-check failed (tridiagonal residuals, orthonormality, scale range 2^-450 .. 2^450 for
 *   c128 / 2^-50 .. 2^50 for c64): repeat that member on a library eigh.  Householder reduction to a REAL symmetric
 *   tridiagonal (reflectors chosen so that the sub-diagonal is real), bisection, inverse iteration,
 *   back-transformation.  One workgroup per matrix, packed triangle in LDS.  Limits: 1 <= p <= 16, p <= k <= 128
 *   (both types; xk_herm_eigh_lds_bytes(k, p, 8 | 4) <= 160 KiB).  ws: xk_herm_eigh_workspace_elems(B, k, p)
 *   real elements (inverse-iteration factors), ws_elems its size.
 * xk_herm_ritz: X = Y^T V, Tn = -R with R = Y^T AV - diag(lam) Y^T MV (MV = NULL: V), status[1 + b] = max |R_b|
 *   (complex modulus) and status[0] = max over b; status (B + 1 doubles) is zeroed by the call, the maxima are integer
 *   maxima of the bit patterns (order-independent, a NaN propagates).  V, AV, MV: (B, >= k, ld) panels; Y (B, k, p)
 *   with strides (sY, sYa, sYc); lam (B, p) with unit stride along p.  V / AV / MV are read once per 16 columns.
 * xk_herm_cholqr: CholeskyQR of the q-vector block W (B, q, ld) in the (M-)inner product, in place:
 *   G = W^H MW (MW = NULL: W), fixed summation order (bit-reproducible), G + shift_rel trace(G) I = R^H R,
 *   W <- W R^-1 and MW <- MW R^-1; Rinv: scratch of B q q complex elements (holds R^-1 afterwards).  info[b] =
 *   index + 1 of the first non-positive pivot if info[b] was 0 (sticky; the pivot is then taken as 1).  q <= 32. */
long xk_herm_eigh_lds_bytes(int k, int p, int elem_size);
long xk_herm_eigh_workspace_elems(int B, int k, int p);
int xk_herm_eigh_c128(const double* T, double* lam, double* Y, int* info, double* ws, long ws_elems, int B, int k,
                      int p, int uppest, long ldt, long sT, void* stream);
int xk_herm_eigh_c64(const float* T, float* lam, float* Y, int* info, float* ws, long ws_elems, int B, int k, int p,
                     int uppest, long ldt, long sT, void* stream);
int xk_herm_ritz_c128(const double* V, const double* AV, const double* MV, const double* Y, const double* lam,
                      double* X, double* Tn, double* status, int B, int k, int N, int p, long ldv, long sV, long ldav,
                      long sAV, long ldmv, long sMV, long sY, long sYa, long sYc, long sL, long ldx, long sX,
                      long ldtn, long sTn, void* stream);
int xk_herm_ritz_c64(const float* V, const float* AV, const float* MV, const float* Y, const float* lam, float* X,
                     float* Tn, double* status, int B, int k, int N, int p, long ldv, long sV, long ldav, long sAV,
                     long ldmv, long sMV, long sY, long sYa, long sYc, long sL, long ldx, long sX, long ldtn,
                     long sTn, void* stream);
int xk_herm_cholqr_c128(double* W, double* MW, double* Rinv, int* info, int B, int q, int N, long ldw, long sW,
                        long ldmw, long sMW, double shift_rel, void* stream);
int xk_herm_cholqr_c64(float* W, float* MW, float* Rinv, int* info, int B, int q, int N, long ldw, long sW,
                       long ldmw, long sMW, double shift_rel, void* stream);

/* ---- fused BLAS-1 of the quasi-Newton (Broyden) driver -------------------------------------------------
 * The reference's _nonlin_solver / LowRankMatrix (xitorch/_impls/optimize/root/rootsolver.py:96-143,
 * _jacobian.py:99-119,172-189) run torch.dot / .norm() / axpy chains on one flat length-L vector with a host sync
 * after almost every one.
 * xk_vec_dots: out[i] = <a_i, b_i>, i < npairs <= 4, in one streaming pass + a fixed-order device fold (double
 *   results; `partials`: scratch of xk_vec_dots_workspace_elems() doubles).  Replaces the y.norm(), dx.norm(),
 *   x.norm(), torch.dot calls of rootsolver.py:100,113,286-290,375-380 — the driver reads them with ONE sync.
 * xk_broyden_axpy: out = g0*u0 + g1*u1 + gamma * sum_{n<k} coef[n]*scale[n] * V[n*ldv + :]  (u0/u1/scale may be
 *   NULL; out must not alias V).  Replaces LowRankMatrix.mv/rmv's Python loop of axpys (_jacobian.py:172-182) and
 *   the update formulas of BroydenFirst/Second (_jacobian.py:112-119,132-137); `scale[n]` carries 1/<dy_n, v_n>. */
long xk_vec_dots_workspace_elems(void);
int xk_vec_dots_f64(const double* a0, const double* b0, const double* a1, const double* b1, const double* a2,
                    const double* b2, const double* a3, const double* b3, int npairs, long L, double* partials,
                    long npart, double* out, void* stream);
int xk_vec_dots_f32(const float* a0, const float* b0, const float* a1, const float* b1, const float* a2,
                    const float* b2, const float* a3, const float* b3, int npairs, long L, double* partials,
                    long npart, double* out, void* stream);
int xk_broyden_axpy_f64(double* out, const double* u0, double g0, const double* u1, double g1, const double* V,
                        long ldv, const double* coef, const double* scale, int k, double gamma, long L, void* stream);
int xk_broyden_axpy_f32(float* out, const float* u0, double g0, const float* u1, double g1, const float* V, long ldv,
                        const float* coef, const float* scale, int k, double gamma, long L, void* stream);

/* ---- LSMR step kernels (xk_lsmr.hip; extension, no reference counterpart): least squares min |A x - b|^2 + damp^2 |x|^2
 * with a rectangular operator (Fong & Saunders 2011).  Vectors are (S, ld) arrays as above (u side: length m, v side:
 * length n; _c128 / _c64: interleaved complex, N and ld in complex elements); partial buffers are
 * (S, xk_kry_max_partials()) REAL elements of the vector's precision.  The per-system scalars are DOUBLES whatever the
 * vector type: state is (2, S, xk_lsmr_state_len()) doubles, step k reads slot k & 1 and xk_lsmr_update writes slot
 * (k + 1) & 1.  Entry i of a slot: 0 alpha (0: start), 1 beta, 2 alphabar, 3 zetabar, 4 rho, 5 rhobar, 6 cbar, 7 sbar,
 * 8 zeta, 9 betadd, 10 betad, 11 rhodold, 12 tautildeold, 13 thetatilde, 14 d, 15 normA^2, 16 maxrbar, 17 minrbar,
 * 18 steps taken, 19 stop code (0 running, 1 S1, 2 S2, 3 S3 = conlim, 4 alpha = 0, 5 beta = 0), 20 |b|, 21 |rbar|,
 * 22 |Abar^H rbar|, 23 |A| (the Frobenius norm of the bidiagonal, capped by an estimate of |A|_2 so that it stays
 * below |A|_F when the Lanczos vectors lose orthogonality), 24 cond(Abar), 25 the |x| the S1 test used, 26 alpha_1.  Systems with a non-zero
 * stop code are frozen: their state is carried from slot to slot and nothing else of theirs is written.
 * xk_lsmr_init: beta_1 = sqrt(sum Pb); uh <- b; slot k & 1 (alpha = 0); beta_1 = 0: stop code 1; run[s * 64] <- 1 / 0.
 * xk_lsmr_bidiag: y <- Op / nu_x - (nu_x / nu_y) y, nu_x = sqrt(sum of the nblk_in partials Pin), nu_y = beta (half 0,
 *   the u half) or alpha (half 1, the v half; 0: y is not read); Pout <- the nblk block partials of |y|^2; nu_x = 0: y
 *   stays and the partials are 0.
 * xk_lsmr_update: beta_{k+1} = sqrt(sum of the nblk_u partials Pu), alpha_{k+1} = sqrt(sum Pv); rotations; hbar <- h - c1
 *   hbar, x <- x + c2 hbar, h <- vh / alpha_{k+1} - c3 h; Pxout <- partials of |x|^2 (Pxin: those of the step before);
 *   estimates and stop code into slot (k + 1) & 1; run[s * 64] <- 1 while the system runs, else 0 (a one-partial
 *   array for xk_kry_status with nblk = 1 and stop = 0.5).  On a start slot only h <- vh / alpha_1 and the state.
 * XK_ERR_ARG, nothing launched: N <= 0, S < 0, k < 0, nblk (nblk_in, nblk_u) outside 1 .. 64, ld below N rounded up
 *   to the 16 B vector, a NULL pointer, aliased vectors, damp < 0.  XK_ERR_UNSUPPORTED, nothing launched: a vector
 *   pointer or a pitch that is not 16 B aligned. */
int xk_lsmr_state_len(void);
int xk_lsmr_init_f64(const double* b, double* uh, const double* Pb, double* state, double* run, int S, int N, long ld, int nblk,
                     int k, void* stream);
int xk_lsmr_bidiag_f64(const double* Op, double* y, const double* Pin, double* Pout, const double* state, int half, int S, int N,
                       long ld, int nblk, int nblk_in, int k, void* stream);
int xk_lsmr_update_f64(const double* vh, double* h, double* hbar, double* x, const double* Pu, const double* Pv, const double* Pxin, double* Pxout,
                       double* state, double* run, int S, int N, long ld, int nblk, int nblk_u, int k, double damp,
                       double atol, double btol, double conlim, void* stream);
int xk_lsmr_init_f32(const float* b, float* uh, const float* Pb, double* state, float* run, int S, int N, long ld, int nblk,
                     int k, void* stream);
int xk_lsmr_bidiag_f32(const float* Op, float* y, const float* Pin, float* Pout, const double* state, int half, int S, int N,
                       long ld, int nblk, int nblk_in, int k, void* stream);
int xk_lsmr_update_f32(const float* vh, float* h, float* hbar, float* x, const float* Pu, const float* Pv, const float* Pxin, float* Pxout,
                       double* state, float* run, int S, int N, long ld, int nblk, int nblk_u, int k, double damp,
                       double atol, double btol, double conlim, void* stream);
int xk_lsmr_init_c128(const double* b, double* uh, const double* Pb, double* state, double* run, int S, int N, long ld, int nblk,
                     int k, void* stream);
int xk_lsmr_bidiag_c128(const double* Op, double* y, const double* Pin, double* Pout, const double* state, int half, int S, int N,
                       long ld, int nblk, int nblk_in, int k, void* stream);
int xk_lsmr_update_c128(const double* vh, double* h, double* hbar, double* x, const double* Pu, const double* Pv, const double* Pxin, double* Pxout,
                       double* state, double* run, int S, int N, long ld, int nblk, int nblk_u, int k, double damp,
                       double atol, double btol, double conlim, void* stream);
int xk_lsmr_init_c64(const float* b, float* uh, const float* Pb, double* state, float* run, int S, int N, long ld, int nblk,
                     int k, void* stream);
int xk_lsmr_bidiag_c64(const float* Op, float* y, const float* Pin, float* Pout, const double* state, int half, int S, int N,
                       long ld, int nblk, int nblk_in, int k, void* stream);
int xk_lsmr_update_c64(const float* vh, float* h, float* hbar, float* x, const float* Pu, const float* Pv, const float* Pxin, float* Pxout,
                       double* state, float* run, int S, int N, long ld, int nblk, int nblk_u, int k, double damp,
                       double atol, double btol, double conlim, void* stream);

/* ---- stochastic Lanczos quadrature (xk_slq.hip; extension, no reference counterpart): z^H f(A) z of a Hermitian
 * operator by Gauss quadrature on the Lanczos tridiagonal.  Vectors are (S, ld) arrays as above (_c128 / _c64:
 * interleaved complex, N and ld in complex elements); Pb and Pa are the partials xk_kry_dots writes ((S, 64) real, or
 * (S, 64, 2) (re, im) pairs for the complex types, of which the real part is used), Pin / Pout are (S, 64) REAL
 * partials of |y|^2.  The per-system scalars are DOUBLES whatever the vector type: state is (2, S, xk_slq_state_len())
 * doubles, step k reads slot k & 1 and writes slot (k + 1) & 1.  Entry i of a slot: 0 beta (norm of the Lanczos vector
 * of the last step; after init |z|), 1 the norm before it (0: none), 2 flag (0 running, 1 frozen by a breakdown, 2
 * z = 0), 3 m (steps recorded), 4 tnorm (running maximum row sum of the Jacobi matrix), 5 the last row's sum short of
 * its next beta, 6 |z|^2, 7 the last alpha.  Tal, Tbe: (S, nsteps) doubles; the Jacobi matrix of system s is
 * diag(Tal[s, 0 .. m)) with the off-diagonal Tbe[s, 1 .. m) (Tbe[s, 0] = |z|).
 * xk_slq_init: beta_1 = sqrt(sum Pb); r2 <- z; the start state into slot k & 1 (z = 0: flag 2).
 * xk_slq_step: beta = sqrt(sum Pin) (first step: the state's); beta <= 64 eps tnorm (eps: machine epsilon of the
 *   vector type): the system is frozen (flag 1) and nothing else of it is written, now or later; else alpha =
 *   sum Pa / beta^2, r1 <- W / beta - (alpha / beta) r2 - (beta / oldb) r1 (first step: r1 is not read), Pout <- the
 *   nblk block partials of |r1|^2, Tal[s, m] <- alpha, Tbe[s, m] <- beta, m + 1 and the rest into slot (k + 1) & 1.
 *   The caller swaps r1 and r2, and Pin and Pout.
 * xk_slq_quad (double, whatever the vector type): for every system the eigenvalues theta[s, 0 .. m) and the squared
 *   first eigenvector components weight[s, 0 .. m) of its Jacobi matrix (implicit QL; entries [m, nsteps) are set to
 *   0), out[s] = |z|^2 sum_k weight f(theta) with fn 0 log, 1 1/x, 2 sqrt, 3 1/sqrt, 4 exp(param x), 5 x, and flag[s]:
 *   bit 0 a node <= 0 under fn 0 .. 3, bit 1 the QL iteration did not converge; a flagged system's out is NaN.
 *   m and |z|^2 are read from slot k & 1.
 * XK_ERR_ARG, nothing launched: N <= 0 or beyond 2^31 - 1 real elements (complex: 2 N), S < 0, k < 0, nblk outside
 *   1 .. 64, ld below N rounded up to the 16 B vector, a NULL pointer, aliased arrays, nsteps outside 1 .. 128, an
 *   unknown fn.  XK_ERR_UNSUPPORTED, nothing launched: a
 *   vector pointer or a pitch that is not 16 B aligned.  S = 0 returns 0 and launches nothing. */
int xk_slq_state_len(void);
int xk_slq_init_f64(const double* z, double* r2, const double* Pb, double* state, int S, int N, long ld, int nblk, int k,
                    void* stream);
int xk_slq_step_f64(const double* W, const double* r2, double* r1, const double* Pa, const double* Pin, double* Pout,
                    double* state, double* Tal, double* Tbe, int S, int N, long ld, int nblk, int nsteps, int k,
                    void* stream);
int xk_slq_init_f32(const float* z, float* r2, const float* Pb, double* state, int S, int N, long ld, int nblk, int k,
                    void* stream);
int xk_slq_step_f32(const float* W, const float* r2, float* r1, const float* Pa, const float* Pin, float* Pout,
                    double* state, double* Tal, double* Tbe, int S, int N, long ld, int nblk, int nsteps, int k,
                    void* stream);
int xk_slq_init_c128(const double* z, double* r2, const double* Pb, double* state, int S, int N, long ld, int nblk, int k,
                     void* stream);
int xk_slq_step_c128(const double* W, const double* r2, double* r1, const double* Pa, const double* Pin, double* Pout,
                     double* state, double* Tal, double* Tbe, int S, int N, long ld, int nblk, int nsteps, int k,
                     void* stream);
int xk_slq_init_c64(const float* z, float* r2, const float* Pb, double* state, int S, int N, long ld, int nblk, int k,
                    void* stream);
int xk_slq_step_c64(const float* W, const float* r2, float* r1, const float* Pa, const float* Pin, float* Pout,
                    double* state, double* Tal, double* Tbe, int S, int N, long ld, int nblk, int nsteps, int k,
                    void* stream);
int xk_slq_quad(const double* Tal, const double* Tbe, const double* state, double* theta, double* weight, double* out,
                int* flag, int S, int nsteps, int k, int fn, double param, void* stream);

/* ---- f(A) B by two-pass Lanczos (xk_fnm.hip; extension, no reference counterpart).  Pass 1 is the xk_slq_init /
 * xk_slq_step run above on the start vectors b; the entry points here turn its Tal, Tbe and state into the coefficients
 * of f(A) b in the Lanczos basis and replay the recurrence to accumulate X = sum_k (c_k / beta_k) r2_k without a stored
 * basis.  Vectors, pitches, Tal, Tbe and state are laid out as in the xk_slq block.
 * xk_fnm_eig (double, whatever the vector type): for every system the eigenvalues theta[s, 0 .. m) and the eigenvector
 *   matrix of its Jacobi matrix by implicit QL with the rotations accumulated: Qt (S, nsteps, nsteps) doubles,
 *   COLUMN-major: Qt[s, k, j] is component j of the eigenvector of theta[s, k].  Entries at and beyond m are set to 0.
 *   flag[s] (int): 2 when QL did not converge within the sweep cap of xk_slq_quad, else 0.  m is read from slot k & 1.
 * xk_fnm_coeff: C[s, j] = |b_s| sum_k Qt[s, k, j] f_k Qt[s, k, 0], k ascending, for j < m; 0 for j >= m.  fn 0 .. 5:
 *   f_k = the named function of xk_slq_quad at theta[s, k] (param: fn 4); a node <= 0 under fn 0 .. 3 sets bit 0 of
 *   flag[s].  fn = -1: f_k = fvals[s, k], the caller's values of the function at theta ((S, nsteps) doubles; cplx != 0:
 *   (S, nsteps, 2) (re, im) pairs).  C is (S, nsteps) doubles, or (S, nsteps, 2) pairs when cplx != 0 (a named function
 *   has imaginary part 0).  flag[s] must hold what xk_fnm_eig wrote; a flagged system's C[s, 0 .. m) is NaN.
 *   tail[s] = |C[s, m-4 .. m)| / |C[s, 0 .. m)| in the 2-norm, 0 when m <= 4.  m and |b|^2 are read from slot k & 1.
 * xk_fnm_step: step k of pass 2 for every system with k < m (m and the flag from slot kstate & 1) whose flag is not 2:
 *   X += (C[s, k] / Tbe[s, k]) r2 (_c128 / _c64: C holds (re, im) pairs); then, unless `last` != 0 or k + 1 = m,
 *   r1 <- (W c0 - c2 r2) - c1 r1 with c0 = 1 / beta, c2 = alpha / beta, c1 = beta / Tbe[s, k - 1] formed from
 *   alpha = Tal[s, k], beta = Tbe[s, k] exactly as xk_slq_step forms them, so that r1 is the vector pass 1 wrote, bit
 *   for bit (k = 0: no r1 term, r1 is not read).  The caller swaps r1 and r2.  W == NULL means last; r1 may then be
 *   NULL too.  Every other system is left untouched.
 * XK_ERR_ARG / XK_ERR_UNSUPPORTED: as in the xk_slq block; also k >= nsteps or kstate < 0 (xk_fnm_step), fn outside
 *   -1 .. 5 or fn = -1 without fvals (xk_fnm_coeff).  XK_ERR_UNSUPPORTED also when xk_slq_state_len() is not the state
 *   length these entry points were written for. */
int xk_fnm_eig(const double* Tal, const double* Tbe, const double* state, double* theta, double* Qt, int* flag, int S,
               int nsteps, int k, void* stream);
int xk_fnm_coeff(const double* Qt, const double* theta, const double* state, const double* fvals, double* C,
                 double* tail, int* flag, int S, int nsteps, int k, int fn, double param, int cplx, void* stream);
int xk_fnm_step_f64(const double* W, const double* r2, double* r1, double* X, const double* C, const double* Tal,
                    const double* Tbe, const double* state, int S, int N, long ld, int nblk, int nsteps, int k,
                    int kstate, int last, void* stream);
int xk_fnm_step_f32(const float* W, const float* r2, float* r1, float* X, const double* C, const double* Tal,
                    const double* Tbe, const double* state, int S, int N, long ld, int nblk, int nsteps, int k,
                    int kstate, int last, void* stream);
int xk_fnm_step_c128(const double* W, const double* r2, double* r1, double* X, const double* C, const double* Tal,
                     const double* Tbe, const double* state, int S, int N, long ld, int nblk, int nsteps, int k,
                     int kstate, int last, void* stream);
int xk_fnm_step_c64(const float* W, const float* r2, float* r1, float* X, const double* C, const double* Tal,
                    const double* Tbe, const double* state, int S, int N, long ld, int nblk, int nsteps, int k,
                    int kstate, int last, void* stream);

/* ---- device-side collectives of the sharded solvers (RCCL over xGMI) -------------------------
 * The per-iteration exchanges that reproduce the reference's GLOBAL decisions under batch sharding — MAX of
 * {max|resid|, flags} (xitorch/_impls/linalg/symeig.py:188-203), MAX of {max residual norm, unconverged flag}
 * (_impls/linalg/solve.py:157,166,301,310), SUM of the Broyden inner products (_impls/optimize/root/_jacobian.py:172-182) —
 * as in-place all-reduces enqueued on the caller's stream, right behind the kernel that wrote the few doubles: the
 * host's one status read per iteration then returns reduced values.  librccl is looked up at the first call (the copy
 * the process already maps first); without it every entry point returns -2.  No RCCL type crosses the ABI.
 * xk_comm_available: 1 when a librccl was found.
 * xk_comm_unique_id: fills 128 opaque bytes on ONE rank; the caller distributes them (any side channel).
 * xk_comm_init_rank: this process' communicator of `nranks` ranks on HIP device `device` (collective over the ranks).
 * xk_comm_init_all: ndev communicators of one process, one per device devs[i] (devs == NULL: 0 .. ndev-1).
 * xk_comm_size: ranks / this rank of a communicator.   xk_comm_destroy: releases it (NULL: no-op).
 * xk_allreduce_f64 / _f32: buf[0..n) <- reduction over the ranks, op 0 = SUM, 1 = MAX, 2 = MIN, in place, on `stream`.
 *   One communicator serves one stream at a time.  Return codes: 0 ok, < 0 argument / unsupported, 1000 + ncclResult_t. */
int xk_comm_available(void);
int xk_comm_unique_id(void* id128);
int xk_comm_init_rank(const void* id128, int nranks, int rank, int device, void** comm);
int xk_comm_init_all(int ndev, const int* devs, void** comms);
int xk_comm_size(void* comm, int* nranks, int* rank);
int xk_comm_destroy(void* comm);
int xk_allreduce_f64(void* comm, double* buf, long n, int op, void* stream);
int xk_allreduce_f32(void* comm, float* buf, long n, int op, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* XITORCH_AMD_H */
