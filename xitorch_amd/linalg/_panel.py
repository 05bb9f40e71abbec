"""The panel layer every native driver stands on: the panel layout, its geometry rules and the operator applies.

A *panel* is a padded device array (Bt, p, ld): Bt batch members, p vectors each, every vector a
contiguous length-N run (ld >= N, pads zero) — the reference's Fortran-order (.., N, p) view
(xitorch/_utils/tensor.py:21-32) seen as its transpose.

Geometry, stated once: `pad_len` (the pitch), `batch_count`, `real_dtype`, `kry_blocks` (workgroups = partial sums per
system of the fused Krylov kernels) and `require_hip` (the device / dtype guard of every driver).

`RectPanelOperator.apply` computes out[b, c, :m] = A_b x[b, c, :n] (or A_b^H on the swapped lengths) without any layout
copies for the native storage kinds; `PanelOperator` is the square case of the eigensolvers and Krylov solvers:

  MatrixLinearOperator  -> xk_dense_mm   (K1; square: column-oriented variant when the matrix is symmetric, K1s / K1sw
                                          on exactly symmetric storage)
  BandedLinearOperator  -> xk_banded_mm
  SparseLinearOperator  -> xk_csr_mm     (fp32 / fp64 / complex64 / complex128 values; the adjoint on the pattern's
                                          CSC view, complex values conjugated by the kernel)
  FSAIOperator          -> xk_csr_mm twice (G, then G^H on G's CSC view) through a cached scratch panel (square only)
  FSAILUOperator        -> xk_csr_mm twice (G_L, then W^H; the adjoint: W, then G_L^H) on the one pattern, same scratch
  anything else         -> the operator's own .mm/.rmm on the (.., N, p) strided view
"""
import math
import torch
from xitorch_amd import kernels as K
from xitorch_amd._capi import NativeLibraryError, fn

__all__ = ["PanelOperator", "RectPanelOperator", "pad_len", "batch_count", "real_dtype", "kry_blocks", "require_hip",
           "to_panel", "from_panel"]

K1S_MIN_BYTES = 1.5e9      # operator storage from which the upper-triangle kernel K1s beats the full-matrix kernels
REAL_DTYPES = (torch.float64, torch.float32)
COMPLEX_DTYPES = (torch.complex128, torch.complex64)
VEC_ELEMS = {torch.float64: 2, torch.float32: 4, torch.complex128: 1, torch.complex64: 2}     # elements per 16 B vector


def pad_len(n):
    return (n + 7) // 8 * 8     # elements: keeps every vector 64 B aligned for f64 and f32


def batch_count(bdims):
    """number of batch members of a batch shape (1 for `()`)"""
    return math.prod(bdims)


def real_dtype(dtype):
    """element type of the kernels' norms, scalars and partial sums: the real type of the same precision"""
    return {torch.complex128: torch.float64, torch.complex64: torch.float32}.get(dtype, dtype)


def kry_blocks(N, dtype):
    """Workgroups (= partial sums) per system of the fused Krylov kernels on vectors of length N: one per 256 threads x
    4 vectors of 16 B, at most xk_kry_max_partials().  The kernels read exactly this many partials."""
    per_block = 256 * VEC_ELEMS[dtype] * 4
    return max(1, min(fn("xk_kry_max_partials")(), (N + per_block - 1) // per_block))


def require_hip(A, who):
    """The native drivers serve float64 / float32 / complex128 / complex64 operators on a HIP device and nothing else."""
    device = torch.device(A.device)
    if device.type != "cuda":
        raise NativeLibraryError("xitorch_amd %s runs on a HIP device only (operator is on %s)" % (who, device))
    if A.dtype not in REAL_DTYPES + COMPLEX_DTYPES:
        raise NativeLibraryError("xitorch_amd %s supports float64/float32 and complex128/complex64 operators, got %s"
                                 % (who, A.dtype))


def to_panel(X, bdims, Bt, N):
    """(*batch, N, p) (broadcastable to bdims) -> zero-padded panel (Bt, p, ld)."""
    p = X.shape[-1]
    out = torch.zeros((Bt, p, pad_len(N)), dtype=X.dtype, device=X.device)
    out[:, :, :N].copy_(X.expand(*bdims, N, p).reshape(Bt, N, p).transpose(-2, -1))
    return out


def from_panel(P, bdims, N):
    """panel (Bt, p, ld) -> (*bdims, N, p) (a strided view, Fortran order like the reference's)."""
    return P[:, :, :N].transpose(-2, -1).reshape(*bdims, N, P.shape[1])


def _native(t, dtypes=REAL_DTYPES + COMPLEX_DTYPES):
    return t.is_cuda and t.dtype in dtypes


def _csr_values(S):
    """the stored values of a SparseLinearOperator as (nA, nnz) rows of unit stride (a lazily conjugated view: its
    numbers)"""
    vals = S.values.resolve_conj().reshape(-1, S.nnz)
    return vals.contiguous() if S.nnz > 1 and vals.stride(-1) != 1 else vals


class RectPanelOperator:
    """Panel apply of a rectangular operator (*BA, m, n): out[:, :, :m] = A x[:, :, :n] or out[:, :, :n] = A^H x[:, :, :m]
    on (Bt, p, ld) panels, without layout copies for the native storage kinds.  `kind` says which one serves the
    operator: "dense" (`mat`, with the orientation flags `flip` / `cj` of a transposed / lazily conjugated view),
    "banded" (`band`), "csr" (`pat`, `vals`), or "generic": the operator's own .mm / .rmm."""

    def __init__(self, A, bdims, Bt):
        from xitorch_amd.linop import MatrixLinearOperator, BandedLinearOperator, SparseLinearOperator
        self.A, self.bdims, self.Bt = A, list(bdims), Bt
        self.m, self.n = A.shape[-2], A.shape[-1]
        self.kind = "generic"
        self.napply = 0
        self.torch_applies = 0      # applies served by the operator's own torch expression (.mm / .rmm)
        self.cplx, self.cj, self.flip = False, False, False
        nA = batch_count(A.shape[:-2])
        self.batch_ok = nA in (1, Bt)       # the native kernels take one operator per member, or one shared by all
        if not self.batch_ok:
            pass
        elif isinstance(A, MatrixLinearOperator) and _native(A.mat):
            mat = A.mat
            if mat.is_complex():
                # complex operator: applied by the real K1 kernels on its interleaved storage (K.dense_mm_complex);
                # lazily conjugated / transposed views (A.H = mat^T.conj()) only set orientation flags
                self.cplx = True
                if mat.is_conj():
                    mat, self.cj = mat.conj(), True
            flip = False
            if mat.dim() >= 2 and mat.stride(-1) != 1 and mat.stride(-2) == 1:
                mat, flip = mat.transpose(-2, -1), True           # a transposed view (e.g. A.H)
            if mat.is_contiguous() or mat.dim() == 2 and mat.stride(-1) == 1:
                self.kind, self.flip = "dense", flip
                self.mat = mat.reshape(nA, *mat.shape[-2:]) if mat.dim() > 2 else mat
        elif isinstance(A, BandedLinearOperator) and _native(A.band, REAL_DTYPES) and A.band.is_contiguous():
            self.kind = "banded"
            self.band = A.band.reshape(nA, *A.band.shape[-2:])
        elif isinstance(A, SparseLinearOperator) and _native(A.values):
            self.kind = "csr"
            self.cplx = A.values.is_complex()
            self.pat = A._pattern
            self.vals = _csr_values(A)

    def apply(self, X, out, trans=False):
        """X, out: (Bt, p, ld) panels; trans False: out[..., :m] = A X[..., :n]; True: out[..., :n] = A^H X[..., :m]"""
        self.napply += 1
        if self.kind != "generic":
            return self._native(X, out, trans)
        self.torch_applies += 1
        nin, nout = (self.m, self.n) if trans else (self.n, self.m)
        p = X.shape[1]
        x = X[:, :, :nin].transpose(-2, -1).reshape(*self.bdims, nin, p)
        y = self.A.rmm(x) if trans else self.A.mm(x)
        out[:, :, :nout].copy_(y.expand(*self.bdims, nout, p).reshape(self.Bt, nout, p).transpose(-2, -1))
        return out

    def _native(self, X, out, trans):
        nin, nout = (self.m, self.n) if trans else (self.n, self.m)
        Xn, On = X[:, :, :nin], out[:, :, :nout]
        if self.kind == "dense" and self.cplx:
            # stored matrix S, operator = S / S^T / conj(S) / S^H by (flip, cj); trans asks for the operator's adjoint
            K.dense_mm_complex(self.mat if self.mat.dim() == 3 else self.mat.unsqueeze(0), Xn,
                               adjoint=(self.flip != trans), conj_io=(self.flip != self.cj), out=On)
        elif self.kind == "dense":
            K.dense_mm(self.mat, Xn, out=On, trans=(trans != self.flip))
        elif self.kind == "csr":
            K.csr_mm(self.pat, self.vals, Xn, out=On, trans=trans)
        else:
            K.banded_mm(self.band, Xn, out=On, trans=trans)
        return out


class PanelOperator(RectPanelOperator):
    """The square operator (*BA, N, N) of the eigensolvers and the Krylov solvers: the rectangular apply plus what only
    a square operator has -- the symmetric-storage kernels K1s / K1sw and the column-oriented K1 of a verified
    symmetric matrix, the dropped `trans` of a Hermitian operator, FSAIOperator (kind "fsai"), FSAILUOperator (kind
    "fsai_lu"), `diagonal()`, the
    two-stream `apply_on` and the event hooks of the measurements."""

    def __init__(self, A, bdims, Bt, N):
        from xitorch_amd.linalg.precond import FSAIOperator, FSAILUOperator
        super().__init__(A, bdims, Bt)
        self.N = N
        self.symm = False
        self.symm_narrow = False
        self.last_kernel = None     # which panel kernel served the last native apply (K1s / K1w / K1wr / K1 / banded / csr / fsai / fsai_lu)
        self.events = None          # when a list: (start, end, p) HIP events around every native launch
        self.hermitian = bool(getattr(A, "is_hermitian", False))
        if self.kind == "dense":
            self.herm_verified = bool(getattr(A, "hermitian_verified", False))
            vn = VEC_ELEMS[self.mat.dtype]
            # exactly symmetric storage: stream the upper triangle only (K1s)
            self.symm = bool(getattr(A, "symmetric_storage", False)) and N % vn == 0 and \
                self.mat.stride(-2) % vn == 0 and not self.cplx
            # ... where that pays: K1s walks 1024-row tiles, one workgroup each, and has a floor of ~235 us per
            # launch (two launches) however small the operator; the one-launch full-matrix kernels are faster up to
            # ~1.5 GB of operator storage although they read twice the bytes (scripts/k1s_small_crossover.py,
            # profiles/r04_k1s_small_crossover.jsonl: 1 x 512^2 fp64 127 vs 11 us, 8 x 2048^2 236 vs 44, 4 x 4096^2
            # 238 vs 95)
            self.symm_narrow = self.symm and self.mat.numel() * self.mat.element_size() >= K1S_MIN_BYTES
        elif isinstance(A, FSAIOperator) and _native(A.G.values) and self.batch_ok:
            # P = G^H G: two CSR products on the padded panels
            self.kind = "fsai"
            self.cplx = A.G.values.is_complex()
            self.pat = A.G._pattern
            self.pat.csc()                    # the view of G^H, built here rather than in the first iteration
            self.vals = _csr_values(A.G)
            self._scratch = None              # G x; reallocated only when the column count grows
        elif isinstance(A, FSAILUOperator) and _native(A.GL.values) and _native(A.W.values) and self.batch_ok:
            # P = W^H G_L (adjoint flag: P^H = G_L^H W): two CSR products on the padded panels, one shared pattern
            self.kind = "fsai_lu"
            self.cplx = A.GL.values.is_complex()
            self.adjoint = A.adjoint
            self.pat = A.GL._pattern
            self.pat.csc()
            self.vals = _csr_values(A.GL)
            self.vals_w = _csr_values(A.W)
            self._scratch = None

    def diagonal(self):
        """diag(A) as a contiguous (nA, N) array (native operators only)."""
        if self.kind == "dense":
            mat = self.mat if self.mat.dim() == 3 else self.mat.unsqueeze(0)
            return mat.diagonal(dim1=-2, dim2=-1).contiguous()
        if self.kind == "banded":
            hb = (self.band.shape[-2] - 1) // 2
            return self.band[:, hb, :].contiguous()
        if self.kind == "csr":
            # once per solve: the stored entries on the diagonal, duplicates summed
            on = self.pat.row_of == self.pat.col
            d = torch.zeros((self.vals.shape[0], self.N), dtype=self.vals.dtype, device=self.vals.device)
            return d.index_add(1, self.pat.col[on].to(torch.int64), self.vals[:, on]).contiguous()
        raise NativeLibraryError("the diagonal of a generic LinearOperator is not available: pass it "
                                 "explicitly (precond=<tensor (*batch, N)>) or use a LinearOperator")

    def apply(self, X, out, trans=False):
        """out[:, :, :N] = A X  (trans: A^H X).  X, out: (Bt, p, ld)."""
        if self.hermitian:
            trans = False
        if self.events is None or self.kind == "generic":
            return super().apply(X, out, trans)
        self.napply += 1
        e0, e1 = K.timing_event_pair()
        e0.record()
        self._native(X, out, trans)
        e1.record()
        self.events.append((e0, e1, X.shape[1], X.shape[0]))
        return out

    def apply_on(self, X, out, k1_stream):
        """out = A X with the panel product running on `k1_stream` (the two-group pipeline's CU-masked stream)
        and the result ordered into the current stream.  For the symmetric-storage kernel only the tile kernel
        goes to `k1_stream`; its small fold runs on the current stream, off the panel-product critical path."""
        N = self.N
        if self.kind == "dense" and self.symm and self.symm_narrow and X.shape[1] <= 6 and not self.flip:
            self.napply += 1
            self.last_kernel = "K1s"
            e0, e1 = K.dense_symm_split(self.mat, X[:, :, :N], out[:, :, :N], k1_stream,
                                        timed=self.events is not None)
            if self.events is not None:
                self.events.append((e0, e1, X.shape[1], X.shape[0]))
            return out
        if self.kind == "dense" and self.symm and not self.flip and K.symm_wide_ok(self.mat, X[:, :, :N]):
            self.napply += 1
            self.last_kernel = "K1sw"
            e0, e1 = K.dense_symm_wide_split(self.mat, X[:, :, :N], out[:, :, :N], k1_stream,
                                             timed=self.events is not None)
            if self.events is not None:
                self.events.append((e0, e1, X.shape[1], X.shape[0]))
            return out
        cur = torch.cuda.current_stream()
        ready, done = K.sync_events(cur)            # cached per issuing stream, re-recorded on every launch
        ready.record(cur)
        with torch.cuda.stream(k1_stream):
            k1_stream.wait_event(ready)
            self.apply(X, out)
            done.record(k1_stream)
        cur.wait_event(done)
        return out

    def _native(self, X, out, trans):
        N = self.N
        if self.kind in ("fsai", "fsai_lu"):
            self.last_kernel = self.kind
            p = X.shape[1]
            if self._scratch is None or self._scratch.shape[0] != X.shape[0] or self._scratch.shape[1] < p or \
                    self._scratch.dtype != X.dtype:
                self._scratch = torch.empty((X.shape[0], p, N), dtype=X.dtype, device=X.device)
            scr = self._scratch[:, :p]
            first, second = self.vals, self.vals                   # fsai: G, then G^H
            if self.kind == "fsai_lu":
                # P = W^H G_L; the adjoint (the operator's flag, or the caller's trans, not both) is G_L^H W
                first, second = (self.vals_w, self.vals) if trans != self.adjoint else (self.vals, self.vals_w)
            K.csr_mm(self.pat, first, X[:, :, :N], out=scr, trans=False)
            K.csr_mm(self.pat, second, scr, out=out[:, :, :N], trans=True)
        elif self.kind != "dense" or self.cplx:
            if self.kind != "dense":
                self.last_kernel = self.kind                   # "csr" / "banded"
            super()._native(X, out, trans)
        elif self.symm and not self.flip and K.symm_wide_ok(self.mat, X[:, :, :N]):
            # exactly symmetric fp32 storage, 9 .. 16 columns: the triangle once, both products on the matrix cores
            self.last_kernel = "K1sw"
            K.dense_symm_wide(self.mat, X[:, :, :N], out=out[:, :, :N])
        elif self.symm and self.symm_narrow and X.shape[1] < K.WIDE_MIN_P:
            self.last_kernel = "K1s"
            K.dense_symm(self.mat, X[:, :, :N], out=out[:, :, :N])
        else:
            t = (trans != self.flip)
            # a real symmetric matrix equals its transpose: the column-oriented K1 variant (lanes own
            # output columns, panel values are wave-uniform scalars) measured 6.8 vs 6.3 TB/s at p = 6
            # (only for matrices whose symmetry was verified by LinearOperator.m — otherwise the product stays the
            # reference's mat @ x)
            if self.hermitian and not self.flip and self.herm_verified:
                t = True
            # (many columns in the ROW orientation — A X, non-Hermitian A — go to K1wr inside dense_mm: one pass over
            # the operator per 32 columns, no transposed copy)
            Xn = X[:, :, :N]
            wide = Xn.shape[1] >= K.WIDE_MIN_P
            if t:
                mat3 = self.mat
                self.last_kernel = "K1w" if wide and K._wide_ok(mat3, mat3.shape[-1], mat3.stride(-2),
                                                                mat3.stride(0) if mat3.dim() == 3 else 0) else "K1"
            else:
                self.last_kernel = "K1wr" if wide else "K1"
            K.dense_mm(self.mat, Xn, out=out[:, :, :N], trans=t)
        return out
