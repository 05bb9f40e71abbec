"""Preconditioners for sparse operators.

`fsai(A)` — the factorised sparse approximate inverse (Kolotilina & Yeremin 1993) of a Hermitian positive definite
`SparseLinearOperator`: a sparse lower-triangular G with G A G^H ~ I, built row by row from small dense solves with no
dependency between rows (xk_fsai_build_* on a HIP device, host_precond.fsai_values in host memory), and applied as two
CSR products P x = G^H (G x).  P is Hermitian positive definite for any non-singular G, so it is a legal
preconditioner for `cg` and for `minres` (also on an indefinite A).  DESIGN.md §3.11.

`fsai_lu(A)` — its unsymmetric form for a general square `SparseLinearOperator`: two sparse triangular factors on one
lower-triangular pattern with G_L A G_U ~ I, each row from one small pivoted LU of the full block A[S_i, S_i]
(xk_fsai_lu_build_* on a HIP device, host_precond.fsai_lu_values in host memory), applied as P x = G_U (G_L x), again two
CSR products.  For `gmres(precond_r=)` and `bicgstab(precond_l= / precond_r=)`.  DESIGN.md §3.18.
"""
import warnings
import torch
from xitorch_amd.linop import LinearOperator, SparseLinearOperator, AdjointLinearOperator, _native_dtype
from xitorch_amd._util import MathWarning
from xitorch_amd import kernels as K
from xitorch_amd.linalg import host_precond

__all__ = ["fsai", "FSAIOperator", "fsai_lu", "FSAILUOperator", "named_preconditioner"]

MAX_ROW = 32          # xk_fsai_max_row(): the longest row of G the kernel factors inside one wavefront
MAX_POWER = 4


class FSAIOperator(LinearOperator):
    """P = G^H G with G a lower-triangular `SparseLinearOperator` (`.G`: columns sorted and unique, the diagonal last
    in every row, real and positive).  `.nfallback` (*batch,) counts the rows of G that are Jacobi rows because their
    block of A was not numerically positive definite.  Carries no parameters: no gradient flows through a
    preconditioner."""

    def __init__(self, G, nfallback):
        super().__init__(shape=G.shape, is_hermitian=True, dtype=G.dtype, device=G.device,
                         _suppress_hermit_warning=True)
        self.G = G
        self.nfallback = nfallback

    def _mv(self, x):
        return self._mm(x.unsqueeze(-1)).squeeze(-1)

    def _mm(self, x):
        return self.G.rmm(self.G.mm(x))

    def _rmv(self, x):
        return self._mv(x)

    def _rmm(self, x):
        return self._mm(x)

    def _getparamnames(self, prefix=""):
        return []


def fsai(A, power=1, max_row=MAX_ROW):
    r"""
    Factorised sparse approximate inverse preconditioner :math:`\mathbf{P=G^HG}`, :math:`\mathbf{GAG^H\approx I}`, of a
    Hermitian positive definite sparse operator.

    Arguments
    ---------
    A: SparseLinearOperator ``(*B, N, N)``
        Taken as Hermitian: only its stored lower triangle (``col <= row``) is read; duplicates add up, columns may be
        unsorted, the imaginary part of a diagonal entry is ignored.  ``A.values`` is read detached.
    power: int, 1..4
        Row ``i`` of ``G`` takes the lower-triangle columns of row ``i`` of :math:`|\mathbf{A}|^{power}` (and ``i``).
    max_row: int, 1..32
        A longer row keeps its ``max_row`` columns nearest the diagonal.

    Returns
    -------
    FSAIOperator
        Hermitian, of A's shape, dtype and device.  A row whose block of ``A`` is not numerically positive definite
        becomes the Jacobi row :math:`1/\sqrt{|a_{ii}|}` (1 for a zero or non-finite diagonal); if there is any, one
        ``MathWarning`` names their number.
    """
    if not isinstance(A, SparseLinearOperator):
        raise TypeError("fsai: A must be a SparseLinearOperator, got %s" % type(A).__name__)
    N = A.shape[-1]
    if A.shape[-2] != N:
        raise TypeError("fsai: A must be square, got shape %s" % (tuple(A.shape),))
    if not isinstance(power, int) or not 1 <= power <= MAX_POWER:
        raise ValueError("fsai: power must be an integer in 1..%d, got %r" % (MAX_POWER, power))
    if not isinstance(max_row, int) or not 1 <= max_row <= MAX_ROW:
        raise ValueError("fsai: max_row must be an integer in 1..%d, got %r" % (MAX_ROW, max_row))
    pat = A._pattern
    vals = A.values.detach().resolve_conj()
    vshape = tuple(vals.shape[:-1])
    vals = vals.reshape(-1, A.nnz).contiguous()
    g_ptr, g_idx = host_precond.fsai_pattern(pat.row_of, A.col, N, power, max_row)
    if N == 0:
        g_val = vals.new_zeros((vals.shape[0], 0))
        nfail = torch.zeros((vals.shape[0],), dtype=torch.int64, device=vals.device)
    elif _native_dtype(vals):
        g_val, nfail = K.fsai_build(A.crow, A.col, vals, g_ptr, g_idx, N)
    else:
        g_val, nfail = host_precond.fsai_values(pat.row_of, A.col, vals, g_ptr, g_idx, N)
    nbad = int(nfail.sum())
    if nbad:
        warnings.warn(MathWarning("fsai: %d row(s) of G fell back to the Jacobi row: their block of A is not "
                                  "numerically positive definite" % nbad))
    G = SparseLinearOperator(g_ptr, g_idx, g_val.reshape(*vshape, g_idx.numel()), tuple(A.shape))
    return FSAIOperator(G, nfail.to(torch.int64).reshape(vshape).expand(A.shape[:-2]))


class FSAILUOperator(LinearOperator):
    """P = G_U G_L = W^H G_L with `.GL` and `.W` two lower-triangular `SparseLinearOperator`s on one pattern (columns
    sorted and unique, the diagonal last in every row; `.GL` has a unit diagonal, `.W` holds G_U^H).  Not Hermitian:
    `.H` is a twin on the same factors with the `adjoint` flag flipped, P^H = G_L^H W, so the adjoint runs on the same
    two CSR products.  `.nfallback` (*batch,) counts the rows that fell back to the scaled unit row.  Carries no
    parameters: no gradient flows through a preconditioner."""

    def __init__(self, GL, W, nfallback, adjoint=False):
        super().__init__(shape=GL.shape, is_hermitian=False, dtype=GL.dtype, device=GL.device)
        self.GL, self.W = GL, W
        self.nfallback = nfallback
        self.adjoint = bool(adjoint)

    def _apply(self, x, adjoint):
        if adjoint:
            return self.GL.rmm(self.W.mm(x))
        return self.W.rmm(self.GL.mm(x))

    def _mv(self, x):
        return self._mm(x.unsqueeze(-1)).squeeze(-1)

    def _mm(self, x):
        return self._apply(x, self.adjoint)

    def _rmv(self, x):
        return self._rmm(x.unsqueeze(-1)).squeeze(-1)

    def _rmm(self, x):
        return self._apply(x, not self.adjoint)

    @property
    def H(self):
        return FSAILUOperator(self.GL, self.W, self.nfallback, adjoint=not self.adjoint)

    def _getparamnames(self, prefix=""):
        return []


def fsai_lu(A, power=1, max_row=MAX_ROW):
    r"""
    Unsymmetric factorised sparse approximate inverse preconditioner :math:`\mathbf{P=G_UG_L}`,
    :math:`\mathbf{G_LAG_U\approx I}`, of a general square sparse operator.

    Arguments
    ---------
    A: SparseLinearOperator ``(*B, N, N)``
        Every stored entry is read, both triangles; duplicates add up, columns may be unsorted.  ``A.values`` is read
        detached.
    power: int, 1..4
        Row ``i`` of both factors takes the columns ``j <= i`` of row ``i`` of :math:`|\bar{\mathbf{A}}|^{power}` (and
        ``i``), :math:`\bar{\mathbf{A}}` being the stored structure of ``A`` mirrored.
    max_row: int, 1..32
        A longer row keeps its ``max_row`` columns nearest the diagonal.

    Returns
    -------
    FSAILUOperator
        Of A's shape, dtype and device, not Hermitian; ``.H`` is its adjoint on the same factors.  A row whose block of
        ``A`` has a zero or non-finite pivot (or a non-finite solution) becomes the unit row scaled by
        :math:`1/a_{ii}` (1 for a zero or non-finite diagonal); if there is any, one ``MathWarning`` names their number.
    """
    if not isinstance(A, SparseLinearOperator):
        raise TypeError("fsai_lu: A must be a SparseLinearOperator, got %s" % type(A).__name__)
    N = A.shape[-1]
    if A.shape[-2] != N:
        raise TypeError("fsai_lu: A must be square, got shape %s" % (tuple(A.shape),))
    if not isinstance(power, int) or not 1 <= power <= MAX_POWER:
        raise ValueError("fsai_lu: power must be an integer in 1..%d, got %r" % (MAX_POWER, power))
    if not isinstance(max_row, int) or not 1 <= max_row <= MAX_ROW:
        raise ValueError("fsai_lu: max_row must be an integer in 1..%d, got %r" % (MAX_ROW, max_row))
    pat = A._pattern
    vals = A.values.detach().resolve_conj()
    vshape = tuple(vals.shape[:-1])
    vals = vals.reshape(-1, A.nnz).contiguous()
    g_ptr, g_idx = host_precond.fsai_pattern(pat.row_of, A.col, N, power, max_row, full=True)
    if N == 0:
        gl = vals.new_zeros((vals.shape[0], 0))
        w = vals.new_zeros((vals.shape[0], 0))
        nfail = torch.zeros((vals.shape[0],), dtype=torch.int64, device=vals.device)
    elif _native_dtype(vals):
        gl, w, nfail = K.fsai_lu_build(A.crow, A.col, vals, g_ptr, g_idx, N)
    else:
        gl, w, nfail = host_precond.fsai_lu_values(pat.row_of, A.col, vals, g_ptr, g_idx, N)
    nbad = int(nfail.sum())
    if nbad:
        warnings.warn(MathWarning("fsai_lu: %d row(s) fell back to the scaled unit row: their block of A has a zero or "
                                  "non-finite pivot" % nbad))
    GL = SparseLinearOperator(g_ptr, g_idx, gl.reshape(*vshape, g_idx.numel()), tuple(A.shape))
    W = SparseLinearOperator(g_ptr, g_idx, w.reshape(*vshape, g_idx.numel()), tuple(A.shape))
    return FSAILUOperator(GL, W, nfail.to(torch.int64).reshape(vshape).expand(A.shape[:-2]))


def named_preconditioner(name, A, method):
    """The operator behind `solve(..., precond=<str>)`: "fsai" builds `fsai(A)` with its defaults (cg, minres),
    "fsai_lu" builds `fsai_lu(A)` (gmres, bicgstab).  The backward solve arrives with `A.H`: for the adjoint of a
    `SparseLinearOperator` the answer is `fsai_lu(A.obj).H`."""
    if name == "fsai_lu" and method in ("gmres", "bicgstab"):
        if isinstance(A, SparseLinearOperator):
            return fsai_lu(A)
        if isinstance(A, AdjointLinearOperator) and isinstance(A.obj, SparseLinearOperator):
            return fsai_lu(A.obj).H
        raise TypeError("solve(method=%r): the preconditioner \"fsai_lu\" needs a SparseLinearOperator A (or the adjoint "
                        "of one), got %s; build an operator yourself and pass it instead" % (method, type(A).__name__))
    if name != "fsai" or method not in ("cg", "minres"):
        names = "\"fsai_lu\"" if method in ("gmres", "bicgstab") else "\"fsai\""
        raise TypeError("solve(method=%r): unknown preconditioner name %r (the only named preconditioner is %s; "
                        "otherwise pass a LinearOperator)" % (method, name, names))
    if not isinstance(A, SparseLinearOperator):
        raise TypeError("solve(method=%r): precond=\"fsai\" needs a SparseLinearOperator A, got %s; build an operator "
                        "yourself and pass it as precond=" % (method, type(A).__name__))
    return fsai(A)
