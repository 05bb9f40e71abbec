"""LinearOperator — the batched implicit-operator contract, with MI355X-native dense and
banded operators underneath.

Drop-in for the reference's operator contract (xitorch/_core/linop.py:15-812): subclass,
call ``super().__init__(shape, is_hermitian, dtype, device)``, implement ``_mv`` (mandatory) and
optionally ``_mm/_rmv/_rmm/_fullmatrix/_getparamnames``; ``mv/mm/rmv/rmm/fullmatrix/H/matmul/
+ - *`` and ``check()`` behave as in the reference, including the error messages.

What is different underneath: ``MatrixLinearOperator`` (what ``LinearOperator.m(mat)`` returns)
and ``BandedLinearOperator`` apply themselves through the hand-written HIP kernels of
libxitorch_amd.so whenever their tensors live on a HIP device (K1, xk_dense_mm / xk_banded_mm),
wrapped in ``torch.autograd.Function`` so they stay differentiable to any order.  On a HIP
device there is no fallback: a missing library raises.  Host (CPU) tensors are served by plain
torch so that the operator algebra and the dense/exact methods remain usable for host-side
checks; the native iterative methods refuse CPU operators.
"""
import traceback
import warnings
from abc import abstractmethod
from contextlib import contextmanager
import torch
from xitorch_amd.editable import EditableModule
from xitorch_amd.debug import is_debug_enabled
from xitorch_amd._util import bcast_shape
from xitorch_amd import kernels as _k

__all__ = ["LinearOperator", "MatrixLinearOperator", "BandedLinearOperator", "SparseLinearOperator",
           "RowShardedMatrixLinearOperator"]


class LinearOperator(EditableModule):
    """Base class of operators of shape ``(*B, p, q)`` defined by their action.

    See the module docstring; reference: xitorch/_core/linop.py:15-552.
    """
    _is_mv_implemented = False
    _is_mm_implemented = False
    _is_rmv_implemented = False
    _is_rmm_implemented = False
    _is_fullmatrix_implemented = False
    _is_gpn_implemented = False

    def __new__(cls, *args, **kwargs):
        # detect once per concrete class which optional methods are overridden
        if "_impl_checked_" not in cls.__dict__:
            def overridden(name):
                return getattr(cls, name) is not getattr(LinearOperator, name)
            cls._is_mv_implemented = overridden("_mv")
            cls._is_mm_implemented = overridden("_mm")
            cls._is_rmv_implemented = overridden("_rmv")
            cls._is_rmm_implemented = overridden("_rmm")
            cls._is_fullmatrix_implemented = overridden("_fullmatrix")
            cls._is_gpn_implemented = overridden("_getparamnames")
            cls._impl_checked_ = True
            if not cls._is_mv_implemented:
                raise RuntimeError("LinearOperator must have at least _mv(self) method implemented")
        return super(LinearOperator, cls).__new__(cls)

    @classmethod
    def m(cls, mat, is_hermitian=None):
        """Wrap a (batched) matrix; ``is_hermitian=None`` checks the symmetry, ``True`` asserts it
        (reference: linop.py:59-107)."""
        exact = False
        if is_hermitian is None:
            is_hermitian, exact = _is_hermitian_matrix(mat)
        elif is_hermitian:
            ok, exact = _is_hermitian_matrix(mat)
            if not ok:
                raise RuntimeError("The linear operator is indicated to be hermitian, but the matrix is not")
        # the symmetry scan above also tells whether the storage is EXACTLY symmetric; only then may the
        # native apply read the upper triangle alone (K1s) without changing the reference's semantics
        op = MatrixLinearOperator(mat, is_hermitian, symmetric_storage=bool(is_hermitian and exact))
        if is_hermitian:
            op._herm_token = _storage_token(mat)        # symmetry of THIS tensor was checked (allclose) just now
        return op

    def __init__(self, shape, is_hermitian=False, dtype=None, device=None, _suppress_hermit_warning=False):
        super(LinearOperator, self).__init__()
        if len(shape) < 2:
            raise RuntimeError("The shape must have at least 2 dimensions")
        self._shape = shape
        self._batchshape = list(shape[:-2])
        self._is_hermitian = is_hermitian
        self._dtype = dtype if dtype is not None else torch.float32
        self._device = device if device is not None else torch.device("cpu")
        if is_hermitian and shape[-1] != shape[-2]:
            raise RuntimeError("The object is indicated as Hermitian, but the shape is not square")
        if not _suppress_hermit_warning and is_hermitian and \
                (self._is_rmv_implemented or self._is_rmm_implemented):
            warnings.warn("The LinearOperator is Hermitian with implemented rmv or rmm. We will use the "
                          "mv and mm methods instead", stacklevel=2)

    def __repr__(self):
        return "LinearOperator (%s) with shape %s, dtype = %s, device = %s" % \
            (self.__class__.__name__, _shape2str(self.shape), self.dtype, self.device)

    # ------------------------------------------------------------ to be implemented by subclasses
    @abstractmethod
    def _getparamnames(self, prefix=""):
        return []

    @abstractmethod
    def _mv(self, x):
        pass

    def _rmv(self, x):
        raise NotImplementedError()

    def _mm(self, x):
        raise NotImplementedError()

    def _rmm(self, x):
        raise NotImplementedError()

    def _fullmatrix(self):
        raise NotImplementedError()

    # ------------------------------------------------------------ parameters
    def getlinopparams(self):
        return self.getuniqueparams("mm")

    @contextmanager
    def uselinopparams(self, *params):
        # NOTE: swaps the attributes of this object in place (not re-entrant), exactly like the
        # reference (linop.py:204-212); native operators therefore read their tensors at call time.
        saved = self.getuniqueparams("mm")
        try:
            self.setuniqueparams("mm", *params)
            yield self
        finally:
            self.setuniqueparams("mm", *saved)

    def getparamnames(self, methodname, prefix=""):
        if methodname in ("mv", "rmv", "mm", "rmm", "fullmatrix"):
            return self._getparamnames(prefix=prefix)
        raise KeyError("getparamnames for method %s is not implemented" % methodname)

    # ------------------------------------------------------------ the operator actions
    def _need_init(self):
        if "_shape" not in self.__dict__:
            raise RuntimeError("super().__init__ must be executed first")

    def mv(self, x):
        """``A x`` for ``x`` of shape ``(..., q)`` (batch dims broadcastable)."""
        self._need_init()
        if x.shape[-1] != self.shape[-1]:
            raise RuntimeError("Cannot operate .mv on shape %s. Expected (...,%d)" %
                               (str(tuple(x.shape)), self.shape[-1]))
        return self._mv(x)

    def mm(self, x):
        """``A X`` for ``X`` of shape ``(..., q, r)``."""
        self._need_init()
        if x.shape[-2] != self.shape[-1]:
            raise RuntimeError("Cannot operate .mm on shape %s. Expected (...,%d,*)" %
                               (str(tuple(x.shape)), self.shape[-1]))
        if self._is_mm_implemented:
            return self._mm(x)
        return self._columns_through(self._mv, x)

    def rmv(self, x):
        """``A^H x`` for ``x`` of shape ``(..., p)``."""
        self._need_init()
        if x.shape[-1] != self.shape[-2]:
            raise RuntimeError("Cannot operate .rmv on shape %s. Expected (...,%d)" %
                               (str(tuple(x.shape)), self.shape[-2]))
        if self._is_hermitian:
            return self._mv(x)
        if not self._is_rmv_implemented:
            return self._rmv_by_autograd(x)
        return self._rmv(x)

    def rmm(self, x):
        """``A^H X`` for ``X`` of shape ``(..., p, r)``."""
        self._need_init()
        if x.shape[-2] != self.shape[-2]:
            raise RuntimeError("Cannot operate .rmm on shape %s. Expected (...,%d,*)" %
                               (str(tuple(x.shape)), self.shape[-2]))
        if self._is_hermitian:
            return self.mm(x)
        if self._is_rmm_implemented:
            return self._rmm(x)
        return self._columns_through(self._rmv if self._is_rmv_implemented else self.rmv, x)

    def _columns_through(self, vecfn, x):
        # matrix product through the batched vector product: the column axis goes to the front
        # as an extra batch dim (so `_mv` may see extra leading dims and strided input, Q13)
        xb = list(x.shape[:-2])
        if len(xb) < len(self._batchshape):
            xb = [1] * (len(self._batchshape) - len(xb)) + xb
        cols_first = x.reshape(1, *xb, *x.shape[-2:]).transpose(0, -1).squeeze(-1)   # (r, ..., q)
        y = vecfn(cols_first)                                                        # (r, ..., p)
        return y.unsqueeze(-1).transpose(0, -1).squeeze(0)

    def _rmv_by_autograd(self, xt):
        # A^H x as the vector-Jacobian product of x -> A x  (reference: linop.py:524-543)
        bshape = bcast_shape(xt.shape[:-1], self.shape[:-2])
        p, q = self.shape[-2:]
        probe = torch.zeros((*bshape, q), dtype=xt.dtype, device=xt.device).requires_grad_()
        with torch.enable_grad():
            y = self.mv(probe)
        return torch.autograd.grad(y, probe, grad_outputs=xt.contiguous().expand_as(y),
                                   create_graph=torch.is_grad_enabled())[0]

    def fullmatrix(self):
        if self._is_fullmatrix_implemented:
            return self._fullmatrix()
        self._need_init()
        eye = torch.eye(self._shape[-1], dtype=self._dtype, device=self._device)
        return self.mm(eye)

    def scipy_linalg_op(self):
        from scipy.sparse.linalg import LinearOperator as _SpOp
        tt = lambda v: torch.tensor(v, dtype=self.dtype, device=self.device)
        npy = lambda t: t.detach().cpu().numpy()
        return _SpOp(shape=self.shape,
                     matvec=lambda v: npy(self.mv(tt(v))), rmatvec=lambda v: npy(self.rmv(tt(v))),
                     matmat=lambda v: npy(self.mm(tt(v))), rmatmat=lambda v: npy(self.rmm(tt(v))))

    # ------------------------------------------------------------ algebra
    @property
    def H(self):
        """The adjoint operator."""
        if self._is_hermitian:
            return self
        if isinstance(self, MatrixLinearOperator):
            return LinearOperator.m(self.fullmatrix().transpose(-2, -1).conj())
        return AdjointLinearOperator(self)

    def matmul(self, b, is_hermitian=False):
        """The operator ``self @ b``."""
        if self.shape[-1] != b.shape[-2]:
            raise RuntimeError("Mismatch shape of matmul operation: %s and %s" % (self.shape, b.shape))
        if isinstance(self, MatrixLinearOperator) and isinstance(b, MatrixLinearOperator):
            return LinearOperator.m(self.fullmatrix() @ b.fullmatrix(), is_hermitian=is_hermitian)
        return MatmulLinearOperator(self, b, is_hermitian=is_hermitian)

    def __add__(self, b):
        assert isinstance(b, LinearOperator), "Only addition with another LinearOperator is supported"
        if self.shape[-2:] != b.shape[-2:]:
            raise RuntimeError("Mismatch shape of add operation: %s and %s" % (self.shape, b.shape))
        if isinstance(self, MatrixLinearOperator) and isinstance(b, MatrixLinearOperator):
            return LinearOperator.m(self.fullmatrix() + b.fullmatrix())
        return AddLinearOperator(self, b)

    def __sub__(self, b):
        assert isinstance(b, LinearOperator), "Only subtraction with another LinearOperator is supported"
        if self.shape[-2:] != b.shape[-2:]:
            raise RuntimeError("Mismatch shape of add operation: %s and %s" % (self.shape, b.shape))
        if isinstance(self, MatrixLinearOperator) and isinstance(b, MatrixLinearOperator):
            return LinearOperator.m(self.fullmatrix() - b.fullmatrix())
        return AddLinearOperator(self, b, -1)

    def __rsub__(self, b):
        return b.__sub__(self)

    def __mul__(self, f):
        if not isinstance(f, (int, float)):
            raise TypeError("LinearOperator multiplication only supports integer or floating point")
        if isinstance(self, MatrixLinearOperator):
            return LinearOperator.m(self.fullmatrix() * f)
        return MulLinearOperator(self, f)

    def __rmul__(self, f):
        return self.__mul__(f)

    # ------------------------------------------------------------ properties
    dtype = property(lambda self: self._dtype)
    device = property(lambda self: self._device)
    shape = property(lambda self: self._shape)
    is_hermitian = property(lambda self: self._is_hermitian)
    is_mv_implemented = property(lambda self: True)
    is_mm_implemented = property(lambda self: self._is_mm_implemented)
    is_rmv_implemented = property(lambda self: self._is_rmv_implemented)
    is_rmm_implemented = property(lambda self: self._is_rmm_implemented)
    is_fullmatrix_implemented = property(lambda self: self._is_fullmatrix_implemented)
    is_getparamnames_implemented = property(lambda self: self._is_gpn_implemented)

    # ------------------------------------------------------------ debugging
    def check(self, warn=None):
        """Exercise mv/mm/rmv/rmm on all the shapes the functionals may use and test linearity
        (reference: linop.py:492-521, 710-802)."""
        if warn is None:
            warn = not is_debug_enabled()
        if warn:
            warnings.warn("The linear operator check is performed. This might slow down your program.",
                          stacklevel=2)
        checklinop(self)
        print("Check linear operator done")


# ------------------------------------------------------------------------ composed operators
class AdjointLinearOperator(LinearOperator):
    def __init__(self, obj):
        super().__init__(shape=(*obj.shape[:-2], obj.shape[-1], obj.shape[-2]), is_hermitian=obj.is_hermitian,
                         dtype=obj.dtype, device=obj.device, _suppress_hermit_warning=True)
        self.obj = obj

    def __repr__(self):
        return "AdjointLinearOperator with shape %s of:\n - %s" % (_shape2str(self.shape), _indent(repr(self.obj), 3))

    def _mv(self, x):
        if not self.obj.is_rmv_implemented:
            raise RuntimeError("The ._rmv of must be implemented to call .H.mv()")
        return self.obj._rmv(x)

    def _rmv(self, x):
        return self.obj._mv(x)

    def _getparamnames(self, prefix=""):
        return self.obj._getparamnames(prefix=prefix + "obj.")

    @property
    def H(self):
        return self.obj


class MatmulLinearOperator(LinearOperator):
    def __init__(self, a, b, is_hermitian=False):
        super().__init__(shape=(*bcast_shape(a.shape[:-2], b.shape[:-2]), a.shape[-2], b.shape[-1]),
                         is_hermitian=is_hermitian, dtype=a.dtype, device=a.device, _suppress_hermit_warning=True)
        self.a, self.b = a, b

    def __repr__(self):
        return "MatmulLinearOperator with shape %s of:\n * %s\n * %s" % \
            (_shape2str(self.shape), _indent(repr(self.a), 3), _indent(repr(self.b), 3))

    def _mv(self, x):
        return self.a._mv(self.b._mv(x))

    def _rmv(self, x):
        return self.b.rmv(self.a.rmv(x))

    def _getparamnames(self, prefix=""):
        return self.a._getparamnames(prefix=prefix + "a.") + self.b._getparamnames(prefix=prefix + "b.")


class AddLinearOperator(LinearOperator):
    def __init__(self, a, b, mul=1):
        super().__init__(shape=(*bcast_shape(a.shape[:-2], b.shape[:-2]), a.shape[-2], b.shape[-1]),
                         is_hermitian=a.is_hermitian and b.is_hermitian, dtype=a.dtype, device=a.device,
                         _suppress_hermit_warning=True)
        assert mul == 1 or mul == -1
        self.a, self.b, self.mul = a, b, mul

    def __repr__(self):
        return "AddLinearOperator with shape %s of:\n * %s\n * %s" % \
            (_shape2str(self.shape), _indent(repr(self.a), 3), _indent(repr(self.b), 3))

    def _mv(self, x):
        return self.a._mv(x) + self.mul * self.b._mv(x)

    def _rmv(self, x):
        return self.a.rmv(x) + self.mul * self.b.rmv(x)

    def _getparamnames(self, prefix=""):
        return self.a._getparamnames(prefix=prefix + "a.") + self.b._getparamnames(prefix=prefix + "b.")


class MulLinearOperator(LinearOperator):
    def __init__(self, a, f):
        super().__init__(shape=a.shape, is_hermitian=a.is_hermitian, dtype=a.dtype, device=a.device,
                         _suppress_hermit_warning=True)
        self.a, self.f = a, f

    def __repr__(self):
        return "MulLinearOperator with shape %s of: \n * %s\n * %s" % \
            (_shape2str(self.shape), _indent(repr(self.a), 3), _indent(repr(self.f), 3))

    def _mv(self, x):
        return self.a._mv(x) * self.f

    def _rmv(self, x):
        return self.a._rmv(x) * self.f

    def _getparamnames(self, prefix=""):
        return self.a._getparamnames(prefix=prefix + "a.")


# ------------------------------------------------------------------------ native dense operator
_NATIVE_DTYPES = (torch.float64, torch.float32, torch.complex128, torch.complex64)


def _native_dtype(t):
    return t.is_cuda and t.dtype in _NATIVE_DTYPES


def _native_real_dtype(t):
    return t.is_cuda and t.dtype in (torch.float64, torch.float32)


def _grad_wanted(t):
    """Inside a custom backward: will the running autograd call actually consume a gradient for `t`?

    `ctx.needs_input_grad` is fixed at forward time.  During the implicit backward solves the Jacobian operator
    is applied many times with `autograd.grad(..., inputs=(y,))` only, and materialising the B*N^2 outer
    product for the operator matrix on every one of those applies would dominate the solve.  The engine knows
    which nodes it will execute; anything uncertain counts as wanted."""
    try:
        node = torch.autograd.graph.get_gradient_edge(t).node
        return bool(torch._C._will_engine_execute_node(node))
    except Exception:
        return True


def _sum_to_shape(t, shape):
    """Reduce a broadcast gradient back to ``shape``."""
    shape = tuple(shape)
    if tuple(t.shape) == shape:
        return t
    lead = t.dim() - len(shape)
    if lead > 0:
        t = t.sum(dim=tuple(range(lead)))
    dims = tuple(i for i, (a, b) in enumerate(zip(t.shape, shape)) if a != b)
    if dims:
        t = t.sum(dim=dims, keepdim=True)
    return t


def dense_apply(mat, x, trans=False):
    """``mat @ x`` (or ``mat^H @ x``) through the K1 HIP kernel for HIP float / complex tensors.

    mat ``(*BA, M, N)``, x ``(*BX, n_in, r)`` with broadcastable batch dims.  Batch dims along
    which only ``x`` varies are folded into the panel width so the operator is streamed once.
    Never copies ``mat`` when it is contiguous or a transposed / conjugated view of a contiguous matrix:
    views flip the kernel's orientation flags instead.
    """
    cplx = mat.is_complex()
    conj_io = False
    if cplx:
        cj = mat.is_conj()
        if cj:
            mat = mat.conj()                              # drops the lazy-conjugation bit: the stored numbers
        flip = mat.dim() >= 2 and mat.stride(-1) != 1 and mat.stride(-2) == 1
        if flip:
            mat = mat.transpose(-2, -1)
        trans = (trans != flip)                            # adjoint of the STORED matrix wanted?
        conj_io = (flip != cj)                             # A^T x = conj(A^H conj x), conj(A) x = conj(A conj x)
        x = x.resolve_conj()
    elif mat.stride(-1) != 1 and mat.stride(-2) == 1 and mat.dim() >= 2:
        mat, trans = mat.transpose(-2, -1), not trans      # a transposed view: flip the kernel
    M, N = mat.shape[-2:]
    n_in, n_out = (M, N) if trans else (N, M)
    r = x.shape[-1]
    nb, FB, keep, fold = _batch_plan(list(mat.shape[:-2]), list(x.shape[:-2]))
    xp = _to_panel(x, nb, FB, keep, fold)                                    # panel-major (copy only if needed)
    matf = mat.reshape(-1, M, N) if mat.is_contiguous() else mat.contiguous().reshape(-1, M, N)
    if cplx:
        y = _k.dense_mm_complex(matf, xp, adjoint=trans, conj_io=conj_io)    # (nkeep, P, n_out)
    else:
        y = _k.dense_mm(matf, xp, trans=trans)
    y = y.reshape(*[FB[d] for d in keep], *[FB[d] for d in fold], r, n_out)
    inv = [0] * (nb + 2)
    for pos, d in enumerate(keep + fold + [nb + 1, nb]):
        inv[d] = pos
    return y.permute(*inv)


class _DenseMM(torch.autograd.Function):
    """Differentiable wrapper of the native dense apply (any order: backward re-enters itself)."""

    @staticmethod
    def forward(ctx, mat, x, trans):
        ctx.save_for_backward(mat, x)
        ctx.trans = trans
        return dense_apply(mat, x, trans)

    @staticmethod
    def backward(ctx, gy):
        mat, x = ctx.saved_tensors
        gmat = gx = None
        if ctx.needs_input_grad[1] and _grad_wanted(x):
            gx = _sum_to_shape(_DenseMM.apply(mat, gy, not ctx.trans), x.shape)
        if ctx.needs_input_grad[0] and _grad_wanted(mat):
            # the B*N^2 outer product is only materialised when this backward call really asks for it
            gmat = _DenseOuter.apply(x, gy, tuple(mat.shape)) if ctx.trans else \
                _DenseOuter.apply(gy, x, tuple(mat.shape))
        return gmat, gx, None


def _batch_plan(op_batch, *operand_batches):
    """Batch bookkeeping shared by the native applies and their gradients: pads the batch shapes to a common
    rank, returns (full batch FB, dims the operator varies along `keep`, dims only the operands vary along `fold`)."""
    nb = max([len(op_batch)] + [len(b) for b in operand_batches])
    BAp = [1] * (nb - len(op_batch)) + list(op_batch)
    padded = [[1] * (nb - len(b)) + list(b) for b in operand_batches]
    FB = bcast_shape(BAp, *padded)
    keep = [d for d in range(nb) if BAp[d] == FB[d]]
    fold = [d for d in range(nb) if BAp[d] != FB[d]]
    return nb, FB, keep, fold


def _to_panel(t, nb, FB, keep, fold):
    """(*batch, n, r) -> panel-major (prod(keep dims), prod(fold dims) * r, n), contiguous vectors."""
    n, r = t.shape[-2:]
    tb = [1] * (nb - (t.dim() - 2)) + list(t.shape[:-2])
    te = t.reshape(*tb, n, r).expand(*FB, n, r)
    nkeep = 1
    for d in keep:
        nkeep *= FB[d]
    tp = te.permute(*keep, *fold, nb + 1, nb).reshape(nkeep, -1, n)
    if tp.stride(-1) != 1 or (tp.shape[1] > 1 and tp.stride(1) < n):
        tp = tp.contiguous()
    return tp


class _DenseOuter(torch.autograd.Function):
    """G[..., i, j] = sum_c u[..., i, c] w[..., j, c] reduced to the operator's shape: the gradient of the dense
    apply w.r.t. the matrix, written by the streaming HIP kernel xk_dense_outer (in the reference: the matmul
    backward under `torch.autograd.grad(loss, params, ...)`, linalg/solve.py:188-195).  Bilinear, so its own
    backward is two dense applies and any order of differentiation works."""

    @staticmethod
    def forward(ctx, u, w, mat_shape):
        ctx.save_for_backward(u, w)
        ctx.mat_shape = mat_shape
        M, N = mat_shape[-2:]
        nb, FB, keep, fold = _batch_plan(mat_shape[:-2], u.shape[:-2], w.shape[:-2])
        up, wp = _to_panel(u, nb, FB, keep, fold), _to_panel(w, nb, FB, keep, fold)
        if u.is_complex():
            g = _k.dense_outer_complex(up.resolve_conj(), wp.resolve_conj())    # sum_c u conj(w): gy x^H
        else:
            g = _k.dense_outer(up, wp)                                  # (nkeep, M, N): folded dims summed
        return g.reshape(*[FB[d] for d in keep], M, N).reshape(mat_shape)

    @staticmethod
    def backward(ctx, gg):
        u, w = ctx.saved_tensors
        gu = gw = None
        if ctx.needs_input_grad[0]:
            gu = _sum_to_shape(_DenseMM.apply(gg, w, False), u.shape)
        if ctx.needs_input_grad[1]:
            gw = _sum_to_shape(_DenseMM.apply(gg, u, True), w.shape)
        return gu, gw, None


def _dense_mm(mat, x, trans):
    if _native_dtype(mat) and x.dtype == mat.dtype:
        if not x.is_cuda:
            raise RuntimeError("operator lives on %s but the operand on %s" % (mat.device, x.device))
        return _DenseMM.apply(mat, x, trans)
    # host tensors / mixed dtypes: plain torch (not the accelerated path)
    op = mat.transpose(-2, -1).conj() if trans else mat
    return torch.matmul(op, x)


class MatrixLinearOperator(LinearOperator):
    """Dense operator.  HIP float32/float64 matrices are applied by the K1 kernel, complex64/complex128 ones by
    the same kernel on their interleaved (real-embedded) storage (replaces linop.py:676-708 of the reference)."""

    def __init__(self, mat, is_hermitian, symmetric_storage=False):
        super().__init__(shape=mat.shape, is_hermitian=is_hermitian, dtype=mat.dtype, device=mat.device,
                         _suppress_hermit_warning=True)
        self.mat = mat
        # True = the caller (or LinearOperator.m's scan) guarantees mat == mat^T bit for bit; the native
        # eigensolver / Krylov loops then stream only the upper triangle (xk_dense_symm).  The promise is about
        # ONE tensor: it is remembered together with that tensor's identity and dropped when `mat` is swapped
        # (uselinopparams / setuniqueparams put graph-connected clones or user tensors there).
        self._symm_promise = bool(symmetric_storage) and bool(is_hermitian) and not torch.is_complex(mat)
        self._symm_token = _storage_token(mat) if self._symm_promise else None

    @property
    def symmetric_storage(self):
        """Exactly-symmetric-storage promise, valid only for the tensor it was made about: a different `mat`
        (other storage, other version counter) falls back to the full-matrix kernels = the reference's
        `mat @ x` semantics."""
        return bool(self._symm_promise and self._symm_token == _storage_token(self.mat))

    @property
    def hermitian_verified(self):
        """True when the symmetry of the current `mat` was actually checked (LinearOperator.m) — only then may a
        native apply substitute mat^T x for mat x; a bare `MatrixLinearOperator(mat, True)` is taken at its word
        for the algorithm choice but its products stay the reference's `mat @ x`."""
        tok = getattr(self, "_herm_token", None)
        return bool(self._is_hermitian and tok is not None and tok == _storage_token(self.mat)) or \
            self.symmetric_storage

    @symmetric_storage.setter
    def symmetric_storage(self, value):
        self._symm_promise = bool(value) and bool(self._is_hermitian) and not torch.is_complex(self.mat)
        self._symm_token = _storage_token(self.mat) if self._symm_promise else None

    def __repr__(self):
        return "MatrixLinearOperator with shape %s:\n   %s" % (_shape2str(self.shape), _indent(repr(self.mat), 3))

    def _mv(self, x):
        return _dense_mm(self.mat, x.unsqueeze(-1), False).squeeze(-1)

    def _mm(self, x):
        return _dense_mm(self.mat, x, False)

    def _rmv(self, x):
        return _dense_mm(self.mat, x.unsqueeze(-1), True).squeeze(-1)

    def _rmm(self, x):
        return _dense_mm(self.mat, x, True)

    def _fullmatrix(self):
        return self.mat

    def _getparamnames(self, prefix=""):
        return [prefix + "mat"]


# ------------------------------------------------------------------------ row-block sharded dense operator
def _all_gather_rows(y_loc, bounds, rank, group):
    """concatenation over the ranks of their row blocks (blocks of unequal height are padded for the collective)"""
    import torch.distributed as dist
    world = len(bounds) - 1
    nmax = max(bounds[r + 1] - bounds[r] for r in range(world))
    pad = torch.zeros((*y_loc.shape[:-2], nmax, y_loc.shape[-1]), dtype=y_loc.dtype, device=y_loc.device)
    pad[..., :bounds[rank + 1] - bounds[rank], :] = y_loc
    parts = [torch.empty_like(pad) for _ in range(world)]
    dist.all_gather(parts, pad.contiguous(), group=group)
    return torch.cat([parts[r][..., :bounds[r + 1] - bounds[r], :] for r in range(world)], dim=-2)


# The four autograd pieces of the row-sharded products.  Everything outside the operator is REPLICATED: every rank holds
# the same x, computes the same y and the same loss, so the gradient of a replicated tensor is the sum (or the
# concatenation) of what the ranks' local graphs produce, and each collective's backward is its dual collective.  The
# backward collectives run in the same order on every rank because the ranks differentiate the same replicated graph.
class _GatherRows(torch.autograd.Function):
    """y = all-gather of the ranks' row blocks; every rank continues with the same replicated y, so the gradient
    w.r.t. this rank's block is its own slice of grad y."""

    @staticmethod
    def forward(ctx, y_loc, bounds, rank, group):
        ctx.lo, ctx.hi = bounds[rank], bounds[rank + 1]
        return _all_gather_rows(y_loc, bounds, rank, group)

    @staticmethod
    def backward(ctx, gy):
        return gy[..., ctx.lo:ctx.hi, :], None, None, None


class _ReplicatedIn(torch.autograd.Function):
    """identity on a replicated input whose consumers are rank-local (this rank's row block times x): the gradient of
    the replicated x is the SUM over the ranks of the local contributions local_r^H gy[lo_r:hi_r]."""

    @staticmethod
    def forward(ctx, x, group):
        ctx.group = group
        return x.view_as(x)

    @staticmethod
    def backward(ctx, gx):
        import torch.distributed as dist
        gx = gx.contiguous().clone()
        dist.all_reduce(gx, op=dist.ReduceOp.SUM, group=ctx.group)
        return gx, None


class _SumOverRanks(torch.autograd.Function):
    """y = all-reduce(SUM) of the ranks' partial results; y is replicated, so every partial receives grad y as it is."""

    @staticmethod
    def forward(ctx, y_part, group):
        import torch.distributed as dist
        y = y_part.contiguous().clone()
        dist.all_reduce(y, op=dist.ReduceOp.SUM, group=group)
        return y

    @staticmethod
    def backward(ctx, gy):
        return gy, None


class _OwnRows(torch.autograd.Function):
    """this rank's row slice of a replicated x; the gradient of the replicated x is the all-gather of the slices'."""

    @staticmethod
    def forward(ctx, x, bounds, rank, group):
        ctx.bounds, ctx.rank, ctx.group = bounds, rank, group
        return x[..., bounds[rank]:bounds[rank + 1], :]

    @staticmethod
    def backward(ctx, gs):
        return _all_gather_rows(gs, ctx.bounds, ctx.rank, ctx.group), None, None, None


class RowShardedMatrixLinearOperator(LinearOperator):
    """One dense operator ``A (*B, N, N)`` split by ROW BLOCKS over the ranks of a process group — the sharding for
    fewer operators than GPUs (last bullet: the batched-operator dimension cannot spread B < G members; a
    single huge operator otherwise never leaves one GPU).  Rank r holds rows ``[lo_r, hi_r)`` of every batch member
    (``local_rows (*B, hi_r - lo_r, N)``, contiguous blocks in rank order, `dist.shard_range`); vectors are REPLICATED:

        A x      each rank streams its row block once (K1 on HIP tensors) -> its rows of the result; one all-gather of
                 the p-column panel (N p s bytes: 786 KB at N = 16384, p = 6 fp64)        (reference product: linop.py:692-702)
        A^H x    each rank contracts its rows; one all-reduce(SUM) of the (N, p) result

    Everything else of a solver — Gram / Rayleigh blocks, the small eigenproblem, the stopping rule — then runs
    replicated and identical on every rank (same start block, deterministic kernels), so no further collective and no
    ``process_group=`` option is needed: pass this operator to `symeig` / `solve` as it is.  The operator stream, which is
    the whole cost at these sizes, is divided by the number of ranks; the O(k N) chain is not (k N << N^2 / G)."""

    def __init__(self, local_rows, n, process_group=None, is_hermitian=False):
        import torch.distributed as dist
        from xitorch_amd.dist import shard_range
        self.group = process_group
        world = dist.get_world_size(process_group) if (dist.is_available() and dist.is_initialized()) else 1
        rank = dist.get_rank(process_group) if world > 1 else 0
        self.world, self.rank = world, rank
        self.bounds = [shard_range(n, world, r)[0] for r in range(world)] + [n]
        if local_rows.shape[-1] != n or local_rows.shape[-2] != self.bounds[rank + 1] - self.bounds[rank]:
            raise RuntimeError("rank %d of %d holds rows [%d, %d) of the (%d, %d) operator: local block must be "
                               "(*B, %d, %d), got %s" % (rank, world, self.bounds[rank], self.bounds[rank + 1], n, n,
                                                         self.bounds[rank + 1] - self.bounds[rank], n,
                                                         tuple(local_rows.shape)))
        super().__init__(shape=(*local_rows.shape[:-2], n, n), is_hermitian=is_hermitian, dtype=local_rows.dtype,
                         device=local_rows.device, _suppress_hermit_warning=True)
        self.local = local_rows

    @classmethod
    def from_full(cls, mat, process_group=None, is_hermitian=False):
        """the row block of this rank cut out of a replicated full matrix (tests, small problems)"""
        import torch.distributed as dist
        from xitorch_amd.dist import shard_range
        world = dist.get_world_size(process_group) if (dist.is_available() and dist.is_initialized()) else 1
        rank = dist.get_rank(process_group) if world > 1 else 0
        lo, hi = shard_range(mat.shape[-1], world, rank)
        return cls(mat[..., lo:hi, :].contiguous(), mat.shape[-1], process_group, is_hermitian)

    def _gather(self, y_loc):
        if self.world == 1:
            return y_loc
        return _GatherRows.apply(y_loc, self.bounds, self.rank, self.group)

    def _mm(self, x):
        if self.world > 1 and x.requires_grad and torch.is_grad_enabled():
            x = _ReplicatedIn.apply(x, self.group)            # grad x = sum over the ranks of local^H gy[own rows]
        return self._gather(_dense_mm(self.local, x, False))

    def _mv(self, x):
        return self._mm(x.unsqueeze(-1)).squeeze(-1)

    def _rmm(self, x):
        lo, hi = self.bounds[self.rank], self.bounds[self.rank + 1]
        if self.world == 1:
            return _dense_mm(self.local, x[..., lo:hi, :], True)
        if x.requires_grad and torch.is_grad_enabled():
            xs = _OwnRows.apply(x, self.bounds, self.rank, self.group)     # grad x = all-gather of the slices' gradients
        else:
            xs = x[..., lo:hi, :]
        return _SumOverRanks.apply(_dense_mm(self.local, xs, True), self.group)

    def _rmv(self, x):
        return self._rmm(x.unsqueeze(-1)).squeeze(-1)

    def _fullmatrix(self):
        return self._gather(self.local)

    def _getparamnames(self, prefix=""):
        return [prefix + "local"]


# ------------------------------------------------------------------------ native banded operator
def banded_apply_torch(band, x, trans=False):
    """Reference semantics of the banded apply in plain torch (host tensors)."""
    nd, n = band.shape[-2:]
    hb = nd // 2
    y = torch.zeros((*bcast_shape(band.shape[:-2], x.shape[:-2]), *x.shape[-2:]), dtype=x.dtype, device=x.device)
    for d in range(nd):
        off = d - hb
        lo, hi = max(0, -off), min(n, n - off)
        if hi <= lo:
            continue
        coef = band[..., d, lo:hi].unsqueeze(-1)
        if not trans:
            y[..., lo:hi, :] += coef * x[..., lo + off:hi + off, :]
        else:
            y[..., lo + off:hi + off, :] += coef.conj() * x[..., lo:hi, :]
    return y


class _BandedMM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, band, x, trans):
        ctx.save_for_backward(band, x)
        ctx.trans = trans
        return _banded_native(band, x, trans)

    @staticmethod
    def backward(ctx, gy):
        band, x = ctx.saved_tensors
        gband = gx = None
        if ctx.needs_input_grad[1] and _grad_wanted(x):
            gx = _sum_to_shape(_BandedMM.apply(band, gy, not ctx.trans), x.shape)
        if ctx.needs_input_grad[0] and _grad_wanted(band):
            # d/dband[d,i] = sum_c gy[i,c] x[i+off,c]  (trans: x[i,c] gy[i+off,c]) — one streaming HIP kernel
            gband = _BandGrad.apply(x, gy, tuple(band.shape)) if ctx.trans else \
                _BandGrad.apply(gy, x, tuple(band.shape))
        return gband, gx, None


class _BandGrad(torch.autograd.Function):
    """G[..., d, i] = sum_c u[..., i, c] w[..., i+d-hb, c] reduced to the band's shape (xk_banded_grad): the
    gradient of the banded apply w.r.t. the DIA storage — what `torch.autograd.grad(loss, params, v)` of
    solve_torchfcn.backward (xitorch/linalg/solve.py:188-195) asks of a banded operator.  Bilinear: its
    backward is two banded applies with G as the band."""

    @staticmethod
    def forward(ctx, u, w, band_shape):
        ctx.save_for_backward(u, w)
        nd, n = band_shape[-2:]
        nb, FB, keep, fold = _batch_plan(band_shape[:-2], u.shape[:-2], w.shape[:-2])
        up, wp = _to_panel(u, nb, FB, keep, fold), _to_panel(w, nb, FB, keep, fold)
        g = _k.banded_grad(up, wp, nd)                                  # (nkeep, nd, n): folded dims summed
        return g.reshape(*[FB[d] for d in keep], nd, n).reshape(band_shape)

    @staticmethod
    def backward(ctx, gg):
        u, w = ctx.saved_tensors
        gu = gw = None
        if ctx.needs_input_grad[0]:
            gu = _sum_to_shape(_BandedMM.apply(gg, w, False), u.shape)
        if ctx.needs_input_grad[1]:
            gw = _sum_to_shape(_BandedMM.apply(gg, u, True), w.shape)
        return gu, gw, None


def _banded_native(band, x, trans):
    nd, n = band.shape[-2:]
    r = x.shape[-1]
    BA, BX = list(band.shape[:-2]), list(x.shape[:-2])
    nb = max(len(BA), len(BX))
    BAp = [1] * (nb - len(BA)) + BA
    BXp = [1] * (nb - len(BX)) + BX
    FB = bcast_shape(BAp, BXp)
    keep = [d for d in range(nb) if BAp[d] == FB[d]]
    fold = [d for d in range(nb) if BAp[d] != FB[d]]
    nkeep = 1
    for d in keep:
        nkeep *= FB[d]
    xe = x.reshape(*BXp, n, r).expand(*FB, n, r)
    xp = xe.permute(*keep, *fold, nb + 1, nb).reshape(nkeep, -1, n).contiguous()
    bandf = band.contiguous().reshape(-1, nd, n)
    y = _k.banded_mm(bandf, xp, trans=trans)
    y = y.reshape(*[FB[d] for d in keep], *[FB[d] for d in fold], r, n)
    inv = [0] * (nb + 2)
    for pos, d in enumerate(keep + fold + [nb + 1, nb]):
        inv[d] = pos
    return y.permute(*inv)


class BandedLinearOperator(LinearOperator):
    """Square banded operator in DIA storage: ``band (*B, 2*hb+1, N)``, ``band[..., d, i] = A[i, i+d-hb]``
    (entries outside the matrix are ignored).  Not present in the reference — there a user would
    write the same thing as a custom ``_mv`` (cf. ``ALarge``, _tests/test_linop_fcns.py:129-150); it
    is the operator of BASELINE.json configs[2] and is applied by the xk_banded_mm HIP kernel."""

    def __init__(self, band, is_hermitian=False):
        nd, n = band.shape[-2:]
        if nd % 2 != 1:
            raise RuntimeError("The band must have an odd number (2*hb+1) of diagonals")
        super().__init__(shape=(*band.shape[:-2], n, n), is_hermitian=is_hermitian, dtype=band.dtype,
                         device=band.device, _suppress_hermit_warning=True)
        self.band = band

    def _apply(self, x, trans):
        if _native_real_dtype(self.band) and x.dtype == self.band.dtype:
            return _BandedMM.apply(self.band, x, trans)
        return banded_apply_torch(self.band, x, trans)

    def _mv(self, x):
        return self._apply(x.unsqueeze(-1), False).squeeze(-1)

    def _mm(self, x):
        return self._apply(x, False)

    def _rmv(self, x):
        return self._apply(x.unsqueeze(-1), True).squeeze(-1)

    def _rmm(self, x):
        return self._apply(x, True)

    def _getparamnames(self, prefix=""):
        return [prefix + "band"]


# ------------------------------------------------------------------------ native CSR sparse operator
_CSR_BIN_EDGES = (4, 32, 1024)      # row-length bin edges of xk_csr_mm (1 / 8 / 64 / 256 lanes per row), all dtypes


class _CsrView:
    """One orientation of a pattern as xk_csr_mm reads it: pointers, indices, the value permutation (None in the
    CSR orientation), the output rows grouped by length bin (bin_off: host int[5]) and the segments of the long rows
    (seg_q: long row of each segment, seg_off: first segment of each long row), plus the segment-sum scratch."""

    def __init__(self, ptr, idx, perm, n_out, n_in):
        import ctypes
        self.ptr, self.idx, self.perm, self.n_out, self.n_in = ptr, idx, perm, n_out, n_in
        lens = (ptr[1:] - ptr[:-1]).to(torch.int64)
        edges = torch.tensor(_CSR_BIN_EDGES, dtype=torch.int64, device=ptr.device)
        binid = torch.bucketize(lens, edges, right=False)             # len <= 4 -> 0, <= 32 -> 1, <= 1024 -> 2, else 3
        order = torch.sort(binid, stable=True).indices                  # rows ascending inside each bin
        self.rows = order.to(torch.int32).contiguous()
        counts = torch.bincount(binid, minlength=4).tolist()
        offs = [0]
        for c in counts:
            offs.append(offs[-1] + int(c))
        self.bin_counts = counts
        self.bin_off = (ctypes.c_int * 5)(*offs)
        self.seg_q = self.seg_off = None
        self.nseg = 0
        self._ws = None
        if counts[3]:
            seg = int(_k.fn("xk_csr_seg_len")())
            nsq = (lens[order[offs[3]:]] + seg - 1) // seg                 # segments of each long row
            so = torch.zeros(counts[3] + 1, dtype=torch.int64, device=ptr.device)
            so[1:] = torch.cumsum(nsq, 0)
            self.nseg = int(so[-1])
            self.seg_off = so.to(torch.int32)
            self.seg_q = torch.repeat_interleave(torch.arange(counts[3], dtype=torch.int32, device=ptr.device), nsq,
                                                 output_size=self.nseg)

    def scratch(self, n, dtype):
        if self._ws is None or self._ws.numel() < n or self._ws.dtype != dtype:
            self._ws = torch.empty(n, dtype=dtype, device=self.ptr.device)
        return self._ws


class _CsrPattern:
    """Sparsity structure shared by the batch: int32 CSR arrays, the row of every entry, and — built on first
    use — the row bins of the native apply and the CSC view (stable argsort of (col, row)) of the transposed one."""

    def __init__(self, crow, col, M, N):
        self.crow, self.col, self.M, self.N = crow, col, M, N
        self.nnz = col.numel()
        self.row_of = torch.repeat_interleave(torch.arange(M, dtype=torch.int32, device=crow.device),
                                              (crow[1:] - crow[:-1]).to(torch.int64), output_size=self.nnz)
        self._csr = self._csc = None
        self._ccol = self._row_idx = self._perm = None

    def csr(self):
        if self._csr is None:
            self._csr = _CsrView(self.crow, self.col, None, self.M, self.N)
        return self._csr

    def transposed(self):
        """(ccol_ptr (N+1,), row_idx (nnz,), perm (nnz,)) int32: the CSC view; perm[k] = CSR position of entry k."""
        if self._perm is None:
            key = self.col.to(torch.int64) * max(self.M, 1) + self.row_of.to(torch.int64)
            perm = torch.sort(key, stable=True).indices
            cnt = torch.bincount(self.col.to(torch.int64), minlength=self.N)
            ccol = torch.zeros(self.N + 1, dtype=torch.int64, device=self.col.device)
            ccol[1:] = torch.cumsum(cnt, 0)
            self._ccol = ccol.to(torch.int32)
            self._row_idx = self.row_of[perm].contiguous()
            self._perm = perm.to(torch.int32).contiguous()
        return self._ccol, self._row_idx, self._perm

    def csc(self):
        if self._csc is None:
            ccol, row_idx, perm = self.transposed()
            self._csc = _CsrView(ccol, row_idx, perm, self.N, self.M)
        return self._csc


def csr_apply_torch(crow, col, values, x, M, N, trans=False, row_of=None):
    """Reference semantics of the CSR apply in plain torch (host tensors, complex values): y = A x (trans: A^H x),
    A[..., i, col[k]] += values[..., k] for crow[i] <= k < crow[i+1] — duplicates add up.  x (*Bx, N, r) (trans:
    (*Bx, M, r)); values (*Bv, nnz)."""
    if row_of is None:
        row_of = torch.repeat_interleave(torch.arange(M, device=crow.device), (crow[1:] - crow[:-1]).to(torch.int64),
                                         output_size=col.numel())
    row_of, col = row_of.to(torch.int64), col.to(torch.int64)
    src, dst, nout = (row_of, col, N) if trans else (col, row_of, M)
    v = values.conj() if trans else values
    dt = torch.promote_types(values.dtype, x.dtype)
    terms = v.unsqueeze(-1).to(dt) * x.index_select(-2, src).to(dt)          # (*FB, nnz, r)
    y = torch.zeros((*terms.shape[:-2], nout, x.shape[-1]), dtype=dt, device=x.device)
    return y.index_add(-2, dst, terms)


class _CsrMM(torch.autograd.Function):
    @staticmethod
    def forward(ctx, values, x, pat, trans):
        ctx.save_for_backward(values, x)
        ctx.pat, ctx.trans = pat, trans
        return _csr_native(pat, values, x, trans)

    @staticmethod
    def backward(ctx, gy):
        values, x = ctx.saved_tensors
        pat = ctx.pat
        gval = gx = None
        if ctx.needs_input_grad[1] and _grad_wanted(x):
            gx = _sum_to_shape(_CsrMM.apply(values, gy, pat, not ctx.trans), x.shape)
        if ctx.needs_input_grad[0] and _grad_wanted(values):
            # d/dval[k] = sum_c gy[row_k, c] conj(x[col_k, c])  (adjoint: x[row_k, c] conj(gy[col_k, c])) — xk_csr_sddmm
            # (torch's convention for complex gradients; y = A^H x depends on conj(val), which swaps the operands)
            gval = _CsrGrad.apply(x, gy, pat, tuple(values.shape)) if ctx.trans else \
                _CsrGrad.apply(gy, x, pat, tuple(values.shape))
        return gval, gx, None, None


class _CsrGrad(torch.autograd.Function):
    """G[..., k] = sum_c u[..., row_k, c] conj(w[..., col_k, c]) reduced to the values' shape (xk_csr_sddmm): the
    gradient of the CSR apply w.r.t. the stored values.  Batch dims the values do not have are folded into the
    columns, so the kernel sums them in a fixed order.  Bilinear for real dtypes, sesquilinear for complex ones
    (linear in u, antilinear in w): its backward is two CSR applies with G as the values, grad u = A_gg w and
    grad w = A_gg^H u — the adjoint apply conjugates gg, which is what the antilinear slot asks for."""

    @staticmethod
    def forward(ctx, u, w, pat, vshape):
        ctx.save_for_backward(u, w)
        ctx.pat = pat
        nb, FB, keep, fold = _batch_plan(vshape[:-1], u.shape[:-2], w.shape[:-2])
        up, wp = _to_panel(u, nb, FB, keep, fold), _to_panel(w, nb, FB, keep, fold)
        g = _k.csr_sddmm(pat, up.resolve_conj(), wp.resolve_conj())        # (nkeep, nnz)
        return g.reshape(vshape)

    @staticmethod
    def backward(ctx, gg):
        u, w = ctx.saved_tensors
        pat = ctx.pat
        gu = gw = None
        if ctx.needs_input_grad[0]:
            gu = _sum_to_shape(_CsrMM.apply(gg, w, pat, False), u.shape)
        if ctx.needs_input_grad[1]:
            gw = _sum_to_shape(_CsrMM.apply(gg, u, pat, True), w.shape)
        return gu, gw, None, None


def _csr_native(pat, values, x, trans):
    nout = pat.N if trans else pat.M
    r = x.shape[-1]
    nb, FB, keep, fold = _batch_plan(list(values.shape[:-1]), list(x.shape[:-2]))
    xp = _to_panel(x, nb, FB, keep, fold).resolve_conj()                   # (nkeep, fold * r, nin)
    valf = values.resolve_conj().reshape(-1, pat.nnz)   # a lazily conjugated view: the conjugated numbers
    if pat.nnz > 1 and valf.stride(-1) != 1:
        valf = valf.contiguous()
    y = _k.csr_mm(pat, valf, xp, trans=trans)
    y = y.reshape(*[FB[d] for d in keep], *[FB[d] for d in fold], r, nout)
    inv = [0] * (nb + 2)
    for pos, d in enumerate(keep + fold + [nb + 1, nb]):
        inv[d] = pos
    return y.permute(*inv)


class SparseLinearOperator(LinearOperator):
    """Sparse operator in CSR storage with one pattern shared by the batch: ``crow_indices (M+1,)``,
    ``col_indices (nnz,)`` (int32 or int64, kept as int32) and ``values (*B, nnz)`` or ``(nnz,)`` (broadcast over
    the batch); ``shape`` is ``(M, N)`` or ``(*B, M, N)``.  Duplicate (row, col) entries add up, columns need not be
    sorted, empty rows and nnz = 0 are legal.  The structure is validated once, here.

    fp32 / fp64 / complex64 / complex128 values on a HIP device are applied by the xk_csr_mm HIP kernels (the
    adjoint on a CSC view built on first use, complex values conjugated as they are loaded) and differentiated
    w.r.t. the values by xk_csr_sddmm; host tensors and mixed dtypes use the torch expression
    ``csr_apply_torch``.  Only ``values`` is a parameter (``_getparamnames``): the indices are
    structure, so ``uselinopparams`` and the implicit backward swap the values alone."""

    def __init__(self, crow_indices, col_indices, values, shape, is_hermitian=False):
        shape = tuple(int(s) for s in shape)
        if len(shape) < 2:
            raise RuntimeError("SparseLinearOperator: shape must be (*B, M, N), got %s" % (shape,))
        M, N = shape[-2:]
        bshape = shape[:-2] if len(shape) > 2 else tuple(values.shape[:-1])
        crow, col = crow_indices, col_indices
        for name, t in (("crow_indices", crow), ("col_indices", col)):
            if not isinstance(t, torch.Tensor) or t.dim() != 1 or t.dtype not in (torch.int32, torch.int64):
                raise RuntimeError("SparseLinearOperator: %s must be a 1-D int32 / int64 tensor" % name)
        if not isinstance(values, torch.Tensor) or values.dim() < 1:
            raise RuntimeError("SparseLinearOperator: values must be a tensor (*B, nnz) or (nnz,)")
        nnz = col.numel()
        if M < 0 or N < 0 or M >= 2 ** 31 or N >= 2 ** 31:
            raise RuntimeError("SparseLinearOperator: dimensions (%d, %d) out of the int32 range" % (M, N))
        if nnz >= 2 ** 31:
            raise RuntimeError("SparseLinearOperator: nnz = %d does not fit int32 indices (< 2^31)" % nnz)
        if crow.numel() != M + 1:
            raise RuntimeError("SparseLinearOperator: crow_indices must have M+1 = %d entries, got %d"
                               % (M + 1, crow.numel()))
        if values.shape[-1] != nnz:
            raise RuntimeError("SparseLinearOperator: values have %d entries per member, col_indices %d"
                               % (values.shape[-1], nnz))
        if tuple(values.shape[:-1]) not in ((), bshape):
            raise RuntimeError("SparseLinearOperator: values batch %s does not match the operator batch %s"
                               % (tuple(values.shape[:-1]), bshape))
        if crow.device != values.device or col.device != values.device:
            raise RuntimeError("SparseLinearOperator: indices and values must live on one device (%s, %s, %s)"
                               % (crow.device, col.device, values.device))
        c64 = crow.to(torch.int64)
        if int(c64[0]) != 0:
            raise RuntimeError("SparseLinearOperator: crow_indices[0] must be 0, got %d" % int(c64[0]))
        if M > 0 and bool((c64[1:] < c64[:-1]).any()):
            raise RuntimeError("SparseLinearOperator: crow_indices must be non-decreasing")
        if int(c64[-1]) != nnz:
            raise RuntimeError("SparseLinearOperator: crow_indices[-1] = %d must equal nnz = %d" % (int(c64[-1]), nnz))
        if nnz > 0:
            lo, hi = int(col.min()), int(col.max())
            if lo < 0 or hi >= N:
                raise RuntimeError("SparseLinearOperator: column index out of range [0, %d): found %d"
                                   % (N, lo if lo < 0 else hi))
        super().__init__(shape=(*bshape, M, N), is_hermitian=is_hermitian, dtype=values.dtype, device=values.device,
                         _suppress_hermit_warning=True)
        self.crow = crow.to(torch.int32).contiguous()
        self.col = col.to(torch.int32).contiguous()
        self.values = values
        self.nnz = nnz
        self._pattern = _CsrPattern(self.crow, self.col, M, N)
        if values.is_cuda:
            self._pattern.csr()               # bin the rows once, at construction

    @classmethod
    def from_torch(cls, t, is_hermitian=False):
        """From a 2-D torch sparse CSR or COO tensor, or a batched CSR tensor whose members share one pattern."""
        if not isinstance(t, torch.Tensor):
            raise RuntimeError("SparseLinearOperator.from_torch: expected a torch sparse tensor, got %s" % type(t))
        if t.layout == torch.sparse_coo:
            if t.dim() != 2 or t.dense_dim() != 0:
                raise RuntimeError("SparseLinearOperator.from_torch: only a 2-D COO tensor is accepted, got %s"
                                   % (tuple(t.shape),))
            M, N = t.shape
            idx = t._indices().to(torch.int64)
            vals = t._values()
            # stable sort by row: entries keep their order inside a row, duplicates are summed by the apply
            order = torch.sort(idx[0], stable=True).indices
            rows, cols, vals = idx[0][order], idx[1][order], vals[order]
            crow = torch.zeros(M + 1, dtype=torch.int64, device=t.device)
            crow[1:] = torch.cumsum(torch.bincount(rows, minlength=M), 0)
            return cls(crow, cols, vals, (M, N), is_hermitian)
        if t.layout == torch.sparse_csr:
            if t.dense_dim() != 0:
                raise RuntimeError("SparseLinearOperator.from_torch: hybrid CSR tensors are not supported")
            crow, col, vals = t.crow_indices(), t.col_indices(), t.values()
            if t.dim() == 2:
                return cls(crow, col, vals, tuple(t.shape), is_hermitian)
            bshape = tuple(t.shape[:-2])
            crow2, col2 = crow.reshape(-1, crow.shape[-1]), col.reshape(-1, col.shape[-1])
            if not (bool((crow2 == crow2[:1]).all()) and bool((col2 == col2[:1]).all())):
                raise RuntimeError("SparseLinearOperator.from_torch: the members of a batched CSR tensor must share "
                                   "one sparsity pattern")
            return cls(crow2[0], col2[0], vals.reshape(*bshape, -1), tuple(t.shape), is_hermitian)
        raise RuntimeError("SparseLinearOperator.from_torch: expected a sparse CSR or COO tensor, got layout %s"
                           % t.layout)

    def _apply(self, x, trans):
        if _native_dtype(self.values) and x.dtype == self.values.dtype:
            return _CsrMM.apply(self.values, x, self._pattern, trans)
        return csr_apply_torch(self.crow, self.col, self.values, x, self.shape[-2], self.shape[-1], trans,
                               row_of=self._pattern.row_of)

    def _mv(self, x):
        return self._apply(x.unsqueeze(-1), False).squeeze(-1)

    def _mm(self, x):
        return self._apply(x, False)

    def _rmv(self, x):
        return self._apply(x.unsqueeze(-1), True).squeeze(-1)

    def _rmm(self, x):
        return self._apply(x, True)

    def _fullmatrix(self):
        M, N = self.shape[-2:]
        v = self.values
        dense = torch.zeros((*v.shape[:-1], M * N), dtype=v.dtype, device=v.device)
        lin = self._pattern.row_of.to(torch.int64) * N + self.col.to(torch.int64)
        dense = dense.index_add(-1, lin, v).reshape(*v.shape[:-1], M, N)
        return dense.expand(*self.shape)

    def _getparamnames(self, prefix=""):
        return [prefix + "values"]


# ------------------------------------------------------------------------ helpers
def _storage_token(t):
    """Identity of a tensor's contents as far as it can be known without reading them: storage address,
    view geometry and the in-place version counter."""
    return (t.data_ptr(), tuple(t.shape), tuple(t.stride()), t._version)


def _is_hermitian_matrix(mat):
    """-> (hermitian within torch.allclose like the reference's check, exactly hermitian bit for bit)."""
    if mat.shape[-2] != mat.shape[-1]:
        return False, False
    if mat.numel() <= (1 << 24) or mat.dim() == 2:
        mt = mat.transpose(-2, -1).conj()
        close = bool(torch.allclose(mat, mt))
        return close, close and bool(torch.equal(mat, mt))
    # large batched matrices: one member at a time, to bound the temporaries
    flat = mat.reshape(-1, *mat.shape[-2:])
    exact = True
    for i in range(flat.shape[0]):
        mt = flat[i].transpose(-2, -1).conj()
        if not torch.allclose(flat[i], mt):
            return False, False
        exact = exact and bool(torch.equal(flat[i], mt))
    return True, exact


def checklinop(linop):
    """Shape / linearity / batching checks of an operator (reference: linop.py:710-802)."""
    shape = linop.shape
    p, q = shape[-2:]
    bs = tuple(shape[:-2])

    def runtest(name, xshape, yshape):
        x = torch.rand(xshape, dtype=linop.dtype, device=linop.device)
        fcn = getattr(linop, name)
        try:
            y = fcn(x)
        except Exception:
            raise RuntimeError("An error is raised from .%s with input shape: %s (linear operator shape: %s)\n"
                               "--- full traceback ---\n%s" % (name, tuple(xshape), tuple(linop.shape),
                                                               traceback.format_exc()))
        assert list(y.shape) == list(yshape), \
            "The output shape of .%s is not correct. Input: %s, expected output: %s, output: %s\n%s" % \
            (name, tuple(x.shape), tuple(yshape), tuple(y.shape), str(linop))
        x2 = 1.25 * x
        y2 = fcn(x2)
        assert torch.allclose(y2, 1.25 * y), "Linearity check fails\n%s\n" % str(linop)
        assert torch.allclose(fcn(0 * x), y * 0), "Linearity check (with 0) fails\n" + str(linop)
        both = fcn(torch.stack((x, x2), dim=0))
        msg = "Batched test fails (expanding batches changes the results)" + str(linop)
        assert torch.allclose(both[0], y), msg
        assert torch.allclose(both[1], y2), msg

    def shapes(inner, outer):
        xs = [(inner,), (1, inner), (1, 1, inner), (*bs, inner), (1, *bs, inner)]
        ys = [(*bs, outer), (*bs, outer) if len(bs) >= 1 else (1, outer),
              (*bs, outer) if len(bs) >= 2 else (1, 1, outer), (*bs, outer), (1, *bs, outer)]
        return zip(xs, ys)

    r = 2
    for xs, ys in shapes(q, p):
        runtest("mv", xs, ys)
        runtest("mm", (*xs, r), (*ys, r))
    if not linop.is_rmv_implemented:
        return
    for xs, ys in shapes(p, q):
        runtest("rmv", xs, ys)
        runtest("rmm", (*xs, r), (*ys, r))


def _indent(s, nspace):
    pad = " " * nspace
    lines = s.split("\n")
    return "\n".join([lines[0]] + [pad + ln for ln in lines[1:]])


def _shape2str(shape):
    return "(%s)" % (", ".join(str(s) for s in shape))
