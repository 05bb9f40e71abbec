"""lstsq — least squares with a rectangular LinearOperator:  min |A x - b|^2 + damp^2 |x|^2  per column of B.

An extension (the reference has no lstsq): LSMR (Fong & Saunders, SIAM J. Sci. Comput. 33 (2011) 2950) on A itself,
never on A^H A — the normal equations square the condition number.  Device operators run on the HIP kernels of
xk_lsmr.hip (`native_lsmr.lsmr`), operators in host memory on the same iteration in torch ops (`host_lsmr.lsmr`).
The backward is implicit: two more LSMR solves and VJPs through `A.mm`, no graph through the iteration.
"""
import torch
from xitorch_amd._util import assert_runtime, merge_options, get_method

__all__ = ["lstsq"]


def lstsq(A, B, damp=0.0, bck_options={}, method=None, **fwd_options):
    r"""
    Solve :math:`\min_x \|\mathbf{A}x - b\|^2 + \mathrm{damp}^2\|x\|^2` for every column ``b`` of ``B``.

    Arguments
    ---------
    A: LinearOperator ``(*BA, m, n)``, any ``m``, ``n``
    B: torch.Tensor ``(*BB, m, ncols)``
    damp: float
        Non-negative Tikhonov parameter (a Python number: it is not differentiated)
    bck_options: dict
        LSMR options of the two solves of the backward pass (default: the forward's)
    method: str or None
        ``None`` or ``"lsmr"``
    **fwd_options
        ``max_niter`` (default ``4 min(m, n)``), ``atol``, ``btol`` (default ``1e-6``), ``conlim`` (default ``1e8``):
        the stopping rules S1, S2, S3 of the paper's section 6, as SciPy documents them; ``resid_calc_every`` (default
        10): how often the host reads the number of unfinished systems; ``max_restart`` (default 2); ``verbose``;
        ``trace``: a dict that receives ``niter``, ``napply``, ``torch_applies``, ``host_reads``, ``restarts``

    Returns ``X`` of shape ``(*BAB, n, ncols)``.  With ``damp = 0`` and a rank-deficient or wide ``A`` it is the
    minimum-norm minimiser (the iteration starts from 0 and never leaves the range of ``A^H``).  A
    ``ConvergenceWarning`` is issued when members end on ``max_niter``, and when members end on ``conlim`` (the result
    is then a regularised solution).  ``E``, ``M``, ``process_group`` and preconditioners are refused
    (``NotImplementedError``).

    The backward assumes full column rank when ``m >= n`` or ``damp > 0``, and full ROW rank when ``m < n`` and
    ``damp = 0``.
    """
    assert_runtime(A.shape[-2] == B.shape[-2], "Mismatch shape of A & B (A: %s, B: %s)" % (A.shape, B.shape))
    assert_runtime(not torch.is_grad_enabled() or A.is_getparamnames_implemented,
                   "The _getparamnames(self, prefix) of linear operator A must be "
                   "implemented if using lstsq with grad enabled")
    if method is None:
        method = "lsmr"
    get_method("lstsq", {"lsmr": _lsmr}, method)       # raises RuntimeError("Unknown lstsq method: ...")
    if callable(method):
        raise RuntimeError("Unknown lstsq method: %r" % (method,))
    from xitorch_amd.linalg import host_lsmr
    host_lsmr.check_lsmr_options(A, B, damp, fwd_options)
    params = A.getlinopparams()
    return _LstsqFunction.apply(A, B, float(damp), fwd_options, bck_options, *params)


def _lsmr(A, B, damp, stack=None, **options):
    """device dispatch: host memory -> host_lsmr, everything else -> the HIP kernels.  stack: None (A with damp),
    "A" (the stacked [A; damp I], B has m + n rows) or "AH" (its adjoint; the result has m + n rows)."""
    from xitorch_amd.linalg import host_lsmr, native_lsmr
    if torch.device(A.device).type == "cpu":
        if stack is None:
            return host_lsmr.lsmr(A, B, damp, **options)
        return host_lsmr.lsmr_stacked(A, B, damp, stack, **options)
    return native_lsmr.lsmr(A, B, damp, stack=stack, **options)


class _LstsqFunction(torch.autograd.Function):
    """Forward: LSMR, graph-free.  Backward: with N = A^H A + damp^2 I, r = b - A x and gx the incoming gradient,
    from  dx = N^-1 (dA^H r - A^H dA x + A^H db):
      column rank (m >= n or damp > 0):  z = Abar w is the minimum-norm solution of Abar^H z = gx (Abar = [A; damp I]),
        w = N^-1 gx the zero-residual least-squares solution of Abar w = z;  grad_B = A w = z[:m];  parameters: the VJP
        of A.mm(w) with cotangent r plus that of A.mm(x) with cotangent -A w;
      row rank (m < n, damp = 0; x = A^H (A A^H)^-1 b):  p = argmin |A^H p - gx|, q = gx - A^H p, y = argmin |A^H y - x|;
        grad_B = p;  parameters: the VJP of A.mm(x) with cotangent -p plus that of A.mm(q) with cotangent y."""

    @staticmethod
    def forward(ctx, A, B, damp, fwd_options, bck_options, *params):
        config = merge_options({}, fwd_options)
        bck = merge_options({}, fwd_options)
        bck.pop("trace", None)
        ctx.bck_config = merge_options(bck, bck_options)
        with A.uselinopparams(*params):
            x = _lsmr(A, B, damp, **config)
        ctx.A, ctx.damp = A, damp
        ctx.save_for_backward(x, B, *params)
        return x

    @staticmethod
    def backward(ctx, gx):
        x, B = ctx.saved_tensors[:2]
        params = ctx.saved_tensors[2:]
        A, damp, cfg = ctx.A, ctx.damp, ctx.bck_config
        m, n = A.shape[-2], A.shape[-1]
        gx = gx.to(x.dtype)
        with torch.no_grad(), A.uselinopparams(*params):
            if m >= n or damp > 0:
                z = _lsmr(A, gx, damp, stack="AH", **cfg)
                w = _lsmr(A, z, damp, stack="A", **cfg)
                Aw = z[..., :m, :]
                grad_B = Aw
                r = B - A.mm(x)
                pairs = ((w, r), (x, -Aw))
            else:
                p = _lsmr(A, gx, 0.0, stack="AH", **cfg)
                q = gx - A.rmm(p)
                y = _lsmr(A, x, 0.0, stack="AH", **cfg)
                grad_B = p
                pairs = ((x, -p), (q, y))
        grad_B = _sum_to_shape(grad_B, B.shape)
        grad_params = [None] * len(params)
        if params:
            with torch.enable_grad():
                ps = [p_.clone().requires_grad_() for p_ in params]
                with A.uselinopparams(*ps):
                    outs = [A.mm(vec.detach()) for vec, _ in pairs]
            cots = [cot.detach().expand_as(o) for (_, cot), o in zip(pairs, outs)]
            grad_params = torch.autograd.grad(outs, ps, grad_outputs=cots, allow_unused=True)
        return (None, grad_B, None, None, None, *grad_params)


def _sum_to_shape(g, shape):
    """reduce a broadcast gradient (*BAB, m, nc) to the shape of B"""
    if tuple(g.shape) == tuple(shape):
        return g
    extra = g.dim() - len(shape)
    if extra > 0:
        g = g.sum(dim=tuple(range(extra)))
    dims = tuple(i for i, (a, b) in enumerate(zip(g.shape, shape)) if b == 1 and a != 1)
    if dims:
        g = g.sum(dim=dims, keepdim=True)
    return g
