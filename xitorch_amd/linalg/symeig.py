"""symeig / lsymeig / usymeig / svd — functional front-ends of the eigen path.

Same signatures, defaults, argument checks and implicit-differentiation backward as the
reference (xitorch/linalg/symeig.py:17-461); the forward method table points at the native
HIP eigensolver (xitorch_amd/linalg/native_eig.py) and the backward solve goes through
`xitorch_amd.linalg.solve` (native Krylov kernels).
"""
import warnings
import torch
from xitorch_amd.linop import LinearOperator  # noqa: F401  (re-exported for type references in user code)
from xitorch_amd.linalg.solve import solve
from xitorch_amd.linalg.native_eig import davidson, exacteig
from xitorch_amd.linalg.native_chebfsi import chebfsi
from xitorch_amd.linalg.native_lobpcg import lobpcg
from xitorch_amd.debug import is_debug_enabled
from xitorch_amd._util import assert_runtime, merge_options, null_context, get_method, pop_keys, MathWarning

__all__ = ["lsymeig", "usymeig", "symeig", "svd"]


def lsymeig(A, neig=None, M=None, bck_options={}, method=None, **fwd_options):
    return symeig(A, neig, "lowest", M, method=method, bck_options=bck_options, **fwd_options)


def usymeig(A, neig=None, M=None, bck_options={}, method=None, **fwd_options):
    return symeig(A, neig, "uppest", M, method=method, bck_options=bck_options, **fwd_options)


def symeig(A, neig=None, mode="lowest", M=None, bck_options={}, method=None, **fwd_options):
    r"""
    Obtain ``neig`` lowest (or uppermost) eigenvalues and eigenvectors of a Hermitian linear
    operator, :math:`\mathbf{AX = MXE}`.

    Arguments
    ---------
    A: LinearOperator
        Hermitian operator of shape ``(*BA, q, q)``
    neig: int or None
        Number of eigenpairs (``None``: all)
    mode: str
        ``"lowest"``, ``"uppermost"``/``"uppest"``, or ``"nearest"`` (extension): the ``neig`` pairs whose eigenvalues
        are nearest the target ``sigma=`` (a forward option: a number, or a real tensor broadcastable to the batch
        dimensions; it carries no gradient).  Served by ``method="exacteig"`` (full ``eigh``, then the selection) and
        ``method="chebfsi"`` (a Jackson-damped Chebyshev band-pass filter centred on ``sigma``, ``M=None``; options
        ``filter_degree`` (``None``: adaptive), ``max_degree`` (1000), ``filter_tail`` (0.1)); ``"davidson"`` and
        ``"lobpcg"`` raise ``NotImplementedError``.  A ``sigma`` outside the spectrum gives the ``"lowest"`` /
        ``"uppest"`` pairs.  A ``sigma`` deep inside a spectral gap (its distance to the nearest eigenvalue far
        exceeds the spread of the wanted ones) converges slowly with ``chebfsi``: no filter centred on ``sigma`` then
        separates the ``neig``-th from the next eigenvalue well.  An exact tie in ``|lambda - sigma|`` at the boundary
        of the wanted set makes the answer ambiguous.  Missing ``sigma`` raises ``ValueError``.
    M: LinearOperator or None
        Hermitian right-hand-side operator ``(*BM, q, q)`` (``None``: identity)
    bck_options: dict
        Options of :func:`solve` for the backward pass, plus ``degen_atol`` / ``degen_rtol``
        (thresholds below which two eigenvalues are treated as degenerate; defaults
        ``eps**0.6`` / ``eps**0.4``)
    method: str or callable or None
        ``"exacteig"`` (default, dense), ``"davidson"`` (native HIP block Davidson), ``"chebfsi"`` (Chebyshev-filtered
        subspace iteration on the HIP kernels: a fixed block of ``neig + nguard`` vectors, for many pairs; ``M=None``; complex
        blocks wider than 32 vectors solve their small eigenproblem with ``torch.linalg.eigh``), ``"lobpcg"`` (LOBPCG in
        its basis-orthonormal form on the HIP kernels: constant storage of three stacks of ``3 (neig + nguard)`` vectors,
        takes ``M`` and ``precond=`` like ``davidson``; complex blocks wider than 16 vectors solve their small
        eigenproblem with ``torch.linalg.eigh``), or a callable
        ``f(A, neig, mode, M, **fwd_options) -> (evals, evecs)``
    **fwd_options
        Method-specific options

    Returns
    -------
    (eigenvalues ``(*BAM, neig)``, eigenvectors ``(*BAM, q, neig)``), eigenvalues ascending.
    """
    assert_runtime(A.is_hermitian, "The linear operator A must be Hermitian")
    assert_runtime(not torch.is_grad_enabled() or A.is_getparamnames_implemented,
                   "The _getparamnames(self, prefix) of linear operator A must be "
                   "implemented if using symeig with grad enabled")
    if M is not None:
        assert_runtime(M.is_hermitian, "The linear operator M must be Hermitian")
        assert_runtime(M.shape[-1] == A.shape[-1], "The shape of A & M must match (A: %s, M: %s)" % (A.shape, M.shape))
        assert_runtime(not torch.is_grad_enabled() or M.is_getparamnames_implemented,
                       "The _getparamnames(self, prefix) of linear operator M must be "
                       "implemented if using symeig with grad enabled")
    mode = mode.lower()
    if mode == "uppermost":
        mode = "uppest"
    if method is None:
        method = "exacteig"          # the reference's default for every operator kind (quirk Q7)
    if neig is None:
        neig = A.shape[-1]
    if is_debug_enabled():
        A.check()
        if M is not None:
            M.check()
    if mode == "nearest" and fwd_options.get("sigma") is None:
        raise ValueError("symeig: mode='nearest' needs the target: pass sigma= (a number, or a real tensor "
                         "broadcastable to the batch dimensions)")
    if method == "exacteig":
        return exacteig(A, neig, mode, M, sigma=fwd_options.get("sigma")) if mode == "nearest" \
            else exacteig(A, neig, mode, M)
    fwd_options["method"] = method
    params = A.getlinopparams()
    mparams = M.getlinopparams() if M is not None else []
    return _SymeigFunction.apply(A, neig, mode, M, fwd_options, bck_options, len(params), *params, *mparams)


def svd(A, k=None, mode="uppest", bck_options={}, method=None, **fwd_options):
    r"""
    Singular value decomposition :math:`\mathbf{A} = \mathbf{U\Sigma V}^H` of an operator
    ``(*BA, m, n)`` through ``symeig`` of ``A^H A`` or ``A A^H`` (whichever is smaller).
    Returns ``(u (*BA,m,k), s (*BA,k), vh (*BA,k,n))``.  (reference: symeig.py:146-250)

    ``method="gkl"`` (extension; every other value keeps the route above) works on ``A`` itself: Golub-Kahan-Lanczos
    bidiagonalisation with thick restart on the HIP kernels (``native_gkl.gkl``; an operator in host memory is served
    by ``host_eig.gkl``).  The route above squares the condition number, so a singular value below
    ``sqrt(eps) * sigma_max`` comes back as noise; ``gkl`` returns every wanted triplet to about
    ``min_eps * sigma_max``, ``mode="lowest"`` included.  Forward options: ``ncv`` (basis size, ``k < ncv <= 64``,
    default ``min(max(2k + 8, 20), min(m, n))``), ``max_niter`` (restart cycles), ``min_eps`` (a triplet is converged
    when ``|beta P[last, i]| <= min_eps * sigma_max``), ``V0`` (``(*BA, n, k0)`` guesses of right singular vectors),
    ``v_init``, ``verbose``, ``trace``.  ``process_group`` raises ``NotImplementedError``; ``k > ncv - 1`` or
    ``ncv > 64`` raise ``ValueError``; a problem whose short side is ``<= max(2k, 16)`` goes to ``torch.linalg.svd``.
    When ``max_niter`` ends first the last Ritz block is returned with a ``ConvergenceWarning`` (thick restart keeps
    the wanted triplets, so no separate best block is tracked).  A breakdown (``alpha`` or ``beta`` below
    ``u * sigma_max``) never raises: the member continues from a random vector; on the device each recovery costs one
    more read of the status words and a rerun of the rest of the cycle, so keep ``ncv`` below the numerical rank.
    ``RuntimeError`` is raised only for a zero start vector or a projected SVD that hits its sweep limit.
    ``s`` is ascending, as on the other route; ``u`` carries the iteration's own orthonormality (it is not
    ``A v / clamp(s)``).

    Gradient of ``method="gkl"``: the triplets are eigenpairs ``(s, [u; v] / sqrt(2))`` of the Hermitian augmented
    operator ``[[0, A], [A^H, 0]]``, and ``symeig``'s implicit backward is applied to that operator unchanged: one
    shifted solve per backward pass.  That system is indefinite, so the backward solver defaults to
    ``bck_options={"method": "minres"}`` (any ``method`` given in ``bck_options`` is respected).  For ``m != n`` the
    augmented operator has ``|m - n|`` zero eigenvalues: the backward of a triplet with ``s`` close to 0 is
    ill-conditioned.  The loss must not depend on the phase of a pair ``(u_i, v_i)``.
    """
    if is_debug_enabled():
        A.check()
    if method == "gkl":
        return _svd_gkl(A, k, mode, bck_options, fwd_options)
    m, n = A.shape[-2], A.shape[-1]
    if m < n:
        AA = A.matmul(A.H, is_hermitian=True)
    else:
        AA = A.H.matmul(A, is_hermitian=True)
    evals, evecs = symeig(AA, k, mode, bck_options=bck_options, method=method, **fwd_options)
    s = torch.sqrt(torch.clamp(evals, min=0.0))
    sdiv = torch.clamp(s, min=1e-12).unsqueeze(-2)
    if m < n:
        u = evecs
        v = A.rmm(u) / sdiv
    else:
        v = evecs
        u = A.mm(v) / sdiv
    return u, s, v.transpose(-2, -1).conj()


class _AugmentedOperator(LinearOperator):
    """The Hermitian operator ``[[0, A], [A^H, 0]]`` of order m + n whose eigenpairs with positive eigenvalue are
    ``(sigma, [u; v] / sqrt(2))``: what the implicit backward of ``svd(method="gkl")`` differentiates.  Its parameters
    are A's."""

    def __init__(self, A):
        m, n = A.shape[-2], A.shape[-1]
        super().__init__(shape=(*A.shape[:-2], m + n, m + n), is_hermitian=True, dtype=A.dtype, device=A.device,
                         _suppress_hermit_warning=True)
        self.A = A
        self._m = m

    def _mv(self, x):
        return self._mm(x.unsqueeze(-1)).squeeze(-1)

    def _mm(self, x):
        m = self._m
        return torch.cat((self.A.mm(x[..., m:, :]), self.A.rmm(x[..., :m, :])), dim=-2)

    def _getparamnames(self, prefix=""):
        return self.A._getparamnames(prefix=prefix + "A.")


def _svd_gkl(A, k, mode, bck_options, fwd_options):
    from xitorch_amd.linalg.native_gkl import gkl
    mode = mode.lower()
    if mode == "uppermost":
        mode = "uppest"
    m, n = A.shape[-2], A.shape[-1]
    if k is None:
        k = min(m, n)
    wants_grad = torch.is_grad_enabled() and A.is_getparamnames_implemented and \
        any(p.requires_grad for p in A.getlinopparams())
    if not wants_grad:
        with torch.no_grad():
            u, s, v = gkl(A, k, mode, **fwd_options)
        return u, s, v.transpose(-2, -1).conj()
    rt2 = 2.0 ** 0.5

    def method(aug, neig, mode_, M, **opts):
        u, s, v = gkl(aug.A, neig, mode, **opts)
        return s, torch.cat((u, v), dim=-2) / rt2

    bck = dict(bck_options)
    bck.setdefault("method", "minres")
    evals, evecs = symeig(_AugmentedOperator(A), k, mode, bck_options=bck, method=method, **fwd_options)
    u, v = evecs[..., :m, :] * rt2, evecs[..., m:, :] * rt2
    return u, evals, v.transpose(-2, -1).conj()


def _custom_exacteig(A, neig, mode, M=None, **options):
    return exacteig(A, neig, mode, M, sigma=options.get("sigma"))


_SYMEIG_METHODS = {"davidson": davidson, "chebfsi": chebfsi, "lobpcg": lobpcg, "custom_exacteig": _custom_exacteig}


class _SymeigFunction(torch.autograd.Function):
    """Forward: run the chosen eigensolver without a graph.  Backward: implicit differentiation of
    the (possibly degenerate) partial eigendecomposition (reference: symeig.py:252-402,
    arXiv:2011.04366): one shifted multi-RHS solve ``(A - lam_i M) g_i = -P b_i`` plus a VJP
    through ``A.mm`` (and ``M.mm``)."""

    @staticmethod
    def forward(ctx, A, neig, mode, M, fwd_options, bck_options, na, *amparams):
        params, mparams = amparams[:na], amparams[na:]
        config = merge_options({}, fwd_options)
        ctx.bck_config = merge_options({"degen_atol": None, "degen_rtol": None}, bck_options)
        ctx.bck_alg_config = pop_keys(ctx.bck_config, ["degen_atol", "degen_rtol"])
        method = config.pop("method")
        with A.uselinopparams(*params), (M.uselinopparams(*mparams) if M is not None else null_context()):
            fcn = get_method("symeig", _SYMEIG_METHODS, method)
            evals, evecs = fcn(A, neig, mode, M, **config)
        ctx.save_for_backward(evals, evecs, *amparams)
        ctx.na, ctx.A, ctx.M = na, A, M
        return evals, evecs

    @staticmethod
    def backward(ctx, grad_evals, grad_evecs):
        evals, evecs = ctx.saved_tensors[:2]
        amparams = ctx.saved_tensors[2:]
        na, A, M = ctx.na, ctx.A, ctx.M
        params, mparams = amparams[:na], amparams[na:]
        atol, rtol = ctx.bck_alg_config["degen_atol"], ctx.bck_alg_config["degen_rtol"]
        eps = torch.finfo(evals.dtype).eps
        atol = eps ** 0.6 if atol is None else atol
        rtol = eps ** 0.4 if rtol is None else rtol

        idx_degen = None
        if atol > 0 or rtol > 0:
            dmap, isdegen = _check_degen(evals, atol, rtol)
            if isdegen:
                idx_degen = dmap

        # connect A.mm(evecs) to fresh leaf copies of the operator parameters
        with torch.enable_grad():
            params = [p.clone().requires_grad_() for p in params]
            with A.uselinopparams(*params):
                loss = A.mm(evecs)

        if is_debug_enabled() and idx_degen is not None:
            xtg = torch.matmul(evecs.transpose(-2, -1).conj(), grad_evecs)
            req = idx_degen * (xtg - xtg.transpose(-2, -1).conj())
            tol = xtg.abs().max() * grad_evecs.shape[-2] * torch.finfo(grad_evecs.dtype).eps
            if not torch.all(torch.abs(req) <= tol):
                warnings.warn(MathWarning(
                    "Degeneracy appears but the loss function seem to depend strongly on the eigenvector. "
                    "The gradient might be incorrect.\nEigenvalues:\n%s\nDegenerate map:\n%s\n"
                    "Requirements (should be all 0s):\n%s" % (str(evals), str(idx_degen), str(req))))

        gevalsA = grad_evals.unsqueeze(-2) * evecs
        with (M.uselinopparams(*mparams) if M is not None else null_context()):
            Bmat = _ortho(grad_evecs, evecs, D=idx_degen, M=M, mright=False)
            shift = evals + 1e-14 if torch.is_complex(Bmat) else evals
            with A.uselinopparams(*params):
                gevecs = solve(A, -Bmat, shift, M, bck_options=ctx.bck_config, **ctx.bck_config)
            gevecsA = _ortho(gevecs, evecs, D=None, M=M, mright=True)

        gaccumA = gevalsA + gevecsA
        grad_params = torch.autograd.grad(outputs=(loss,), inputs=params, grad_outputs=(gaccumA,),
                                          create_graph=torch.is_grad_enabled())
        grad_mparams = []
        if M is not None:
            with torch.enable_grad():
                mparams = [p.clone().requires_grad_() for p in mparams]
                with M.uselinopparams(*mparams):
                    mloss = M.mm(evecs)
            ev = evals.unsqueeze(-2)
            par = (-0.5 * torch.einsum("...ae,...ae->...e", grad_evecs, evecs.conj())).unsqueeze(-2) * evecs
            gaccumM = -gevalsA * ev - gevecsA * ev + par
            grad_mparams = torch.autograd.grad(outputs=(mloss,), inputs=mparams, grad_outputs=(gaccumM,),
                                               create_graph=torch.is_grad_enabled())
        return (None, None, None, None, None, None, None, *grad_params, *grad_mparams)


def _check_degen(evals, degen_atol, degen_rtol):
    # (*, neig, neig) 0/1 map of eigenvalue pairs closer than atol + rtol*|lam|  (symeig.py:404-414)
    diff = torch.abs(evals.unsqueeze(-2) - evals.unsqueeze(-1))
    thresh = degen_atol + degen_rtol * torch.abs(evals).unsqueeze(-1)
    dmap = (diff < thresh).to(evals.dtype)
    return dmap, bool(torch.sum(dmap) > torch.numel(evals))


def _ortho(A, B, *, D=None, M=None, mright=False):
    """Remove from every column of ``A`` its component along the matching column of ``B`` (or along
    the whole degenerate block given by the map ``D``), in the ``M`` inner product
    (reference: symeig.py:416-448)."""
    if D is None:
        Bc = B.conj()
        dot = lambda X: torch.einsum("...rc,...rc->...c", X, Bc).unsqueeze(-2)
        if M is None:
            return A - dot(A) * B
        if mright:
            return A - dot(M.mm(A)) * B
        return A - M.mm(dot(A) * B)
    BH = B.transpose(-2, -1).conj()
    if M is None:
        return A - torch.matmul(B, D * torch.matmul(BH, A))
    if mright:
        return A - torch.matmul(B, D * torch.matmul(BH, M.mm(A)))
    return A - M.mm(torch.matmul(B, D * torch.matmul(BH, A)))
