"""eigs — a few eigenpairs of a NON-Hermitian LinearOperator: convection-diffusion stencils, transition matrices,
Jacobians, non-Hermitian Hamiltonians, on dense, banded, CSR and matrix-free operators.

An extension (the reference's eigensolvers assume A = A^H); what `scipy.sparse.linalg.eigs` offers without
shift-and-invert.  The method is Krylov-Schur Arnoldi (Stewart 2001): device operators run on the HIP kernels
(`native_arnoldi.arnoldi`: the apply and Gram-Schmidt kernels of `svd(method="gkl")` plus xk_arn_finish and the small
Schur kernel xk_arn_schur), operators in host memory on the same iteration in torch ops (`host_eig.arnoldi`).
"""
import torch
from xitorch_amd.linalg import host_eig

__all__ = ["eigs"]

_OPTIONS = ("max_niter", "min_eps", "ncv", "V0", "v_init", "rng_device", "verbose", "trace", "M", "process_group")


def _refuse_grad(A):
    if torch.is_grad_enabled() and any(p.requires_grad for p in A.getlinopparams()):
        raise NotImplementedError("eigs is forward-only (the gradient needs left eigenvectors, which are not built): "
                                  "the operator's parameters require grad; call it under torch.no_grad() or detach "
                                  "the parameters")


def eigs(A, neig, which="LM", method=None, **fwd_options):
    r"""
    ``neig`` eigenpairs :math:`\mathbf{A}\mathbf{x}_i = \lambda_i \mathbf{x}_i` of a square operator that need not be
    Hermitian.

    Arguments
    ---------
    A: LinearOperator ``(*BA, n, n)``
        float64, float32, complex128 or complex64.  ``is_hermitian`` is ignored: the operator is treated as general
        (for a Hermitian one ``symeig`` is cheaper and returns real eigenvalues).
    neig: int
    which: str
        ``"LM"`` largest ``|lambda|``; ``"LR"`` / ``"SR"`` largest / smallest real part; ``"LI"`` / ``"SI"`` largest /
        smallest imaginary part (complex operators only: ``ValueError`` on a real one).  ``"SM"`` is refused: it needs
        shift-and-invert, which is not built.
    method: str or None
        ``"arnoldi"`` (default) or ``"exacteig"`` (``torch.linalg.eig`` of ``A.fullmatrix()`` in host memory and the
        same selection)
    **fwd_options
        ``max_niter=100`` restart cycles; ``min_eps=1e-6``: a Ritz pair is converged when ``|H[ncv, ncv-1]| |y_i[last]|
        <= min_eps * max(|theta_i|, u |H|_F)``; ``ncv=None``: basis size, default ``min(max(2 neig + 8, 20), n)``, with
        ``neig + 2 <= ncv <= 48`` (``xk_arn_max_rows()``); ``V0`` ``(*batch, n, k0)``: guesses whose sum starts the
        iteration; ``v_init``, ``rng_device``: the start vector, as for ``davidson``; ``verbose``; ``trace``: a dict
        that receives ``niter``, ``restarts``, ``napply``, ``ncv``, ``keep``, ``converged_history``, ``breakdowns``,
        ``host_reads``, ``torch_applies``, ``converged``, ``resid`` (the true residuals ``|A x_i - theta_i x_i|``
        from one more apply) and ``kept_history`` (per restart, the vectors every member kept), or ``handed_to``
        for the dense route.

    Returns ``(evals (*BA, neig), evecs (*BA, n, neig))``, always complex (complex128 for 64-bit operators, complex64
    for 32-bit ones, as ``torch.linalg.eig``).  The eigenvalues come best first by ``which``; a complex-conjugate pair
    of a real operator is adjacent, positive imaginary part first.  Each eigenvector has unit 2-norm; its phase is
    unspecified.  Pairs whose true residual misses ``min_eps * max(|theta_i|, u |H|_F)`` by more than a factor 2 raise
    one ``ConvergenceWarning`` with their count; the last Ritz block is returned.  A problem with ``n <= max(2 neig,
    16)`` is handed to the dense route.

    Forward only: operator parameters that require grad, ``M=`` and ``process_group=`` raise ``NotImplementedError``;
    ``neig > ncv - 2`` raises ``ValueError``.  Left eigenvectors: run it on ``A.H``.
    """
    unknown = [k for k in fwd_options if k not in _OPTIONS]
    if unknown:
        raise TypeError("eigs: unknown option(s) %s" % ", ".join(sorted(unknown)))
    if method is None:
        method = "arnoldi"
    if method not in ("arnoldi", "exacteig"):
        raise RuntimeError("Unknown eigs method: %s" % (method,))
    trace = fwd_options.get("trace")
    if trace is not None and not isinstance(trace, dict):
        raise TypeError("eigs: trace must be a dict or None")
    _refuse_grad(A)
    with torch.no_grad():
        if method == "exacteig":
            _, neig = host_eig._arn_check(A, neig, which, fwd_options.get("M"), fwd_options.get("process_group"))
            if trace is not None:
                trace.update(niter=0, napply=0, handed_to="dense_eig")
            return host_eig._arn_dense(A, neig, which)
        from xitorch_amd.linalg.native_arnoldi import arnoldi
        return arnoldi(A, neig, which, **fwd_options)

