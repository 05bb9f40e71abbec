"""logdet, trace_fn, quadform — what can be said about a Hermitian LinearOperator as a whole: log det A, tr A^-1,
tr f(A), by stochastic Lanczos quadrature.

An extension (the reference has none of them).  `quadform` computes z^H f(A) z by Gauss quadrature on the Lanczos
tridiagonal started on z (Golub & Meurant); `trace_fn` is the Hutchinson estimator on top of it (Ubaru, Chen & Saad,
SIAM J. Matrix Anal. Appl. 38 (2017) 1075); `logdet` is `trace_fn(A, "log")` with an implicit backward through
`solve`.  Storage is three vectors per probe whatever the step count; the operator is only ever applied.  Device
operators run on the HIP kernels of xk_slq.hip (`native_slq.forms`), operators in host memory on the same iteration in
torch ops (`host_slq.forms`).
"""
import math
import warnings
import torch
from xitorch_amd._util import MathWarning, merge_options, assert_runtime
from xitorch_amd.linalg import host_slq

__all__ = ["quadform", "trace_fn", "logdet"]


def _forms(A, Z, opt):
    """device dispatch: host memory -> host_slq, everything else -> the HIP kernels"""
    from xitorch_amd.linalg import native_slq
    if torch.device(A.device).type == "cpu":
        return host_slq.forms(A, Z, opt)
    return native_slq.forms(A, Z, opt)


def _refuse_grad(who, A, *tensors):
    if torch.is_grad_enabled() and (any(p.requires_grad for p in A.getlinopparams())
                                    or any(isinstance(t, torch.Tensor) and t.requires_grad for t in tensors)):
        raise NotImplementedError("%s is not differentiable (only logdet is): call it under torch.no_grad() or detach "
                                  "the parameters" % who)


def _run(who, A, Z, opt):
    """the forms of every column of Z and the ONE host read of a call: the number of batch members that are not
    numerically positive definite and the step counts.  Returns (q (*BAZ, p) float64 with NaN rows for such members,
    trace entries)."""
    q, bad, m, napply = _forms(A, Z, opt)
    badm = bad.any(-1)                                                 # per batch member
    q = torch.where(badm[..., None], torch.full_like(q, float("nan")), q)
    reads = 0
    summary = torch.cat([badm.sum().reshape(1).to(torch.int64), m.reshape(-1)]).tolist()      # the one read
    reads += 1                                                         # (counted where it happens, as native_lsmr does)
    nbad = summary[0]
    if nbad:
        if not callable(opt["fn"]) and opt["fn"] in host_slq.NEEDS_POSITIVE:
            warnings.warn(MathWarning("%s: %d member(s) are not numerically positive definite (a quadrature node <= 0 "
                                      "under fn='%s'): their result is NaN" % (who, nbad, opt["fn"])))
        else:
            warnings.warn(MathWarning("%s: the quadrature of %d member(s) did not converge: their result is NaN"
                                      % (who, nbad)))
    used = torch.tensor(summary[1:], dtype=torch.int64).reshape(m.shape)
    info = dict(nsteps_used=used, napply=napply, host_reads=reads)
    if opt["verbose"]:
        print("%s: %d Lanczos steps, %d operator applies, %d member(s) flagged" % (who, opt["nsteps"], napply, nbad))
    return q, info


def quadform(A, Z, fn="log", nsteps=None, **options):
    r"""
    The quadratic forms :math:`z_j^H f(\mathbf{A}) z_j` for every column :math:`z_j` of ``Z``, by ``nsteps``-point Gauss
    quadrature on the Lanczos tridiagonal of ``A`` started on :math:`z_j`.

    Arguments
    ---------
    A: LinearOperator ``(*BA, n, n)``, Hermitian (dense, banded, CSR or a user operator; float64, float32, complex128,
        complex64)
    Z: torch.Tensor ``(*BZ, n, ncols)``
    fn: str or callable
        ``"log"``, ``"inv"``, ``"sqrt"``, ``"invsqrt"``, ``"exp"`` (option ``t``: ``exp(t x)``) or ``"identity"``:
        summed inside the quadrature kernel; a callable is applied in torch, on the operator's device, to the
        ``(S, nsteps)`` node array (``S`` systems: batch members times columns)
    nsteps: int or None
        Lanczos steps = quadrature nodes, default ``min(n, 50)``, at most 128
    **options
        ``t`` (``fn="exp"``), ``verbose``, ``trace``: a dict that receives ``nsteps_used`` (per system: fewer than
        ``nsteps`` where Lanczos found an invariant subspace, the quadrature is then exact), ``napply``, ``host_reads``

    Returns a real tensor ``(*BAZ, ncols)``.  ``"log"``, ``"inv"``, ``"sqrt"`` and ``"invsqrt"`` need every quadrature
    node to be positive: a batch member with a node ``<= 0`` returns ``NaN`` and one ``MathWarning`` names how many
    members are not numerically positive definite.  Not differentiable (``NotImplementedError`` with grad enabled and a
    parameter that requires grad); ``M=`` and ``process_group=`` are refused (``NotImplementedError``).
    """
    opt = host_slq.check_options("quadform", A, fn, nsteps, options)
    assert_runtime(A.shape[-1] == Z.shape[-2], "Mismatch shape of A & Z (A: %s, Z: %s)" % (A.shape, Z.shape))
    _refuse_grad("quadform", A, Z)
    with torch.no_grad():
        q, info = _run("quadform", A, Z, opt)
    if opt["trace"] is not None:
        opt["trace"].update(info)
    return q.to(host_slq._real_dtype(A.dtype))


def _probes(who, A, probes, seed, dist):
    """the probe block (.., n, p) on the operator's device, and whether the caller supplied it"""
    n = A.shape[-1]
    if isinstance(probes, torch.Tensor):
        if probes.dim() < 2 or probes.shape[-2] != n or probes.shape[-1] < 1:
            raise ValueError("%s: a probe tensor must be (*, n, p) with n = %d, got %s" % (who, n, tuple(probes.shape)))
        return probes.detach().to(device=A.device, dtype=A.dtype)
    if isinstance(probes, bool) or not isinstance(probes, int) or probes < 1:
        raise ValueError("%s: probes must be a positive int or a tensor (*, n, p), got %r" % (who, probes))
    return host_slq.draw_probes(n, probes, A.dtype, seed, dist).to(A.device)


def _estimate(q):
    """Hutchinson: the mean over the probes and its sample standard error"""
    p = q.shape[-1]
    est = q.mean(-1)
    if p > 1:
        stderr = q.std(-1, unbiased=True) / math.sqrt(p)
    else:
        stderr = torch.full_like(est, float("nan"))
    return est, stderr


def _trace_fn(who, A, fn, probes, nsteps, seed, options):
    opt = host_slq.check_options(who, A, fn, nsteps, options)
    Z = _probes(who, A, probes, seed, opt["dist"])
    with torch.no_grad():
        q, info = _run(who, A, Z, opt)
        est, stderr = _estimate(q)
    rd = host_slq._real_dtype(A.dtype)
    if opt["trace"] is not None:
        opt["trace"].update(info, stderr=stderr.to(rd))
    return est.to(rd), Z


def trace_fn(A, fn, probes=32, nsteps=None, seed=0, **options):
    r"""
    The Hutchinson estimate of :math:`\mathrm{tr} f(\mathbf{A})`: the mean of ``quadform(A, Z, fn)`` over probes with
    :math:`E[z z^H] = I`.

    Arguments
    ---------
    A, fn, nsteps: as in ``quadform``
    probes: int or torch.Tensor
        an int ``p`` draws that many probes ``(n, p)``, shared by all batch members, on the HOST from a generator of
        their own seeded by ``seed`` (a host run and a device run of one call use the same probes); a tensor
        ``(*, n, p)`` is used as it is.  Complex operators get real probes.
    seed: int
    **options
        ``dist``: ``"rademacher"`` (default) or ``"gaussian"``; ``t``, ``verbose``; ``trace``: a dict that receives
        ``stderr`` (the sample standard error over the probes, ``(*BA,)``), ``nsteps_used``, ``napply``, ``host_reads``

    Returns a real tensor ``(*BA,)``.  Domain errors, gradients and refusals: as in ``quadform``.
    """
    _refuse_grad("trace_fn", A, probes)
    return _trace_fn("trace_fn", A, fn, probes, nsteps, seed, options)[0]


def logdet(A, probes=32, nsteps=None, seed=0, bck_options={}, **options):
    r"""
    :math:`\log\det\mathbf{A}` of a Hermitian positive definite operator as ``trace_fn(A, "log", ...)``,
    differentiable with respect to the operator's parameters.

    Arguments: those of ``trace_fn``, and ``bck_options``: the options of the one ``solve(A, Z)`` of the backward
    pass (default ``method="cg"``; ``precond=`` passes through, so ``"fsai"`` works on a CSR operator).

    The backward is implicit, with no graph through the iteration:
    :math:`d \log\det\mathbf{A} = \mathrm{tr}(\mathbf{A}^{-1} d\mathbf{A}) \approx \frac{1}{p} \sum_j
    (\mathbf{A}^{-1} z_j)^H\, d\mathbf{A}\, z_j` on the SAME probes: one ``solve`` under ``no_grad`` and one VJP of
    ``A.mm(Z)`` with the cotangent :math:`\bar g\,\mathbf{A}^{-1} Z / p`.  This is an unbiased estimate of the TRUE
    gradient, not the derivative of the forward estimate; the two coincide when :math:`Z Z^H = p I`.
    """
    assert_runtime(not torch.is_grad_enabled() or A.is_getparamnames_implemented,
                   "The _getparamnames(self, prefix) of linear operator A must be "
                   "implemented if using logdet with grad enabled")
    host_slq.check_options("logdet", A, "log", nsteps, options)
    params = A.getlinopparams()
    return _LogdetFunction.apply(A, probes, nsteps, seed, options, bck_options, *params)


class _LogdetFunction(torch.autograd.Function):
    """Forward: the Hutchinson estimate, graph-free.  Backward: X = A^-1 Z by one solve, then the VJP of A.mm(Z) with
    the cotangent g X / p (see `logdet`)."""

    @staticmethod
    def forward(ctx, A, probes, nsteps, seed, options, bck_options, *params):
        ctx.bck_config = merge_options({"method": "cg"}, bck_options)
        with A.uselinopparams(*params):
            est, Z = _trace_fn("logdet", A, "log", probes, nsteps, seed, dict(options))
        ctx.A = A
        ctx.save_for_backward(Z, *params)
        return est

    @staticmethod
    def backward(ctx, g):
        from xitorch_amd.linalg.solve import solve
        Z = ctx.saved_tensors[0]
        params = ctx.saved_tensors[1:]
        A, cfg = ctx.A, dict(ctx.bck_config)
        p = Z.shape[-1]
        with torch.no_grad(), A.uselinopparams(*params):
            X = solve(A, Z, **cfg)                                     # (*BA, n, p)
        cot = X * (g.to(X.dtype)[..., None, None] / p)
        grad_params = [None] * len(params)
        if params:
            with torch.enable_grad():
                ps = [p_.clone().requires_grad_() for p_ in params]
                with A.uselinopparams(*ps):
                    out = A.mm(Z.detach())
            grad_params = torch.autograd.grad([out], ps, grad_outputs=[cot.detach().expand_as(out)], allow_unused=True)
        return (None, None, None, None, None, None, *grad_params)
