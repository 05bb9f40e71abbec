"""funm_multiply, expm_multiply — the action f(A) B of a function of a Hermitian LinearOperator on a block of vectors:
A^{1/2} z, A^{-1/2} b, exp(-t A) b, exp(-i t H) psi, on dense, banded, CSR and matrix-free operators.

An extension (the reference has none of them).  The method is Lanczos-FA, f(A) b ~ |b| V_m f(T_m) e_1 (Druskin &
Knizhnerman 1989; its finite-precision behaviour: Musco, Musco & Sidford 2018), in its two-pass form: the basis V_m is
never stored, the recurrence is run a second time to accumulate the result, so storage is five vectors per column
whatever the step count and a call costs 2 nsteps - 1 operator applies.  Device operators run on the HIP kernels of
xk_slq.hip and xk_fnm.hip (`native_fnm.funm`), operators in host memory on the same iteration in torch ops
(`host_slq.funm`).

Convergence is that of the best polynomial approximation of f of degree nsteps - 1 on the spectrum, NOT the squared
rate the quadrature of `quadform` enjoys: with condition number 4, 24 steps give 1e-12 for sqrt, invsqrt, inv, log and
exp; with 100, 32 steps give 4e-7 for sqrt and 2e-4 for inv; with 1e4, 60 steps leave inv at 0.3.  `rtol=` asks for a
warning from the size of the last coefficients.
"""
import warnings
import torch
from xitorch_amd._util import MathWarning, assert_runtime
from xitorch_amd.linalg import host_slq

__all__ = ["funm_multiply", "expm_multiply"]


def _funm(A, B, opt):
    """device dispatch: host memory -> host_slq, everything else -> the HIP kernels"""
    from xitorch_amd.linalg import native_fnm
    if torch.device(A.device).type == "cpu":
        return host_slq.funm(A, B, opt)
    return native_fnm.funm(A, B, opt)


def _refuse_grad(who, A):
    if torch.is_grad_enabled() and any(p.requires_grad for p in A.getlinopparams()):
        raise NotImplementedError("%s is differentiable with respect to B only: the operator's parameters require "
                                  "grad; call it under torch.no_grad() or detach the parameters" % who)


def _conj_fn(fn):
    """the function of the backward pass: f(A)^H = conj(f)(A) for a Hermitian A"""
    if not callable(fn):
        return fn                                                      # the named functions are real
    return lambda x: torch.conj(fn(x)).resolve_conj()


def _run(who, A, B, opt):
    """f(A) B and the ONE host read of a call: flagged members, step counts, tails"""
    X, flag, m, tail, napply = _funm(A, B, opt)
    # per batch member, as quadform; the two causes apart: bit 0 a node <= 0 under a positivity function, bit 1 the
    # eigensolver of the small matrix did not converge
    domm, qlm = ((flag & 1) != 0).any(-1), ((flag & 2) != 0).any(-1)
    X = torch.where((domm | qlm)[..., None, None], torch.full_like(X, float("nan")), X)
    nsys = m.numel()
    summary = torch.cat([domm.sum().reshape(1).to(torch.float64), qlm.sum().reshape(1).to(torch.float64),
                         m.reshape(-1).to(torch.float64), tail.reshape(-1).to(torch.float64)]).tolist()   # the one read
    ndom, nql = int(summary[0]), int(summary[1])
    used = torch.tensor(summary[2:2 + nsys], dtype=torch.float64).to(torch.int64).reshape(m.shape)
    tails = torch.tensor(summary[2 + nsys:], dtype=torch.float64).reshape(m.shape)
    # (the drivers report 0 where there are no more than four coefficients; those four are then the whole result)
    tails = torch.where((used > 0) & (used <= 4), torch.ones_like(tails), tails)
    if ndom:
        warnings.warn(MathWarning("%s: %d member(s) are not numerically positive definite (a node of the Lanczos "
                                  "matrix <= 0 under fn='%s'): their result is NaN" % (who, ndom, opt["fn"])))
    if nql:
        warnings.warn(MathWarning("%s: the eigensolver of the Lanczos matrix of %d member(s) did not converge: "
                                  "their result is NaN" % (who, nql)))
    n, ns = A.shape[-1], opt["nsteps"]
    if opt["rtol"] is not None and ns < n:
        # a column that stopped early (breakdown) or ran m = n steps is exact, whatever its tail
        late = int(((used == ns) & (tails > opt["rtol"])).sum())
        if late:
            warnings.warn(MathWarning("%s: %d column(s) have not converged in %d Lanczos steps (the last four "
                                      "coefficients carry more than rtol = %g of the result): raise nsteps"
                                      % (who, late, ns, opt["rtol"])))
    return X, dict(nsteps=used, napply=napply, tail=tails)


class _FunmFunction(torch.autograd.Function):
    """Forward: f(A) B, graph-free.  Backward: f(A) is linear in B, so the cotangent of B is conj(f)(A) applied to the
    cotangent of the result: one more call."""

    @staticmethod
    def forward(ctx, A, B, opt, who):
        ctx.A, ctx.opt, ctx.who, ctx.bshape = A, opt, who, B.shape
        with torch.no_grad():
            X, info = _run(who, A, B, opt)
        if opt["trace"] is not None:
            opt["trace"].update(info)
        return X

    @staticmethod
    def backward(ctx, G):
        opt = dict(ctx.opt, fn=_conj_fn(ctx.opt["fn"]), trace=None, rtol=None)
        with torch.no_grad():
            gB, _ = _run(ctx.who, ctx.A, G, opt)
        extra = gB.dim() - len(ctx.bshape)                             # B was broadcast over A's batch: sum it back
        if extra > 0:
            gB = gB.sum(tuple(range(extra)))
        for i, sz in enumerate(ctx.bshape):
            if sz == 1 and gB.shape[i] != 1:
                gB = gB.sum(i, keepdim=True)
        return None, gB, None, None


def funm_multiply(A, B, fn, nsteps=None, t=1.0, rtol=None, trace=None, **options):
    r"""
    :math:`f(\mathbf{A})\,\mathbf{B}` for a Hermitian operator by ``nsteps`` steps of two-pass Lanczos.

    Arguments
    ---------
    A: LinearOperator ``(*BA, n, n)``, Hermitian (dense, banded, CSR or a user operator; float64, float32, complex128,
        complex64)
    B: torch.Tensor ``(*BB, n, p)``
    fn: str or callable
        ``"log"``, ``"inv"``, ``"sqrt"``, ``"invsqrt"``, ``"exp"`` (``exp(t x)``) or ``"identity"``; a callable is
        applied in torch, on the operator's device, to the ``(S, nsteps)`` array of the nodes (``S`` systems: batch
        members times columns).  On a complex operator it may return complex values (``lambda x: torch.exp(-1j * x)``);
        on a real operator a complex result is refused: cast ``A``.
    nsteps: int or None
        Lanczos steps, default ``min(n, 50)``, at most 128.  The error falls like that of the best polynomial
        approximation of ``fn`` of degree ``nsteps - 1`` on the spectrum of ``A`` (not at the squared rate of
        ``quadform``): well-conditioned operators need a few dozen steps, ``inv`` at condition number 1e4 is not
        reached by 60.
    t: float
        the scale of ``fn="exp"``
    rtol: positive real number or None
        when given, one ``MathWarning`` counts the columns whose last four coefficients carry more than ``rtol`` of the
        result (columns that ran all ``nsteps < n`` steps only: after a breakdown or ``n`` steps the result is exact)
    trace: dict or None
        receives ``nsteps`` (per column), ``napply`` and ``tail``

    Returns ``(*BAB, n, p)`` in the operator's dtype.  ``"log"``, ``"inv"``, ``"sqrt"`` and ``"invsqrt"`` need every
    node of the Lanczos matrix to be positive: a batch member with a node ``<= 0`` returns ``NaN`` columns and one
    ``MathWarning`` names how many members are not numerically positive definite (members whose small eigenproblem
    did not converge are NaN too and get a ``MathWarning`` of their own).  Differentiable with respect to ``B``
    (the backward is one more call with the conjugated function); operator parameters that require grad, ``M=`` and
    ``process_group=`` are refused (``NotImplementedError``).
    """
    return _entry("funm_multiply", A, B, fn, nsteps, t, rtol, trace, options)


def expm_multiply(A, B, t=1.0, **kw):
    r""":math:`\exp(t\mathbf{A})\,\mathbf{B}`: ``funm_multiply(A, B, "exp", t=t, ...)``."""
    return _entry("expm_multiply", A, B, "exp", kw.pop("nsteps", None), t, kw.pop("rtol", None), kw.pop("trace", None),
                  kw)


def _entry(who, A, B, fn, nsteps, t, rtol, trace, options):
    unknown = [k for k in options if k not in ("M", "process_group")]
    if unknown:
        raise TypeError("%s: unknown option(s) %s" % (who, ", ".join(sorted(unknown))))
    if fn != "exp" and float(t) != 1.0:
        raise TypeError("%s: t belongs to fn='exp'" % who)
    opt = host_slq.check_options(who, A, fn, nsteps, dict(options, t=float(t) if fn == "exp" else None))
    if rtol is not None:
        try:
            ok = not isinstance(rtol, (bool, complex, torch.Tensor, str)) and float(rtol) > 0
        except (TypeError, ValueError):
            ok = False
        if not ok:
            raise ValueError("%s: rtol must be a positive real number or None, got %r" % (who, rtol))
        rtol = float(rtol)
    if trace is not None and not isinstance(trace, dict):
        raise TypeError("%s: trace must be a dict or None" % who)
    assert_runtime(B.dim() >= 2 and A.shape[-1] == B.shape[-2],
                   "Mismatch shape of A & B (A: %s, B: %s)" % (A.shape, B.shape))
    _refuse_grad(who, A)
    opt = dict(fn=opt["fn"], t=opt["t"], nsteps=opt["nsteps"], rtol=rtol, trace=trace)
    return _FunmFunction.apply(A, B.to(device=A.device, dtype=A.dtype), opt, who)
