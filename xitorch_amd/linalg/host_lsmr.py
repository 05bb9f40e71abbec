"""LSMR (Fong & Saunders 2011) in host memory: the iteration of `native_lsmr.lsmr` in torch ops, for operators whose
tensors live on the CPU.  Device operators never reach this module (`calls` counts the entries; the GPU tests assert
that it stays 0).

The recurrence is the normalised textbook one (u, v of unit length), all scalars float64 `(*batch, 1, ncols)`; systems
that stopped are frozen by masks.  Options, stopping rules S1 / S2 / S3, the confirmation of the returned iterate on
the true `A^H (b - A x) - damp^2 x` and `b - A x`, the at most `max_restart` resumptions on the correction equation and
the warnings are those of the native driver.  `|x|` of the S1 test is the norm of the iterate itself (the kernels use
that of the step before).
"""
import warnings
import torch
from xitorch_amd._util import ConvergenceWarning, bcast_shape

__all__ = ["lsmr", "lsmr_stacked", "stacked_shape", "check_lsmr_options", "calls"]

calls = {"lsmr": 0}


def check_lsmr_options(A, B, damp, options, shape=None):
    """argument checks shared by the host and the native driver; returns the options with their defaults.  shape: (m, n)
    of the operator really iterated on (the stacked ones of the backward), default that of A"""
    known = ("max_niter", "atol", "btol", "conlim", "resid_calc_every", "verbose", "max_restart", "trace")
    for name, what in (("process_group", "batch sharding (process_group=)"), ("E", "a shift E="), ("M", "a metric M="),
                       ("precond", "a preconditioner (precond=)"), ("precond_l", "a preconditioner (precond_l=)"),
                       ("precond_r", "a preconditioner (precond_r=)"), ("x0", "a warm start (x0=)")):
        if options.get(name) is not None:
            raise NotImplementedError("lstsq: %s is not supported by lsmr" % what)
    unknown = [k for k in options if k not in known and options[k] is not None]
    if unknown:
        raise TypeError("lstsq: unknown option(s) %s" % ", ".join(sorted(unknown)))
    if isinstance(damp, torch.Tensor) or not isinstance(damp, (int, float)) or isinstance(damp, bool) or not damp >= 0:
        raise ValueError("lstsq: damp must be a non-negative Python float, got %r" % (damp,))
    m, n = (A.shape[-2], A.shape[-1]) if shape is None else shape
    if m != B.shape[-2]:
        raise RuntimeError("Mismatch shape of A & B (A: %s, B: %s)" % (tuple(A.shape), tuple(B.shape)))
    opt = dict(max_niter=options.get("max_niter"), atol=options.get("atol", 1e-6), btol=options.get("btol", 1e-6),
               conlim=options.get("conlim", 1e8), resid_calc_every=options.get("resid_calc_every", 10),
               verbose=bool(options.get("verbose", False)), max_restart=options.get("max_restart", 2),
               trace=options.get("trace"))
    if opt["max_niter"] is None:
        opt["max_niter"] = 4 * min(m, n)
    for k, default in (("atol", 1e-6), ("btol", 1e-6), ("conlim", 1e8)):
        opt[k] = float(default if opt[k] is None else opt[k])
    opt["resid_calc_every"] = max(1, int(opt["resid_calc_every"] or 10))
    opt["max_restart"] = 2 if opt["max_restart"] is None else int(opt["max_restart"])
    return opt


def _nrm(t):
    return torch.linalg.vector_norm(t, dim=-2, keepdim=True).to(torch.float64)


def _div(a, d):
    one = torch.ones_like(d)
    return torch.where(d == 0, torch.zeros_like(d), a / torch.where(d == 0, one, d))


def _rot(a, b):
    """(c, s, r) of the plane rotation with r = sqrt(a^2 + b^2); r = 0: the identity"""
    r = torch.sqrt(a * a + b * b)
    return torch.where(r == 0, torch.ones_like(r), _div(a, r)), _div(b, r), r


def _recurrence(fwd, adj, b, x, damp, atol, btol, conlim, nsteps, normb, code0=None):
    """LSMR on `min |fwd(dx) - b|^2 + damp^2 |dx|^2` added to x in place, at most nsteps steps.  code0: systems with
    a non-zero entry stay frozen.  Returns (code, est, steps): the stop codes (0 still running), the estimates
    {normr, normar, normA, condA} and the number of steps taken."""
    f64 = torch.float64
    rdt = x.real.dtype if x.is_complex() else x.dtype
    sc = lambda s: s.to(rdt)
    beta = _nrm(b)
    u = b * sc(_div(torch.ones_like(beta), beta))
    v = adj(u)
    alpha = _nrm(v)
    v = v * sc(_div(torch.ones_like(alpha), alpha))
    zero, one = torch.zeros_like(beta), torch.ones_like(beta)
    code = torch.where(beta == 0, one, torch.where(alpha == 0, 4 * one, zero))
    if code0 is not None:
        code = torch.where(code0 != 0, code0.to(f64), code)
    zetabar, alphabar = alpha * beta, alpha.clone()
    rho, rhobar, cbar, sbar, zeta = one.clone(), one.clone(), one.clone(), zero.clone(), zero.clone()
    betadd, betad, rhodold, tautildeold, thetatilde, d = beta.clone(), zero.clone(), one.clone(), zero.clone(), \
        zero.clone(), zero.clone()
    normA2, maxrbar, minrbar = alpha * alpha, zero.clone(), 1e100 * one
    est = dict(normr=beta.clone(), normar=alpha * beta, normA=alpha.clone(), condA=one.clone(), alpha1=alpha.clone(),
               maxrbar=zero.clone())
    h, hbar = v.clone(), torch.zeros_like(v)
    steps = 0
    for it in range(nsteps):
        live = code == 0
        if not bool(live.any()):
            break
        steps += 1
        u = fwd(v) - sc(alpha) * u
        beta = _nrm(u)
        u = u * sc(_div(one, beta))
        v = adj(u) - sc(beta) * v
        alpha = _nrm(v)
        v = v * sc(_div(one, alpha))
        chat, shat, alphahat = _rot(alphabar, damp * one)
        rhoold = rho
        c, s, rho = _rot(alphahat, beta)
        thetanew, alphabar_n = s * alpha, c * alpha
        rhobarold, zetaold, thetabar, rhotemp = rhobar, zeta, sbar * rho, cbar * rho
        cbar_n, sbar_n, rhobar = _rot(rhotemp, thetanew)
        zeta, zetabar_n = cbar_n * zetabar, -sbar_n * zetabar
        c1, c2, c3 = _div(thetabar * rho, rhoold * rhobarold), _div(zeta, rho * rhobar), _div(thetanew, rho)
        hbar_n = h - sc(c1) * hbar
        x_n = x + sc(c2) * hbar_n
        h_n = v - sc(c3) * h
        # |rbar|
        betaacute, betacheck = chat * betadd, -shat * betadd
        betahat, betadd_n = c * betaacute, -s * betaacute
        thetatildeold = thetatilde
        ctildeold, stildeold, rhotildeold = _rot(rhodold, thetabar)
        thetatilde_n, rhodold_n = stildeold * rhobar, ctildeold * rhobar
        betad_n = -stildeold * betad + ctildeold * betahat
        tautildeold_n = _div(zetaold - thetatildeold * tautildeold, rhotildeold)
        taud = _div(zeta - thetatilde_n * tautildeold_n, rhodold_n)
        d_n = d + betacheck * betacheck
        normr = torch.sqrt(d_n + (betad_n - taud) ** 2 + betadd_n * betadd_n)
        na2 = normA2 + beta * beta
        maxrbar_n = torch.maximum(maxrbar, rhobarold)
        # the Frobenius norm of the bidiagonal, capped by an estimate of |A|_2 (see xk_lsmr.hip)
        two = torch.sqrt(torch.clamp(maxrbar_n * maxrbar_n - damp * damp, min=0.0))
        normA = torch.minimum(torch.sqrt(na2), torch.maximum(two, est["alpha1"]))
        minrbar_n = torch.minimum(minrbar, rhobarold) if it >= 1 else minrbar
        condA = _div(torch.maximum(maxrbar_n, rhotemp), torch.minimum(minrbar_n, rhotemp))
        normar = zetabar_n.abs()
        normx = _nrm(x_n)
        new = zero.clone()
        new = torch.where(condA >= conlim, 3 * one, new)
        new = torch.where(normar <= atol * normA * normr, 2 * one, new)
        new = torch.where(normr <= btol * normb + atol * normA * normx, one, new)
        new = torch.where(alpha == 0, 4 * one, new)
        new = torch.where(beta == 0, 5 * one, new)
        L = live
        upd = lambda a, bnew: torch.where(L, bnew, a)
        hbar, h = upd(hbar, hbar_n), upd(h, h_n)
        x.copy_(upd(x, x_n))
        alphabar, zetabar, rhobar, cbar, sbar = upd(alphabar, alphabar_n), upd(zetabar, zetabar_n), \
            upd(rhobarold, rhobar), upd(cbar, cbar_n), upd(sbar, sbar_n)
        rho, zeta = upd(rhoold, rho), upd(zetaold, zeta)
        betadd, betad, rhodold, tautildeold, thetatilde, d = upd(betadd, betadd_n), upd(betad, betad_n), \
            upd(rhodold, rhodold_n), upd(tautildeold, tautildeold_n), upd(thetatildeold, thetatilde_n), upd(d, d_n)
        normA2, maxrbar, minrbar = upd(normA2, na2 + alpha * alpha), upd(maxrbar, maxrbar_n), upd(minrbar, minrbar_n)
        for name, val in (("normr", normr), ("normar", normar), ("normA", normA), ("condA", condA),
                          ("maxrbar", maxrbar_n)):
            est[name] = upd(est[name], val)
        code = upd(code, new)
    return code, est, steps


def _stacked(fwd, adj, m, damp):
    """[A; damp I] and its adjoint on (..., m + n, nc) / (..., n, nc) tensors"""
    def sf(v):
        return torch.cat([fwd(v), damp * v], dim=-2)

    def sa(u):
        return adj(u[..., :m, :]) + damp * u[..., m:, :]
    return sf, sa


def solve_with(fwd, adj, B, xshape, damp, opt, what="lsmr"):
    """the driver on closures `fwd` / `adj` (also the stacked operators of the lstsq backward)"""
    f64 = torch.float64
    atol, btol, conlim, max_niter = opt["atol"], opt["btol"], opt["conlim"], opt["max_niter"]
    m = B.shape[-2]
    x = torch.zeros(xshape, dtype=B.dtype, device=B.device)
    normb = _nrm(B)
    napply = [0]

    def cf(v):
        napply[0] += 1
        return fwd(v)

    def ca(u):
        napply[0] += 1
        return adj(u)

    code, est, niter = _recurrence(cf, ca, B, x, damp, atol, btol, conlim, max_niter, normb)
    restarts = 0
    normA = est["normA"]
    while True:
        r = B - cf(x)
        g = ca(r) - (damp * damp) * x
        nr, ng, nx = _nrm(r), _nrm(g), _nrm(x)
        nrbar = torch.sqrt(nr * nr + (damp * nx) ** 2)
        ok1 = nrbar <= 2 * (btol * normb + atol * normA * nx)
        ok2 = ng <= 2 * atol * normA * nrbar
        redo = ((code == 1) & ~ok1) | ((code == 2) & ~ok2)         # each member by the rule it stopped on
        if not bool(redo.any()) or restarts >= opt["max_restart"] or niter >= max_niter:
            break
        restarts += 1
        frozen = torch.where(redo, torch.zeros_like(code), torch.where(code == 0, 6 * torch.ones_like(code), code))
        if damp > 0:
            sf, sa = _stacked(cf, ca, m, damp)
            c2, e2, st = _recurrence(sf, sa, torch.cat([r, -damp * x], dim=-2), x, 0.0, atol, btol, conlim,
                                     max_niter - niter, normb, code0=frozen)
        else:
            c2, e2, st = _recurrence(cf, ca, r, x, 0.0, atol, btol, conlim, max_niter - niter, normb, code0=frozen)
        niter += st
        code = torch.where(redo, c2, code)
    nmax, ncon = int((code == 0).sum()), int((code == 3).sum())
    if nmax:
        warnings.warn(ConvergenceWarning("%s: %d system(s) did not meet atol = %.1e / btol = %.1e after %d iterations "
                                         "(max |A^H r - damp^2 x| = %.3e)" % (what, nmax, atol, btol, niter,
                                                                             float(ng.max()))))
    if ncon:
        warnings.warn(ConvergenceWarning("%s: %d system(s) stopped on cond(A) >= conlim = %.1e: the result is a "
                                         "regularised solution" % (what, ncon, conlim)))
    if opt.get("trace") is not None:
        opt["trace"].update(niter=niter, napply=napply[0], torch_applies=napply[0], host_reads=niter + 1 + restarts,
                            restarts=restarts, stop_codes=code.reshape(-1).to(torch.int64).tolist())
    if opt["verbose"]:
        print("%s: %d iterations, %d restarts, stop codes %s" % (what, niter, restarts,
                                                                 code.reshape(-1).to(torch.int64).tolist()))
    return x


def lsmr(A, B, damp=0.0, **options):
    """`lstsq(A, B, damp)` for an operator in host memory; see `native_lsmr.lsmr` for the options"""
    calls["lsmr"] += 1
    opt = check_lsmr_options(A, B, damp, options)
    bdims = bcast_shape(A.shape[:-2], B.shape[:-2])
    m, n, nc = A.shape[-2], A.shape[-1], B.shape[-1]
    B = B.to(A.dtype).expand(*bdims, m, nc)
    if torch.allclose(B, B * 0):
        return torch.zeros((*bdims, n, nc), dtype=A.dtype, device=B.device)
    return solve_with(A.mm, A.rmm, B, (*bdims, n, nc), float(damp), opt)


def stacked_shape(A, damp, stack):
    """(m, n) of the operator `stack` names: "A" -> [A; damp I], "AH" -> its adjoint (damp = 0: A and A^H themselves)"""
    m, n = A.shape[-2], A.shape[-1]
    rows = m + n if damp > 0 else m
    return (rows, n) if stack == "A" else (n, rows)


def lsmr_stacked(A, B, damp, stack, **options):
    """zero-damping LSMR on the stacked operator Abar = [A; damp I] ("A") or on Abar^H ("AH"): the solves of the
    lstsq backward"""
    calls["lsmr"] += 1
    mm, nn = stacked_shape(A, damp, stack)
    opt = check_lsmr_options(A, B, damp, options, shape=(mm, nn))
    bdims = bcast_shape(A.shape[:-2], B.shape[:-2])
    nc = B.shape[-1]
    B = B.to(A.dtype).expand(*bdims, mm, nc)
    if torch.allclose(B, B * 0):
        return torch.zeros((*bdims, nn, nc), dtype=A.dtype, device=B.device)
    fwd, adj = A.mm, A.rmm
    if damp > 0:
        fwd, adj = _stacked(A.mm, A.rmm, A.shape[-2], damp)
    if stack == "AH":
        fwd, adj = adj, fwd
    return solve_with(fwd, adj, B, (*bdims, nn, nc), 0.0, opt)
