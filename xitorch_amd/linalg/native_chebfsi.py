"""Chebyshev-filtered subspace iteration on the HIP kernels: `symeig(..., method="chebfsi")`.

An extension (the reference has no counterpart; Zhou, Saad, Tiago, Chelikowsky, J. Comput. Phys. 219 (2006) 172).
Block Davidson grows a basis and repeats a Rayleigh-Ritz over all of it every iteration; for MANY pairs of a large
operator that chain becomes the cost.  Here the block has a fixed width w = neig + nguard and an outer iteration is

  1. `degree` times: one operator-panel product on the whole block (`PanelOperator.apply`: the wide panel kernels) and
     one `xk_cheb_step` — the only pass over the block between two applies — on a ring of panels; the coefficient table
     of the whole filter is a handful of torch ops on (Bt,) device tensors, no step synchronises with the host;
  2. two passes of CholeskyQR on the filtered block (`xk_davidson_orth`; complex: `xk_herm_cholqr` in chunks of 32);
  3. one more apply, the Gram block Q^H A Q on K1, the native dense eigensolver on it (`native_partial_eigh`; complex:
     `xk_herm_eigh` up to 32 vectors, the library beyond), the rotation (`xk_ritz_residual` for the wanted columns, `xk_lincomb` for the guard columns), the
     a-posteriori guard max|X^H X - I| (`xk_ritz_guard`) and ONE host read of {max|resid|, Cholesky flag, guard} — plus
     the read of the dense eigensolver's self-check flags inside `native_partial_eigh` / `herm_partial_eigh` (one per
     call: one for real blocks and complex blocks up to 16 vectors, two and a seam test for complex blocks of 17 .. 32).

Storage: the Ritz block, the two ring panels, the product panel, the best block seen and a residual panel.  The spectral bounds come from
a short Lanczos run on the device (`xk_kry_dots` + `xk_cheb_step` as its three-term update).  `host_eig.chebfsi` is the
same algorithm in torch ops for operators in host memory.  Not built: an overlap operator M, batch sharding, locking of
converged columns.

`mode="nearest"` with `sigma=` (`_nearest`; Li, Xi, Vecharynski, Yang, Saad, SIAM J. Sci. Comput. 38 (2016) A2512) runs
the same outer iteration around a Jackson-damped Chebyshev band-pass centred on sigma: the filter is evaluated by
Clenshaw's recurrence, one `xk_cheb_clenshaw` between two applies, on the same five panels (the pre-filter block is the
X0 of every step: no accumulator panel); the Ritz pairs are ordered by |lambda - sigma| on the device; the degree of the
next filter is chosen from the block's Ritz values (one more host read per outer iteration).  DESIGN.md section 3.14.
"""
import warnings
from types import SimpleNamespace
import torch
from xitorch_amd import kernels as K
from xitorch_amd._util import ConvergenceWarning
from xitorch_amd.linalg._panel import PanelOperator, pad_len, batch_count, real_dtype, require_hip
from xitorch_amd.linalg._block import block_ops, native_partial_eigh, GUARD_BAD
from xitorch_amd.linalg.native_krylov import _Kry
from xitorch_amd.linalg import host_eig
from xitorch_amd.linalg.host_eig import (cheb_coefficients, cheb_default_nguard, chebwin_coefficients, chebwin_select,
                                         chebwin_sigma, chebwin_first_degree, chebwin_interval, chebwin_angle,
                                         chebwin_degree, chebwin_dref, CHEBWIN_FIRST_DEGREE)

__all__ = ["chebfsi"]


def _rayleigh_ritz(ops, Q, AQ, X, scratch, hstatus, neig, sign, sigma=None):
    """X <- the Ritz block of span(Q) ordered by sign * lambda ascending — with `sigma` (Bt,) (mode="nearest", sign =
    1) by |lambda - sigma| ascending, a permutation of the small device tensors; returns (lam (Bt, w) true eigenvalues
    in that order, mu = sign * lam (ascending), [max|resid| over the wanted columns, Cholesky flag, guard])"""
    w = ops.w
    T = ops.rr_matrix(Q, AQ, sign)                                       # T[b, i, c] = sign <Q_i, (A Q)_c>
    mu, Y = ops.eigh_lowest(T, w, w)                                     # (Bt, w), (Bt, w, w) = [basis index, pair]
    lam = (mu * sign).contiguous()
    if sigma is not None:
        sel = chebwin_select(lam, sigma)
        lam = torch.gather(lam, -1, sel).contiguous()
        Y = torch.gather(Y, -1, sel.unsqueeze(-2).expand_as(Y)).contiguous()
    if hstatus is None:
        ops.rmax.zero_()
        K.ritz_residual(Q, AQ, Y, lam, X, scratch, ops.rmax, w, neig)
    else:
        K.herm_ritz(Q, AQ, Y, lam, X, scratch, hstatus, w, neig)
    if w > neig:
        ops.combine(Q, Y[:, :, neig:], out=X[:, neig:])                  # the guard columns
    # the one host read of the outer iteration
    return lam, mu, ops.status(X, w, None if hstatus is None else hstatus[0], ops.info)


def _lanczos_bounds(op, Bt, N, dtype, device, bdims, steps, sign):
    """Ritz values and residual norm of a `steps`-step Lanczos run from one random vector per operator, all on the
    device: apply, xk_kry_dots for <v, A v> and |f|^2, xk_cheb_step for f = A v - alpha v - beta v_prev and for the
    normalisation.  Returns (theta (Bt, steps) of sign * A ascending, |f_k| (Bt,)) as float64 device tensors."""
    ld = pad_len(N)
    kr = _Kry(SimpleNamespace(S=Bt, N=N, ld=ld, dtype=dtype, device=device))

    def dot(x, y):
        P = kr.partial()
        kr.dots(x, y, P)
        P = P[:, :kr.nblk, 0] if kr.cplx else P[:, :kr.nblk]
        return P.to(torch.float64).sum(dim=1)

    bufs = [torch.zeros((Bt, 1, ld), dtype=dtype, device=device) for _ in range(3)]
    v0 = host_eig._cheb_lanczos_vector(bdims, N, dtype).reshape(Bt, N).to(device)
    v0 = v0 / torch.linalg.vector_norm(v0, dim=-1, keepdim=True)
    bufs[0][:, 0, :N].copy_(v0)
    v, vprev, av = bufs
    zero = torch.zeros((Bt,), dtype=torch.float64, device=device)
    one = torch.ones_like(zero)
    beta = zero
    alphas, betas = [], []
    for j in range(steps):
        op.apply(v, av)
        al = dot(v, av)
        K.cheb_step(av, v, vprev, torch.stack((one, -al, -beta), dim=-1).contiguous(), N=N)     # f, over v_prev
        f = vprev
        beta = torch.sqrt(torch.clamp(dot(f, f), min=0.0))
        alphas.append(al)
        if j + 1 < steps:
            betas.append(beta)
            inv = torch.where(beta > 0, 1.0 / beta, zero)
            K.cheb_step(v, f, av, torch.stack((zero, inv, zero), dim=-1).contiguous(), N=N)      # f / beta, over A v
            v, vprev, av = av, v, f
    Tl = torch.diag_embed(torch.stack(alphas, dim=-1))
    if betas:
        off = torch.stack(betas, dim=-1)
        Tl = Tl + torch.diag_embed(off, offset=1) + torch.diag_embed(off, offset=-1)
    Tl = (Tl * sign).contiguous()
    if steps <= K.SMALL_EIGH_MAX_P:
        theta, _, _ = K.small_eigh(Tl, steps, steps)
    else:
        theta, _ = native_partial_eigh(Tl, steps, "lowest")
    return theta, beta


def _nearest(ops, op, hstatus, orth, panels, Tn, theta, fnorm, sigma, neig, w, N, bdims, rdt, max_niter, min_eps,
             filter_degree, max_degree, filter_tail, verbose, trace):
    """mode="nearest" on the five panels of `chebfsi`: see `host_eig._chebfsi_nearest`, whose decisions these are.  Per
    filter of degree m: b_m = c_m X by one `xk_cheb_step`, then m times [apply, `xk_cheb_clenshaw`] on a ring of two
    panels with the pre-filter block X as the X0 of every step; the coefficient table and the degree rule are torch ops
    on (Bt,) device tensors."""
    X, R0, R1, AY, best_X = panels
    theta = theta.to(torch.float64)
    emin, emax = theta.min(dim=-1)[0], theta.max(dim=-1)[0]
    lo, hi = emin - fnorm, emax + fnorm
    deg_now, fixed = chebwin_first_degree(filter_degree, max_degree)
    capped = (not fixed) and deg_now == int(max_degree) and deg_now < CHEBWIN_FIRST_DEGREE
    gbad = GUARD_BAD[rdt]
    best_resid, best_lam = float("inf"), None
    history, redo, degrees = [], [], []
    niter, passes, halved = 0, 2, False
    for it in range(max_niter):
        niter = it + 1
        sigma_c = torch.minimum(torch.maximum(sigma, emin), emax)
        while True:
            coef = chebwin_coefficients(lo, hi, sigma_c, deg_now).contiguous()           # (degree + 1, Bt, 4)
            # ring: b_{k+2} is overwritten by b_k; the pre-filter block X is the X0 of every step and is kept
            K.cheb_step(X, X, R0, coef[0, :, :3].contiguous(), out=R0, N=N)              # b_m = c_m X (R0 is not read)
            Yp, Y = R1, R0
            for j in range(1, deg_now + 1):
                op.apply(Y, AY)
                K.cheb_clenshaw(AY, Y, Yp, X, coef[j], N=N)                              # row 1: gamma = 0, Yp not read
                Yp, Y = Y, Yp
            Q, other = Y, Yp                                                             # p(A) X, and b_1 (dead)
            orth(Q, passes)
            op.apply(Q, AY)
            lam, _mu, (max_resid, chol_flag, guard) = _rayleigh_ritz(ops, Q, AY, other, Tn, hstatus, neig, 1.0, sigma)
            if guard != guard:
                guard = float("inf")
            if chol_flag == 0 and guard <= gbad:
                break
            redo.append({"iter": niter, "guard": guard, "chol_flag": chol_flag, "passes": 3,
                         "degree": max(1, deg_now // 2)})
            if len(redo) > 1:
                raise RuntimeError("xitorch_amd chebfsi: the filtered block lost its orthonormality twice (max|X^H X - "
                                   "I| = %.2e, Cholesky flag %d, at iteration %d)" % (guard, int(chol_flag), niter))
            passes, deg_now, halved = 3, max(1, deg_now // 2), True
        # the new Ritz block lives in `other`: it becomes X; the old X and Q are the ring of the next filter
        X, R0, R1 = other, X, Q
        degrees.append(deg_now)
        if max_resid != max_resid:
            max_resid = float("inf")
        history.append(max_resid)
        if verbose:
            print("Iter %3d (block of %d, degree %d): resid: %.3e" % (niter, w, deg_now, max_resid))
        if max_resid < best_resid:
            best_resid, best_lam = max_resid, lam[:, :neig]
            best_X.copy_(X)
        if max_resid < min_eps:
            break
        lam64 = lam.to(torch.float64)
        emin, emax = torch.minimum(emin, lam64.min(dim=-1)[0]), torch.maximum(emax, lam64.max(dim=-1)[0])
        lo, hi = torch.minimum(lo, emin), torch.maximum(hi, emax)
        if not fixed:
            c, e, _flat = chebwin_interval(lo, hi)
            theta_s = chebwin_angle(torch.minimum(torch.maximum(sigma, emin), emax), c, e)
            deg_now, capped = chebwin_degree(theta_s, chebwin_dref(lam64, theta_s, c, e, neig, w), filter_tail,
                                             max_degree)                                 # the one extra host read
            if halved:
                deg_now = max(1, deg_now // 2)
    if best_lam is None:
        raise RuntimeError("xitorch_amd chebfsi: no finite residual was produced")
    if not best_resid < min_eps:
        warnings.warn(ConvergenceWarning("chebfsi: convergence is not achieved after %d iterations (max |resid| = %.3e "
                                         ">= min_eps = %.3e); the best block is returned" % (niter, best_resid, min_eps)))
    if trace is not None:
        trace.update(niter=niter, napply=op.napply, degree=degrees[-1], degrees=degrees, w=w, resid_history=history,
                     best_resid=best_resid, sigma_centre=sigma_c.reshape(tuple(bdims)).tolist(), degree_capped=bool(capped),
                     bounds={k: v.reshape(tuple(bdims)).tolist() for k, v in (("lo", lo), ("hi", hi), ("emin", emin),
                                                                        ("emax", emax))},
                     small_eigh=ops.small_eigh, guard_redo=redo,
                     panel_kernel=op.last_kernel if op.kind != "generic" else "generic")
    order = torch.argsort(best_lam, dim=-1)                                              # ascending, like every mode
    evals = torch.gather(best_lam, -1, order).reshape(*bdims, neig)
    evecs = ops.result(best_X, neig, bdims)
    return evals, torch.gather(evecs, -1, order.reshape(*bdims, 1, neig).expand_as(evecs))


def chebfsi(A, neig, mode, M=None, max_niter=100, min_eps=1e-6, degree=12, nguard=None, V0=None, v_init="randn",
            rng_device="cpu", lanczos_steps=12, verbose=False, trace=None, process_group=None, sigma=None,
            filter_degree=None, max_degree=1000, filter_tail=0.1, **unused):
    """
    Chebyshev-filtered subspace iteration for the ``neig`` lowest / uppermost eigenpairs of a large Hermitian operator
    (dense, banded, CSR or a user ``_mv``; float64, float32, complex128, complex64; any batch shape), on the HIP kernels.
    Meant for MANY pairs (32 .. 256), where block Davidson's Rayleigh-Ritz chain over a growing basis is the cost.

    Keyword arguments
    -----------------
    max_niter: int
        Maximum number of outer iterations (each: ``degree + 1`` operator applies on the whole block)
    min_eps: float
        Stop when the largest residual element ``max|A X - X diag(lam)|`` over the wanted columns of all operators is
        below this (davidson's rule); otherwise the best block seen is returned with a ``ConvergenceWarning``
    degree: int
        Degree of the Chebyshev filter (``"lowest"`` / ``"uppest"``; not used by ``"nearest"``)
    sigma: number or real tensor broadcastable to the batch dimensions
        ``mode="nearest"``: the ``neig`` pairs nearest ``sigma`` (no gradient flows to it).  The filter is the
        Jackson-damped Chebyshev expansion of a delta function (Li, Xi, Vecharynski, Yang, Saad, SISC 2016), centred on
        ``sigma`` clipped to the Ritz extremes seen so far and evaluated by Clenshaw's recurrence: per filter ``m``
        applies and ``m`` streaming passes (one ``xk_cheb_step``, ``m`` ``xk_cheb_clenshaw``), no accumulator panel
    filter_degree: int or None
        ``mode="nearest"``: ``None`` = the first filter has degree 20 and after every Rayleigh-Ritz the smallest degree
        of the ladder 8, 11, 14, 18, ... whose filter has fallen to ``filter_tail`` at the angular distance of the
        ``(neig + ceil(nguard / 2))``-th nearest Ritz value is taken (one more host read per outer iteration, of that
        integer); an int fixes the degree
    max_degree, filter_tail: int, float
        ``mode="nearest"``: the cap of the ladder (reported in ``trace["degree_capped"]``) and the tail level
    nguard: int or None
        Guard vectors: the block has ``neig + nguard`` columns.  Default ``max(8, ceil(neig / 4))``, capped at the order
    V0: tensor or None
        Start block ``(*batch, na, k)``; completed by random columns when ``k < neig + nguard``
    v_init, rng_device: str
        The start block, as for ``davidson`` (seed 12421)
    lanczos_steps: int
        Steps of the Lanczos run that estimates the spectral bounds (upper bound ``theta_max + |f_k|``)
    trace: dict or None
        Receives ``niter``, ``napply``, ``degree``, ``w``, ``bounds``, ``small_eigh`` (``"native"`` / ``"library"``),
        ``guard_redo``, ``panel_kernel``, ``resid_history``; ``mode="nearest"`` adds ``degrees`` (per outer
        iteration), ``sigma_centre``, ``degree_capped`` and ``bounds`` = ``lo, hi, emin, emax``

    ``M`` and ``process_group`` raise ``NotImplementedError``.  ``mode="uppest"`` filters ``-A`` by negating the
    coefficients.  A block wide enough to span (half of) the space is handed to ``exacteig``.  A block that fails the
    a-posteriori guard ``max|X^H X - I| > GUARD_BAD`` is redone from the pre-filter block with a third orthonormalisation
    pass and half the degree, and both stay in force for the rest of the run (a block that lost its orthonormality once
    is not given the longer filter again); a second failure raises.
    """
    from xitorch_amd.linalg.native_eig import exacteig
    device = torch.device(A.device)
    if device.type == "cpu":
        # device dispatch (see native_eig.davidson): an operator in HOST memory is served by host_eig.py
        return host_eig.chebfsi(A, neig, mode, M, max_niter=max_niter, min_eps=min_eps, degree=degree, nguard=nguard,
                                V0=V0, v_init=v_init, rng_device=rng_device, lanczos_steps=lanczos_steps,
                                verbose=verbose, trace=trace, process_group=process_group, sigma=sigma,
                                filter_degree=filter_degree, max_degree=max_degree, filter_tail=filter_tail)
    host_eig._cheb_check_args("chebfsi", M, process_group)
    require_hip(A, "chebfsi")
    dtype = A.dtype
    N = A.shape[-1]
    bdims = list(A.shape[:-2])
    Bt = batch_count(bdims)
    if nguard is None:
        nguard = cheb_default_nguard(neig, N)
    w = min(N, neig + int(nguard))
    if V0 is not None and w < V0.shape[-1]:
        w = min(N, V0.shape[-1])
    nearest = mode == "nearest"
    if nearest:
        sigma = chebwin_sigma(sigma, bdims, device)
    if N <= max(2 * w, 16):
        if trace is not None:
            trace.update(niter=0, napply=0, degree=degree, w=w, handed_to="exacteig")
        return exacteig(A, neig, mode, None, sigma=sigma) if nearest else exacteig(A, neig, mode, None)
    sign = 1.0 if mode == "lowest" or nearest else -1.0
    rdt = real_dtype(dtype)
    ops = block_ops(Bt, N, w, dtype, device, wide=True)
    hstatus = torch.zeros((Bt + 1,), dtype=torch.float64, device=device) if dtype.is_complex else None   # xk_herm_ritz
    op = PanelOperator(A, bdims, Bt, N)
    if trace is not None and trace.get("k1_events") is not None:
        op.events = trace["k1_events"]

    def orth(P, passes):
        # two passes of CholeskyQR (the first shifted); complex blocks in chunks of xk_herm_cholqr's 32 vectors
        ops.info.zero_()
        ops.orth(P, 0, w, passes, ops.info, chunk=K.HERM_CHOLQR_MAX_Q)

    X, R0, R1, AY, best_X = (ops.panel(w) for _ in range(5))
    Tn = ops.panel(w)[:, :neig]                      # residual panel xk_ritz_residual writes beside the wanted columns
    ops.load(X, host_eig._cheb_start_block(v_init, V0, bdims, Bt, N, w, dtype, device, rng_device))
    orth(X, 2)
    if int(ops.info.max().item()) != 0:
        raise RuntimeError("chebfsi: the start block is rank deficient (linearly dependent start vectors)")

    ks = max(2, min(int(lanczos_steps), N - 1))
    theta, fnorm = _lanczos_bounds(op, Bt, N, dtype, device, bdims, ks, sign)
    if nearest:
        return _nearest(ops, op, hstatus, orth, (X, R0, R1, AY, best_X), Tn, theta, fnorm, sigma.reshape(Bt), neig, w, N,
                        bdims, rdt, max_niter, min_eps, filter_degree, max_degree, filter_tail, verbose, trace)
    b_sup = theta.max(dim=-1)[0].to(torch.float64) + fnorm
    a0 = theta.min(dim=-1)[0].to(torch.float64)
    a = theta.to(torch.float64).median(dim=-1)[0]

    gbad = GUARD_BAD[rdt]
    best_resid, best_lam = float("inf"), None
    history, redo = [], []
    niter, deg_now, passes = 0, int(degree), 2
    for it in range(max_niter):
        niter = it + 1
        while True:
            coef = cheb_coefficients(a, b_sup, a0, deg_now, sign).contiguous()           # (degree, Bt, 3) on the device
            # ring: Y_{i-2} is overwritten by Y_i; the pre-filter block X is kept (a guard failure restarts from it)
            Yp, Y, free = X, X, [R0, R1]
            for i in range(deg_now):
                op.apply(Y, AY)
                if i == 0:
                    out = free.pop()
                    K.cheb_step(AY, Y, out, coef[0], out=out, N=N)                       # gamma = 0: out is not read
                elif i == 1:
                    out = free.pop()
                    K.cheb_step(AY, Y, Yp, coef[1], out=out, N=N)
                else:
                    out = Yp
                    K.cheb_step(AY, Y, Yp, coef[i], N=N)
                Yp, Y = Y, out
            Q = Y
            other = R1 if Q is R0 else R0                                                # Y_{m-1} (dead) or unused
            orth(Q, passes)
            op.apply(Q, AY)
            lam, mu, (max_resid, chol_flag, guard) = _rayleigh_ritz(ops, Q, AY, other, Tn, hstatus, neig, sign)
            if guard != guard:
                guard = float("inf")
            if chol_flag == 0 and guard <= gbad:
                break
            redo.append({"iter": niter, "guard": guard, "chol_flag": chol_flag, "passes": 3,
                         "degree": max(1, deg_now // 2)})
            if len(redo) > 1:
                raise RuntimeError("xitorch_amd chebfsi: the filtered block lost its orthonormality twice (max|X^H X - "
                                   "I| = %.2e, Cholesky flag %d, at iteration %d)" % (guard, int(chol_flag), niter))
            passes, deg_now = 3, max(1, deg_now // 2)
        # the new Ritz block lives in `other`: it becomes X; the old X and Q are the ring of the next filter
        X, R0, R1 = other, X, Q
        if max_resid != max_resid:
            max_resid = float("inf")
        history.append(max_resid)
        if verbose:
            print("Iter %3d (block of %d, degree %d): resid: %.3e" % (niter, w, deg_now, max_resid))
        if max_resid < best_resid:
            best_resid, best_lam = max_resid, lam[:, :neig]
            best_X.copy_(X)
        if max_resid < min_eps:
            break
        a, a0 = mu.max(dim=-1)[0].to(torch.float64), mu.min(dim=-1)[0].to(torch.float64)
    if best_lam is None:
        raise RuntimeError("xitorch_amd chebfsi: no finite residual was produced")
    if not best_resid < min_eps:
        warnings.warn(ConvergenceWarning("chebfsi: convergence is not achieved after %d iterations (max |resid| = %.3e "
                                         ">= min_eps = %.3e); the best block is returned" % (niter, best_resid, min_eps)))
    if trace is not None:
        trace.update(niter=niter, napply=op.napply, degree=deg_now, w=w, resid_history=history, best_resid=best_resid,
                     bounds={"a": a.tolist(), "b_sup": b_sup.tolist(), "a0": a0.tolist()},
                     small_eigh=ops.small_eigh, guard_redo=redo,
                     panel_kernel=op.last_kernel if op.kind != "generic" else "generic")
    evals = best_lam.reshape(*bdims, neig)
    evecs = ops.result(best_X, neig, bdims)
    if mode != "lowest":
        evals, evecs = evals.flip(-1), evecs.flip(-1)
    return evals, evecs
