"""LSMR on the HIP kernels of xk_lsmr.hip: `lstsq(A, B, damp)` for rectangular operators on a device.

An extension (the reference has no lstsq; Fong & Saunders, SIAM J. Sci. Comput. 33 (2011) 2950).  Every (batch member,
column) pair is one system; all S = Bt * ncols systems advance in lock step on (Bt, ncols, ld) panels, the u side of
length m and the v side of length n.  One step:

  apply A   on vh   -> xk_lsmr_bidiag (u half): uh <- A vh / alpha - (alpha / beta) uh, partials of |uh|^2
  apply A^H on uh   -> xk_lsmr_bidiag (v half): vh <- A^H uh / beta' - (beta' / alpha) vh, partials of |vh|^2
  xk_lsmr_update: the rotations, hbar, x, h in one pass, the estimates and the per-system stop code

The applies are those of `RectPanelOperator` (dense, CSR, banded natively; the operator's own .mm / .rmm otherwise).  The
host reads ONE word (the number of running systems, xk_kry_status on the kernels' run flags) every `resid_calc_every`
steps and nothing else.  When no system runs (or max_niter is reached) the returned iterate is confirmed by one true
evaluation of b - A x and A^H (b - A x) - damp^2 x (xk_kry_resid on the applies); members that stopped on S1 or S2 but
miss that rule by more than the factor 2 are resumed, at most `max_restart` times, on the correction equation
min |Abar dx - rbar| with Abar = [A; damp I], rbar = [b - A x; -damp x] (the stacked apply is a panel copy and a
scale), x accumulating in place.

Not built: preconditioning, warm start, batch sharding, a dense `exact` method, LSQR.
"""
import warnings
import torch
from xitorch_amd import kernels as K
from xitorch_amd._util import ConvergenceWarning, bcast_shape
from xitorch_amd.linalg._panel import RectPanelOperator, pad_len, batch_count, require_hip, to_panel, from_panel
from xitorch_amd.linalg.native_krylov import _Kry
from xitorch_amd.linalg import host_lsmr

__all__ = ["lsmr"]

ST_FLAG, ST_NORMB, ST_NORMA = 19, 20, 23
KEPT = 6.0          # stop code the driver gives members that sit out a resumption


class _Adj:
    """the adjoint of a panel operator"""

    def __init__(self, op):
        self.op, self.m, self.n = op, op.n, op.m

    def apply(self, X, out, adjoint):
        return self.op.apply(X, out, not adjoint)


class _Stacked:
    """[A; damp I] (m + n rows) on panels: the apply of A plus a panel copy and a scale"""

    def __init__(self, op, damp):
        self.op, self.damp, self.m0 = op, damp, op.m
        self.m, self.n = op.m + op.n, op.n

    def apply(self, X, out, adjoint):
        m0, n = self.m0, self.n
        self.op.apply(X, out, adjoint)
        if adjoint:
            out[:, :, :n].add_(X[:, :, m0:m0 + n], alpha=self.damp)
        else:
            torch.mul(X[:, :, :n], self.damp, out=out[:, :, m0:m0 + n])
        return out


class _Side:
    """buffers of one vector length: geometry, the shared Krylov kernels on it (`kr`), panels and partial arrays"""

    def __init__(self, N, Bt, nc, dtype, device):
        self.N, self.ld = N, pad_len(N)
        self.shape = (Bt, nc, self.ld)
        self.dtype, self.device, self.S = dtype, device, Bt * nc
        self.kr = _Kry(self)
        self.nblk, self.partial = self.kr.nblk, self.kr.partial_real

    def new(self):
        return torch.zeros(self.shape, dtype=self.dtype, device=self.device)

    def resid(self, b, y, r, Prr):
        """r = b - y (y None: only the partials of |b|^2 are wanted), Prr <- block partials of |r|^2"""
        self.kr.resid(b, y, r, None, Prr, None, init=y is None)

    def norm(self, P):
        return P[:, :self.nblk].double().sum(-1).sqrt()


def lsmr(A, B, damp=0.0, stack=None, **options):
    r"""
    LSMR for :math:`\min \|A x - b\|^2 + \mathrm{damp}^2 \|x\|^2` on the HIP kernels (dense, banded, CSR or a user
    operator; float64, float32, complex128, complex64).  Options: see ``linalg.lstsq``.  ``stack`` (used by the
    ``lstsq`` backward): ``"A"`` iterates on the stacked ``[A; damp I]`` without damping, ``"AH"`` on its adjoint.
    """
    device = torch.device(A.device)
    if device.type == "cpu":
        if stack is None:
            return host_lsmr.lsmr(A, B, damp, **options)
        return host_lsmr.lsmr_stacked(A, B, damp, stack, **options)
    require_hip(A, "lsmr")
    dtype = A.dtype
    mm, nn = host_lsmr.stacked_shape(A, damp, stack) if stack is not None else (A.shape[-2], A.shape[-1])
    opt = host_lsmr.check_lsmr_options(A, B, damp, options, shape=(mm, nn))
    damp = float(damp)
    bdims = list(bcast_shape(A.shape[:-2], B.shape[:-2]))
    Bt = batch_count(bdims)
    nc = B.shape[-1]
    if torch.allclose(B, B * 0):
        return torch.zeros((*bdims, nn, nc), dtype=dtype, device=device)
    base = RectPanelOperator(A, bdims, Bt)
    op, kdamp = base, damp
    if stack is not None:
        kdamp = 0.0
        if damp > 0:
            op = _Stacked(op, damp)
        if stack == "AH":
            op = _Adj(op)
    S = Bt * nc
    atol, btol, conlim, max_niter, every = opt["atol"], opt["btol"], opt["conlim"], opt["max_niter"], \
        opt["resid_calc_every"]

    V = _Side(nn, Bt, nc, dtype, device)
    rdtype = V.kr.rdtype
    x, h, hbar, vh, opv, gbuf = (V.new() for _ in range(6))
    Pv, Px, Pg, Pxx = V.partial(), (V.partial(), V.partial()), V.partial(), V.partial()
    runp = V.partial()
    state = K.lsmr_state(S, device)
    half = torch.full((S,), 0.5, dtype=rdtype, device=device)
    tr = dict(niter=0, host_reads=0, restarts=0)
    k = [0]

    def running():
        tr["host_reads"] += 1
        return int(V.kr.check_status(runp, half, nblk=1)[1])          # the one word the host reads

    def recurrence(rop, U, rhs, rdamp, normb=None, keep=None):
        """LSMR on min |rop dx - rhs|^2 + rdamp^2 |dx|^2, dx added to x; members of `keep` sit out (stop code KEPT)"""
        uh, opu, Pu = U.new(), U.new(), U.partial()
        kk = k[0]
        U.resid(rhs, None, None, Pu)
        K.lsmr_init(rhs, uh, Pu, state, runp, S, U.N, U.ld, U.nblk, kk)
        if normb is not None:
            state[kk & 1, :, ST_NORMB] = normb
        if keep is not None:
            state[kk & 1, :, ST_FLAG] = torch.where(keep, torch.full_like(normb, KEPT), state[kk & 1, :, ST_FLAG])
            runp[:, 0] = torch.where(keep, torch.zeros_like(runp[:, 0]), runp[:, 0])
        rop.apply(uh, opv, True)
        K.lsmr_bidiag(opv, vh, Pu, Pv, state, 1, S, V.N, V.ld, V.nblk, U.nblk, kk)
        upd = lambda q: K.lsmr_update(vh, h, hbar, x, Pu, Pv, Px[q & 1], Px[(q + 1) & 1], state, runp, S, V.N, V.ld,
                                      V.nblk, U.nblk, q, damp=rdamp, atol=atol, btol=btol, conlim=conlim)
        upd(kk)
        kk += 1
        it = 0
        while tr["niter"] < max_niter:
            rop.apply(vh, opu, False)
            K.lsmr_bidiag(opu, uh, Pv, Pu, state, 0, S, U.N, U.ld, U.nblk, V.nblk, kk)
            rop.apply(uh, opv, True)
            K.lsmr_bidiag(opv, vh, Pu, Pv, state, 1, S, V.N, V.ld, V.nblk, U.nblk, kk)
            upd(kk)
            kk += 1
            it += 1
            tr["niter"] += 1
            if it % every == 0 and running() == 0:
                break
        k[0] = kk

    U0 = _Side(mm, Bt, nc, dtype, device)
    rhs0 = to_panel(B.to(dtype), bdims, Bt, mm)
    rtrue, opu0, Pr = U0.new(), U0.new(), U0.partial()
    recurrence(op, U0, rhs0, kdamp)
    code = state[k[0] & 1, :, ST_FLAG].clone()
    normA = state[k[0] & 1, :, ST_NORMA].clone()
    normb = state[k[0] & 1, :, ST_NORMB].clone()
    while True:
        # confirmation on the true residuals
        op.apply(x, opu0, False)
        U0.resid(rhs0, opu0, rtrue, Pr)
        op.apply(rtrue, opv, True)
        xs = torch.mul(x, kdamp * kdamp) if kdamp > 0 else None
        V.resid(opv, xs, gbuf, Pg)
        V.resid(x, None, None, Pxx)
        nr, ng, nx = U0.norm(Pr), V.norm(Pg), V.norm(Pxx)
        nrbar = torch.sqrt(nr * nr + (kdamp * nx) ** 2)
        ok1 = nrbar <= 2 * (btol * normb + atol * normA * nx)
        ok2 = ng <= 2 * atol * normA * nrbar
        redo = ((code == 1) & ~ok1) | ((code == 2) & ~ok2)         # each member by the rule it stopped on
        # one read: the number of members to resume, the largest optimality residual, the stop codes
        summary = torch.cat([torch.stack([redo.sum().double(), ng.max()]), code]).tolist()
        tr["host_reads"] += 1
        if summary[0] == 0 or tr["restarts"] >= opt["max_restart"] or tr["niter"] >= max_niter:
            break
        tr["restarts"] += 1
        hbar.zero_()
        keep = ~redo
        if kdamp > 0:
            rop = _Stacked(op, kdamp)
            U = _Side(rop.m, Bt, nc, dtype, device)
            rhs = U.new()
            rhs[:, :, :mm].copy_(rtrue[:, :, :mm])
            torch.mul(x[:, :, :nn], -kdamp, out=rhs[:, :, mm:mm + nn])
        else:
            rop, U, rhs = op, U0, rtrue.clone()
        recurrence(rop, U, rhs, 0.0, normb=normb, keep=keep)
        new = state[k[0] & 1, :, ST_FLAG]
        code = torch.where(redo, new, code)
    codes = [int(c) for c in summary[2:]]
    nmax, ncon = codes.count(0), codes.count(3)
    if nmax:
        warnings.warn(ConvergenceWarning("lsmr: %d system(s) did not meet atol = %.1e / btol = %.1e after %d iterations "
                                         "(max |A^H r - damp^2 x| = %.3e)" % (nmax, atol, btol, tr["niter"], summary[1])))
    if ncon:
        warnings.warn(ConvergenceWarning("lsmr: %d system(s) stopped on cond(A) >= conlim = %.1e: the result is a "
                                         "regularised solution" % (ncon, conlim)))
    if opt["verbose"]:
        print("lsmr: %d iterations, %d restarts, %d host reads" % (tr["niter"], tr["restarts"], tr["host_reads"]))
    if opt["trace"] is not None:
        opt["trace"].update(niter=tr["niter"], napply=base.napply, torch_applies=base.torch_applies,
                            host_reads=tr["host_reads"], restarts=tr["restarts"], panel_kernel=base.kind,
                            stop_codes=codes)
    return from_panel(x, bdims, nn)
