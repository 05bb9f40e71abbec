"""Golub-Kahan-Lanczos bidiagonalisation with thick restart on the HIP kernels: `svd(..., method="gkl")`.

An extension (the reference's svd goes through symeig of A^H A, which squares the condition number; Baglama & Reichel,
SIAM J. Sci. Comput. 27 (2005) 19; full reorthogonalisation as in Larsen's PROPACK).  The iteration works on A itself,
batched over *BA with one Lanczos vector per member and step, always in the tall orientation (on A^H when m < n: started
on the long side the null space of A pollutes the small Ritz values and mode="lowest" does not converge).

One Lanczos step j:
  u_j = A v_j, orthogonalised against U[:j]     -> alpha_j = |u_j|, stored straight into the projected matrix Bm[j, j]
  v_{j+1} = A^H u_j, orthogonalised against V[:j+1] -> beta_j = |v_{j+1}|, stored into Bm[j, j+1] (the last one apart)
Each half: one rectangular apply (`RectPanelOperator`: dense through `trans`, CSR on its CSC view, banded, or the operator's
own .mm / .rmm) into the vector's basis slot, then CGS2 in THREE xk_gkl_sweep passes over the basis (accumulate / apply
and accumulate / apply and take the norm) with an xk_gkl_finish after each, and a fourth, basis-free sweep that scales
the slot by 1 / norm.  Nothing is read by the host inside a cycle.  At the end of a cycle xk_gkl_bsvd takes the SVD of
Bm (one-sided Jacobi, never Bm^T Bm) and writes the residual estimates |beta P[last, i]|, the projected matrix of the
restarted basis and ONE status word per member, which the host reads (`trace["host_reads"]` counts these reads).  A
restart keeps k + (ncv - k) // 2 plain Ritz triplets (uppest: the largest, lowest: the smallest): V Q[:, :keep] and
U P[:, :keep] through xk_lincomb into a second pair of panels.

Breakdown (alpha or beta <= u * the largest norm seen, flagged on the device by xk_gkl_finish): the member's entry of
Bm is 0, its vector is zero for the rest of the cycle; the status word of the cycle reports the first such half-step,
the host replaces that vector by a random one orthogonalised against the basis (same kernels) and the cycle is resumed
from the half-step after it (members without a breakdown recompute the same bits).  That recovery costs one more status
read.

Not built: block (multi-vector) GKL, harmonic Ritz restarts (plain Ritz is used for both modes), batch sharding, a
native small SVD beyond order 64, tracking of a "best" block (thick restart keeps the wanted Ritz triplets, so the last
block is the one returned).  `host_eig.gkl` is the same algorithm in torch ops for operators in host memory.
"""
import warnings
import torch
from xitorch_amd import kernels as K
from xitorch_amd._util import ConvergenceWarning
from xitorch_amd.linalg._panel import RectPanelOperator, pad_len, batch_count, real_dtype, require_hip
from xitorch_amd.linalg import host_eig

__all__ = ["gkl"]


class _Side:
    """One basis (the U or the V side): two (Bt, cap, ld) panels (the restart writes the transformed basis into the
    other one), the vector length N and the sweep's partial-sum geometry."""

    def __init__(self, Bt, cap, N, dtype, device):
        self.N, self.ld, self.cap = N, pad_len(N), cap
        self.panel = torch.zeros((Bt, cap, self.ld), dtype=dtype, device=device)
        self.other = torch.zeros((Bt, cap, self.ld), dtype=dtype, device=device)
        self.nchunk = K.gkl_chunks(N, dtype)

    def swap(self):
        self.panel, self.other = self.other, self.panel


class _State:
    def __init__(self, Bt, ncv, mm, nn, dtype, device):
        f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device=device)
        self.Bt, self.ncv, self.dtype, self.device = Bt, ncv, dtype, device
        self.rdt = real_dtype(dtype)
        self.u_round = float(torch.finfo(self.rdt).eps)
        self.U = _Side(Bt, ncv, mm, dtype, device)
        self.V = _Side(Bt, ncv + 1, nn, dtype, device)
        self.Bm, self.Bnext = f64(Bt, ncv, ncv), f64(Bt, ncv, ncv)
        self.beta, self.smax, self.nrm, self.rnrm = f64(Bt), f64(Bt), f64(Bt), f64(Bt)
        self.brk = torch.full((Bt,), -1, dtype=torch.int32, device=device)
        self.coef = f64(Bt, 2 * K.GKL_MAX_ROWS)
        nval = K.gkl_nval(K.GKL_MAX_ROWS, dtype)
        self.part = f64(Bt * nval * max(self.U.nchunk, self.V.nchunk))
        self.bsvd_out = (f64(Bt, ncv), f64(Bt, ncv, ncv), f64(Bt, ncv, ncv), f64(Bt, ncv),
                         torch.zeros((Bt, 4), dtype=torch.int32, device=device))

    def orthonormalise(self, side, j, dst=None, code=0, sel=None):
        """CGS2 of slot j of `side` against its rows [0, j) in three sweeps, the norm into dst (a (Bt,) view of the
        projected matrix, or beta), then the slot scaled to unit length.  sel: a batch slice (breakdown recovery)."""
        s = slice(None) if sel is None else sel
        Q = side.panel[s]
        w = Q[:, j]
        Bt = w.shape[0]
        coef, nrm, rnrm, part = self.coef[s], self.nrm[s], self.rnrm[s], self.part
        nval = K.gkl_nval(j, self.dtype)
        cview = coef[:, :nval - 1]
        fin = dict(smax=None, u=0.0, brk=None)
        K.gkl_sweep(Q, j, w, w, None, None, part, side.N)
        K.gkl_finish(part, Bt, nval, side.nchunk, cview, nrm, rnrm, **fin)
        K.gkl_sweep(Q, j, w, w, cview, None, part, side.N)
        K.gkl_finish(part, Bt, nval, side.nchunk, cview, nrm, rnrm, **fin)
        K.gkl_sweep(Q, j, w, w, cview, None, part, side.N)
        # (a recovery vector is random: its norm says nothing about sigma_max and cannot break down)
        K.gkl_finish(part, Bt, nval, side.nchunk, None, nrm, rnrm, dst=dst, smax=None if sel is not None else self.smax,
                     u=self.u_round, brk=None if sel is not None else self.brk, code=code)
        K.gkl_sweep(None, 0, w, w, None, rnrm, part, side.N)


def _rotate(side, C, ncols, ncv):
    """side.other[:, :ncols] = sum_a C[:, a, :ncols] side.panel[:, a] (a < ncv), C (Bt, ncv, ncv) float64"""
    dtype = side.panel.dtype
    if dtype.is_complex:
        Cc = C[:, :, :ncols].transpose(1, 2).to(dtype).contiguous()                   # (Bt, ncols, ncv): the "ca" layout
        K.lincomb_c(side.panel, Cc, side.other, ncv, ncols, N=side.ld)
    else:
        K.lincomb(side.panel, C[:, :, :ncols].to(dtype).contiguous(), side.other, ncv, ncols, coef_layout="ac")


def gkl(A, k, mode, max_niter=100, min_eps=1e-6, ncv=None, V0=None, v_init="randn", rng_device="cpu", verbose=False,
        trace=None, process_group=None, **unused):
    """
    Golub-Kahan-Lanczos bidiagonalisation with thick restart for the ``k`` largest / smallest singular triplets of a
    large operator ``(*BA, m, n)`` (dense, banded, CSR or a user ``_mv`` / ``_rmv``; float64, float32, complex128,
    complex64), on the HIP kernels.  Works on ``A`` itself, never on ``A^H A``.

    Keyword arguments
    -----------------
    max_niter: int
        Maximum number of restart cycles
    min_eps: float
        A triplet is converged when ``|beta P[last, i]| <= min_eps * sigma_max``; the iteration stops when the ``k``
        wanted triplets of every member are; otherwise the last Ritz block is returned with a ``ConvergenceWarning``
    ncv: int or None
        Basis size, ``k < ncv <= min(64, short side)``; default ``min(max(2k + 8, 20), short side)``
    V0: tensor or None
        ``(*batch, n, k0)`` guesses of right singular vectors: their sum is the start vector
    v_init, rng_device: str
        The start vector, as for ``davidson`` (seed 12421)
    trace: dict or None
        Receives ``niter``, ``restarts``, ``napply``, ``ncv``, ``keep``, ``converged_history`` (per cycle, the number
        of converged wanted triplets of every member: the status words; the residuals themselves stay on the device),
        ``breakdowns``, ``host_reads``, ``torch_applies``, ``panel_kernel``, ``tall``, ``converged``

    ``process_group`` raises ``NotImplementedError``; ``k > ncv - 1`` or ``ncv > 64`` raise ``ValueError``;
    ``RuntimeError`` when the start vector is zero or the Jacobi SVD of the projected matrix hits its sweep limit.  A
    breakdown never raises: the member continues from a random vector.  Each recovery costs one more read of the status
    words and a rerun of the rest of the cycle (at most one per half-step, so at most ``2 ncv`` per cycle): an operator
    whose numerical rank is below ``ncv`` pays that in every cycle -- choose ``ncv`` below the rank.  A problem
    whose short side is ``<= max(2k, 16)`` is handed to ``torch.linalg.svd``.  Returns ``(u (*BA, m, k), s (*BA, k)
    ascending, v (*BA, n, k))``.
    """
    device = torch.device(A.device)
    if device.type == "cpu":
        # device dispatch (see native_eig.davidson): an operator in HOST memory is served by host_eig.py
        return host_eig.gkl(A, k, mode, max_niter=max_niter, min_eps=min_eps, ncv=ncv, V0=V0, v_init=v_init,
                            rng_device=rng_device, verbose=verbose, trace=trace, process_group=process_group)
    m, n, tall, mm, nn, k, ncv, keep, dense = host_eig._gkl_setup(A, k, mode, ncv, process_group)
    require_hip(A, "gkl")
    dtype = A.dtype
    if dense:
        if trace is not None:
            trace.update(niter=0, napply=0, ncv=ncv, handed_to="dense_svd")
        return host_eig._gkl_dense(A, k, mode)
    bdims = list(A.shape[:-2])
    Bt = batch_count(bdims)
    op = RectPanelOperator(A, bdims, Bt)
    st = _State(Bt, ncv, mm, nn, dtype, device)
    U, V = st.U, st.V
    descending = mode != "lowest"

    v0 = host_eig._gkl_start_vector(A, V0, v_init, bdims, Bt, nn, tall, dtype, device, rng_device)
    nv0 = torch.linalg.vector_norm(v0, dim=-1, keepdim=True)
    if bool((nv0 == 0).any()):
        raise RuntimeError("gkl: the start vector is zero")
    V.panel[:, 0, :nn].copy_(v0 / nv0)
    gen = torch.Generator().manual_seed(12421 + 7)

    def half_step(h):
        j = h // 2
        if h % 2 == 0:
            op.apply(V.panel[:, j:j + 1], U.panel[:, j:j + 1], trans=not tall)
            st.orthonormalise(U, j, dst=st.Bm[:, j, j], code=h)
        else:
            op.apply(U.panel[:, j:j + 1], V.panel[:, j + 1:j + 2], trans=tall)
            st.orthonormalise(V, j + 1, dst=st.Bm[:, j, j + 1] if j + 1 < ncv else st.beta, code=h)

    def recover(h, members):
        # the vector of half-step h broke down for `members`: a random one, orthonormalised against the basis before it
        side, slot = (U, h // 2) if h % 2 == 0 else (V, h // 2 + 1)
        for b in members:
            r = host_eig._gkl_random(gen, 1, side.N, dtype).to(device)
            side.panel[b, slot, :side.N].copy_(r[0])
            st.orthonormalise(side, slot, dst=None, sel=slice(b, b + 1))

    start, niter, host_reads, history, breakdowns, done = 0, 0, 0, [], [], False
    for cycle in range(max_niter):
        niter = cycle + 1
        h0 = 2 * start
        while True:
            st.brk.fill_(-1)
            for h in range(h0, 2 * ncv):
                half_step(h)
            K.gkl_bsvd(st.Bm, st.beta, st.smax, st.brk, k=k, keep=keep, descending=descending, tol=min_eps,
                       Bnext=st.Bnext, out=st.bsvd_out)
            status = st.bsvd_out[4].tolist()                      # the one host read of the cycle
            host_reads += 1
            if any(row[2] for row in status):
                raise RuntimeError("xitorch_amd gkl: the Jacobi SVD of the projected matrix hit its sweep limit")
            broken = [(row[3], b) for b, row in enumerate(status) if row[3] >= 0]
            if not broken:
                break
            hb = min(h for h, _ in broken)
            members = [b for h, b in broken if h == hb]
            breakdowns.append((hb, members))
            recover(hb, members)
            h0 = hb + 1                       # strictly increasing: at most one recovery per half-step of the cycle
        nconv = [row[0] for row in status]
        history.append(nconv)
        if verbose:
            print("Cycle %3d (basis of %d): converged triplets per member %s" % (niter, ncv, nconv))
        if min(nconv) >= k:
            done = True
            break
        if cycle + 1 == max_niter:
            break
        sigma, P, Q, res, _ = st.bsvd_out
        _rotate(V, Q, keep, ncv)
        V.other[:, keep].copy_(V.panel[:, ncv])
        _rotate(U, P, keep, ncv)
        U.swap()
        V.swap()
        st.Bm, st.Bnext = st.Bnext, st.Bm
        start = keep
    sigma, P, Q, res, _ = st.bsvd_out
    if not done:
        worst = float((res[:, :k] / torch.clamp(torch.maximum(sigma.max(dim=-1)[0], st.smax), min=1e-300)
                       .unsqueeze(-1)).max())
        warnings.warn(ConvergenceWarning("gkl: convergence is not achieved after %d restart cycles (max |beta P[last, i]| "
                                         "/ sigma_max = %.3e > min_eps = %.3e); the last Ritz block is returned"
                                         % (niter, worst, min_eps)))
    _rotate(V, Q, k, ncv)
    _rotate(U, P, k, ncv)
    uu = U.other[:, :k, :mm].transpose(-2, -1)
    vv = V.other[:, :k, :nn].transpose(-2, -1)
    ss = sigma[:, :k].to(st.rdt)
    if descending:
        uu, vv, ss = uu.flip(-1), vv.flip(-1), ss.flip(-1)
    if not tall:
        uu, vv = vv, uu
    if trace is not None:
        trace.update(niter=niter, restarts=niter - 1, napply=op.napply, ncv=ncv, keep=keep, converged_history=history,
                     breakdowns=breakdowns, host_reads=host_reads, torch_applies=op.torch_applies,
                     panel_kernel=op.kind, tall=tall, converged=done)
    return uu.reshape(*bdims, m, k), ss.reshape(*bdims, k), vv.reshape(*bdims, n, k)
