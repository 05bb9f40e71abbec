"""Krylov-Schur Arnoldi on the HIP kernels: `eigs(..., method="arnoldi")`, eigenpairs of a NON-Hermitian operator.

An extension (the reference's eigensolvers assume A = A^H; Stewart, SIAM J. Matrix Anal. Appl. 23 (2001) 601).  Batched
over *BA with one Arnoldi vector per member and step; the driver has the structure of `native_gkl.gkl`.

One step j:  w = A v_j by one rectangular apply (`RectPanelOperator`: dense, CSR, banded, or the operator's own .mm) into
slot j + 1 of the basis panel, CGS2 against rows [0, j] in the THREE xk_gkl_sweep passes of the GKL driver, each followed
by an xk_arn_finish: the first stores its coefficients in column j of the device-resident projected matrix H
(Bt, ncv + 1, ncv; double, interleaved complex for complex operators), the second adds its own (the Arnoldi column is
c1 + c2), the third writes the norm to H[j + 1, j], keeps the running maximum and flags a breakdown; a fourth,
basis-free sweep scales the slot.  Nothing is read by the host inside a cycle.  At j = ncv ONE launch of xk_arn_schur
does the small work of every member — Schur form of H[:ncv, :ncv], ranking by `which`, reordering, Ritz vectors and
residual estimates |beta| |y_i[last]| of the wanted pairs, the restart coefficients Q and the restarted H — and writes
one status row per member, which the host reads (`trace["host_reads"]` counts these reads).  A restart keeps
keep' = neig + (ncv - neig) // 2 Schur vectors (one more when the cut would separate a conjugate pair of a real
operator; the kernel decides per member): V Q[:, :keep'] through xk_lincomb into the second panel, the residual vector
copied behind them.  The restarted H is a full keep' x keep' block plus the spike in row keep'; the step needs no
special case: the sweep orthogonalises against all rows, the columns come out full.

Members of one batch may keep different counts.  The cycle then starts at the smallest; a step below a member's own
count leaves that member's column of H and basis slot as they were (saved before the step, put back after it, on the
device).

Breakdown (H[j+1, j] <= u * the largest norm seen: an invariant subspace): as in gkl — H[j+1, j] stays 0, the status row
reports the first such step, the host replaces that vector by a random one orthogonalised against the basis (same
kernels) and the cycle is resumed from the step after it at the cost of one more status read.

Not built: gradients (they need left eigenvectors), shift-and-invert, block Arnoldi, harmonic Ritz extraction, left
eigenvectors (run it on A.H), batch sharding.  `host_eig.arnoldi` is the same algorithm in torch ops for operators in
host memory.
"""
import torch
from xitorch_amd import kernels as K
from xitorch_amd.linalg._panel import RectPanelOperator, batch_count, real_dtype, require_hip
from xitorch_amd.linalg import host_eig
from xitorch_amd.linalg.native_gkl import _Side, _rotate

__all__ = ["arnoldi"]

NOT_CLOSED_RETRIES = 2       # relaunches of xk_arn_schur with one more kept vector for members whose real basis is open


class _State:
    def __init__(self, Bt, ncv, n, neig, dtype, device):
        f64 = lambda *s: torch.zeros(s, dtype=torch.float64, device=device)
        i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=device)
        self.Bt, self.ncv, self.dtype, self.device = Bt, ncv, dtype, device
        self.rdt = real_dtype(dtype)
        self.u_round = float(torch.finfo(self.rdt).eps)
        self.hdt = torch.complex128 if dtype.is_complex else torch.float64
        self.V = _Side(Bt, ncv + 1, n, dtype, device)
        self.H = torch.zeros((Bt, ncv + 1, ncv), dtype=self.hdt, device=device)
        self.Hnext = torch.zeros_like(self.H)
        self.smax, self.nrm, self.rnrm = f64(Bt), f64(Bt), f64(Bt)
        self.brk = torch.full((Bt,), -1, dtype=torch.int32, device=device)
        self.keep_add = i32(Bt)
        self.coef = f64(Bt, 2 * K.GKL_MAX_ROWS)
        self.part = f64(Bt * K.gkl_nval(K.GKL_MAX_ROWS, dtype) * self.V.nchunk)
        self.out = (torch.zeros((Bt, ncv), dtype=torch.complex128, device=device),
                    torch.zeros((Bt, ncv, neig), dtype=torch.complex128, device=device), f64(Bt, neig),
                    torch.zeros((Bt, ncv, ncv), dtype=self.hdt, device=device), i32(Bt, K.arn_status_words()))

    def norm_slot(self, j):
        """the (Bt,) float64 view of H[:, j + 1, j] (its real part for a complex H) the third finish writes"""
        Hr = torch.view_as_real(self.H) if self.H.is_complex() else self.H.unsqueeze(-1)
        return Hr[:, j + 1, j, 0]

    def orthogonalise(self, j):
        """CGS2 of slot j + 1 against rows [0, j], the Arnoldi column into H[:, :j+1, j], the norm into H[:, j+1, j]"""
        side, Bt = self.V, self.Bt
        Q, w, rows = side.panel, side.panel[:, j + 1], j + 1
        nval = K.gkl_nval(rows, self.dtype)
        cview, hcol = self.coef[:, :nval - 1], self.H[:, :rows, j]
        fin = (self.part, Bt, nval, side.nchunk)
        K.gkl_sweep(Q, rows, w, w, None, None, self.part, side.N)
        K.arn_finish(*fin, cview, self.nrm, self.rnrm, hcol=hcol, accumulate=False)
        K.gkl_sweep(Q, rows, w, w, cview, None, self.part, side.N)
        K.arn_finish(*fin, cview, self.nrm, self.rnrm, hcol=hcol, accumulate=True)
        K.gkl_sweep(Q, rows, w, w, cview, None, self.part, side.N)
        K.arn_finish(*fin, None, self.nrm, self.rnrm, dst=self.norm_slot(j), smax=self.smax, u=self.u_round,
                     brk=self.brk, code=j)
        K.gkl_sweep(None, 0, w, w, None, self.rnrm, self.part, side.N)

    def orthonormalise_member(self, slot, b):
        """a replacement vector in `slot` of member b: CGS2 against rows [0, slot) and unit length; H is not touched"""
        side = self.V
        s = slice(b, b + 1)
        Q = side.panel[s]
        w = Q[:, slot]
        nval = K.gkl_nval(slot, self.dtype)
        coef, nrm, rnrm = self.coef[s], self.nrm[s], self.rnrm[s]
        cview = coef[:, :nval - 1]
        for c in (None, cview, cview):
            K.gkl_sweep(Q, slot, w, w, c, None, self.part, side.N)
            K.gkl_finish(self.part, 1, nval, side.nchunk, cview, nrm, rnrm)
        K.gkl_sweep(None, 0, w, w, None, rnrm, self.part, side.N)


def arnoldi(A, neig, which="LM", max_niter=100, min_eps=1e-6, ncv=None, V0=None, v_init="randn", rng_device="cpu",
            verbose=False, trace=None, M=None, process_group=None, **unused):
    """
    Krylov-Schur Arnoldi for the ``neig`` eigenpairs of a square, not necessarily Hermitian operator ``(*BA, n, n)``
    (dense, banded, CSR or a user ``_mv``; float64, float32, complex128, complex64) that ``which`` asks for, on the HIP
    kernels.  See ``xitorch_amd.linalg.eigs`` for the options; an operator in host memory is served by
    ``host_eig.arnoldi``.  ``RuntimeError`` when the start vector is zero, when the projected matrix holds a
    non-finite entry or when the QR iteration of the small Schur form hits its limit of ``30 ncv`` iterations.
    """
    device = torch.device(A.device)
    if device.type == "cpu":
        # device dispatch (see native_eig.davidson): an operator in HOST memory is served by host_eig.py
        return host_eig.arnoldi(A, neig, which, max_niter=max_niter, min_eps=min_eps, ncv=ncv, V0=V0, v_init=v_init,
                                rng_device=rng_device, verbose=verbose, trace=trace, M=M, process_group=process_group)
    n, neig, ncv, keep, dense = host_eig._arn_setup(A, neig, which, ncv, M, process_group)
    require_hip(A, "eigs")
    dtype = A.dtype
    if dense:
        if trace is not None:
            trace.update(niter=0, napply=0, ncv=ncv, handed_to="dense_eig")
        return host_eig._arn_dense(A, neig, which)
    if ncv > K.arn_max_rows():
        raise ValueError("eigs: ncv = %d is beyond the native small Schur kernel (ncv <= %d)" % (ncv, K.arn_max_rows()))
    real_op = not dtype.is_complex
    cdt = host_eig._arn_complex_dtype(dtype)
    bdims = list(A.shape[:-2])
    Bt = batch_count(bdims)
    op = RectPanelOperator(A, bdims, Bt)
    st = _State(Bt, ncv, n, neig, dtype, device)
    V = st.V

    v0 = host_eig._arn_start_vector(A, V0, v_init, bdims, Bt, n, dtype, device, rng_device)
    nv0 = torch.linalg.vector_norm(v0, dim=-1, keepdim=True)
    if bool((nv0 == 0).any()):
        raise RuntimeError("eigs: the start vector is zero")
    V.panel[:, 0, :n].copy_(v0 / nv0)
    gen = torch.Generator().manual_seed(12421 + 11)
    kps = [0] * Bt                                  # vectors every member kept at its last restart

    def step(j):
        ahead = [b for b in range(Bt) if kps[b] > j]
        if ahead:
            # these members hold column j already: what the step is about to overwrite is saved and put back
            live = torch.tensor([kps[b] <= j for b in range(Bt)], device=device)
            saved = (V.panel[:, j + 1].clone(), st.H[:, :, j].clone(), st.smax.clone(), st.brk.clone())
        op.apply(V.panel[:, j:j + 1], V.panel[:, j + 1:j + 2])
        st.orthogonalise(j)
        if ahead:
            V.panel[:, j + 1].copy_(torch.where(live.unsqueeze(-1), V.panel[:, j + 1], saved[0]))
            st.H[:, :, j].copy_(torch.where(live.unsqueeze(-1), st.H[:, :, j], saved[1]))
            st.smax.copy_(torch.where(live, st.smax, saved[2]))
            st.brk.copy_(torch.where(live, st.brk, saved[3]))

    def recover(j, members):
        # the vector of step j broke down for `members`: a random one, orthonormalised against the basis before it
        for b in members:
            r = host_eig._gkl_random(gen, 1, n, dtype).to(device)
            V.panel[b, j + 1, :n].copy_(r[0])
            st.orthonormalise_member(j + 1, b)

    def schur():
        K.arn_schur(st.H, neig, keep, which=which, tol=min_eps, u=st.u_round, keep_add=st.keep_add, brk=st.brk,
                    Hnext=st.Hnext, out=st.out)
        status = st.out[4].tolist()                               # the one host read of the cycle
        for row in status:
            if row[2] & K.ARN_FLAG_NONFINITE:
                raise RuntimeError("xitorch_amd eigs: the projected matrix holds a non-finite entry")
            if row[2] & K.ARN_FLAG_QR_LIMIT:
                raise RuntimeError("xitorch_amd eigs: the QR iteration of the projected matrix hit its limit of %d "
                                   "iterations" % (30 * ncv))
        return status

    niter, host_reads, history, kept, breakdowns, done = 0, 0, [], [], [], False
    for cycle in range(max_niter):
        niter = cycle + 1
        j0 = min(kps)
        st.keep_add.zero_()
        while True:
            st.brk.fill_(-1)
            for j in range(j0, ncv):
                step(j)
            status = schur()
            host_reads += 1
            broken = [(row[4], b) for b, row in enumerate(status) if row[4] >= 0]
            if not broken:
                break
            jb = min(j for j, _ in broken)
            members = [b for j, b in broken if j == jb]
            breakdowns.append((jb, members))
            recover(jb, members)
            j0 = jb + 1                       # strictly increasing: at most one recovery per step of the cycle
        nconv = [row[0] for row in status]
        history.append(nconv)
        if verbose:
            print("Cycle %3d (basis of %d): converged pairs per member %s" % (niter, ncv, nconv))
        if min(nconv) >= neig:
            done = True
            break
        if cycle + 1 == max_niter:
            break
        for _ in range(NOT_CLOSED_RETRIES):
            open_ = [b for b, row in enumerate(status) if row[2] & K.ARN_FLAG_NOT_CLOSED and row[3] < ncv - 1]
            if not open_:
                break
            st.keep_add[open_] += 1
            status = schur()
            host_reads += 1
        kps = [row[3] for row in status]
        kept.append(list(kps))
        Q = st.out[3]
        kmax = max(kps)
        if kmax > 0:
            _rotate(V, Q, kmax, ncv)          # (columns of Q beyond a member's own count are zero)
        if min(kps) == kmax:
            V.other[:, kmax].copy_(V.panel[:, ncv])
        else:
            for b in range(Bt):
                V.other[b, kps[b]].copy_(V.panel[b, ncv])
        V.swap()
        st.H, st.Hnext = st.Hnext, st.H
    theta, Y = st.out[0], st.out[1]
    # Ritz vectors x_i = V y_i (a real basis: the real and the imaginary part by one real lincomb each), unit length
    ncol = neig if not real_op else 2 * neig
    Xp = torch.zeros((Bt, ncol, V.ld), dtype=dtype, device=device)
    if real_op:
        C = torch.cat([Y.real, Y.imag], dim=-1).to(dtype).contiguous()                        # (Bt, ncv, 2 neig)
        K.lincomb(V.panel, C, Xp, ncv, ncol, coef_layout="ac")
        nx = torch.sqrt(torch.linalg.vector_norm(Xp[:, :neig], dim=-1) ** 2 +
                        torch.linalg.vector_norm(Xp[:, neig:], dim=-1) ** 2)
        Xp.div_(torch.cat([nx, nx], dim=-1).unsqueeze(-1))
    else:
        K.lincomb_c(V.panel, Y.transpose(1, 2).to(dtype).contiguous(), Xp, ncv, ncol, N=V.ld)
        Xp.div_(torch.linalg.vector_norm(Xp, dim=-1, keepdim=True))
    AXp = torch.zeros_like(Xp)
    op.apply(Xp, AXp)                                             # one more apply: the true residuals
    if real_op:
        X = torch.complex(Xp[:, :neig, :n], Xp[:, neig:, :n])
        AX = torch.complex(AXp[:, :neig, :n], AXp[:, neig:, :n])
    else:
        X, AX = Xp[:, :, :n], AXp[:, :, :n]
    lam = theta[:, :neig].to(cdt)
    resid = torch.linalg.vector_norm(AX - X * lam.unsqueeze(-1), dim=-1)
    hfro = torch.linalg.matrix_norm(st.H[:, :ncv, :ncv]).to(torch.float64)
    host_eig._arn_finish_report(resid, lam, hfro, st.u_round, min_eps, niter, done)
    if trace is not None:
        trace.update(niter=niter, restarts=niter - 1, napply=op.napply, ncv=ncv, keep=keep, converged_history=history,
                     breakdowns=breakdowns, host_reads=host_reads, torch_applies=op.torch_applies,
                     panel_kernel=op.kind, converged=done, resid=resid.reshape(*bdims, neig), kept_history=kept)
    return lam.reshape(*bdims, neig), X.transpose(-2, -1).reshape(*bdims, n, neig)
