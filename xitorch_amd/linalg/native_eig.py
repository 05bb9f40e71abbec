"""Native (HIP) block-Davidson eigensolver + the dense `exacteig` method.

`davidson` is the drop-in for the reference method of the same name
(xitorch/_impls/linalg/symeig.py:100-227): same signature, same options, same stopping rule
(global max|resid| over batch and columns < min_eps, or the basis became square), same
best-so-far return, same start block (CPU generator seeded with 12421, quirk Q5), no restart,
no preconditioner.  It performs the same mathematical iteration — Rayleigh–Ritz on the growing
orthonormal basis, residual block appended — but restructured so that the operator-panel
product K1 is the only O(N^2) work and everything else is an O(k N) stream:

  * the basis V and A V live PANEL-MAJOR in two growing (B, cap, Npad) buffers; new panels are
    written in place (no `cat`, no Fortran-order copies — symeig.py:210-223);
  * T = V^T A V is extended by its new rows/columns only (symeig.py:170 recomputes it all);
  * Ritz rotation, residual, max-norm and the next panel come from ONE fused kernel
    (symeig.py:178-188, 207);
  * the full CholeskyQR of [V, t] (tallqr, _utils/tensor.py:8-19) becomes block Gram–Schmidt of
    the new panel against the (already orthonormal) basis + CholeskyQR of the panel alone — in
    exact arithmetic the same Q, since chol([[I, C],[C^T, G]]) = [[I, C],[0, chol(G - C^T C)]];
  * one host sync per iteration and batch group (the reference has three: symeig.py:196,200,202), also in sharded
    runs: the all-reduce of the status runs on the device, in stream order, before that read;
  * large batches of native dense operators run as two groups: the panel products of both groups back to back on
    one CU-masked stream, each group's small kernels on its own hardware queue underneath the other group's
    panel product (option `overlap`).

All numerics run in libxitorch_amd.so (xk_dense_mm, xk_lincomb, xk_ritz_residual,
xk_panel_chol, xk_panel_transform); the only library call is the small k x k `eigh` of T.
Operators that are not native dense matrices are applied through their own `.mm`.
"""
import os
import torch
from xitorch_amd import kernels as K
from xitorch_amd._capi import NativeLibraryError
from xitorch_amd._util import bcast_shape
from xitorch_amd.linalg._panel import PanelOperator, pad_len, batch_count, require_hip
# (EXACTEIG_NATIVE_MAX_P is not used below: re-exported under the name the tests know, like the rest of this list)
from xitorch_amd.linalg._block import (cholqr_step, take_eigpairs, native_partial_eigh, _native_dense_ok, _initial_block,
                                       _shard_of_global_batch, _preconditioner, _pc_slice, K3G_MAX_K, GUARD_GOOD,
                                       GUARD_BAD, GUARD_MAX_REDO, EXACTEIG_NATIVE_MAX_P)
from xitorch_amd.dist import allreduce_max_

__all__ = ["davidson", "exacteig", "take_eigpairs", "tallqr_extend", "native_partial_eigh"]

_PRELAUNCH = True          # enqueue the next group's chain early (module attribute: measurement scripts flip it for A/B)
# largest basis the global-memory Rayleigh-Ritz solver (K3g, tridiagonalisation spread over several workgroups per
# matrix: xk_eigh_big.hip) serves before the library takes over (>= 16 matrices per group, fewer)
CHAIN_CUS = "all"             # units of the chain streams in the two-group pipeline: "all" | "reserved" (only the units the
                              # panel stream's mask leaves) | "auto" (measurement knob, scripts/timeline_gaps.py)
K3P_MIN_K = int(os.environ.get("XITORCH_K3P_MIN_K", "80"))   # from this order on K3p + K3g's final kernel replace K3t
                              # (r06; the environment variable is a measurement knob: 129 restores K3t)


def _gram(Vrows, k, panel, p, N):
    """G[b, c, a] = <V_a, panel_c>  (B, p, k) via K1 with the basis as the 'matrix'."""
    return K.dense_mm(Vrows[:, :k, :N], panel[:, :p, :N])


class _Group:
    """State of the Davidson iteration for one contiguous block of the batch, bound to one HIP stream."""

    def __init__(self, opA, opM, B, N, Npad, p, nguess, dtype, device, mode, small_eigh, orth_passes,
                 precond=None, restart=None, capacity=None):
        self.opA, self.opM = opA, opM
        self.precond = precond                    # None | ("diag", dA, dM) | ("op", PanelOperator)
        # (extension) thick restart: None = never (the reference's ever-growing basis); an int = largest basis
        # width; `keep` Ritz vectors survive a restart
        self.restart = restart
        # 2p Ritz vectors survive a restart: the p wanted ones and the p nearest unwanted ones, which is what keeps the
        # convergence of the unrestarted iteration (with only the wanted ones the restarted iteration stagnates:
        # measured, 10 of 1536 never converge).  Beyond 16 the restart step's Rayleigh-Ritz is the library eigh.
        self.keep = 2 * p
        self._compress = None                     # (Yt (B, pk, k), lam_all (B, pk)) of a pending restart
        self.nrestart = 0
        self.k1_stream = None                     # two-group pipeline: the (CU-masked) stream of the panel products
        self.k1_sched = None                      # (optional) [(basis width from, stream)]: the panel stream by basis width
        self.pg = None                            # sharded runs: the process group whose ranks decide together
        self.timeline, self.tag = None, 0         # debugging: (tag, label, start event, end event) per phase
        self.B, self.N, self.Npad, self.p = B, N, Npad, p
        self.dtype, self.device, self.mode = dtype, device, mode
        self.small_eigh, self.orth_passes = small_eigh, orth_passes
        self.nguess0 = nguess
        # basis storage: known up front with a thick restart (never more than `restart` vectors + one block) or a
        # caller's `basis_capacity`; otherwise a first guess that `grow` doubles (each growth is a fresh hipMalloc + copy:
        # ~0.2 s over an un-restarted 64 x 16384 run that reaches 582 vectors — the first call of a process pays it)
        if restart is not None:
            want = restart + p
        elif capacity is not None:
            want = int(capacity)
        else:
            want = nguess + 8 * p
        self.cap = max(nguess, min(N, want)) if N > nguess else nguess
        z = lambda *shape: torch.zeros(shape, dtype=dtype, device=device)
        self.Vs, self.AVs = z(B, self.cap, Npad), z(B, self.cap, Npad)
        self.MVs = z(B, self.cap, Npad) if opM is not None else None
        self.T = z(B, self.cap, self.cap)
        self.Wflat = torch.empty((B * 32 * 32,), dtype=dtype, device=device)
        self._cscratch = None                     # coefficient scratch of the one-call chain stages, B * p * cap
        self.info = torch.zeros((B,), dtype=torch.int32, device=device)
        # max|resid|, chol flag, K3t self-check flag, squared pivot ratio of the last orthonormalised panel(s),
        # a-posteriori guard max|X^T M X - I| of the Ritz block(s) formed since the last status
        self.status = torch.zeros((5,), dtype=torch.float64, device=device)
        self.cond = torch.zeros((B,), dtype=dtype, device=device)
        self.orth = torch.zeros((B,), dtype=dtype, device=device)
        self.MXtmp = z(B, p, Npad) if opM is not None else None
        self.adaptive = False                     # orth_passes="auto": one pass until a panel's condition estimate says no
        self.passes_now = 2                       # (the first panel is orthonormalised with two)
        self.two_pass_from = None
        self.rmax = z(B)
        self.Xbuf = [z(B, p, Npad), z(B, p, Npad)]
        self.k = 0
        self.fast = True          # chain stages as single C calls (xk_davidson_*); False: kernel by kernel (A/B, tests)
        self.best_slot, self.best_evals = -1, None
        self.slot, self.lam, self.newpanel, self.nadd = 0, None, None, 0

    def grow(self, need):
        if need <= self.cap:
            return
        new = min(self.N, max(need, 2 * self.cap))

        def bigger(old):
            buf = torch.zeros((self.B, new, self.Npad), dtype=self.dtype, device=self.device)
            buf[:, :old.shape[1]].copy_(old)
            return buf
        self.Vs, self.AVs = bigger(self.Vs), bigger(self.AVs)
        if self.MVs is not None:
            self.MVs = bigger(self.MVs)
        Tn = torch.zeros((self.B, new, new), dtype=self.dtype, device=self.device)
        Tn[:, :self.cap, :self.cap].copy_(self.T)
        self.T, self.cap = Tn, new

    def scratch(self, q):
        n = self.B * max(q, self.p) * (self.cap + q)
        if self._cscratch is None or self._cscratch.numel() < n:
            self._cscratch = torch.empty((n,), dtype=self.dtype, device=self.device)
        return self._cscratch

    def cholqr(self, k0, q, shifted=False):
        """Orthonormalise basis rows k0..k0+q among themselves (M-inner product if M).  shifted: the first step of
        shifted CholeskyQR (Gram matrix + 11 (N q + q (q + 1)) u trace(G) I, xk_chain.hip): leaves a well-conditioned,
        not yet orthonormal panel; a plain pass follows."""
        N = self.N
        if self.opM is None and self.fast and not shifted:
            K.davidson_orth(self.Vs, N, k0, q, self.scratch(q), self.Wflat, self.info, passes=0)
            return
        bufs = [self.Vs[:, k0:k0 + q]]
        if self.opM is not None:
            bufs.append(self.MVs[:, k0:k0 + q])
            self.opM.apply(bufs[0], bufs[1])
        Wq = self.Wflat[:self.B * q * q].view(self.B, q, q)      # compact (B, q, q), as the C ABI expects
        cholqr_step(bufs, bufs[-1], N, q, self.info, Wq, shift=shifted)

    def project_out(self, k0, q):
        """panel <- panel - V (V^H M panel) for the basis rows [0, k0)."""
        panel = self.Vs[:, k0:k0 + q]
        basis_for_coef = self.Vs if self.opM is None else self.MVs
        C = _gram(basis_for_coef, k0, panel, q, self.N)            # C[b,c,a] = <(M)V_a, t_c>
        K.lincomb(self.Vs, C, panel, k0, q, coef_layout="ca", alpha=-1.0, beta=1.0)

    def extend_T(self, k0, q):
        """rows/cols k0..k0+q of T = V^T A V from the new A V panel only."""
        N = self.N
        if self.fast:
            K.davidson_extend_t(self.Vs, self.AVs, self.T, self.scratch(q), N, k0, q)
            return
        Tn = K.dense_mm(self.Vs[:, :k0 + q, :N], self.AVs[:, k0:k0 + q, :N])     # (B, q, k0+q): <V_a, AV_c>
        self.T[:, k0:k0 + q, :k0 + q] = Tn
        self.T[:, :k0, k0:k0 + q] = Tn[:, :, :k0].transpose(-2, -1)

    def _mark(self, label, stream=None):
        """timeline instrumentation: returns a closer that records the end event"""
        if self.timeline is None:
            return lambda: None
        st = stream if stream is not None else torch.cuda.current_stream()
        e0 = torch.cuda.Event(enable_timing=True)
        e0.record(st)

        def close():
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record(st)
            self.timeline.append((self.tag, label, e0, e1))
        return close

    def apply_A(self, X, out):
        """out = A X.  In the two-group pipeline the panel products of both groups are funnelled through one
        stream (so they run back to back) whose CU mask leaves compute units free for the other group's small
        kernels; the group's own stream waits for the result."""
        if self.k1_stream is None:
            self.opA.apply(X, out)
            return
        n0 = len(self.opA.events) if (self.timeline is not None and self.opA.events is not None) else None
        k1s = self.k1_stream
        if self.k1_sched is not None:
            # the chain beside a launch grows with the basis: the panel stream leaves it more units as the run gets long
            for kfrom, st in self.k1_sched:
                if self.k >= kfrom:
                    k1s = st
        self.opA.apply_on(X, out, k1s)
        if n0 is not None and len(self.opA.events) > n0:            # timeline: the launch's own events
            e0, e1 = self.opA.events[-1][:2]
            self.timeline.append((self.tag, "k1", e0, e1))

    def start(self, V0p):
        k = V0p.shape[1]
        self.grow(k + self.p)
        self.Vs[:, :k, :self.N].copy_(V0p)
        self.cholqr(0, k)
        self.cholqr(0, k)          # CholeskyQR2: the second pass only removes rounding-level loss
        self.apply_A(self.Vs[:, :k], self.AVs[:, :k])
        self.extend_T(0, k)
        self.k = k

    def small(self, force_jacobi=False):
        """Rayleigh-Ritz on the current basis: K3 + fused rotation/residual; leaves {max|resid|, Cholesky flag,
        K3t self-check flag} in self.status (device) and the next panel in the basis.  No host sync.  Re-runnable:
        the driver repeats it with force_jacobi=True when the tridiagonalisation kernel flagged its own result."""
        k, p, N = self.k, self.p, self.N
        tri_flag = None
        self._orth_done = False                   # a new residual panel is about to replace the one orthonormalised
        # thick restart due after this Rayleigh-Ritz?  then the small eigensolver also returns the extra Ritz pairs
        # that will survive (pk >= p of them; the wanted p are the first / last p of the ascending list)
        due = self.restart is not None and k + p > self.restart and k > self.keep and k < N
        pk = min(self.keep, k) if due else p
        self._compress = None
        # r06: from order K3P_MIN_K on — and wherever K3t does not fit the LDS (order 126 with 6 pairs used to fall to the
        # Jacobi kernel: 2.8 ms against 0.45) — the persistent register-resident tridiagonalisation + K3g's final kernel
        # are ahead of the LDS-resident K3t (profiles/r06_k3p_orders.jsonl: 0.36 vs 0.41 ms at order 96, 0.23 vs 0.24 at 64)
        tri_fits = K.small_eigh_tri_ok(k, p, self.dtype) and K.small_eigh_tri_ok(k, pk, self.dtype)
        # — where the solver is on the critical path (one batch group).  Beside a panel stream (two groups) K3t stays: the
        # chain is hidden there and the configs[4] pipeline measured 1.4 % slower with K3p (85.5 / 86.2 / 85.4 against
        # 83.8 / 85.1 / 84.2 ms, interleaved)
        prefer_big = self.small_eigh == "native" and not force_jacobi and k <= K.SMALL_EIGH_MAX_K and \
            pk <= K.SMALL_EIGH_MAX_P and ((k >= K3P_MIN_K and getattr(self, "chain_exposed", False)) or
                                          (k >= K.SMALL_EIGH_TRI_MIN_K and not tri_fits)) and \
            K.small_eigh_big_ok(k, pk, self.dtype)
        if self.small_eigh in ("native", "jacobi", "tri") and k <= K.SMALL_EIGH_MAX_K and pk <= K.SMALL_EIGH_MAX_P \
                and not prefer_big:
            end = self._mark("k3")
            # K3t (tridiagonalisation + bisection + inverse iteration) from order 16 on: the O(k^3) work is done
            # once instead of ~8 Jacobi sweeps; small orders and anything K3t cannot hold in LDS go to Jacobi
            use_tri = (not force_jacobi) and self.small_eigh != "jacobi" and \
                (k >= K.SMALL_EIGH_TRI_MIN_K or self.small_eigh == "tri") and K.small_eigh_tri_ok(k, p, self.dtype)
            use_tri = use_tri and K.small_eigh_tri_ok(k, pk, self.dtype)
            if use_tri:
                lam, Yt, tri_flag = K.small_eigh(self.T, k, pk, uppest=(self.mode != "lowest"), method="tri")
            else:
                lam, Yt, _ = K.small_eigh(self.T, k, pk, uppest=(self.mode != "lowest"))  # K3: LDS Jacobi kernel
            end()
            if due:
                self._compress = (Yt, lam)
                sl = slice(0, p) if self.mode == "lowest" else slice(pk - p, pk)
                lam, Yt = lam[:, sl].contiguous(), Yt[:, sl]
            Y = Yt.transpose(1, 2)                                                        # (B, k, p) view
        elif self.small_eigh in ("native", "tri") and not force_jacobi and \
                (k > K.SMALL_EIGH_MAX_K or pk > K.SMALL_EIGH_MAX_P or prefer_big) and \
                k <= K3G_MAX_K[0 if self.B >= 16 else 1] and K.small_eigh_big_ok(k, pk, self.dtype):
            # K3g: bases of 129 .. 1536 vectors (the un-restarted iteration on slowly converging spectra) or 17 .. 64
            # wanted pairs at any order (wide eigen-blocks, thick restarts that keep 2 neig > 16 vectors): the same
            # tridiagonalisation route with the matrix in global memory: from order 192 on (fp64 to 614) the two-stage
            # form (band by block reflectors, bulge chasing in LDS: xk_eigh_band.hip), else one launch per Householder
            # step over several workgroups per matrix (xk_eigh_big.hip); a flagged result is
            # redone on the library (the driver's force_jacobi re-run lands in the branch below)
            end = self._mark("k3")
            lam, Yt, tri_flag = K.small_eigh_big(self.T, k, pk, uppest=(self.mode != "lowest"))
            end()
            if due:
                self._compress = (Yt, lam)
                sl = slice(0, p) if self.mode == "lowest" else slice(pk - p, pk)
                lam, Yt = lam[:, sl].contiguous(), Yt[:, sl]
            Y = Yt.transpose(1, 2)
        else:
            lam_all, Y_all = torch.linalg.eigh(self.T[:, :k, :k])                         # library eigh: > 256 pairs, > 1536 vectors
            if due:
                lk, Yk = take_eigpairs(lam_all, Y_all, pk, self.mode)
                self._compress = (Yk.transpose(1, 2).contiguous(), lk.contiguous())
            lam, Y = take_eigpairs(lam_all, Y_all, p, self.mode)
            lam = lam.contiguous()
        end_ritz = self._mark("ritz")
        self.grow(min(N, k + p))
        self.nadd = min(p, N - k)
        self.slot = 1 - self.best_slot if self.best_slot >= 0 else 0
        X = self.Xbuf[self.slot]
        if not (self.fast and self.opM is None and self.precond is None):
            self.rmax.zero_()
        if self.nadd == p and not due:
            self.newpanel = self.Vs[:, k:k + p]                 # the next panel is produced in place
        else:
            self.newpanel = torch.empty((self.B, p, self.Npad), dtype=self.dtype, device=self.device)
        fused_status = self.fast and self.opM is None and self.precond is None
        if fused_status:
            # rotation + residual + status in one C call; rmax comes back zeroed for the next step
            K.davidson_ritz(self.Vs, self.AVs, Y, lam, X, self.newpanel, self.rmax, self.info, tri_flag, self.status,
                            k, p, cond=self.cond, orth=self.orth)
        elif self.opM is None:
            K.ritz_residual(self.Vs, self.AVs, Y, lam, X, self.newpanel, self.rmax, k, p)
            K.ritz_guard(X, self.orth, p, self.Npad)
        else:
            # residual A X - lam (M X): rotate M V instead of V, then the eigenvectors separately
            K.ritz_residual(self.MVs, self.AVs, Y, lam, self.MXtmp, self.newpanel, self.rmax, k, p)
            K.lincomb(self.Vs, Y, X, k, p, coef_layout="ac", alpha=1.0, beta=0.0)
            K.ritz_guard(X, self.orth, p, self.Npad, MX=self.MXtmp)
        if self.precond is not None:
            # (extension) preconditioned correction t = K^-1 (-resid); the residual test above is unaffected
            if self.precond[0] == "diag":
                K.diag_precond(self.newpanel, self.precond[1], lam, p, m=self.precond[2])
            else:
                tmp = torch.zeros_like(self.newpanel)
                self.precond[1].apply(self.newpanel, tmp)
                self.newpanel.copy_(tmp)
        self.lam = lam
        if not fused_status:
            K.group_status(self.rmax, self.info, tri_flag, self.status, orth=self.orth)
        if self.pg is not None:
            # sharded run: the status the host is about to read becomes the GLOBAL one right here, in stream order
            # behind the kernel that wrote it (MAX over the ranks of {max|resid|, Cholesky flag, K3 flag, condition
            # estimate, guard}: symeig.py:188-203 decide on the maximum over ALL batch members) — through the C ABI on
            # this group's stream when the group is RCCL (dist.device_comm), else c10d.  Every decision below — stop,
            # K3 fallback, orthonormalisation passes, guard roll-back — is then the same on every rank by construction.
            torch.nan_to_num_(self.status, nan=float("inf"), posinf=float("inf"))
            allreduce_max_(self.status, self.pg)
        end_ritz()

    def compress(self):
        """Thick restart (extension; off by default): replace the basis by the `pk` Ritz vectors V Y of the
        Rayleigh-Ritz step just done — A V Y and M V Y come from the stored products, no operator apply — after
        which T is the diagonal matrix of their Ritz values.  The span keeps the wanted approximations and the
        nearest unwanted ones, which is what carries the convergence of the unrestarted iteration."""
        Yt, lam_all = self._compress
        self._compress = None
        k, pk = self.k, Yt.shape[1]
        for name in ("Vs", "AVs", "MVs"):
            buf = getattr(self, name)
            if buf is None:
                continue
            tmp = torch.zeros((self.B, pk, self.Npad), dtype=self.dtype, device=self.device)
            K.lincomb(buf, Yt, tmp, k, pk, coef_layout="ca", alpha=1.0, beta=0.0)
            buf[:, :pk].copy_(tmp)
        self.T.zero_()
        self.T[:, :pk, :pk] = torch.diag_embed(lam_all)
        # the kept Ritz block becomes the basis and T its diagonal: only true if the block is (M-)orthonormal — the same
        # a-posteriori guard as for a returned block, folded into the next status read
        K.ritz_guard(self.Vs, self.orth, pk, self.Npad, MX=self.MVs)
        self.k = pk
        self.nrestart += 1

    def rollback(self, k_good, passes):
        """Guard failure: back to the last basis width whose Ritz block passed (the basis is append-only between thick
        restarts, so rows [0, k_good) of V, A V, M V and the leading block of T are exactly that basis), the rest of the
        run on `passes` re-orthogonalised projection passes."""
        self.k = k_good
        self._compress = None
        self._orth_done = False
        self.adaptive = False
        self.orth_passes = max(int(self.orth_passes), int(passes))
        self.info.zero_()
        self.cond.zero_()
        self.orth.zero_()
        # (the best iterate so far stays: it passed the guard when it was recorded, and its block lives in the X buffer
        #  the void step did not write — a roll-back on the last allowed iteration still returns it, like the reference
        #  returns its best iterate with a ConvergenceWarning, symeig.py:196-200)
        self.reorthonormalise(k_good)

    def reorthonormalise(self, k):
        """What the reference does every iteration — CholeskyQR of the WHOLE basis (tallqr, _utils/tensor.py:8-19,
        symeig.py:207-223) — done once, after a guard failure, on the basis the run returns to: block Gram-Schmidt with
        re-orthogonalisation over the first k vectors, panel by panel ([projection against the panels before it,
        CholeskyQR], twice, the first CholeskyQR shifted).  The products A V and M V receive the same linear
        transformations (no operator apply), then T = V^T A V is rebuilt whole.  The basis a roll-back returns to
        passed the guard only in the directions of its Ritz block; without this step what it has lost elsewhere stays
        (measured: a residual floor of |A| times the loss, the run then grows to the full space)."""
        N = self.N
        bufs = [b for b in (self.Vs, self.AVs, self.MVs) if b is not None]
        coef_basis = self.Vs if self.opM is None else self.MVs
        k0 = 0
        while k0 < k:
            q = min(self.p if k0 > 0 else max(self.nguess0, 1), 32, k - k0)
            panel = self.Vs[:, k0:k0 + q]
            for it in range(2):
                if k0 > 0:
                    C = _gram(coef_basis, k0, panel, q, N)                  # C[b,c,a] = <(M)V_a, t_c>
                    for buf in bufs:
                        K.lincomb(buf, C, buf[:, k0:k0 + q], k0, q, coef_layout="ca", alpha=-1.0, beta=1.0)
                Mp = panel if self.opM is None else self.MVs[:, k0:k0 + q]
                cholqr_step([buf[:, k0:k0 + q] for buf in bufs], Mp, N, q, self.info, shift=(it == 0), symmetrise=True)
            k0 += q
        Tn = K.dense_mm(self.Vs[:, :k, :N], self.AVs[:, :k, :N], wide=False)   # Tn[b,c,a] = <V_a, (A V)_c>
        self.T[:, :k, :k] = (Tn + Tn.transpose(1, 2)) * 0.5

    def expand_orth(self):
        """First half of the expansion: (thick restart if due,) the residual panel of the last Rayleigh-Ritz step is
        orthonormalised against the basis.  Cheap and free of side effects beyond basis rows >= k, so the driver
        enqueues it BEFORE it reads the step's status: the host round trip (status -> decision -> next launches)
        then runs under these kernels instead of leaving the GPU idle (a step that is repeated — K3 fallback, guard
        roll-back — simply overwrites these rows)."""
        restarted = self._compress is not None
        if restarted:
            self.compress()
        k, nadd = self.k, self.nadd
        if nadd != self.p or restarted:
            self.Vs[:, k:k + nadd].copy_(self.newpanel[:, :nadd])
        end = self._mark("orth")
        if self.fast and self.opM is None:
            K.davidson_orth(self.Vs, self.N, k, nadd, self.scratch(nadd), self.Wflat, self.info,
                            passes=self.current_passes(nadd), cond=self.cond)
        else:
            # (the order of xk_davidson_orth: one pass = projection + CholeskyQR; more = [projection, CholeskyQR] per
            #  pass with the first CholeskyQR shifted — robust for nearly dependent residual blocks)
            rounds = self.current_passes(nadd)
            for it in range(rounds):
                self.project_out(k, nadd)
                if rounds >= 2 or it == rounds - 1:
                    self.cholqr(k, nadd, shifted=(rounds >= 2 and it == 0))
        end()
        self._orth_done = True

    # A panel whose squared pivot ratio (xk_davidson_orth's cond) is below this may be followed by ONE-pass panels.  Two
    # regimes were measured (scripts/orth_passes_scan.py, the headline workload): a benign plateau — the 64 operators of
    # BASELINE configs[1] settle at 1e3 .. 2e3 from iteration 7 on, S1 at order 2048 at 8e2 — where one pass loses
    # ~5e-15 of orthogonality per iteration, and exponential growth (~20x per iteration: S1 with neig = 8, pairs
    # converging one after the other) that ends at 1e11 and in duplicated eigenpairs.  The estimate reaches the host two
    # panels late (the next orthonormalisation is enqueued before the status is read), so with the threshold between
    # the two regimes one pass never meets a squared condition number above ~4e6: an orthogonality loss of ~2e-13 per
    # iteration at worst.  Beyond the threshold the run stays on two passes.
    ONE_PASS_MAX_COND2 = 1e4                     # fp64; fp32 runs use 1e2 (the loss per iteration is eps * condition)

    def current_passes(self, q):
        """projection passes of the next panel orthonormalisation"""
        if not self.adaptive:
            return max(1, self.orth_passes)
        if q > 8 or not (self.fast and self.opM is None and self.precond is None):
            return 2                              # (no condition estimate on these paths)
        return self.passes_now

    def note_condition(self, cond2, it):
        """the driver hands over status[3] after every status read"""
        limit = self.ONE_PASS_MAX_COND2 if self.dtype == torch.float64 else min(self.ONE_PASS_MAX_COND2, 1e2)
        if self.adaptive and self.passes_now == 1 and not (cond2 <= limit):
            self.passes_now = 2
            self.two_pass_from = it
        elif self.adaptive and self.two_pass_from is None and self.passes_now == 2 and cond2 <= limit and it >= 1:
            self.passes_now = 1                   # the start block and the first panel were benign: fast order

    def distrust(self, it):
        """the guard is above its 'good' level: no more one-pass panels in this run"""
        if self.adaptive and self.passes_now == 1:
            self.passes_now = 2
        if self.adaptive and self.two_pass_from is None:
            self.two_pass_from = it

    def speculate_orth(self):
        """expand_orth ahead of the status read — unless the step is not repeatable afterwards (a pending thick
        restart rewrites the basis) or there is nothing to add (square basis)"""
        if self._compress is None and self.nadd > 0 and self.k < self.N:
            self.expand_orth()

    def expand_apply(self):
        """Second half: the operator applied to the new block, T extended."""
        k, nadd = self.k, self.nadd
        self.apply_A(self.Vs[:, k:k + nadd], self.AVs[:, k:k + nadd])
        end = self._mark("extT")
        self.extend_T(k, nadd)
        end()
        self.k = k + nadd
        self._orth_done = False

    def expand(self):
        """Orthonormalise the residual panel against the basis, apply the operator to it, extend T."""
        if not getattr(self, "_orth_done", False):
            self.expand_orth()
        self.expand_apply()


def tallqr_extend(V, t, M=None, orth_passes=2):
    """Orthonormal extension of a basis on the device: given ``V (B, N, k)`` with (M-)orthonormal columns and a new
    block ``t (B, N, p)``, return ``Q (B, N, k+p)`` whose first k columns are V and whose last p columns span
    ``t`` minus its components along V, (M-)orthonormal — what the reference obtains from the full CholeskyQR
    ``tallqr(cat(V, t))`` (xitorch/_utils/tensor.py:8-19, _impls/linalg/symeig.py:207-220), computed here like in
    the Davidson loop: ``orth_passes`` rounds of [block Gram–Schmidt of the new panel against the basis, CholeskyQR of
    the panel alone] (the first CholeskyQR shifted when there are two or more).  In exact arithmetic the two agree column by column, since
    chol([[I, C], [C^T, G]]) = [[I, C], [0, chol(G - C^T C)]].  Raises RuntimeError when the panel Gram matrix is
    not positive definite (the reference raises from torch.linalg.cholesky)."""
    B, N, k = V.shape
    p = t.shape[-1]
    dev, dtype = V.device, V.dtype
    opM = PanelOperator(M, [B], B, N) if M is not None else None
    grp = _Group(None, opM, B, N, pad_len(N), p, k, dtype, dev, "lowest", "native", orth_passes)
    grp.grow(k + p)
    grp.Vs[:, :k, :N].copy_(V.transpose(-2, -1))
    grp.Vs[:, k:k + p, :N].copy_(t.transpose(-2, -1))
    if opM is not None:
        opM.apply(grp.Vs[:, :k], grp.MVs[:, :k])
    rounds = max(1, orth_passes)
    for it in range(rounds):                 # the order of the Davidson loop: [projection, CholeskyQR] per pass, the first
        grp.project_out(k, p)                # CholeskyQR shifted when another pass follows
        if rounds >= 2 or it == rounds - 1:
            grp.cholqr(k, p, shifted=(rounds >= 2 and it == 0))
    if int(grp.info.max().item()) != 0:
        raise RuntimeError("xitorch_amd tallqr_extend: the panel Gram matrix is not positive definite "
                           "(linearly dependent vectors)")
    return grp.Vs[:, :k + p, :N].transpose(-2, -1)


def _sub_operator(A, B, N, b0, b1):
    from xitorch_amd.linop import MatrixLinearOperator
    mat = A.mat.reshape(B, N, N)[b0:b1]
    sub = MatrixLinearOperator(mat, A.is_hermitian, symmetric_storage=getattr(A, "symmetric_storage", False))
    if getattr(A, "hermitian_verified", False):
        from xitorch_amd.linop import _storage_token
        sub._herm_token = _storage_token(mat)           # a slice of a verified matrix is verified
    return sub


class _GuardFailure(RuntimeError):
    """the a-posteriori guard failed and the run cannot be rolled back to a basis that passed it"""


def davidson(A, neig, mode, M=None, max_niter=1000, nguess=None, v_init="randn", max_addition=None,
             min_eps=1e-6, verbose=False, V0=None, orth_passes="auto", process_group=None, trace=None,
             rng_device="cpu", small_eigh="native", overlap="auto", precond=None, reserve_cus="auto", restart=None,
             groups="auto", chain="calls", basis_capacity=None, **unused):
    """Block Davidson on the HIP kernels; see `_davidson` for the options.  This wrapper is the last line of the
    a-posteriori guard: a run whose Ritz blocks fail it and that cannot be rolled back (thick restarts rewrite the
    basis) is repeated once from the start block with three re-orthogonalised projection passes; a second failure
    raises — a block that fails the guard is never returned."""
    from xitorch_amd.linalg.host_eig import refuse_nearest
    refuse_nearest("davidson", mode)
    kw = dict(M=M, max_niter=max_niter, nguess=nguess, v_init=v_init, max_addition=max_addition, min_eps=min_eps,
              verbose=verbose, V0=V0, process_group=process_group, trace=trace, rng_device=rng_device,
              small_eigh=small_eigh, overlap=overlap, precond=precond, reserve_cus=reserve_cus, restart=restart,
              groups=groups, chain=chain, basis_capacity=basis_capacity, **unused)
    try:
        return _davidson(A, neig, mode, orth_passes=orth_passes, **kw)
    except _GuardFailure as err:
        if isinstance(orth_passes, int) and orth_passes >= 3:
            raise RuntimeError("xitorch_amd davidson: %s" % err)
        first = dict(trace) if trace is not None else None
        try:
            res = _davidson(A, neig, mode, orth_passes=3, **kw)
        except _GuardFailure as err2:
            raise RuntimeError("xitorch_amd davidson: %s (also with three orthogonalisation passes)" % err2)
        if trace is not None:
            trace["orth_rerun"] = {"reason": str(err), "first_run": {k: first.get(k) for k in ("niter", "orth_redo")}}
        return res


class _GuardPolicy:
    """What the driver does with the a-posteriori check of every Rayleigh-Ritz block (`xk_ritz_guard`: max|X^T M X - I|,
    read with the iteration's status): which steps are void, where a void step returns to, when the run gives up.
    The same decisions on every group and rank (the values it sees are the folded / all-reduced ones)."""

    def __init__(self, dtype, k_start):
        self.good, self.bad = GUARD_GOOD[dtype], GUARD_BAD[dtype]
        self.k_good = k_start                     # widest basis whose Ritz block passed `good` (None: none left)
        self.history, self.redo = [], []
        self._restarts = 0

    def seen(self, guard, nrestart):
        self.history.append(guard)
        if nrestart != self._restarts:            # a thick restart rewrote the basis since the last step
            self._restarts, self.k_good = nrestart, None

    def void(self, chol_flag, guard):
        return chol_flag != 0 or guard > self.bad

    def roll_back(self, chol_flag, guard, k_rr, niter, trace):
        """-> (basis width to return to, projection passes from now on); raises when nothing is left to return to"""
        if self.k_good is None or self.k_good >= k_rr or len(self.redo) >= GUARD_MAX_REDO:
            if chol_flag != 0 and not self.redo:
                raise RuntimeError("xitorch_amd davidson: the panel Gram matrix is not positive definite "
                                   "(linearly dependent guess/residual vectors)")
            if trace is not None:
                trace.update(niter=niter, orth_redo=self.redo, orth_guard_history=self.history)
            raise _GuardFailure("the Ritz block lost its orthonormality (max|X^T M X - I| = %.2e at iteration %d, "
                                "basis of %d vectors) and no earlier basis is left to return to" % (guard, niter, k_rr))
        self.redo.append({"iter": niter, "guard": guard, "chol_flag": chol_flag, "k_from": k_rr, "k_to": self.k_good,
                          "passes": 2 + len(self.redo)})
        return self.k_good, 2 + len(self.redo) - 1

    def passed(self, guard, k_rr):
        """a block at or below `good` makes this basis width the new roll-back point; between `good` and `bad` the step
        counts but the groups stop trusting one projection pass"""
        if guard <= self.good:
            self.k_good = k_rr
            return True
        return False


class _Plan:
    """What `_plan_groups` decides for one davidson call: how many batch groups, which streams."""
    __slots__ = ("two", "ngrp", "reserve_cus", "spans", "ops", "streams", "k1_streams", "k1_sched", "distributed")


def _plan_groups(A, whole, M, B, N, p, dtype, device, precond, overlap, groups, reserve_cus, k1_streams_opt,
                 reserve_schedule, process_group):
    """The pipeline policy of one davidson call (no kernel is launched here): one batch group on the caller's stream,
    or `ngrp` groups whose small-kernel chains run on their own hardware queues while their operator-panel products
    go to CU-masked streams (see `_davidson`'s `overlap` / `groups` / `reserve_cus` / `k1_streams` options)."""
    plan = _Plan()
    nA = 1
    for d in A.shape[:-2]:
        nA *= d
    # Two groups pay off when a half-batch panel product is long enough (>= ~1 ms) to hide the other half's
    # small-kernel chain: "auto" switches them on from 8 GiB of operator storage (config 2: 137 GB).
    can_two = M is None and whole.kind == "dense" and not whole.flip and nA == B and B >= 2 \
        and not (precond is not None and not isinstance(precond, (str, torch.Tensor)))
    big = B * N * N * (8 if dtype == torch.float64 else 4) >= 2 ** 33
    two = can_two and (overlap is True or (overlap == "auto" and big))
    ngrp = 2
    if two:
        if groups == "auto":
            ngrp = 2
        else:
            ngrp = max(2, min(int(groups), B))
    reserve_auto = reserve_cus == "auto"
    if reserve_cus == "auto":
        wide_symm = whole.kind == "dense" and whole.symm and dtype == torch.float32 and \
            K.SYMM_WIDE_MIN_P <= p <= K.SYMM_WIDE_MAX_P and N >= K.SYMM_WIDE_MIN_N and N % 64 == 0
        reserve_cus = 32 if wide_symm else 64
        # resident K1s launches of the two groups on two streams (below): the panel stream gains more from 32 further
        # units than the chain loses (configs[1]: 211.4 ms per call with 64 left to the chain, 209.9 with 48, 206.7 with
        # 32, 211.6 with 16 — profiles/r05_k1s_pipeline_ab.jsonl)
        # (only where the per-group panel streams will be taken: on ONE stream 64 measured better — ADVICE r05)
        if can_two and K.K1S_OPTS is None and whole.kind == "dense" and whole.symm and whole.symm_narrow and p <= 6 \
                and (k1_streams_opt == "auto" or bool(k1_streams_opt)):
            total_cus = torch.cuda.get_device_properties(device).multi_processor_count
            if K.k1s_auto_opts(B // ngrp, N, dtype, max(1, total_cus - 32), pipelined=True) & K.K1S_PERSIST:
                reserve_cus = 32
    grp_streams, k1_streams, k1_sched = None, [None], None
    if two:
        try:
            chain_reserved = CHAIN_CUS == "reserved" or (CHAIN_CUS == "auto" and wide_symm and bool(K.K1SW_OPTS & 8))
            if chain_reserved and reserve_cus > 0:
                # (r06) the K1sw r06 form leaves ~100 registers per lane and 58 KB of LDS free on its units: chain
                # workgroups that move in beside it cost the panel kernel more than they gain — the chain streams get
                # the units the panel stream leaves, and only those
                grp_streams = [K.masked_stream(device, reserve_cus, slot=1 + g, only_reserved=True) for g in range(ngrp)]
            else:
                grp_streams = [K.masked_stream(device, 0, slot=1 + g) for g in range(ngrp)]
            k1_stream = K.masked_stream(device, reserve_cus)
            # Resident K1s launches (kernels.K1S_PERSIST): every group's panel product gets its own CU-masked stream.
            # A resident launch holds every workgroup slot of the masked units until its run queue is empty, so the
            # next group's launch — already enqueued on its stream — moves into the slots the tail frees instead of
            # waiting for the last workgroup (one stream: a kernel boundary per launch, the tail of a launch of 8.5
            # workgroup rounds leaves slots idle).  One-workgroup-per-run launches on two streams would share the slots
            # evenly and finish together: they stay on one stream.
            k1_streams = [k1_stream] * ngrp
            if k1_streams_opt == "auto":
                k1o = K.K1S_OPTS if K.K1S_OPTS is not None else \
                    K.k1s_auto_opts(B // ngrp, N, dtype, K.stream_cus(k1_stream), pipelined=True)
                split_k1 = bool(k1o & K.K1S_PERSIST) and whole.kind == "dense" and whole.symm \
                    and whole.symm_narrow and p <= 6
            else:
                split_k1 = bool(k1_streams_opt)
            if k1_streams_opt == "auto" and not split_k1 and whole.kind == "dense" and whole.symm and \
                    dtype == torch.float32 and K.SYMM_WIDE_MIN_P <= p <= K.SYMM_WIDE_MAX_P and \
                    N >= K.SYMM_WIDE_MIN_N and N % 64 == 0:
                # K1sw (fp32, 9 .. 16 columns): the same, when its launches are resident (kernels._k1sw_opts)
                split_k1 = bool(K._k1sw_opts(k1_stream, B // ngrp, N, pipelined=True) & K.K1SW_PERSIST)
            if split_k1:
                k1_streams = [K.masked_stream(device, reserve_cus, slot=64 + g) for g in range(ngrp)]
                sched = reserve_schedule
                if sched == "auto":
                    # un-restarted runs on slowly converging spectra reach bases of several hundred vectors; the chain
                    # of one group (five passes over the basis + the Rayleigh-Ritz solve) then outlasts the other
                    # group's panel product and wants the units back (S2, 64 x 16384^2, basis to 582, one box: 1.72 s
                    # with 32 units throughout, 1.58 with 64, 1.67 with 96, 1.66 with 32 / 64 / 96 from 0 / 160 / 320
                    # vectors: profiles/r05_c2_S2_schedule.jsonl)
                    sched = [(0, 32), (132, 64)] if (reserve_auto and reserve_cus == 32) else None
                if sched:
                    k1_sched = [(int(kf), [K.masked_stream(device, int(reserve_cus if cu is None else cu), slot=64 + g)
                                           for g in range(ngrp)]) for (kf, cu) in sched]
        except NativeLibraryError as err:            # no CU-mask support: same kernels, one group, one stream
            import warnings
            warnings.warn("xitorch_amd davidson: CU-masked streams unavailable (%s); running one batch group" % err)
            two = False
    distributed = process_group is not None and torch.distributed.get_world_size(process_group) > 1
    if distributed:
        # Sharded run: every batch group issues one status all-reduce per iteration (`_Group.small`), so the ranks must
        # run the SAME number of groups.  What a rank would pick depends on its local shard (B >= 2, the 8 GiB
        # threshold, whether CU-masked streams came up): the ranks agree on the minimum before any group exists.
        g_local = ngrp if two else 1
        g_all = torch.tensor([-float(g_local)], dtype=torch.float64, device=device)
        # (through c10d: a one-off on the caller's stream is not worth a communicator of its own)
        torch.distributed.all_reduce(g_all, op=torch.distributed.ReduceOp.MAX, group=process_group)
        g_common = int(round(-g_all.item()))
        if g_common < g_local:
            if g_common <= 1:
                two = False
            else:
                ngrp = g_common
                grp_streams, k1_streams = grp_streams[:ngrp], k1_streams[:ngrp]
                k1_sched = [(kf, sts[:ngrp]) for (kf, sts) in k1_sched] if k1_sched is not None else None
    if two:
        cuts = [(B * g) // ngrp for g in range(ngrp + 1)]
        spans = [(cuts[g], cuts[g + 1]) for g in range(ngrp)]
        ops = [PanelOperator(_sub_operator(A, B, N, b0, b1), [b1 - b0], b1 - b0, N) for (b0, b1) in spans]
        cur = torch.cuda.current_stream()
        # each group gets a stream with its own hardware queue (see kernels.masked_stream).  The caller's
        # stream is not used for a group: it usually is the legacy null stream, which synchronises implicitly
        # with every blocking stream and serialises the pipeline (measured: 280 instead of 224 ms)
        streams = grp_streams
        for st in streams + list(set(k1_streams)) + [t for (_, sts) in (k1_sched or []) for t in sts]:
            st.wait_stream(cur)
    else:
        spans, ops, streams, k1_streams, k1_sched = [(0, B)], [whole], [torch.cuda.current_stream()], [None], None
    plan.two, plan.ngrp, plan.reserve_cus, plan.spans, plan.ops, plan.streams = two, ngrp, reserve_cus, spans, ops, streams
    plan.k1_streams, plan.k1_sched, plan.distributed = k1_streams, k1_sched, distributed
    return plan


def _davidson(A, neig, mode, M=None, max_niter=1000, nguess=None, v_init="randn", max_addition=None,
              min_eps=1e-6, verbose=False, V0=None, orth_passes="auto", process_group=None, trace=None,
              rng_device="cpu", small_eigh="native", overlap="auto", precond=None, reserve_cus="auto", restart=None,
              groups="auto", chain="calls", basis_capacity=None, k1_streams="auto", reserve_schedule="auto",
              reserve_early=None, **unused):
    """
    Block Davidson method for the lowest / uppermost eigenpairs of a large Hermitian operator,
    running on MI355X HIP kernels.

    Keyword arguments
    -----------------
    max_niter: int
        Maximum number of iterations
    nguess: int or None
        Number of start vectors (default ``neig``)
    v_init: str
        Mode of the initial guess (``"randn"``, ``"rand"``, ``"eye"``); drawn on the CPU generator
        with seed 12421 like the reference's CPU path, then moved to the device.  ``"cos"``
        (extension) is an RNG-free closed form generated on the device
    max_addition: int or None
        Accepted for compatibility; like in the reference it has no effect
    min_eps: float
        Stop when the largest residual element over all batches and columns is below this
    verbose: bool
        Print the progress
    rng_device: str
        (extension) ``"cpu"`` (default): the random start block comes from the CPU generator, i.e. the
        reference's CPU path bit for bit; ``"device"``: drawn on the operator's device, which is what
        the reference does for a GPU-resident operator
    small_eigh: str
        (extension) ``"native"`` (default): the wanted eigenpairs of the Rayleigh–Ritz matrix come from native
        kernels — up to 128 basis vectors LDS-resident: Householder tridiagonalisation + bisection + inverse
        iteration (K3t) from order 16 on, parallel Jacobi (K3) below that and as the fallback when K3t's self-check
        flags a result; from 129 to 1536 vectors, or 17 to 256 wanted / kept pairs at any order, the same
        route with the matrix in global memory (K3g: from order 192 on — fp64 to 614 — a two-stage reduction, band by
        block reflectors then bulge chasing in LDS; else one launch per Householder step over several workgroups per
        matrix; 3.5x / 2.4x the library at order 582, measured; fallback: the library);
        ``torch.linalg.eigh`` beyond 1536 vectors or 256 pairs; ``"jacobi"`` / ``"tri"`` force one of
        the LDS kernels; ``"library"``: always ``torch.linalg.eigh``
    overlap: str or bool
        (extension) a batch of native dense operators can be processed as two groups: the operator-panel
        products of both groups run on streams whose CU mask leaves ``reserve_cus`` compute units free (one stream for
        both, or one each: ``k1_streams``), and the small Rayleigh–Ritz / orthogonalisation kernels of one group run
        on those CUs (own hardware queue) underneath the panel product of the other.  Iteration counts and the stopping rule are
        unchanged.  ``"auto"`` (default): on from 8 GiB of operator storage; ``True`` / ``False`` force it
    groups: str or int
        (extension) number of batch groups of the overlapped form.  ``"auto"`` (default): two.  More groups
        would hide a longer small-kernel chain under the other groups' panel products, but every group costs one
        host read of its status and ~20 kernel launches per iteration, and at the batch sizes where the chain is
        exposed the host is the limit: 8 operators of order 16384: 32.7 ms with 2 groups, 40.1 with 3, 52 with 4;
        16 operators: 56.6 vs 69.8 ms with 4 (r02).  An integer forces it (clamped to the batch size)
    reserve_cus: int or str
        (extension) compute units the panel-product stream leaves to the small kernels.  ``"auto"`` (default): 32 with
        resident K1s launches on per-group streams (r05: 211.4 ms per configs[1] call with 64, 209.9 with 48, 206.7 with
        32, 211.6 with 16), else 64 of 256 for the HBM-bound panel kernels (as fast on 192 CUs as on all of them; whole 32-CU mask words measured best:
        224.2 ms per config-2 call with 64, 227.5 with 32, 233 with 48 or 8, 241 with 96), 32 when the panel product is
        K1sw (fp32, 9 .. 16 columns, symmetric storage: issue-bound on the matrix cores, it scales with the CUs it gets —
        configs[4] shard: 120.6 ms per call with 64, 109.5 with 32, 109.8 with 16 or 8)
    k1_streams: str or bool
        (extension, r05) ``"auto"`` (default): each batch group's operator-panel product runs on its OWN CU-masked stream
        when its launches are resident (``kernels.k1s_auto_opts``: workgroups that take tile runs from a queue hold the
        machine until the queue is empty, so the other group's launch fills the slots the tail frees: 217.6 -> 211.9 ms
        per BASELINE configs[1] call); otherwise both groups share one masked stream.  ``True`` / ``False`` force it
    reserve_schedule: str, list or None
        (extension, r05) compute units left to the chains BY BASIS WIDTH, with per-group panel streams: a list of
        ``(basis width from, units)``.  ``"auto"`` (default): ``[(0, 32), (132, 64)]`` when ``reserve_cus`` is
        ``"auto"`` — the chain of a group grows with the basis, and on un-restarted runs to several hundred vectors it
        outlasts the other group's panel product; ``None``: ``reserve_cus`` throughout.  ``reserve_early=(cus, k)``
        (measurement) = ``[(0, cus), (k, reserve_cus)]``
    chain: str
        (extension) ``"calls"`` (default): every stage between two operator-panel products (rotation + residual +
        status, orthonormalisation of the new block, extension of T) is enqueued by one C call
        (``xk_davidson_ritz`` / ``_orth`` / ``_extend_t``); ``"kernels"``: kernel by kernel from the host loop — the
        same arithmetic up to the summation order inside the panel's Gram matrix (A/B, tests)
    precond: None, str, tensor or LinearOperator
        (extension; the reference has no preconditioner, symeig.py:206-207) ``None`` (default): new directions
        are the negated residuals, exactly like the reference.  ``"diag"``: Davidson's diagonal correction
        ``t = -r / (diag(A) - lam diag(M))`` with the operator's own diagonal (native dense / banded
        operators); a tensor ``(*batch, na)``: the same with that diagonal; a ``LinearOperator``: ``t = K (-r)``
    restart: int or None
        (extension) ``None`` (default): the basis grows until convergence, like the reference, which never restarts
        (symeig.py:132-135).  An integer: thick restart — whenever the next expansion would exceed this many basis
        vectors, the basis is replaced by the ``2 * neig`` Ritz vectors nearest the wanted end (the wanted ``neig``
        among them) before the new residual block is appended.  Bounds the memory (2 x restart x N per
        batch member) and keeps the Rayleigh–Ritz matrix inside the LDS-resident eigensolver on slowly converging
        spectra; costs extra iterations.  Must be >= ``3 * neig``.
    basis_capacity: int or None
        (extension) basis vectors to allocate storage for up front (2 x capacity x N elements per batch member).  Default:
        ``restart + neig`` with a thick restart, otherwise ``nguess + 8 neig`` doubled on demand — each doubling is a fresh
        device allocation and a copy, which the first call of a process pays (~0.2 s for a 64 x 16384 run that reaches
        582 vectors); a caller that knows the run is long can size it once
    V0: tensor or None
        (extension) start block ``(*batch, na, nguess)`` replacing the random draw
    orth_passes: int or str
        (extension) Gram–Schmidt passes of the new panel against the basis.  The reference re-orthonormalises the
        WHOLE basis every iteration (one CholeskyQR of ``[V, t]``, symeig.py:207-220); restricted to the new block that
        is one projection + one CholeskyQR, which is only safe while the residual block is well conditioned: the
        inverse factor amplifies the rounding-sized basis components the projection left by the block's condition
        number, and once some pairs have converged and others have not that number reaches 1e7 and more.  Measured
        with ONE pass throughout (round 3's first default): S1 with neig = 8 .. 16 lost the basis' orthogonality after
        ~30 iterations and returned duplicated eigenpairs (eigenvalue error 50) with a residual below ``min_eps``.
        ``"auto"`` (default): two passes in the order [projection, shifted CholeskyQR, projection, CholeskyQR]
        (xk_chain.hip) — except that blocks of up to 8 vectors take ONE pass while the fused CholeskyQR kernel's
        condition estimate (squared pivot ratio, read with the iteration's status) stays below 1e4; the first panel
        that exceeds it puts the rest of the run on two passes (``trace["orth_two_pass_from"]``).  With a
        preconditioner, ``restart=``, ``M`` or ``chain="kernels"``: always two.  An integer forces the number of passes.
        Whatever the setting, every Rayleigh–Ritz block is checked a posteriori (``max|X^T M X - I|``, one small kernel,
        read with the iteration's status): a block above ``GUARD_BAD`` is never a best / converged iterate, the run goes
        back to the last basis width whose block passed and continues with re-orthogonalised passes
        (``trace["orth_redo"]``, ``trace["orth_guard_history"]``).
    process_group: torch.distributed group or None
        (extension) when given, the batch is sharded over the group's ranks and the stopping test
        uses the all-reduced (MAX) residual, so all ranks iterate in lock step (RCCL over xGMI)
    """
    na = A.shape[-1]
    if nguess is None:
        nguess = neig
    bdims = list(A.shape[:-2]) if M is None else bcast_shape(A.shape[:-2], M.shape[:-2])
    dtype, device = A.dtype, torch.device(A.device)
    if device.type == "cpu":
        # device dispatch, like the reference (symeig.py:149): an operator in HOST memory is served by host_eig.py
        # (the same iteration in torch ops); any device operator by the HIP kernels below and by nothing else
        from xitorch_amd.linalg import host_eig
        return host_eig.davidson(A, neig, mode, M, max_niter=max_niter, nguess=nguess, v_init=v_init,
                                 max_addition=max_addition, min_eps=min_eps, verbose=verbose, V0=V0,
                                 process_group=process_group, trace=trace, precond=precond, restart=restart)
    require_hip(A, "davidson")
    if dtype.is_complex:
        # complex Hermitian operators: the same iteration on the complex kernels (native_eig_herm.py); the reference's
        # davidson is real-only (unconjugated transposes, symeig.py:163)
        from xitorch_amd.linalg import native_eig_herm
        return native_eig_herm.davidson(A, neig, mode, M, max_niter=max_niter, nguess=nguess, v_init=v_init,
                                        max_addition=max_addition, min_eps=min_eps, verbose=verbose, V0=V0,
                                        process_group=process_group, trace=trace, rng_device=rng_device,
                                        precond=precond, restart=restart)
    B = batch_count(bdims)
    N, Npad = na, pad_len(na)
    p = neig
    if restart is not None:
        restart = int(restart)
        if restart < 3 * p or restart < nguess + p:
            raise ValueError("restart must be at least 3 * neig (and nguess + neig), got %d" % restart)
    if (nguess > 32 or p > 32) and M is not None:
        raise NativeLibraryError("neig / nguess > 32 with an overlap operator M is not supported by the native "
                                 "davidson (the chunked panel orthonormalisation serves M = None)")
    adaptive = orth_passes == "auto" and precond is None and restart is None
    if orth_passes == "auto":
        orth_passes = 2
    events = trace.get("k1_events") if trace is not None else None

    # ---- batch groups: one, or two pipelined on their own streams (policy: `_plan_groups`) --------------------------
    whole = PanelOperator(A, bdims, B, N)
    plan = _plan_groups(A, whole, M, B, N, p, dtype, device, precond, overlap, groups, reserve_cus, k1_streams,
                        ([(0, int(reserve_early[0])), (int(reserve_early[1]), None)] if reserve_early is not None
                         else reserve_schedule), process_group)
    two, spans, ops, streams = plan.two, plan.spans, plan.ops, plan.streams
    k1_streams, k1_sched, distributed = plan.k1_streams, plan.k1_sched, plan.distributed
    for op in ops:
        op.events = events                       # bench.py: per-launch HIP events of the panel product
    G = len(spans)
    pc_full = _preconditioner(precond, whole, M, bdims, B, N, dtype, device)

    shard = None
    if distributed and V0 is None and v_init.lower() in ("randn", "rand", "random"):
        shard = _shard_of_global_batch(B, device, process_group)
    V0p = _initial_block(v_init, V0, bdims, B, N, nguess, dtype, device, rng_device, shard)       # (B, nguess, N)
    if two:
        for st in streams:
            st.wait_stream(torch.cuda.current_stream())
    groups = []
    for g, (b0, b1) in enumerate(spans):
        with torch.cuda.stream(streams[g]):
            opM = PanelOperator(M, bdims, B, N) if M is not None else None
            grp = _Group(ops[g], opM, b1 - b0, N, Npad, p, nguess, dtype, device, mode, small_eigh, orth_passes,
                         precond=_pc_slice(pc_full, b0, b1), restart=restart, capacity=basis_capacity)
            grp.k1_stream = k1_streams[g]
            grp.chain_exposed = not two          # one group: nothing hides the Rayleigh-Ritz solver
            if two and k1_sched is not None:
                grp.k1_sched = [(kf, sts[g]) for (kf, sts) in k1_sched]
            grp.adaptive = adaptive
            # (panels wider than 32 need the chunked orthonormalisation of xk_davidson_orth)
            grp.fast = (chain != "kernels") or p > 32 or nguess > 32
            if trace is not None and "timeline" in trace:
                grp.timeline, grp.tag = trace["timeline"], g
            grp.start(V0p[b0:b1])
            groups.append(grp)

    best_resid = float("inf")
    history = []
    stop_reason = "max_niter"
    niter = 0
    for grp in groups:
        grp.pg = process_group if distributed else None
    n_fallback = [0]
    cond_hist = [[] for _ in range(G)]            # squared pivot ratio of each group's panels (status[3]), as read
    policy = _GuardPolicy(dtype, groups[0].k)     # roll-back point at the start: the start block (CholeskyQR2)
    guard_hist, redo = policy.history, policy.redo
    for it in range(max_niter):
        niter = it + 1
        local_max, bad, guard = 0.0, 0.0, 0.0
        deferred = []
        k_rr = groups[0].k                      # the basis width this iteration's Rayleigh-Ritz runs on (all groups)
        # Every group's Rayleigh-Ritz chain AND the orthonormalisation of its next block are enqueued before the host
        # blocks on any status: the chain starts the moment the group's panel product is done, and the host round
        # trip (read the status, decide, launch the next panel product) runs under the orthonormalisation kernels.
        # Only the cheap half of the expansion is speculative: the panel product is launched once the status rules
        # out convergence, so nothing expensive is ever wasted.
        for g in range(G):
            if g == 0 or _PRELAUNCH:
                with torch.cuda.stream(streams[g]):
                    groups[g].small()
                    groups[g].speculate_orth()
        for g in range(G):
            if not _PRELAUNCH and g > 0:
                with torch.cuda.stream(streams[g]):
                    groups[g].small()
                    groups[g].speculate_orth()
            with torch.cuda.stream(streams[g]):
                # host waits for THIS group's stream only
                st_g, bad_g, tri_g, cond_g, orth_g = groups[g].status.tolist()
                if tri_g != 0:
                    # the tridiagonalisation kernel's self-check failed for some member: same step on Jacobi (the
                    # speculative orthonormalisation consumed its output: redo that too, it only touched rows >= k).
                    # A flagged result may hold zero / non-finite eigenvectors; the speculative CholeskyQR of the panel
                    # made from them then set the STICKY Cholesky flag (and cond / the guard) although the step that
                    # counts is the repeated one: clear what the speculation left, unless it was set before
                    if bad_g == 0:
                        groups[g].info.zero_()
                    groups[g].cond.zero_()
                    groups[g].orth.zero_()
                    groups[g].small(force_jacobi=True)
                    groups[g].speculate_orth()
                    st_g, bad_g, tri_g, cond_g, orth_g = groups[g].status.tolist()
                    n_fallback[0] += 1
                groups[g].note_condition(cond_g, it)
                cond_hist[g].append(cond_g)
            if st_g != st_g:
                st_g = float("inf")
            if orth_g != orth_g:
                orth_g = float("inf")
            local_max, bad, guard = max(local_max, st_g), max(bad, bad_g), max(guard, orth_g)
            # a local residual above the threshold already rules out global convergence (the global value is the max
            # over groups and ranks): the panel product of this group — and of the ones deferred so far — is certain
            if local_max >= min_eps and bad == 0 and k_rr < N:
                for gg in deferred + [g]:
                    with torch.cuda.stream(streams[gg]):
                        groups[gg].expand()
                deferred = []
            else:
                deferred.append(g)
        # (sharded runs: every group's status was all-reduced on the device before the host read it — `_Group.small` —
        #  so the values folded above already are the global ones: no further exchange, no further host read)
        max_resid = local_max
        policy.seen(guard, groups[0].nrestart)
        if policy.void(bad, guard):
            # The basis lost its orthogonality (or a panel its rank).  The reference cannot get here: it
            # re-orthonormalises the whole basis every iteration (tallqr of [V, t], _utils/tensor.py:8-19,
            # symeig.py:207-223).  This step is void; every rank / group takes the same decision (the values are the
            # all-reduced ones), so the groups stay in lock step.
            k_to, passes = policy.roll_back(bad, guard, k_rr, niter, trace)
            for g in range(G):
                with torch.cuda.stream(streams[g]):
                    groups[g].rollback(k_to, passes)
            history.append(max_resid)
            if verbose:
                print("Iter %3d (guess size: %d): guard %.2e: back to %d vectors" % (it + 1, k_rr, guard, k_to))
            continue
        if not policy.passed(guard, k_rr):
            for grp in groups:
                grp.distrust(it)
        history.append(max_resid)
        if verbose:
            print("Iter %3d (guess size: %d): resid: %.3e" % (it + 1, k_rr, max_resid))
        if max_resid < best_resid:
            best_resid = max_resid
            for grp in groups:
                grp.best_slot, grp.best_evals = grp.slot, grp.lam
        if max_resid < min_eps:
            stop_reason = "converged"
            break
        if k_rr == N:
            stop_reason = "full_basis"
            break
        for g in deferred:                      # (every local residual was below the threshold, another rank's is not)
            with torch.cuda.stream(streams[g]):
                groups[g].expand()

    if groups[0].best_slot < 0:     # max_niter == 0 or NaN residuals throughout
        raise RuntimeError("xitorch_amd davidson: no finite residual was produced")
    if two:
        cur = torch.cuda.current_stream()
        for st in streams + list(set(k1_streams)) + [t for (_, sts) in (k1_sched or []) for t in sts]:
            cur.wait_stream(st)
        evals = torch.cat([grp.best_evals for grp in groups], dim=0)
        Xall = torch.cat([grp.Xbuf[grp.best_slot] for grp in groups], dim=0)
        for grp in groups:                      # memory handed to the caller's stream
            grp.best_evals.record_stream(cur)
            grp.Xbuf[grp.best_slot].record_stream(cur)
    else:
        evals, Xall = groups[0].best_evals, groups[0].Xbuf[groups[0].best_slot]
    if trace is not None:
        trace.update(niter=niter, napply=sum(op.napply for op in ops) // G, resid_history=history,
                     basis_size=groups[0].k, best_resid=best_resid, stop_reason=stop_reason, groups=G,
                     k3_fallbacks=n_fallback[0], restarts=groups[0].nrestart, panel_kernel=ops[0].last_kernel,
                     orth_two_pass_from=[grp.two_pass_from for grp in groups], orth_adaptive=bool(adaptive),
                     orth_cond2_history=cond_hist, orth_guard_history=guard_hist, orth_redo=redo)
    evals = evals.reshape(*bdims, p)
    evecs = Xall[:, :, :N].transpose(-2, -1).reshape(*bdims, N, p)
    return evals, evecs


davidson.__doc__ = _davidson.__doc__ + "\n    (" + davidson.__doc__ + ")\n"


class _NativeEigh(torch.autograd.Function):
    """``neig`` extreme eigenpairs of a dense symmetric matrix from the native HIP eigensolver, with the reference's
    degeneracy-aware backward (degen_symeig, symeig.py:47-98).  The backward pass completes the eigenbasis with the
    differentiable `_DegenEigh` (only there), expresses the incoming eigenvector gradient in that basis — X = U_sel R^T
    with R = X^T U_sel, a signed permutation unless wanted eigenvalues coincide — and applies the same masked formula;
    being built from differentiable torch ops on the saved INPUT it supports higher derivatives like the reference's."""

    @staticmethod
    def forward(ctx, A, neig, mode):
        lam, X = native_partial_eigh(A.detach(), neig, mode)
        ctx.save_for_backward(A, X)
        ctx.neig, ctx.mode = neig, mode
        return lam, X

    @staticmethod
    def backward(ctx, glam, gX):
        A, X = ctx.saved_tensors
        n, p = A.shape[-1], ctx.neig
        lam_all, U = _DegenEigh.apply(A)
        lo, hi = (0, p) if ctx.mode == "lowest" else (n - p, n)
        pad = (lo, n - hi)
        gl = torch.nn.functional.pad(glam, pad) if glam is not None else None
        gU = None
        if gX is not None:
            R = torch.matmul(X.transpose(-2, -1), U[..., lo:hi]).detach()
            gU = torch.nn.functional.pad(torch.matmul(gX, R), pad)
        return _degen_eigh_backward(lam_all, U, gl, gU), None, None


def exacteig(A, neig, mode, M=None, sigma=None):
    """Eigendecomposition by building the full matrix (reference: exacteig, symeig.py:11-44).  On a HIP device, for real
    matrices of order 8 .. 1536 and up to 256 wanted pairs — the reference's own benchmark shapes, n in {100, 350, 700} with
    neig = 10 (benchmarks/benchmarks_solve.py:37-59) — the eigenpairs come from the native dense eigensolver
    (`native_partial_eigh`: only the wanted pairs are computed); everything else (CPU tensors, complex Hermitian, larger
    orders) is `torch.linalg.eigh` like the reference.  Both carry the degeneracy-aware backward of degen_symeig.
    mode="nearest" (extension) takes the full `eigh` and gathers the `neig` pairs nearest `sigma`, ascending."""
    nearest = mode == "nearest"
    if nearest and sigma is None:
        raise ValueError("exacteig: mode='nearest' needs the target: pass sigma=")
    Amat = A.fullmatrix()
    if M is None:
        if not nearest and _native_dense_ok(Amat, neig):
            return _NativeEigh.apply(Amat, neig, mode)
        evals, evecs = _DegenEigh.apply(Amat)
        return take_eigpairs(evals, evecs, neig, mode, sigma)
    L = torch.linalg.cholesky(M.fullmatrix())
    Linv = torch.inverse(L)
    LinvH = Linv.transpose(-2, -1).conj()
    A2 = torch.matmul(Linv, torch.matmul(Amat, LinvH))
    if not nearest and _native_dense_ok(A2, neig):
        A2 = (A2 + A2.transpose(-2, -1)) * 0.5          # (the kernels read one triangle: make both agree)
        evals, evecs = _NativeEigh.apply(A2, neig, mode)
    else:
        evals, evecs = _DegenEigh.apply(A2)
        evals, evecs = take_eigpairs(evals, evecs, neig, mode, sigma)
    return evals, torch.matmul(LinvH, evecs)


class _DegenEigh(torch.autograd.Function):
    """`eigh` whose backward masks (near-)degenerate pairs instead of dividing by ~0
    (reference: degen_symeig, symeig.py:47-98; arXiv:2011.04366)."""

    @staticmethod
    def forward(ctx, A):
        lam, U = torch.linalg.eigh(A)
        ctx.save_for_backward(lam, U)
        return lam, U

    @staticmethod
    def backward(ctx, glam, gU):
        lam, U = ctx.saved_tensors
        return _degen_eigh_backward(lam, U, glam, gU)


def _degen_eigh_backward(lam, U, glam, gU):
    import warnings
    from xitorch_amd.debug import is_debug_enabled
    from xitorch_amd._util import MathWarning
    UH = U.transpose(-2, -1).conj()
    thresh = torch.finfo(lam.dtype).eps ** 0.6
    if gU is not None:
        gap = lam.unsqueeze(-2) - lam.unsqueeze(-1)
        degen = torch.abs(gap) <= thresh
        gap = gap.masked_fill(degen, float("inf"))
        if is_debug_enabled():
            xtg = UH @ gU
            viol = (xtg - xtg.transpose(-2, -1).conj())[degen]
            if not torch.allclose(viol, torch.zeros_like(viol)):
                warnings.warn(MathWarning(
                    "Degeneracy appears but the loss function seem to depend strongly on the "
                    "eigenvector. The gradient might be incorrect.\nEigenvalues:\n%s\nDegenerate map:\n%s\n"
                    "Requirements (should be all 0s):\n%s" % (str(lam), str(degen), str(viol))))
        inner = gap.pow(-1) * torch.matmul(UH, gU)
        res = torch.matmul(U, torch.matmul(inner, UH))
    else:
        res = torch.zeros_like(U)
    if glam is not None:
        res = res + torch.matmul(U, glam.unsqueeze(-1) * UH)
    return (res + res.transpose(-2, -1).conj()) * 0.5
