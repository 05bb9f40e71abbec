"""The block layer of the native eigensolvers: what a driver does to a block of vectors, stated once per dtype.

It stands on the panel layer (`_panel.py`) and `kernels` and below every driver (it imports none of them):

  * what all eigensolver drivers and their host twin share: the start block, the preconditioner grammar, the
    a-posteriori guard levels `GUARD_*`, the first-pass shift of shifted CholeskyQR, `take_eigpairs`;
  * the routers of the small dense eigensolve, `native_partial_eigh` (real: K3t / K3g) and `herm_partial_eigh`
    (complex: xk_herm_eigh), members whose self-check fails redone on the library;
  * `RealBlockOps` (zero-padded (Bt, rows, pad_len(N)) panels on the Davidson chain kernels) and `ComplexBlockOps`
    ((Bt, rows, N) panels on the xk_herm_* kernels): allocation, Gram block and combination on K1, block
    orthonormalisation (projection against earlier rows + CholeskyQR, first pass shifted), the lowest pairs of a small
    Rayleigh-Ritz matrix with the bookkeeping of who served them, the guard with its ONE host read, Jacobi's diagonal
    preconditioner.

Every kernel is reached through an attribute of `kernels` at call time, never through a name bound at import.
"""
import torch
from xitorch_amd import kernels as K
from xitorch_amd.linalg._panel import PanelOperator, pad_len, real_dtype

__all__ = ["RealBlockOps", "ComplexBlockOps", "block_ops", "cholqr_step", "native_partial_eigh", "herm_partial_eigh",
           "take_eigpairs", "GUARD_GOOD", "GUARD_BAD", "GUARD_MAX_REDO"]


def take_eigpairs(evals, evecs, neig, mode, sigma=None):
    """First (``lowest``) or last (``uppest``) ``neig`` pairs of an ascending ``eigh`` result; the
    returned eigenvalues are ascending in both modes (reference: symeig.py:255-264).  ``nearest`` (extension): the
    ``neig`` pairs whose eigenvalues are nearest ``sigma`` (a number or a real tensor broadcastable to the batch
    dimensions; no gradient flows to it), ascending as well."""
    if mode == "nearest":
        if sigma is None:
            raise ValueError("mode='nearest' needs the target: pass sigma=")
        s = sigma.detach() if isinstance(sigma, torch.Tensor) else torch.as_tensor(sigma)
        s = s.to(device=evals.device, dtype=evals.dtype).expand(evals.shape[:-1]).unsqueeze(-1)
        idx = torch.argsort((evals.detach() - s).abs(), dim=-1, stable=True)[..., :neig]
        idx = torch.sort(idx, dim=-1)[0]                     # eigh's order: the picked eigenvalues ascend
        return torch.gather(evals, -1, idx), torch.gather(evecs, -1, idx.unsqueeze(-2).expand(*evecs.shape[:-1], neig))
    if mode == "lowest":
        return evals[..., :neig], evecs[..., :neig]
    return evals[..., -neig:], evecs[..., -neig:]


def _shift_rel(N, q, rdtype):
    """first-pass shift of shifted CholeskyQR (Fukaya et al.), relative to trace(G): 11 (N q + q (q + 1)) u, capped, as
    xk_davidson_orth chooses it"""
    u = torch.finfo(rdtype).eps * 0.5
    return min(11.0 * (N * q + q * (q + 1)) * u, 1e-3)


def _shard_of_global_batch(B, device, process_group):
    """(offset, total) of this rank's B members in the group's global batch: the ranks hold consecutive blocks in rank
    order (how `dist.shard_range` deals a batch out); one all-gather of the local counts, once per call."""
    world = torch.distributed.get_world_size(process_group)
    rank = torch.distributed.get_rank(process_group)
    mine = torch.tensor([float(B)], dtype=torch.float64, device=device)
    allb = [torch.zeros_like(mine) for _ in range(world)]
    torch.distributed.all_gather(allb, mine, group=process_group)
    counts = [int(round(v.item())) for v in allb]
    return sum(counts[:rank]), sum(counts)


def _initial_block(v_init, V0, bdims, B, N, nguess, dtype, device, rng_device="cpu", shard=None):
    """The start block (reference: symeig.py:236-246).  `shard` = (offset, total) on a batch-sharded run: the random
    kinds draw the block of the WHOLE batch from seed 12421 and keep this rank's members, so that member b of an
    N-GPU run starts from the same vectors as member b of the one-GPU run (same iterates, same iteration count)."""
    if V0 is not None:
        if V0.shape[-2] != N:
            raise RuntimeError("V0 must have shape (*batch, %d, nguess), got %s" % (N, tuple(V0.shape)))
        V = V0.to(device=device, dtype=dtype).expand(*bdims, N, V0.shape[-1]).reshape(B, N, V0.shape[-1])
        return V.transpose(-2, -1)
    kind = v_init.lower()
    if kind == "cos":
        # (extension) RNG-free closed form generated on the device: V0[i,j] = cos(0.1 (i+1)(j+1) + 0.05 b)
        from xitorch_amd import synthetic
        return synthetic.start_block(B, N, nguess, dtype, device)
    # seed 12421 on the global generators, like the reference (symeig.py:236-246, quirk Q5).
    # rng_device="cpu" (default) draws from the CPU stream = the reference's CPU path (parity runs);
    # rng_device="device" draws on the operator's device = what the reference does for a GPU operator.
    torch.manual_seed(12421)
    rdev = torch.device("cpu") if rng_device == "cpu" else device
    if kind == "eye":
        V = torch.eye(N, nguess, dtype=dtype, device=rdev).unsqueeze(0).repeat(B, 1, 1)
    elif kind in ("randn", "rand", "random"):
        draw = torch.randn if kind == "randn" else torch.rand
        if shard is not None and shard[1] != B:
            off, total = shard
            # (the generators fill a tensor as a function of its whole size: draw the whole batch, keep the shard)
            V = draw((total, N, nguess), dtype=dtype, device=rdev)[off:off + B].clone()
        else:
            V = draw((*bdims, N, nguess), dtype=dtype, device=rdev).reshape(B, N, nguess)
    else:
        raise ValueError("Unknown v_init type: %s" % kind)
    return V.to(device).transpose(-2, -1)


# A-posteriori guard on every Rayleigh-Ritz block, g = max|X^T M X - I| over the batch (status[4]):
#   g <= GOOD            the basis width of this step becomes the roll-back point
#   GOOD < g <= BAD      the rest of the run takes two projection passes (nothing is undone)
#   g > BAD (or NaN)     the step is void: never a best / converged iterate; the run goes back to the last roll-back
#                        point with re-orthogonalised passes (trace["orth_redo"]); with none left it is repeated from the
#                        start block with three passes, and if that fails too an error is raised
#                        point — whose basis is re-orthonormalised as a whole, like the reference does every iteration —
# Healthy runs measure 1e-15 .. 1.3e-12 (fp64) / 1e-6 .. 1e-5 (fp32) (profiles/r04_guard_scan.jsonl); two copies of one
# eigenpair give 1.
GUARD_GOOD = {torch.float64: 1e-10, torch.float32: 5e-5}
GUARD_BAD = {torch.float64: 1e-8, torch.float32: 5e-4}
GUARD_MAX_REDO = 3


def _preconditioner(precond, whole, M, bdims, B, N, dtype, device):
    """(extension; the reference has none, symeig.py:206-207) the preconditioner of the new directions in the form the
    groups take it: None, ("diag", diag A, diag M or None) or ("op", panel operator)."""
    if precond is None:
        return None
    from xitorch_amd.linop import LinearOperator as _LinOp
    if isinstance(precond, str):
        if precond.lower() not in ("diag", "jacobi", "davidson"):
            raise RuntimeError("Unknown davidson preconditioner: %s" % precond)
        dA = whole.diagonal()
        dM = PanelOperator(M, bdims, B, N).diagonal() if M is not None else None
        return ("diag", dA, dM)
    if isinstance(precond, torch.Tensor):
        if precond.shape[-1] != N:
            raise RuntimeError("precond diagonal must have shape (*batch, %d), got %s" % (N, tuple(precond.shape)))
        dA = precond.to(device=device, dtype=dtype).expand(*bdims, N).reshape(B, N).contiguous()
        dM = PanelOperator(M, bdims, B, N).diagonal() if M is not None else None
        return ("diag", dA, dM)
    if isinstance(precond, _LinOp):
        return ("op", PanelOperator(precond, bdims, B, N))
    raise TypeError("precond must be None, 'diag', a tensor or a LinearOperator, got %s" % type(precond))


def _pc_slice(pc_full, b0, b1):
    if pc_full is None or pc_full[0] == "op":
        return pc_full
    cut = lambda t: None if t is None else (t if t.shape[0] == 1 else t[b0:b1])
    return ("diag", cut(pc_full[1]), cut(pc_full[2]))


# ---- the small dense eigensolve

K3G_MAX_K = [1536, 1024]      # largest basis K3g serves before the library takes over, [>= 16 matrices per group, fewer]:
                              # measured r06 (order 1200 / 1536, ms): 1 matrix 44.5 / 83.1 native against 28.2 / 37.1 library,
                              # 4: 45.6 / 85.1 against 34.8 / 50.5, 32: 76.2 / 150.4 against 111.8 / 198.6; at 1024: 26.6 / 24.0, 44.2 / 75.1
# orders / widths the native dense eigensolvers serve (K3g: xk_eigh_big.hip; below 129 / 17 also the LDS kernels)
EXACTEIG_NATIVE_MAX_N = K.SMALL_EIGH_BIG_MAX_K
EXACTEIG_NATIVE_MAX_P = K.SMALL_EIGH_BIG_MAX_P


def _native_dense_ok(mat, neig):
    n = mat.shape[-1]
    nb = mat.numel() // max(1, n * n)
    # (beyond order 1024 the native form is ahead of the library from 16 matrices on only: K3G_MAX_K)
    return (mat.is_cuda and mat.dtype in (torch.float64, torch.float32) and 8 <= n <= EXACTEIG_NATIVE_MAX_N
            and n <= K3G_MAX_K[0 if nb >= 16 else 1]
            and 1 <= neig <= min(EXACTEIG_NATIVE_MAX_P, n) and mat.numel() > 0
            and K.small_eigh_big_ok(n, neig, mat.dtype))


def native_partial_eigh(mat, neig, mode):
    """Lowest / uppermost ``neig`` eigenpairs of the dense symmetric matrices ``mat (*B, n, n)`` on the native HIP
    eigensolvers — Householder tridiagonalisation, bisection, inverse iteration, back-transformation: K3t (LDS-resident,
    n <= 128, neig <= 16) or K3g (global-memory work matrix, n <= 1536, neig <= 256).  Only the wanted pairs are computed
    (the reference's exacteig computes all n and slices, symeig.py:22-24,255-264).  Returns ``evals (*B, neig)``
    ascending and ``evecs (*B, n, neig)``; members whose self-check flags the result are redone on
    ``torch.linalg.eigh``."""
    bdims, n = mat.shape[:-2], mat.shape[-1]
    T = mat.reshape(-1, n, n)
    if T.stride(-1) != 1:
        T = T.contiguous()
    upp = (mode != "lowest")
    if n <= K.SMALL_EIGH_MAX_K and neig <= K.SMALL_EIGH_MAX_P and n >= K.SMALL_EIGH_TRI_MIN_K and \
            K.small_eigh_tri_ok(n, neig, T.dtype):
        lam, Yt, flag = K.small_eigh(T, n, neig, uppest=upp, method="tri")
    else:
        lam, Yt, flag = K.small_eigh_big(T, n, neig, uppest=upp)
    X = Yt.transpose(1, 2)
    if int(flag.max().item()) != 0:                   # (rare) self-check failed somewhere: those members on the library
        bad = torch.nonzero(flag, as_tuple=False).flatten()
        l2, U2 = torch.linalg.eigh(T[bad])
        l2, U2 = take_eigpairs(l2, U2, neig, mode)
        lam = lam.clone()
        X = X.clone()
        lam[bad], X[bad] = l2, U2
    return lam.reshape(*bdims, neig), X.reshape(*bdims, n, neig)


def herm_partial_eigh(T, k, p, mode, counts=None):
    """Lowest / uppermost p eigenpairs of the Hermitian (B, >=k, >=k) complex T[:, :k, :k]: lam (B, p) real
    ascending, Y (B, k, p) complex.  Native kernel inside its range, members whose self-check fails redone on
    torch.linalg.eigh, the library beyond the range; `counts` ({"rr_native": .., "rr_library": ..}) counts the calls
    served each way (a call with any redone member counts as a library call)."""
    B = T.shape[0]
    if K.herm_eigh_ok(k, p):
        lam, Yt, flag = K.herm_eigh(T, k, p, uppest=(mode != "lowest"))
        Y = Yt.transpose(1, 2)
        if int(flag.max().item()) == 0:
            if counts is not None:
                counts["rr_native"] += 1
            return lam, Y
        bad = torch.nonzero(flag, as_tuple=False).flatten()
        l2, U2 = _library_eigh(T[bad, :k, :k], p, mode)
        lam, Y = lam.clone(), Y.clone()
        lam[bad], Y[bad] = l2, U2
    else:
        lam, Y = _library_eigh(T[:B, :k, :k], p, mode)
    if counts is not None:
        counts["rr_library"] += 1
    return lam, Y


def _library_eigh(T, p, mode):
    lam, U = torch.linalg.eigh(T)                     # (lower triangle, like the kernel)
    if mode == "lowest":
        return lam[..., :p].contiguous(), U[..., :p]
    return lam[..., -p:].contiguous(), U[..., -p:]


# ---- the two dtype backends

def cholqr_step(bufs, Mp, N, q, info, Wq=None, shift=False, symmetrise=False):
    """One real CholeskyQR step: G = <panel, Mp> of the q-row panel bufs[0] and its M-image Mp (the panel itself
    without M), G + shift * trace(G) I = R^T R when `shift`, every buffer of `bufs` <- its rows times R^-1.  Wq: the
    (B, q, q) home of R^-1 (default: a fresh one); the Cholesky flags land in `info` (sticky)."""
    panel = bufs[0]
    G = K.dense_mm(panel[:, :, :N], Mp[:, :, :N])
    if symmetrise:
        G = (G + G.transpose(1, 2)) * 0.5
    if shift:
        tr = torch.diagonal(G, dim1=-2, dim2=-1).sum(-1)
        G = G + (_shift_rel(N, q, panel.dtype) * tr)[:, None, None] * torch.eye(q, dtype=G.dtype, device=G.device)
    if Wq is None:
        Wq = torch.empty((panel.shape[0], q, q), dtype=panel.dtype, device=panel.device)
    K.panel_chol(G.contiguous(), Wq, info, q)
    for buf in bufs:
        K.panel_transform(buf, Wq, q)


class _BlockOps:
    """what both backends share: geometry, allocation, load / result, the Rayleigh-Ritz matrix.  `w` is the width of
    the caller's block, `kmax` the most rows a block is ever projected against (they size the scratch).  wide: the
    caller's Rayleigh-Ritz wants ALL w pairs of a block of any width (chebfsi), not the lowest few of a wider matrix:
    whether the native dense solvers serve that is decided here, once."""

    def __init__(self, Bt, N, w, dtype, device, wide):
        self.Bt, self.N, self.w, self.dtype, self.device = Bt, N, w, dtype, device
        self.wide, self.native = wide, not wide or self.eigh_native(w, w)
        self.rdtype = real_dtype(dtype)
        self.ld = self.ld_of(N)
        self.info = torch.zeros((Bt,), dtype=torch.int32, device=device)          # Cholesky flags (sticky)
        self.counts = {"rr_native": 0, "rr_library": 0}                           # eigh_lowest calls served each way
        self.small_eigh = "native"
        self._pc = None                                   # the Jacobi preconditioner's tables, made on first use

    def panel(self, rows):
        return torch.zeros((self.Bt, rows, self.ld), dtype=self.dtype, device=self.device)

    def load(self, P, V0p):
        P[:, :, :self.N].copy_(V0p)

    def result(self, X, neig, bdims):
        return X[:, :neig, :self.N].transpose(-2, -1).reshape(*bdims, self.N, neig)

    def rr_matrix(self, Pa, Pb, sign):
        """sign * the Hermitian part of Pa^H Pb, contiguous: the Rayleigh-Ritz matrix of Pb = A Pa"""
        T = self.gram(Pa, Pb)
        return ((T + T.transpose(1, 2).conj()) * (0.5 * sign)).contiguous()


class RealBlockOps(_BlockOps):
    """fp64 / fp32: zero-padded (Bt, rows, pad_len(N)) panels on the Davidson chain kernels"""
    ld_of = staticmethod(pad_len)

    def __init__(self, Bt, N, w, dtype, device, kmax=None, wide=False):
        super().__init__(Bt, N, w, dtype, device, wide)
        self.C = torch.empty((Bt * max(w, 32) * max(kmax or w, 32),), dtype=dtype, device=device)
        self.Wq = torch.empty((Bt * 32 * 32,), dtype=dtype, device=device)
        self.rmax = torch.zeros((Bt,), dtype=dtype, device=device)
        self.orth_g = torch.zeros((Bt,), dtype=dtype, device=device)
        self.st = torch.zeros((5,), dtype=torch.float64, device=device)

    def gram(self, Pa, Pb):
        """G[b, i, c] = <Pa_i, Pb_c>"""
        return K.dense_mm(Pa[:, :, :self.N], Pb[:, :, :self.N]).transpose(1, 2)

    def combine(self, P, C, out):
        """out[b, c, :] = sum_i C[b, i, c] P[b, i, :]"""
        K.lincomb(P, C, out, C.shape[1], C.shape[2], coef_layout="ac", alpha=1.0, beta=0.0)
        return out

    def orth(self, S, k0, q, passes, info, MS=None, opM=None, chunk=None):
        """rows [k0, k0 + q) of S (M-)orthonormal and (M-)orthogonal to rows [0, k0): `passes` passes of projection +
        CholeskyQR, the first shifted when there are several.  Without M one xk_davidson_orth call (which takes wide
        blocks in chunks by itself: `chunk` is the complex backend's); with M the rows of MS follow (M is applied once,
        then transformed alongside)."""
        N = self.N
        if MS is None:
            K.davidson_orth(S, N, k0, q, self.C, self.Wq, info, passes=passes)
            return
        W, MW = S[:, k0:k0 + q], MS[:, k0:k0 + q]
        opM.apply(W, MW)
        Wq = self.Wq[:self.Bt * q * q].view(self.Bt, q, q)
        for r in range(passes):
            if k0 > 0:
                C = K.dense_mm(MS[:, :k0, :N], W[:, :, :N])                   # C[b, c, a] = <M S_a, W_c>
                K.lincomb(S, C, W, k0, q, coef_layout="ca", alpha=-1.0, beta=1.0)
                K.lincomb(MS, C, MW, k0, q, coef_layout="ca", alpha=-1.0, beta=1.0)
            cholqr_step([W, MW], MW, N, q, info, Wq, shift=(r == 0 and passes > 1))

    def eigh_native(self, n, p):
        """do the native dense solvers serve p pairs of order n?  (K3t / K3g from order 8, the Jacobi kernel below)"""
        return (8 <= n and p <= EXACTEIG_NATIVE_MAX_P and K.small_eigh_big_ok(n, p, self.dtype)) or \
            (n < 8 and p <= K.SMALL_EIGH_MAX_P)

    def eigh_lowest(self, T, n, p):
        """(mu (Bt, p) ascending, Y (Bt, n, p)) of the symmetric (Bt, n, n) T on the native dense solvers; a `wide`
        block beyond `eigh_native`: all its pairs from the library"""
        if not self.native:
            self.small_eigh = "library"
            return torch.linalg.eigh(T)
        if n >= 8:
            return native_partial_eigh(T, p, "lowest")
        mu, Yt, _ = K.small_eigh(T, n, p)                                     # LDS Jacobi kernel (tiny blocks)
        return mu, Yt.transpose(1, 2)

    def status(self, X, w, resid, info, MX=None):
        """(max|resid|, Cholesky flag, guard max|X^T M X - I| of the first w rows of X): the ONE host read.  resid:
        (Bt,) maxima per member (None: self.rmax holds them already)"""
        if resid is not None:
            self.rmax.copy_(resid)
        K.ritz_guard(X, self.orth_g, w, self.ld, MX=MX)
        K.group_status(self.rmax, info, None, self.st, orth=self.orth_g)
        st = self.st.tolist()
        return st[0], st[1], st[4]

    def precond_diag(self, R, d):
        """R <- R / |d| (Jacobi; xk_diag_precond with a zero shift table)"""
        w = R.shape[1]
        if self._pc is None:
            self._pc = (d.abs().contiguous(), torch.zeros((self.Bt, w), dtype=self.dtype, device=self.device))
        K.diag_precond(R, self._pc[0], self._pc[1], w)


class ComplexBlockOps(_BlockOps):
    """complex128 / complex64: (Bt, rows, N) panels on the Hermitian Davidson kernels (xk_herm_*)"""
    ld_of = staticmethod(int)

    def __init__(self, Bt, N, w, dtype, device, kmax=None, wide=False):
        super().__init__(Bt, N, w, dtype, device, wide)
        self.eye = torch.eye(w, dtype=dtype, device=device)

    def gram(self, Pa, Pb):
        """G[b, i, c] = sum_n conj(Pa[b, i, n]) Pb[b, c, n]  (B, k, q): Pa^H Pb on K1 with Pa as the matrix"""
        return K.dense_mm_complex(Pa, Pb, conj_io=True).transpose(1, 2)

    def combine(self, P, C, out=None):
        """out[b, c, :] = sum_i C[b, i, c] P[b, i, :]  (B, q, N): the combination P C on K1"""
        res = K.dense_mm_complex(P, C.transpose(1, 2).contiguous(), adjoint=True, conj_io=True)
        return res if out is None else out.copy_(res)

    def orth_block(self, W, V, passes, info, shift_first, MW=None, MV=None, opM=None):
        """W (B, q, N) in place (M-)orthonormal and (M-)orthogonal to the rows of V (None: nothing before it): per pass
        the projection on K1 and xk_herm_cholqr, the first pass shifted when `shift_first`.  MW / MV: the M-images;
        MW is projected and transformed alongside, or, with `opM`, recomputed after every projection."""
        q = W.shape[1]
        for r in range(passes):
            if V is not None:
                C = self.gram(MV if MV is not None else V, W)
                W.sub_(self.combine(V, C))
                if MW is not None and opM is None:
                    MW.sub_(self.combine(MV, C))
            if opM is not None:
                opM.apply(W, MW)
            K.herm_cholqr(W, info, MW=MW, shift_rel=_shift_rel(self.N, q, self.rdtype) if (r == 0 and shift_first)
                          else 0.0)

    def orth(self, S, k0, q, passes, info, MS=None, opM=None, chunk=None):
        """rows [k0, k0 + q) of S (M-)orthonormal and (M-)orthogonal to rows [0, k0); with M the rows of MS follow (M
        is applied once).  The first pass is shifted when there are several.  chunk: blocks wider than the `chunk`
        vectors of xk_herm_cholqr are taken that many rows at a time, like xk_davidson_orth takes real ones: every
        chunk is projected against the rows before it and orthonormalised among itself, the later ones at least
        twice — block Gram-Schmidt with CholeskyQR inside the blocks."""
        if MS is not None:
            opM.apply(S[:, k0:k0 + q], MS[:, k0:k0 + q])
        step = chunk or q
        for off in range(k0, k0 + q, step):
            qc = min(step, k0 + q - off)
            np_ = passes if chunk is None else max(1 if off == k0 else 2, passes)
            self.orth_block(S[:, off:off + qc], S[:, :off] if off > 0 else None, np_, info, np_ > 1,
                            MW=MS[:, off:off + qc] if MS is not None else None,
                            MV=MS[:, :off] if MS is not None and off > 0 else None)

    def eigh_native(self, n, p):
        """xk_herm_eigh returns up to 16 pairs from either end of the spectrum: blocks of up to 32 vectors get all
        their pairs from two native calls (the lowest 16 and the uppermost p - 16); wider ones go to the library"""
        return p <= 2 * K.HERM_EIGH_MAX_P and n <= K.HERM_EIGH_MAX_K

    def eigh_lowest(self, T, n, p):
        """(mu (Bt, p) ascending, Y (Bt, n, p)) of the Hermitian (Bt, n, n) T: `herm_partial_eigh` (the library beyond
        16 pairs).  A `wide` block gets all its pairs: 17 .. 32 from two native calls and the seam test, and beyond
        `eigh_native` from the library."""
        if not self.wide or p <= K.HERM_EIGH_MAX_P:
            res = herm_partial_eigh(T, n, p, "lowest", self.counts)
        elif self.native:
            res = self._eigh_two_calls(T, n, p)
        else:
            self.counts["rr_library"] += 1
            res = torch.linalg.eigh(T)
        if self.counts["rr_library"]:
            self.small_eigh = "library"
        return res

    def _eigh_two_calls(self, T, n, p):
        P16 = K.HERM_EIGH_MAX_P
        mu_lo, Y_lo = herm_partial_eigh(T, n, P16, "lowest", self.counts)
        mu_hi, Y_hi = herm_partial_eigh(T, n, p - P16, "uppest", self.counts)
        # The seam.  xk_herm_eigh orthogonalises its vectors only within one call: vector 16 and vector 17 come out
        # orthogonal to about eps |T| / gap.  Where that could reach the guard's GOOD level — eigenvalues 16 and 17 of
        # some member closer than eps |T| / GUARD_GOOD — the call is served by the library, whose vectors are orthonormal
        # whatever the gaps (one more host read, only for blocks of 17 .. 32 vectors).  Otherwise what is left across
        # the seam is removed by one projection of the upper set against the lower and a renormalisation, a
        # perturbation of the upper vectors below GUARD_GOOD.
        scale = torch.maximum(mu_lo[:, 0].abs(), mu_hi[:, -1].abs())
        tol = torch.finfo(self.rdtype).eps / GUARD_GOOD[self.rdtype]
        if bool(((mu_hi[:, 0] - mu_lo[:, -1]) <= tol * scale).any()):
            self.counts["rr_library"] += 1
            return torch.linalg.eigh(T)
        Y_hi = Y_hi - torch.matmul(Y_lo, torch.matmul(Y_lo.transpose(1, 2).conj(), Y_hi))
        Y_hi = Y_hi / torch.linalg.vector_norm(Y_hi, dim=1, keepdim=True)
        return torch.cat((mu_lo, mu_hi), dim=-1), torch.cat((Y_lo, Y_hi), dim=-1)

    def status(self, X, w, resid, info, MX=None):
        """(max|resid|, Cholesky flag, guard max|X^H M X - I| of the first w rows of X): the ONE host read.  resid:
        the maximum on the device, or (Bt,) maxima per member"""
        X = X[:, :w]
        guard = (self.gram(X, MX[:, :w] if MX is not None else X) - self.eye).abs().max().to(torch.float64)
        st = torch.stack((resid if resid.dim() == 0 else resid.max(), info.max().to(torch.float64), guard)).tolist()
        return st[0], st[1], st[2]

    def precond_diag(self, R, d):
        """R <- R / |d| (Jacobi): the real kernel xk_diag_precond on the interleaved storage, every diagonal entry
        taken twice, with a zero shift table"""
        w = R.shape[1]
        if self._pc is None:
            self._pc = (d.abs().to(self.rdtype).repeat_interleave(2, dim=-1).contiguous(),
                        torch.zeros((self.Bt, w), dtype=self.rdtype, device=self.device))
        Rr = torch.view_as_real(R).reshape(R.shape[0], R.shape[1], 2 * R.shape[2])
        K.diag_precond(Rr, self._pc[0], self._pc[1], w)


def block_ops(Bt, N, w, dtype, device, **kw):
    """the backend of `dtype`"""
    return (ComplexBlockOps if dtype.is_complex else RealBlockOps)(Bt, N, w, dtype, device, **kw)
