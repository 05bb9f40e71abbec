"""-m gpu: the CSR operator on the HIP kernels — xk_csr_mm / its transpose / xk_csr_sddmm against a float64
restatement with per-entry bounds, untouched pads, determinism, and the solvers through the "csr" panel kind."""
import pytest
import torch
import xitorch_amd as xa
from xitorch_amd import kernels as K
from xitorch_amd.linop import SparseLinearOperator
from xitorch_amd.linalg import symeig, solve, svd
from xitorch_amd.linalg._panel import PanelOperator
from xitorch_amd.linalg.native_eig import davidson

pytestmark = pytest.mark.gpu
SENT = 7.25e5          # sentinel in pads / columns outside the written range


def _pattern(kind, M, N, seed):
    """host (crow, col) int64 for the named pattern kinds"""
    g = torch.Generator().manual_seed(seed)
    if kind == "diag":
        n = min(M, N)
        crow = torch.cat([torch.arange(n + 1), torch.full((M - n,), n)])
        return crow, torch.arange(n)
    if kind == "fullrow":            # one full row, the rest short
        lens = torch.randint(0, 4, (M,), generator=g)
        lens[M // 3] = N
    elif kind == "powerlaw":
        lens = (N * torch.rand(M, generator=g) ** 6).long().clamp(max=N)
    elif kind == "empty":
        lens = torch.randint(0, 9, (M,), generator=g)
        lens[::3] = 0
    else:                            # "random" with duplicates and unsorted columns
        lens = torch.randint(20, 40, (M,), generator=g)
    crow = torch.zeros(M + 1, dtype=torch.int64)
    crow[1:] = torch.cumsum(lens, 0)
    col = torch.randint(0, N, (int(crow[-1]),), generator=g)
    if kind == "fullrow":
        r = M // 3
        col[crow[r]:crow[r + 1]] = torch.randperm(N, generator=g)
    if col.numel() > 2:
        col[1::7] = col[0::7][:col[1::7].numel()]          # duplicates
    return crow, col


def _check_mm(crow, col, vals, X, Y, M, N, trans, dtype):
    rows = torch.repeat_interleave(torch.arange(M), crow[1:] - crow[:-1])
    src, dst, nout = (rows, col, N) if trans else (col, rows, M)
    terms = vals.double().unsqueeze(1) * X.double()[:, :, src]           # (B, C, nnz)
    B, C = X.shape[:2]
    ref = torch.zeros(B, C, nout, dtype=torch.float64).index_add(2, dst, terms)
    mag = torch.zeros(B, C, nout, dtype=torch.float64).index_add(2, dst, terms.abs())
    cnt = torch.zeros(nout, dtype=torch.float64).index_add(0, dst, torch.ones(dst.numel(), dtype=torch.float64))
    u = torch.finfo(dtype).eps / 2
    bound = 8 * u * (cnt + 2) * mag + 1e-300
    err = (Y.double() - ref).abs()
    assert bool((err <= bound).all()), float((err / bound).max())


def _panel(B, C, n, ld, dtype, dev, g, sB=None):
    """strided (B, C, n) view into a sentinel-filled buffer (pitch ld, batch pitch sB)"""
    sB = sB or C * ld + 5
    buf = torch.full((B * sB + 8,), SENT, dtype=dtype, device=dev)
    view = buf.as_strided((B, C, n), (sB, ld, 1), 3)
    view.copy_(torch.randn(B, C, n, generator=g, dtype=torch.float64).to(dtype))
    return buf, view


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("kind", ["random", "empty", "diag", "fullrow", "powerlaw"])
def test_csr_mm_vs_float64(dev, dtype, kind):
    g = torch.Generator().manual_seed(5)
    for (M, N) in ((1003, 1003), (515, 1301), (1301, 203)):
        crow, col = _pattern(kind, M, N, seed=M + N)
        for B, bcast in ((1, False), (5, False), (5, True)):
            vals = torch.randn(1 if bcast else B, col.numel(), generator=g, dtype=torch.float64).to(dtype)
            A = SparseLinearOperator(crow.to(dev), col.to(dev), (vals[0] if bcast else vals).to(dev),
                                     (B, M, N) if bcast else (M, N))
            pat = A._pattern
            for trans in (False, True):
                nin, nout = (M, N) if trans else (N, M)
                for C in range(1, 18) if (M, N) == (1003, 1003) else (1, 6, 9):
                    _, X = _panel(B, C, nin, nin + 3, dtype, dev, g)
                    ybuf, Y = _panel(B, C, nout, nout + 11, dtype, dev, g)
                    before = ybuf.clone()
                    K.csr_mm(pat, vals.to(dev), X, out=Y, trans=trans)
                    _check_mm(crow, col, vals.cpu().expand(B, -1), X.cpu(), Y.cpu(), M, N, trans, dtype)
                    # everything outside Y's (B, C, nout) entries keeps its sentinel
                    mask = torch.ones_like(ybuf, dtype=torch.bool)
                    mask.as_strided(Y.shape, Y.stride(), Y.storage_offset()).fill_(False)
                    assert torch.equal(ybuf[mask], before[mask])


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_csr_mm_long_rows_in_segments(dev, dtype):
    """rows longer than one segment (xk_csr_seg_len entries): full rows of 20011 and a power-law tail"""
    g = torch.Generator().manual_seed(8)
    seg = int(K.fn("xk_csr_seg_len")())
    for kind, (M, N) in (("fullrow", (301, 20011)), ("powerlaw", (97, 3 * seg + 5))):
        crow, col = _pattern(kind, M, N, seed=N)
        lens = crow[1:] - crow[:-1]
        assert int(lens.max()) > 2 * seg
        for B, bcast in ((1, False), (3, False), (3, True)):
            vals = torch.randn(1 if bcast else B, col.numel(), generator=g, dtype=torch.float64).to(dtype)
            A = SparseLinearOperator(crow.to(dev), col.to(dev), (vals[0] if bcast else vals).to(dev),
                                     (B, M, N) if bcast else (M, N))
            assert A._pattern.csr().nseg > A._pattern.csr().bin_counts[3]
            for trans in (False, True):
                nin, nout = (M, N) if trans else (N, M)
                for C in (1, 6, 9):
                    _, X = _panel(B, C, nin, nin + 3, dtype, dev, g)
                    ybuf, Y = _panel(B, C, nout, nout + 11, dtype, dev, g)
                    before = ybuf.clone()
                    K.csr_mm(A._pattern, vals.to(dev), X, out=Y, trans=trans)
                    _check_mm(crow, col, vals.cpu().expand(B, -1), X.cpu(), Y.cpu(), M, N, trans, dtype)
                    mask = torch.ones_like(ybuf, dtype=torch.bool)
                    mask.as_strided(Y.shape, Y.stride(), Y.storage_offset()).fill_(False)
                    assert torch.equal(ybuf[mask], before[mask])
                    Y2 = torch.empty_like(Y)
                    K.csr_mm(A._pattern, vals.to(dev), X, out=Y2, trans=trans)
                    assert torch.equal(Y2, Y)


def test_csr_kernels_are_deterministic(dev):
    g = torch.Generator().manual_seed(9)
    crow, col = _pattern("powerlaw", 4099, 4099, seed=1)
    vals = torch.randn(3, col.numel(), generator=g, dtype=torch.float64).to(dev)
    A = SparseLinearOperator(crow.to(dev), col.to(dev), vals, (4099, 4099))
    X = torch.randn(3, 6, 4099, generator=g, dtype=torch.float64).to(dev)
    for fn in (lambda: K.csr_mm(A._pattern, vals, X), lambda: K.csr_mm(A._pattern, vals, X, trans=True),
               lambda: K.csr_sddmm(A._pattern, X, X), lambda: K.csr_sddmm(A._pattern, X.reshape(1, 18, 4099),
                                                                          X.reshape(1, 18, 4099))):
        outs = [fn().clone() for _ in range(3)]
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[1], outs[2])


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_csr_sddmm_vs_torch(dev, dtype):
    g = torch.Generator().manual_seed(4)
    M, N = 777, 1201
    crow, col = _pattern("empty", M, N, seed=2)
    A = SparseLinearOperator(crow.to(dev), col.to(dev), torch.ones(col.numel(), dtype=dtype, device=dev), (M, N))
    rows = torch.repeat_interleave(torch.arange(M), crow[1:] - crow[:-1])
    B, C = 4, 3
    _, U = _panel(B, C, M, M + 5, dtype, dev, g)
    _, W = _panel(B, C, N, N + 1, dtype, dev, g)
    tol = 1e-12 if dtype == torch.float64 else 1e-4
    ref = (U.cpu().double()[:, :, rows] * W.cpu().double()[:, :, col]).sum(1)      # (B, nnz)
    G = K.csr_sddmm(A._pattern, U, W)
    assert torch.allclose(G.cpu().double(), ref, atol=tol, rtol=tol)
    # values broadcast over the batch: the batch folded into the columns, summed inside the kernel
    Gs = K.csr_sddmm(A._pattern, U.contiguous().reshape(1, B * C, M), W.contiguous().reshape(1, B * C, N))
    assert Gs.shape == (1, col.numel()) and torch.allclose(Gs.cpu().double()[0], ref.sum(0), atol=4 * tol, rtol=tol)
    # transposed apply: the operands swap (U lives on the columns, W on the rows)
    _, Wt = _panel(B, C, M, M, dtype, dev, g)
    _, Ut = _panel(B, C, N, N, dtype, dev, g)
    reft = (Wt.cpu().double()[:, :, rows] * Ut.cpu().double()[:, :, col]).sum(1)
    assert torch.allclose(K.csr_sddmm(A._pattern, Wt, Ut).cpu().double(), reft, atol=tol, rtol=tol)


def _sym_sparse(N, seed, batch=(), dtype=torch.float64, shift=0.0):
    """symmetric sparse (random pattern + its transpose + diagonal), as (crow, col, vals) host tensors"""
    g = torch.Generator().manual_seed(seed)
    i = torch.randint(0, N, (4 * N,), generator=g)
    j = torch.randint(0, N, (4 * N,), generator=g)
    ii = torch.cat([i, j, torch.arange(N)])
    jj = torch.cat([j, i, torch.arange(N)])
    w = torch.rand((*batch, 4 * N), generator=g, dtype=torch.float64) - 0.5
    d = shift + torch.linspace(1.0, 3.0, N, dtype=torch.float64).expand(*batch, N) + \
        0.1 * torch.rand((*batch, N), generator=g, dtype=torch.float64)
    v = torch.cat([w, w, d], dim=-1)
    order = torch.sort(ii, stable=True).indices
    crow = torch.zeros(N + 1, dtype=torch.int64)
    crow[1:] = torch.cumsum(torch.bincount(ii, minlength=N), 0)
    return crow, jj[order], v[..., order].to(dtype)


@pytest.mark.parametrize("dtype,tol", [(torch.float64, 1e-10), (torch.float32, 1e-4)])
@pytest.mark.parametrize("mode", ["lowest", "uppest"])
@pytest.mark.parametrize("withM", [False, True])
@pytest.mark.parametrize("precond", [None, "diag"])
def test_davidson_on_csr_matches_exacteig(dev, dtype, tol, mode, withM, precond):
    N = 400
    crow, col, v = _sym_sparse(N, seed=3, batch=(2,), dtype=dtype)
    A = SparseLinearOperator(crow.to(dev), col.to(dev), v.to(dev), (2, N, N), is_hermitian=True)
    Mop = None
    Md = None
    if withM:
        cm, colm, vm = _sym_sparse(N, seed=8, dtype=dtype, shift=3.0)
        vm = torch.where(torch.repeat_interleave(torch.arange(N), cm[1:] - cm[:-1]) == colm, vm, 0.05 * vm)
        Mop = SparseLinearOperator(cm.to(dev), colm.to(dev), vm.to(dev), (N, N), is_hermitian=True)
        Md = Mop.fullmatrix().cpu().double()
    Ad = A.fullmatrix().cpu().double()
    tr = {}
    ev, X = davidson(A, 4, mode, Mop, min_eps=1e-9 if dtype == torch.float64 else 1e-4, precond=precond, trace=tr)
    assert tr["panel_kernel"] == "csr"
    if Md is None:
        ref = torch.linalg.eigvalsh(Ad)
    else:
        Lc = torch.linalg.cholesky(Md)
        Li = torch.linalg.inv(Lc)
        ref = torch.linalg.eigvalsh(Li @ Ad @ Li.transpose(-2, -1))
    ref = ref[..., :4] if mode == "lowest" else ref[..., -4:]
    scale = float(ref.abs().max())
    assert (ev.cpu().double().sort(-1).values - ref.sort(-1).values).abs().max() <= tol * scale


@pytest.mark.parametrize("method", ["cg", "bicgstab", "gmres"])
def test_krylov_on_csr_batch(dev, method, monkeypatch):
    N = 600
    crow, col, v = _sym_sparse(N, seed=6, batch=(3,), shift=2.0)
    A = SparseLinearOperator(crow.to(dev), col.to(dev), v.to(dev), (3, N, N), is_hermitian=True)
    assert PanelOperator(A, [3], 3, N).kind == "csr"
    calls = [0]
    real = K.csr_mm

    def counted(*a, **k):
        calls[0] += 1
        return real(*a, **k)
    monkeypatch.setattr(K, "csr_mm", counted)
    Bm = torch.randn(3, N, 2, dtype=torch.float64)
    x = solve(A, Bm.to(dev), method=method, rtol=1e-11, atol=1e-14)
    ref = torch.linalg.solve(A.fullmatrix().cpu(), Bm)
    assert calls[0] > 0
    assert (x.cpu() - ref).abs().max() <= 1e-8 * ref.abs().max()


def test_no_device_call_reaches_host_drivers(dev):
    from xitorch_amd.linalg import host_eig, host_krylov
    N = 300
    crow, col, v = _sym_sparse(N, seed=2, batch=(2,), shift=2.0)
    A = SparseLinearOperator(crow.to(dev), col.to(dev), v.to(dev), (2, N, N), is_hermitian=True)
    before = (dict(host_krylov.calls), dict(host_eig.calls))
    symeig(A, 3, "lowest", method="davidson", min_eps=1e-8)
    for meth in ("cg", "bicgstab", "gmres"):
        solve(A, torch.randn(2, N, 1, dtype=torch.float64, device=dev), method=meth, rtol=1e-9)
    assert (dict(host_krylov.calls), dict(host_eig.calls)) == before


def test_solve_backward_matches_dense(dev):
    N = 200
    crow, col, v = _sym_sparse(N, seed=12, shift=2.0)
    rows = torch.repeat_interleave(torch.arange(N), crow[1:] - crow[:-1])
    vals = v.to(dev).requires_grad_()
    Bm = torch.randn(N, 2, dtype=torch.float64, device=dev, requires_grad=True)
    A = SparseLinearOperator(crow.to(dev), col.to(dev), vals, (N, N), is_hermitian=True)
    bck = dict(method="cg", rtol=1e-13, atol=1e-15)
    x = solve(A, Bm, method="cg", rtol=1e-12, atol=1e-14, bck_options=bck)
    gv, gb = torch.autograd.grad((x ** 2).sum(), (vals, Bm))
    D = A.fullmatrix().detach().clone().requires_grad_()
    B2 = Bm.detach().clone().requires_grad_()
    x2 = solve(xa.LinearOperator.m(D, True), B2, method="cg", rtol=1e-12, atol=1e-14, bck_options=bck)
    gD, gb2 = torch.autograd.grad((x2 ** 2).sum(), (D, B2))
    # d/dvals[k] = dL/dA[row_k, col_k]: the dense gradient sampled at the pattern (duplicates share it)
    gref = gD[rows.to(dev), col.to(dev)]
    assert torch.allclose(gv, gref, atol=1e-8, rtol=1e-6)
    assert torch.allclose(gb, gb2, atol=1e-9, rtol=1e-7)


@pytest.mark.parametrize("vbatch,xbatch", [((), (4,)), ((3,), (3,)), ((3,), (2, 3)), ((2, 1), (2, 3))])
@pytest.mark.parametrize("trans", [False, True])
def test_native_autograd_matches_torch_expression(dev, vbatch, xbatch, trans):
    """_CsrMM / _CsrGrad (first and second order) against csr_apply_torch on the device: batched, broadcast and
    transposed applies"""
    from xitorch_amd.linop import csr_apply_torch
    M, N = 517, 389
    crow, col = _pattern("empty", M, N, seed=31)
    g = torch.Generator().manual_seed(2)
    v0 = torch.randn((*vbatch, col.numel()), generator=g, dtype=torch.float64).to(dev)
    x0 = torch.randn((*xbatch, M if trans else N, 3), generator=g, dtype=torch.float64).to(dev)
    w = torch.randn((*torch.broadcast_shapes(vbatch, xbatch), N if trans else M, 3), generator=g,
                    dtype=torch.float64).to(dev)
    crow_d, col_d = crow.to(dev), col.to(dev)
    outs = []
    for native in (True, False):
        v = v0.clone().requires_grad_()
        x = x0.clone().requires_grad_()
        if native:
            A = SparseLinearOperator(crow_d, col_d, v, (*vbatch, M, N))
            y = A.rmm(x) if trans else A.mm(x)
        else:
            y = csr_apply_torch(crow_d, col_d, v, x, M, N, trans)
        gv, gx = torch.autograd.grad((y * w).sum(), (v, x), create_graph=True)
        ggv, ggx = torch.autograd.grad((gv ** 2).sum() + (gx ** 2).sum(), (v, x))
        outs.append((y, gv, gx, ggv, ggx))
    for a, b in zip(*outs):
        assert a.shape == b.shape and torch.allclose(a, b, rtol=1e-11, atol=1e-11)


def test_symeig_backward_wrt_values(dev):
    N = 160
    crow, col, v = _sym_sparse(N, seed=13)
    rows = torch.repeat_interleave(torch.arange(N), crow[1:] - crow[:-1])
    vals = v.to(dev).requires_grad_()
    A = SparseLinearOperator(crow.to(dev), col.to(dev), vals, (N, N), is_hermitian=True)
    ev, X = symeig(A, 3, "lowest", method="davidson", min_eps=1e-11)
    gv, = torch.autograd.grad(ev.sum(), (vals,))
    # d lambda / dA = x x^T, sampled at the pattern
    ev_ref, V = torch.linalg.eigh(A.fullmatrix().detach().cpu())
    G = (V[:, :3] @ V[:, :3].T)
    gref = G[rows, col]
    assert torch.allclose(gv.cpu(), gref, atol=1e-7)


def test_svd_of_rectangular_csr(dev):
    M, N = 300, 120
    crow, col = _pattern("random", M, N, seed=21)
    g = torch.Generator().manual_seed(0)
    vals = torch.randn(col.numel(), generator=g, dtype=torch.float64)
    A = SparseLinearOperator(crow.to(dev), col.to(dev), vals.to(dev), (M, N))
    u, s, vh = svd(A, 4, "uppest", method="davidson", min_eps=1e-10)
    ref = torch.linalg.svdvals(A.fullmatrix().cpu())[:4]
    assert torch.allclose(s.cpu().sort(descending=True).values, ref, rtol=1e-9)


# ------------------------------------------------------------------------------------------ at size
def _apply_rot(x, start, c, s):
    """pairs (start+2m, start+2m+1) rotated by (c_m, s_m) along the last dim"""
    n = x.shape[-1]
    npair = (n - start) // 2
    a = x[..., start:start + 2 * npair:2]
    b = x[..., start + 1:start + 2 * npair:2]
    cc, ss = c[:npair], s[:npair]
    y = x.clone()
    y[..., start:start + 2 * npair:2] = cc * a - ss * b
    y[..., start + 1:start + 2 * npair:2] = ss * a + cc * b
    return y


def rotated_diagonal(N, dev, seed=17):
    """A = P Q D Q^T P^T, Q = G2 G1 (2x2 rotations at angles <= 0.3 on (0,1),(2,3).. and (1,2),(3,4)..), P a random
    permutation: spectrum exactly d, at most 6 entries per row.  -> (SparseLinearOperator, d)"""
    g = torch.Generator(device=dev).manual_seed(seed)
    d = 1.0 + 0.25 * torch.arange(N, device=dev, dtype=torch.float64)
    t1 = 0.3 * torch.rand(N // 2, generator=g, device=dev, dtype=torch.float64)
    t2 = 0.3 * torch.rand(N // 2, generator=g, device=dev, dtype=torch.float64)
    c1, s1, c2, s2 = t1.cos(), t1.sin(), t2.cos(), t2.sin()
    Q = lambda x: _apply_rot(_apply_rot(x, 0, c1, s1), 1, c2, s2)
    Qt = lambda x: _apply_rot(_apply_rot(x, 1, c2, -s2), 0, c1, -s1)
    # Q D Q^T has half-bandwidth 3: probe it with 7 comb vectors
    ar = torch.arange(N, device=dev)
    rows, cols, vals = [], [], []
    for r in range(7):
        y = Q(d * Qt((ar % 7 == r).double()))
        for o in range(-3, 4):
            i = ar[(ar + o >= 0) & (ar + o < N) & ((ar + o) % 7 == r)]
            v = y[i]
            keep = v != 0
            rows.append(i[keep])
            cols.append(i[keep] + o)
            vals.append(v[keep])
    rows, cols, vals = torch.cat(rows), torch.cat(cols), torch.cat(vals)
    perm = torch.randperm(N, generator=g, device=dev)
    pr, pc = perm[rows], perm[cols]
    order = torch.sort(pr, stable=True).indices
    crow = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    crow[1:] = torch.cumsum(torch.bincount(pr, minlength=N), 0)
    assert int((crow[1:] - crow[:-1]).max()) <= 6
    return SparseLinearOperator(crow, pc[order], vals[order], (N, N), is_hermitian=True), d


def lowest_diagonal_start(A, k):
    """Davidson's classical start block: unit vectors at the k smallest diagonal entries (the diagonal correction
    refines toward eigenvalues near the current Ritz values, so a random start on a spectrum spread over [1, N/4]
    locks onto interior ones)"""
    N = A.shape[-1]
    dA = PanelOperator(A, [], 1, N).diagonal()[0]
    V0 = torch.zeros(N, k, dtype=dA.dtype, device=dA.device)
    V0[dA.argsort()[:k], torch.arange(k, device=dA.device)] = 1.0
    return V0


def test_davidson_rotated_diagonal_at_size(dev):
    A, d = rotated_diagonal(1 << 22, dev)
    tr = {}
    ev, X = davidson(A, 6, "lowest", min_eps=1e-9, precond="diag", V0=lowest_diagonal_start(A, 12), max_niter=200,
                     trace=tr)
    assert tr["panel_kernel"] == "csr"
    ref = d[:6]
    assert (ev - ref).abs().max().item() <= 1e-10 * float(ref.abs().max())
    R = A.mm(X) - X * ev.unsqueeze(-2)
    assert R.abs().max().item() <= 1e-8
    G = X.transpose(-2, -1) @ X
    assert (G - torch.eye(6, dtype=G.dtype, device=dev)).abs().max().item() <= 1e-9


def poisson7(n, dev, dtype=torch.float64):
    """3-D 7-point Laplacian (Dirichlet) on an n^3 grid as CSR, columns ascending in each row"""
    N = n ** 3
    ar = torch.arange(N, device=dev)
    z, y, x = ar // (n * n), (ar // n) % n, ar % n
    cols, vals, ok = [], [], []
    for dz, dy, dx in ((-1, 0, 0), (0, -1, 0), (0, 0, -1), (0, 0, 0), (0, 0, 1), (0, 1, 0), (1, 0, 0)):
        valid = (z + dz >= 0) & (z + dz < n) & (y + dy >= 0) & (y + dy < n) & (x + dx >= 0) & (x + dx < n)
        cols.append(ar + dz * n * n + dy * n + dx)
        vals.append(torch.full((N,), 6.0 if (dz, dy, dx) == (0, 0, 0) else -1.0, dtype=dtype, device=dev))
        ok.append(valid)
    ok = torch.stack(ok, 1)
    col = torch.stack(cols, 1)[ok].to(torch.int32)
    val = torch.stack(vals, 1)[ok]
    crow = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    crow[1:] = torch.cumsum(ok.sum(1), 0)
    return crow, col, val


def test_cg_poisson7_at_size(dev):
    n = 256
    crow, col, val = poisson7(n, dev)
    A = SparseLinearOperator(crow, col, val, (n ** 3, n ** 3), is_hermitian=True)
    h = torch.arange(n ** 3, device=dev)
    xs = torch.sin(0.01 * (h % n).double()) + torch.cos(0.02 * ((h // n) % n).double()) * (h // (n * n)).double() / n
    b = A.mv(xs).unsqueeze(-1)
    x = solve(A, b, method="cg", rtol=1e-8, atol=0.0, max_niter=4000)
    r = (b - A.mm(x)).norm() / b.norm()
    assert r.item() <= 2e-8
    assert ((x[:, 0] - xs).norm() / xs.norm()).item() <= 1e-3
