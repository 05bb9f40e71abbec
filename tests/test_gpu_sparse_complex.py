"""-m gpu: complex CSR operators on the HIP kernels — xk_csr_mm_c128 / _c64 (plain and adjoint) and
xk_csr_sddmm_c128 / _c64 against a complex128 restatement with per-entry bounds, untouched pads, determinism, the
autograd rules against the torch expression, and the solvers through the "csr" panel kind without one call of
csr_apply_torch."""
import pytest
import torch
import xitorch_amd as xa
from xitorch_amd import kernels as K
from xitorch_amd import linop
from xitorch_amd.linop import SparseLinearOperator
from xitorch_amd.linalg import symeig, solve, svd
from xitorch_amd.linalg._panel import PanelOperator
from xitorch_amd.linalg.native_eig import davidson

pytestmark = pytest.mark.gpu
SENT = complex(7.25e5, -3.5e5)          # sentinel in pads / columns outside the written range
c128, c64 = torch.complex128, torch.complex64
CDTYPES = [c128, c64]


def _pattern(kind, M, N, seed):
    """host (crow, col) int64 for the named pattern kinds (the shapes of tests/test_gpu_sparse.py)"""
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


def _crandn(g, *shape, dtype=c128):
    """complex normal draws, rounded to `dtype`"""
    return torch.complex(torch.randn(*shape, generator=g, dtype=torch.float64),
                         torch.randn(*shape, generator=g, dtype=torch.float64)).to(dtype)


def _l1(z):
    return z.real.abs() + z.imag.abs()


def _check_mm(crow, col, vals, X, Y, M, N, trans, dtype):
    """per output entry, real and imaginary part separately: |err| <= 8 u (cnt + 2) mag + 1e-300 with
    mag = sum_k (|Re v_k| + |Im v_k|) (|Re x_k| + |Im x_k|): every component of a complex product is a 2-term sum of
    real products, each bounded by that magnitude, so the real test's bound carries over with it"""
    rows = torch.repeat_interleave(torch.arange(M), crow[1:] - crow[:-1])
    src, dst, nout = (rows, col, N) if trans else (col, rows, M)
    v = vals.to(c128)
    if trans:
        v = v.conj().resolve_conj()
    xg = X.to(c128)[:, :, src]
    terms = v.unsqueeze(1) * xg                                          # (B, C, nnz)
    B, C = X.shape[:2]
    ref = torch.zeros(B, C, nout, dtype=c128).index_add(2, dst, terms)
    mag = torch.zeros(B, C, nout, dtype=torch.float64).index_add(2, dst, _l1(v).unsqueeze(1) * _l1(xg))
    cnt = torch.zeros(nout, dtype=torch.float64).index_add(0, dst, torch.ones(dst.numel(), dtype=torch.float64))
    u = torch.finfo(dtype).eps / 2                                       # unit roundoff of the component type
    bound = 8 * u * (cnt + 2) * mag + 1e-300
    err = Y.to(c128) - ref
    worst = max(float((err.real.abs() / bound).max()), float((err.imag.abs() / bound).max()))
    assert bool((err.real.abs() <= bound).all()) and bool((err.imag.abs() <= bound).all()), worst
    return worst


def _panel(B, C, n, ld, dtype, dev, g, sB=None):
    """strided (B, C, n) view into a sentinel-filled buffer (pitch ld, batch pitch sB)"""
    sB = sB or C * ld + 5
    buf = torch.full((B * sB + 8,), SENT, dtype=dtype, device=dev)
    view = buf.as_strided((B, C, n), (sB, ld, 1), 3)
    view.copy_(_crandn(g, B, C, n, dtype=dtype))
    return buf, view


def _pads_untouched(ybuf, before, Y):
    mask = torch.ones(ybuf.shape, dtype=torch.bool, device=ybuf.device)
    mask.as_strided(Y.shape, Y.stride(), Y.storage_offset()).fill_(False)
    return torch.equal(torch.view_as_real(ybuf)[mask], torch.view_as_real(before)[mask])


# ------------------------------------------------------------------------------------------ 1. per-entry product
@pytest.mark.parametrize("dtype", CDTYPES)
@pytest.mark.parametrize("kind", ["random", "empty", "diag", "fullrow", "powerlaw"])
def test_csr_mm_complex_vs_complex128(dev, dtype, kind):
    g = torch.Generator().manual_seed(5)
    worst = 0.0
    for (M, N) in ((1003, 1003), (515, 1301), (1301, 203)):
        crow, col = _pattern(kind, M, N, seed=M + N)
        for B, bcast in ((1, False), (5, False), (5, True)):
            vals = _crandn(g, 1 if bcast else B, col.numel(), dtype=dtype)
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
                    worst = max(worst, _check_mm(crow, col, vals.cpu().expand(B, -1), X.cpu(), Y.cpu(), M, N, trans,
                                                 dtype))
                    # everything outside Y's (B, C, nout) entries keeps its sentinel
                    assert _pads_untouched(ybuf, before, Y)
    print("worst err / bound (%s, %s): %.4f" % (kind, dtype, worst))


# ------------------------------------------------------------------------------------------ 2. long rows
@pytest.mark.parametrize("dtype", CDTYPES)
def test_csr_mm_complex_long_rows_in_segments(dev, dtype):
    """rows longer than one segment (xk_csr_seg_len entries): full rows of 20011 and a power-law tail"""
    g = torch.Generator().manual_seed(8)
    seg = int(K.fn("xk_csr_seg_len")())
    for kind, (M, N) in (("fullrow", (301, 20011)), ("powerlaw", (97, 3 * seg + 5))):
        crow, col = _pattern(kind, M, N, seed=N)
        lens = crow[1:] - crow[:-1]
        assert int(lens.max()) > 2 * seg
        for B, bcast in ((1, False), (3, False), (3, True)):
            vals = _crandn(g, 1 if bcast else B, col.numel(), dtype=dtype)
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
                    assert _pads_untouched(ybuf, before, Y)
                    Y2 = torch.empty_like(Y)
                    K.csr_mm(A._pattern, vals.to(dev), X, out=Y2, trans=trans)
                    assert torch.equal(torch.view_as_real(Y2), torch.view_as_real(Y.contiguous()))


# ------------------------------------------------------------------------------------------ 3. determinism
@pytest.mark.parametrize("dtype", CDTYPES)
def test_complex_csr_kernels_are_deterministic(dev, dtype):
    g = torch.Generator().manual_seed(9)
    crow, col = _pattern("powerlaw", 4099, 4099, seed=1)
    vals = _crandn(g, 3, col.numel(), dtype=dtype).to(dev)
    A = SparseLinearOperator(crow.to(dev), col.to(dev), vals, (4099, 4099))
    X = _crandn(g, 3, 6, 4099, dtype=dtype).to(dev)
    for fn in (lambda: K.csr_mm(A._pattern, vals, X), lambda: K.csr_mm(A._pattern, vals, X, trans=True),
               lambda: K.csr_sddmm(A._pattern, X, X), lambda: K.csr_sddmm(A._pattern, X.reshape(1, 18, 4099),
                                                                          X.reshape(1, 18, 4099))):
        outs = [torch.view_as_real(fn().clone()) for _ in range(3)]
        assert torch.equal(outs[0], outs[1]) and torch.equal(outs[1], outs[2])


# ------------------------------------------------------------------------------------------ 4. values gradient
@pytest.mark.parametrize("dtype", CDTYPES)
def test_csr_sddmm_complex_vs_complex128(dev, dtype):
    g = torch.Generator().manual_seed(4)
    M, N = 777, 1201
    crow, col = _pattern("empty", M, N, seed=2)
    A = SparseLinearOperator(crow.to(dev), col.to(dev), torch.ones(col.numel(), dtype=dtype, device=dev), (M, N))
    rows = torch.repeat_interleave(torch.arange(M), crow[1:] - crow[:-1])
    B, C = 4, 3
    _, U = _panel(B, C, M, M + 5, dtype, dev, g)
    _, W = _panel(B, C, N, N + 1, dtype, dev, g)
    tol = 1e-12 if dtype == c128 else 1e-4
    ref = (U.cpu().to(c128)[:, :, rows] * W.cpu().to(c128)[:, :, col].conj()).sum(1)      # (B, nnz)
    G = K.csr_sddmm(A._pattern, U, W)
    assert torch.allclose(G.cpu().to(c128), ref, atol=tol, rtol=tol)
    # values broadcast over the batch: the batch folded into the columns, summed inside the kernel
    Gs = K.csr_sddmm(A._pattern, U.contiguous().reshape(1, B * C, M), W.contiguous().reshape(1, B * C, N))
    assert Gs.shape == (1, col.numel()) and torch.allclose(Gs.cpu().to(c128)[0], ref.sum(0), atol=4 * tol, rtol=tol)
    # adjoint apply: the operands swap (U lives on the columns, W on the rows)
    _, Wt = _panel(B, C, M, M, dtype, dev, g)
    _, Ut = _panel(B, C, N, N, dtype, dev, g)
    reft = (Wt.cpu().to(c128)[:, :, rows] * Ut.cpu().to(c128)[:, :, col].conj()).sum(1)
    assert torch.allclose(K.csr_sddmm(A._pattern, Wt, Ut).cpu().to(c128), reft, atol=tol, rtol=tol)


# ------------------------------------------------------------------------------------------ 5. autograd
@pytest.mark.parametrize("vbatch,xbatch", [((), (4,)), ((3,), (3,)), ((3,), (2, 3)), ((2, 1), (2, 3))])
@pytest.mark.parametrize("trans", [False, True])
@pytest.mark.parametrize("loss", ["abs2", "weighted"])
def test_complex_native_autograd_matches_torch_expression(dev, vbatch, xbatch, trans, loss):
    """_CsrMM / _CsrGrad (first and second order) against autograd through csr_apply_torch on the device.  The
    weighted loss Re(sum w y) + 0.3 Im(sum w y) with a fixed complex w is not invariant under conjugating y, values
    or x, and the second-order functional mixes |g|^2 with Im(sum g g): a missing conjugation shows."""
    M, N = 517, 389
    crow, col = _pattern("empty", M, N, seed=31)
    g = torch.Generator().manual_seed(2)
    v0 = _crandn(g, *vbatch, col.numel()).to(dev)
    x0 = _crandn(g, *xbatch, M if trans else N, 3).to(dev)
    w = _crandn(g, *torch.broadcast_shapes(vbatch, xbatch), N if trans else M, 3).to(dev)
    crow_d, col_d = crow.to(dev), col.to(dev)

    def lossfn(y):
        if loss == "abs2":
            return (y.abs() ** 2).sum()
        s = (y * w).sum()
        return s.real + 0.3 * s.imag
    outs = []
    for native in (True, False):
        v = v0.clone().requires_grad_()
        x = x0.clone().requires_grad_()
        if native:
            A = SparseLinearOperator(crow_d, col_d, v, (*vbatch, M, N))
            y = A.rmm(x) if trans else A.mm(x)
        else:
            y = linop.csr_apply_torch(crow_d, col_d, v, x, M, N, trans)
        gv, gx = torch.autograd.grad(lossfn(y), (v, x), create_graph=True)
        second = (gv.abs() ** 2).sum() + (gx.abs() ** 2).sum() + (gv * gv).sum().imag + (gx * gx).sum().imag
        ggv, ggx = torch.autograd.grad(second, (v, x))
        outs.append((y, gv, gx, ggv, ggx))
    for a, b in zip(*outs):
        assert a.shape == b.shape and torch.allclose(a, b, rtol=1e-11, atol=1e-11), float((a - b).abs().max())


# ------------------------------------------------------------------------------------------ 6. / 7. solvers
def _herm_sparse(N, seed, batch=(), dtype=c128, shift=0.0, off=1.0):
    """Hermitian sparse (random pattern + its mirror + real diagonal) as (crow, col, vals) host tensors: the
    _sym_sparse recipe of tests/test_gpu_sparse.py with complex off-diagonal entries w (real and imaginary part
    uniform in +-0.5, times `off`), mirrored as conj(w), the i == j draws removed so the diagonal stays real"""
    g = torch.Generator().manual_seed(seed)
    i = torch.randint(0, N, (4 * N,), generator=g)
    j = torch.randint(0, N, (4 * N,), generator=g)
    w = torch.complex(torch.rand((*batch, 4 * N), generator=g, dtype=torch.float64) - 0.5,
                      torch.rand((*batch, 4 * N), generator=g, dtype=torch.float64) - 0.5) * off
    d = shift + torch.linspace(1.0, 3.0, N, dtype=torch.float64).expand(*batch, N) + \
        0.1 * torch.rand((*batch, N), generator=g, dtype=torch.float64)
    keep = i != j
    i, j, w = i[keep], j[keep], w[..., keep]
    ii = torch.cat([i, j, torch.arange(N)])
    jj = torch.cat([j, i, torch.arange(N)])
    v = torch.cat([w, w.conj(), d.to(c128)], dim=-1)
    order = torch.sort(ii, stable=True).indices
    crow = torch.zeros(N + 1, dtype=torch.int64)
    crow[1:] = torch.cumsum(torch.bincount(ii, minlength=N), 0)
    return crow, jj[order], v[..., order].resolve_conj().to(dtype)


def test_generator_is_exactly_hermitian(dev):
    crow, col, v = _herm_sparse(400, seed=3, batch=(2,))
    D = SparseLinearOperator(crow, col, v, (2, 400, 400), is_hermitian=True).fullmatrix()
    assert float((D - D.transpose(-2, -1).conj()).abs().max()) == 0.0


def test_panel_operator_kind_is_csr_for_complex_values(dev):
    for dtype in CDTYPES:
        crow, col, v = _herm_sparse(300, seed=1, batch=(2,), dtype=dtype)
        A = SparseLinearOperator(crow.to(dev), col.to(dev), v.to(dev), (2, 300, 300), is_hermitian=True)
        op = PanelOperator(A, [2], 2, 300)
        assert op.kind == "csr" and op.cplx
        # diagonal() keeps working: the stored diagonal, real
        dref = A.fullmatrix().diagonal(dim1=-2, dim2=-1)
        assert torch.equal(torch.view_as_real(op.diagonal()), torch.view_as_real(dref.contiguous()))
        # the panel apply is the operator's product
        g = torch.Generator().manual_seed(0)
        X = _crandn(g, 2, 5, 300, dtype=dtype).to(dev)
        out = torch.empty_like(X)
        op.apply(X, out)
        ref = A.fullmatrix().to(c128) @ X.to(c128).transpose(1, 2)
        assert torch.allclose(out.to(c128).transpose(1, 2), ref, rtol=1e-12 if dtype == c128 else 1e-4,
                              atol=1e-12 if dtype == c128 else 1e-4)


def test_lazily_conjugated_values_give_the_conjugated_matrix(dev):
    g = torch.Generator().manual_seed(6)
    M, N = 311, 207
    crow, col = _pattern("random", M, N, seed=5)
    v = _crandn(g, col.numel()).to(dev)
    vc = v.conj()
    assert vc.is_conj()
    A = SparseLinearOperator(crow.to(dev), col.to(dev), vc, (M, N))
    Aref = SparseLinearOperator(crow.to(dev), col.to(dev), v, (M, N)).fullmatrix().conj().resolve_conj()
    x = _crandn(g, N, 3).to(dev)
    y = _crandn(g, M, 3).to(dev)
    assert torch.allclose(A.mm(x), Aref @ x, rtol=1e-12, atol=1e-12)
    assert torch.allclose(A.rmm(y), Aref.transpose(0, 1).conj() @ y, rtol=1e-12, atol=1e-12)
    assert torch.allclose(A.mm(x.conj()), Aref @ x.conj().resolve_conj(), rtol=1e-12, atol=1e-12)
    op = PanelOperator(A, [], 1, N)
    assert op.kind == "csr"
    with pytest.raises(K._capi.NativeLibraryError):
        K.csr_mm(A._pattern, vc.reshape(1, -1), x.transpose(0, 1).contiguous().unsqueeze(0))


def _count_calls(monkeypatch):
    torch_calls, native_calls = [0], [0]
    real_torch, real_native = linop.csr_apply_torch, K.csr_mm

    def counted_torch(*a, **k):
        torch_calls[0] += 1
        return real_torch(*a, **k)

    def counted_native(*a, **k):
        native_calls[0] += 1
        return real_native(*a, **k)
    monkeypatch.setattr(linop, "csr_apply_torch", counted_torch)
    monkeypatch.setattr(K, "csr_mm", counted_native)
    return torch_calls, native_calls


def test_no_solver_call_reaches_the_torch_expression(dev, monkeypatch):
    """device symeig (davidson), solve with cg and bicgstab, and svd, forward and backward: csr_apply_torch is never
    called, K.csr_mm is, and the host drivers' counters do not move"""
    from xitorch_amd.linalg import host_eig, host_krylov
    N = 300
    crow, col, v = _herm_sparse(N, seed=2, batch=(2,), shift=2.0)
    torch_calls, native_calls = _count_calls(monkeypatch)
    before = (dict(host_krylov.calls), dict(host_eig.calls))
    vals = v.to(dev).requires_grad_()
    A = SparseLinearOperator(crow.to(dev), col.to(dev), vals, (2, N, N), is_hermitian=True)
    tr = {}
    davidson(A, 3, "lowest", min_eps=1e-8, trace=tr)
    assert tr["panel_kernel"] == "csr"
    ev, X = symeig(A, 3, "lowest", method="davidson", min_eps=1e-9)
    torch.autograd.grad(ev.sum(), (vals,))
    n0 = native_calls[0]
    assert n0 > 0
    g = torch.Generator().manual_seed(1)
    for meth in ("cg", "bicgstab"):
        b = _crandn(g, 2, N, 2).to(dev).requires_grad_()
        x = solve(A, b, method=meth, rtol=1e-9)
        torch.autograd.grad((x.abs() ** 2).sum(), (vals, b))
    assert native_calls[0] > n0
    n0 = native_calls[0]
    Mr, Nr = 260, 110
    cr, cc = _pattern("random", Mr, Nr, seed=21)
    rv = _crandn(g, cc.numel()).to(dev).requires_grad_()
    R = SparseLinearOperator(cr.to(dev), cc.to(dev), rv, (Mr, Nr))
    u, s, vh = svd(R, 3, "uppest", method="davidson", min_eps=1e-9)
    torch.autograd.grad(s.sum(), (rv,))
    assert native_calls[0] > n0
    assert torch_calls[0] == 0
    assert (dict(host_krylov.calls), dict(host_eig.calls)) == before


@pytest.mark.parametrize("dtype,tol", [(c128, 1e-10), (c64, 1e-4)])
@pytest.mark.parametrize("mode", ["lowest", "uppest"])
def test_davidson_on_complex_csr_matches_eigvalsh(dev, dtype, tol, mode):
    N = 400
    crow, col, v = _herm_sparse(N, seed=3, batch=(2,), dtype=dtype)
    A = SparseLinearOperator(crow.to(dev), col.to(dev), v.to(dev), (2, N, N), is_hermitian=True)
    Ad = A.fullmatrix().cpu().to(c128)
    tr = {}
    ev, X = davidson(A, 4, mode, min_eps=1e-9 if dtype == c128 else 1e-4, trace=tr)
    assert tr["panel_kernel"] == "csr"
    ref = torch.linalg.eigvalsh(Ad)
    ref = ref[..., :4] if mode == "lowest" else ref[..., -4:]
    scale = float(ref.abs().max())
    err = float((ev.cpu().double().sort(-1).values - ref.sort(-1).values).abs().max())
    print("davidson %s %s: err %.3e (bound %.3e)" % (dtype, mode, err, tol * scale))
    assert err <= tol * scale


@pytest.mark.parametrize("mode", ["lowest", "uppest"])
def test_davidson_on_complex_csr_with_hermitian_csr_M(dev, mode):
    N = 400
    crow, col, v = _herm_sparse(N, seed=3, batch=(2,))
    A = SparseLinearOperator(crow.to(dev), col.to(dev), v.to(dev), (2, N, N), is_hermitian=True)
    cm, colm, vm = _herm_sparse(N, seed=8, shift=3.0, off=0.05)
    Mop = SparseLinearOperator(cm.to(dev), colm.to(dev), vm.to(dev), (N, N), is_hermitian=True)
    assert PanelOperator(Mop, [2], 2, N).kind == "csr"
    Ad, Md = A.fullmatrix().cpu(), Mop.fullmatrix().cpu()
    tr = {}
    ev, X = davidson(A, 4, mode, Mop, min_eps=1e-9, trace=tr)
    assert tr["panel_kernel"] == "csr"
    Li = torch.linalg.inv(torch.linalg.cholesky(Md))
    ref = torch.linalg.eigvalsh(Li @ Ad @ Li.transpose(-2, -1).conj())
    ref = ref[..., :4] if mode == "lowest" else ref[..., -4:]
    scale = float(ref.abs().max())
    assert (ev.cpu().double().sort(-1).values - ref.sort(-1).values).abs().max() <= 1e-10 * scale


@pytest.mark.parametrize("method", ["cg", "bicgstab"])
def test_krylov_on_complex_csr_batch(dev, method, monkeypatch):
    N = 600
    crow, col, v = _herm_sparse(N, seed=6, batch=(3,), shift=4.0)
    A = SparseLinearOperator(crow.to(dev), col.to(dev), v.to(dev), (3, N, N), is_hermitian=True)
    assert PanelOperator(A, [3], 3, N).kind == "csr"
    torch_calls, native_calls = _count_calls(monkeypatch)
    g = torch.Generator().manual_seed(0)
    Bm = _crandn(g, 3, N, 2)
    x = solve(A, Bm.to(dev), method=method, rtol=1e-11, atol=1e-14)
    ref = torch.linalg.solve(A.fullmatrix().cpu(), Bm)
    assert native_calls[0] > 0 and torch_calls[0] == 0
    err = float((x.cpu() - ref).abs().max())
    print("%s: err %.3e (bound %.3e)" % (method, err, 1e-8 * float(ref.abs().max())))
    assert err <= 1e-8 * float(ref.abs().max())


def test_complex_solve_backward_matches_dense(dev):
    N = 200
    crow, col, v = _herm_sparse(N, seed=12, shift=4.0)
    rows = torch.repeat_interleave(torch.arange(N), crow[1:] - crow[:-1])
    g = torch.Generator().manual_seed(3)
    vals = v.to(dev).requires_grad_()
    Bm = _crandn(g, N, 2).to(dev).requires_grad_()
    A = SparseLinearOperator(crow.to(dev), col.to(dev), vals, (N, N), is_hermitian=True)
    bck = dict(method="cg", rtol=1e-13, atol=1e-15)
    x = solve(A, Bm, method="cg", rtol=1e-12, atol=1e-14, bck_options=bck)
    wgt = _crandn(g, N, 2).to(dev)
    lossfn = lambda x: (x.abs() ** 2).sum() + (x * wgt).sum().imag
    gv, gb = torch.autograd.grad(lossfn(x), (vals, Bm))
    D = A.fullmatrix().detach().clone().requires_grad_()
    B2 = Bm.detach().clone().requires_grad_()
    x2 = solve(xa.LinearOperator.m(D, True), B2, method="cg", rtol=1e-12, atol=1e-14, bck_options=bck)
    gD, gb2 = torch.autograd.grad(lossfn(x2), (D, B2))
    # d/dvals[k] = dL/dA[row_k, col_k]: the dense gradient sampled at the pattern (duplicates share it)
    gref = gD[rows.to(dev), col.to(dev)]
    assert torch.allclose(gv, gref, atol=1e-8, rtol=1e-6), float((gv - gref).abs().max())
    assert torch.allclose(gb, gb2, atol=1e-9, rtol=1e-7), float((gb - gb2).abs().max())


def test_complex_symeig_backward_wrt_values(dev):
    N = 160
    crow, col, v = _herm_sparse(N, seed=13)
    rows = torch.repeat_interleave(torch.arange(N), crow[1:] - crow[:-1])
    vals = v.to(dev).requires_grad_()
    A = SparseLinearOperator(crow.to(dev), col.to(dev), vals, (N, N), is_hermitian=True)
    ev, X = symeig(A, 3, "lowest", method="davidson", min_eps=1e-11)
    gv, = torch.autograd.grad(ev.sum(), (vals,))
    # d lambda / dA = x x^H (torch's convention), sampled at the pattern
    ev_ref, V = torch.linalg.eigh(A.fullmatrix().detach().cpu())
    G = V[:, :3] @ V[:, :3].transpose(0, 1).conj()
    gref = G[rows, col]
    assert torch.allclose(gv.cpu(), gref, atol=1e-7), float((gv.cpu() - gref).abs().max())


def test_svd_of_rectangular_complex_csr(dev):
    M, N = 300, 120
    crow, col = _pattern("random", M, N, seed=21)
    g = torch.Generator().manual_seed(0)
    vals = _crandn(g, col.numel())
    A = SparseLinearOperator(crow.to(dev), col.to(dev), vals.to(dev), (M, N))
    u, s, vh = svd(A, 4, "uppest", method="davidson", min_eps=1e-10)
    ref = torch.linalg.svdvals(A.fullmatrix().cpu())[:4]
    assert torch.allclose(s.cpu().sort(descending=True).values, ref, rtol=1e-9)
