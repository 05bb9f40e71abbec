"""-m gpu: block Davidson on complex Hermitian operators (native_eig_herm.py, xk_herm_davidson.hip).

The reference's davidson is real-only (T = V^T A V with an unconjugated transpose, symeig.py:165-174), so the yardstick
here is torch.linalg.eigh in complex128 on the CPU, and the host driver (host_eig.py), not a golden."""
import pytest
import torch
import xitorch_amd as xa
from xitorch_amd import kernels as K
from xitorch_amd import _capi
from xitorch_amd._capi import NativeLibraryError
from xitorch_amd.linalg import symeig, svd, host_eig, native_eig_herm
from xitorch_amd.linalg.native_eig import davidson

pytestmark = pytest.mark.gpu
c128, c64 = torch.complex128, torch.complex64


def _crand(g, *shape):
    return torch.complex(torch.randn(shape, dtype=torch.float64, generator=g),
                         torch.randn(shape, dtype=torch.float64, generator=g))


def _herm(g, B, n):
    H = _crand(g, B, n, n)
    return (H + H.transpose(-2, -1).conj()) * 0.5


def _unitary(g, B, n):
    Q, _ = torch.linalg.qr(_crand(g, B, n, n))
    return Q


def _separated(g, B, n):
    """Hermitian matrices whose 8 lowest and 8 uppermost eigenvalues are well separated from each other and the bulk"""
    ends = torch.tensor([-10.0, -9.0, -8.2, -7.5, -6.7, -6.0, -5.4, -4.8])
    d = torch.cat((ends, torch.rand(n - 16, dtype=torch.float64, generator=g) * 2 - 1, -ends.flip(0)))
    Q = _unitary(g, B, n)
    return torch.matmul(Q * d.to(c128), Q.transpose(-2, -1).conj())


def _op(mat, dev, dtype=c128):
    return xa.LinearOperator.m(mat.to(dtype).to(dev), is_hermitian=True)


def _check_pairs(A, lam, X, tol_res, tol_orth, M=None):
    """A X = M X diag(lam) and X^H M X = I (all in complex128 on the CPU)"""
    A, X, lam = A.to(c128), X.cpu().to(c128), lam.cpu().to(torch.float64)
    MX = X if M is None else torch.matmul(M, X)
    res = (torch.matmul(A, X) - MX * lam.unsqueeze(-2)).abs().max().item()
    G = torch.matmul(X.transpose(-2, -1).conj(), MX)
    orth = (G - torch.eye(G.shape[-1], dtype=c128)).abs().max().item()
    assert res <= tol_res, res
    assert orth <= tol_orth, orth


# ---------------------------------------------------------------------------------------------- 1. Rayleigh-Ritz kernel
@pytest.mark.parametrize("dtype", [c128, c64])
@pytest.mark.parametrize("mode", ["lowest", "uppest"])
@pytest.mark.parametrize("n,p", [(n, p) for n in (2, 7, 33, 64, 100, K.HERM_EIGH_MAX_K) for p in (1, 6, 16) if p <= n])
def test_rr_kernel_vs_eigh(dev, dtype, mode, n, p):
    g = torch.Generator().manual_seed(1000 * n + p)
    T = _herm(g, 3, n)
    lam, Yt, flag = K.herm_eigh(T.to(dtype).to(dev), n, p, uppest=(mode == "uppest"))
    assert int(flag.max().item()) == 0
    ref = torch.linalg.eigvalsh(T)
    ref = ref[..., :p] if mode == "lowest" else ref[..., -p:]
    tnorm = torch.linalg.matrix_norm(T, ord=2).max().item()
    tol = 1e-12 if dtype == c128 else 1e-5
    assert (lam.cpu().double() - ref).abs().max().item() <= tol * tnorm
    Y = Yt.cpu().to(c128).transpose(-2, -1)
    _check_pairs(T, lam, Y, (1e-12 if dtype == c128 else 2e-5) * n * tnorm, 1e-12 if dtype == c128 else 5e-5)


def _edge(kind, n, g):
    if kind == "diagonal":
        return torch.diag_embed(torch.randn(2, n, dtype=torch.float64, generator=g)).to(c128)
    if kind == "zero":
        return torch.zeros(2, n, n, dtype=c128)
    if kind == "real":
        H = torch.randn(2, n, n, dtype=torch.float64, generator=g)
        return ((H + H.transpose(-2, -1)) * 0.5).to(c128)
    if kind == "imaginary":
        H = torch.randn(2, n, n, dtype=torch.float64, generator=g)
        S = (H - H.transpose(-2, -1)) * 0.5                     # i S is Hermitian with a zero diagonal
        return torch.complex(torch.diag_embed(torch.randn(2, n, dtype=torch.float64, generator=g)), S)
    if kind == "blocks":
        T = torch.zeros(2, n, n, dtype=c128)
        h = n // 2
        T[:, :h, :h] = _herm(g, 2, h)
        T[:, h:, h:] = _herm(g, 2, n - h) + 3
        return T
    if kind == "cluster":                                        # a 5-fold eigenvalue at the low end
        d = torch.cat((torch.full((5,), -3.0, dtype=torch.float64), torch.rand(n - 5, dtype=torch.float64, generator=g)))
        Q = _unitary(g, 2, n)
        return torch.matmul(Q * d.to(c128), Q.transpose(-2, -1).conj())
    raise ValueError(kind)


@pytest.mark.parametrize("dtype", [c128, c64])
@pytest.mark.parametrize("kind", ["diagonal", "zero", "real", "imaginary", "blocks", "cluster"])
@pytest.mark.parametrize("n", [33, 128])
def test_rr_kernel_edge_matrices(dev, dtype, kind, n):
    g = torch.Generator().manual_seed(n)
    T = _edge(kind, n, g)
    p = 6
    lam, Y = native_eig_herm.herm_partial_eigh(T.to(dtype).to(dev), n, p, "lowest")
    ref = torch.linalg.eigvalsh(T)[..., :p]
    tnorm = max(torch.linalg.matrix_norm(T, ord=2).max().item(), 1e-30)      # (the zero matrix: an absolute floor)
    tol = 1e-12 if dtype == c128 else 1e-5
    assert (lam.cpu().double() - ref).abs().max().item() <= tol * tnorm
    # (degenerate eigenvalues: only the subspace is defined, so the pairs are checked, not the vectors)
    _check_pairs(T, lam, Y, (1e-12 if dtype == c128 else 2e-5) * n * tnorm, 1e-12 if dtype == c128 else 5e-5)


@pytest.mark.parametrize("dtype,scale", [(c128, 1e-150), (c64, 1e-30)])
def test_rr_kernel_flags_out_of_range_scale(dev, dtype, scale):
    g = torch.Generator().manual_seed(5)
    T = _herm(g, 2, 40) * scale
    _, _, flag = K.herm_eigh(T.to(dtype).to(dev), 40, 4)
    assert flag.cpu().tolist() == [1, 1]


# ---------------------------------------------------------------------------------------------- 2. Ritz step, CholeskyQR
@pytest.mark.parametrize("dtype", [c128, c64])
@pytest.mark.parametrize("with_m", [False, True])
@pytest.mark.parametrize("k,p", [(5, 1), (40, 6), (70, 20)])
def test_ritz_kernel_vs_torch(dev, dtype, with_m, k, p):
    g = torch.Generator().manual_seed(k + p)
    B, N = 3, 1037
    V, AV, MV = (_crand(g, B, k + 3, N) for _ in range(3))
    Y = _crand(g, B, k, p)
    lam = torch.randn(B, p, dtype=torch.float64, generator=g)
    to = lambda t: t.to(dtype).to(dev)
    rdt = torch.float64 if dtype == c128 else torch.float32
    X = torch.empty(B, p, N, dtype=dtype, device=dev)
    Tn = torch.empty(B, p, N, dtype=dtype, device=dev)
    status = torch.full((B + 1,), 7.0, dtype=torch.float64, device=dev)
    K.herm_ritz(to(V), to(AV), to(Y), lam.to(rdt).to(dev), X, Tn, status, k, p, MV=to(MV) if with_m else None)
    Yt = Y.transpose(-2, -1)
    Xr = torch.matmul(Yt, V[:, :k])
    R = torch.matmul(Yt, AV[:, :k]) - lam.unsqueeze(-1) * torch.matmul(Yt, (MV if with_m else V)[:, :k])
    tol = (1e-12 if dtype == c128 else 1e-4) * k
    assert (X.cpu().to(c128) - Xr).abs().max().item() <= tol
    assert (Tn.cpu().to(c128) + R).abs().max().item() <= tol * 10
    rm = R.abs().reshape(B, -1).max(dim=-1)[0]
    st = status.cpu()
    assert (st[1:] - rm).abs().max().item() <= tol * 10
    assert st[0].item() == st[1:].max().item()


@pytest.mark.parametrize("dtype", [c128, c64])
@pytest.mark.parametrize("q", [1, 6, 32])
@pytest.mark.parametrize("with_m,shift", [(False, 0.0), (True, 0.0), (False, 1e-10)])
def test_cholqr_kernel(dev, dtype, q, with_m, shift):
    g = torch.Generator().manual_seed(q)
    B, N = 2, 777
    W = _crand(g, B, q, N)
    Mm = None
    if with_m:
        L = _crand(g, B, N, N) * (0.3 / N ** 0.5)
        Mm = torch.matmul(L, L.transpose(-2, -1).conj()) + torch.eye(N, dtype=c128)
    MW = torch.matmul(W, Mm.transpose(-2, -1)) if with_m else None        # rows: (M w_c)^T = w_c^T M^T
    Wd = W.to(dtype).to(dev).contiguous()
    MWd = MW.to(dtype).to(dev).contiguous() if with_m else None
    info = torch.zeros(B, dtype=torch.int32, device=dev)
    K.herm_cholqr(Wd, info, MW=MWd, shift_rel=shift)
    assert info.cpu().tolist() == [0, 0]
    Q = Wd.cpu().to(c128)
    Qc = Q.transpose(-2, -1)                                                 # (B, N, q) columns
    MQc = Qc if not with_m else torch.matmul(Mm, Qc)
    G = torch.matmul(Qc.transpose(-2, -1).conj(), MQc)
    orth = (G - torch.eye(q, dtype=c128)).abs().max().item()
    # (the shifted pass only conditions the block: orthonormal to O(shift cond^2))
    assert orth <= ((1e-6 if shift else 1e-13) if dtype == c128 else 1e-4)
    if with_m:                                                               # MW transformed alike
        assert (MWd.cpu().to(c128) - MQc.transpose(-2, -1)).abs().max().item() <= (1e-12 if dtype == c128 else 1e-4)
    # same span: W = Q (Q^H M W)
    Wc = W.transpose(-2, -1)
    P = torch.matmul(Qc, torch.matmul(MQc.transpose(-2, -1).conj(), Wc))
    tol = (1e-6 if shift else 1e-11) if dtype == c128 else 1e-3
    assert (P - Wc).abs().max().item() <= tol * Wc.abs().max().item()


def test_cholqr_kernel_flags_rank_deficient_block(dev):
    g = torch.Generator().manual_seed(3)
    W = _crand(g, 2, 4, 300)
    W[1, 2] = 0                                                  # member 1: third vector zero -> pivot 3 is zero
    info = torch.zeros(2, dtype=torch.int32, device=dev)
    K.herm_cholqr(W.to(dev), info)
    assert info.cpu().tolist() == [0, 3]
    W2 = _crand(g, 2, 4, 300)
    W2[1, 0] = 0
    K.herm_cholqr(W2.to(dev), info)                              # sticky: the first flag stays
    assert info.cpu().tolist() == [0, 3]


# ---------------------------------------------------------------------------------------------- 3.-7. the solver
@pytest.mark.parametrize("N", [300, 1000])
@pytest.mark.parametrize("neig", [1, 4, 8])
@pytest.mark.parametrize("mode", ["lowest", "uppest"])
def test_solver_c128(dev, N, neig, mode):
    g = torch.Generator().manual_seed(N + neig)
    A = _separated(g, 3, N)
    min_eps = 1e-9
    tr = {}
    lam, X = davidson(_op(A, dev), neig, mode, min_eps=min_eps, trace=tr)
    assert tr["stop_reason"] == "converged" and tr["groups"] == 1
    ref_l, ref_X = torch.linalg.eigh(A)
    sl = slice(0, neig) if mode == "lowest" else slice(N - neig, N)
    anorm = torch.linalg.matrix_norm(A, ord=2).max().item()
    assert (lam.cpu() - ref_l[..., sl]).abs().max().item() <= 1e-9 * anorm
    _check_pairs(A, lam, X, 10 * min_eps, 1e-10)
    s = torch.linalg.svdvals(torch.matmul(ref_X[..., sl].transpose(-2, -1).conj(), X.cpu()))
    assert s.min().item() >= 1 - 1e-8


def test_solver_generalised(dev):
    g = torch.Generator().manual_seed(11)
    B, N, neig = 2, 400, 4
    A = _separated(g, B, N)
    L = _crand(g, B, N, N) * (0.5 / N ** 0.5)
    M = torch.matmul(L, L.transpose(-2, -1).conj()) + torch.eye(N, dtype=c128)
    lam, X = davidson(_op(A, dev), neig, "lowest", M=_op(M, dev), min_eps=1e-9)
    _check_pairs(A, lam, X, 1e-8, 1e-10, M=M)
    Li = torch.linalg.inv(torch.linalg.cholesky(M))
    ref = torch.linalg.eigvalsh(torch.matmul(Li, torch.matmul(A, Li.transpose(-2, -1).conj())))[..., :neig]
    assert (lam.cpu() - ref).abs().max().item() <= 1e-9 * 10


@pytest.mark.parametrize("mode", ["lowest", "uppest"])
def test_solver_c64(dev, mode):
    g = torch.Generator().manual_seed(64)
    A = _separated(g, 2, 500)
    lam, X = davidson(_op(A, dev, c64), 4, mode, min_eps=1e-4)
    assert lam.dtype == torch.float32 and X.dtype == c64
    ref = torch.linalg.eigvalsh(A)
    ref = ref[..., :4] if mode == "lowest" else ref[..., -4:]
    assert (lam.cpu().double() - ref).abs().max().item() <= 1e-4
    _check_pairs(A, lam, X, 1e-3, 1e-5)


def test_real_operator_cast_to_complex(dev):
    from xitorch_amd import synthetic
    mat = synthetic.dense_symmetric(2, 256, "S1")
    lr, Xr = davidson(xa.LinearOperator.m(mat.to(dev), is_hermitian=True), 4, "lowest", min_eps=1e-9)
    lc, Xc = davidson(_op(mat.to(c128), dev), 4, "lowest", min_eps=1e-9)
    assert (lc.cpu() - lr.cpu()).abs().max().item() <= 1e-10
    ov = torch.matmul(Xc.cpu().transpose(-2, -1).conj(), Xr.cpu().to(c128)).diagonal(dim1=-2, dim2=-1).abs()
    assert (ov - 1).abs().max().item() <= 1e-8


def test_device_matches_host(dev):
    g = torch.Generator().manual_seed(7)
    A = _separated(g, 2, 300)
    lh, _ = davidson(xa.LinearOperator.m(A, is_hermitian=True), 4, "lowest", min_eps=1e-10)
    before = host_eig.calls["davidson"]
    ld, _ = davidson(_op(A, dev), 4, "lowest", min_eps=1e-10)
    assert host_eig.calls["davidson"] == before
    assert (ld.cpu() - lh).abs().max().item() <= 1e-10


# ---------------------------------------------------------------------------------------------- 8.-9.
def test_no_library_eigh_inside_native_range(dev, monkeypatch):
    g = torch.Generator().manual_seed(8)
    A = _separated(g, 2, 600)
    Aop = _op(A, dev)

    def _refuse(*a, **k):
        raise AssertionError("library eigh called")
    with monkeypatch.context() as m:
        m.setattr(torch.linalg, "eigh", _refuse)
        tr = {}
        davidson(Aop, 4, "lowest", min_eps=1e-9, trace=tr)
    assert tr["basis_size"] <= K.HERM_EIGH_MAX_K and tr["rr_library"] == 0 and tr["rr_native"] == tr["niter"]
    # a basis that grows past the native range: the library serves the large Rayleigh-Ritz steps
    H = _herm(g, 1, 400)
    tr2 = {}
    davidson(_op(H, dev), 16, "lowest", min_eps=1e-13, max_niter=12, trace=tr2)
    assert tr2["basis_size"] > K.HERM_EIGH_MAX_K and tr2["rr_library"] > 0 and tr2["rr_native"] > 0


def test_bit_reproducible(dev):
    g = torch.Generator().manual_seed(9)
    Aop = _op(_separated(g, 2, 500), dev)
    l1, X1 = davidson(Aop, 6, "lowest", min_eps=1e-9)
    l2, X2 = davidson(Aop, 6, "lowest", min_eps=1e-9)
    assert torch.equal(l1, l2) and torch.equal(X1, X2)


# ---------------------------------------------------------------------------------------------- 10.-12. front end
@pytest.mark.parametrize("bck", [{}, {"method": "cg", "rtol": 1e-12, "atol": 1e-14}])
def test_backward_matches_exacteig(dev, bck):
    g = torch.Generator().manual_seed(10)
    A0 = _separated(g, 2, 120).to(dev)
    Bm = _herm(g, 2, 120).to(dev)

    def grad(method, **kw):
        # gradient with respect to the Hermitian A = (P + P^H) / 2: exacteig's eigh reads one triangle and davidson the
        # whole matrix, so only their Hermitian parts are comparable
        P = A0.clone().requires_grad_()
        A = (P + P.transpose(-2, -1).conj()) * 0.5
        lam, X = symeig(xa.LinearOperator.m(A, is_hermitian=True), 3, "lowest", method=method, bck_options=bck, **kw)
        loss = lam.sum() + torch.einsum("bnc,bnm,bmc->", X.conj(), Bm, X).real
        (gA,) = torch.autograd.grad(loss, P)
        return gA
    gd = grad("davidson", min_eps=1e-11)
    ge = grad("exacteig")
    assert (gd - ge).abs().max().item() <= 1e-9


def test_svd_davidson_complex(dev):
    g = torch.Generator().manual_seed(12)
    A = _crand(g, 2, 300, 200)
    u, s, vh = svd(xa.LinearOperator.m(A.to(dev)), k=4, method="davidson", min_eps=1e-10)
    ref = torch.linalg.svdvals(A)[..., :4].flip(-1)
    assert (s.cpu().sort(dim=-1)[0] - ref).abs().max().item() <= 1e-9


def test_full_size_closed_form(dev, monkeypatch):
    B, N = 2, 8192
    g = torch.Generator().manual_seed(13)
    d = torch.cat((torch.tensor([-5.0, -4.3, -3.7, -3.2, -2.8, -2.5]), torch.linspace(-1.0, 1.0, N - 6,
                                                                                       dtype=torch.float64)))
    A = torch.diag_embed(d.to(c128).to(dev)).unsqueeze(0).repeat(B, 1, 1)
    for _ in range(3):                                       # A <- H A H, H = I - 2 u u^H
        u = _crand(g, B, N, 1).to(dev)
        u = u / torch.linalg.vector_norm(u, dim=-2, keepdim=True)
        A = A - 2 * torch.matmul(u, torch.matmul(u.transpose(-2, -1).conj(), A))
        A = A - 2 * torch.matmul(torch.matmul(A, u), u.transpose(-2, -1).conj())
    A = (A + A.transpose(-2, -1).conj()) * 0.5

    def _refuse(*a, **k):
        raise AssertionError("library eigh called")
    tr = {}
    with monkeypatch.context() as m:
        m.setattr(torch.linalg, "eigh", _refuse)
        lam, X = davidson(xa.LinearOperator.m(A, is_hermitian=True), 6, "lowest", min_eps=1e-8, trace=tr)
    del A
    assert tr["rr_library"] == 0
    assert (lam.cpu() - d[:6]).abs().max().item() <= 1e-9


def test_missing_library_raises(dev, monkeypatch):
    g = torch.Generator().manual_seed(14)
    Aop = _op(_separated(g, 1, 100), dev)

    def _gone(name):
        raise NativeLibraryError("symbol %s missing" % name)
    monkeypatch.setattr(_capi, "fn", _gone)
    monkeypatch.setattr(K, "fn", _gone)
    with pytest.raises(NativeLibraryError):
        davidson(Aop, 2, "lowest")


@pytest.mark.parametrize("kw", [{"precond": "diag"}, {"restart": 12}])
def test_unsupported_options_raise(dev, kw):
    g = torch.Generator().manual_seed(15)
    with pytest.raises(NativeLibraryError, match="xk_herm_davidson"):
        davidson(_op(_separated(g, 1, 100), dev), 2, "lowest", **kw)
