"""-m gpu: the two dtype backends of the block layer (linalg/_block.py) on the device, against float64 / complex128
computations on the CPU: block orthonormalisation, the routing of the small dense eigensolve, the guard and its one
host read.  Bt = 2, N in {257, 1037} (odd, no multiple of the panel padding), four dtypes, with and without a dense
Hermitian positive definite M."""
import functools
import pytest
import torch
import xitorch_amd as xa
from xitorch_amd import kernels as K
from xitorch_amd.linalg._panel import PanelOperator, real_dtype
from xitorch_amd.linalg import _block
from xitorch_amd.linalg._block import block_ops, GUARD_GOOD, EXACTEIG_NATIVE_MAX_P

pytestmark = pytest.mark.gpu
F64, F32, C128, C64 = torch.float64, torch.float32, torch.complex128, torch.complex64
DTYPES = [F64, F32, C128, C64]
IDS = ["f64", "f32", "c128", "c64"]
BT = 2
C_TOL = 8.0          # the constant of every rounding bound of the kernel tests (tests/davidson_ref.py, tests/herm_ref.py)


def _rand(g, cplx, *shape):
    re = torch.randn(shape, dtype=F64, generator=g)
    return torch.complex(re, torch.randn(shape, dtype=F64, generator=g)) if cplx else re


def _H(x):
    return x.transpose(-2, -1).conj()


def _wide(t):
    t = t.detach().cpu()
    return t.to(C128) if t.is_complex() else t.to(F64)


@functools.lru_cache(maxsize=None)
def _pool(cplx, N):
    """(M (BT, N, N) dense Hermitian positive definite: I + 2 U U^H, spectrum in [1, ~4]; 80 seeded normal rows)"""
    g = torch.Generator().manual_seed(1000 * N + cplx)
    U = _rand(g, cplx, BT, N, 8) / N ** 0.5
    M = torch.eye(N, dtype=U.dtype) + 2.0 * U @ _H(U)
    return (M + _H(M)) * 0.5, _rand(g, cplx, BT, 80, N)


def _m_rows(M, S):
    """rows M s_c of the rows s_c of S (BT, r, N)"""
    return (M @ S.transpose(1, 2)).transpose(1, 2)


def _gram(S, MS):
    """G[b, i, c] = <s_i, M s_c>"""
    return S.conj() @ MS.transpose(1, 2)


def _stacks(ops, dev, rows_new, k0, M):
    """S with k0 M-orthonormal rows (made in double, rounded to the dtype) followed by `rows_new`; M S with the images
    of the first k0 rows and zeros (orth applies M to the new ones itself); the panel operator of M"""
    dtype, N, q = ops.dtype, ops.N, rows_new.shape[1]
    S = ops.panel(k0 + q)
    MS = opM = None
    if k0 > 0:
        Z = _pool(dtype.is_complex, N)[1][:, 40:40 + k0]
        MZ = _m_rows(M, Z) if M is not None else Z
        L = torch.linalg.cholesky(_gram(Z, MZ))                  # G = L L^H: the rows conj(L)^-1 Z are M-orthonormal
        S[:, :k0, :N] = torch.linalg.solve_triangular(L.conj(), Z, upper=False).to(dtype).to(dev)
    S[:, k0:, :N] = rows_new.to(dtype).to(dev)
    if M is not None:
        MS = ops.panel(k0 + q)
        MS[:, :k0, :N] = _m_rows(M, _wide(S[:, :k0, :N])).to(dtype).to(dev)
        opM = PanelOperator(xa.LinearOperator.m(M.to(dtype).to(dev), is_hermitian=True), [BT], BT, N)
    return S, MS, opM


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("N", [257, 1037])
@pytest.mark.parametrize("with_m", [False, True], ids=["plain", "M"])
def test_orth(dev, dtype, N, with_m):
    cplx, rdt = dtype.is_complex, real_dtype(dtype)
    Mfull, rows = _pool(cplx, N)
    M = Mfull if with_m else None
    Mk = M.to(dtype).to(C128 if cplx else F64) if with_m else None                     # the M the kernels read
    u = torch.finfo(rdt).eps / 2
    shapes = [(0, 5), (6, 6)] + ([(33, 33)] if cplx else [])                           # (33, 33): two chunks
    for (k0, q) in shapes:
        for passes in (2, 3):
            what = "%s N=%d M=%s k0=%d q=%d passes=%d" % (dtype, N, with_m, k0, q, passes)
            ops = block_ops(BT, N, q, dtype, dev, kmax=k0)
            S, MS, opM = _stacks(ops, dev, rows[:, :q], k0, M)
            S0, MS0 = S.clone(), (MS.clone() if with_m else None)
            ops.orth(S, k0, q, passes, ops.info, MS=MS, opM=opM, chunk=K.HERM_CHOLQR_MAX_Q if q > 32 else None)
            assert ops.info.cpu().tolist() == [0] * BT, what
            assert torch.equal(S[:, :k0], S0[:, :k0]) and torch.equal(S[:, :, N:], S0[:, :, N:]), what
            Sd = _wide(S[:, :, :N])
            MSd = _m_rows(Mk, Sd) if with_m else Sd
            E = (_gram(Sd, MSd) - torch.eye(k0 + q, dtype=Sd.dtype)).abs()
            worst = max(E[:, k0:, :].max().item(), E[:, :, k0:].max().item())
            print("%s: max|Q^H M Q - I| over the new rows %.3e (GUARD_GOOD %.1e)" % (what, worst, GUARD_GOOD[rdt]))
            assert worst <= GUARD_GOOD[rdt], what
            if with_m:
                assert torch.equal(MS[:, :k0], MS0[:, :k0]) and torch.equal(MS[:, :, N:], MS0[:, :, N:]), what
                # M is applied once and M S then follows S through `passes` projections (k0 terms) and triangular
                # transformations (q terms), both also applied to S: the linear maps cancel in M S - M (S), what is
                # left are their roundings, the 2N of the one product with M, and the rounding of the comparison's
                # own M S; the first transformation scales by R^-1 and can amplify what is there by kappa(R) <=
                # kappa_2(G), G the M-Gram matrix of the drawn rows.  In the form of the kernel tests' bounds:
                # C_TOL u (roundings) kappa_2(G) max(|M| |S|).
                W0 = rows[:, :q]
                k2 = torch.linalg.cond(_gram(W0, _m_rows(M, W0))).max().item()
                mag = (Mk.abs() @ Sd[:, k0:].abs().transpose(1, 2)).max().item()
                bound = C_TOL * u * (2 * N + 2 * passes * (k0 + q + 1)) * k2 * mag
                err = (_wide(MS[:, k0:, :N]) - MSd[:, k0:]).abs().max().item()
                print("%s: max|MS - M S| %.3e (bound %.3e, kappa_2 %.2f)" % (what, err, bound, k2))
                assert err <= bound, what


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("with_m", [False, True], ids=["plain", "M"])
def test_orth_flags_a_duplicated_row(dev, dtype, with_m):
    """one unshifted pass on a block whose rows 0 and 1 are the same vector: the second pivot is G11 - G01^2 / G00 = 0.
    The vector has 128 entries +1 and 128 entries -1 and M = 4 I + 1 1^T, so that every number up to that pivot is a
    small integer in every dtype (G00 = 256, or 1024 with M: M w = 4 w) with an exact square root: the pivot is
    exactly 0, not a rounding of it, and info names row 1 (index + 1 = 2) for both members."""
    N, q = 257, 5
    cplx = dtype.is_complex
    w = torch.zeros(N, dtype=F64)
    w[:128], w[128:256] = 1.0, -1.0
    rows = _pool(cplx, N)[1][:, :q].clone()
    rows[:, 0] = w
    rows[:, 1] = w
    M = (4.0 * torch.eye(N, dtype=rows.dtype) + 1.0).expand(BT, N, N).contiguous() if with_m else None
    ops = block_ops(BT, N, q, dtype, dev)
    S, MS, opM = _stacks(ops, dev, rows, 0, M)
    ops.orth(S, 0, q, 1, ops.info, MS=MS, opM=opM)
    assert ops.info.cpu().tolist() == [2] * BT


# ------------------------------------------------------------------------------------------------ eigh_lowest
def _hermitian(cplx, n, seed):
    g = torch.Generator().manual_seed(seed)
    T = _rand(g, cplx, BT, n, n)
    return (T + _H(T)) * 0.5


def _count_eigh(monkeypatch):
    calls, real_eigh = [], torch.linalg.eigh
    monkeypatch.setattr(torch.linalg, "eigh", lambda *a, **k: (calls.append(1), real_eigh(*a, **k))[1])
    return calls


def _check_pairs(T, mu, Y, n, p, dtype):
    """Tolerances of the tests these kernels already have.  Real: test_native_partial_eigh_sizes_and_dtypes of
    test_gpu_exacteig.py (eigenvalues 1e-11 n / 2e-4, residual ten times that) and, for X^T X = I,
    test_native_exacteig_vs_reference_golden (1e-10; float32: the 5e-5 of the complex64 kernel below).  Complex:
    test_rr_kernel_edge_matrices of test_gpu_davidson_hermitian.py (eigenvalues 1e-12 / 1e-5 |T|, residual 1e-12 / 2e-5
    n |T|, orthonormality 1e-12 / 5e-5)."""
    assert mu.shape == (BT, p) and Y.shape == (BT, n, p)
    ref = torch.linalg.eigvalsh(T)[:, :p]
    mu, Y = mu.cpu().to(F64), _wide(Y)
    single = real_dtype(dtype) == F32
    if dtype.is_complex:
        tnorm = torch.linalg.matrix_norm(T, ord=2).max().item()
        tol_lam, tol_res, tol_orth = [(1e-12 * tnorm, 1e-12 * n * tnorm, 1e-12), (1e-5 * tnorm, 2e-5 * n * tnorm, 5e-5)][single]
    else:
        tol_lam, tol_res, tol_orth = [(1e-11 * n, 1e-10 * n, 1e-10), (2e-4, 2e-3, 5e-5)][single]
    lam_err = (mu - ref).abs().max().item()
    res = (T.to(Y.dtype) @ Y - Y * mu.unsqueeze(-2)).abs().max().item()
    orth = (_H(Y) @ Y - torch.eye(p, dtype=Y.dtype)).abs().max().item()
    print("eigh_lowest %s n=%d p=%d: lam %.3e (%.1e) res %.3e (%.1e) orth %.3e (%.1e)"
          % (dtype, n, p, lam_err, tol_lam, res, tol_res, orth, tol_orth))
    assert lam_err <= tol_lam and res <= tol_res and orth <= tol_orth


@pytest.mark.parametrize("dtype", [F64, F32], ids=IDS[:2])
@pytest.mark.parametrize("n,p,wide,served", [(7, 7, False, "native"), (7, 7, True, "native"), (8, 8, False, "native"),
                                             (8, 8, True, "native"), (48, 16, False, "native"),
                                             (EXACTEIG_NATIVE_MAX_P + 1, EXACTEIG_NATIVE_MAX_P + 1, True, "library")])
def test_eigh_lowest_real_routes(dev, dtype, n, p, wide, served, monkeypatch):
    T = _hermitian(False, n, 100 * n + p)
    Td = T.to(dtype).to(dev)
    ops = block_ops(BT, 64, p, dtype, dev, wide=wide)
    assert ops.eigh_native(n, p) == (served == "native")
    routes = []
    for name in ("small_eigh", "small_eigh_big"):                        # (the Jacobi kernel / K3t, and K3g)
        monkeypatch.setattr(K, name, lambda *a, _f=getattr(K, name), _n=name, **k: (
            routes.append((_n, k.get("method"))), _f(*a, **k))[1])
    calls = _count_eigh(monkeypatch)
    mu, Y = ops.eigh_lowest(Td, n, p)
    monkeypatch.undo()
    assert ops.small_eigh == served and len(calls) == (served == "library")
    # order < 8: the Jacobi kernel; from 8 on native_partial_eigh (K3t inside its range, K3g beyond)
    want = [] if served == "library" else [("small_eigh", None)] if n < 8 else \
        [("small_eigh", "tri")] if K.small_eigh_tri_ok(n, p, dtype) and n >= K.SMALL_EIGH_TRI_MIN_K else \
        [("small_eigh_big", None)]
    assert routes == want
    _check_pairs(T.to(dtype).to(F64), mu, Y[:, :, :p], n, p, dtype)


@pytest.mark.parametrize("dtype", [C128, C64], ids=IDS[2:])
@pytest.mark.parametrize("n,p,wide,native,library", [
    (32, 16, False, 1, 0), (32, 17, False, 0, 1),                        # 16 pairs per call; beyond: the library
    (32, 32, True, 2, 0), (32, 32, False, 0, 1),                         # all pairs of 17 .. 32: the two-call seam
    (K.HERM_EIGH_MAX_K + 1, 6, False, 0, 1), (K.HERM_EIGH_MAX_K + 1, 6, True, 0, 1),
    (40, 40, True, 0, 1)])                                               # wider than two calls serve
def test_eigh_lowest_complex_routes(dev, dtype, n, p, wide, native, library, monkeypatch):
    T = _hermitian(True, n, 100 * n + p)
    Td = T.to(dtype).to(dev)
    ops = block_ops(BT, 64, p, dtype, dev, wide=wide)
    calls = _count_eigh(monkeypatch)
    mu, Y = ops.eigh_lowest(Td, n, p)
    monkeypatch.undo()
    assert ops.counts == {"rr_native": native, "rr_library": library}
    assert ops.small_eigh == ("library" if library else "native") and len(calls) == library
    _check_pairs(T.to(dtype).to(C128), mu, Y[:, :, :p], n, p, dtype)


# ------------------------------------------------------------------------------------------------ status
@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("N", [257, 1037])
@pytest.mark.parametrize("with_m", [False, True], ids=["plain", "M"])
def test_status(dev, dtype, N, with_m, monkeypatch):
    """(max|resid|, Cholesky flag, guard) against the same three numbers in double on the CPU; the guard to the bound
    of test_ritz_guard_kernel_vs_torch (test_gpu_guard.py): 1e-12 / 3e-5 times max(1, guard), ten times that with M"""
    cplx, rdt = dtype.is_complex, real_dtype(dtype)
    w = 6
    Mfull, rows = _pool(cplx, N)
    ops = block_ops(BT, N, w, dtype, dev)
    g = torch.Generator().manual_seed(N)
    Q = torch.linalg.qr(rows[:, :w].transpose(1, 2))[0] + 1e-3 * _rand(g, cplx, BT, N, w)   # visibly not orthonormal
    X = ops.panel(w + 2)
    X[:, :w, :N] = Q.transpose(1, 2).to(dtype).to(dev)
    X[:, w:, :N] = 7.0                                                   # rows beyond w are not read
    Xd = _wide(X[:, :w, :N])
    MX = MXd = None
    if with_m:
        MXd = _m_rows(Mfull, Xd)
        MX = ops.panel(w + 2)
        MX[:, :w, :N] = MXd.to(dtype).to(dev)
        MXd = _wide(MX[:, :w, :N])
    want_guard = (_gram(Xd, MXd if with_m else Xd) - torch.eye(w, dtype=Xd.dtype)).abs().max().item()
    resid = torch.tensor([0.25, 0.5], dtype=F64, device=dev)            # (exact in every dtype)
    info = torch.tensor([0, 3], dtype=torch.int32, device=dev)
    reads = []
    for name in ("tolist", "item"):
        monkeypatch.setattr(torch.Tensor, name, lambda self, *a, _f=getattr(torch.Tensor, name), _n=name, **k: (
            reads.append(_n), _f(self, *a, **k))[1])
    got = ops.status(X, w, resid, info, MX=MX)
    monkeypatch.undo()
    assert reads == ["tolist"]                                           # the ONE host read
    tol = (1e-12 if rdt == F64 else 3e-5) * (10 if with_m else 1) * max(1.0, want_guard)
    print("status %s N=%d M=%s: guard %.6e, CPU %.6e (tol %.1e)" % (dtype, N, with_m, got[2], want_guard, tol))
    assert got[0] == 0.5 and got[1] == 3.0 and abs(got[2] - want_guard) <= tol
    # a NaN residual entry does not come back as a smaller number
    resid[0] = float("nan")
    first = ops.status(X, w, resid, info, MX=MX)[0]
    assert first != first or first == float("inf")
    if not cplx:
        # (resid=None: the residual kernel has written ops.rmax itself, as in chebfsi)
        ops.rmax.copy_(torch.tensor([2.0, 1.0], dtype=F64))
        assert ops.status(X, w, None, info, MX=MX)[0] == 2.0
    else:
        assert ops.status(X, w, torch.tensor(4.0, dtype=F64, device=dev), info, MX=MX)[0] == 4.0      # a 0-dim maximum
    assert _block.GUARD_GOOD[rdt] < want_guard                           # (the block is visibly not orthonormal)
