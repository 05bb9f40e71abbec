"""SparseLinearOperator on host tensors: construction, the torch expression csr_apply_torch against the densified
matrix, gradients, the host solvers, and the C ABI declarations of the CSR kernels (no GPU needed)."""
import os
import re
import pytest
import torch
import xitorch_amd as xa
from xitorch_amd import _capi
from xitorch_amd.linop import SparseLinearOperator, csr_apply_torch, checklinop
from xitorch_amd.linalg import symeig, solve

DT = torch.float64


def _random_csr(M, N, nnz_per_row, seed, dup=True, unsorted=True, empty_every=0):
    g = torch.Generator().manual_seed(seed)
    crow, cols = [0], []
    for i in range(M):
        n = 0 if (empty_every and i % empty_every == 0) else int(torch.randint(0, nnz_per_row + 1, (1,), generator=g))
        c = torch.randint(0, N, (n,), generator=g)
        if not unsorted:
            c = c.sort().values
        if dup and n > 1:
            c[-1] = c[0]                     # a duplicate (row, col) pair
        cols.append(c)
        crow.append(crow[-1] + n)
    col = torch.cat(cols) if cols else torch.zeros(0, dtype=torch.int64)
    return torch.tensor(crow), col


def _dense(crow, col, vals, M, N):
    rows = torch.repeat_interleave(torch.arange(M), crow[1:] - crow[:-1])
    D = torch.zeros((*vals.shape[:-1], M, N), dtype=vals.dtype)
    for k in range(col.numel()):
        D[..., rows[k], col[k]] += vals[..., k]
    return D


def _spd_operator(N, seed, batch=()):
    """symmetric diagonally dominant sparse matrix (duplicates included) as a SparseLinearOperator + dense copy"""
    g = torch.Generator().manual_seed(seed)
    ii, jj = [], []
    for i in range(N):
        for j in (i - 3, i - 1, i + 1, i + 3):
            if 0 <= j < N:
                ii.append(i)
                jj.append(j)
        ii += [i, i]
        jj += [i, i]
    ii, jj = torch.tensor(ii), torch.tensor(jj)
    order = torch.sort(ii, stable=True).indices
    ii, jj = ii[order], jj[order]
    w = torch.rand((*batch, N, N), generator=g, dtype=DT)
    w = w + w.transpose(-2, -1)
    vals = torch.where(ii == jj, 2.0 + torch.arange(N, dtype=DT)[ii] / N, 0.2 * w[..., ii, jj] - 0.1)
    crow = torch.zeros(N + 1, dtype=torch.int64)
    crow[1:] = torch.cumsum(torch.bincount(ii, minlength=N), 0)
    A = SparseLinearOperator(crow, jj, vals, (*batch, N, N), is_hermitian=True)
    return A, A.fullmatrix()


# ------------------------------------------------------------------------------------------ construction
def test_construction_accepts_legal_structures():
    crow, col = _random_csr(9, 7, 5, seed=1, empty_every=3)
    v = torch.randn(col.numel(), dtype=DT)
    A = SparseLinearOperator(crow, col, v, (9, 7))
    assert A.shape == (9, 7) and A.crow.dtype == torch.int32 and A.col.dtype == torch.int32
    assert torch.allclose(A.fullmatrix(), _dense(crow, col, v, 9, 7))
    A32 = SparseLinearOperator(crow.to(torch.int32), col.to(torch.int32), v, (9, 7))
    assert torch.equal(A32.fullmatrix(), A.fullmatrix())
    Z = SparseLinearOperator(torch.zeros(5, dtype=torch.int64), torch.zeros(0, dtype=torch.int64),
                             torch.zeros(0, dtype=DT), (4, 6))
    assert torch.equal(Z.mm(torch.randn(6, 3, dtype=DT)), torch.zeros(4, 3, dtype=DT))
    # duplicates add up
    D = SparseLinearOperator(torch.tensor([0, 3]), torch.tensor([1, 1, 0]), torch.tensor([1.0, 2.0, 5.0], dtype=DT),
                             (1, 2))
    assert torch.equal(D.fullmatrix(), torch.tensor([[5.0, 3.0]], dtype=DT))
    # batched values, shape given as (M, N) or (*B, M, N)
    vb = torch.randn(3, col.numel(), dtype=DT)
    assert SparseLinearOperator(crow, col, vb, (9, 7)).shape == (3, 9, 7)
    assert SparseLinearOperator(crow, col, vb, (3, 9, 7)).shape == (3, 9, 7)
    assert SparseLinearOperator(crow, col, v, (3, 9, 7)).shape == (3, 9, 7)


def test_from_torch_csr_and_coo():
    D = torch.tensor([[0, 2.0, 0, 1.0], [0, 0, 0, 0], [3.0, 0, 4.0, 0]], dtype=DT)
    A = SparseLinearOperator.from_torch(D.to_sparse_csr())
    assert torch.equal(A.fullmatrix(), D)
    idx = torch.tensor([[2, 0, 0, 2, 2], [0, 3, 1, 2, 0]])
    val = torch.tensor([1.0, 1.0, 2.0, 4.0, 2.0], dtype=DT)                 # (2, 0) twice, uncoalesced
    C = SparseLinearOperator.from_torch(torch.sparse_coo_tensor(idx, val, (3, 4)))
    assert torch.equal(C.fullmatrix(), D)
    Db = torch.stack([D, 2 * D])
    Ab = SparseLinearOperator.from_torch(Db.to_sparse_csr())
    assert Ab.shape == (2, 3, 4) and torch.equal(Ab.fullmatrix(), Db)


def test_construction_rejects_bad_structures():
    col = torch.tensor([0, 1, 2])
    v = torch.ones(3, dtype=DT)
    with pytest.raises(RuntimeError, match=r"crow_indices\[0\]"):
        SparseLinearOperator(torch.tensor([1, 2, 3]), col, v, (2, 3))
    with pytest.raises(RuntimeError, match="non-decreasing"):
        SparseLinearOperator(torch.tensor([0, 3, 2, 3]), col, v, (3, 3))
    with pytest.raises(RuntimeError, match="must equal nnz"):
        SparseLinearOperator(torch.tensor([0, 1, 2]), col, v, (2, 3))
    with pytest.raises(RuntimeError, match="M\\+1"):
        SparseLinearOperator(torch.tensor([0, 3]), col, v, (2, 3))
    with pytest.raises(RuntimeError, match="out of range"):
        SparseLinearOperator(torch.tensor([0, 1, 3]), torch.tensor([0, 1, 3]), v, (2, 3))
    with pytest.raises(RuntimeError, match="out of range"):
        SparseLinearOperator(torch.tensor([0, 1, 3]), torch.tensor([0, -1, 2]), v, (2, 3))
    with pytest.raises(RuntimeError, match="entries per member"):
        SparseLinearOperator(torch.tensor([0, 1, 3]), col, torch.ones(4, dtype=DT), (2, 3))
    with pytest.raises(RuntimeError, match="batch"):
        SparseLinearOperator(torch.tensor([0, 1, 3]), col, torch.ones(2, 3, dtype=DT), (4, 2, 3))
    with pytest.raises(RuntimeError, match="int32 / int64"):
        SparseLinearOperator(torch.tensor([0, 1, 3]), col.double(), v, (2, 3))
    D = torch.tensor([[[1.0, 0], [0, 1.0]], [[0, 1.0], [1.0, 0]]], dtype=DT)
    with pytest.raises(RuntimeError, match="share one sparsity pattern"):
        SparseLinearOperator.from_torch(D.to_sparse_csr())
    with pytest.raises(RuntimeError, match="sparse CSR or COO"):
        SparseLinearOperator.from_torch(D[0])


def test_nnz_limit_is_checked_before_anything_is_built():
    # an index vector with 2^31 entries would need 8 GiB; the limit is a plain comparison on numel()
    col = torch.zeros(1, dtype=torch.int32).expand(2 ** 31)
    with pytest.raises(RuntimeError, match="2\\^31"):
        SparseLinearOperator(torch.zeros(2, dtype=torch.int64), col, torch.zeros(1, dtype=DT).expand(2 ** 31), (1, 1))


# ------------------------------------------------------------------------------------------ torch expression
@pytest.mark.parametrize("batch", [(), (3,), (2, 3)])
@pytest.mark.parametrize("shape", [(11, 11), (9, 6), (5, 13)])
def test_csr_apply_torch_matches_dense(batch, shape):
    M, N = shape
    crow, col = _random_csr(M, N, 6, seed=M * N, empty_every=4)
    vals = torch.randn((*batch, col.numel()), dtype=DT)
    A = SparseLinearOperator(crow, col, vals, (*batch, M, N))
    D = _dense(crow, col, vals, M, N)
    x = torch.randn((*batch, N, 3), dtype=DT)
    z = torch.randn((*batch, M, 3), dtype=DT)
    assert torch.allclose(A.mm(x), D @ x, atol=1e-13)
    assert torch.allclose(A.mv(x[..., 0]), (D @ x)[..., 0], atol=1e-13)
    assert torch.allclose(A.rmm(z), D.transpose(-2, -1) @ z, atol=1e-13)
    assert torch.allclose(A.rmv(z[..., 0]), (D.transpose(-2, -1) @ z)[..., 0], atol=1e-13)
    assert torch.allclose(A.fullmatrix(), D.expand(*batch, M, N))
    assert torch.allclose(csr_apply_torch(A.crow, A.col, vals, x, M, N), D @ x, atol=1e-13)
    # values broadcast over a batch of right-hand sides
    v1 = torch.randn(col.numel(), dtype=DT)
    A1 = SparseLinearOperator(crow, col, v1, (M, N))
    xb = torch.randn(4, N, 2, dtype=DT)
    assert torch.allclose(A1.mm(xb), _dense(crow, col, v1, M, N) @ xb, atol=1e-13)


def test_checklinop_passes():
    crow, col = _random_csr(10, 8, 4, seed=5)
    A = SparseLinearOperator(crow, col, torch.randn(col.numel(), dtype=DT), (10, 8))
    checklinop(A)
    A.check()
    S, _ = _spd_operator(12, seed=2)
    S.check()


def test_params_are_the_values_only():
    crow, col = _random_csr(6, 6, 3, seed=7)
    A = SparseLinearOperator(crow, col, torch.randn(col.numel(), dtype=DT), (6, 6))
    assert A.getlinopparams() == [A.values]


def test_complex_values_take_the_torch_expression():
    crow, col = _random_csr(7, 7, 3, seed=8)
    v = torch.randn(col.numel(), dtype=torch.complex128)
    A = SparseLinearOperator(crow, col, v, (7, 7))
    D = _dense(crow, col, v, 7, 7)
    x = torch.randn(7, 2, dtype=torch.complex128)
    assert torch.allclose(A.mm(x), D @ x) and torch.allclose(A.rmm(x), D.conj().transpose(-2, -1) @ x)


# ------------------------------------------------------------------------------------------ gradients
@pytest.mark.parametrize("vbatch", [(), (2,)])
@pytest.mark.parametrize("trans", [False, True])
def test_gradcheck_values_and_x(vbatch, trans):
    M, N = 6, 5
    crow, col = _random_csr(M, N, 4, seed=11, empty_every=5)
    vals = torch.randn((*vbatch, col.numel()), dtype=DT, requires_grad=True)
    x = torch.randn(2, M if trans else N, 3, dtype=DT, requires_grad=True)

    def f(v, xx):
        A = SparseLinearOperator(crow, col, v, (M, N))
        return A.rmm(xx) if trans else A.mm(xx)
    assert torch.autograd.gradcheck(f, (vals, x))
    assert torch.autograd.gradgradcheck(f, (vals, x))


# ------------------------------------------------------------------------------------------ host solvers
@pytest.mark.parametrize("mode", ["lowest", "uppest"])
def test_host_davidson_matches_exacteig(mode):
    A, D = _spd_operator(60, seed=3, batch=(2,))
    ev, evec = symeig(A, neig=3, mode=mode, method="davidson", min_eps=1e-10)
    ref = torch.linalg.eigvalsh(D)
    ref = ref[..., :3] if mode == "lowest" else ref[..., -3:].flip(-1)
    assert torch.allclose(ev.sort(-1).values, ref.sort(-1).values, atol=1e-8)
    ev2, _ = symeig(A, neig=3, mode=mode, method="exacteig")
    assert torch.allclose(ev.sort(-1).values, ev2.sort(-1).values, atol=1e-8)


@pytest.mark.parametrize("method", ["cg", "bicgstab", "gmres"])
def test_host_solve_matches_dense(method):
    A, D = _spd_operator(50, seed=4, batch=(2,))
    B = torch.randn(2, 50, 2, dtype=DT)
    x = solve(A, B, method=method, rtol=1e-11, atol=1e-14)
    assert torch.allclose(x, torch.linalg.solve(D, B), atol=1e-8)


# ------------------------------------------------------------------------------------------ C ABI
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Fn:
    argtypes = None
    restype = None


class _FakeLib:
    def __init__(self, names):
        for n in names:
            setattr(self, n, _Fn())


def test_header_and_binding_declare_csr_entry_points():
    syms = set(_capi.header_symbols())
    names = ["xk_csr_mm_f64", "xk_csr_mm_f32", "xk_csr_sddmm_f64", "xk_csr_sddmm_f32"]
    assert set(names) <= syms
    L = _FakeLib(sorted(syms))
    _capi._declare(L)
    txt = open(_capi.HEADER_PATH).read()
    for name in names:
        f = getattr(L, name)
        assert f.argtypes is not None and f.restype is not None, name
        proto = re.search(r"\b%s\s*\(([^)]*)\)" % name, txt).group(1)
        assert len(f.argtypes) == len(proto.split(",")), name
    src = open(os.path.join(ROOT, "xitorch_amd", "csrc", "xk_sparse.hip")).read()
    for name in names:
        assert name.rsplit("_", 1)[0] + "_##SUF" in src
