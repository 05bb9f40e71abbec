"""CPU: fsai() on host-memory operators (linalg/host_precond.py) against a dense numpy restatement written from the
formulas (tests/fsai_cases.py: per row, solve A_JJ y = e_m, g = conj(y) / sqrt(Re y_m)).

Per-entry bound: the row is the last column of A_JJ^-1 scaled, computed through a Cholesky factorisation, so
|g - g_ref| <= c m eps kappa_2(A_JJ) |g_ref|_inf; c = 16 covers the factorisation, the one triangular solve and the
restatement's own LU solve.  The three exact properties hold to rounding whatever the pattern."""
import warnings
import numpy as np
import pytest
import torch
import xitorch_amd as xa
from xitorch_amd.linop import SparseLinearOperator
from xitorch_amd.linalg import fsai, FSAIOperator
from tests import fsai_cases as fc
from tests.fsai_cases import random_hpd, check_rows

DTYPES = [torch.float64, torch.complex128, torch.float32, torch.complex64]
N = 61


def op_of(crow, col, vals, dtype, n=N):
    v = torch.as_tensor(vals).to(dtype)
    return SparseLinearOperator(torch.as_tensor(crow), torch.as_tensor(col), v, (*v.shape[:-1], n, n),
                                is_hermitian=True)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("power", [1, 2])
def test_values_properties_and_pattern(dtype, power):
    crow, col, vals, H = random_hpd(dtype, density=0.12 if power == 1 else 0.04, n=N)
    A = op_of(crow, col, vals, dtype)
    P = fsai(A, power=power)
    assert isinstance(P, FSAIOperator) and P.is_hermitian and P.shape == A.shape
    assert P.dtype == dtype and P.device == A.device and P._getparamnames() == []
    assert P.nfallback.shape == (2,) and int(P.nfallback.sum()) == 0 and not P.nfallback.dtype.is_floating_point
    Gd = fc.g_dense(P)
    Ain = torch.as_tensor(vals).to(dtype).numpy()                   # the values as the operator holds them
    for b in range(2):
        Ad = fc.dense_of(crow, col, Ain[b], N)[0]
        pattern = fc.pattern_dense(H[b], power, 32)
        # stored structure of G: sorted, unique, the diagonal last
        gp, gi = P.G.crow.numpy(), P.G.col.numpy()
        for i in range(N):
            assert list(gi[gp[i]:gp[i + 1]]) == pattern[i]
        check_rows(Gd[b], Ad, pattern, dtype)


def test_max_row_keeps_the_columns_nearest_the_diagonal():
    n = 40
    rng = np.random.default_rng(3)
    rows, cols = np.nonzero(np.tril(np.ones((n, n), dtype=bool)))          # a dense lower triangle
    crow = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=crow[1:])
    vals = np.where(rows == cols, 2.0 * n, rng.uniform(-1, 1, rows.size))
    P = fsai(op_of(crow, cols, vals, torch.float64, n), max_row=6)
    pattern = [list(range(max(0, i - 5), i + 1)) for i in range(n)]
    gp, gi = P.G.crow.numpy(), P.G.col.numpy()
    for i in range(n):
        assert list(gi[gp[i]:gp[i + 1]]) == pattern[i]
    assert int(P.nfallback) == 0
    check_rows(fc.g_dense(P)[0], fc.dense_of(crow, cols, vals, n)[0], pattern, torch.float64)


def test_a_missing_diagonal_entry_is_added_to_the_pattern():
    n = 30
    # lower bidiagonal storage, the diagonal entries of rows 5 and 17 not stored: a_ii = 0 there, so the blocks of rows
    # 5, 6, 17 and 18 are indefinite
    rows = np.array([i for i in range(n) for j in (i - 1, i) if j >= 0 and not (j == i and i in (5, 17))])
    cols = np.array([j for i in range(n) for j in (i - 1, i) if j >= 0 and not (j == i and i in (5, 17))])
    crow = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=crow[1:])
    vals = np.where(rows == cols, 4.0, -1.0)
    with pytest.warns(xa.MathWarning, match="4 row"):
        P = fsai(op_of(crow, cols, vals, torch.float64, n))
    pattern = [list(range(max(0, i - 1), i + 1)) for i in range(n)]
    gp, gi = P.G.crow.numpy(), P.G.col.numpy()
    for i in range(n):
        assert list(gi[gp[i]:gp[i + 1]]) == pattern[i]
    assert int(P.nfallback) == 4
    Gd = fc.g_dense(P)[0]
    Gr, nfall, _ = fc.fsai_dense(fc.dense_of(crow, cols, vals, n)[0], pattern)
    assert nfall == 4 and np.abs(Gd - Gr).max() <= 1e-15
    assert Gd[5, 5] == 1.0 and Gd[17, 17] == 1.0 and Gd[6, 6] == 0.5 and Gd[6, 5] == 0.0


def test_upper_triangle_and_diagonal_imaginary_part_are_not_read():
    crow, col, vals, H = random_hpd(torch.complex128, nb=1)
    rows = np.repeat(np.arange(N), np.diff(crow))
    P0 = fsai(op_of(crow, col, vals, torch.complex128))
    junk = vals.copy()
    junk[:, col > rows] = 1e30 + 5j
    junk[:, col == rows] += 3j
    P1 = fsai(op_of(crow, col, junk, torch.complex128))
    assert torch.equal(P0.G.values, P1.G.values) and torch.equal(P0.G.col, P1.G.col)


def test_duplicates_add_up():
    crow, col, vals, H = random_hpd(torch.float64, nb=1)
    rows = np.repeat(np.arange(N), np.diff(crow))
    # every entry stored twice, as 0.25 v and 0.75 v
    order = np.argsort(np.concatenate([rows, rows]), kind="stable")
    col2 = np.concatenate([col, col])[order]
    vals2 = np.concatenate([0.25 * vals, 0.75 * vals], axis=1)[:, order]
    P0, P1 = fsai(op_of(crow, col, vals, torch.float64)), fsai(op_of(2 * crow, col2, vals2, torch.float64))
    assert torch.equal(P0.G.col, P1.G.col)
    assert torch.allclose(P0.G.values, P1.G.values, rtol=1e-13, atol=0)


@pytest.mark.parametrize("dtype", [torch.float64, torch.complex64])
def test_indefinite_block_falls_back_with_a_warning(dtype):
    crow, col, vals, H = random_hpd(dtype, nb=2)
    rows = np.repeat(np.arange(N), np.diff(crow))
    vals = vals.copy()
    vals[1, (rows == 30) & (col == 30)] = -4.0                        # member 1 only: a negative diagonal entry
    A = op_of(crow, col, vals, dtype)
    with pytest.warns(xa.MathWarning, match="fell back"):
        P = fsai(A)
    nf = P.nfallback.tolist()
    assert nf[0] == 0 and nf[1] >= 1
    Gd = fc.g_dense(P)
    assert Gd[1][30, 30] == pytest.approx(0.5) and np.count_nonzero(Gd[1][30]) == 1
    # every block that contains index 30 is indefinite as well; P stays positive definite
    ev = np.linalg.eigvalsh(P.fullmatrix().numpy().astype(np.complex128))
    assert ev.min() > 0


def test_nan_is_flagged():
    crow, col, vals, H = random_hpd(torch.float64, nb=1)
    rows = np.repeat(np.arange(N), np.diff(crow))
    vals = vals.copy()
    k = np.nonzero((rows == 20) & (col < 20))[0][0]
    vals[0, k] = np.nan
    vals[0, (rows == 40) & (col == 40)] = np.inf
    with pytest.warns(xa.MathWarning):
        P = fsai(op_of(crow, col, vals, torch.float64))
    assert int(P.nfallback.sum()) >= 2
    assert bool(torch.isfinite(P.G.values).all())
    Gd = fc.g_dense(P)[0]
    assert np.count_nonzero(Gd[20]) == 1 and Gd[40, 40] == 1.0 and np.count_nonzero(Gd[40]) == 1


@pytest.mark.parametrize("dtype", [torch.float64, torch.complex128])
def test_operator_is_hermitian_positive_definite(dtype):
    crow, col, vals, H = random_hpd(dtype, nb=2)
    A = op_of(crow, col, vals, dtype)
    P = fsai(A)
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, N, 3, dtype=dtype, generator=g)
    assert torch.equal(P.mm(x), P.rmm(x)) and torch.equal(P.mv(x[..., 0]), P.rmv(x[..., 0]))
    F = P.fullmatrix()
    assert torch.allclose(F, F.mH, rtol=0, atol=1e-14)
    Gd = torch.as_tensor(fc.g_dense(P))
    assert torch.allclose(F, Gd.mH @ Gd, rtol=1e-13, atol=1e-15)
    assert float(torch.linalg.eigvalsh(F).min()) > 0
    # quality: G A G^H is far better conditioned than A scaled by its diagonal would need to be; here only sanity
    M = Gd @ torch.as_tensor(H) @ Gd.mH
    assert float(torch.linalg.cond(M).max()) < float(torch.linalg.cond(torch.as_tensor(H)).max()) + 1e-9


def test_values_are_read_detached_and_broadcast_values():
    crow, col, vals, H = random_hpd(torch.float64, nb=1)
    v = torch.as_tensor(vals[0]).requires_grad_()
    A = SparseLinearOperator(torch.as_tensor(crow), torch.as_tensor(col), v, (3, N, N), is_hermitian=True)
    P = fsai(A)
    assert not P.G.values.requires_grad and P.G.values.dim() == 1 and tuple(P.shape) == (3, N, N)
    assert tuple(P.nfallback.shape) == (3,)
    y = P.mm(torch.ones(3, N, 2, dtype=torch.float64))
    assert y.shape == (3, N, 2) and not y.requires_grad


def test_argument_checks():
    crow, col, vals, H = random_hpd(torch.float64, nb=1)
    A = op_of(crow, col, vals, torch.float64)
    with pytest.raises(TypeError):
        fsai(xa.LinearOperator.m(torch.eye(4, dtype=torch.float64)))
    rect = SparseLinearOperator(torch.tensor([0, 1, 2]), torch.tensor([0, 1]), torch.ones(2), (2, 3))
    with pytest.raises(TypeError):
        fsai(rect)
    for bad in (dict(power=0), dict(power=5), dict(max_row=0), dict(max_row=33), dict(power=1.5)):
        with pytest.raises(ValueError):
            fsai(A, **bad)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        fsai(A, power=4, max_row=1)                         # max_row = 1 is Jacobi scaling, no fallback involved
