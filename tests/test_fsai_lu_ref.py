"""CPU: the host restatement of the unsymmetric FSAI (linalg/host_precond.fsai_lu_values, the full-structure pattern of
fsai_pattern) against a plain per-row numpy restatement (tests/fsai_lu_cases.fsai_lu_dense: np.linalg.solve on each
gathered block and on its transpose), the exact properties of the factors in double, duplicates and unsorted columns,
the structurally exact fallback rows, and the equality with fsai(A) on a Hermitian positive definite operator."""
import warnings
import numpy as np
import pytest
import torch
from xitorch_amd._util import MathWarning
from xitorch_amd.linop import SparseLinearOperator
from xitorch_amd.linalg import fsai, fsai_lu, host_precond as hp
from tests import fsai_cases as fc
from tests import fsai_lu_cases as lc

DTYPES = [torch.float64, torch.float32, torch.complex128, torch.complex64]
WIDE = {torch.float64: np.float64, torch.float32: np.float64, torch.complex128: np.complex128,
        torch.complex64: np.complex128}
NP = {torch.float64: np.float64, torch.float32: np.float32, torch.complex128: np.complex128,
      torch.complex64: np.complex64}


def _values(dtype, crow, col, vals, n, power=1, max_row=32):
    rows_t, col_t = torch.as_tensor(lc.rows_of(crow)), torch.as_tensor(col)
    v = torch.as_tensor(np.ascontiguousarray(vals)).to(dtype).contiguous()
    g_ptr, g_idx = hp.fsai_pattern(rows_t, col_t, n, power, max_row, full=True)
    gl, w, nf = hp.fsai_lu_values(rows_t, col_t, v, g_ptr, g_idx, n)
    return v, g_ptr.numpy(), g_idx.numpy(), gl, w, nf


def _against_numpy(dtype, crow, col, vals, n, power=1, max_row=32, c=16):
    """both factors per row against the numpy restatement in double, within c m eps kappa |ref|_inf"""
    v, g_ptr, g_idx, gl, w, nf = _values(dtype, crow, col, vals, n, power, max_row)
    assert nf.tolist() == [0] * v.shape[0]
    eps = torch.finfo(dtype).eps
    Ad = lc.dense_of(crow, col, v.numpy().astype(WIDE[dtype]), n)
    pattern = lc.pattern_lists(g_ptr, g_idx)
    GLs = lc.dense_of(g_ptr, g_idx, gl.numpy().astype(WIDE[dtype]), n)
    GUs = np.conj(np.swapaxes(lc.dense_of(g_ptr, g_idx, w.numpy().astype(WIDE[dtype]), n), -2, -1))
    for b in range(v.shape[0]):
        GLr, GUr, nfall, kap = lc.fsai_lu_dense(Ad[b], pattern)
        assert nfall == 0
        for i, S in enumerate(pattern):
            assert set(np.nonzero(GLs[b][i])[0]) <= set(S) and set(np.nonzero(GUs[b][:, i])[0]) <= set(S)
            unit = len(S) * eps * kap[i]
            assert np.abs(GLs[b][i] - GLr[i]).max() <= c * unit * np.abs(GLr[i]).max(), (b, i)
            assert np.abs(GUs[b][:, i] - GUr[:, i]).max() <= c * unit * np.abs(GUr[:, i]).max(), (b, i)
    return Ad, pattern, GLs, GUs


@pytest.mark.parametrize("dtype", DTYPES)
def test_values_against_the_numpy_restatement(dtype):
    for name, crow, col, vals, n, power, max_row in lc.kernel_cases(dtype.is_complex, NP[dtype]):
        _against_numpy(dtype, crow, col, vals, n, power, max_row)


@pytest.mark.parametrize("dtype", [torch.float64, torch.complex128])
def test_exact_properties_in_double(dtype):
    """(G_L A)[i, j] = 0 and (A G_U)[j, i] = 0 for j in S_i other than i, diag(G_L A G_U) = 1, a unit diagonal of G_L:
    every residual within 16 m eps kappa_2(A_SS) times the row's scale"""
    eps = torch.finfo(dtype).eps
    cases = lc.kernel_cases(dtype.is_complex, NP[dtype])
    Ac = lc.convdiff_complex(8, 0.5) if dtype.is_complex else lc.convdiff(8, 0.5)
    cases.append(("convdiff", *lc.csr_of_dense(Ac)[:2], lc.csr_of_dense(Ac)[2][None], 64, 2, 32))
    for name, crow, col, vals, n, power, max_row in cases:
        Ad, pattern, GL, GU = _against_numpy(dtype, crow, col, vals, n, power, max_row)
        for b in range(Ad.shape[0]):
            A = Ad[b]
            GLA, AGU = GL[b] @ A, A @ GU[b]
            absGLA, absAGU = np.abs(GL[b]) @ np.abs(A), np.abs(A) @ np.abs(GU[b])
            d = np.diag(GL[b] @ A @ GU[b])
            for i, S in enumerate(pattern):
                kap = np.linalg.cond(A[np.ix_(S, S)])
                tol = 16 * len(S) * eps * kap
                assert GL[b][i, i] == 1
                for j in S[:-1]:
                    assert abs(GLA[i, j]) <= tol * absGLA[i, S].max(), (name, i, j)
                    assert abs(AGU[j, i]) <= tol * absAGU[S, i].max(), (name, i, j)
                assert abs(d[i] - 1) <= tol * max(1.0, (np.abs(GL[b][i]) @ np.abs(A) @ np.abs(GU[b][:, i]))), (name, i)


@pytest.mark.parametrize("power", [1, 2, 3])
def test_pattern_symmetrises_the_whole_structure(power):
    rng = np.random.default_rng(power)
    n = 45
    stored = rng.random((n, n)) < 0.06                  # unsymmetric structure, some rows with nothing below the diagonal
    stored[7, :] = False
    stored[7, 30] = True                                # row 7 stores an upper entry only: (30, 7) enters row 30
    rows, cols = np.nonzero(stored)
    for max_row in (32, 5, 1):
        g_ptr, g_idx = hp.fsai_pattern(torch.as_tensor(rows), torch.as_tensor(cols), n, power, max_row, full=True)
        want = lc.pattern_dense(stored, power, max_row)
        assert lc.pattern_lists(g_ptr.numpy(), g_idx.numpy()) == want
        assert all(S[-1] == i for i, S in enumerate(want))
        if max_row == 5:
            full = lc.pattern_dense(stored, power, n)
            assert any(len(S) > 5 for S in full)
            assert all(S5 == S[-5:] for S5, S in zip(want, full)), "the cap keeps the columns nearest the diagonal"
    assert 7 in lc.pattern_dense(stored, 1, 32)[30]
    # the Hermitian pattern function is untouched: the lower triangle alone, as before
    g_ptr, g_idx = hp.fsai_pattern(torch.as_tensor(rows), torch.as_tensor(cols), n, power, 32)
    assert lc.pattern_lists(g_ptr.numpy(), g_idx.numpy()) == fc.pattern_dense(stored.astype(float), power, 32)


@pytest.mark.parametrize("dtype", DTYPES)
def test_duplicates_and_unsorted_columns(dtype):
    n = 37
    crow, col, vals, _ = lc.random_dominant(dtype.is_complex, nb=2, seed=11, density=0.2, n=n)
    rows = lc.rows_of(crow)
    order = np.lexsort((col, rows))
    can = _values(dtype, crow, col[order], vals[:, order], n)          # canonical: columns ascending, nothing twice
    uns = _values(dtype, crow, col, vals, n)
    dup = _values(dtype, *lc.with_duplicates(crow, col, vals, NP[dtype]), n)
    for other in (uns, dup):
        assert np.array_equal(can[1], other[1]) and np.array_equal(can[2], other[2])
    assert torch.equal(can[3], uns[3]) and torch.equal(can[4], uns[4])   # the sum of one entry has no order
    eps = torch.finfo(dtype).eps
    for k in (3, 4):
        assert float((can[k] - dup[k]).abs().max()) <= 16 * 32 * eps * 3 * float(can[k].abs().max())


@pytest.mark.parametrize("dtype", DTYPES)
def test_fallback_rows(dtype):
    crow, col, vals, counts = lc.fallback_case(dtype.is_complex)
    n = 12
    v, g_ptr, g_idx, gl, w, nf = _values(dtype, crow, col, vals, n)
    assert nf.tolist() == counts
    assert bool(torch.isfinite(gl).all()) and bool(torch.isfinite(w).all())
    GL = lc.dense_of(g_ptr, g_idx, gl.numpy(), n)
    W = lc.dense_of(g_ptr, g_idx, w.numpy(), n)
    for b, i, scale in ((1, 3, 1.0), (1, 5, 1.0), (1, 6, 1.0), (2, 9, 1.0), (2, 11, 0.25)):
        assert GL[b][i, i] == 1 and W[b][i, i] == scale, (b, i)
        assert np.count_nonzero(GL[b][i]) == 1 and np.count_nonzero(W[b][i]) == 1
    # the numpy restatement agrees on which rows fall back
    Ad = lc.dense_of(crow, col, v.numpy().astype(WIDE[dtype]), n)
    for b in range(3):
        assert lc.fsai_lu_dense(Ad[b], lc.pattern_lists(g_ptr, g_idx))[2] == counts[b]
    # through the public function: one warning that names the number
    A = SparseLinearOperator(torch.as_tensor(crow), torch.as_tensor(col), v, (3, n, n))
    with pytest.warns(MathWarning, match="5 row"):
        P = fsai_lu(A)
    assert P.nfallback.tolist() == counts


@pytest.mark.parametrize("phase", [False, True])
def test_equals_fsai_on_a_hermitian_positive_definite_operator(phase):
    dtype = torch.complex128 if phase else torch.float64
    A, dense = fc.grid_operator(10, nmembers=2, dtype=dtype, phase=phase)
    N = 100
    with warnings.catch_warnings():
        warnings.simplefilter("error", MathWarning)
        P, Plu = fsai(A), fsai_lu(A)
    eye = torch.eye(N, dtype=dtype).expand(2, N, N)
    Pd, Plud = P.mm(eye).numpy(), Plu.mm(eye).numpy()
    eps = torch.finfo(dtype).eps
    for b in range(2):
        bound = 64 * eps * np.linalg.cond(dense[b]) * np.linalg.norm(Pd[b], 2)
        assert np.abs(Pd[b] - Plud[b]).max() <= bound
        assert np.abs(Plu.H.mm(eye).numpy()[b] - np.conj(Plud[b].T)).max() <= bound
