"""-m gpu: xk_fsai_build_{f64,f32,c128,c64} per entry against the float64 / complex128 host restatement
(linalg/host_precond.fsai_values on the CPU, itself checked against a dense numpy restatement by tests/test_fsai_ref.py).

Tolerance per row: |g - g_ref|_inf <= 16 m eps(dtype) kappa_2(A_JJ) |g_ref|_inf — the Cholesky-solve error bound with
a constant for the gather sums; kappa_2 is computed here in float64 and the inputs are strictly diagonally dominant
(kappa_2 <= 10 for every block, asserted), so the bound means something in fp32 too.  The kernel is never compared
with itself except for run-to-run reproducibility.  Every case is a handful of rows: well under a second."""
import numpy as np
import pytest
import torch
from xitorch_amd import kernels as K
from xitorch_amd.linalg import host_precond as hp
from tests import fsai_cases as fc

pytestmark = pytest.mark.gpu
DTYPES = [torch.float64, torch.float32, torch.complex128, torch.complex64]
WIDE = {torch.float64: torch.float64, torch.float32: torch.float64, torch.complex128: torch.complex128,
        torch.complex64: torch.complex128}


def _rows_of(crow):
    return np.repeat(np.arange(len(crow) - 1), np.diff(crow))


def _run(dev, dtype, crow, col, vals, n, power=1, max_row=32, broadcast=False):
    """kernel output, its failure counts and the wide host restatement on one pattern.  vals (nb, nnz) numpy in
    float64 / complex128; broadcast: the kernel gets the first member as a (1, nnz) array with stride 0"""
    crow_t, col_t = torch.as_tensor(crow), torch.as_tensor(col)
    rows_t = torch.as_tensor(_rows_of(crow))
    v = torch.as_tensor(np.ascontiguousarray(vals)).to(dtype).contiguous()   # the numbers the kernel sees
    if broadcast:
        v = v[:1].contiguous()
    g_ptr, g_idx = hp.fsai_pattern(rows_t, col_t, n, power, max_row)
    ref, nf_ref = hp.fsai_values(rows_t, col_t, v.to(WIDE[dtype]), g_ptr, g_idx, n)
    args = (crow_t.to(torch.int32).to(dev), col_t.to(torch.int32).to(dev), v.to(dev), g_ptr.to(dev), g_idx.to(dev), n)
    out, nfail = K.fsai_build(*args)
    out2, nfail2 = K.fsai_build(*args)
    assert torch.equal(out, out2) and torch.equal(nfail, nfail2), "two runs differ"
    assert out.dtype == dtype and out.shape == ref.shape
    return out.cpu(), nfail.cpu(), ref, nf_ref, g_ptr.numpy(), g_idx.numpy(), v


def _check(out, ref, g_ptr, g_idx, crow, col, v, n, dtype, c=16, kappa_max=10.0):
    """per row against the wide restatement with the kappa-scaled bound; then the exact properties in double"""
    eps = torch.finfo(dtype).eps
    Ain = v.to(WIDE[dtype]).numpy()
    worst = 0.0
    for b in range(out.shape[0]):
        H = fc.hermitian_from_lower(fc.dense_of(crow, col, Ain[b], n)[0])
        o, r = out[b].to(WIDE[dtype]).numpy(), ref[b].numpy()
        pattern = []
        for i in range(n):
            S = list(g_idx[g_ptr[i]:g_ptr[i + 1]])
            pattern.append(S)
            kap = np.linalg.cond(H[np.ix_(S, S)])
            assert kap <= kappa_max, (i, kap)
            seg = slice(g_ptr[i], g_ptr[i + 1])
            err = np.abs(o[seg] - r[seg]).max()
            unit = len(S) * eps * kap * np.abs(r[seg]).max()
            worst = max(worst, err / unit)
            assert err <= c * unit, (b, i, err / unit)
        Gd = fc.dense_of(g_ptr, g_idx, o, n)[0]
        fc.check_rows(Gd, H, pattern, dtype, c=c)
    return worst


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", [1, 2, 5, 257])
def test_random_patterns_vs_wide_restatement(dev, dtype, n):
    # n = 5 and 257: a partial last workgroup (four rows per workgroup); B = 3 member-specific values, then B = 1
    # with one broadcast set.  Unsorted columns, both triangles stored.
    density = {1: 0.0, 2: 1.0, 5: 0.6, 257: 0.03}[n]
    crow, col, vals, H = fc.random_hpd(dtype, nb=3, seed=n, density=density, n=n)
    if n == 257:
        # the blocks contain pairs that A does not store: S_i x S_i is not a clique of A's graph
        g_ptr, g_idx = hp.fsai_pattern(torch.as_tensor(_rows_of(crow)), torch.as_tensor(col), n)
        stored = set(zip(_rows_of(crow).tolist(), col.tolist()))
        missing = sum((int(a), int(b)) not in stored for i in range(n)
                      for a in g_idx[g_ptr[i]:g_ptr[i + 1]] for b in g_idx[g_ptr[i]:g_ptr[i + 1]] if b < a)
        assert missing > 0
    for broadcast in (False, True):
        out, nfail, ref, nf_ref, g_ptr, g_idx, v = _run(dev, dtype, crow, col, vals, n, broadcast=broadcast)
        assert out.shape[0] == (1 if broadcast else 3)
        assert nfail.tolist() == [0] * out.shape[0] and int(nf_ref.sum()) == 0
        _check(out, ref, g_ptr, g_idx, crow, col, v, n, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_diagonal_matrix(dev, dtype):
    n = 7
    crow, col = np.arange(n + 1), np.arange(n)
    vals = np.array([[0.25, 1.0, 4.0, 9.0, 16.0, 100.0, 1e-4]])
    out, nfail, ref, nf_ref, g_ptr, g_idx, v = _run(dev, dtype, crow, col, vals, n)
    assert list(np.diff(g_ptr)) == [1] * n and int(nfail) == 0
    _check(out, ref, g_ptr, g_idx, crow, col, v, n, dtype)
    expect = torch.as_tensor(1 / np.sqrt(vals)).to(dtype)
    assert torch.allclose(out, expect, rtol=4 * torch.finfo(dtype).eps, atol=0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("power,max_row", [(1, 32), (1, 31), (2, 32)])
def test_rows_at_the_cap(dev, dtype, power, max_row):
    # a dense lower triangle of order 40: rows 31 .. 39 have exactly 32 columns after the truncation (m = 32 fills the
    # packed triangle in LDS); power = 2 on a band of half-width 20 reaches the cap through the pattern product
    n = 40
    rng = np.random.default_rng(7)
    full = np.tril(np.ones((n, n), dtype=bool))
    if power == 2:
        full &= (np.arange(n)[:, None] - np.arange(n)[None, :]) <= 20
    rows, cols = np.nonzero(full)
    crow = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=crow[1:])
    cplx = dtype.is_complex
    vals = rng.uniform(-1, 1, (2, rows.size)) + (1j * rng.uniform(-1, 1, (2, rows.size)) if cplx else 0)
    vals[:, rows == cols] = 3.0 * n                                # strictly dominant: kappa <= 10
    out, nfail, ref, nf_ref, g_ptr, g_idx, v = _run(dev, dtype, crow, cols, vals, n, power=power, max_row=max_row)
    assert int(np.diff(g_ptr).max()) == max_row and nfail.tolist() == [0, 0]
    _check(out, ref, g_ptr, g_idx, crow, cols, v, n, dtype)


@pytest.mark.parametrize("dtype", DTYPES)
def test_duplicates_unsorted_and_upper_garbage(dev, dtype):
    n = 37
    crow, col, vals, H = fc.random_hpd(dtype, nb=2, seed=11, density=0.2, n=n)
    rows = _rows_of(crow)
    # canonical form: columns ascending, nothing stored twice
    order = np.lexsort((col, rows))
    can = _run(dev, dtype, crow, col[order], vals[:, order], n)
    # every entry stored twice in the unsorted order of random_hpd, as a = 0.75 v (rounded in the kernel's dtype) and
    # b = v - a, which is exact there (a lies within a factor two of v), so both operators hold the same matrix
    nd = {torch.float64: np.float64, torch.float32: np.float32, torch.complex128: np.complex128,
          torch.complex64: np.complex64}[dtype]
    vn = np.ascontiguousarray(vals.astype(nd))
    rd = vn.real.dtype
    a = (vn.view(rd) * rd.type(0.75)).view(nd)
    b = vn - a
    assert np.array_equal(a + b, vn)
    order2 = np.argsort(np.concatenate([rows, rows]), kind="stable")
    col2 = np.concatenate([col, col])[order2]
    vals2 = np.concatenate([a, b], axis=1)[:, order2].astype(vals.dtype)
    dup = _run(dev, dtype, 2 * crow, col2, vals2, n)
    for out, nfail, ref, nf_ref, g_ptr, g_idx, v in (can, dup):
        assert nfail.tolist() == [0, 0]
    assert np.array_equal(can[4], dup[4]) and np.array_equal(can[5], dup[5])
    _check(can[0], can[2], can[4], can[5], crow, col[order], can[6], n, dtype)
    _check(dup[0], dup[2], dup[4], dup[5], 2 * crow, col2, dup[6], n, dtype)
    # ... and the two kernel results agree within the same bound (through the canonical reference)
    _check(dup[0], can[2], can[4], can[5], crow, col[order], can[6], n, dtype)
    # garbage above the diagonal (and an imaginary part on it) changes nothing, bit for bit
    junk = vals.copy()
    junk[:, col > rows] = 1e30
    if dtype.is_complex:
        junk[:, col == rows] += 2j
    g = _run(dev, dtype, crow, col, junk, n)
    plain = _run(dev, dtype, crow, col, vals, n)
    assert torch.equal(g[0], plain[0])
    # only the lower triangle stored: the same G
    low = col <= rows
    crow_l = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows[low], minlength=n), out=crow_l[1:])
    lo = _run(dev, dtype, crow_l, col[low], vals[:, low], n)
    assert torch.equal(lo[0], plain[0])


@pytest.mark.parametrize("dtype", DTYPES)
def test_fallback_rows_and_counts(dev, dtype):
    """member 0: all rows fine; member 1: the block of row 6 is indefinite ([[1, 2], [2, 1]]); member 2: a zero
    diagonal in row 3 (an uncoupled row) and a NaN on the diagonal of the uncoupled row 9.  Counts are exact."""
    n = 12
    ent = [(i, i) for i in range(n)] + [(6, 5), (5, 6), (2, 1), (1, 2), (11, 10), (10, 11)]
    ent.sort()
    rows, cols = np.array([e[0] for e in ent]), np.array([e[1] for e in ent])
    crow = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=crow[1:])
    base = np.where(rows == cols, 4.0, 1.0)
    vals = np.stack([base, base, base]).astype(np.complex128 if dtype.is_complex else np.float64)
    k = lambda r, c: int(np.nonzero((rows == r) & (cols == c))[0][0])
    vals[1, k(5, 5)] = vals[1, k(6, 6)] = 1.0
    vals[1, k(6, 5)] = vals[1, k(5, 6)] = 2.0
    vals[2, k(3, 3)] = 0.0
    vals[2, k(9, 9)] = np.nan
    crow_t, col_t, rows_t = torch.as_tensor(crow), torch.as_tensor(cols), torch.as_tensor(rows)
    v = torch.as_tensor(np.ascontiguousarray(vals)).to(dtype).contiguous()
    g_ptr, g_idx = hp.fsai_pattern(rows_t, col_t, n)
    ref, nf_ref = hp.fsai_values(rows_t, col_t, v.to(WIDE[dtype]), g_ptr, g_idx, n)
    out, nfail = K.fsai_build(crow_t.to(torch.int32).to(dev), col_t.to(torch.int32).to(dev), v.to(dev), g_ptr.to(dev),
                              g_idx.to(dev), n)
    assert nfail.tolist() == [0, 1, 2] and nf_ref.tolist() == [0, 1, 2]
    assert bool(torch.isfinite(out).all())
    G = fc.dense_of(g_ptr.numpy(), g_idx.numpy(), out.cpu().numpy(), n)
    assert G[1][6, 6] == 1.0 and G[1][6, 5] == 0.0                  # Jacobi row: 1 / sqrt(|a_66|), a_66 = 1
    assert G[2][3, 3] == 1.0 and G[2][9, 9] == 1.0                  # zero and non-finite diagonal: 1
    assert G[0][6, 6] != 1.0 and G[2][6, 5] != 0.0
    tol = 16 * 2 * torch.finfo(dtype).eps * 4
    assert float((out.cpu().to(WIDE[dtype]) - ref).abs().max()) <= tol
    # a NaN off the diagonal: the rows whose block holds it are flagged, the others are not, nothing hangs
    vals[2, k(9, 9)] = 4.0
    vals[2, k(11, 10)] = np.nan
    v = torch.as_tensor(np.ascontiguousarray(vals)).to(dtype).contiguous()
    out, nfail = K.fsai_build(crow_t.to(torch.int32).to(dev), col_t.to(torch.int32).to(dev), v.to(dev), g_ptr.to(dev),
                              g_idx.to(dev), n)
    assert nfail.tolist() == [0, 1, 2] and bool(torch.isfinite(out).all())
    G = fc.dense_of(g_ptr.numpy(), g_idx.numpy(), out.cpu().numpy(), n)
    assert G[2][11, 11] == 0.5 and G[2][11, 10] == 0.0


def test_pattern_beyond_the_cap_is_refused_by_the_wrapper(dev):
    n = 40
    rows, cols = np.nonzero(np.tril(np.ones((n, n), dtype=bool)))
    crow = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=crow[1:])
    ci = lambda a: torch.as_tensor(a).to(torch.int32).to(dev)
    vals = torch.ones((1, rows.size), dtype=torch.float64, device=dev)
    from xitorch_amd._capi import NativeLibraryError
    with pytest.raises(NativeLibraryError, match="cap"):
        K.fsai_build(ci(crow), ci(cols), vals, ci(crow), ci(cols), n)          # G's pattern = A's: rows of 40
