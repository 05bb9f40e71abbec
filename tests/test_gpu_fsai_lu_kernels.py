"""-m gpu: xk_fsai_lu_build_{f64,f32,c128,c64} per row against the float64 / complex128 host restatement
(linalg/host_precond.fsai_lu_values on the CPU, itself checked against a per-row numpy restatement by
tests/test_fsai_lu_ref.py).

Tolerance per row and per factor: |g - g_ref|_inf <= C m eps(dtype) kappa_2(A_SS) |g_ref|_inf with C = 16, the form and
constant of tests/test_gpu_fsai_kernels.py; kappa_2 is computed here in double from the values the kernel sees, and
every block of every input has kappa_2 <= 10 (asserted), so the bound means something in fp32 too.

The constant comes from the Cholesky case and is not derived for pivoted LU, so it was checked against a library LU
before being relied on, never against the kernel: the float32 / complex64 host restatement (LAPACK getrf / getrs through
torch) against the float64 / complex128 one on the very inputs below (tests/fsai_lu_cases.kernel_cases, CPU,
test_library_lu_uses_under_a_quarter_of_the_bound below repeats it) reaches a worst ratio err / (m eps kappa |ref|) of
0.44 to 0.58 for float32 (two machines, two builds of the library) and 0.59 for complex64, well under a quarter of 16,
so C stays 16.  On an MI355X the kernel's own worst ratio was 0.45 (float64), 0.44 (float32), 0.42 (complex128) and
0.59 (complex64), in the pivoting and the full-row cases.  The kernel is never compared with itself except for run-to-run reproducibility.  Every case is a handful of rows:
well under a second."""
import numpy as np
import pytest
import torch
from xitorch_amd import kernels as K
from xitorch_amd._capi import NativeLibraryError
from xitorch_amd.linalg import host_precond as hp
from tests import fsai_lu_cases as lc

DTYPES = [torch.float64, torch.float32, torch.complex128, torch.complex64]
WIDE = {torch.float64: torch.float64, torch.float32: torch.float64, torch.complex128: torch.complex128,
        torch.complex64: torch.complex128}
NP = {torch.float64: np.float64, torch.float32: np.float32, torch.complex128: np.complex128,
      torch.complex64: np.complex64}
C = 16


def _host(dtype, crow, col, vals, n, power, max_row):
    """pattern, the values as `dtype` holds them, and the wide host restatement of them"""
    rows_t, col_t = torch.as_tensor(lc.rows_of(crow)), torch.as_tensor(col)
    v = torch.as_tensor(np.ascontiguousarray(vals)).to(dtype).contiguous()
    g_ptr, g_idx = hp.fsai_pattern(rows_t, col_t, n, power, max_row, full=True)
    ref = hp.fsai_lu_values(rows_t, col_t, v.to(WIDE[dtype]), g_ptr, g_idx, n)
    return rows_t, col_t, v, g_ptr, g_idx, ref


def _ratios(outs, refs, g_ptr, g_idx, crow, col, v, n, dtype, kappa_max=10.0):
    """worst err / (m eps kappa |ref|_inf) over rows, members and the two factors; asserts kappa <= kappa_max"""
    eps = torch.finfo(dtype).eps
    Ad = lc.dense_of(crow, col, v.to(WIDE[dtype]).numpy(), n)
    g_ptr, g_idx = g_ptr.numpy(), g_idx.numpy()
    worst = 0.0
    for b in range(outs[0].shape[0]):
        for i in range(n):
            S = list(g_idx[g_ptr[i]:g_ptr[i + 1]])
            kap = np.linalg.cond(Ad[b if Ad.shape[0] > 1 else 0][np.ix_(S, S)])
            assert kap <= kappa_max, (i, kap)
            seg = slice(g_ptr[i], g_ptr[i + 1])
            for o, r in zip(outs, refs):
                o_, r_ = o[b].to(WIDE[dtype]).numpy()[seg], r[b].numpy()[seg]
                worst = max(worst, np.abs(o_ - r_).max() / (len(S) * eps * kap * np.abs(r_).max()))
    return worst


def _kernel(dev, crow, col, v, g_ptr, g_idx, n):
    ci = lambda a: torch.as_tensor(a).to(torch.int32).to(dev)
    args = (ci(crow), ci(col), v.to(dev), g_ptr.to(dev), g_idx.to(dev), n)
    gl, w, nfail = K.fsai_lu_build(*args)
    gl2, w2, nfail2 = K.fsai_lu_build(*args)
    assert torch.equal(gl, gl2) and torch.equal(w, w2) and torch.equal(nfail, nfail2), "two runs differ"
    assert gl.dtype == v.dtype and w.dtype == v.dtype
    return gl.cpu(), w.cpu(), nfail.cpu()


@pytest.mark.parametrize("dtype", [torch.float32, torch.complex64])
def test_library_lu_uses_under_a_quarter_of_the_bound(dtype):
    """CPU: the calibration of C — the single-precision library restatement against the double one"""
    worst = 0.0
    for name, crow, col, vals, n, power, max_row in lc.kernel_cases(dtype.is_complex, NP[dtype]):
        rows_t, col_t, v, g_ptr, g_idx, ref = _host(dtype, crow, col, vals, n, power, max_row)
        gl, w, nf = hp.fsai_lu_values(rows_t, col_t, v, g_ptr, g_idx, n)
        assert int(nf.sum()) == 0 and int(ref[2].sum()) == 0
        worst = max(worst, _ratios((gl, w), ref[:2], g_ptr, g_idx, crow, col, v, n, dtype))
    print("library LU, %s: worst err / (m eps kappa |ref|) = %.3f" % (dtype, worst))
    assert worst <= C / 4, worst


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_cases_vs_wide_restatement(dev, dtype):
    """N = 5, 33, 70 (N B not a multiple of the waves per workgroup: idle waves in the last one), rows of 1, 2, 31 and
    32 columns, the cap through power = 2, a row of A of 120 stored entries with duplicates, unsorted columns, blocks
    that need pivoting (zero and 1e-9 diagonal entries), pivot ties; member-specific values and one broadcast set"""
    worst = {}
    lens = set()
    for name, crow, col, vals, n, power, max_row in lc.kernel_cases(dtype.is_complex, NP[dtype]):
        rows_t, col_t, v, g_ptr, g_idx, ref = _host(dtype, crow, col, vals, n, power, max_row)
        lens |= set(np.diff(g_ptr.numpy()).tolist())
        for v_k in (v, v[:1].contiguous()):                                   # B members, then sV = 0
            gl, w, nfail = _kernel(dev, crow, col, v_k, g_ptr, g_idx, n)
            nb = v_k.shape[0]
            assert gl.shape == (nb, g_idx.numel()) and nfail.tolist() == [0] * nb and int(ref[2].sum()) == 0
            r = _ratios((gl, w), (ref[0][:nb], ref[1][:nb]), g_ptr, g_idx, crow, col, v_k, n, dtype)
            worst[name] = max(worst.get(name, 0.0), r)
            # unit diagonal of G_L, exactly
            assert bool((gl[:, (g_ptr[1:] - 1).long()] == 1).all())
    print("%s: worst err / (m eps kappa |ref|) per case: %s" % (dtype, {k: round(x, 3) for k, x in worst.items()}))
    assert {1, 2, 31, 32} <= lens
    assert max(worst.values()) <= C, worst


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_single_member_sizes(dev, dtype):
    # B = 1 with N = 5, 33, 70: N B = 5, 33, 70 rows on 4 (complex128: 2) waves per workgroup
    for n, density in ((5, 0.6), (33, 0.15), (70, 0.06)):
        crow, col, vals, _ = lc.random_dominant(dtype.is_complex, nb=1, seed=100 + n, density=density, n=n)
        rows_t, col_t, v, g_ptr, g_idx, ref = _host(dtype, crow, col, vals, n, 1, 32)
        gl, w, nfail = _kernel(dev, crow, col, v, g_ptr, g_idx, n)
        assert nfail.tolist() == [0]
        assert _ratios((gl, w), ref[:2], g_ptr, g_idx, crow, col, v, n, dtype) <= C


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_pivot_tie(dev, dtype):
    """[[1, 5], [t, 1]] with |re t| + |im t| = 1 (t = -1, or 0.5 + 0.5i): a tie in the first column.  Either choice gives
    the same factors up to rounding, u = (-5, 1) / (1 - 5 t) and g = (-t, 1) / (1 - 5 t): the kernel must settle the tie
    (the lowest row) and land on them; the larger tie cases are in kernel_cases."""
    t = (0.5 + 0.5j) if dtype.is_complex else -1.0
    crow, col = np.array([0, 2, 4]), np.array([1, 0, 0, 1])
    vals = np.array([[5.0, 1.0, t, 1.0]])
    rows_t, col_t, v, g_ptr, g_idx, ref = _host(dtype, crow, col, vals, 2, 1, 32)
    gl, w, nfail = _kernel(dev, crow, col, v, g_ptr, g_idx, 2)
    assert nfail.tolist() == [0]
    den = 1 - 5 * t
    eps = torch.finfo(dtype).eps
    want_gl = np.array([1.0, -t, 1.0])
    want_w = np.conj(np.array([1.0, -5 / den, 1 / den]))
    assert np.abs(gl[0].numpy() - want_gl).max() <= 4 * eps
    assert np.abs(w[0].numpy() - want_w).max() <= 4 * eps
    assert _ratios((gl, w), ref[:2], g_ptr, g_idx, crow, col, v, 2, dtype) <= C


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", DTYPES)
def test_fallback_rows_and_counts(dev, dtype):
    crow, col, vals, counts = lc.fallback_case(dtype.is_complex)
    n = 12
    rows_t, col_t, v, g_ptr, g_idx, ref = _host(dtype, crow, col, vals, n, 1, 32)
    gl, w, nfail = _kernel(dev, crow, col, v, g_ptr, g_idx, n)
    assert nfail.tolist() == counts and ref[2].tolist() == counts
    assert bool(torch.isfinite(gl).all()) and bool(torch.isfinite(w).all())
    GL = lc.dense_of(g_ptr.numpy(), g_idx.numpy(), gl.numpy(), n)
    W = lc.dense_of(g_ptr.numpy(), g_idx.numpy(), w.numpy(), n)
    for b, i, scale in ((1, 3, 1.0), (1, 5, 1.0), (1, 6, 1.0), (2, 9, 1.0), (2, 11, 0.25)):
        assert GL[b][i, i] == 1 and W[b][i, i] == scale, (b, i)
        assert np.count_nonzero(GL[b][i]) == 1 and np.count_nonzero(W[b][i]) == 1
    assert GL[0][6, 5] != 0 and GL[2][6, 5] != 0                     # the same rows are served in the other members
    eps = torch.finfo(dtype).eps
    for o, r in zip((gl, w), ref[:2]):
        assert float((o.to(WIDE[dtype]) - r).abs().max()) <= C * 2 * eps * 4


@pytest.mark.gpu
def test_pattern_beyond_the_cap_is_refused_by_the_wrapper(dev):
    n = 40
    rows, cols = np.nonzero(np.tril(np.ones((n, n), dtype=bool)))
    crow = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(rows, minlength=n), out=crow[1:])
    ci = lambda a: torch.as_tensor(a).to(torch.int32).to(dev)
    vals = torch.ones((1, rows.size), dtype=torch.float64, device=dev)
    with pytest.raises(NativeLibraryError, match="cap"):
        K.fsai_lu_build(ci(crow), ci(cols), vals, ci(crow), ci(cols), n)
    g_ptr33 = crow[:34].copy()                                        # rows 0 .. 32: the longest has 33 entries
    with pytest.raises(NativeLibraryError, match="33 columns"):
        K.fsai_lu_build(ci(crow[:34]), ci(cols[:crow[33]]), vals[:, :crow[33]], ci(g_ptr33), ci(cols[:crow[33]]), 33)
