"""CPU: tests/gkl_ref.py against plain numpy — the restatement of xk_gkl_sweep / xk_gkl_finish on random data, and the
one-sided-Jacobi model of xk_gkl_bsvd against numpy.linalg.svd on the matrices the GPU test uses."""
import numpy as np
import pytest
from tests import gkl_ref as gref

DTYPES = [np.float64, np.float32, np.complex128, np.complex64]


@pytest.mark.parametrize("dtype", DTYPES, ids=["f64", "f32", "c128", "c64"])
@pytest.mark.parametrize("N,j", [(1, 0), (7, 1), (257, 5), (1027, 63)])
def test_sweep_restatement_against_numpy(dtype, N, j):
    rng = np.random.default_rng(N + j)
    cplx = np.dtype(dtype).kind == "c"
    wide = np.complex128 if cplx else np.float64
    draw = lambda *s: (rng.standard_normal(s) + (1j * rng.standard_normal(s) if cplx else 0)).astype(dtype).astype(wide)
    Q, w, c = draw(j, N), draw(N), draw(j)
    dst, bound, part, pbound = gref.sweep(Q, w, c, 0.75, j, N, dtype)
    exact = 0.75 * (w - (c @ Q if j else 0))
    assert (np.abs(dst - exact) <= bound).all()
    assert dst.astype(dtype).astype(wide).tobytes() == dst.tobytes()             # representable in the storage type
    L = gref.chunk_elems(dtype)
    assert part.shape == ((2 * j if cplx else j) + 1, (N + L - 1) // L)
    coef, norm = gref.finish(part)
    dots = Q.conj() @ dst if j else np.zeros(0)
    got = coef[0::2] + 1j * coef[1::2] if cplx else coef
    assert np.allclose(got, dots, rtol=0, atol=1e-12 * max(1.0, np.abs(dots).max(initial=0)))
    assert abs(norm - np.linalg.norm(dst)) <= 1e-13 * max(norm, 1e-300)
    assert (pbound >= 0).all() and np.isfinite(pbound).all()


def test_sweep_null_coefficients_is_a_copy():
    rng = np.random.default_rng(0)
    Q, w = rng.standard_normal((3, 40)), rng.standard_normal(40)
    dst, _, part, _ = gref.sweep(Q, w, None, None, 3, 40, np.float64)
    assert np.array_equal(dst, w) and np.allclose(part[:3, 0], Q @ w) and np.isclose(part[3, 0], w @ w)


def test_cgs2_from_the_restatement_meets_the_orthogonality_constant():
    """three sweeps (accumulate, apply + accumulate, apply + norm) and the scaling store, as the driver chains them:
    the basis built this way stays orthonormal within ORTH_C u ncv — the constant the solver tests use"""
    for dtype in (np.float64, np.float32):
        rng = np.random.default_rng(3)
        N, ncv = 300, 40
        u = gref.unit_roundoff(dtype) * 2
        Q = np.zeros((ncv, N))
        for j in range(ncv):
            w = rng.standard_normal(N).astype(dtype).astype(np.float64)
            if j:
                w = w + 1e3 * Q[:j].T @ rng.standard_normal(j)                   # heavy cancellation in the first pass
                w = w.astype(dtype).astype(np.float64)
            w, _, part, _ = gref.sweep(Q, w, None, None, j, N, dtype)
            for _ in range(2):
                coef, _ = gref.finish(part)
                w, _, part, _ = gref.sweep(Q, w, coef, None, j, N, dtype)
            _, norm = gref.finish(part)
            Q[j], _, _, _ = gref.sweep(Q, w, None, 1.0 / norm, 0, N, dtype)
        assert np.abs(Q @ Q.T - np.eye(ncv)).max() <= gref.ORTH_C * u * ncv


CASES = gref.projected_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_jacobi_model_against_numpy(name):
    B = CASES[name]
    n = B.shape[0]
    assert n in (2, 3, 8, 17, 28, 64) and np.array_equal(B, np.triu(B))
    vals, sweeps = gref.jacobi_values(B)
    ref = np.linalg.svd(B, compute_uv=False)
    assert sweeps < 40
    assert (np.abs(vals - ref) <= gref.jacobi_bound(B, sweeps) + 4 * n * gref.U64 * ref.max(initial=0)).all()


def test_jacobi_model_graded_values_keep_relative_accuracy_where_B_is_scaled_by_columns():
    """graded 1 .. 1e-12: the absolute bound above is what the solver needs; the model also resolves the small values
    to a relative 1e-6 (one-sided Jacobi works on the columns, never on B^T B, whose small eigenvalues would be lost
    below 1e-16 sigma_max^2 = (1e-8 sigma_max)^2)"""
    B = CASES["graded17"]
    vals, _ = gref.jacobi_values(B)
    ref = np.linalg.svd(B, compute_uv=False)
    assert ref.min() < 1e-9 * ref.max()
    assert (np.abs(vals - ref) <= 1e-6 * ref).all()
    squared = np.sqrt(np.clip(np.linalg.eigvalsh(B.T @ B)[::-1], 0, None))
    assert np.abs(squared - ref).max() > gref.jacobi_bound(B, 40) or (np.abs(squared - ref) > 1e-6 * ref).any()


def test_jacobi_model_with_fused_arithmetic_ends_on_a_rank_deficient_matrix():
    """28 columns inside an 8-dimensional space (20 zero rows).  With fused multiply-adds a null column never cancels
    to exact zero: it stays rounding noise inside the span of the others, is never orthogonal to them relative to its
    own length, and a Jacobi that keeps rotating it does not end (it shrinks by about eps per sweep until its squared
    norm underflows).  The rule of the kernel — columns no longer than eps |B|_F are left alone — ends it."""
    B = CASES["rankdef28"]
    vals, sweeps = gref.jacobi_values(B, fused=True)
    ref = np.linalg.svd(B, compute_uv=False)
    assert sweeps < 20
    assert (np.abs(vals - ref) <= gref.jacobi_bound(B, sweeps) + 4 * 28 * gref.U64 * ref.max()).all()
