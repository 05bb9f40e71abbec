"""CPU: the Davidson kernel checker of tests/davidson_ref.py accepts a correct output rounded to the kernel dtype and
rejects plausible kernel bugs (tests/davidson_ref.py FAULTS) at shapes where they matter -- the evidence that
tests/test_gpu_davidson_kernels.py would fail on a subtly wrong kernel."""
import math
import pytest
import torch
from tests import davidson_ref as dref

DTYPES = [torch.float64, torch.float32]
IDS = ["f64", "f32"]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _r(t, dtype):
    """what the kernel reads: the value rounded to its dtype, seen in float64"""
    return t.to(dtype).to(torch.float64)


def _rand(g, dtype, *shape, scale=1.0):
    return _r(dref.rand(g, *shape, scale=scale), dtype)


def _expect_rejected(mut, ref, dtype, fault):
    with pytest.raises(AssertionError):
        dref.check(dref.values(mut, dtype), ref, dtype, what=fault)


def _expect_accepted(ref, dtype):
    assert dref.check(dref.values(ref, dtype), ref, dtype, what="accept") <= 1.0


def _basis(g, dtype, B, k, N):
    V = dref.rand(g, B, k, N)
    dref.add_sentinels(V, dtype, cols=dref.sentinel_columns(N, dtype))
    return _r(V, dtype)


def _coef(g, dtype, B, k, P):
    C = dref.rand(g, B, k, P)
    dref.add_sentinels(C, dtype, rows=[k - 1], cols=[P - 1])
    return _r(C, dtype)


def _orthonormal_rows(g, B, k, N):
    Q, _ = torch.linalg.qr(dref.rand(g, B, N, k))
    return Q.transpose(1, 2).contiguous()


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_checker_accepts_reference_rounded_to_kernel_dtype(dtype):
    g = _gen(1)
    vn = dref.VEC_ELEMS[dtype]
    B, k, P, N = 3, 13, 9, 5 * 256 * vn + 37
    V, AV = _basis(g, dtype, B, k, N), _basis(g, dtype, B, k, N)
    C, Out = _coef(g, dtype, B, k, P), _rand(g, dtype, B, P, N)
    _expect_accepted(dref.lincomb(V, C, Out, 1.0, 0.5, dtype), dtype)
    lam = _rand(g, dtype, B, P)
    _expect_accepted(dref.ritz_residual(V, AV, C, lam, dtype), dtype)
    d, m = _rand(g, dtype, 1, N), _r(1 + dref.rand(g, B, N).abs(), dtype)
    _expect_accepted(dref.diag_precond(Out, d, m, lam, dref.cast(1e-4, dtype), dtype), dtype)
    W = _rand(g, dtype, B, P, P)
    _expect_accepted(dref.panel_transform(Out, W, dtype), dtype)
    _expect_accepted(dref.extend_t(V, AV, 7, 5, dtype), dtype)
    Vo = _r(_orthonormal_rows(g, B, 12, N), dtype)
    ref = dref.orth(Vo, 7, 5, 2, dtype, cond=torch.zeros(B))
    assert bool((ref["_meta"]["kappa2"] <= dref.KAPPA2_MAX[dtype]).all())
    _expect_accepted(ref, dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("fault,k", [("drop_k8", 13), ("drop_k4", 13), ("drop_k4", 7), ("drop_k2", 9)])
def test_lincomb_rejects_a_dropped_k_remainder(dtype, fault, k):
    g = _gen(2)
    B, P, N = 3, 3, 1000
    V, C, Out = _basis(g, dtype, B, k, N), _coef(g, dtype, B, k, P), _rand(g, dtype, B, P, N)
    ref = dref.lincomb(V, C, Out, -1.0, 1.0, dtype)
    _expect_rejected(dref.lincomb(V, C, Out, -1.0, 1.0, dtype, fault=fault), ref, dtype, fault)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("fault,k", [("drop_k4", 13), ("drop_k4", 3), ("drop_k2", 7), ("drop_k2", 129)])
def test_ritz_residual_rejects_a_dropped_k_remainder(dtype, fault, k):
    g = _gen(3)
    B, P, N = 3, 3, 1000
    V, AV, Y = _basis(g, dtype, B, k, N), _basis(g, dtype, B, k, N), _coef(g, dtype, B, k, P)
    lam = _rand(g, dtype, B, P)
    ref = dref.ritz_residual(V, AV, Y, lam, dtype)
    _expect_rejected(dref.ritz_residual(V, AV, Y, lam, dtype, fault=fault), ref, dtype, fault)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("N", [1, 3, 5 * 1024 + 37, 100003])
def test_every_streaming_kernel_rejects_a_dropped_last_vector(dtype, N):
    g = _gen(4)
    B, k, P = 3, 9, 3
    V, AV, C = _basis(g, dtype, B, k, N), _basis(g, dtype, B, k, N), _coef(g, dtype, B, k, P)
    Out, lam = _rand(g, dtype, B, P, N), _rand(g, dtype, B, P)
    f = "drop_last_vec"
    _expect_rejected(dref.lincomb(V, C, Out, 1.0, 0.0, dtype, fault=f), dref.lincomb(V, C, Out, 1.0, 0.0, dtype),
                     dtype, f)
    _expect_rejected(dref.ritz_residual(V, AV, C, lam, dtype, fault=f), dref.ritz_residual(V, AV, C, lam, dtype),
                     dtype, f)
    W = _rand(g, dtype, B, P, P)
    _expect_rejected(dref.panel_transform(Out, W, dtype, fault=f), dref.panel_transform(Out, W, dtype), dtype, f)
    _expect_rejected(dref.extend_t(V, AV, 6, 3, dtype, fault=f), dref.extend_t(V, AV, 6, 3, dtype), dtype, f)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("P", [9, 16, 17])
def test_rejects_a_wrong_column_chunk_offset(dtype, P):
    g = _gen(5)
    B, k, N = 3, 8, 1000
    V, AV, C = _basis(g, dtype, B, k, N), _basis(g, dtype, B, k, N), _coef(g, dtype, B, k, P)
    Out, lam = _rand(g, dtype, B, P, N), _rand(g, dtype, B, P)
    for f in ("chunk_coef", "chunk_out"):
        _expect_rejected(dref.lincomb(V, C, Out, 1.0, 1.0, dtype, fault=f), dref.lincomb(V, C, Out, 1.0, 1.0, dtype),
                         dtype, f)
    ref = dref.ritz_residual(V, AV, C, lam, dtype)
    for f in ("chunk_coef", "chunk_lam", "chunk_out"):
        _expect_rejected(dref.ritz_residual(V, AV, C, lam, dtype, fault=f), ref, dtype, f)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_lincomb_rejects_swapped_layout_and_ignored_beta(dtype):
    g = _gen(6)
    B, k, N = 3, 8, 1000
    V, C, Out = _basis(g, dtype, B, k, N), _rand(g, dtype, B, k, k), _rand(g, dtype, B, k, N)
    ref = dref.lincomb(V, C, Out, 1.0, 0.5, dtype)
    _expect_rejected(dref.lincomb(V, C, Out, 1.0, 0.5, dtype, fault="swap_layout"), ref, dtype, "swap_layout")
    _expect_rejected(dref.lincomb(V, C, Out, 1.0, 0.5, dtype, fault="beta_ignored"), ref, dtype, "beta_ignored")


def test_lincomb_with_beta_zero_ignores_nan_in_out():
    g = _gen(7)
    V, C = _basis(g, torch.float64, 2, 3, 10), _rand(g, torch.float64, 2, 3, 2)
    Out = torch.full((2, 2, 10), math.nan, dtype=torch.float64)
    val, bnd = dref.lincomb(V, C, Out, 1.0, 0.0, torch.float64)["Out"]
    assert bool(torch.isfinite(val).all()) and bool(torch.isfinite(bnd).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("P", [2, 9])
def test_panel_transform_rejects_a_lower_triangle_read(dtype, P):
    g = _gen(8)
    Tp, W = _rand(g, dtype, 3, P, 700), _rand(g, dtype, 3, P, P)
    _expect_rejected(dref.panel_transform(Tp, W, dtype, fault="w_lower"), dref.panel_transform(Tp, W, dtype), dtype,
                     "w_lower")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("k0,q", [(1, 3), (7, 3), (40, 9)])
def test_extend_t_rejects_missing_or_misplaced_mirror_and_dropped_row(dtype, k0, q):
    g = _gen(9)
    N = 3001
    V, AV = _basis(g, dtype, 3, k0 + q, N), _basis(g, dtype, 3, k0 + q, N)
    ref = dref.extend_t(V, AV, k0, q, dtype)
    for f in ("no_mirror", "mirror_off", "drop_last_row"):
        _expect_rejected(dref.extend_t(V, AV, k0, q, dtype, fault=f), ref, dtype, f)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("bad", [math.nan, math.inf])
def test_ritz_residual_requires_nonfinite_residual_as_inf(dtype, bad):
    """a NaN (or inf) in one AV entry of one member: rmax of that member must be +inf, the others stay finite; the
    old kernel's rmax (NaN entries dropped) is rejected for NaN"""
    g = _gen(10)
    B, k, P, N = 3, 5, 9, 1000
    V, AV, Y, lam = (_basis(g, dtype, B, k, N), _basis(g, dtype, B, k, N), _rand(g, dtype, B, k, P),
                     _rand(g, dtype, B, P))
    AV[1, 2, 17] = bad
    ref = dref.ritz_residual(V, AV, Y, lam, dtype)
    assert ref["rmax"][0][1].item() == math.inf and bool(torch.isfinite(ref["rmax"][0][[0, 2]]).all())
    _expect_accepted(ref, dtype)
    mut = dref.ritz_residual(V, AV, Y, lam, dtype, fault="nan_dropped")
    if math.isnan(bad):
        _expect_rejected(mut, ref, dtype, "nan_dropped")
        assert dref.status_of(mut["rmax"][0], torch.zeros(B, dtype=torch.int32))[0] < math.inf
    assert dref.status_of(ref["rmax"][0], torch.zeros(B, dtype=torch.int32))[0] == math.inf


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_diag_precond_floor_rule_and_rejected_faults(dtype):
    g = _gen(11)
    B, P, N = 3, 3, 600
    floor = dref.cast(1e-3, dtype)
    Tn, lam = _rand(g, dtype, B, P, N), _rand(g, dtype, B, P)
    dbuf = _rand(g, dtype, B, N)
    d = dbuf[:1]
    # exact zeros and tiny denominators of both signs in member 0, column 0 (d - lam exact by Sterbenz)
    lam0 = lam[0, 0].item()
    d[0, :4] = torch.tensor([lam0, lam0 + 1e-4 * abs(lam0), lam0 - 1e-4 * abs(lam0), lam0], dtype=torch.float64)
    d[0] = _r(d[0], dtype)
    d[0, 5] = math.nan
    ref = dref.diag_precond(Tn, d, None, lam, floor, dtype)
    val = ref["Tn"][0]
    den = d[0, :4] - lam0
    assert bool((den[[0, 3]] == 0).all()) and float(den[1]) > 0 > float(den[2])
    assert val[0, 0, 0].item() == pytest.approx(Tn[0, 0, 0].item() / floor, rel=1e-12)
    assert val[0, 0, 2].item() == pytest.approx(-Tn[0, 0, 2].item() / floor, rel=1e-12)
    assert bool(torch.isnan(val[:, :, 5]).all())
    _expect_accepted(ref, dtype)
    _expect_rejected(dref.diag_precond(Tn, d, None, lam, floor, dtype, fault="floor_sign"), ref, dtype, "floor_sign")
    _expect_rejected(dref.diag_precond(Tn, d, None, lam, floor, dtype, fault="d_stride", d_wrong=dbuf), ref, dtype,
                     "d_stride")


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_orth_cond_rejects_missing_shift_and_wrong_round(dtype):
    """passes = 2, q <= 8: cond is the squared pivot ratio of the SHIFTED first CholeskyQR; an unshifted one, or the
    ratio of the second round (~1), moves it by many bounds"""
    g = _gen(12)
    B, k0, q, N = 3, 5, 4, 1000
    V = _orthonormal_rows(g, B, k0 + q, N)
    V[:, k0:] *= torch.tensor([1.0, 3.0, 0.3, 10.0], dtype=torch.float64).view(1, q, 1)   # kappa ~ 30
    V = _r(V, dtype)
    cond0 = torch.zeros(B, dtype=torch.float64)
    ref = dref.orth(V, k0, q, 2, dtype, cond=cond0)
    _expect_accepted(ref, dtype)
    for f in ("no_shift", "cond_round"):
        mut = dref.orth(V, k0, q, 2, dtype, cond=cond0, fault=f)
        with pytest.raises(AssertionError):
            dref.check({"cond": mut["cond"][0]}, {"cond": ref["cond"]}, dtype, what=f)


def test_orth_rejects_a_missing_second_projection():
    """a new block nearly inside span(V): in float32 arithmetic the first projection leaves ~u / 1e-5 of V in it after
    CholeskyQR; the second projection removes that, without it the orthogonality property fails"""
    dtype = torch.float32
    g = _gen(13)
    B, k0, q, N = 2, 8, 3, 2000
    V = _orthonormal_rows(g, B, k0 + q, N)
    V[:, k0:] = torch.einsum("bca,ban->bcn", dref.rand(g, B, q, k0), V[:, :k0]) + 1e-5 * V[:, k0:]
    V = _r(V, dtype)
    tol = dref.orth_tolerance(dtype, N, k0, q)
    good = dref.orth(V, k0, q, 2, dtype, work=dtype)
    po, pq = dref.orth_properties(V, good["Q"][0], k0, dtype)
    assert bool((po <= tol).all()) and bool((pq <= tol).all()), (po, pq, tol)
    bad = dref.orth(V, k0, q, 2, dtype, work=dtype, fault="no_second_projection")
    po, _ = dref.orth_properties(V, bad["Q"][0], k0, dtype)
    assert bool((po > tol).all()), (po, tol)


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
@pytest.mark.parametrize("q", [3, 9, 40])
def test_orth_info_reports_the_first_zero_row(dtype, q):
    g = _gen(14)
    B, k0, N = 3, 4, 300
    V = _r(_orthonormal_rows(g, B, k0 + q, N), dtype)
    V[1, k0 + 2] = 0
    for passes in (0, 1):
        ref = dref.orth(V, k0, q, passes, dtype)
        assert ref["info"][0].tolist() == [0.0, 3.0, 0.0]
    info = torch.tensor([5, 0, 0])
    assert dref.orth(V, k0, q, 1, dtype, info=info)["info"][0].tolist() == [5.0, 3.0, 0.0]
