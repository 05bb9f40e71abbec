"""CPU: the float64 restatement of the Lanczos quadrature kernels (tests/slq_ref.py) against dense truth, and its QL
quadrature against numpy.linalg.eigh of the same Jacobi matrix.

Figures this file prints (relative error of z^T log(A) z, A = Q diag(geomspace(1, 100, n)) Q^T, Rademacher z, n = 48,
nsteps = 32): 5.5e-10 in float64 arithmetic, 1.6e-7 in float32 arithmetic (gates 1e-6 and 1e-5).  The a-priori Gauss
bound ~ 4 rho^(-2m), rho = (sqrt(kappa) + 1) / (sqrt(kappa) - 1) = 11 / 9, is 6e-6 at m = 32.  The QL quadrature reaches
0.164 of its bound (C_Q = 4; 0.66 with constant 1)."""
import math
import numpy as np
import pytest
import torch
from tests import slq_ref as sref


def _truth(Q, lam, z, f=np.log):
    return float(((z @ Q) ** 2 * f(lam)).sum())


@pytest.mark.parametrize("arith,gate", [(np.float64, 1e-6), (np.float32, 1e-5)], ids=["f64", "f32"])
def test_restated_iteration_against_dense_truth(arith, gate):
    rng = np.random.default_rng(0)
    n, nsteps = 48, 32
    A, Q, lam = sref.spd_matrix(rng, n)
    z = rng.choice([-1.0, 1.0], n)
    got, m, flag = sref.forms(A, z, nsteps, arith)
    ex = _truth(Q, lam, z)
    rel = abs(got - ex) / abs(ex)
    print("slq_ref %s: n = %d, nsteps = %d: relative error %.2e (gate %.0e)" % (arith.__name__, n, nsteps, rel, gate))
    assert flag == 0 and m == nsteps
    assert rel <= gate


@pytest.mark.parametrize("name", ["inv", "sqrt", "invsqrt", "exp", "identity"])
def test_restated_iteration_other_functions(name):
    rng = np.random.default_rng(1)
    n = 40
    A, Q, lam = sref.spd_matrix(rng, n, 1.0, 20.0)
    z = rng.standard_normal(n)
    t = -0.3
    got, m, flag = sref.forms(A, z, 30, np.float64, name, t)
    ex = _truth(Q, lam, z, sref.fn_of(name, t)[0])
    assert flag == 0 and abs(got - ex) <= 1e-6 * abs(ex)


def test_restated_breakdown_is_exact():
    """3 distinct eigenvalues: the Krylov space is exhausted after 3 steps, the quadrature over the 3 x 3 matrix exact"""
    rng = np.random.default_rng(2)
    n = 16
    lam = np.resize(np.array([1.0, 3.0, 7.0]), n)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    A = (Q * lam) @ Q.T
    z = rng.standard_normal(n)
    for arith in (np.float64, np.float32):
        got, m, flag = sref.forms(A, z, 8, arith)
        ex = _truth(Q, lam, z)
        assert m == 3 and flag == 0
        assert abs(got - ex) <= 64 * n * np.finfo(arith).eps * abs(ex)


def test_restated_zero_probe_and_indefinite():
    rng = np.random.default_rng(3)
    A, Q, lam = sref.spd_matrix(rng, 12)
    out, m, flag = sref.forms(A, np.zeros(12), 6)
    assert (out, m, flag) == (0.0, 0, 0)
    out, m, flag = sref.forms(A - 5.0 * np.eye(12), rng.standard_normal(12), 12)
    assert flag == 1 and math.isnan(out)
    out, m, flag = sref.forms(A - 5.0 * np.eye(12), rng.standard_normal(12), 12, name="exp", t=0.1)
    assert flag == 0 and math.isfinite(out)


@pytest.mark.parametrize("kappa", [1e2, 1e6], ids=["k1e2", "k1e6"])
@pytest.mark.parametrize("m", [1, 2, 3, 8, 16, 33, 64, 128])
def test_ql_quadrature_against_eigh(m, kappa):
    """the QL quadrature of the restatement against eigh of the same T, under the bound of slq_ref's docstring"""
    rng = np.random.default_rng(m)
    n = 4 * m
    A, Q, lam = sref.spd_matrix(rng, n, 1.0, kappa)
    z = rng.choice([-1.0, 1.0], n)
    zz = float(z @ z)
    v, vp, b = z / math.sqrt(zz), np.zeros(n), 0.0
    al, be = np.zeros(m), np.zeros(m)
    be[0] = math.sqrt(zz)
    for k in range(m):
        w = A @ v
        al[k] = v @ w
        w = w - al[k] * v - b * vp
        b = float(np.linalg.norm(w))
        if k + 1 < m:
            be[k + 1] = b
        vp, v = v, w / b
    worst = 0.0
    for name in sref.FN_CODES:
        t = -1.0 / kappa
        d, w, out, flag = sref.quad(al, be, m, zz, name, t)
        th, w2, ex, bound = sref.quad_truth(al, be, m, zz, name, t)
        assert flag == 0
        assert abs(out - ex) <= bound, (name, out, ex, bound)
        worst = max(worst, abs(out - ex) / bound)
        order = np.argsort(d)
        tn = np.abs(sref.jacobi(al, be, m)).sum(1).max()
        assert np.all(np.abs(d[order] - th) <= sref.C_Q * m * sref.EPS64 * tn)
        assert abs(w.sum() - 1.0) <= sref.C_Q * m * sref.EPS64
    print("ql quadrature m = %d kappa = %.0e: worst error / bound %.3f" % (m, kappa, worst))


def test_ql_decoupled_matrix():
    """some beta = 0: the blocks below the first zero carry no weight"""
    al = np.array([2.0, 3.0, 5.0, 7.0, 11.0])
    be = np.array([9.0, 0.5, 0.0, 0.25, 0.0])           # be[0] = |z| is not part of T
    d, w, out, flag = sref.quad(al, be, 5, 81.0, "log")
    th, w2, ex, bound = sref.quad_truth(al, be, 5, 81.0, "log")
    assert flag == 0 and abs(out - ex) <= bound
    assert np.count_nonzero(w) == 2


def test_step_restatement_freezes_and_counts():
    """one step of the restated kernel: a running system takes it, a small beta freezes, a frozen one is carried"""
    dtype, S, N, nblk = torch.float32, 3, 10, 1
    env = sref.Env(dtype, S, N, nblk)
    g = torch.Generator().manual_seed(0)
    W, r2, r1 = (torch.randn(S, N, dtype=torch.float64, generator=g) for _ in range(3))
    st = sref.rand_state(g, S, 0, frozen=(2,))
    Pa = torch.full((S, 64), math.nan, dtype=torch.float32)
    Pin = torch.full((S, 64), math.nan, dtype=torch.float32)
    Pa[:, 0] = 0.7
    Pin[:, 0] = torch.tensor([0.9, 1e-13, 0.9])
    ref = sref.step(env, W, r2, r1, Pa, Pin, st, 0, 8)
    assert ref["live"].tolist() == [True, False, False] and ref["broke"].tolist() == [False, True, False]
    so = ref["state"][0]
    assert so[:, sref.M].tolist() == [4.0, 3.0, 3.0] and so[:, sref.FLAG].tolist() == [0.0, 1.0, 1.0]
    assert torch.equal(ref["y"][0][1:], r1[1:])
    beta = math.sqrt(float(Pin[0, 0]))
    alpha = float(Pa[0, 0]) / beta ** 2
    want = W[0] / beta - alpha / beta * r2[0] - beta / st[0, 0, sref.BETA] * r1[0]
    assert torch.allclose(ref["y"][0][0], want, rtol=1e-14, atol=0)
