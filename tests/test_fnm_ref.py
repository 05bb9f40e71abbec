"""CPU: the restatement of two-pass Lanczos f(A) b (tests/fnm_ref.py) against dense truth, and its plain-Python QL with
accumulated vectors against numpy.linalg.eigh.  The figures measured here are the yardstick of the host and device tests
(their gates are multiples of the restatement's own error on the same input).

Inputs: A = Q diag(geomspace(1, kappa, n)) Q^H, Gaussian b, 4 seeds, real and complex, vector arithmetic in double and
in single precision.  Relative 2-norm errors, worst over sqrt, invsqrt, inv, log, exp(-x) and the seeds:

    kappa   n    nsteps   float64 arithmetic   float32 arithmetic
    4       40   24       <= 1e-12             <= 3e-7         (polynomial approximation error of degree 23)
    4       257  30       <= 8e-15             <= 4e-7
    4       24   24       <= 4e-15             <= 3e-7         (m = n: exact up to rounding)
    100     48   32       sqrt 4e-7, inv 2e-4  (the same: the approximation error dominates)

The gates are twice these figures: they were measured on other seeds."""
import math
import numpy as np
import pytest
from tests import slq_ref as sref
from tests import fnm_ref as fref
from tests.test_gpu_slq_kernels import _lanczos_T

FNS = {"sqrt": np.sqrt, "invsqrt": lambda x: 1 / np.sqrt(x), "inv": lambda x: 1 / x, "log": np.log,
       "expm": lambda x: np.exp(-x)}
SEEDS = 4
TABLE = [(4.0, 40, 24, 1e-12, 3e-7), (4.0, 257, 30, 8e-15, 4e-7), (4.0, 24, 24, 4e-15, 3e-7)]


def _rel(x, want):
    return float(np.linalg.norm(x - want) / np.linalg.norm(want))


def _worst(kappa, n, nsteps, cplx, single, names):
    arith = {(False, False): np.float64, (False, True): np.float32, (True, False): np.complex128,
             (True, True): np.complex64}[(cplx, single)]
    worst = {}
    for seed in range(SEEDS):
        rng = np.random.default_rng(100 * n + seed)
        A = fref.hpd_matrix(rng, n, kappa, cplx)
        b = rng.standard_normal(n) + (1j * rng.standard_normal(n) if cplx else 0)
        for name in names:
            x, m, _ = fref.funm(A, b, nsteps, FNS[name], arith)
            assert m == nsteps
            worst[name] = max(worst.get(name, 0.0), _rel(x, fref.dense_truth(A, b, FNS[name])))
    return worst


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
@pytest.mark.parametrize("kappa,n,nsteps,tol64,tol32", TABLE)
def test_table_kappa_4(kappa, n, nsteps, tol64, tol32, cplx):
    for single, tol in ((False, tol64), (True, tol32)):
        w = _worst(kappa, n, nsteps, cplx, single, list(FNS))
        print("kappa %g n %d nsteps %d %s %s: %s" % (kappa, n, nsteps, "complex" if cplx else "real",
                                                      "fp32" if single else "fp64",
                                                      ", ".join("%s %.2e" % kv for kv in sorted(w.items()))))
        assert max(w.values()) <= 2 * tol, w


@pytest.mark.parametrize("cplx", [False, True], ids=["real", "complex"])
def test_kappa_100_converges_like_the_polynomial(cplx):
    for single in (False, True):
        w = _worst(100.0, 48, 32, cplx, single, ["sqrt", "inv"])
        print("kappa 100 n 48 nsteps 32 %s %s: sqrt %.2e inv %.2e" % ("complex" if cplx else "real",
                                                                        "fp32" if single else "fp64", w["sqrt"], w["inv"]))
        if not single:
            assert w["sqrt"] <= 2 * 4e-7 and w["inv"] <= 2 * 2e-4
        else:
            # single precision loses orthogonality earlier, which delays convergence (measured: sqrt 1.4e-6, inv 4.4e-4);
            # the figure is reported, the assertion is only that the iteration still converges
            assert w["sqrt"] <= 1e-4 and w["inv"] <= 1e-2
        assert w["inv"] > 1e-6                         # far from the squared rate of the quadrature


def test_replay_is_bit_identical():
    rng = np.random.default_rng(5)
    for arith in (np.float64, np.float32, np.complex128, np.complex64):
        cplx = np.iscomplexobj(np.zeros(1, arith))
        A = fref.hpd_matrix(rng, 40, 100.0, cplx)
        b = rng.standard_normal(40) + (1j * rng.standard_normal(40) if cplx else 0)
        al, be, m, zz, v1 = fref.lanczos(A, b, 30, arith)
        _, v2 = fref.replay(A, b, al, be, m, np.ones(m), arith)
        assert m == 30 and len(v1) == len(v2) == m
        for x, y in zip(v1, v2):
            assert x.tobytes() == y.tobytes()


def test_breakdown_and_zero():
    rng = np.random.default_rng(6)
    A = fref.hpd_matrix(rng, 30, 4.0)
    lam, U = np.linalg.eigh(A)
    b = U[:, [2, 11, 17]] @ np.array([1.0, -2.0, 0.5])
    x, m, _ = fref.funm(A, b, 12, np.sqrt)
    assert m == 3 and _rel(x, fref.dense_truth(A, b, np.sqrt)) <= 64 * 30 * fref.EPS64
    x, m, _ = fref.funm(A, np.zeros(30), 12, np.sqrt)
    assert m == 0 and not x.any()


WORST_QL = {}


@pytest.mark.parametrize("m", [1, 2, 3, 17, 64, 128])
def test_ql_vectors_against_eigh(m):
    """the Python QL with accumulated vectors under the bound of xk_fnm_coeff with a margin of at least 4: this is what
    fixes C_K.  Also Q orthonormal to 64 m EPS64 and the decomposition itself."""
    worst = 0.0
    for kappa in (1e2, 1e6):
        rng = np.random.default_rng(m * 100 + int(math.log10(kappa)))
        al, be, zz = _lanczos_T(rng, m, kappa)
        th, Z, ok = fref.ql_vectors(al[:m], be[1:m])
        assert ok
        T = sref.jacobi(al, be, m)
        tn = np.abs(T).sum(1).max()
        assert np.abs(Z.T @ Z - np.eye(m)).max() <= fref.C_QORTH * m * fref.EPS64
        assert np.abs((Z * th) @ Z.T - T).max() <= fref.C_QORTH * m * fref.EPS64 * tn
        for name in sref.FN_CODES:
            t = -0.01
            _, _, c, tail, flag = fref.coeff(al, be, m, zz, name, t)
            want, bound = fref.coeff_truth(al, be, m, zz, name, t)
            assert flag == 0
            err = float(np.linalg.norm(c - want))
            assert err * 4 <= bound, "m=%d kappa=%g %s: error %.3e, bound %.3e" % (m, kappa, name, err, bound)
            worst = max(worst, err / bound)
            assert abs(tail - fref.tail_of(want)) <= 2 * bound / np.linalg.norm(want)
    WORST_QL[m] = worst
    print("ql_vectors m = %d: worst error / bound %.3f (C_K = %g)" % (m, worst, fref.C_K))


WORST_CASES = {}


@pytest.mark.parametrize("S", [1, 70])
@pytest.mark.parametrize("nsteps", [1, 2, 3, 17, 64, 128])
def test_ql_vectors_on_the_kernel_test_inputs(nsteps, S):
    """the Python QL on the very inputs tests/test_gpu_fnm_kernels.py feeds xk_fnm_eig / xk_fnm_coeff (mixed m_s, a
    decoupled matrix, an indefinite one, b = 0), every named function: the margin under the bound must be >= 4"""
    Tal, Tbe, state, k, ms, zzs = fref.eig_cases(_lanczos_T, nsteps, S)
    worst = 0.0
    for s in range(S):                                            # every system of the kernel test
        m = ms[s]
        if m == 0:
            continue
        eig = fref.ql_vectors(Tal[s][:m], Tbe[s][1:m])           # once per system, for every function
        for name in sref.FN_CODES:
            _, _, c, _, flag = fref.coeff(Tal[s], Tbe[s], m, zzs[s], name, -0.01, eig=eig)
            if s == fref.INDEFINITE and name in sref.NEEDS_POSITIVE:
                assert flag == 1
                continue
            want, bound = fref.coeff_truth(Tal[s], Tbe[s], m, zzs[s], name, -0.01)
            err = float(np.linalg.norm(c - want))
            assert flag == 0 and err * 4 <= bound, "nsteps=%d s=%d m=%d %s: %.3e vs %.3e" % (nsteps, s, m, name, err,
                                                                                             bound)
            if bound > 0:
                worst = max(worst, err / bound)
    WORST_CASES[(nsteps, S)] = worst
    print("ql_vectors on the kernel test inputs nsteps = %d S = %d: worst error / bound %.3f (C_K = %g)"
          % (nsteps, S, worst, fref.C_K))


def test_indefinite_is_flagged():
    rng = np.random.default_rng(8)
    al, be, zz = _lanczos_T(rng, 8, 1e2)
    al = al - (np.linalg.eigvalsh(sref.jacobi(al, be, 8)).min() + 0.5)
    _, _, c, tail, flag = fref.coeff(al, be, 8, zz, "sqrt")
    assert flag == 1 and np.isnan(c).all()
    _, _, c, _, flag = fref.coeff(al, be, 8, zz, "exp", -0.1)
    assert flag == 0 and np.isfinite(c).all()


def test_worst_ratio_report():
    """(runs last in this file)"""
    for m, w in sorted(WORST_QL.items()):
        print("ql_vectors: worst error / bound at m = %d: %.3f" % (m, w))
