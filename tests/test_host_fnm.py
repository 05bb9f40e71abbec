"""CPU: funm_multiply / expm_multiply on operators in host memory (host_slq.funm) against dense eigh truth.

`operators`, `problem` and `check_against_restatement` build and judge the problems; tests/test_gpu_fnm.py runs the same
cases, with the same gates, on device operators.  The gate of a column is

    4 x (the error of tests/fnm_ref.funm on the same column in the same arithmetic) + 16 n eps_T

relative to the 2-norm of the truth: an implementation may round differently from the restatement, it may not converge
more slowly."""
import functools
import math
import warnings
import numpy as np
import pytest
import torch
from tests import fnm_ref as fref
from tests.test_host_slq import hermitian
from xitorch_amd import LinearOperator, MathWarning
from xitorch_amd.linop import SparseLinearOperator, BandedLinearOperator
from xitorch_amd.linalg import funm_multiply, expm_multiply, host_slq

DTYPES = [torch.float64, torch.complex128, torch.float32, torch.complex64]
IDS = ["f64", "c128", "f32", "c64"]
CPU = torch.device("cpu")
KINDS = [("dense", d) for d in DTYPES] + [("csr", torch.float64), ("csr", torch.complex64), ("banded", torch.float64),
                                         ("banded", torch.float32), ("user", torch.float64),
                                         ("user", torch.complex64)]
KIND_IDS = ["%s-%s" % (k, IDS[DTYPES.index(d)]) for k, d in KINDS]
SHAPES = [(40, 24), (24, 24)]
# name -> (fn argument, t, numpy function of the eigenvalues)
FUNCS = {"sqrt": ("sqrt", 1.0, np.sqrt), "invsqrt": ("invsqrt", 1.0, lambda x: 1 / np.sqrt(x)),
         "inv": ("inv", 1.0, lambda x: 1 / x), "log": ("log", 1.0, np.log), "exp": ("exp", -1.0, lambda x: np.exp(-x))}


class User(LinearOperator):
    """a user operator with .mm only"""

    def __init__(self, mat):
        super().__init__(shape=mat.shape, is_hermitian=True, dtype=mat.dtype, device=mat.device)
        self.mat = mat

    def _mv(self, x):                       # (abstract in LinearOperator, so it has to exist; it must never be called)
        raise AssertionError("the drivers apply a user operator through .mm only")

    def _mm(self, x):
        return torch.matmul(self.mat, x)

    def _getparamnames(self, prefix=""):
        return [prefix + "mat"]


def _banded_matrix(n, dtype, hb=2, seed=6):
    """symmetric pentadiagonal, eigenvalues within [2.4, 4.6] (Gershgorin): dense float64 matrix of the numbers the
    band holds in `dtype`, and the band (2 hb + 1, n)"""
    g = torch.Generator().manual_seed(seed)
    A = torch.zeros(n, n, dtype=torch.float64)
    for d in range(1, hb + 1):
        off = 0.3 * (torch.rand(n - d, dtype=torch.float64, generator=g) - 0.5)
        A += torch.diag(off, d) + torch.diag(off, -d)
    A += torch.diag(3.0 + torch.rand(n, dtype=torch.float64, generator=g))
    A = A.to(dtype).to(torch.float64)
    band = torch.zeros(2 * hb + 1, n, dtype=torch.float64)
    for d in range(2 * hb + 1):
        for i in range(n):
            j = i + d - hb
            if 0 <= j < n:
                band[d, i] = A[i, j]
    return A, band.to(dtype)


def operators(kind, dtype, n, dev=CPU, kappa=4.0):
    """(operator on `dev`, dense float64 / complex128 matrix of the numbers it holds)"""
    if kind == "banded":
        A, band = _banded_matrix(n, dtype)
        return BandedLinearOperator(band.to(dev), is_hermitian=True), A
    A, _, _ = hermitian(n, dtype, kappa=kappa)
    Ad = A.to(dtype)
    A = Ad.to(A.dtype)
    A = (A + A.conj().T) / 2
    if kind == "dense":
        op = LinearOperator.m(Ad.to(dev), is_hermitian=True)
    elif kind == "csr":
        crow = torch.arange(0, n * n + 1, n, dtype=torch.int64)
        cols = torch.arange(n, dtype=torch.int64).repeat(n)
        op = SparseLinearOperator(crow.to(dev), cols.to(dev), Ad.reshape(n * n).to(dev), (n, n), is_hermitian=True)
    else:
        op = User(Ad.to(dev))
    return op, A


def rhs(n, p, dtype, seed=21):
    g = torch.Generator().manual_seed(seed)
    B = torch.randn(n, p, dtype=torch.float64, generator=g)
    if dtype.is_complex:
        B = torch.complex(B, torch.randn(n, p, dtype=torch.float64, generator=g))
    return B.to(dtype)


@functools.lru_cache(maxsize=None)
def problem(kind, dtype, n, nsteps, p=3):
    """what host and device tests share, computed once: dense matrix A, B (n, p) in `dtype`, and per function the truth
    (n, p) and the restatement's relative error per column in the arithmetic of `dtype`"""
    _, A = operators(kind, dtype, n)
    B = rhs(n, p, dtype)
    An, Bn = A.numpy(), B.to(A.dtype).numpy()
    truth, referr = {}, {}
    for name, (_, _, f) in FUNCS.items():
        tr = np.stack([fref.dense_truth(An, Bn[:, j], f) for j in range(p)], -1)
        err = []
        for j in range(p):
            x, m, _ = fref.funm(An, Bn[:, j], nsteps, f, fref.ARITH[dtype])
            err.append(float(np.linalg.norm(x - tr[:, j]) / np.linalg.norm(tr[:, j])))
        truth[name], referr[name] = torch.from_numpy(tr), err
    return A, B, truth, referr


def colerr(X, truth):
    X = X.detach().cpu().to(truth.dtype)
    return (torch.linalg.norm(X - truth, dim=-2) / torch.linalg.norm(truth, dim=-2)).tolist()


def check_against_restatement(op, kind, dtype, n, nsteps, what):
    """every function of FUNCS on `op` against the truth under the gate of the module docstring; returns the results"""
    A, B, truth, referr = problem(kind, dtype, n, nsteps)
    eps = torch.finfo(dtype).eps
    out = {}
    for name, (fn, t, _) in FUNCS.items():
        tr = {}
        X = funm_multiply(op, B.to(op.device), fn, nsteps=nsteps, t=t, trace=tr)
        assert X.shape == (n, 3) and X.dtype == dtype and X.device.type == torch.device(op.device).type
        assert tr["nsteps"].tolist() == [nsteps] * 3 and tr["napply"] == 2 * nsteps - 1
        err = colerr(X, truth[name])
        gate = [4 * r + 16 * n * eps for r in referr[name]]
        print("%s %s n=%d nsteps=%d: error %s, restatement %s" % (what, name, n, nsteps,
              " ".join("%.2e" % e for e in err), " ".join("%.2e" % e for e in referr[name])))
        assert all(e <= g for e, g in zip(err, gate)), "%s %s: errors %r, gates %r" % (what, name, err, gate)
        out[name] = X
    return out


@pytest.mark.parametrize("n,nsteps", SHAPES)
@pytest.mark.parametrize("kind,dtype", KINDS, ids=KIND_IDS)
def test_against_truth(kind, dtype, n, nsteps):
    before = host_slq.calls["funm"]
    op, _ = operators(kind, dtype, n)
    check_against_restatement(op, kind, dtype, n, nsteps, "host %s %s" % (kind, dtype))
    assert host_slq.calls["funm"] == before + len(FUNCS)


def test_batch_broadcasting(dev=CPU):
    n = 12
    A, Q, lam = hermitian(n, torch.float64, kappa=4.0)
    op = LinearOperator.m(torch.stack([A, 3 * A]).to(dev), is_hermitian=True)          # (2, n, n)
    g = torch.Generator().manual_seed(4)
    B = torch.randn(3, 1, n, 2, dtype=torch.float64, generator=g)                      # (3, 1, n, 2)
    X = funm_multiply(op, B.to(dev), "sqrt", nsteps=n).cpu()
    assert X.shape == (3, 2, n, 2)
    for i in range(3):
        for b, s in enumerate((1.0, 3.0)):
            want = (Q * torch.sqrt(s * lam)) @ (Q.T @ B[i, 0])
            assert float((X[i, b] - want).norm() / want.norm()) <= 1e-12
    one = funm_multiply(LinearOperator.m(A.to(dev), is_hermitian=True), B[0, 0].to(dev), "sqrt", nsteps=n).cpu()
    assert one.shape == (n, 2) and float((one - X[0, 0]).norm() / one.norm()) <= 1e-13


def test_expm_multiply_both_signs(dev=CPU):
    n = 24
    A, Q, lam = hermitian(n, torch.float64, kappa=4.0)
    op = LinearOperator.m(A.to(dev), is_hermitian=True)
    B = rhs(n, 2, torch.float64)
    for t in (-0.7, 0.5):
        want = (Q * torch.exp(t * lam)) @ (Q.T @ B)
        X = expm_multiply(op, B.to(dev), t, nsteps=n).cpu()
        assert float((X - want).norm() / want.norm()) <= 16 * n * torch.finfo(torch.float64).eps * math.exp(4 * abs(t))
        same = funm_multiply(op, B.to(dev), "exp", t=t, nsteps=n).cpu()
        assert torch.equal(X, same)
    tr = {}
    expm_multiply(op, B.to(dev), trace=tr)
    assert tr["napply"] == 2 * n - 1                          # default nsteps = min(n, 50)


def test_complex_callable_against_eigh(dev=CPU):
    n, t = 24, 0.8
    A, Q, lam = hermitian(n, torch.complex128, kappa=4.0)
    op = LinearOperator.m(A.to(dev), is_hermitian=True)
    B = rhs(n, 2, torch.complex128)
    X = funm_multiply(op, B.to(dev), lambda x: torch.exp(-1j * t * x), nsteps=n).cpu()
    want = (Q * torch.exp(-1j * t * lam)) @ (Q.conj().T @ B)
    assert X.dtype == torch.complex128 and float((X - want).norm() / want.norm()) <= 16 * n * 2.0 ** -52
    assert abs(float(X.norm() / B.norm()) - 1) <= 1e-13       # unitary
    # a real callable equals the named function
    a = funm_multiply(op, B.to(dev), torch.sqrt, nsteps=n).cpu()
    b = funm_multiply(op, B.to(dev), "sqrt", nsteps=n).cpu()
    assert float((a - b).norm() / b.norm()) <= 1e-13
    # on a real operator a complex result is refused
    Ar, _, _ = hermitian(n, torch.float64, kappa=4.0)
    with pytest.raises(RuntimeError, match="cast A"):
        funm_multiply(LinearOperator.m(Ar.to(dev), is_hermitian=True), B.real.contiguous().to(dev),
                      lambda x: torch.exp(-1j * t * x), nsteps=n)
    with pytest.raises(RuntimeError, match="same shape"):
        funm_multiply(op, B.to(dev), lambda x: x.sum(), nsteps=n)


@pytest.mark.parametrize("dtype", DTYPES[:2], ids=IDS[:2])
def test_gradient_with_respect_to_B(dtype):
    n = 12
    A, _, _ = hermitian(n, dtype, kappa=4.0)
    op = LinearOperator.m(A, is_hermitian=True)
    B = rhs(n, 2, dtype).requires_grad_()
    assert torch.autograd.gradcheck(lambda b: funm_multiply(op, b, "invsqrt", nsteps=n), (B,))
    if dtype.is_complex:
        assert torch.autograd.gradcheck(lambda b: funm_multiply(op, b, lambda x: torch.exp(-0.5j * x), nsteps=n), (B,))
    # B broadcast over the operator's batch: the cotangent is summed back
    opb = LinearOperator.m(torch.stack([A, 2 * A]), is_hermitian=True)
    assert torch.autograd.gradcheck(lambda b: funm_multiply(opb, b, "sqrt", nsteps=n), (B,))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_breakdown_is_exact(dtype, dev=CPU):
    n = 16
    lam = torch.tensor([1.0, 3.0, 7.0], dtype=torch.float64).repeat(6)[:n]
    A, Q, _ = hermitian(n, dtype, evals=lam)
    B = rhs(n, 4, torch.float64)
    tr = {}
    with warnings.catch_warnings():
        warnings.simplefilter("error")                        # (and no rtol warning: a breakdown is exact)
        X = funm_multiply(LinearOperator.m(A.to(dtype).to(dev), is_hermitian=True), B.to(dtype).to(dev), "sqrt",
                          nsteps=8, rtol=1e-6, trace=tr).cpu()
    want = (Q * torch.sqrt(lam)) @ (Q.T @ B)
    # (the host driver sees the breakdown and stops: 4 + 2 applies; the device driver reads nothing and runs them all)
    assert tr["nsteps"].tolist() == [3, 3, 3, 3] and tr["napply"] == (15 if dev.type == "cuda" else 6)
    assert float((X.double() - want).norm() / want.norm()) <= 64 * n * torch.finfo(dtype).eps


def test_zero_column(dev=CPU):
    n = 24
    op, A = operators("dense", torch.float64, n, dev)
    B = rhs(n, 3, torch.float64)
    B[:, 1] = 0
    tr = {}
    X = funm_multiply(op, B.to(dev), "invsqrt", nsteps=n, trace=tr).cpu()
    assert tr["nsteps"].tolist() == [n, 0, n] and not bool(X[:, 1].any())
    lam, U = torch.linalg.eigh(A)
    want = (U * lam ** -0.5) @ (U.T @ B)
    assert float((X - want).norm() / want.norm()) <= 16 * n * 2.0 ** -52


def test_indefinite_member_is_nan_with_one_warning(dev=CPU):
    n = 16
    A, _, _ = hermitian(n, torch.float64, kappa=4.0)
    Ab = torch.stack([A, A - 2.0 * torch.eye(n, dtype=torch.float64), 2 * A])
    op = LinearOperator.m(Ab.to(dev), is_hermitian=True)
    B = rhs(n, 2, torch.float64).to(dev)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        X = funm_multiply(op, B, "sqrt", nsteps=n).cpu()
    mw = [x for x in w if issubclass(x.category, MathWarning)]
    assert len(mw) == 1 and "1 member" in str(mw[0].message)
    assert bool(torch.isnan(X[1]).all()) and bool(torch.isfinite(X[[0, 2]]).all())
    alone = funm_multiply(LinearOperator.m(Ab[[0, 2]].to(dev), is_hermitian=True), B, "sqrt", nsteps=n).cpu()
    assert torch.equal(X[[0, 2]], alone)                      # the other members are untouched
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert bool(torch.isfinite(expm_multiply(op, B, -0.5, nsteps=n)).all())


def test_rtol_warning(dev=CPU):
    n = 24
    A, _, _ = hermitian(n, torch.float64, kappa=100.0)
    op = LinearOperator.m(A.to(dev), is_hermitian=True)
    B = rhs(n, 3, torch.float64).to(dev)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        tr = {}
        funm_multiply(op, B, "inv", nsteps=4, rtol=1e-6, trace=tr)
    mw = [x for x in w if issubclass(x.category, MathWarning)]
    assert len(mw) == 1 and "3 column(s)" in str(mw[0].message)
    assert tr["tail"].shape == (3,) and bool((tr["tail"] > 1e-6).all())
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        funm_multiply(op, B, "inv", nsteps=n, rtol=1e-6)      # m = n: exact whatever the tail
        funm_multiply(op, B, "inv", nsteps=4)                 # not asked: no warning


def test_rtol_takes_any_positive_real():
    n = 8
    A, _, _ = hermitian(n, torch.float64, kappa=4.0)
    op = LinearOperator.m(A, is_hermitian=True)
    B = torch.ones(n, 2, dtype=torch.float64)
    want = funm_multiply(op, B, "sqrt", nsteps=4)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", MathWarning)
        for rtol in (1, 1e-3, np.float32(0.5), np.float64(1e-3), np.int64(2)):
            assert torch.equal(funm_multiply(op, B, "sqrt", nsteps=4, rtol=rtol), want)
    for rtol in (0, -1, 0.0, float("nan"), True, "1e-3", 1j, torch.tensor(1e-3)):
        with pytest.raises(ValueError, match="positive real"):
            funm_multiply(op, B, "sqrt", rtol=rtol)


def test_the_two_flag_bits_get_their_own_warning(monkeypatch):
    """bit 0 (a node <= 0) and bit 1 (the eigensolver of the small matrix did not converge) are told apart, also under
    a function that needs positivity: the drivers' flags are replaced here, since no input makes QL fail"""
    from xitorch_amd.linalg import fnm
    n = 8
    A, _, _ = hermitian(n, torch.float64, kappa=4.0)
    op = LinearOperator.m(torch.stack([A, A, A]), is_hermitian=True)
    B = torch.ones(n, 2, dtype=torch.float64)
    real = fnm._funm

    def flagged(bits):
        def f(A_, B_, opt):
            X, flag, m, tail, napply = real(A_, B_, opt)
            return X, torch.tensor(bits, dtype=torch.int64), m, tail, napply
        return f

    for bits, texts in (([[0, 0], [2, 0], [0, 0]], ["1 member(s) did not converge"]),
                        ([[1, 0], [0, 0], [1, 1]], ["2 member(s) are not numerically positive"]),
                        ([[1, 0], [0, 2], [0, 0]], ["1 member(s) are not numerically positive",
                                                    "1 member(s) did not converge"])):
        monkeypatch.setattr(fnm, "_funm", flagged(bits))
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            X = funm_multiply(op, B, "sqrt", nsteps=n)
        msgs = [str(x.message) for x in w if issubclass(x.category, MathWarning)]
        assert len(msgs) == len(texts) and all(t in m for t, m in zip(texts, msgs)), msgs
        for b in range(3):
            assert bool(torch.isnan(X[b]).all()) == any(bits[b])


def test_refusals():
    n = 8
    A, _, _ = hermitian(n, torch.float64, kappa=4.0)
    op = LinearOperator.m(A, is_hermitian=True)
    B = torch.ones(n, 2, dtype=torch.float64)
    nonherm = LinearOperator.m(A + torch.triu(torch.ones(n, n, dtype=torch.float64), 1), is_hermitian=False)
    for call in (lambda **kw: funm_multiply(kw.pop("A", op), B, "sqrt", **kw),
                 lambda **kw: expm_multiply(kw.pop("A", op), B, **kw)):
        with pytest.raises(RuntimeError, match="Hermitian"):
            call(A=nonherm)
        with pytest.raises(NotImplementedError, match="M="):
            call(M=op)
        with pytest.raises(NotImplementedError, match="process_group"):
            call(process_group=object())
        with pytest.raises(ValueError, match="128"):
            call(nsteps=129)
        with pytest.raises(ValueError):
            call(nsteps=0)
        with pytest.raises(ValueError):
            call(rtol=-1.0)
        with pytest.raises(TypeError):
            call(no_such_option=1)
        with pytest.raises(TypeError):
            call(trace=[])
    with pytest.raises(ValueError):
        funm_multiply(op, B, "cosh")
    with pytest.raises(TypeError):
        funm_multiply(op, B, "sqrt", t=2.0)
    with pytest.raises(RuntimeError):
        funm_multiply(op, torch.ones(n + 1, 2, dtype=torch.float64), "sqrt")
    # differentiable with respect to B only
    opg = LinearOperator.m(A.clone().requires_grad_(), is_hermitian=True)
    with pytest.raises(NotImplementedError, match="B only"):
        funm_multiply(opg, B, "sqrt")
    with torch.no_grad():
        assert bool(torch.isfinite(funm_multiply(opg, B, "sqrt")).all())
    assert funm_multiply(op, B.clone().requires_grad_(), "sqrt").requires_grad
