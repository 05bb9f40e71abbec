"""CPU: logdet / trace_fn / quadform on operators in host memory (linalg/host_slq.py) against dense truth.

`cases()` builds the problems once; tests/test_gpu_slq.py runs the same cases, with the same gates, on device
operators."""
import math
import warnings
import pytest
import torch
import xitorch_amd
from xitorch_amd import LinearOperator, MathWarning
from xitorch_amd.linalg import logdet, trace_fn, quadform, host_slq

DTYPES = [torch.float64, torch.complex128, torch.float32, torch.complex64]
IDS = ["f64", "c128", "f32", "c64"]
# logdet with orthogonal probes against slogdet: relative gates (float64: the iteration's own rounding at kappa = 100;
# single precision: eps32 * kappa with a margin of 10)
GATE = {torch.float64: 1e-10, torch.complex128: 1e-10, torch.float32: 1e-4, torch.complex64: 1e-4}


def hermitian(n, dtype, kappa=100.0, seed=3, evals=None):
    """(A in float64 / complex128 with eigenvalues geomspace(1, kappa, n) or `evals`, its eigenvectors Q, eigenvalues)"""
    g = torch.Generator().manual_seed(seed)
    hp = torch.complex128 if dtype.is_complex else torch.float64
    X = torch.randn(n, n, dtype=torch.float64, generator=g)
    if dtype.is_complex:
        X = torch.complex(X, torch.randn(n, n, dtype=torch.float64, generator=g))
    Q = torch.linalg.qr(X)[0]
    lam = torch.logspace(0, math.log10(kappa), n, dtype=torch.float64) if evals is None else evals
    A = (Q * lam.to(hp)) @ Q.conj().T
    return (A + A.conj().T) / 2, Q, lam


def orthogonal_probes(n, seed=11):
    """Z = sqrt(n) Q, p = n: Z Z^T = n I, so the Hutchinson mean is the exact trace"""
    g = torch.Generator().manual_seed(seed)
    return math.sqrt(n) * torch.linalg.qr(torch.randn(n, n, dtype=torch.float64, generator=g))[0]


def rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_logdet_orthogonal_probes(dtype):
    """Measured: 4.8e-11 (float64) and 8.9e-11 (complex128) against the gate 1e-10, on the host and on the kernels
    alike.  The error is that of the n-point Gauss rule of an un-reorthogonalised Lanczos run of n steps, not rounding
    noise: over 12 seeds of `hermitian` it stays within 2.2e-11 .. 4.6e-11 (float64) and 6.1e-11 .. 9.1e-11
    (complex128).  The margin at complex128 is thin (1.1 on this seed): another BLAS or torch version could tip it.
    The float32 / complex64 gates are met at the rounding of the float32 result itself."""
    n = 24
    A, _, _ = hermitian(n, dtype)
    op = LinearOperator.m(A.to(dtype), is_hermitian=True)
    tr = {}
    got = logdet(op, probes=orthogonal_probes(n).to(dtype), nsteps=n, trace=tr)
    truth = torch.linalg.slogdet(A)[1]
    print("host logdet %s: relative error %.2e (gate %.0e)" % (dtype, rel(got, truth), GATE[dtype]))
    assert got.shape == () and not got.is_complex()
    assert rel(got, truth) <= GATE[dtype]
    assert tr["host_reads"] == 1 and tr["napply"] == n
    assert tr["nsteps_used"].shape == (n,) and bool((tr["nsteps_used"] == n).all())


@pytest.mark.parametrize("dtype", DTYPES[:2], ids=IDS[:2])
def test_logdet_gradient(dtype):
    n = 24
    A, _, _ = hermitian(n, dtype)
    mat = A.clone().requires_grad_()
    op = LinearOperator.m(mat, is_hermitian=True)
    got = logdet(op, probes=orthogonal_probes(n).to(dtype), nsteps=n, bck_options={"rtol": 1e-10})
    g1, = torch.autograd.grad(got, mat)
    m2 = A.clone().requires_grad_()
    g2, = torch.autograd.grad(torch.linalg.slogdet(m2)[1], m2)
    err = float((g1 - g2).abs().max() / g2.abs().max())
    print("host logdet gradient %s: relative error %.2e (gate 1e-8 = rtol * kappa)" % (dtype, err))
    assert err <= 1e-8


def test_hutchinson_within_its_standard_error():
    """fixed seed, 64 Rademacher probes; measured: truth 110.52, estimate 111.81, stderr 1.72"""
    n = 48
    A, _, _ = hermitian(n, torch.float64, seed=5)
    op = LinearOperator.m(A, is_hermitian=True)
    tr = {}
    est = trace_fn(op, "log", probes=64, nsteps=24, seed=0, trace=tr)
    truth = torch.linalg.slogdet(A)[1]
    print("hutchinson: truth %.2f estimate %.2f stderr %.2f" % (float(truth), float(est), float(tr["stderr"])))
    assert tr["stderr"].shape == ()
    assert abs(float(est - truth)) <= 4 * float(tr["stderr"])
    assert float(tr["stderr"]) <= 0.05 * abs(float(truth))
    # logdet is trace_fn(A, "log"), and the gaussian probes obey the same law
    assert float(logdet(op, probes=64, nsteps=24, seed=0)) == float(est)
    trg = {}
    estg = trace_fn(op, "log", probes=64, nsteps=24, seed=0, dist="gaussian", trace=trg)
    assert float(estg) != float(est) and abs(float(estg - truth)) <= 4 * float(trg["stderr"])


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_breakdown_is_exact(dtype):
    n = 16
    lam = torch.tensor([1.0, 3.0, 7.0], dtype=torch.float64).repeat(6)[:n]
    A, Q, _ = hermitian(n, dtype, evals=lam)
    g = torch.Generator().manual_seed(1)
    Z = torch.randn(n, 4, dtype=torch.float64, generator=g)
    tr = {}
    q = quadform(LinearOperator.m(A.to(dtype), is_hermitian=True), Z.to(dtype), "log", nsteps=8, trace=tr)
    ex = ((Q.T @ Z) ** 2 * torch.log(lam)[:, None]).sum(0)
    assert tr["nsteps_used"].tolist() == [3, 3, 3, 3]
    assert rel(q, ex) <= 64 * n * torch.finfo(dtype).eps


def test_indefinite_member_is_nan_with_one_warning():
    n = 16
    A, _, _ = hermitian(n, torch.float64, kappa=10.0)
    Ab = torch.stack([A, A - 2.0 * torch.eye(n, dtype=torch.float64), 2 * A])
    op = LinearOperator.m(Ab, is_hermitian=True)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        est = trace_fn(op, "log", probes=8, nsteps=n, seed=2)
    mw = [x for x in w if issubclass(x.category, MathWarning)]
    assert len(mw) == 1 and "1 member" in str(mw[0].message)
    assert math.isnan(float(est[1])) and bool(torch.isfinite(est[[0, 2]]).all())
    alone = trace_fn(LinearOperator.m(Ab[[0, 2]], is_hermitian=True), "log", probes=8, nsteps=n, seed=2)
    assert torch.equal(est[[0, 2]], alone)                  # the other members are untouched
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert bool(torch.isfinite(trace_fn(op, "exp", probes=8, nsteps=n, t=-0.5)).all())


def test_callable_matches_named_and_functions_match_truth():
    n = 20
    A, Q, lam = hermitian(n, torch.float64, kappa=30.0)
    op = LinearOperator.m(A, is_hermitian=True)
    Z = orthogonal_probes(n)
    fns = {"log": torch.log, "inv": lambda x: 1 / x, "sqrt": torch.sqrt, "invsqrt": lambda x: x ** -0.5,
           "identity": lambda x: x}
    for name, f in fns.items():
        a = trace_fn(op, name, probes=Z, nsteps=n)
        b = trace_fn(op, f, probes=Z, nsteps=n)
        assert rel(a, b) <= 1e-13, name
        assert rel(a, f(lam).sum()) <= 1e-10, name
    a = trace_fn(op, "exp", probes=Z, nsteps=n, t=-0.2)
    assert rel(a, trace_fn(op, lambda x: torch.exp(-0.2 * x), probes=Z, nsteps=n)) <= 1e-13
    assert rel(a, torch.exp(-0.2 * lam).sum()) <= 1e-10


def test_batch_broadcasting_and_seeds():
    n = 12
    A, Q, lam = hermitian(n, torch.float64, kappa=10.0)
    Ab = torch.stack([A, 3 * A])                                            # (2, n, n)
    op = LinearOperator.m(Ab, is_hermitian=True)
    g = torch.Generator().manual_seed(4)
    Z = torch.randn(3, 1, n, 2, dtype=torch.float64, generator=g)           # (3, 1, n, 2) against (2, n, n)
    q = quadform(op, Z, "log", nsteps=n)
    assert q.shape == (3, 2, 2)
    for i in range(3):
        for b, s in enumerate((1.0, 3.0)):
            ex = ((Q.T @ Z[i, 0]) ** 2 * torch.log(s * lam)[:, None]).sum(0)
            assert rel(q[i, b], ex) <= 1e-10
    one = quadform(LinearOperator.m(A, is_hermitian=True), Z[0, 0], "log", nsteps=n)
    assert one.shape == (2,) and rel(one, q[0, 0]) <= 1e-13
    a, b, c = (trace_fn(op, "log", probes=5, nsteps=n, seed=s) for s in (7, 7, 8))
    assert a.shape == (2,) and torch.equal(a, b) and not torch.equal(a, c)
    assert torch.equal(host_slq.draw_probes(n, 5, torch.float64, 7), host_slq.draw_probes(n, 5, torch.float64, 7))
    zc = host_slq.draw_probes(n, 5, torch.complex64, 7)
    assert zc.dtype == torch.complex64 and bool((zc.imag == 0).all()) and bool((zc.real.abs() == 1).all())


def test_default_nsteps_and_single_probe():
    n = 60
    A, _, _ = hermitian(n, torch.float64, kappa=10.0)
    op = LinearOperator.m(A, is_hermitian=True)
    tr = {}
    trace_fn(op, "log", probes=1, trace=tr)
    assert tr["napply"] == 50 and math.isnan(float(tr["stderr"]))
    A8 = A[:8, :8]
    tr = {}
    trace_fn(LinearOperator.m(A8, is_hermitian=True), "log", probes=2, trace=tr)
    assert tr["napply"] == 8


def test_refusals():
    n = 8
    A, _, _ = hermitian(n, torch.float64, kappa=10.0)
    op = LinearOperator.m(A, is_hermitian=True)
    Z = torch.ones(n, 2, dtype=torch.float64)
    nonherm = LinearOperator.m(A + torch.triu(torch.ones(n, n, dtype=torch.float64), 1), is_hermitian=False)
    for call in (lambda **kw: quadform(kw.pop("A", op), Z, **kw), lambda **kw: trace_fn(kw.pop("A", op), "log", **kw),
                 lambda **kw: logdet(kw.pop("A", op), **kw)):
        with pytest.raises(RuntimeError, match="Hermitian"):
            call(A=nonherm)
        with pytest.raises(NotImplementedError):
            call(M=op)
        with pytest.raises(NotImplementedError):
            call(process_group=object())
        with pytest.raises(ValueError, match="128"):
            call(nsteps=129)
        with pytest.raises(ValueError):
            call(nsteps=0)
        with pytest.raises(TypeError):
            call(no_such_option=1)
    with pytest.raises(ValueError):
        trace_fn(op, "cosh")
    with pytest.raises(ValueError):
        trace_fn(op, "log", dist="uniform")
    with pytest.raises(ValueError):
        trace_fn(op, "log", probes=0)
    with pytest.raises(ValueError):
        trace_fn(op, "log", probes=torch.ones(n + 1, 2, dtype=torch.float64))
    with pytest.raises(TypeError):
        trace_fn(op, "log", t=2.0)
    with pytest.raises(RuntimeError):
        quadform(op, torch.ones(n + 1, 2, dtype=torch.float64))
    # only logdet is differentiable
    mat = A.clone().requires_grad_()
    opg = LinearOperator.m(mat, is_hermitian=True)
    with pytest.raises(NotImplementedError):
        trace_fn(opg, "log")
    with pytest.raises(NotImplementedError):
        quadform(opg, Z)
    with pytest.raises(NotImplementedError):
        quadform(op, Z.clone().requires_grad_())
    with torch.no_grad():
        assert bool(torch.isfinite(trace_fn(opg, "log", probes=4)))
    assert logdet(opg, probes=4).requires_grad
