"""-m gpu: logdet / trace_fn / quadform on the HIP kernels (native_slq.py) — dense, CSR, banded and user operators.

The cases and gates are those of tests/test_host_slq.py, against the same dense truth; every device result is also
set beside the host result of the same call on the same probes (both are held to their gates against the truth: this is
no mutual comparison).  The host reads once per call, the operator is applied nsteps times, and a device operator never
reaches the host driver."""
import math
import warnings
import numpy as np
import pytest
import torch
from tests import fsai_cases as fc
from tests.test_host_slq import hermitian, orthogonal_probes, rel, GATE, DTYPES, IDS
from xitorch_amd import LinearOperator, MathWarning
from xitorch_amd.linop import SparseLinearOperator, BandedLinearOperator
from xitorch_amd.linalg import logdet, trace_fn, quadform, host_slq

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _csr(A, dtype):
    """CSR operator on the device from the dense host matrix A (n, n): full pattern"""
    n = A.shape[-1]
    crow = torch.arange(0, n * n + 1, n, dtype=torch.int64)
    cols = torch.arange(n, dtype=torch.int64).repeat(n)
    return SparseLinearOperator(crow.to(DEV), cols.to(DEV), A.reshape(n * n).to(dtype).to(DEV), (n, n),
                                is_hermitian=True)


def _banded(n, dtype, hb=2, seed=6):
    """symmetric positive definite pentadiagonal operator on the device (diagonally dominant) and its dense matrix"""
    g = torch.Generator().manual_seed(seed)
    A = torch.zeros(n, n, dtype=torch.float64)
    for d in range(1, hb + 1):
        off = 0.4 * torch.randn(n - d, dtype=torch.float64, generator=g)
        A += torch.diag(off, d) + torch.diag(off, -d)
    A += torch.diag(2.0 + 3.0 * torch.rand(n, dtype=torch.float64, generator=g))
    A = A.to(dtype).to(torch.float64)
    band = torch.zeros(2 * hb + 1, n, dtype=torch.float64)
    for d in range(2 * hb + 1):
        for i in range(n):
            j = i + d - hb
            if 0 <= j < n:
                band[d, i] = A[i, j]
    return BandedLinearOperator(band.to(dtype).to(DEV), is_hermitian=True), A


class _User(LinearOperator):
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


def _device_call(f, *args, **kw):
    """f(...) on a device operator: the host driver's counter must not move; returns (result on the host, trace)"""
    before = host_slq.calls["forms"]
    tr = {}
    out = f(*args, trace=tr, **kw)
    assert host_slq.calls["forms"] == before, "a device operator reached the host driver"
    assert out.device.type == "cuda"
    assert tr["host_reads"] == 1
    return out.cpu(), tr


KINDS = [("dense", d) for d in DTYPES] + [("csr", torch.float64), ("csr", torch.complex64), ("banded", torch.float64),
                                         ("banded", torch.float32), ("user", torch.float64),
                                         ("user", torch.complex64)]
KIND_IDS = ["%s-%s" % (k, IDS[DTYPES.index(d)]) for k, d in KINDS]


def _operators(kind, dtype, n):
    """(device operator, host operator of the same numbers, dense float64 / complex128 matrix)"""
    if kind == "banded":
        op, A = _banded(n, dtype)
        return op, LinearOperator.m(A.to(dtype), is_hermitian=True), A
    A, _, _ = hermitian(n, dtype)
    Ad = A.to(dtype)
    A = Ad.to(A.dtype)                                   # the truth is that of the numbers the operator holds
    A = (A + A.conj().T) / 2
    if kind == "dense":
        op = LinearOperator.m(Ad.to(DEV), is_hermitian=True)
    elif kind == "csr":
        op = _csr(Ad, dtype)
    else:
        op = _User(Ad.to(DEV))
    return op, LinearOperator.m(Ad, is_hermitian=True), A


@pytest.mark.parametrize("kind,dtype", KINDS, ids=KIND_IDS)
def test_logdet_orthogonal_probes(kind, dtype):
    """(the margins are those of tests/test_host_slq.py::test_logdet_orthogonal_probes: thin at complex128, and the
    single-precision cases are decided by the rounding of the float32 result, so they say little about the kernels --
    tests/test_gpu_slq_kernels.py carries that weight per entry)"""
    n = 24
    op, hop, A = _operators(kind, dtype, n)
    Z = orthogonal_probes(n).to(dtype)
    got, tr = _device_call(logdet, op, probes=Z.to(DEV), nsteps=n)
    truth = torch.linalg.slogdet(A)[1]
    host = logdet(hop, probes=Z, nsteps=n)
    print("logdet %s %s: kernels %.2e, host path %.2e (gate %.0e)" % (kind, dtype, rel(got, truth), rel(host, truth),
                                                                     GATE[dtype]))
    assert rel(got, truth) <= GATE[dtype]
    assert rel(host, truth) <= GATE[dtype]
    assert tr["napply"] == n and bool((tr["nsteps_used"] == n).all())


@pytest.mark.parametrize("dtype", DTYPES[:2], ids=IDS[:2])
def test_logdet_gradient_dense(dtype):
    n = 24
    A, _, _ = hermitian(n, dtype)
    mat = A.to(DEV).requires_grad_()
    got = logdet(LinearOperator.m(mat, is_hermitian=True), probes=orthogonal_probes(n).to(dtype).to(DEV), nsteps=n,
                 bck_options={"rtol": 1e-10})
    g1, = torch.autograd.grad(got, mat)
    m2 = A.clone().requires_grad_()
    g2, = torch.autograd.grad(torch.linalg.slogdet(m2)[1], m2)
    err = float((g1.cpu() - g2).abs().max() / g2.abs().max())
    print("logdet gradient %s: relative error %.2e (gate 1e-8 = rtol * kappa)" % (dtype, err))
    assert err <= 1e-8


def test_logdet_backward_csr_fsai():
    """the backward solve preconditioned by fsai on a CSR operator: d logdet / d values[k] = (A^-1)[col, row], exact for
    orthogonal probes up to the solve: rtol * kappa, kappa from the dense matrix"""
    m = 6
    N = m * m
    crow, col, vals = fc.grid_csr(m)
    dense = torch.as_tensor(fc.dense_of(crow, col, vals, N)[0])
    ev = torch.linalg.eigvalsh(dense)
    kappa = float(ev[-1] / ev[0])
    v = torch.as_tensor(vals[0]).to(DEV).requires_grad_()
    A = SparseLinearOperator(torch.as_tensor(crow).to(DEV), torch.as_tensor(col).to(DEV), v, (N, N), is_hermitian=True)
    Z = orthogonal_probes(N).to(DEV)
    rtol = 1e-10
    got = logdet(A, probes=Z, nsteps=N, bck_options={"precond": "fsai", "rtol": rtol})
    g, = torch.autograd.grad(got, v)
    rows = np.repeat(np.arange(N), np.diff(crow))
    want = torch.linalg.inv(dense)[torch.as_tensor(col), torch.as_tensor(rows)]
    err = float((g.cpu() - want).abs().max() / want.abs().max())
    print("logdet backward csr + fsai: kappa %.1e, relative error %.2e (gate %.1e)" % (kappa, err, rtol * kappa))
    assert err <= rtol * kappa


def test_hutchinson_within_its_standard_error():
    n = 48
    A, _, _ = hermitian(n, torch.float64, seed=5)
    est, tr = _device_call(trace_fn, LinearOperator.m(A.to(DEV), is_hermitian=True), "log", probes=64, nsteps=24, seed=0)
    trh = {}
    host = trace_fn(LinearOperator.m(A, is_hermitian=True), "log", probes=64, nsteps=24, seed=0, trace=trh)
    truth = torch.linalg.slogdet(A)[1]
    se = float(tr["stderr"])
    print("hutchinson: truth %.2f kernels %.2f (stderr %.2f) host path %.2f (stderr %.2f)"
          % (float(truth), float(est), se, float(host), float(trh["stderr"])))
    assert abs(float(est - truth)) <= 4 * se and se <= 0.05 * abs(float(truth))
    assert abs(float(host - truth)) <= 4 * float(trh["stderr"])
    assert tr["napply"] == 24 and tr["stderr"].device.type == "cuda"


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32], ids=["f64", "f32"])
def test_breakdown_is_exact(dtype):
    n = 16
    lam = torch.tensor([1.0, 3.0, 7.0], dtype=torch.float64).repeat(6)[:n]
    A, Q, _ = hermitian(n, dtype, evals=lam)
    g = torch.Generator().manual_seed(1)
    Z = torch.randn(n, 4, dtype=torch.float64, generator=g)
    q, tr = _device_call(quadform, LinearOperator.m(A.to(dtype).to(DEV), is_hermitian=True), Z.to(dtype).to(DEV), "log",
                         nsteps=8)
    ex = ((Q.T @ Z) ** 2 * torch.log(lam)[:, None]).sum(0)
    assert tr["nsteps_used"].tolist() == [3, 3, 3, 3] and tr["napply"] == 8
    assert rel(q, ex) <= 64 * n * torch.finfo(dtype).eps


def test_indefinite_member_is_nan_with_one_warning():
    n = 16
    A, _, _ = hermitian(n, torch.float64, kappa=10.0)
    Ab = torch.stack([A, A - 2.0 * torch.eye(n, dtype=torch.float64), 2 * A])
    op = LinearOperator.m(Ab.to(DEV), is_hermitian=True)
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        est, _ = _device_call(trace_fn, op, "log", probes=8, nsteps=n, seed=2)
    mw = [x for x in w if issubclass(x.category, MathWarning)]
    assert len(mw) == 1 and "1 member" in str(mw[0].message)
    assert math.isnan(float(est[1])) and bool(torch.isfinite(est[[0, 2]]).all())
    alone, _ = _device_call(trace_fn, LinearOperator.m(Ab[[0, 2]].to(DEV), is_hermitian=True), "log", probes=8,
                            nsteps=n, seed=2)
    assert torch.equal(est[[0, 2]], alone)                  # the other members are untouched
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ex, _ = _device_call(trace_fn, op, "exp", probes=8, nsteps=n, t=-0.5)
    assert bool(torch.isfinite(ex).all())


def test_callable_matches_named_and_functions_match_truth():
    n = 20
    A, Q, lam = hermitian(n, torch.float64, kappa=30.0)
    op = LinearOperator.m(A.to(DEV), is_hermitian=True)
    Z = orthogonal_probes(n).to(DEV)
    fns = {"log": torch.log, "inv": lambda x: 1 / x, "sqrt": torch.sqrt, "invsqrt": lambda x: x ** -0.5,
           "identity": lambda x: x, "exp": lambda x: torch.exp(-0.2 * x)}
    for name, f in fns.items():
        kw = {"t": -0.2} if name == "exp" else {}
        a, _ = _device_call(trace_fn, op, name, probes=Z, nsteps=n, **kw)
        b, _ = _device_call(trace_fn, op, f, probes=Z, nsteps=n)
        assert rel(a, b) <= 1e-13, name
        assert rel(a, f(lam).sum()) <= 1e-10, name


def test_batch_broadcasting_and_seeds():
    n = 12
    A, Q, lam = hermitian(n, torch.float64, kappa=10.0)
    op = LinearOperator.m(torch.stack([A, 3 * A]).to(DEV), is_hermitian=True)
    g = torch.Generator().manual_seed(4)
    Z = torch.randn(3, 1, n, 2, dtype=torch.float64, generator=g)
    q, tr = _device_call(quadform, op, Z.to(DEV), "log", nsteps=n)
    assert q.shape == (3, 2, 2) and tr["nsteps_used"].shape == (3, 2, 2)
    for i in range(3):
        for b, s in enumerate((1.0, 3.0)):
            ex = ((Q.T @ Z[i, 0]) ** 2 * torch.log(s * lam)[:, None]).sum(0)
            assert rel(q[i, b], ex) <= 1e-10
    a, b, c = (_device_call(trace_fn, op, "log", probes=5, nsteps=n, seed=s)[0] for s in (7, 7, 8))
    assert a.shape == (2,) and torch.equal(a, b) and not torch.equal(a, c)
    host = trace_fn(LinearOperator.m(torch.stack([A, 3 * A]), is_hermitian=True), "log", probes=5, nsteps=n, seed=7)
    assert rel(a, host) <= 1e-10                             # the same probes on the host and on the device


def test_default_nsteps_and_single_probe():
    n = 60
    A, _, _ = hermitian(n, torch.float64, kappa=10.0)
    _, tr = _device_call(trace_fn, LinearOperator.m(A.to(DEV), is_hermitian=True), "log", probes=1)
    assert tr["napply"] == 50 and math.isnan(float(tr["stderr"])) and tr["nsteps_used"].tolist() == [50]
    _, tr = _device_call(trace_fn, LinearOperator.m(A[:8, :8].to(DEV), is_hermitian=True), "log", probes=2)
    assert tr["napply"] == 8


def test_refusals_on_device_operators():
    n = 8
    A, _, _ = hermitian(n, torch.float64, kappa=10.0)
    op = LinearOperator.m(A.to(DEV), is_hermitian=True)
    with pytest.raises(NotImplementedError):
        trace_fn(op, "log", M=op)
    with pytest.raises(ValueError, match="128"):
        logdet(op, nsteps=129)
    opg = LinearOperator.m(A.to(DEV).requires_grad_(), is_hermitian=True)
    with pytest.raises(NotImplementedError):
        trace_fn(opg, "log")
