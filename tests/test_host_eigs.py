"""CPU: eigs on operators in host memory (host_eig.arnoldi, the torch-op statement of native_arnoldi.arnoldi) against
closed forms and numpy.linalg.eig: the solver cases of tests/test_gpu_eigs.py, every refusal, the output order, the dense
hand-over, an invariant-subspace start, batches, and the dispatch rule (a device operator never reaches the host twin).

Restart cycles on the host path (min_eps = 1e-8 for the 64-bit, 1e-4 for the 32-bit types), the figures the GPU file's
choice of spectra rests on: normal operators n = 200, neig = 4, ncv = 20: 1 to 4 cycles by dtype; Toeplitz n = 64,
ncv = 32: bc < 0 (LM) 7, bc > 0 (LR) 5 — all below a quarter of max_niter = 100.  (At ncv = 20 the Toeplitz cases
need 16 and 12 cycles; with bc < 0 every eigenvalue has the same real part, so "LR" does not separate them.)"""
import warnings
import numpy as np
import pytest
import torch
from tests import arn_cases as ac
from xitorch_amd import LinearOperator
from xitorch_amd._capi import NativeLibraryError
from xitorch_amd._util import ConvergenceWarning
from xitorch_amd.linalg import eigs, symeig, host_eig

pytestmark = pytest.mark.filterwarnings("error::xitorch_amd._util.ConvergenceWarning")
DTYPES = [torch.float64, torch.float32, torch.complex128, torch.complex64]
IDS = ["f64", "f32", "c128", "c64"]


def _eps(dtype):
    return 1e-8 if dtype in (torch.float64, torch.complex128) else 1e-4


def _ueps(dtype):
    return float(torch.finfo(dtype).eps)


def _pairs_ok(A, lam, X, min_eps):
    """A (n, n) complex128 numpy; the true residuals in complex128 and the unit norms"""
    lam, X = lam.to(torch.complex128).numpy(), X.to(torch.complex128).numpy()
    r = np.linalg.norm(A @ X - X * lam, axis=0)
    assert np.all(r <= 2 * min_eps * np.abs(lam)), (r, lam)
    assert np.allclose(np.linalg.norm(X, axis=0), 1.0, atol=1e-5)
    return r


@pytest.mark.parametrize("dtype", DTYPES, ids=IDS)
def test_normal_operator(dtype):
    n, neig = 200, 4
    A, ev = ac.normal_matrix(n, neig, dtype.is_complex)
    At = torch.from_numpy(A).to(dtype)
    trace = {}
    lam, X = eigs(LinearOperator.m(At), neig, "LM", min_eps=_eps(dtype), trace=trace)
    assert trace["converged"] and trace["niter"] <= 25 and trace["panel_kernel"] == "host"
    assert lam.dtype == X.dtype == (torch.complex128 if dtype in (torch.float64, torch.complex128) else torch.complex64)
    A128 = At.to(torch.complex128).numpy()
    r = _pairs_ok(A128, lam, X, _eps(dtype))
    want = ev[np.argsort(-np.abs(ev), kind="stable")][:neig]
    got = lam.to(torch.complex128).numpy()
    # normal matrix: |theta - lambda| <= residual (Bauer-Fike with condition 1) + the rounding of A itself
    for i in range(neig):
        assert np.abs(want - got[i]).min() <= r[i] + 16 * n * _ueps(dtype) * 2.0
    if not dtype.is_complex:                          # pairs adjacent, positive imaginary part first, best first
        assert got[0].imag > 0 and abs(got[1] - np.conj(got[0])) <= 1e-3 and got[2].imag > 0
        assert abs(got[0]) >= abs(got[2]) - 1e-3


@pytest.mark.parametrize("which", ["LM", "LR", "SR", "LI", "SI"])
def test_which_orders_best_first(which):
    n, neig = 120, 3
    rng = np.random.default_rng(5)
    ev = np.concatenate([[2.0 + 0.2j, -2.1 + 0.1j, 0.3 + 2.2j, 0.2 - 2.3j, 1.8 - 0.3j, -1.9 - 0.2j, 0.1 + 1.9j, -0.2 - 2.0j,
                          1.6 + 0.5j, -1.7 + 0.4j, 0.5 + 1.6j, 0.4 - 1.7j],
                         0.8 * np.sqrt(rng.uniform(0, 1, n - 12)) * np.exp(2j * np.pi * rng.uniform(0, 1, n - 12))])
    U, _ = np.linalg.qr(rng.standard_normal((n, n)) + 1j * rng.standard_normal((n, n)))
    A = (U * ev) @ U.conj().T
    lam, X = eigs(LinearOperator.m(torch.from_numpy(A)), neig, which, min_eps=1e-9, ncv=24)
    key = {"LM": np.abs(ev), "LR": ev.real, "SR": -ev.real, "LI": ev.imag, "SI": -ev.imag}[which]
    want = ev[np.argsort(-key)][:neig]
    assert np.abs(lam.numpy() - want).max() <= 1e-7
    _pairs_ok(A, lam, X, 1e-9)
    le, Xe = eigs(LinearOperator.m(torch.from_numpy(A)), neig, which, method="exacteig")
    assert np.abs(le.numpy() - want).max() <= 1e-10


@pytest.mark.parametrize("kind", ["banded", "csr"])
@pytest.mark.parametrize("bc", [(-0.8, 1.2), (0.7, 1.3)], ids=["complex_spectrum", "real_nonnormal"])
def test_toeplitz_closed_form(kind, bc):
    n, a, (b, c) = 64, 0.5, bc
    T = ac.toeplitz_dense(n, a, b, c)
    op = ac.toeplitz_operator(kind, n, a, b, c, torch.float64, "cpu")
    assert np.allclose(op.fullmatrix().numpy(), T)
    trace = {}
    # bc < 0: every eigenvalue has the real part a, so the modulus ranks them; bc > 0: real, non-normal
    lam, X = eigs(op, 4, "LM" if b * c < 0 else "LR", min_eps=1e-8, ncv=32, trace=trace)
    assert trace["converged"] and trace["niter"] <= 25
    r = _pairs_ok(T.astype(np.complex128), lam, X, 1e-8)
    ev = ac.toeplitz_eigs(n, a, b, c)
    cond = ac.toeplitz_cond(n, b, c)
    for i in range(4):
        assert np.abs(ev - lam[i].item()).min() <= cond * r[i] + 16 * n * 2.2e-16 * cond * np.abs(T).sum(1).max()
    if b * c < 0:
        assert lam[0].imag > 0 and abs(lam[1] - lam[0].conj()) <= 1e-6


def test_stochastic_matrix_has_the_perron_pair():
    P = ac.stochastic(150)
    lam, X = eigs(LinearOperator.m(torch.from_numpy(P)), 1, "LM", min_eps=1e-10)
    assert abs(lam[0].item() - 1.0) <= 1e-9
    x = X[:, 0].numpy()
    x = x * np.conj(x[np.argmax(np.abs(x))]) / abs(x[np.argmax(np.abs(x))])        # up to phase
    assert np.all(x.real > 0) and np.abs(x.imag).max() <= 1e-8


def test_invariant_subspace_start_recovers():
    n, nb = 100, 10
    A, ev = ac.block_diagonal(n, nb)
    V0 = torch.zeros(n, 1, dtype=torch.float64)
    V0[:nb, 0] = torch.from_numpy(np.random.default_rng(2).standard_normal(nb))
    trace = {}
    lam, X = eigs(LinearOperator.m(torch.from_numpy(A)), 4, "LM", V0=V0, min_eps=1e-8, trace=trace)
    assert trace["breakdowns"] and trace["converged"]          # the Krylov space of V0 has dimension nb < ncv
    _pairs_ok(A.astype(np.complex128), lam, X, 1e-8)
    want = ev[np.argsort(-np.abs(ev), kind="stable")][:4]
    assert max(np.abs(want - z).min() for z in lam.numpy()) <= 1e-7


@pytest.mark.parametrize("bshape", [(1,), (2, 3)])
def test_batches_equal_single_members(bshape):
    n, neig = 80, 2
    mats = [ac.normal_matrix(n, 4, False, seed=s)[0] for s in range(int(np.prod(bshape)))]
    A = torch.from_numpy(np.stack(mats)).reshape(*bshape, n, n)
    V0 = torch.from_numpy(np.random.default_rng(9).standard_normal((n, 1)))
    lam, X = eigs(LinearOperator.m(A), neig, "LM", V0=V0, min_eps=1e-9)
    assert lam.shape == (*bshape, neig) and X.shape == (*bshape, n, neig)
    for i, M in enumerate(mats):
        l1, X1 = eigs(LinearOperator.m(torch.from_numpy(M)), neig, "LM", V0=V0, min_eps=1e-9)
        idx = np.unravel_index(i, bshape)
        assert np.abs(lam[idx].numpy() - l1.numpy()).max() <= 64 * n * 2.2e-16 * 2.0
        ph = (X1.conj() * X[idx]).sum(0)
        assert np.abs((X[idx] / (ph / ph.abs()) - X1).numpy()).max() <= 1e-7


def test_members_that_keep_different_counts():
    """a real eigenvalue above the wanted pairs shifts the parity of member 1's ranking: the cut at keep = 11 separates a
    conjugate pair of members 0 and 2 (they keep 12) and none of member 1 (it keeps 11); the cycle then starts at 11 and
    the steps below 12 leave members 0 and 2 alone"""
    n, neig = 80, 3
    mats = [ac.normal_matrix(n, 4, False, seed=0)[0], ac.normal_matrix(n, 4, False, seed=1, extra_real=(2.5, 0.3))[0],
            ac.normal_matrix(n, 4, False, seed=2)[0]]
    V0 = torch.from_numpy(np.random.default_rng(9).standard_normal((n, 1)))
    trace = {}
    lam, X = eigs(LinearOperator.m(torch.from_numpy(np.stack(mats))), neig, "LM", V0=V0, min_eps=1e-9, trace=trace)
    assert trace["converged"] and trace["restarts"] >= 1 and all(k == [12, 11, 12] for k in trace["kept_history"])
    for i, M in enumerate(mats):
        _pairs_ok(M.astype(np.complex128), lam[i], X[i], 1e-9)
        t1 = {}
        l1, X1 = eigs(LinearOperator.m(torch.from_numpy(M)), neig, "LM", V0=V0, min_eps=1e-9, trace=t1)
        assert all(k == [[12, 11, 12][i]] for k in t1["kept_history"])
        la, lb = lam[i].numpy(), l1.numpy()
        assert np.all(np.abs(la - lb) <= 64 * n * 2.220446049250313e-16 * np.abs(lb))


def test_hermitian_operator_equals_symeig():
    n = 90
    rng = np.random.default_rng(4)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    ev = np.concatenate([[3.0, 2.6, 2.2], rng.uniform(-1, 1, n - 3)])
    A = torch.from_numpy((Q * ev) @ Q.T)
    A = (A + A.T) / 2
    op = LinearOperator.m(A, is_hermitian=True)
    lam, X = eigs(op, 3, "LR", min_eps=1e-10)
    se, sX = symeig(op, 3, "uppermost", method="exacteig")
    assert np.abs(lam.real.numpy() - se.flip(-1).numpy()).max() <= 1e-10 and np.abs(lam.imag.numpy()).max() <= 1e-12
    ov = (sX.flip(-1).to(torch.complex128).conj() * X).sum(0).abs()
    assert np.abs(ov.numpy() - 1).max() <= 1e-8


def test_dense_hand_over():
    A = torch.from_numpy(np.random.default_rng(6).standard_normal((16, 16)))
    trace = {}
    lam, X = eigs(LinearOperator.m(A), 3, "LM", trace=trace)
    assert trace["handed_to"] == "dense_eig" and trace["napply"] == 0
    ev = np.linalg.eigvals(A.numpy())
    assert min(abs(abs(lam[0].item()) - np.abs(ev).max()), 1) <= 1e-12
    _pairs_ok(A.numpy().astype(np.complex128), lam, X, 1e-10)
    trace = {}
    eigs(LinearOperator.m(torch.eye(17, dtype=torch.float64) + 0.01 * torch.from_numpy(
        np.random.default_rng(7).standard_normal((17, 17)))), 9, "LM", trace=trace)     # n <= 2 neig
    assert trace["handed_to"] == "dense_eig"


def test_refusals():
    A = torch.from_numpy(ac.normal_matrix(60, 4, False)[0])
    op = LinearOperator.m(A)
    for which in ("LI", "SI"):
        with pytest.raises(ValueError, match="complex operators"):
            eigs(op, 2, which)
    with pytest.raises(ValueError, match="shift-and-invert"):
        eigs(op, 2, "SM")
    with pytest.raises(ValueError, match="which must be"):
        eigs(op, 2, "XX")
    with pytest.raises(NotImplementedError):
        eigs(op, 2, M=LinearOperator.m(torch.eye(60, dtype=torch.float64), True))
    with pytest.raises(NotImplementedError):
        eigs(op, 2, process_group=object())
    with pytest.raises(ValueError, match="neig \\+ 2"):
        eigs(op, 9, ncv=10)
    with pytest.raises(ValueError, match="beyond"):
        eigs(op, 2, ncv=49)
    with pytest.raises(ValueError, match="beyond"):
        eigs(op, 22)                                              # the default ncv = 52
    with pytest.raises(ValueError, match="exceeds"):
        eigs(LinearOperator.m(A[:30, :30]), 2, ncv=31)
    with pytest.raises(ValueError):
        eigs(op, 0)
    with pytest.raises(RuntimeError, match="Unknown eigs method"):
        eigs(op, 2, method="davidson")
    with pytest.raises(TypeError, match="unknown option"):
        eigs(op, 2, nguard=3)
    with pytest.raises(RuntimeError, match="square"):
        eigs(LinearOperator.m(torch.ones(4, 5, dtype=torch.float64)), 1)
    Ag = A.clone().requires_grad_()
    with pytest.raises(NotImplementedError, match="forward-only"):
        eigs(LinearOperator.m(Ag), 2)
    with torch.no_grad():
        eigs(LinearOperator.m(Ag), 2)
    with pytest.raises(RuntimeError, match="start vector is zero"):
        eigs(op, 2, V0=torch.zeros(60, 1, dtype=torch.float64))


def test_unconverged_run_warns_once_with_the_count():
    A = torch.from_numpy(ac.toeplitz_dense(64, 0.5, 0.7, 1.3))
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        trace = {}
        lam, X = eigs(LinearOperator.m(A), 4, "LR", max_niter=2, min_eps=1e-12, trace=trace)
    mine = [x for x in w if issubclass(x.category, ConvergenceWarning)]
    assert len(mine) == 1 and "of 4 eigenpairs" in str(mine[0].message) and not trace["converged"]
    assert trace["niter"] == 2 and lam.shape == (4,)


def test_a_device_operator_never_reaches_the_host_twin():
    class FakeDevice(LinearOperator):
        def __init__(self):
            super().__init__(shape=(40, 40), dtype=torch.float64, device=torch.device("cuda:0"))

        def _mv(self, x):
            return x
    n0 = host_eig.calls["arnoldi"]
    with pytest.raises(NativeLibraryError, match="host memory only"):
        host_eig.arnoldi(FakeDevice(), 2)
    with pytest.raises(Exception):
        eigs(FakeDevice(), 2)                                     # the native driver: no device here, but never the twin
    assert host_eig.calls["arnoldi"] == n0 + 1
